"""What rays() costs (UniformBatch.rays: one wave per instance runs a level-synchronous Bellman-Ford over the uncapacitated arcs and answers
with a negative cycle or with labels, device tensors out) beside solve(), validate() and diagnose() on the same handle.  One MI355X, one
process, plain auto-configured Block Search, the two workloads of tools/gpu_batch_diagnose.py with a triangle and a ring through a quarter
of the nodes appended to the graph (uncapacitated in every case; of cost 1 per arc unless a case plants a negative cycle on them):

  small  4 096 x 200 nodes / 600 + 53 arcs          the LDS tier
  large    256 x 10 000 nodes / 30 000 + 2 503 arcs the global tier: labels, marks and frontiers in the handle's buffer, a node sweep of 157 strides per round

    python tools/gpu_batch_rays.py [--json profiles/batch_rays.json] [--workloads small,large]

Four cases per workload, every one a solve() of its own on the same handle:
  one_round    upper=None, costs 0 .. 19: every arc uncapacitated, nothing falls, one round per instance
  mixed        the generator's capacities with one arc in ten uncapacitated, costs -6 .. 19, nothing planted: several rounds
  short_cycle  mixed, and in every third instance the triangle costs -1 per arc
  long_cycle   mixed, and in every third instance the ring costs -1 per arc
The cost row is ONE for all instances of a workload but for the planted arcs, so that every bounded instance makes the rounds the mixed
case shows and every planted one the same number as its neighbours: rounds of a planted instance = (all rounds - bounded instances x
rounds of a bounded one) / planted instances, and the kernel lasts as long as those, which run side by side -- kernel time over that
number is what a round costs.  (Should the drawn costs hold a negative cycle of their own, the row is drawn again.)  Per case validate(),
diagnose() and rays() run REPEATS times each: wall time and the library's kernel_ns.  The small workload's rows are compared with the
host hook's on the same state, bit for bit.  Every GPU step runs under a time limit of its own (a watchdog thread ends the process when
one passes it), and the script stops at the first failure.  --hooks: a rehearsal without a GPU, every call through the one-lane host
hooks (the times then say nothing)."""
import argparse
import contextlib
import faulthandler
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

REPEATS = 5
WORKLOADS = {
    "small": dict(nodes=200, arcs=600, ends=4, count=4096, seed=1, solve_limit=120, rays_limit=60),
    "large": dict(nodes=10_000, arcs=30_000, ends=100, count=256, seed=100_001, solve_limit=300, rays_limit=120),
}
CASES = ("one_round", "mixed", "short_cycle", "long_cycle")


@contextlib.contextmanager
def limit(seconds, what):
    """A GPU step under its own time limit: past it the process is ended, whatever the main thread is waiting in."""
    print(f"[{what}: at most {seconds} s]", flush=True)
    faulthandler.dump_traceback_later(seconds, exit=True)
    try:
        yield
    finally:
        faulthandler.cancel_dump_traceback_later()


def spread(values_s):
    ms = [v * 1e3 for v in values_s]
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), all_ms=ms)


def timed(name, what, seconds, call, kernel_ns):
    """REPEATS calls after one warm-up: (last result, wall times, kernel times)"""
    with limit(seconds, f"{name}: {what}, warm-up"):
        call()
    wall_s, kernel_s = [], []
    for _ in range(REPEATS):
        with limit(seconds, f"{name}: {what}"):
            t0 = time.perf_counter()
            g = call()
            wall_s.append(time.perf_counter() - t0)
            kernel_s.append(kernel_ns(g) / 1e9)
    return g, wall_s, kernel_s


def graph_of(g, M):
    """The generator's graph with the triangle (nodes 0, 1, 2) and the ring (a quarter of the nodes, every fourth, in a shuffled order) appended"""
    n, m = g.node_count, g.arc_count
    ring = np.random.default_rng(20261102).permutation(np.arange(3, n, 4)[:n // 4])
    tails = np.concatenate([[0, 1, 2], ring]).astype(np.int32)
    heads = np.concatenate([[1, 2, 0], np.roll(ring, -1)]).astype(np.int32)
    src, tgt = np.concatenate([g.source, tails]).astype(np.int32), np.concatenate([g.target, heads]).astype(np.int32)
    extra = len(tails)
    lower = np.concatenate([g.lower, np.zeros(extra, np.int64)])
    upper = np.concatenate([g.upper, np.full(extra, M.INF_CAP, np.int64)])
    return n, src, tgt, lower, upper, slice(m, m + 3), slice(m + 3, m + extra)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--workloads", default="small,large")
    ap.add_argument("--count", type=int, default=0, help="instances per workload (a rehearsal; the default is the workload's own)")
    ap.add_argument("--hooks", action="store_true", help="a rehearsal without a GPU: the one-lane host hooks")
    args = ap.parse_args()
    if not args.hooks:
        import torch  # noqa: F401  (before the library: one HIP runtime per process, torch's)
    import mincostflow_amd as M
    if not args.hooks and M.device_count() < 1:
        raise SystemExit("needs an MI355X")
    to_device = (lambda a: np.ascontiguousarray(a)) if args.hooks else (lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda())
    home = (lambda a: a) if args.hooks else (lambda a: a.cpu().numpy())
    out = {"rule": "BlockSearch (plain, auto-configured)", "repeats": REPEATS, "supply_type": "GEQ", "workloads": {}}
    for name in args.workloads.split(","):
        w = dict(WORKLOADS[name])
        if args.count:
            w["count"] = args.count
        count = w["count"]
        g = M.netgen_like(w["seed"], w["nodes"], w["arcs"], w["ends"], w["ends"])
        n, src, tgt, lower, upper, triangle, ring = graph_of(g, M)
        m = len(src)
        planted = np.arange(count) % 3 == 1
        supply = to_device(np.tile(g.supply, (count, 1)).astype(np.int64))
        u = M.UniformBatch(n, src, tgt, count, rule=M.PivotRule.BlockSearch)
        solve = (lambda **a: u.run_on_host(**a)) if args.hooks else (lambda **a: u.solve(**a))
        rays = (lambda **a: u.rays_on_host(**a)) if args.hooks else (lambda **a: u.rays(**a))
        diagnose = (lambda: u.diagnose_on_host()) if args.hooks else (lambda: u.diagnose())
        res = dict(nodes=n, arcs=m, instances=count, triangle_arcs=3, ring_arcs=ring.stop - ring.start, cases={})
        bounded_rounds = None
        for case in CASES:
            what = f"{name} {case}"
            for draw in range(10):
                rng = np.random.default_rng([20261103, draw])
                row = rng.integers(0 if case == "one_round" else -6, 20, m).astype(np.int64)
                row[triangle], row[ring] = 1, 1
                cost = np.tile(row, (count, 1))
                if case == "short_cycle":
                    cost[planted, triangle] = -1
                if case == "long_cycle":
                    cost[planted, ring] = -1
                caps = upper.copy()
                caps[:g.arc_count][np.random.default_rng([20261104, draw]).random(g.arc_count) < 0.1] = M.INF_CAP
                at = dict(cost=to_device(cost), supply=supply)
                if case != "one_round":
                    at.update(lower=to_device(lower), upper=to_device(caps))
                with limit(w["solve_limit"], f"{what}: solve"):
                    t0 = time.perf_counter()
                    r = solve(**at)
                    status = home(r.status)
                    solve_s = time.perf_counter() - t0
                    solve_stats = u.stats()
                with limit(w["rays_limit"], f"{what}: first rays"):
                    rays()
                first = u.ray_stats()
                if first["cycle"] == (int(planted.sum()) if case.endswith("_cycle") else 0):
                    break
                print(f"{what}: the drawn costs hold a negative cycle of their own ({first['cycle']} instances), drawing again", flush=True)
            else:
                raise SystemExit(f"{what}: no cost row without a negative cycle of its own in 10 draws")
            _, v_wall, v_kernel = timed(what, "validate", 60, lambda: u.validate(r, **at), lambda v: v.summary["kernel_ns"]) if not args.hooks else (None, [0.0], [0.0])
            _, g_wall, g_kernel = timed(what, "diagnose", 60, diagnose, lambda _: u.diagnose_stats()["kernel_ns"])
            d, d_wall, d_kernel = timed(what, "rays", w["rays_limit"], rays, lambda _: u.ray_stats()["kernel_ns"])
            st = u.ray_stats()
            _, b_wall, b_kernel = timed(what, "rays without rows", w["rays_limit"], lambda: rays(arcs=False, labels=False), lambda _: u.ray_stats()["kernel_ns"])
            with limit(120, f"{what}: rows home"):
                verdict, cycle_cost, cycle_length, on_cycle, label = (home(a) for a in (d.verdict, d.cycle_cost, d.cycle_length, d.on_cycle, d.label))
            cyclic = verdict == M.Ray.Cycle
            assert np.array_equal(cyclic, planted if case.endswith("_cycle") else np.zeros(count, bool)) and np.all(verdict[~cyclic] == M.Ray.Bounded)
            assert np.array_equal(on_cycle.sum(axis=1), cycle_length) and np.array_equal((on_cycle * cost).sum(axis=1), cycle_cost) and np.all(cycle_cost[cyclic] < 0)
            open_arcs = (np.ones(m, bool) if case == "one_round" else caps == M.INF_CAP)
            slack = label[:, src[open_arcs]] + cost[:, open_arcs] - label[:, tgt[open_arcs]]
            assert np.all(slack[~cyclic] >= 0) and not label[cyclic].any()
            if case == "short_cycle":                                         # the ring's cycle may be answered by a shorter one through other arcs
                assert np.all(on_cycle[cyclic][:, triangle] == 1) and np.all(cycle_length[cyclic] == 3)
            if name == "small" and not args.hooks:
                with limit(240, f"{what}: the host hook on the same state"):
                    hook = u.rays_on_host()
                for a, b in ((hook.verdict, verdict), (hook.cycle_cost, cycle_cost), (hook.cycle_length, cycle_length), (hook.on_cycle, on_cycle), (hook.label, label)):
                    assert np.array_equal(a, b), f"{what}: the device and the host hook disagree"
                hs = u.ray_stats()
                assert all(hs[k] == st[k] for k in ("rounds", "frontier_nodes", "inc_entries", "cycle_arcs", "cycle", "bounded"))
            if not case.endswith("_cycle"):
                assert st["rounds"] % count == 0                             # one cost row: every instance makes the same rounds
                bounded_rounds = st["rounds"] // count
            cycles = int(cyclic.sum())
            longest = (st["rounds"] - (count - cycles) * bounded_rounds) // cycles if cycles else bounded_rounds
            f = dict(tier="lds" if st["lds_instances"] > 0 else "global", uncapacitated_arcs=int(open_arcs.sum()),
                     status={name_: int((status == value).sum()) for name_, value in (("optimal", 1), ("infeasible", 2), ("unbounded", 3), ("not_solved", 0))},
                     verdicts={k: st[k] for k in ("none", "bounded", "cycle", "bounds")}, optimal_although_unbounded=int(((status == 1) & cyclic).sum()),
                     solve=dict(wall_ms=solve_s * 1e3, kernel_ms=solve_stats["kernel_ns"] / 1e6, total_pivots=solve_stats["total_pivots"]),
                     validate=dict(wall=spread(v_wall), kernel=spread(v_kernel)), diagnose=dict(wall=spread(g_wall), kernel=spread(g_kernel)),
                     rays=dict(wall=spread(d_wall), kernel=spread(d_kernel), rounds=st["rounds"], frontier_nodes=st["frontier_nodes"], inc_entries=st["inc_entries"],
                               cycle_arcs=st["cycle_arcs"], rounds_per_instance=st["rounds"] / count, rounds_of_the_longest_instance=longest,
                               bytes_up=st["bytes_up"], bytes_down=st["bytes_down"]),
                     rays_without_rows=dict(wall=spread(b_wall), kernel=spread(b_kernel)))
            f["rays"]["kernel_us_per_round_of_the_longest_instance"] = f["rays"]["kernel"]["median_ms"] * 1e3 / longest
            f["rays_share_of_solve"] = f["rays"]["wall"]["median_ms"] / f["solve"]["wall_ms"]
            res["cases"][case] = f
            print(f"{what} ({f['tier']}): {f['uncapacitated_arcs']} uncapacitated arcs, status {f['status']}, verdicts {f['verdicts']}; Optimal although unbounded "
                  f"{f['optimal_although_unbounded']}", flush=True)
            print(f"{what}: solve {f['solve']['wall_ms']:.1f} ms wall ({f['solve']['kernel_ms']:.1f} kernel, {f['solve']['total_pivots']} pivots)", flush=True)
            for key in ("validate", "diagnose", "rays", "rays_without_rows"):
                k = f[key]
                print(f"{what} {key}: {k['wall']['median_ms']:.3f} ms wall ({k['wall']['min_ms']:.3f} - {k['wall']['max_ms']:.3f}), kernel {k['kernel']['median_ms']:.3f} ms", flush=True)
            k = f["rays"]
            print(f"{what} rays: {k['rounds']} rounds ({k['rounds_per_instance']:.1f} per instance, {k['rounds_of_the_longest_instance']} in the longest), {k['frontier_nodes']} "
                  f"frontier nodes, {k['inc_entries']} incidence entries, {k['cycle_arcs']} cycle arcs; {k['kernel_us_per_round_of_the_longest_instance']:.2f} us of kernel "
                  f"time per round of the longest; up {k['bytes_up']} B, down {k['bytes_down']} B", flush=True)
        out["workloads"][name] = res
        del u
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
