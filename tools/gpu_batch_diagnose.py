"""What diagnose() costs (UniformBatch.diagnose: one wave per instance reads the unmet supply off the kept flow and walks the residual
graph from the violated nodes level by level, device tensors out) beside solve(), validate() and data_ranges() on the same handle.  One
MI355X, one process, plain auto-configured Block Search, the two workloads of tools/gpu_batch_data_ranges.py:

  small  4 096 x 200 nodes / 600 arcs        the LDS tier
  large    256 x 10 000 nodes / 30 000 arcs  the global tier: marks and frontiers in the handle's buffer, a node sweep of 157 strides per level

    python tools/gpu_batch_diagnose.py [--json profiles/batch_diagnose.json] [--workloads small,large]

Supplies per instance, so that roughly a third of the instances are infeasible (MCF_SUPPLY_GEQ): instance i keeps the generator's
balanced supplies unless i % 3 == 1; of those every other one gets 3 units too many on its largest source (nobody takes them: S is
everything that source reaches, the widest walk there is) and the others get every supply and demand times 1 000 (some capacity is
the bottleneck: S is what lies in front of it).  The verdict counts in the output say what came of it.  Per workload the batch is solved
once, then validate(), data_ranges() and diagnose() run REPEATS times each: wall time and the library's kernel_ns; for diagnose() the
levels, frontier nodes and incidence entries too.  The small workload's rows are compared with the host hook's on the same state, bit
for bit.  Every GPU step runs under a time limit of its own (a watchdog thread ends the process when one passes it), and the script
stops at the first failure."""
import argparse
import contextlib
import faulthandler
import json
import os
import statistics
import sys
import time

import numpy as np
import torch  # noqa: F401  (before the library: one HIP runtime per process, torch's)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import mincostflow_amd as M  # noqa: E402

REPEATS = 5
WORKLOADS = {
    "small": dict(nodes=200, arcs=600, ends=4, count=4096, seed=1, solve_limit=120),
    "large": dict(nodes=10_000, arcs=30_000, ends=100, count=256, seed=100_001, solve_limit=300),
}


@contextlib.contextmanager
def limit(seconds, what):
    """A GPU step under its own time limit: past it the process is ended, whatever the main thread is waiting in."""
    print(f"[{what}: at most {seconds} s]", flush=True)
    faulthandler.dump_traceback_later(seconds, exit=True)
    try:
        yield
    finally:
        faulthandler.cancel_dump_traceback_later()


def to_device(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def spread(values_s):
    ms = [v * 1e3 for v in values_s]
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), all_ms=ms)


def timed(name, what, call, kernel_ns):
    """REPEATS calls after one warm-up: (last result, wall times, kernel times)"""
    with limit(60, f"{name}: {what}, warm-up"):
        call()
    wall_s, kernel_s = [], []
    for _ in range(REPEATS):
        with limit(60, f"{name}: {what}"):
            t0 = time.perf_counter()
            g = call()
            wall_s.append(time.perf_counter() - t0)
            kernel_s.append(kernel_ns(g) / 1e9)
    return g, wall_s, kernel_s


def supplies(base, count):
    out = np.tile(base, (count, 1)).astype(np.int64)
    source = int(np.argmax(base))
    for i in range(1, count, 3):
        if (i // 3) % 2 == 0:
            out[i, source] += 3
        else:
            out[i] *= 1000
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--workloads", default="small,large")
    ap.add_argument("--count", type=int, default=0, help="instances per workload (a rehearsal; the default is the workload's own)")
    args = ap.parse_args()
    if M.device_count() < 1:
        raise SystemExit("needs an MI355X")
    out = {"rule": "BlockSearch (plain, auto-configured)", "repeats": REPEATS, "supply_type": "GEQ", "workloads": {}}
    for name in args.workloads.split(","):
        w = dict(WORKLOADS[name])
        if args.count:
            w["count"] = args.count
        count = w["count"]
        g = M.netgen_like(w["seed"], w["nodes"], w["arcs"], w["ends"], w["ends"])
        n, m = g.node_count, g.arc_count
        cost = np.random.default_rng(20261101).integers(1, 10001, (count, m)).astype(np.int64)
        supply = supplies(g.supply, count)
        with limit(60, f"{name}: upload"):
            at = dict(cost=to_device(cost), supply=to_device(supply), lower=to_device(g.lower), upper=to_device(g.upper))
            u = M.UniformBatch(n, g.source, g.target, count, rule=M.PivotRule.BlockSearch)
            torch.cuda.synchronize()
        with limit(w["solve_limit"], f"{name}: solve"):
            t0 = time.perf_counter()
            r = u.solve(**at)
            solve_s = time.perf_counter() - t0
            solve_stats = u.stats()
            status = r.status.cpu().numpy()
        _, v_wall, v_kernel = timed(name, "validate", lambda: u.validate(r, **at), lambda v: v.summary["kernel_ns"])
        _, r_wall, r_kernel = timed(name, "data ranges", lambda: u.data_ranges(), lambda _: u.data_range_stats()["kernel_ns"])
        d, d_wall, d_kernel = timed(name, "diagnose", lambda: u.diagnose(), lambda _: u.diagnose_stats()["kernel_ns"])
        st = u.diagnose_stats()
        _, b_wall, b_kernel = timed(name, "diagnose without node rows", lambda: u.diagnose(nodes=False), lambda _: u.diagnose_stats()["kernel_ns"])
        with limit(120, f"{name}: rows home"):
            verdict, violation, set_size, side, unmet = (a.cpu().numpy() for a in (d.verdict, d.violation, d.set_size, d.side, d.unmet))
        cut = verdict == M.Verdict.Cut
        assert st["open"] == 0 and st["cut"] == int(cut.sum()) and np.all(violation[cut] > 0) and not violation[~cut].any()
        assert np.array_equal(side.sum(axis=1), set_size) and np.array_equal(np.abs(unmet * side).sum(axis=1)[cut], violation[cut])
        if name == "small":
            with limit(240, f"{name}: the host hook on the same state"):
                hook = u.diagnose_on_host()
            for a, b in ((hook.verdict, verdict), (hook.violation, violation), (hook.set_size, set_size), (hook.side, side), (hook.unmet, unmet)):
                assert np.array_equal(a, b), f"{name}: the device and the host hook disagree"
            hs = u.diagnose_stats()
            assert all(hs[k] == st[k] for k in ("levels", "frontier_nodes", "inc_entries", "cut", "feasible"))
        walked = max(1, st["cut"] + st["open"])
        res = dict(nodes=n, arcs=m, instances=count, tier="lds" if st["lds_instances"] > 0 else "global",
                   status={name_: int((status == value).sum()) for name_, value in (("optimal", 1), ("infeasible", 2), ("unbounded", 3), ("not_solved", 0))},
                   verdicts={k: st[k] for k in ("none", "feasible", "cut", "open", "bounds")},
                   optimal_although_infeasible=int(((status == 1) & cut).sum()), infeasible_although_feasible=int(((status == 2) & (verdict == M.Verdict.Feasible)).sum()),
                   solve=dict(wall_ms=solve_s * 1e3, kernel_ms=solve_stats["kernel_ns"] / 1e6, total_pivots=solve_stats["total_pivots"]),
                   validate=dict(wall=spread(v_wall), kernel=spread(v_kernel)), data_ranges=dict(wall=spread(r_wall), kernel=spread(r_kernel)),
                   diagnose=dict(wall=spread(d_wall), kernel=spread(d_kernel), levels=st["levels"], frontier_nodes=st["frontier_nodes"], inc_entries=st["inc_entries"],
                                 levels_per_walk=st["levels"] / walked, nodes_per_walk=st["frontier_nodes"] / walked, largest_set=int(set_size.max()),
                                 bytes_up=st["bytes_up"], bytes_down=st["bytes_down"]),
                   diagnose_without_node_rows=dict(wall=spread(b_wall), kernel=spread(b_kernel)))
        res["diagnose_share_of_solve"] = res["diagnose"]["wall"]["median_ms"] / res["solve"]["wall_ms"]
        out["workloads"][name] = res
        print(f"{name} ({res['tier']}): status {res['status']}, verdicts {res['verdicts']}; Optimal although infeasible {res['optimal_although_infeasible']}, "
              f"Infeasible although feasible {res['infeasible_although_feasible']}", flush=True)
        print(f"{name}: solve {res['solve']['wall_ms']:.1f} ms wall ({res['solve']['kernel_ms']:.1f} kernel, {res['solve']['total_pivots']} pivots)", flush=True)
        for key in ("validate", "data_ranges", "diagnose", "diagnose_without_node_rows"):
            f = res[key]
            print(f"{name} {key}: {f['wall']['median_ms']:.3f} ms wall ({f['wall']['min_ms']:.3f} - {f['wall']['max_ms']:.3f}), kernel {f['kernel']['median_ms']:.3f} ms", flush=True)
        f = res["diagnose"]
        print(f"{name} diagnose: {f['levels']} levels, {f['frontier_nodes']} frontier nodes, {f['inc_entries']} incidence entries; per walk {f['levels_per_walk']:.1f} levels, "
              f"{f['nodes_per_walk']:.1f} nodes; largest S {f['largest_set']}; up {f['bytes_up']} B, down {f['bytes_down']} B", flush=True)
        del u, at, r, d
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
