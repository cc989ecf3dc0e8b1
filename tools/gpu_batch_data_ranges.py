"""What the supply and bound ranges of a kept basis cost (UniformBatch.data_ranges: one wave per instance, every lane walks the tree
path of one non-tree arc or one pair and gathers the rooms on it, device tensors out) beside cost_ranges() on the same handle and state,
which walks the same cycles and scatters by atomic minima.  One MI355X, one process, plain auto-configured Block Search, the two
workloads of tools/gpu_batch_ranges.py:

  small  4 096 x 200 nodes / 600 arcs        the LDS tier
  large    256 x 10 000 nodes / 30 000 arcs  the global tier: every hop follows par_arc into the workspace

    python tools/gpu_batch_data_ranges.py [--json profiles/batch_data_ranges.json] [--workloads small,large]

Per workload the batch is solved once, then cost_ranges(), data_ranges() and data_ranges() with PAIRS drawn pairs per instance run
REPEATS times each: wall time, the library's kernel_ns, walks and hops, and

    ns per hop per lane = kernel_ns * 64 * resident waves / hops

as gpu_batch_ranges.py defines it (resident waves by the LDS a workgroup of that kernel takes).  cost_ranges() walks the cycle of every
non-tree arc of the search range (the root links among them; it does not count its walks), data_ranges() without pairs that of every
non-tree arc of the caller's; the walk is the same, so the two figures differ by what a hop does: an atomic minimum on a tree arc's word
there, two register minima here.  The small workload's rows are compared with the host hook's on the same state, bit for bit.  Every
GPU step runs under a time limit of its own (a watchdog thread ends the process when one passes it), and the script stops at the
first failure."""
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
from mincostflow_amd import _lib as L  # noqa: E402

REPEATS = 5
PAIRS = 1000
LDS_PER_CU = 160 << 10
WORKLOADS = {
    "small": dict(nodes=200, arcs=600, ends=4, count=4096, seed=1, solve_limit=120),
    "large": dict(nodes=10_000, arcs=30_000, ends=100, count=256, seed=100_001, solve_limit=240),
}
PARENT = {"small": 1087, "large": 3754}     # ns per hop per lane of cost_ranges() in profiles/batch_ranges.json


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


def up16(x):
    return (x + 15) // 16 * 16


def range_footprint(n, m):
    """range_layout_of(m + 2n, n + 1, m).bytes of csrc/ranges_step.hip.h"""
    A, N = m + 2 * n, n + 1
    return sum(up16(b) for b in (4 * A, 4 * A, 8 * A, A, 8 * N, 4 * N, 4 * N, 4 * N, N, 8 * m, 8 * m))


def data_range_footprint(n, m):
    """data_range_layout_of(m, n + 1).bytes of csrc/data_ranges_step.hip.h"""
    N = n + 1
    return sum(up16(b) for b in (4 * m, 4 * m, m, 4 * N, 4 * N, 8 * N, 8 * N))


def spread(values_s):
    ms = [v * 1e3 for v in values_s]
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), all_ms=ms)


def timed(name, what, call, stats):
    """REPEATS calls after one warm-up: (last result, wall times, kernel times, the last call's statistics)"""
    with limit(60, f"{name}: {what}, warm-up"):
        call()
    wall_s, kernel_s = [], []
    for _ in range(REPEATS):
        with limit(60, f"{name}: {what}"):
            t0 = time.perf_counter()
            g = call()
            wall_s.append(time.perf_counter() - t0)
            st = stats()
            kernel_s.append(st["kernel_ns"] / 1e9)
    return g, wall_s, kernel_s, st


def figures(wall_s, kernel_s, st, hops, walks, footprint, count, cus):
    in_lds = st["lds_instances"] > 0
    per_cu = min(32, LDS_PER_CU // footprint) if in_lds else 32
    resident = min(count, cus * per_cu)
    kernel = statistics.median(kernel_s)
    return dict(wall=spread(wall_s), kernel=spread(kernel_s), walks=walks, hops=hops, lds_bytes=footprint if in_lds else 0, resident_waves=resident,
                ns_per_hop_per_lane=kernel * 1e9 * 64 * resident / max(hops, 1), ns_per_hop_of_the_batch=kernel * 1e9 / max(hops, 1),
                bytes_up=st["bytes_up"], bytes_down=st["bytes_down"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--workloads", default="small,large")
    ap.add_argument("--count", type=int, default=0, help="instances per workload (a rehearsal; the default is the workload's own)")
    args = ap.parse_args()
    if M.device_count() < 1:
        raise SystemExit("needs an MI355X")
    cus = L.lib().mcf_device_compute_units(0)
    out = {"rule": "BlockSearch (plain, auto-configured)", "repeats": REPEATS, "pairs_per_instance": PAIRS, "compute_units": cus,
           "cost_ranges_ns_per_hop_per_lane_of_batch_ranges_json": PARENT, "workloads": {}}
    for name in args.workloads.split(","):
        w = dict(WORKLOADS[name])
        if args.count:
            w["count"] = args.count
        count = w["count"]
        g = M.netgen_like(w["seed"], w["nodes"], w["arcs"], w["ends"], w["ends"])
        n, m = g.node_count, g.arc_count
        cost = np.random.default_rng(20261101).integers(1, 10001, (count, m)).astype(np.int64)
        pairs = np.ascontiguousarray(np.random.default_rng(20261102).integers(0, n, (PAIRS, 2)).astype(np.int32))
        with limit(60, f"{name}: upload"):
            at = dict(cost=to_device(cost), supply=to_device(g.supply), lower=to_device(g.lower), upper=to_device(g.upper))
            pairs_at = to_device(pairs)
            u = M.UniformBatch(n, g.source, g.target, count, rule=M.PivotRule.BlockSearch)
            torch.cuda.synchronize()
        with limit(w["solve_limit"], f"{name}: solve"):
            r = u.solve(**at)
            assert bool((r.status == M.SolverStatus.Optimal).all())
        gc, c_wall, c_kernel, c_st = timed(name, "cost ranges", lambda: u.cost_ranges(), u.range_stats)
        gd, d_wall, d_kernel, d_st = timed(name, "data ranges", lambda: u.data_ranges(), u.data_range_stats)
        gp, p_wall, p_kernel, p_st = timed(name, f"data ranges with {PAIRS} pairs", lambda: u.data_ranges(pairs=pairs_at), u.data_range_stats)
        with limit(120, f"{name}: rows home"):
            ranged, state, down, up = (a.cpu().numpy() for a in (gp.ranged, gp.arc_state, gp.flow_down, gp.flow_up))
            forth, back = gp.ship_forth.cpu().numpy(), gp.ship_back.cpu().numpy()
            assert np.array_equal(gd.flow_down.cpu().numpy(), down) and np.array_equal(gd.flow_up.cpu().numpy(), up), "two calls, two answers"
            assert np.array_equal(gc.arc_state.cpu().numpy(), state) and np.array_equal(gc.ranged.cpu().numpy(), ranged)
        off_tree = int(((state != 0) & (ranged[:, None] == 1)).sum())
        assert np.all(down >= 0) and np.all(up >= 0) and np.all(forth >= 0) and np.all(back >= 0)
        assert d_st["ranged"] == int(ranged.sum()) and d_st["walks"] == off_tree and p_st["walks"] == off_tree + PAIRS * int(ranged.sum())
        if name == "small":
            with limit(240, f"{name}: the host hook on the same state"):
                hook = u.data_ranges_on_host(pairs=pairs)
            for a, b in ((hook.ranged, ranged), (hook.arc_state, state), (hook.flow_down, down), (hook.flow_up, up), (hook.ship_forth, forth), (hook.ship_back, back)):
                assert np.array_equal(a, b), f"{name}: the device and the host hook disagree"
            assert u.data_range_stats()["hops"] == p_st["hops"]
        res = dict(nodes=n, arcs=m, instances=count, tier="lds" if d_st["lds_instances"] > 0 else "global", ranged=d_st["ranged"], non_tree_arcs=off_tree,
                   hops_per_non_tree_arc=d_st["hops"] / max(1, off_tree),
                   cost_ranges=figures(c_wall, c_kernel, c_st, c_st["cycle_hops"], None, range_footprint(n, m), count, cus),
                   data_ranges=figures(d_wall, d_kernel, d_st, d_st["hops"], d_st["walks"], data_range_footprint(n, m), count, cus),
                   data_ranges_with_pairs=figures(p_wall, p_kernel, p_st, p_st["hops"], p_st["walks"], data_range_footprint(n, m), count, cus))
        out["workloads"][name] = res
        for key in ("cost_ranges", "data_ranges", "data_ranges_with_pairs"):
            f = res[key]
            print(f"{name} ({res['tier']}) {key}: {f['wall']['median_ms']:.3f} ms wall ({f['wall']['min_ms']:.3f} - {f['wall']['max_ms']:.3f}), kernel {f['kernel']['median_ms']:.3f} ms; "
                  f"{f['walks']} walks, {f['hops']} hops, {f['ns_per_hop_per_lane']:.0f} ns per hop per lane over {f['resident_waves']} resident waves "
                  f"({f['ns_per_hop_of_the_batch']:.3f} ns per hop of the batch); LDS {f['lds_bytes']} B; up {f['bytes_up']} B, down {f['bytes_down']} B", flush=True)
        del u, at, r, gc, gd, gp
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
