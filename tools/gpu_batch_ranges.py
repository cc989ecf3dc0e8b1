"""What the cost ranges of a kept basis cost (UniformBatch.cost_ranges: one wave per instance walks the cycle of every non-tree arc,
device tensors out) beside the solve that left the basis.  One MI355X, one process, plain auto-configured Block Search, one topology
per workload with costs per instance:

  small  4 096 x 200 nodes / 600 arcs        the LDS tier
  large    256 x 10 000 nodes / 30 000 arcs  the global tier: the walks run on the workspace, the minima meet in the caller's rows

    python tools/gpu_batch_ranges.py [--json profiles/batch_ranges.json] [--workloads small,large]

Per workload the batch is solved (timed: small REPEATS times, large once), then cost_ranges() runs REPEATS times: wall time and the
library's kernel_ns, the hops of all walks, and

    ns per hop per lane = kernel_ns * 64 * resident waves / hops

-- what one link of one lane's chain of dependent loads costs if every resident wave keeps its 64 lanes walking for the whole kernel
(they do not: arcs and cycles differ in length, so this is an upper bound on the latency of a link and the honest cost per link).
Resident waves = min(instances, CUs * waves per CU), the latter by the LDS a workgroup takes (at most 32).  DESIGN.md section 8 measured
270 - 340 ns per dependent load in global memory; the figure here stands beside it.
The small workload's rows are compared with the host hook's on the same state, bit for bit.  Every GPU step runs under a time limit of
its own (a watchdog thread ends the process when one passes it), and the script stops at the first failure."""
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
LDS_PER_CU = 160 << 10
WORKLOADS = {
    "small": dict(nodes=200, arcs=600, ends=4, count=4096, seed=1, solves=REPEATS, solve_limit=120),
    "large": dict(nodes=10_000, arcs=30_000, ends=100, count=256, seed=100_001, solves=1, solve_limit=240),
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


def up16(x):
    return (x + 15) // 16 * 16


def range_footprint(n, m):
    """range_layout_of(m + 2n, n + 1, m).bytes of csrc/ranges_step.hip.h"""
    A, N = m + 2 * n, n + 1
    return sum(up16(b) for b in (4 * A, 4 * A, 8 * A, A, 8 * N, 4 * N, 4 * N, 4 * N, N, 8 * m, 8 * m))


def spread(values_s):
    ms = [v * 1e3 for v in values_s]
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), all_ms=ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--workloads", default="small,large")
    ap.add_argument("--count", type=int, default=0, help="instances per workload (a rehearsal; the default is the workload's own)")
    args = ap.parse_args()
    if M.device_count() < 1:
        raise SystemExit("needs an MI355X")
    cus = L.lib().mcf_device_compute_units(0)
    out = {"rule": "BlockSearch (plain, auto-configured)", "repeats": REPEATS, "compute_units": cus, "dependent_load_ns_of_section_8": [270, 340], "workloads": {}}
    for name in args.workloads.split(","):
        w = dict(WORKLOADS[name])
        if args.count:
            w["count"] = args.count
        count = w["count"]
        g = M.netgen_like(w["seed"], w["nodes"], w["arcs"], w["ends"], w["ends"])
        n, m = g.node_count, g.arc_count
        cost = np.random.default_rng(20261101).integers(1, 10001, (count, m)).astype(np.int64)
        with limit(60, f"{name}: upload"):
            at = dict(cost=to_device(cost), supply=to_device(g.supply), lower=to_device(g.lower), upper=to_device(g.upper))
            u = M.UniformBatch(n, g.source, g.target, count, rule=M.PivotRule.BlockSearch)
            torch.cuda.synchronize()
        solve_s = []
        for _ in range(w["solves"] + (w["solves"] > 1)):                   # one warm-up where the solve is short
            with limit(w["solve_limit"], f"{name}: solve"):
                t0 = time.perf_counter()
                r = u.solve(**at)
                solve_s.append(time.perf_counter() - t0)
        solve_s = solve_s[w["solves"] > 1:]
        solve_stats = u.stats()
        with limit(60, f"{name}: cost ranges, warm-up"):
            assert bool((r.status == M.SolverStatus.Optimal).all())
            g0 = u.cost_ranges()                                            # the kernel's code is loaded, the table of instances is up
        wall_s, kernel_s = [], []
        for _ in range(REPEATS):
            with limit(60, f"{name}: cost ranges"):
                t0 = time.perf_counter()
                gr = u.cost_ranges()
                wall_s.append(time.perf_counter() - t0)
                st = u.range_stats()
                kernel_s.append(st["kernel_ns"] / 1e9)
        with limit(120, f"{name}: rows home"):
            ranged, state, down, up = (a.cpu().numpy() for a in (gr.ranged, gr.arc_state, gr.cost_down, gr.cost_up))
            assert all(np.array_equal(a.cpu().numpy(), b) for a, b in ((g0.ranged, ranged), (g0.cost_down, down), (g0.cost_up, up))), "two calls, two answers"
        tree = state == 0
        assert np.all(down >= 0) and np.all(up >= 0) and np.all(up[state == 1] == M.RANGE_INF) and np.all(down[state == -1] == M.RANGE_INF)
        assert st["ranged"] == int(ranged.sum()) and st["tree_arcs"] == int(tree[ranged == 1].sum())
        if name == "small":
            with limit(240, f"{name}: the host hook on the same state"):
                hook = u.cost_ranges_on_host()
            for a, b in ((hook.ranged, ranged), (hook.arc_state, state), (hook.cost_down, down), (hook.cost_up, up)):
                assert np.array_equal(a, b), f"{name}: the device and the host hook disagree"
            assert u.range_stats()["cycle_hops"] == st["cycle_hops"]
        in_lds = st["lds_instances"] > 0
        footprint = range_footprint(n, m) if in_lds else 0
        per_cu = min(32, LDS_PER_CU // footprint) if in_lds else 32
        resident = min(count, cus * per_cu)
        kernel = statistics.median(kernel_s)
        hops = st["cycle_hops"]
        finite = tree & (ranged[:, None] == 1)
        res = dict(nodes=n, arcs=m, instances=count, tier="lds" if in_lds else "global", lds_instances=st["lds_instances"], global_instances=st["global_instances"],
                   ranged=st["ranged"], tree_arcs=st["tree_arcs"], tree_arcs_finite_on_both_sides=int((finite & (down != M.RANGE_INF) & (up != M.RANGE_INF)).sum()),
                   cycle_hops=hops, hops_per_non_tree_arc=hops / max(1, int(((state != 0) & (ranged[:, None] == 1)).sum())),
                   solve=spread(solve_s), solve_kernel_ms=solve_stats["kernel_ns"] / 1e6, solve_pivots=solve_stats["total_pivots"],
                   ranges_wall=spread(wall_s), ranges_kernel=spread(kernel_s), ranges_lds_bytes=footprint, resident_waves=resident,
                   ns_per_hop_per_lane=kernel * 1e9 * 64 * resident / max(hops, 1), ns_per_hop_of_the_batch=kernel * 1e9 / max(hops, 1),
                   ranges_share_of_solve=statistics.median(wall_s) / statistics.median(solve_s), bytes_up=st["bytes_up"], bytes_down=st["bytes_down"])
        out["workloads"][name] = res
        print(f"{name} ({res['tier']}): solve {res['solve']['median_ms']:.2f} ms ({res['solve_pivots']} pivots); cost_ranges {res['ranges_wall']['median_ms']:.3f} ms wall "
              f"({res['ranges_wall']['min_ms']:.3f} - {res['ranges_wall']['max_ms']:.3f}), kernel {res['ranges_kernel']['median_ms']:.3f} ms = {res['ranges_share_of_solve']:.4f} of the solve; "
              f"{hops} hops ({res['hops_per_non_tree_arc']:.1f} per non-tree arc), {res['ns_per_hop_per_lane']:.0f} ns per hop per lane over {resident} resident waves "
              f"({res['ns_per_hop_of_the_batch']:.3f} ns per hop of the batch); ranged {res['ranged']} of {count}, {res['tree_arcs']} tree arcs "
              f"({res['tree_arcs_finite_on_both_sides']} finite on both sides); up {res['bytes_up']} B, down {res['bytes_down']} B", flush=True)
        del u, at, r, gr, g0
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
