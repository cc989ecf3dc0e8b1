"""What a re-solve with new arc costs (mcf_batch_set_costs + mcf_batch_resolve) costs against the only way there was before it: a fresh
batch with mcf_batch_add + mcf_batch_solve on the new costs.  Two families of generated instances, plain auto-configured Block Search:

  small  4 096 x 200 nodes / 600 arcs       (every workspace fits LDS)
  large    256 x 10 000 nodes / 30 000 arcs (the pivots run in place in global memory)

    timeout 1100 python tools/gpu_batch_resolve.py [--json profiles/batch_resolve.json]

Per family the batch is solved once; then 5 % of every instance's costs are redrawn (uniform in the generator's range) and the batch is
re-solved, then 100 %.  Each time the same new costs also go through a fresh batch in the same process, add() included.  Recorded: both
wall times (host clock; both calls end in a synchronising copy), pivots warm against cold, bytes moved, the kernel_ns / host_ns split.
Every instance must end Optimal with the fresh batch's total cost.  The script stops at the first failure."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import mincostflow_amd as M  # noqa: E402

FAMILIES = {
    "small": dict(nodes=200, arcs=600, ends=4, count=4096, seed0=1),
    "large": dict(nodes=10_000, arcs=30_000, ends=100, count=256, seed0=100_001),
}
SHARES = (0.05, 1.0)


def fresh(problems, costs):
    """add + solve of a new batch on the new costs: (seconds with add, seconds of solve alone, stats, total costs, pivots)"""
    t0 = time.perf_counter()
    b = M.BatchSolver(rule=M.PivotRule.BlockSearch)
    for g, c in zip(problems, costs):
        b.add(M.Problem(g.node_count, g.arc_count, g.source, g.target, g.lower, g.upper, c, g.supply))
    t1 = time.perf_counter()
    b.solve()
    t2 = time.perf_counter()
    n = len(problems)
    assert all(b.status(i) == M.SolverStatus.Optimal for i in range(n))
    return t2 - t0, t2 - t1, b.stats(), [b.total_cost(i) for i in range(n)], b.stats()["total_pivots"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--families", default="small,large")
    args = ap.parse_args()
    if M.device_count() < 1:
        raise SystemExit("needs an MI355X")
    out = {"rule": "BlockSearch (plain, auto-configured)", "families": {}}
    for name in args.families.split(","):
        f = FAMILIES[name]
        problems = [M.netgen_like(f["seed0"] + k, f["nodes"], f["arcs"], f["ends"], f["ends"]) for k in range(f["count"])]
        n = len(problems)
        fresh(problems[:8], [g.cost for g in problems[:8]])                 # warm-up of the shape: kernels loaded, allocator primed
        b = M.BatchSolver(rule=M.PivotRule.BlockSearch)
        for g in problems:
            b.add(g)
        t0 = time.perf_counter()
        b.solve()
        first_s = time.perf_counter() - t0
        first = b.stats()
        assert all(b.status(i) == M.SolverStatus.Optimal for i in range(n))
        rng = np.random.default_rng(20261018)
        legs = []
        for share in SHARES:
            costs = []
            for g in problems:
                c = np.array(g.cost, np.int64)
                hit = rng.random(c.size) < share
                c[hit] = rng.integers(1, 10001, int(hit.sum()))
                costs.append(c)
            t0 = time.perf_counter()
            for i, c in enumerate(costs):
                b.set_costs(i, c)
            t1 = time.perf_counter()
            b.resolve()
            t2 = time.perf_counter()
            st = b.resolve_stats()
            assert st["warm_instances"] == n and all(b.status(i) == M.SolverStatus.Optimal for i in range(n))
            fresh_s, fresh_solve_s, fst, totals, fresh_pivots = fresh(problems, costs)
            assert [b.total_cost(i) for i in range(n)] == totals, "a warm re-solve and a fresh batch disagree on an optimum"
            r = dict(share=share, resolve_s=t2 - t1, set_costs_s=t1 - t0, fresh_add_and_solve_s=fresh_s, fresh_solve_s=fresh_solve_s,
                     speedup_vs_fresh=fresh_s / (t2 - t0), pivots_warm=st["total_pivots"], pivots_cold=fresh_pivots, launches=st["launches"],
                     bytes_uploaded=st["bytes_uploaded"], bytes_downloaded=st["bytes_downloaded"], workspace_bytes=first["workspace_bytes"],
                     kernel_s=st["kernel_ns"] / 1e9, host_s=st["host_ns"] / 1e9, fresh_kernel_s=fst["kernel_ns"] / 1e9, fresh_host_s=fst["host_ns"] / 1e9)
            legs.append(r)
            print(f"{name} {share:4.0%} redrawn: set_costs {r['set_costs_s'] * 1e3:8.2f} ms + resolve {r['resolve_s'] * 1e3:9.2f} ms (launches {r['kernel_s'] * 1e3:9.2f}, "
                  f"host {r['host_s'] * 1e3:8.2f}) against add + solve {fresh_s * 1e3:9.2f} ms (solve {fresh_solve_s * 1e3:9.2f}): x{r['speedup_vs_fresh']:.2f};  "
                  f"pivots {r['pivots_warm']} warm / {r['pivots_cold']} cold;  up {r['bytes_uploaded']} B, down {r['bytes_downloaded']} B of a {r['workspace_bytes']} B slab", flush=True)
        out["families"][name] = dict(nodes=f["nodes"], arcs=f["arcs"], instances=n, first_solve_s=first_s, first_pivots=first["total_pivots"], resolves=legs)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
