"""What starting a whole batch from ONE instance's basis (UniformBatch.solve_from with a shared row of arc states) costs against the only
way there was before it: solve() of the batch from the start basis.  Two families on one generated graph each with shared supplies and
bounds, plain auto-configured Block Search, one MI355X, one process, medians of `--repeats` rounds:

  small  4 096 x 200 nodes / 600 arcs       (LDS tier)
  large    256 x 10 000 nodes / 30 000 arcs (global tier)

    timeout 1100 python tools/gpu_batch_start.py [--json profiles/batch_start.json]

Three legs per family.  "costs 5 %" and "costs 100 %": every instance has the base row of costs with that share of it redrawn.  "supplies
5 %": every instance has the base costs and 5 % of its suppliers' and demanders' amounts redrawn (redraw() of gpu_batch_redata.py).
The old way is solve() on the leg's tensors.  The new way is three calls, all of them timed: solve() of a one-instance handle on the base
row and the shared supplies, cost_ranges(costs=False) on it, and solve_from() of the batch with the one row that gives.  The one-instance
solve is the same for the three legs of a round, so it runs once per round and its time is added to each leg's.
Recorded: both times, the start launch, the rounds, the classes, the pivots against the fresh solve's, and the start launch's time per
node (the one-lane walk is most of it in the global tier; it includes the lane-parallel rest and the copy of the slots).  Nothing here
promises a speed-up: the figures say where a shared basis wins and where it loses.  Both ways must agree on every status and every total
cost.  The script stops at the first failure."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch  # noqa: F401  (before the library: one HIP runtime per process, torch's)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mincostflow_amd as M  # noqa: E402
from gpu_batch_redata import FAMILIES, redraw, to_device  # noqa: E402

LEGS = (("costs", 0.05), ("costs", 1.0), ("supplies", 0.05))


def timed(call):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = call()
    return r, (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--families", default="small,large")
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    if M.device_count() < 1:
        raise SystemExit("needs an MI355X")
    out = {"rule": "BlockSearch (plain, auto-configured)", "repeats": args.repeats, "families": {}}
    for name in args.families.split(","):
        f = FAMILIES[name]
        n = f["count"]
        g = M.netgen_like(f["seed"], f["nodes"], f["arcs"], f["ends"], f["ends"])
        rng = np.random.default_rng(20261020)
        base = rng.integers(1, 10001, g.arc_count).astype(np.int64)
        supply = np.asarray(g.supply, np.int64)
        shared = dict(supply=to_device(supply), lower=to_device(np.asarray(g.lower, np.int64)), upper=to_device(np.asarray(g.upper, np.int64)))
        data = []
        for what, share in LEGS:
            if what == "costs":
                cost = np.where(rng.random((n, g.arc_count)) < share, rng.integers(1, 10001, (n, g.arc_count)), base).astype(np.int64)
                data.append(dict(shared, cost=to_device(cost)))
            else:
                data.append(dict(shared, cost=to_device(base), supply=to_device(redraw(rng, np.tile(supply, (n, 1)), share))))
        one = M.UniformBatch(g.node_count, g.source, g.target, 1, rule=M.PivotRule.BlockSearch)
        batch = M.UniformBatch(g.node_count, g.source, g.target, n, rule=M.PivotRule.BlockSearch)
        fresh = M.UniformBatch(g.node_count, g.source, g.target, n, rule=M.PivotRule.BlockSearch)
        base_t = to_device(base)
        rounds = [[] for _ in LEGS]
        basis_ms = []
        warm = 0 if out["families"] else 1               # the process's first round warms both paths up (kernels loaded, allocators primed) and is not counted
        for rep in range(1 - warm, args.repeats + 1):
            (_, solve_one_ms) = timed(lambda: one.solve(base_t, **shared))
            one_pivots = one.stats()["total_pivots"]
            (ranges, ranges_ms) = timed(lambda: one.cost_ranges(tensors=True, costs=False))
            assert int(ranges.ranged[0]) == 1, "the representative instance left no basis to export"
            row = ranges.arc_state[0]
            if rep:
                basis_ms.append(solve_one_ms + ranges_ms)
            for k, a in enumerate(data):
                (r, from_ms) = timed(lambda: batch.solve_from(row, **a))
                ss = batch.start_stats()
                (c, solve_ms) = timed(lambda: fresh.solve(**a))
                cs = fresh.stats()
                assert bool((r.status == c.status).all()) and bool((r.total_cost == c.total_cost).all()), "the start from a basis and the fresh solve disagree"
                if not rep:
                    continue
                rounds[k].append(dict(new_ms=solve_one_ms + ranges_ms + from_ms, solve_one_ms=solve_one_ms, cost_ranges_ms=ranges_ms, solve_from_ms=from_ms,
                                      solve_ms=solve_ms, start_launch_ms=ss["begin_ns"] / 1e6, rounds_ms=ss["kernel_ns"] / 1e6, finish_ms=ss["finish_ns"] / 1e6,
                                      solve_rounds_ms=cs["kernel_ns"] / 1e6, primal_starts=ss["primal_starts"], dual_starts=ss["dual_starts"],
                                      cold_by_rule=ss["cold_instances"], fallback=ss["fallback_instances"], dual_pivots=ss["dual_pivots"],
                                      primal_pivots=ss["primal_pivots"], one_instance_pivots=one_pivots, solve_pivots=cs["total_pivots"], launches=ss["launches"],
                                      solve_launches=cs["launches"], optimal=int((c.status == M.SolverStatus.Optimal).sum()), bytes_up=ss["bytes_up"],
                                      bytes_down=ss["bytes_down"]))
            print(f"{name} round {rep} done", flush=True)
        legs = []
        for (what, share), seen in zip(LEGS, rounds):
            leg = {key: statistics.median(s[key] for s in seen) for key in seen[0]}
            leg.update(change=what, share=share, speedup=leg["solve_ms"] / leg["new_ms"], speedup_without_the_one_instance_solve=leg["solve_ms"] / leg["solve_from_ms"],
                       start_launch_ns_per_node=leg["start_launch_ms"] * 1e6 / f["nodes"])
            legs.append(leg)
            print(f"{name} {what} {share:4.0%}: new way {leg['new_ms']:9.2f} ms (one instance {leg['solve_one_ms']:.2f}, ranges {leg['cost_ranges_ms']:.2f}, solve_from "
                  f"{leg['solve_from_ms']:.2f}: start launch {leg['start_launch_ms']:.2f} = {leg['start_launch_ns_per_node']:.0f} ns per node, rounds {leg['rounds_ms']:.2f}) "
                  f"against solve {leg['solve_ms']:9.2f} ms: x{leg['speedup']:.2f};  primal {leg['primal_starts']:.0f}, dual {leg['dual_starts']:.0f}, cold "
                  f"{leg['cold_by_rule']:.0f}, fallback {leg['fallback']:.0f};  pivots {leg['dual_pivots']:.0f} dual + {leg['primal_pivots']:.0f} primal against "
                  f"{leg['solve_pivots']:.0f}", flush=True)
        out["families"][name] = dict(nodes=f["nodes"], arcs=f["arcs"], instances=n, lds_instances=fresh.stats()["lds_instances"],
                                     one_instance_basis_ms=statistics.median(basis_ms), legs=legs)
        del one, batch, fresh
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
