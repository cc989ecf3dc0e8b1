"""What a re-solve with new supplies or bounds from the kept basis (UniformBatch.resolve_data: dual pivots, then the primal ones) costs
against the only way there was before it: solve() on the same new data.  Two families on one generated graph each, costs drawn per
instance, plain auto-configured Block Search, one MI355X, one process:

  small  4 096 x 200 nodes / 600 arcs       (LDS tier)
  large    256 x 10 000 nodes / 30 000 arcs (global tier)

    timeout 1100 python tools/gpu_batch_redata.py [--json profiles/batch_redata.json]

Per family the batch is solved once from device tensors.  Then three changes follow each other, every one applied to every instance:
5 % of the nodes that supply or demand get new amounts (the sum of the supplies and the sum of the demands kept), then all of them,
then the capacities of 5 % of the arcs are halved (rounded up).  Each time resolve_data() runs on the handle that holds the last
optimum, and solve() runs on a second handle with the same tensors; both return synchronised and are timed by the host clock round the
call.  Recorded: both times, the library's split of the re-solve, warm / cold / fallback instances, the dual pivots against the fresh
solve's pivots.  Nothing here promises a speed-up: the figures say where the dual phase wins and where it loses.  Both paths must agree
on every status and every total cost.  The script stops at the first failure."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch  # noqa: F401  (before the library: one HIP runtime per process, torch's)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import mincostflow_amd as M  # noqa: E402

FAMILIES = {
    "small": dict(nodes=200, arcs=600, ends=4, count=4096, seed=1),
    "large": dict(nodes=10_000, arcs=30_000, ends=100, count=256, seed=100_001),
}
CHANGES = (("supply", 0.05), ("supply", 1.0), ("capacity", 0.05))


def to_device(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def redraw(rng, supply, share):
    """New amounts for `share` of the suppliers and of the demanders of every row (at least two of each where there are two), each side's
    sum kept: every chosen amount is multiplied by a factor drawn from [0.5, 1.5), the amounts are scaled back to their old total and
    rounded down, and the units the rounding lost go to the first of them.  (Dealing the total out afresh among the chosen nodes was
    the first version: it made 30 % of the small family and 86 % of the large one infeasible with 5 % redrawn)"""
    out = supply.copy()
    for row in out:
        for side in (np.flatnonzero(row > 0), np.flatnonzero(row < 0)):
            if len(side) < 2:
                continue
            chosen = rng.choice(side, max(2, int(round(share * len(side)))), replace=False)
            old = np.abs(row[chosen])
            total = int(old.sum())
            drawn = old * rng.uniform(0.5, 1.5, len(chosen))
            parts = np.maximum(1, np.floor(drawn * (total - len(chosen)) / drawn.sum())).astype(np.int64)
            rest = total - int(parts.sum())
            parts += rest // len(parts)
            parts[: rest % len(parts)] += 1
            assert int(parts.sum()) == total
            row[chosen] = np.sign(row[chosen[0]]) * parts
    return out


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
        n = f["count"]
        g = M.netgen_like(f["seed"], f["nodes"], f["arcs"], f["ends"], f["ends"])
        rng = np.random.default_rng(20261020)
        cost_t = to_device(rng.integers(1, 10001, (n, g.arc_count)).astype(np.int64))
        lower_t = to_device(np.asarray(g.lower, np.int64))
        supply = np.tile(np.asarray(g.supply, np.int64), (n, 1))
        upper = np.tile(np.asarray(g.upper, np.int64), (n, 1))
        kept = M.UniformBatch(g.node_count, g.source, g.target, n, rule=M.PivotRule.BlockSearch)
        fresh = M.UniformBatch(g.node_count, g.source, g.target, n, rule=M.PivotRule.BlockSearch)
        data = lambda: dict(supply=to_device(supply), lower=lower_t, upper=to_device(upper))
        fresh.solve(cost_t, **data())                                        # warm-up of both paths: kernels loaded, allocators primed
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        first = kept.solve(cost_t, **data())
        first_s = time.perf_counter() - t0
        first_st = kept.stats()
        kept.resolve_data(cost_t, **data())                                  # warm-up of the re-data kernels: the same data, no pivot
        assert kept.resolve_data_stats()["dual_pivots"] == 0
        legs = []
        for what, share in CHANGES:
            if what == "supply":
                supply = redraw(rng, supply, share)
            else:
                hit = rng.random(upper.shape) < share
                upper = np.where(hit, np.asarray(g.lower, np.int64) + (upper - np.asarray(g.lower, np.int64) + 1) // 2, upper)
            a = data()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = kept.resolve_data(cost_t, **a)
            warm_s = time.perf_counter() - t0
            rs = kept.resolve_data_stats()
            t0 = time.perf_counter()
            c = fresh.solve(cost_t, **a)
            cold_s = time.perf_counter() - t0
            cs = fresh.stats()
            assert bool((r.status == c.status).all()) and bool((r.total_cost == c.total_cost).all()), "the re-solve and the fresh solve disagree"
            leg = dict(change=what, share=share, resolve_data_ms=warm_s * 1e3, solve_ms=cold_s * 1e3, speedup=cold_s / warm_s,
                       optimal=int((c.status == M.SolverStatus.Optimal).sum()), warm=rs["warm_instances"], cold_by_rule=rs["cold_instances"],
                       fallback=rs["fallback_instances"], dual_pivots=rs["dual_pivots"], primal_pivots=rs["primal_pivots"], solve_pivots=cs["total_pivots"],
                       launches=rs["launches"], solve_launches=cs["launches"], redata_ms=rs["begin_ns"] / 1e6, launches_ms=rs["kernel_ns"] / 1e6,
                       finish_ms=rs["finish_ns"] / 1e6, solve_launches_ms=cs["kernel_ns"] / 1e6, bytes_up=rs["bytes_up"], bytes_down=rs["bytes_down"])
            legs.append(leg)
            print(f"{name} {what} {share:4.0%}: resolve_data {leg['resolve_data_ms']:9.2f} ms (re-data {leg['redata_ms']:.2f}, launches {leg['launches_ms']:.2f}, "
                  f"finish {leg['finish_ms']:.2f}) against solve {leg['solve_ms']:9.2f} ms: x{leg['speedup']:.2f};  warm {leg['warm']}, cold {leg['cold_by_rule']}, "
                  f"fallback {leg['fallback']};  pivots {leg['dual_pivots']} dual + {leg['primal_pivots']} primal against {leg['solve_pivots']};  "
                  f"up {leg['bytes_up']} B, down {leg['bytes_down']} B", flush=True)
        out["families"][name] = dict(nodes=f["nodes"], arcs=f["arcs"], instances=n, first_solve_ms=first_s * 1e3, first_pivots=first_st["total_pivots"],
                                     first_optimal=int((first.status == M.SolverStatus.Optimal).sum()), lds_instances=first_st["lds_instances"], changes=legs)
        del kept, fresh
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
