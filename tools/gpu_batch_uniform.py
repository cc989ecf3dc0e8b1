"""What the uniform batch (UniformBatch: one topology, problem data in and results out on the device) costs against the only way there was
before it: BatchSolver with one add() per instance, solve(), and flows, potentials and cost read per index.  Two families on one
generated graph each, costs drawn per instance, plain auto-configured Block Search, one MI355X, one process:

  small  4 096 x 200 nodes / 600 arcs       (LDS tier)
  large    256 x 10 000 nodes / 30 000 arcs (global tier)

    timeout 1100 python tools/gpu_batch_uniform.py [--json profiles/batch_uniform.json]

Per family: REPEATS rounds that alternate the two paths (the large family: one round).  The BatchSolver path is timed from the first
add() to the last getter; the UniformBatch path from device tensors to device tensors round solve(), which returns synchronised, after
one warm-up call of the same shape; its begin / launches / finish split is the library's own (mcf_ubatch_stats, host clock round each
phase, each ended by a synchronise).  Then 5 % and 100 % of every instance's costs are redrawn and both handles re-solve:
set_costs() per instance + resolve() + the getters against resolve() on a device tensor.  Every instance must end Optimal and both
paths must agree on every total cost (the solves also on flows and potentials).  The script stops at the first failure."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch  # noqa: F401  (before the library: one HIP runtime per process, torch's)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import mincostflow_amd as M  # noqa: E402

FAMILIES = {
    "small": dict(nodes=200, arcs=600, ends=4, count=4096, seed=1, repeats=5),
    "large": dict(nodes=10_000, arcs=30_000, ends=100, count=256, seed=100_001, repeats=1),
}
SHARES = (0.05, 1.0)


def to_device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def synchronize():
    import torch
    torch.cuda.synchronize()


def read_all(b, n):
    return [b.total_cost(i) for i in range(n)], [b.flows(i) for i in range(n)], [b.potentials(i) for i in range(n)]


def batch_solver_path(g, cost):
    """(seconds, seconds in add, stats, handle, (costs, flows, potentials))"""
    n = cost.shape[0]
    t0 = time.perf_counter()
    b = M.BatchSolver(rule=M.PivotRule.BlockSearch)
    for c in cost:
        b.add(M.Problem(g.node_count, g.arc_count, g.source, g.target, g.lower, g.upper, c, g.supply))
    t1 = time.perf_counter()
    b.solve()
    got = read_all(b, n)
    t2 = time.perf_counter()
    assert all(b.status(i) == M.SolverStatus.Optimal for i in range(n))
    return t2 - t0, t1 - t0, b.stats(), b, got


def split(st):
    return dict(begin_ms=st["begin_ns"] / 1e6, launches_ms=st["kernel_ns"] / 1e6, finish_ms=st["finish_ns"] / 1e6, launches=st["launches"],
                bytes_up=st["bytes_up"], bytes_down=st["bytes_down"], total_pivots=st["total_pivots"])


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
        rng = np.random.default_rng(20261019)
        cost = rng.integers(1, 10001, (n, g.arc_count)).astype(np.int64)
        shared = dict(supply=to_device(g.supply), lower=to_device(g.lower), upper=to_device(g.upper))
        cost_t = to_device(cost)
        u = M.UniformBatch(g.node_count, g.source, g.target, n, rule=M.PivotRule.BlockSearch)
        batch_solver_path(g, cost[:8])                                      # warm-up of both paths: kernels loaded, allocators primed
        u.solve(cost_t, **shared)
        old_s, new_s, add_s, splits = [], [], [], []
        for _ in range(f["repeats"]):
            s, a, bst, b, got = batch_solver_path(g, cost)
            old_s.append(s)
            add_s.append(a)
            synchronize()
            t0 = time.perf_counter()
            r = u.solve(cost_t, **shared)
            new_s.append(time.perf_counter() - t0)
            splits.append(split(u.stats()))
            assert bool((r.status == M.SolverStatus.Optimal).all())
            assert r.total_cost.cpu().tolist() == got[0], "the two paths disagree on an optimum"
            assert np.array_equal(r.flows.cpu().numpy(), np.stack(got[1])) and np.array_equal(r.potentials.cpu().numpy(), np.stack(got[2]))
        med = lambda v: statistics.median(v)
        k = new_s.index(sorted(new_s)[len(new_s) // 2])
        solve = dict(batch_solver_ms=med(old_s) * 1e3, batch_solver_all_ms=[s * 1e3 for s in old_s], of_it_add_ms=med(add_s) * 1e3,
                     batch_solver_launches_ms=bst["kernel_ns"] / 1e6, uniform_ms=med(new_s) * 1e3, uniform_all_ms=[s * 1e3 for s in new_s],
                     speedup=med(old_s) / med(new_s), uniform_split=splits[k], lds_instances=u.stats()["lds_instances"], workspace_bytes=u.stats()["workspace_bytes"])
        print(f"{name} solve: BatchSolver add + solve + getters {solve['batch_solver_ms']:9.2f} ms (add {solve['of_it_add_ms']:8.2f}, launches {solve['batch_solver_launches_ms']:9.2f}); "
              f"UniformBatch {solve['uniform_ms']:9.2f} ms (begin {splits[k]['begin_ms']:.2f}, launches {splits[k]['launches_ms']:.2f}, finish {splits[k]['finish_ms']:.2f}): "
              f"x{solve['speedup']:.2f};  up {splits[k]['bytes_up']} B, down {splits[k]['bytes_down']} B", flush=True)
        legs = []
        u.resolve(cost_t, **shared)                                         # warm-up of the re-cost kernel: the same costs, no pivot
        for share in SHARES:
            hit = rng.random(cost.shape) < share
            cost = np.where(hit, rng.integers(1, 10001, cost.shape), cost).astype(np.int64)
            cost_t = to_device(cost)
            t0 = time.perf_counter()
            for i in range(n):
                b.set_costs(i, cost[i])
            b.resolve()
            got = read_all(b, n)
            old = time.perf_counter() - t0
            rst = b.resolve_stats()
            synchronize()
            t0 = time.perf_counter()
            r = u.resolve(cost_t, **shared)
            new = time.perf_counter() - t0
            st = split(u.stats())
            assert bool((r.status == M.SolverStatus.Optimal).all()) and all(b.status(i) == M.SolverStatus.Optimal for i in range(n))
            assert r.total_cost.cpu().tolist() == got[0], "the two re-solves disagree on an optimum"
            legs.append(dict(share=share, batch_solver_ms=old * 1e3, batch_solver_launches_ms=rst["kernel_ns"] / 1e6, uniform_ms=new * 1e3, speedup=old / new, uniform_split=st))
            print(f"{name} {share:4.0%} redrawn: set_costs + resolve + getters {old * 1e3:9.2f} ms (launches {rst['kernel_ns'] / 1e6:9.2f}); UniformBatch.resolve {new * 1e3:9.2f} ms "
                  f"(re-cost {st['begin_ms']:.2f}, launches {st['launches_ms']:.2f}, finish {st['finish_ms']:.2f}): x{old / new:.2f}", flush=True)
        out["families"][name] = dict(nodes=f["nodes"], arcs=f["arcs"], instances=n, repeats=f["repeats"], solve=solve, resolves=legs)
        del b, u
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
