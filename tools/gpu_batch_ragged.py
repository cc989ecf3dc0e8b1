"""What the ragged batch (RaggedBatch: a set of graphs in one handle, flat problem data in and results out on the device) costs against the
only way there was before it for instances of different shapes: BatchSolver with one add() per instance, solve(), and the getters per index.

  4 096 instances over 16 NETGEN-like graphs of 100 - 300 nodes with 3 arcs per node, 256 instances each, interleaved (instance k is of graph
  k % 16); costs per instance, supplies per instance (its graph's), as device tensors; plain auto-configured Block Search; one MI355X, one process.

    timeout 900 python tools/gpu_batch_ragged.py [--json profiles/batch_ragged.json]

ROUNDS rounds, each running the legs one after the other:
  (i)   BatchSolver: add() per instance, solve(), status / cost / flows / potentials per index -- the yardstick;
  (ii)  RaggedBatch.solve, device tensors to device tensors, with the begin / launches / finish split of stats();
  (iii) 5 % and then 100 % of every instance's costs redrawn: set_costs() per instance + resolve() + getters against RaggedBatch.resolve;
  (iv)  RaggedBatch.validate of (ii)'s tensors as they lie;
  (v)   RaggedBatch(...) alone: what a caller whose graphs change per call pays each time.
Medians and ranges over the rounds.  Every instance's status and total cost must agree between the paths before any time is reported.
Then one single-graph workload, 4 096 x 200 / 600, through UniformBatch and RaggedBatch in alternation: what the table lookups cost the
begin and finish launches.  The script stops at the first failure."""
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

GRAPHS, PER, ROUNDS = 16, 256, 5
SHARES = (0.05, 1.0)


def to_device(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def spread(v, scale=1e3):
    return dict(median=statistics.median(v) * scale, min=min(v) * scale, max=max(v) * scale, all=[x * scale for x in v])


def split(st):
    return dict(begin_ms=st["begin_ns"] / 1e6, launches_ms=st["kernel_ns"] / 1e6, finish_ms=st["finish_ns"] / 1e6, launches=st["launches"],
                bytes_up=st["bytes_up"], bytes_down=st["bytes_down"], total_pivots=st["total_pivots"])


def read_all(b, n):
    status = [b.status(i) for i in range(n)]
    optimal = [s == M.SolverStatus.Optimal for s in status]
    return status, [b.total_cost(i) if ok else 0 for i, ok in enumerate(optimal)], [b.flows(i) if ok else None for i, ok in enumerate(optimal)], \
        [b.potentials(i) if ok else None for i, ok in enumerate(optimal)]


def agree(r, got, what):
    assert r.status.cpu().tolist() == got[0], f"{what}: the paths disagree on a status"
    assert r.total_cost.cpu().tolist() == got[1], f"{what}: the paths disagree on a total cost"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if M.device_count() < 1:
        raise SystemExit("needs an MI355X")
    graphs = []
    for g in range(GRAPHS):
        nodes = 100 + (200 * g) // (GRAPHS - 1)
        graphs.append(M.netgen_like(1000 + g, nodes, 3 * nodes, 4, 4))
    order = [k % GRAPHS for k in range(GRAPHS * PER)]
    n = len(order)
    triples = [(g.node_count, g.source, g.target) for g in graphs]
    rng = np.random.default_rng(20261106)
    cat = lambda field: np.concatenate([getattr(graphs[g], field) for g in order]).astype(np.int64)
    lower, upper, supply = cat("lower"), cat("upper"), cat("supply")
    cost = rng.integers(1, 10001, lower.shape).astype(np.int64)
    fixed = dict(supply=to_device(supply), lower=to_device(lower), upper=to_device(upper))

    def batch_solver_path(cost, count=n):
        t0 = time.perf_counter()
        b = M.BatchSolver(rule=M.PivotRule.BlockSearch)
        for i in range(count):
            g = graphs[order[i]]
            b.add(M.Problem(g.node_count, g.arc_count, g.source, g.target, g.lower, g.upper, cost[rows[i]:rows[i + 1]], g.supply))
        t1 = time.perf_counter()
        b.solve()
        got = read_all(b, count)
        return time.perf_counter() - t0, t1 - t0, b, got

    u = M.RaggedBatch(triples, order, rule=M.PivotRule.BlockSearch)
    rows = u.arc_rows
    batch_solver_path(cost, 32)                                             # warm-up of both paths: kernels loaded, allocators primed
    cost_t = to_device(cost)
    u.validate(u.solve(cost_t, **fixed), cost_t, **fixed)
    u.resolve(cost_t, **fixed)
    legs = {k: [] for k in ("batch_solver", "batch_solver_add", "batch_solver_launches", "ragged", "validate", "create")}
    splits, resolves = [], {share: dict(batch_solver=[], batch_solver_launches=[], ragged=[], split=[]) for share in SHARES}
    for _ in range(ROUNDS):
        s, a, b, got = batch_solver_path(cost)                              # (i)
        legs["batch_solver"].append(s); legs["batch_solver_add"].append(a); legs["batch_solver_launches"].append(b.stats()["kernel_ns"] / 1e9)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = u.solve(cost_t, **fixed)                                        # (ii)
        legs["ragged"].append(time.perf_counter() - t0)
        splits.append(split(u.stats()))
        agree(r, got, "solve")
        for i in (0, 1, n // 2, n - 1):
            if got[2][i] is not None:
                assert np.array_equal(r.arcs(i).cpu().numpy(), got[2][i]) and np.array_equal(r.nodes(i).cpu().numpy(), got[3][i])
        t0 = time.perf_counter()
        v = u.validate(r, cost_t, **fixed)                                  # (iv)
        legs["validate"].append(time.perf_counter() - t0)
        assert v.summary["bytes_up"] == 16 and v.summary["bytes_down"] == 16
        for share in SHARES:                                                # (iii)
            hit = rng.random(cost.shape) < share
            cost = np.where(hit, rng.integers(1, 10001, cost.shape), cost).astype(np.int64)
            cost_t = to_device(cost)
            t0 = time.perf_counter()
            for i in range(n):
                b.set_costs(i, cost[rows[i]:rows[i + 1]])
            b.resolve()
            got = read_all(b, n)
            old = time.perf_counter() - t0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = u.resolve(cost_t, **fixed)
            new = time.perf_counter() - t0
            agree(r, got, f"re-solve, {share:.0%} redrawn")
            leg = resolves[share]
            leg["batch_solver"].append(old); leg["batch_solver_launches"].append(b.resolve_stats()["kernel_ns"] / 1e9); leg["ragged"].append(new); leg["split"].append(split(u.stats()))
        t0 = time.perf_counter()
        fresh = M.RaggedBatch(triples, order, rule=M.PivotRule.BlockSearch)        # (v)
        legs["create"].append(time.perf_counter() - t0)
        del fresh, b
    k = legs["ragged"].index(sorted(legs["ragged"])[ROUNDS // 2])
    st = u.stats()
    out = dict(rule="BlockSearch (plain, auto-configured)", graphs=GRAPHS, instances=n, nodes=[g.node_count for g in graphs], arcs=[g.arc_count for g in graphs], rounds=ROUNDS,
               lds_instances=st["lds_instances"], global_instances=st["global_instances"], workspace_bytes=st["workspace_bytes"],
               solve={name: spread(v) for name, v in legs.items()}, ragged_split_of_median_round=splits[k], ragged_splits=splits,
               speedup=statistics.median(legs["batch_solver"]) / statistics.median(legs["ragged"]),
               resolves=[dict(share=share, batch_solver_ms=spread(leg["batch_solver"]), batch_solver_launches_ms=spread(leg["batch_solver_launches"]), ragged_ms=spread(leg["ragged"]),
                              ragged_splits=leg["split"], speedup=statistics.median(leg["batch_solver"]) / statistics.median(leg["ragged"])) for share, leg in resolves.items()])
    launches_i, launches_ii = [x * 1e3 for x in legs["batch_solver_launches"]], [s["launches_ms"] for s in splits]
    out["fixed_in_advance"] = dict(
        ragged_launch_time_within_batch_solvers_range=bool(min(launches_i) <= statistics.median(launches_ii) <= max(launches_i)),
        begin_plus_finish_below_launches=bool(all(s["begin_ms"] + s["finish_ms"] < s["launches_ms"] for s in splits)))
    print(f"solve: BatchSolver {out['solve']['batch_solver']['median']:.2f} ms (add {out['solve']['batch_solver_add']['median']:.2f}, launches {out['solve']['batch_solver_launches']['median']:.2f} "
          f"[{min(launches_i):.2f}, {max(launches_i):.2f}]); RaggedBatch {out['solve']['ragged']['median']:.2f} ms [{out['solve']['ragged']['min']:.2f}, {out['solve']['ragged']['max']:.2f}] "
          f"(begin {splits[k]['begin_ms']:.3f}, launches {splits[k]['launches_ms']:.2f}, finish {splits[k]['finish_ms']:.3f}): x{out['speedup']:.2f}; "
          f"validate {out['solve']['validate']['median']:.3f} ms, create {out['solve']['create']['median']:.2f} ms; {out['fixed_in_advance']}", flush=True)
    for leg in out["resolves"]:
        print(f"{leg['share']:4.0%} redrawn: set_costs + resolve + getters {leg['batch_solver_ms']['median']:.2f} ms; RaggedBatch.resolve {leg['ragged_ms']['median']:.2f} ms: x{leg['speedup']:.2f}", flush=True)

    # ---- one graph: the table lookups against the strides
    g = M.netgen_like(1, 200, 600, 4, 4)
    count = 4096
    cost1 = rng.integers(1, 10001, (count, g.arc_count)).astype(np.int64)
    uni = M.UniformBatch(g.node_count, g.source, g.target, count, rule=M.PivotRule.BlockSearch)
    rag = M.RaggedBatch([(g.node_count, g.source, g.target)], [0] * count, rule=M.PivotRule.BlockSearch)
    a2 = dict(cost=to_device(cost1), supply=to_device(np.tile(g.supply, (count, 1))), lower=to_device(np.tile(g.lower, (count, 1))), upper=to_device(np.tile(g.upper, (count, 1))))
    a1 = {name: t.reshape(-1) for name, t in a2.items()}
    uni.solve(**a2); rag.solve(**a1)
    single = dict(uniform=[], ragged=[])
    for _ in range(ROUNDS):
        ru = uni.solve(**a2)
        single["uniform"].append(split(uni.stats()))
        rr = rag.solve(**a1)
        single["ragged"].append(split(rag.stats()))
        assert torch.equal(ru.flows.reshape(-1), rr.flows) and torch.equal(ru.total_cost, rr.total_cost) and torch.equal(ru.potentials.reshape(-1), rr.potentials)
    both = lambda rows: [s["begin_ms"] + s["finish_ms"] for s in rows]
    bu, br = both(single["uniform"]), both(single["ragged"])
    out["single_graph"] = dict(nodes=200, arcs=600, instances=count, uniform=single["uniform"], ragged=single["ragged"],
                               uniform_begin_plus_finish_ms=spread(bu, 1), ragged_begin_plus_finish_ms=spread(br, 1),
                               lookups_cost_no_more_than_uniforms_spread=bool(statistics.median(br) - statistics.median(bu) <= max(bu) - min(bu)))
    print(f"one graph 4096 x 200 / 600: begin + finish UniformBatch {statistics.median(bu):.3f} ms [{min(bu):.3f}, {max(bu):.3f}], RaggedBatch {statistics.median(br):.3f} ms "
          f"[{min(br):.3f}, {max(br):.3f}]", flush=True)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
