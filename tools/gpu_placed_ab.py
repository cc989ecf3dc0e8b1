"""Host-side timing and result digests of the uniform and the ragged batch of ONE checkout, for comparing two builds of the library in
alternating processes (profiles/placed_batch_refactor_same_kernels_same_speed.txt):

    timeout 150 python tools/gpu_placed_ab.py TREE OUT.json          # TREE: the root of a built checkout, this one or another

The workloads of gpu_batch_ragged.py (4 096 instances over 16 graphs) and of gpu_batch_uniform.py's small family (4 096 x 200 / 600),
device tensors in and out, record_trace = 32.  Seven rounds of create, solve, validate, a 5 % and a 100 % re-solve: wall time round each
call and the library's own begin_ns / finish_ns / host_ns; then numpy arrays in (MCF_MEM_HOST: the staged path) for three solves, a
masked re-solve and a validation.  sha256 of every result array of every call and the statistics that are not times go into the JSON,
so that two builds can be compared bit for bit."""
import hashlib
import json
import statistics
import sys
import time

import numpy as np
import torch

root, out_path = sys.argv[1], sys.argv[2]
sys.path.insert(0, root)
import mincostflow_amd as M  # noqa: E402

assert M.LIB_PATH.startswith(root), (M.LIB_PATH, root)
ROUNDS = 7


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def digest(r, names):
    out = {}
    for name in names:
        a = getattr(r, name)
        a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
        out[name] = hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    return out


SOLVE = ("status", "pivots", "total_cost", "flows", "potentials", "trace")
CHECK = ("valid", "errors", "first", "objective", "dual_cost")


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    return r, (time.perf_counter() - t0) * 1e3


def run(make, cost0, fixed, fixed_np):
    """make() -> handle; cost0: numpy costs in the handle's shape"""
    res = dict(times={k: [] for k in ("create", "solve", "resolve_5", "resolve_100", "validate", "solve_numpy")},
               stats={k: [] for k in ("solve", "resolve_5", "resolve_100")}, digests={})
    u, _ = timed(make)
    rng = np.random.default_rng(7)
    cost = cost0.copy()
    cost_t = dev(cost)
    u.validate(u.solve(cost_t, **fixed), cost_t, **fixed)
    u.resolve(cost_t, **fixed)
    keep = ("begin_ns", "finish_ns", "host_ns", "kernel_ns", "bytes_up", "bytes_down", "launches", "total_pivots", "lds_instances", "global_instances", "workspace_bytes")
    for rnd in range(ROUNDS):
        fresh, t = timed(make)
        res["times"]["create"].append(t)
        del fresh
        r, t = timed(lambda: u.solve(cost_t, **fixed))
        res["times"]["solve"].append(t)
        res["stats"]["solve"].append({k: u.stats()[k] for k in keep})
        res["digests"][f"solve_{rnd}"] = digest(r, SOLVE)
        v, t = timed(lambda: u.validate(r, cost_t, **fixed))
        res["times"]["validate"].append(t)
        res["digests"][f"validate_{rnd}"] = dict(digest(v, CHECK), invalid=v.summary["invalid"], bytes=[v.summary["bytes_up"], v.summary["bytes_down"]])
        for share, leg in ((0.05, "resolve_5"), (1.0, "resolve_100")):
            hit = rng.random(cost.shape) < share
            cost = np.where(hit, rng.integers(1, 10001, cost.shape), cost).astype(np.int64)
            cost_t = dev(cost)
            r, t = timed(lambda: u.resolve(cost_t, **fixed))
            res["times"][leg].append(t)
            res["stats"][leg].append({k: u.stats()[k] for k in keep})
            res["digests"][f"{leg}_{rnd}"] = digest(r, SOLVE)
    # MCF_MEM_HOST: the staged path, a solve, a masked re-solve and a validation
    for rnd in range(3):
        r, t = timed(lambda: u.solve(cost, **fixed_np))
        res["times"]["solve_numpy"].append(t)
    res["digests"]["solve_numpy"] = digest(r, SOLVE)
    res["stats"]["solve_numpy"] = {k: u.stats()[k] for k in keep}
    mask = (np.arange(len(u)) % 3 != 1)
    r = u.resolve(cost, changed=mask, **fixed_np)
    res["digests"]["resolve_numpy_masked"] = digest(r, SOLVE)
    res["stats"]["resolve_numpy_masked"] = {k: u.stats()[k] for k in keep}
    v = u.validate(r, cost, **fixed_np)
    res["digests"]["validate_numpy"] = dict(digest(v, CHECK), invalid=v.summary["invalid"], bytes=[v.summary["bytes_up"], v.summary["bytes_down"]])
    res["median"] = {k: statistics.median(v) for k, v in res["times"].items()}
    for leg in ("solve", "resolve_5", "resolve_100"):
        for k in ("begin_ns", "finish_ns", "host_ns"):
            res["median"][f"{leg}.{k[:-3]}_ms"] = statistics.median(s[k] for s in res["stats"][leg]) / 1e6
    return res


def main():
    out = {}
    # ragged: 4 096 instances over 16 graphs of 100 - 300 nodes, interleaved
    graphs = [M.netgen_like(1000 + g, 100 + (200 * g) // 15, 3 * (100 + (200 * g) // 15), 4, 4) for g in range(16)]
    order = [k % 16 for k in range(16 * 256)]
    cat = lambda field: np.concatenate([getattr(graphs[g], field) for g in order]).astype(np.int64)
    fixed_np = dict(supply=cat("supply"), lower=cat("lower"), upper=cat("upper"))
    cost = np.random.default_rng(20261106).integers(1, 10001, fixed_np["lower"].shape).astype(np.int64)
    triples = [(g.node_count, g.source, g.target) for g in graphs]
    out["ragged"] = run(lambda: M.RaggedBatch(triples, order, rule=M.PivotRule.BlockSearch, record_trace=32), cost, {k: dev(v) for k, v in fixed_np.items()}, fixed_np)
    # uniform: 4 096 x 200 / 600, shared supply and bounds
    g = M.netgen_like(1, 200, 600, 4, 4)
    fixed_np = dict(supply=np.asarray(g.supply, np.int64), lower=np.asarray(g.lower, np.int64), upper=np.asarray(g.upper, np.int64))
    cost = np.random.default_rng(20261019).integers(1, 10001, (4096, g.arc_count)).astype(np.int64)
    out["uniform"] = run(lambda: M.UniformBatch(g.node_count, g.source, g.target, 4096, rule=M.PivotRule.BlockSearch, record_trace=32), cost,
                         {k: dev(v) for k, v in fixed_np.items()}, fixed_np)
    with open(out_path, "w") as fh:
        json.dump(out, fh, indent=1)
    for kind in out:
        print(kind, {k: round(v, 3) for k, v in out[kind]["median"].items()}, flush=True)


main()
