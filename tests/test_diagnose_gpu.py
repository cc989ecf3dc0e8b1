"""Why an instance is infeasible, on the MI355X (mcf_ubatch_diagnose / mcf_rbatch_diagnose, DESIGN.md 3.14 "Why infeasible: a cut from the
kept flow"): one wave per instance walks the residual graph of the kept flow level by level -- marks and frontiers in LDS where the
instance is solved in LDS, in a buffer of the handle's otherwise.

Every comparison is exact: against the host hook bit for bit (verdict, violation, set_size, side, unmet and the work counts of the
stats) and against certificate_oracle.py.  The batches and the checkers are test_diagnose_host.py's.  Each test is a few launches over at
most 408 tiny instances, 64 of 161 nodes or 18 padded into the global tier."""
import numpy as np
import pytest
import torch

import mincostflow_amd as M
from oracle import ns_oracle as O

import certificate_oracle as K
import wide_graphs as W
from test_batch_host import padded_fuzz
from test_diagnose_host import (FIELDS, HOST_DIAGNOSE, HOST_SOLVE, FlatNodes, V, assert_same_diagnosis, check_contract, check_deep_path, check_edges, check_fuzz,
                                check_instance, check_one_graph, check_three_queries_on_one_handle, check_untouched, diag_rows, fuzz_flat, same_counts)
from test_ranges_host import small_case
from test_uniform_host import Topology, to_numpy, uniform_of

pytestmark = pytest.mark.gpu
SUMMARY_BYTES = 8 * 8           # five verdict counts and three work counts


def tensors(a):
    return {k: (torch.from_numpy(np.ascontiguousarray(v)).cuda() if isinstance(v, np.ndarray) else v) for k, v in a.items()}


SOLVE = lambda h, a, stype: h.solve(supply_type=stype, **tensors(a))
SOLVE_NUMPY = lambda h, a, stype: h.solve(supply_type=stype, **a)
DIAGNOSE = lambda h: h.diagnose()
DIAGNOSE_NUMPY = lambda h: h.diagnose(tensors=False)


# ---- 1: the adversarial family, from device tensors to device tensors: the LDS tier, frontiers of 1 to 60
def test_adversarial_family_equals_the_hook_and_the_oracle_on_the_device():
    rule = O.RULE_BLOCK
    flat = fuzz_flat()
    host = flat.handle(rule)
    calls = []

    def diagnose(h):
        d = h.diagnose()
        assert all(getattr(d, name).is_cuda for name in FIELDS)
        stype = O.GEQ if not calls else O.LEQ
        HOST_SOLVE(host, flat.arrays, stype)
        assert_same_diagnosis(d, HOST_DIAGNOSE(host), stype)
        st = h.diagnose_stats()
        assert st["lds_instances"] == flat.count and st["global_instances"] == 0 and same_counts(st, host.diagnose_stats()), (st, host.diagnose_stats())
        # MCF_MEM_DEVICE moves the summary words and nothing else; the table of instances goes up with the first call
        assert st["bytes_down"] == SUMMARY_BYTES and st["bytes_up"] == SUMMARY_BYTES + (0 if calls else 4 * flat.count), st
        calls.append(stype)
        return d

    check_fuzz(SOLVE, diagnose, rule)
    assert calls == [O.GEQ, O.LEQ]


# ---- 2: the global tier: a node sweep of 71 strides per level
def test_padded_instances_in_the_global_tier():
    rule = O.RULE_BLOCK
    cases = padded_fuzz(rule)
    flat = FlatNodes([q for q, _, _ in cases])
    assert all(q.n == 4500 for q in flat.problems) and flat.count == 18
    dev, host = flat.handle(rule), flat.handle(rule)
    seen = set()
    for stype in (O.GEQ, O.LEQ):
        r = to_numpy(SOLVE(dev, flat.arrays, stype))
        HOST_SOLVE(host, flat.arrays, stype)
        d = DIAGNOSE(dev)
        assert_same_diagnosis(d, HOST_DIAGNOSE(host), stype)
        st = dev.diagnose_stats()
        assert st["global_instances"] == flat.count and st["lds_instances"] == 0 and same_counts(st, host.diagnose_stats()), (st, host.diagnose_stats())
        assert st["bytes_down"] == SUMMARY_BYTES, st
        rows = diag_rows(d)
        for i, (q, own, _) in enumerate(cases):
            if own != stype:
                continue
            lo, hi = flat.node_rows[i], flat.node_rows[i + 1]
            verdict = int(rows["verdict"][i])
            assert (verdict == V.NoVerdict) == (r["status"][i] == O.UNBOUNDED), i
            check_instance(q, stype, int(r["status"][i]), verdict, int(rows["violation"][i]), int(rows["set_size"][i]), rows["side"][lo:hi], rows["unmet"][lo:hi],
                           K.feasible(q, stype), f"padded instance {i}")
            seen.add(verdict)
    assert {V.NoVerdict, V.Feasible, V.Cut} <= seen, seen


# ---- 3: a frontier wider than a wave: the ballot prefix is carried across strides
HUB_COUNT = 64


def hub_batch():
    """The hub of wide_graphs.py (node 0, 160 leaves, four spokes per leaf and a ring) 64 times with supplies of four kinds by k % 4:
    balanced (feasible), 5 units too many on one leaf (GEQ: nobody takes them, and S is everything the leaf reaches), one leaf asked to ship
    more than its three outgoing arcs carry (S is small), balanced again."""
    n, src, tgt, _, cap_range, _, _ = W.shapes()[W.HUB]
    m = len(src)
    variants = []
    for k in range(HUB_COUNT):
        rng = np.random.default_rng([W.SEED, 9, k])
        cap = rng.integers(cap_range[0], cap_range[1]).astype(np.int64)
        supply = np.zeros(n, np.int64)
        amount = rng.integers(1, 7, 12)
        leaves = rng.choice(np.arange(1, n), 24, replace=False)
        supply[leaves[:12]] += amount
        supply[leaves[12:]] -= amount
        if k % 4 == 1:
            supply[leaves[0]] += 5
        if k % 4 == 2:
            supply[leaves[0]] += 200
            supply[leaves[12]] -= 200
        variants.append(O.Problem(n, m, src, tgt, np.zeros(m, np.int64), cap, rng.integers(1, 20, m).astype(np.int64), supply))
    return Topology(n, src, tgt, variants, [False] * HUB_COUNT)


def walk_levels(p, flow, unmet):
    """The sizes of the levels of the GEQ walk from the caller's flows, restated: breadth first from the violated nodes"""
    out_of, into = [[] for _ in range(p.n)], [[] for _ in range(p.n)]
    for e in range(p.m):
        out_of[int(p.src[e])].append(e); into[int(p.tgt[e])].append(e)
    reached = set(int(v) for v in np.flatnonzero(unmet > 0))
    frontier, sizes = sorted(reached), []
    while frontier:
        sizes.append(len(frontier))
        found = set()
        for v in frontier:
            found |= {int(p.tgt[e]) for e in out_of[v] if flow[e] < p.upper[e]} | {int(p.src[e]) for e in into[v] if flow[e] > p.lower[e]}
        frontier = sorted(found - reached)
        reached |= found
    return sizes, reached


def test_a_frontier_wider_than_a_wave():
    t = hub_batch()
    truth = [K.feasible(p, O.GEQ) for p in t.variants]
    infeasible = sum(f is False for f in truth)
    assert HUB_COUNT * 3 // 8 <= infeasible <= HUB_COUNT * 5 // 8 and None not in truth, infeasible      # about half, by the independent test
    a = t.arrays()
    dev, host = uniform_of(t, O.RULE_BLOCK), uniform_of(t, O.RULE_BLOCK)
    r = to_numpy(SOLVE(dev, a, O.GEQ))
    HOST_SOLVE(host, a, O.GEQ)
    d = DIAGNOSE(dev)
    assert d.side.shape == d.unmet.shape == (HUB_COUNT, t.n) and d.side.is_cuda
    assert_same_diagnosis(d, HOST_DIAGNOSE(host), "hub")
    st = dev.diagnose_stats()
    assert st["lds_instances"] == HUB_COUNT and same_counts(st, host.diagnose_stats()) and st["open"] == 0, (st, host.diagnose_stats())
    assert st["bytes_down"] == SUMMARY_BYTES and st["bytes_up"] == SUMMARY_BYTES + 4 * HUB_COUNT, st
    rows = diag_rows(d)
    widest, levels, nodes = 0, 0, 0
    for k, p in enumerate(t.variants):
        check_instance(p, O.GEQ, int(r["status"][k]), int(rows["verdict"][k]), int(rows["violation"][k]), int(rows["set_size"][k]), rows["side"][k], rows["unmet"][k],
                       truth[k], f"hub instance {k}")
        if rows["verdict"][k] != V.Cut:
            continue
        # a surplus ends Optimal (difference D9), so the flows are in the result and the walk can be restated from them
        if r["status"][k] == O.OPTIMAL:
            sizes, reached = walk_levels(p, r["flows"][k], rows["unmet"][k])
            assert sorted(reached) == [int(v) for v in np.flatnonzero(rows["side"][k])], k
            widest = max(widest, max(sizes))
            levels += len(sizes); nodes += sum(sizes)
    assert widest > 64, widest
    restated = sum(1 for k in range(HUB_COUNT) if rows["verdict"][k] == V.Cut and r["status"][k] == O.OPTIMAL)
    assert restated >= HUB_COUNT // 8 and st["levels"] >= levels and st["frontier_nodes"] >= nodes, (restated, st, levels, nodes)


# ---- 4: depth: 299 levels, two barriers each
def test_a_path_of_299_levels_on_the_device():
    check_deep_path(SOLVE, DIAGNOSE)


# ---- 5: nothing to walk
def test_nothing_infeasible_and_everything_infeasible_by_its_bounds():
    t, a = small_case()
    zero = dict(a, supply=np.zeros_like(a["supply"]), lower=np.zeros_like(a["lower"]), upper=np.ascontiguousarray(np.maximum(a["upper"], 0)),
                cost=np.ascontiguousarray(np.abs(a["cost"])))
    bad = dict(a, upper=np.ascontiguousarray(a["lower"] - 1))
    for arrays, verdict, name in ((zero, V.Feasible, "feasible"), (bad, V.Bounds, "bounds")):
        u = uniform_of(t, O.RULE_BLOCK)
        SOLVE(u, arrays, O.GEQ)
        for d in (DIAGNOSE(u), DIAGNOSE_NUMPY(u), HOST_DIAGNOSE(u), DIAGNOSE(u)):
            rows = diag_rows(d)
            assert np.all(rows["verdict"] == verdict) and not rows["violation"].any() and not rows["set_size"].any() and not rows["side"].any() and not rows["unmet"].any(), name
            st = u.diagnose_stats()
            assert st[name] == t.count == st["instances"] and st["levels"] == st["frontier_nodes"] == st["inc_entries"] == 0, st
        assert u.stats()["instances"] == t.count and u.range_stats()["instances"] == 0 and u.cost_ranges().ranged.shape == (t.count,)
    u = M.UniformBatch(t.n, t.src, t.tgt, 0)
    SOLVE(u, {k: v[:0] for k, v in a.items()}, O.GEQ)
    d = DIAGNOSE(u)
    assert d.verdict.shape == (0,) and d.side.shape == (0, t.n) and u.diagnose_stats()["instances"] == 0


# ---- 6: the rest of the host file on the device
def test_contract_on_the_device():
    check_contract(lambda h, a: h.solve(**a), "diagnose", False)


def test_hand_made_edges_on_the_device():
    check_edges(SOLVE, DIAGNOSE)


def test_one_graph_equals_the_uniform_batch_on_the_device():
    check_one_graph(SOLVE, DIAGNOSE, stypes=(O.LEQ,))


def test_the_kept_state_is_untouched_on_the_device():
    check_untouched(SOLVE, lambda h, a, stype: h.resolve(supply_type=stype, **tensors(a)), DIAGNOSE, lambda h: h.cost_ranges())


def test_host_memory_rows_and_the_state_moving_between_host_and_device():
    t, a = small_case()
    want = None
    for solve_on_device, first_on_device in ((True, True), (True, False), (False, True), (False, False)):
        u = uniform_of(t, O.RULE_BLOCK)
        (SOLVE_NUMPY if solve_on_device else HOST_SOLVE)(u, a, O.GEQ)
        order = (DIAGNOSE_NUMPY, HOST_DIAGNOSE) if first_on_device else (HOST_DIAGNOSE, DIAGNOSE_NUMPY)
        for diagnose in order + order:
            d = diagnose(u)
            assert isinstance(d.side, np.ndarray)
            want = want or d
            assert_same_diagnosis(d, want, (solve_on_device, first_on_device))
    u = uniform_of(t, O.RULE_BLOCK)
    SOLVE_NUMPY(u, a, O.GEQ)
    DIAGNOSE_NUMPY(u)
    st = u.diagnose_stats()
    assert st["bytes_down"] == SUMMARY_BYTES + t.count * (4 + 8 + 4) + t.count * t.n * (1 + 8) and st["bytes_up"] == SUMMARY_BYTES + 4 * t.count, st
    assert V.Cut in diag_rows(want)["verdict"]


# ---- 7: the three queries of the kept state on one handle, device calls and hooks in turn
def test_three_queries_share_one_handle_on_the_device():
    check_three_queries_on_one_handle(SOLVE, lambda h, a, stype: h.resolve(supply_type=stype, **tensors(a)), True, 3)
