"""Why an instance is infeasible (mcf_ubatch_diagnose_on_host / mcf_rbatch_diagnose_on_host, DESIGN.md 3.14 "Why infeasible: a cut from the
kept flow") without a GPU: the hooks run the device's own step (csrc/diagnose_step.hip.h) with one lane on the CPU.

Every comparison is exact.  The reference is certificate_oracle.py: a max-flow feasibility test and an exact-integer check of every cut,
both on the caller's own numbers and neither sharing anything with the code under test.  test_diagnose_gpu.py imports the batches and
the checkers from here."""
import ctypes as C
import functools
import itertools
import os
import subprocess

import numpy as np
import pytest

import mincostflow_amd as M
from mincostflow_amd import _lib as L
from oracle import ns_oracle as O

import certificate_oracle as K
from test_batch_host import ROOT, RULES, fuzz_cases, fuzz_reference
from test_data_ranges_host import two_tiers
from test_ranges_host import Flat, range_rows, small_case
from test_uniform_host import ALL_RULES, family, to_numpy, uniform_of

V = M.Verdict
FIELDS = ("verdict", "violation", "set_size", "side", "unmet")
COUNTS = ("instances", "none", "feasible", "cut", "open", "bounds", "levels", "frontier_nodes", "inc_entries")        # what host and device must agree on


def diag_rows(d):
    get = lambda a: a if a is None or isinstance(a, np.ndarray) else a.cpu().numpy()
    return {name: get(getattr(d, name)) for name in FIELDS}


def assert_same_diagnosis(a, b, what=""):
    a, b = diag_rows(a), diag_rows(b)
    for name in FIELDS:
        assert a[name].dtype == b[name].dtype and np.array_equal(a[name].reshape(-1), b[name].reshape(-1)), (what, name)


def same_counts(a, b):
    return all(a[f] == b[f] for f in COUNTS)


def node_rows_of(problems):
    return np.concatenate([[0], np.cumsum([p.n for p in problems])]).astype(np.int64)


class FlatNodes(Flat):
    """Flat with the node rows a diagnosis is read by"""

    def __init__(self, problems):
        super().__init__(problems)
        self.node_rows = node_rows_of(self.problems)


@functools.lru_cache(maxsize=None)
def fuzz_flat():
    return FlatNodes([p for p, _ in fuzz_cases()])


@functools.lru_cache(maxsize=None)
def fuzz_truth():
    """feasible() per instance of the adversarial family (None: infeasible by an arc's bounds).  Asserted here: it agrees with the SEM_LEMON
    oracle's Optimal / Infeasible wherever that oracle does not answer Unbounded."""
    truth = tuple(K.feasible(p, stype) for p, stype in fuzz_cases())
    compared = 0
    for (p, stype), f in zip(fuzz_cases(), truth):
        if f is None:
            assert np.any(p.upper < p.lower)
            continue
        st, _ = O.Oracle(p, O.SEM_LEMON, O.RULE_BLOCK, supply_type=stype).solve()
        if st == O.UNBOUNDED:
            continue
        assert st in (O.OPTIMAL, O.INFEASIBLE) and (st == O.OPTIMAL) == f, (p.n, p.m, stype, st, f)
        compared += 1
    assert compared >= 300 and sum(f is None for f in truth) == 5
    return truth


def check_instance(p, stype, status, verdict, violation, set_size, side, unmet, truth, what):
    """One diagnosed row against the independent oracle"""
    assert verdict != V.Open, what                                           # the condition, not a measurement
    violated = unmet > 0 if stype == O.GEQ else unmet < 0
    if verdict in (V.NoVerdict, V.Bounds):
        assert not side.any() and not unmet.any() and violation == 0 and set_size == 0, what
        return
    assert (verdict == V.Feasible) == (truth is True), (what, verdict, truth)
    # unmet is zero outside violated and slack nodes by its meaning; what can be said of it without the flow: the caller's arcs create
    # nothing, so the unmet amounts sum to the supplies (the lower bounds' shifts cancel)
    assert int(unmet.sum()) == int(p.supply.sum()), what
    if verdict == V.Feasible:
        assert not violated.any() and not side.any() and violation == 0 and set_size == 0, what
        return
    assert verdict == V.Cut and truth is False, (what, verdict, truth)
    K.check_cut(p, stype, side, violation)
    assert set(np.unique(side)) <= {0, 1} and int(side.sum()) == set_size, what
    assert not np.any(violated & (side == 0)), what                         # every violated node is a seed
    inside = unmet[side == 1]
    assert np.all(inside >= 0 if stype == O.GEQ else inside <= 0) and int(np.abs(inside).sum()) == violation, what


def check_fuzz(solve, diagnose, rule, stats_check=None):
    """The adversarial family in one ragged handle, solved under each supply type; every instance is judged under its own.  Returns
    {supply type: rows} for what the caller adds."""
    cases, flat, truth = fuzz_cases(), fuzz_flat(), fuzz_truth()
    reference = [st for _, st, _ in fuzz_reference(rule)]
    # floors on the independent answers: the oracle's status (the reference's semantics, not the code under test) and feasible()
    diagnosed = [k for k, (st, f) in enumerate(zip(reference, truth)) if st != O.UNBOUNDED and f is not None]
    floors = dict(feasible=sum(truth[k] for k in diagnosed), infeasible=sum(not truth[k] for k in diagnosed),
                  infeasible_leq=sum(not truth[k] and cases[k][1] == O.LEQ for k in diagnosed),
                  optimal_although_infeasible=sum(not truth[k] and reference[k] == O.OPTIMAL for k in diagnosed),
                  infeasible_although_feasible=sum(truth[k] and reference[k] == O.INFEASIBLE for k in diagnosed),
                  infeasible_above_a_stride=sum(not truth[k] and cases[k][0].m + cases[k][0].n > 64 for k in diagnosed))
    print(f"rule {rule}: {floors}, not diagnosed {len(cases) - len(diagnosed)}")
    assert floors["feasible"] >= 150 and floors["infeasible"] >= 200 and floors["infeasible_leq"] >= 30, floors
    assert floors["optimal_although_infeasible"] >= 40 and floors["infeasible_although_feasible"] >= 10 and floors["infeasible_above_a_stride"] >= 100, floors
    h = flat.handle(rule)
    out, seen = {}, {v: 0 for v in range(5)}
    for stype in (O.GEQ, O.LEQ):
        r = to_numpy(solve(h, flat.arrays, stype))
        d = diagnose(h)
        rows = diag_rows(d)
        assert rows["verdict"].shape == rows["violation"].shape == rows["set_size"].shape == (flat.count,)
        assert rows["side"].shape == rows["unmet"].shape == (flat.node_rows[-1],)
        assert rows["verdict"].dtype == rows["set_size"].dtype == np.int32 and rows["violation"].dtype == rows["unmet"].dtype == np.int64 and rows["side"].dtype == np.int8
        for i in (k for k, (_, s) in enumerate(cases) if s == stype):
            p = cases[i][0]
            lo, hi = flat.node_rows[i], flat.node_rows[i + 1]
            verdict, status = int(rows["verdict"][i]), int(r["status"][i])
            assert status == reference[i], i
            assert (verdict == V.NoVerdict) == (status == O.UNBOUNDED), (i, verdict, status)
            assert (verdict == V.Bounds) == (truth[i] is None), (i, verdict)
            side, unmet = d.nodes(i)
            assert len(side) == len(unmet) == hi - lo
            check_instance(p, stype, status, verdict, int(rows["violation"][i]), int(rows["set_size"][i]), rows["side"][lo:hi], rows["unmet"][lo:hi], truth[i],
                           f"instance {i}, supply type {stype}")
            seen[verdict] += 1
        st = h.diagnose_stats()
        assert st["instances"] == flat.count and st["open"] == 0, st
        for name, verdict in (("none", V.NoVerdict), ("feasible", V.Feasible), ("cut", V.Cut), ("bounds", V.Bounds)):
            assert st[name] == int(np.sum(rows["verdict"] == verdict)), (name, st)
        walked = np.isin(rows["verdict"], (V.Cut, V.Open))
        assert st["frontier_nodes"] == int(rows["set_size"][walked].sum()) and st["levels"] >= int(walked.sum()) and st["inc_entries"] > 0, st
        if stats_check:
            stats_check(st)
        out[stype] = rows
    assert sum(seen.values()) == flat.count and seen[V.Feasible] == floors["feasible"] and seen[V.Cut] == floors["infeasible"], (seen, floors)
    return out


HOST_SOLVE = lambda h, a, stype: h.run_on_host(supply_type=stype, **a)
HOST_DIAGNOSE = lambda h: h.diagnose_on_host()


def host_stats(st):
    assert st["lds_instances"] == st["global_instances"] == st["bytes_up"] == st["bytes_down"] == 0, st


# ---- 1: the adversarial family against the independent oracle
@pytest.mark.parametrize("rule", ALL_RULES)
def test_adversarial_family_on_the_host(rule):
    check_fuzz(HOST_SOLVE, HOST_DIAGNOSE, rule, host_stats)


# ---- 2: hand-made edges
def problem(n, arcs, supply):
    """arcs: (tail, head, lower, upper or None, cost)"""
    src, tgt = [a[0] for a in arcs], [a[1] for a in arcs]
    lower, upper, cost = [a[2] for a in arcs], [O.INF_CAP if a[3] is None else a[3] for a in arcs], [a[4] for a in arcs]
    return O.Problem(n, len(arcs), np.array(src, np.int32), np.array(tgt, np.int32), np.array(lower, np.int64), np.array(upper, np.int64), np.array(cost, np.int64),
                     np.array(supply, np.int64))


def one(p, stype=O.GEQ, solve=HOST_SOLVE, diagnose=HOST_DIAGNOSE):
    """(verdict, violation, S as a sorted list, unmet, handle) of p alone in a ragged handle, checked against the oracle"""
    flat = FlatNodes([p])
    h = flat.handle()
    r = to_numpy(solve(h, flat.arrays, stype))
    rows = diag_rows(diagnose(h))
    check_instance(p, stype, int(r["status"][0]), int(rows["verdict"][0]), int(rows["violation"][0]), int(rows["set_size"][0]), rows["side"], rows["unmet"],
                   K.feasible(p, stype), "hand-made")
    return int(rows["verdict"][0]), int(rows["violation"][0]), [int(v) for v in np.flatnonzero(rows["side"])], [int(u) for u in rows["unmet"]], h


def edge_cases():
    """(name, problem, supply type, verdict, violation, S)"""
    bridge = lambda cap, last: problem(4, [(0, 1, 0, 10, 1), (1, 2, 0, cap, 1), (2, 3, 0, last, 1)], [5, 0, 0, -5])
    return (("a saturated bridge", bridge(3, 10), O.GEQ, V.Cut, 2, [0, 1]),
            ("the bridge uncapacitated, the shortfall at the sink's own arc", bridge(None, 3), O.GEQ, V.Cut, 2, [0, 1, 2]),
            ("the same bridge under LEQ: the sink side cannot be served", bridge(3, 10), O.LEQ, V.Cut, 2, [2, 3]),
            ("a bridge wide enough", bridge(5, 10), O.GEQ, V.Feasible, 0, []),
            ("a lower bound on an arc that enters S", problem(2, [(1, 0, 4, 10, 1), (0, 1, 0, 1, 1)], [0, 0]), O.GEQ, V.Cut, 3, [0]),
            ("surplus with no arcs at all", problem(2, [], [3, 0]), O.GEQ, V.Cut, 3, [0]),
            ("one node with a surplus", problem(1, [], [2]), O.GEQ, V.Cut, 2, [0]),
            ("one node with a self loop and nothing to ship", problem(1, [(0, 0, 0, 4, 1)], [0]), O.GEQ, V.Feasible, 0, []),
            ("one node that may keep its demand", problem(1, [], [-2]), O.GEQ, V.Feasible, 0, []),
            ("one node whose demand nobody serves", problem(1, [], [-2]), O.LEQ, V.Cut, 2, [0]),
            ("no arcs, three nodes", problem(3, [], [1, -1, 0]), O.GEQ, V.Cut, 1, [0]),
            ("parallel arcs and a self loop on the way", problem(3, [(0, 1, 0, 2, 1), (0, 1, 0, 1, 2), (1, 1, 0, 5, 0), (1, 2, 0, 9, 1)], [6, 0, -6]), O.GEQ, V.Cut, 3, [0]),
            ("a lower bound that ends in a dead end", problem(2, [(0, 1, 2, 3, 1)], [0, 0]), O.GEQ, V.Cut, 2, [1]))


def check_edges(solve, diagnose):
    for name, p, stype, verdict, violation, cut in edge_cases():
        got = one(p, stype, solve, diagnose)
        assert got[:3] == (verdict, violation, cut), (name, got[:4])


def test_hand_made_edges_on_the_host():
    check_edges(HOST_SOLVE, HOST_DIAGNOSE)


def test_status_is_not_feasibility():
    """The two ways the status word differs from the truth, on three nodes each"""
    # LEQ (net outflow <= supply): the sink must receive 5, the source may send up to 7: the slack stays on a root link -> Infeasible by D9
    p = problem(2, [(0, 1, 0, 9, 1)], [7, -5])
    flat = FlatNodes([p])
    h = flat.handle()
    r = h.run_on_host(supply_type=O.LEQ, **flat.arrays)
    d = h.diagnose_on_host()
    assert K.feasible(p, O.LEQ) and r.status[0] == O.INFEASIBLE and d.verdict[0] == V.Feasible and list(d.unmet) == [2, 0]
    # GEQ with a surplus nobody takes: it ends on an artificial arc and the status says Optimal
    h = flat.handle()
    r = h.run_on_host(supply_type=O.GEQ, **flat.arrays)
    d = h.diagnose_on_host()
    assert not K.feasible(p, O.GEQ) and r.status[0] == O.OPTIMAL and d.verdict[0] == V.Cut and d.violation[0] == 2 and list(d.side) == [1, 1]


def test_diagnose_follows_every_kind_of_solve_call():
    """Made feasible again by resolve_data() and infeasible by it; after resolve() and after solve_from()"""
    wide, narrow = problem(4, [(0, 1, 0, 10, 1), (1, 2, 0, 6, 1), (2, 3, 0, 10, 1)], [5, 0, 0, -5]), problem(4, [(0, 1, 0, 10, 1), (1, 2, 0, 3, 1), (2, 3, 0, 10, 1)], [5, 0, 0, -5])
    fw, fn = FlatNodes([wide]), FlatNodes([narrow])
    h = fn.handle()
    h.run_on_host(**fn.arrays)
    d = h.diagnose_on_host()
    assert d.verdict[0] == V.Cut and d.violation[0] == 2 and list(d.side) == [1, 1, 0, 0]
    h.rerun_data_on_host(**fw.arrays)
    d = h.diagnose_on_host()
    assert d.verdict[0] == V.Feasible and not d.side.any() and not d.unmet.any()
    states = h.cost_ranges_on_host().arc_state.copy()
    assert h.cost_ranges_on_host().ranged[0] == 1
    h.rerun_data_on_host(**fn.arrays)
    d = h.diagnose_on_host()
    assert d.verdict[0] == V.Cut and d.violation[0] == 2 and list(d.side) == [1, 1, 0, 0] and list(d.unmet) == [2, 0, 0, -2]
    # new costs: the cut is the data's, not the costs'
    h.rerun_on_host(**dict(fn.arrays, cost=np.array([3, 1, 2], np.int64)))
    assert_same_diagnosis(h.diagnose_on_host(), d)
    # from a given basis, on a handle that has never solved: the feasible data's basis, then the narrow bridge
    g = fw.handle()
    g.run_from_on_host(states, **fw.arrays)
    assert g.diagnose_on_host().verdict[0] == V.Feasible
    g.run_from_on_host(states, **fn.arrays)
    assert_same_diagnosis(g.diagnose_on_host(), d)


def test_diagnose_before_a_solve_is_refused():
    t, _ = small_case()
    for h in (uniform_of(t, O.RULE_BLOCK), Flat(t.variants).handle()):
        with pytest.raises(M.McfError) as ei:
            h.diagnose_on_host()
        assert ei.value.code == L.ERR_STATE
        with pytest.raises(M.McfError) as ei:
            h.diagnose(tensors=False)
        assert ei.value.code == L.ERR_STATE
        assert h.diagnose_stats() == {name: 0 for name, _ in L.UBatchDiagnoseStats._fields_}


# ---- 3: depth
PATH_NODES = 300


def deep_path(stype):
    """A path of 300 nodes, 5 units to move from node 0 to node 299 and one arc of capacity 2 at the end FAR from where the walk begins:
    299 levels with a frontier of one node each.  GEQ walks from node 0 (it cannot ship) along the arcs and the tight arc is the last one;
    LEQ walks from node 299 (it is not served) against them and the tight arc is the first.  The arcs are numbered against the walk: each
    level finds its arc below the one before."""
    n = PATH_NODES
    tails = np.arange(n - 1)
    if stype == O.GEQ:
        tails = tails[::-1]
    tight = n - 2 if stype == O.GEQ else 0
    supply = np.zeros(n, np.int64)
    supply[0], supply[n - 1] = 5, -5
    return O.Problem(n, n - 1, tails.astype(np.int32), (tails + 1).astype(np.int32), np.zeros(n - 1, np.int64), np.where(tails == tight, 2, 9).astype(np.int64),
                     np.ones(n - 1, np.int64), supply)


def check_deep_path(solve, diagnose):
    for stype in (O.GEQ, O.LEQ):
        p = deep_path(stype)
        verdict, violation, cut, unmet, h = one(p, stype, solve, diagnose)
        assert verdict == V.Cut and violation == 3
        assert cut == (list(range(PATH_NODES - 1)) if stype == O.GEQ else list(range(1, PATH_NODES)))
        st = h.diagnose_stats()
        assert st["levels"] == PATH_NODES - 1 and st["frontier_nodes"] == PATH_NODES - 1 and st["cut"] == 1, st
        assert st["inc_entries"] == 2 * (PATH_NODES - 1) - 1, st            # every node of S reads its own entries: all but the far end's one


def test_a_path_of_299_levels_on_the_host():
    check_deep_path(HOST_SOLVE, HOST_DIAGNOSE)


# ---- 4: the kept state is only read
def check_untouched(solve, resolve, diagnose, ranges, t=None):
    t = t or family("A")[4]
    a = t.arrays()
    new_cost = np.ascontiguousarray(a["cost"][::-1])
    for stype in (O.GEQ, O.LEQ):
        with_call, without = uniform_of(t, O.RULE_BLOCK), uniform_of(t, O.RULE_BLOCK)
        first = to_numpy(solve(with_call, a, stype))
        solve(without, a, stype)
        before = range_rows(ranges(with_call))
        stats = (with_call.stats(), with_call.range_stats(), with_call.data_range_stats(), with_call.resolve_data_stats(), with_call.start_stats())
        d = diag_rows(diagnose(with_call))
        assert len(set(d["verdict"])) >= 3                                  # feasible, cut and by its bounds at least
        again = diag_rows(diagnose(with_call))
        for name in FIELDS:
            assert np.array_equal(d[name], again[name]), name
        after = range_rows(ranges(with_call))
        for name in before:
            assert np.array_equal(before[name], after[name]), name
        now = (with_call.stats(), with_call.range_stats(), with_call.data_range_stats(), with_call.resolve_data_stats(), with_call.start_stats())
        strip = lambda s: {k: v for k, v in s.items() if not k.endswith("_ns") and not k.startswith("bytes_")}       # the first call on a device takes its table up
        for x, y in zip(stats[:1] + stats[2:], now[:1] + now[2:]):
            assert x == y
        assert strip(stats[1]) == strip(now[1])                             # the second ranges call counts what the first counted
        # a resolve afterwards makes the pivots it makes without the call
        ra, rb = to_numpy(resolve(with_call, dict(a, cost=new_cost), stype)), to_numpy(resolve(without, dict(a, cost=new_cost), stype))
        for name in ra:
            assert np.array_equal(ra[name], rb[name]), (stype, name)
        assert first["status"].shape == ra["status"].shape


def test_the_kept_state_is_untouched_on_the_host():
    check_untouched(HOST_SOLVE, lambda h, a, stype: h.rerun_on_host(supply_type=stype, **a), HOST_DIAGNOSE, lambda h: h.cost_ranges_on_host())


# ---- 5: a uniform handle equals a ragged one
def check_one_graph(solve, diagnose, t=None, stypes=(O.GEQ, O.LEQ)):
    t = t or family("A")[4]
    a = t.arrays()
    flat = FlatNodes(t.variants)
    for stype in stypes:
        for shared in (False, True):
            ua, ra = dict(a), dict(flat.arrays)
            if shared:                                                      # one supply row for all: a row that moves something
                row = next(p.supply for p in t.variants if p.supply.any())
                ua["supply"], ra["supply"] = np.ascontiguousarray(row), np.ascontiguousarray(np.tile(row, t.count))
            h, u = flat.handle(), uniform_of(t, O.RULE_BLOCK)
            solve(h, ra, stype)
            solve(u, ua, stype)
            dh, du = diag_rows(diagnose(h)), diag_rows(diagnose(u))
            assert du["side"].shape == du["unmet"].shape == (t.count, t.n) and du["verdict"].shape == (t.count,)
            assert len(set(du["verdict"])) >= 3
            for name in FIELDS:
                assert dh[name].dtype == du[name].dtype and np.array_equal(dh[name].reshape(-1), du[name].reshape(-1)), (stype, shared, name)
            assert same_counts(h.diagnose_stats(), u.diagnose_stats()), (h.diagnose_stats(), u.diagnose_stats())
            bare = diag_rows(diagnose_without_nodes(u, diagnose))
            assert bare["side"] is None and bare["unmet"] is None
            for name in FIELDS[:3]:
                assert np.array_equal(bare[name], du[name]), name
            assert same_counts(h.diagnose_stats(), u.diagnose_stats())      # without `side` the walk still runs


def diagnose_without_nodes(h, diagnose):
    return h.diagnose_on_host(nodes=False) if diagnose is HOST_DIAGNOSE else h.diagnose(nodes=False)


def test_one_graph_equals_the_uniform_batch_on_the_host():
    check_one_graph(HOST_SOLVE, HOST_DIAGNOSE)


# ---- 6: the contract
def diag_io(cls, memory=L.MEM_HOST, **arrays):
    io = cls()
    io.memory = memory
    for name, a in arrays.items():
        setattr(io, name, a.ctypes.data)
    return io


def check_contract(solve, name, host_only):
    lib = L.lib()
    t, a = small_case()
    flat = FlatNodes(t.variants)
    for handle, io_cls, arrays, nodes in ((uniform_of(t, O.RULE_BLOCK), L.UBatchDiagnoseIo, a, t.count * t.n), (flat.handle(), L.RBatchDiagnoseIo, flat.arrays, int(flat.node_rows[-1]))):
        call = getattr(lib, f"{handle._PREFIX}_{name}")
        out = dict(verdict=np.full(t.count, 7, np.int32), violation=np.full(t.count, 7, np.int64), set_size=np.full(t.count, 7, np.int32),
                   side=np.full(nodes, 7, np.int8), unmet=np.full(nodes, 7, np.int64))
        untouched = lambda: all(np.all(v == 7) for v in out.values())
        assert call(handle._h, C.byref(diag_io(io_cls, **out))) == L.ERR_STATE and untouched()
        solve(handle, arrays)
        assert call(handle._h, None) == L.ERR_INVALID and call(None, C.byref(diag_io(io_cls, **out))) == L.ERR_INVALID
        assert call(handle._h, C.byref(diag_io(io_cls, memory=5, **out))) == L.ERR_INVALID
        if host_only:
            assert call(handle._h, C.byref(diag_io(io_cls, memory=L.MEM_DEVICE, **out))) == L.ERR_INVALID
        assert untouched()
        assert call(handle._h, C.byref(diag_io(io_cls, **out))) == 0
        full = {k: v.copy() for k, v in out.items()}
        assert len(set(full["verdict"])) >= 3 and full["side"].any() and full["unmet"].any() and full["violation"].any()
        stats = L.UBatchDiagnoseStats()
        getter = getattr(lib, f"{handle._PREFIX}_get_diagnose_stats")
        assert getter(handle._h, C.byref(stats)) == 0 and stats.cut == np.sum(full["verdict"] == V.Cut) > 0 and stats.levels > 0
        counts = stats.as_dict()
        for present in ((), ("verdict",), ("violation", "set_size"), ("side",), ("unmet",), ("verdict", "unmet")):
            part = {k: np.full_like(v, 7) for k, v in out.items() if k in present}
            assert call(handle._h, C.byref(diag_io(io_cls, **part))) == 0, present
            for k, v in part.items():
                assert np.array_equal(v, full[k]), (present, k)
            assert getter(handle._h, C.byref(stats)) == 0 and same_counts(stats.as_dict(), counts), present
        assert getter(handle._h, None) == L.ERR_INVALID and getter(None, C.byref(stats)) == L.ERR_INVALID


def test_contract_on_the_host():
    check_contract(lambda h, a: h.run_on_host(**a), "diagnose_on_host", True)


def test_without_a_device_the_handle_is_unchanged(have_gpu):
    # no GPU: device 0 is missing; with one, device 99 is
    t, a = small_case()
    u = uniform_of(t, O.RULE_BLOCK, device=99 if have_gpu else 0)
    r = u.run_on_host(**a)
    before, stats, diag_stats = u.diagnose_on_host(), u.stats(), u.diagnose_stats()
    with pytest.raises(M.McfError) as ei:
        u.diagnose(tensors=False)
    assert ei.value.code == L.ERR_NO_DEVICE
    assert u.stats() == stats and u.diagnose_stats() == diag_stats
    assert_same_diagnosis(u.diagnose_on_host(), before)
    again = u.rerun_on_host(**a)
    assert np.array_equal(again.flows, r.flows) and np.array_equal(again.status, r.status)


def test_diagnose_structs_have_the_layout_of_the_header(tmp_path):
    src = tmp_path / "sz.c"
    io_fields = ("memory", "verdict", "violation", "set_size", "side", "unmet")
    s_fields = tuple(name for name, _ in L.UBatchDiagnoseStats._fields_)
    line = lambda struct, fields: 'printf("%zu' + " %zu" * len(fields) + '\\n", sizeof(%s)' % struct + "".join(", offsetof(%s, %s)" % (struct, f) for f in fields) + ");"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void){' % os.path.join(ROOT, "include", "mcf_hip.h")
                   + line("mcf_ubatch_diagnose_io", io_fields) + line("mcf_rbatch_diagnose_io", io_fields) + line("mcf_ubatch_diagnose_stats", s_fields)
                   + 'printf("%d %d %d %d %d\\n", MCF_DIAG_NONE, MCF_DIAG_FEASIBLE, MCF_DIAG_CUT, MCF_DIAG_OPEN, MCF_DIAG_BOUNDS);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", str(src), "-o", str(exe)])
    got = [[int(x) for x in row.split()] for row in subprocess.check_output([str(exe)]).decode().splitlines()]
    for cls, fields, row in zip((L.UBatchDiagnoseIo, L.RBatchDiagnoseIo, L.UBatchDiagnoseStats), (io_fields, io_fields, s_fields), got):
        assert row == [C.sizeof(cls)] + [getattr(cls, f).offset for f in fields], cls
    assert got[3] == [V.NoVerdict, V.Feasible, V.Cut, V.Open, V.Bounds] == [0, 1, 2, 3, 4]


def test_the_certificate_oracle_on_cuts_it_must_refuse():
    """check_cut is the judge: it must refuse a wrong sum, a cut that is not violated, and an uncapacitated arc in the bounding direction"""
    p = problem(3, [(0, 1, 0, 3, 1), (1, 2, 1, None, 1)], [5, 0, -5])
    K.check_cut(p, O.GEQ, [1, 0, 0], 2)
    for side, violation in (([1, 0, 0], 3), ([1, 1, 0], 5), ([0, 1, 0], 1), ([1, 1, 1], 0)):
        with pytest.raises(AssertionError):
            K.check_cut(p, O.GEQ, side, violation)
    assert K.feasible(p, O.GEQ) is False and K.feasible(problem(3, [(0, 1, 0, 5, 1), (1, 2, 1, None, 1)], [5, 0, -5]), O.GEQ) is True
    assert K.feasible(problem(2, [(0, 1, 3, 2, 1)], [0, 0]), O.GEQ) is None


# ---- 7: cost ranges, data ranges and diagnosis share one handle: one driver, one summary buffer, a plan and statistics each
QUERIES = ("cost_ranges", "data_ranges", "diagnose")
QUERY_STATS = dict(cost_ranges="range_stats", data_ranges="data_range_stats", diagnose="diagnose_stats")
QUERY_COUNTS = dict(cost_ranges=("instances", "ranged", "tree_arcs", "cycle_hops"), data_ranges=("instances", "ranged", "walks", "hops"), diagnose=COUNTS)
QUERY_WORDS = dict(cost_ranges=3, data_ranges=3, diagnose=8)       # summary words: up zeroed and down with every device call
SLOT_BYTES = 104 + C.sizeof(L.BlockConfig)                          # BatchSlot of csrc/batch_layout.hip.h, which has no padding


def query_rows(result):
    get = lambda a: a if isinstance(a, np.ndarray) else a.cpu().numpy()
    return {name: get(getattr(result, name)) for name, _, _ in type(result).FIELDS}


def check_three_queries_on_one_handle(solve, resolve, device_calls, rounds):
    """The two-tier ragged batch of test_data_ranges_host.py, solved once per handle, then the three queries in each of their six orders,
    `rounds` times over.  device_calls: call k of a handle runs on the device (tensors: only the summary words, the query's table of
    instances and the kept state cross the bus in the library) when k plus the order's number is even, and is the hook otherwise, so
    that the state moves between every two calls; without it every call is the hook.  Every row and every count must be the hook's on a
    second handle freshly solved; the table of instances goes up with a query's first device call on the handle and never again,
    whatever ran before; stats() and a resolve() afterwards are what they are without any query."""
    flat, graphs, graph_of, pair_lists = two_tiers()
    a, count = flat.arrays, flat.count
    fresh = lambda: M.RaggedBatch(graphs, graph_of=graph_of, rule=RULES[O.RULE_BLOCK])
    hook = lambda h, q: h.data_ranges_on_host(pairs=pair_lists) if q == "data_ranges" else getattr(h, q + "_on_host")()
    on_device = lambda h, q: h.data_ranges(pairs=pair_lists, tensors=True) if q == "data_ranges" else getattr(h, q)(tensors=True)
    stats_of = lambda h, q: getattr(h, QUERY_STATS[q])()
    strip = lambda s: {k: v for k, v in s.items() if not k.endswith("_ns") and not k.startswith("bytes_")}
    new_cost = dict(a, cost=np.ascontiguousarray(a["cost"] + np.arange(len(a["cost"])) % 3))

    ref = fresh()
    HOST_SOLVE(ref, a, O.GEQ)
    want = {q: (query_rows(hook(ref, q)), stats_of(ref, q)) for q in QUERIES}
    assert want["cost_ranges"][1]["ranged"] >= 20 and want["data_ranges"][1]["walks"] > 0 and want["diagnose"][1]["instances"] == count == 24
    plain = fresh()                                                         # never queried
    solve(plain, a, O.GEQ)
    plain_stats = strip(plain.stats())
    plain_rows = to_numpy(resolve(plain, new_cost, O.GEQ))
    plain_after = strip(plain.stats())

    for number, order in enumerate(itertools.permutations(QUERIES)):
        h = fresh()
        solve(h, a, O.GEQ)
        solved = h.stats()
        state_bytes = solved["workspace_bytes"] + count * SLOT_BYTES
        state_on_host = not device_calls
        table_is_up = set()
        for k, q in enumerate(order * rounds):
            what = (order, k, q)
            if device_calls and (k + number) % 2 == 0:
                rows, st = query_rows(on_device(h, q)), stats_of(h, q)
                assert st["lds_instances"] == 16 and st["global_instances"] == 8, (what, st)
                up = 8 * QUERY_WORDS[q] + (0 if q in table_is_up else 4 * count) + (state_bytes if state_on_host else 0)
                assert st["bytes_up"] == up and st["bytes_down"] == 8 * QUERY_WORDS[q], (what, st, up)
                table_is_up.add(q)
                state_on_host = False
            else:
                rows, st = query_rows(hook(h, q)), stats_of(h, q)
                assert st["lds_instances"] == st["global_instances"] == st["bytes_up"] == st["bytes_down"] == 0, (what, st)
                state_on_host = True
            for name, row in want[q][0].items():
                assert rows[name].dtype == row.dtype and np.array_equal(rows[name], row), (what, name)
            assert all(st[f] == want[q][1][f] for f in QUERY_COUNTS[q]), (what, st, want[q][1])
            for other in QUERIES:                                           # a call replaces its own query's statistics and no other's
                if other not in order[:k + 1]:
                    assert stats_of(h, other)["instances"] == 0, (what, other)
        assert h.stats() == solved and strip(solved) == plain_stats, order
        assert not any(h.resolve_data_stats().values()) and not any(h.start_stats().values()), order
        rows = to_numpy(resolve(h, new_cost, O.GEQ))
        for name in plain_rows:
            assert np.array_equal(rows[name], plain_rows[name]), (order, name)
        assert strip(h.stats()) == plain_after, order


def test_three_queries_share_one_handle_on_the_host():
    check_three_queries_on_one_handle(HOST_SOLVE, lambda h, a, stype: h.rerun_on_host(supply_type=stype, **a), False, 2)
