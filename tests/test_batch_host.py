"""The batch solver (mcf_batch_*) without a GPU: mcf_batch_run_on_host runs the kernel's own pivot code
(csrc/batch_step.hip.h) with one lane on the CPU, so everything but the launch machinery is checked here.

The reference is the CPU oracle in SEM_CSHARP.  For Block Search the batch runs what `new NetworkSimplex(g).Solve()` runs -- the
auto-configured, adaptive rule -- so the oracle is built with auto_config=True (the oracle's own default is the bare `new
OptimizationConfig()`); the configuration does not touch the other two rules."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import mincostflow_amd as M
from mincostflow_amd import _lib as L
from oracle import ns_oracle as O

from adversarial import adversarial_batch
from helpers import fixtures, load, problem_from_dict
from kat_data import CSHARP_KATS, LEMON_TABLE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RULES = {O.RULE_FIRST: M.PivotRule.FirstEligible, O.RULE_BEST: M.PivotRule.BestEligible, O.RULE_BLOCK: M.PivotRule.BlockSearch}
TRACE = 1 << 18          # above every fixture's pivot count (the largest: 124 916)
OVERSIZE = {"netgen_8_14a", "transport_400x300"}                     # above MCF_BATCH_MAX_ARCS
SLOW_FIRST_ELIGIBLE = {"circulation_1000_0_05", "netgen_8_13a"}      # above 30 000 arcs: minutes on one core


def oracle_of(p, rule, supply_type=O.GEQ, trace_cap=TRACE):
    o = O.Oracle(p, O.SEM_CSHARP, rule, supply_type=supply_type, auto_config=True)
    st, tr = o.solve(trace_cap=trace_cap)
    return o, st, tr


def assert_equals_oracle(b, i, o, st, tr, what=""):
    assert b.status(i) == st, (what, b.status(i), st)
    assert b.pivots(i) == o.n_pivots, (what, b.pivots(i), o.n_pivots)
    assert np.array_equal(b.trace(i), tr), what
    if st == O.OPTIMAL:
        assert b.total_cost(i) == o.total_cost, what
        assert np.array_equal(b.flows(i), o.flow()), what
        assert np.array_equal(b.potentials(i), o.potential()), what
    else:
        for getter in (b.total_cost, b.flows, b.potentials):             # "Solution not optimal", as mcf_ns_get_*
            with pytest.raises(M.McfError) as ei:
                getter(i)
            assert ei.value.code == L.ERR_STATE


def mixed_cases():
    """[(name, problem, supply type, recorded status or None, recorded cost or None, recorded flows or None)]: the reference's known answers,
    the LEMON table and the degenerate graphs of test_degenerate_graphs -- infeasible, unbounded and optimal next to each other."""
    out = []
    for name, d, st, cost, flows in CSHARP_KATS:
        out.append((name, problem_from_dict(d), O.GEQ, st, cost, flows))
    for cid, d, stype, _, _ in LEMON_TABLE:
        out.append((f"lemon_{cid}", problem_from_dict(d), stype, None, None, None))
    none = np.zeros(0, np.int32)
    none64 = np.zeros(0, np.int64)
    out.append(("no_arcs_balanced", O.Problem(3, 0, none, none, none64, none64, none64, [0, 0, 0]), O.GEQ, 1, 0, None))
    out.append(("no_arcs_unconnected", O.Problem(2, 0, none, none, none64, none64, none64, [1, -1]), O.GEQ, 2, None, None))
    out.append(("self_loop_and_parallel", O.Problem(2, 4, [0, 0, 0, 1], [1, 1, 0, 1], [0] * 4, [5, 5, 9, 9], [3, 2, -1, 4], [7, -7]), O.GEQ, None, None, None))
    # The C# semantics answers Unbounded only through NS.cs:321-325 (no blocking arc and delta == 0; it answers Optimal on LEMON's two
    # unbounded networks, difference D7): an eligible arc of capacity 0 whose cycle nothing blocks.
    out.append(("zero_capacity_unblocked", O.Problem(2, 1, [0], [1], [0], [0], [-5], [0, -3]), O.GEQ, 3, None, None))
    return out


def check_mixed_batch(b, cases, rule):
    """b holds `cases` in order and has been solved."""
    seen = set()
    for i, (name, p, stype, st_rec, cost_rec, flows_rec) in enumerate(cases):
        o, st, tr = oracle_of(p, rule, stype)
        assert_equals_oracle(b, i, o, st, tr, name)
        if st_rec is not None:
            assert b.status(i) == st_rec, name
        if cost_rec is not None:
            assert b.total_cost(i) == cost_rec, name
        if flows_rec is not None:
            assert list(b.flows(i)) == flows_rec, name
        seen.add(b.status(i))
    assert {M.SolverStatus.Optimal, M.SolverStatus.Infeasible, M.SolverStatus.Unbounded} <= seen


def generated(seed, nodes=200, arcs=600):
    g = M.netgen_like(seed, nodes, arcs, max(2, nodes // 50), max(2, nodes // 50))
    return O.Problem(g.node_count, g.arc_count, g.source, g.target, g.lower, g.upper, g.cost, g.supply)


# ---- the adversarial fuzz (tests/adversarial.py): the batch, and per rule the oracle's answers, computed once and left unchanged
FUZZ_TRACE = 2048        # above the longest solve of the batch (asserted in fuzz_reference)


@functools.lru_cache(maxsize=None)
def fuzz_cases():
    return tuple(adversarial_batch())


def bound_infeasible(p):
    return bool(np.any(p.upper < p.lower))


@functools.lru_cache(maxsize=None)
def fuzz_reference(rule):
    """((oracle, status, trace) per instance of fuzz_cases()).  Everything the fuzz needs of its reference is asserted here, on the oracle's
    answers alone: its numbers did not overflow, the traces are whole, and the batch holds what it was built for -- above one stride of
    the wave (m + n > 64) at least 10 Optimal, 10 Infeasible and 10 Unbounded, 5 of each with costs above 2^32, and at least 3 instances
    infeasible by their bounds between neighbours that run on the device."""
    cases = fuzz_cases()
    refs = tuple(oracle_of(p, rule, stype, trace_cap=FUZZ_TRACE) for p, stype in cases)
    count = {st: [0, 0] for st in (O.OPTIMAL, O.INFEASIBLE, O.UNBOUNDED)}          # status -> [above one stride, of these with 64-bit costs]
    by_bounds = []
    for k, ((p, _), (o, st, tr)) in enumerate(zip(cases, refs)):
        assert st in count and o.n_pivots < FUZZ_TRACE and len(tr) == o.n_pivots, k
        if st == O.OPTIMAL:
            assert o.total_cost == sum(int(f) * int(c) for f, c in zip(o.flow(), p.cost)), k
            assert max((abs(int(v)) for v in o.potential()), default=0) < 1 << 62, k
        if bound_infeasible(p):
            assert st == O.INFEASIBLE and o.n_pivots == 0, k
            by_bounds.append(k)
        if p.m + p.n > 64:
            count[st][0] += 1
            count[st][1] += int(np.abs(p.cost).max() > 1 << 32)
    print(f"fuzz, rule {rule}: {len(cases)} instances, longest solve {max(o.n_pivots for o, _, _ in refs)} pivots; above 64 search arcs (of these with 64-bit costs): "
          f"Optimal {count[O.OPTIMAL]}, Infeasible {count[O.INFEASIBLE]}, Unbounded {count[O.UNBOUNDED]}; infeasible by bounds: {by_bounds}")
    assert len(cases) < 500 and max(p.m for p, _ in cases) <= 1000
    for st, (above, wide) in count.items():
        assert above >= 10 and wide >= 5, (st, above, wide)
    assert len(by_bounds) >= 3
    for k in by_bounds:
        assert 0 < k < len(cases) - 1 and not bound_infeasible(cases[k - 1][0]) and not bound_infeasible(cases[k + 1][0]), k
    return refs


def fuzz_solver(rule, **kw):
    b = M.BatchSolver(rule=RULES[rule], record_trace=FUZZ_TRACE, **kw)
    for k, (p, stype) in enumerate(fuzz_cases()):
        assert b.add(p, supply_type=stype) == k
    return b


def assert_fuzz_equals_oracle(b, rule):
    """Every instance, none left out."""
    refs = fuzz_reference(rule)
    compared = 0
    for k, (o, st, tr) in enumerate(refs):
        assert_equals_oracle(b, k, o, st, tr, f"fuzz instance {k}")
        compared += 1
    assert compared == len(fuzz_cases()) == len(b)


# ---- the workspace of DESIGN.md 3.14, restated: 15 arrays in the documented order, each rounded up to 16 bytes
LDS_LIMITS = (160 << 10, 64 << 10)       # the MI355X's figure; the default limit that holds where the opt-in above it is refused
LDS_DIVISORS = (16, 8, 4, 3, 2, 1)


def footprint(A, N):
    up16 = lambda b: (b + 15) // 16 * 16
    constant = [4 * A, 4 * A, 8 * A, 8 * A]                                        # tail, head i32 | cost, upper i64
    changing = [8 * A, 8 * N] + 6 * [4 * N] + [4 * (N + 1), A, N]                  # flow, pi i64 | par, par_arc, nxt, prv, sub, fin i32 | scratch[N + 1] i32 | state, par_dir i8
    assert len(constant + changing) == 15
    total = sum(up16(b) for b in constant + changing)
    assert 0 <= total - (33 * A + 37 * N + 4) <= 15 * 15
    return total


def footprint_of(p, supply_type=O.GEQ):
    """A = the m arcs, the n root links and one artificial arc per node that cannot hang on its root link: supply (after the lower bounds
    have been moved into it) > 0 under GEQ, < 0 under LEQ (start_basis)."""
    if bound_infeasible(p):
        return 0                                                                   # never set up: no workspace
    s = p.supply.copy()
    np.subtract.at(s, p.src, p.lower)
    np.add.at(s, p.tgt, p.lower)
    hung = int(np.sum(s > 0) if supply_type == O.GEQ else np.sum(s < 0))
    return footprint(p.m + p.n + hung, p.n + 1)


@functools.lru_cache(maxsize=None)
def ladder():
    """((problem, footprint, limit, fits) ...): for every class limit L / d the generated() instance with the last arc count whose workspace
    fits and the one with the first that does not.  400 nodes where such an arc count exists (generated() needs nodes - sources arcs
    for its skeleton: 41 344 bytes at 400 nodes), 30 nodes for the limits below that."""
    out = []
    for L in LDS_LIMITS:
        for d in LDS_DIVISORS:
            limit = L // d
            for n in (400, 30):
                sources = max(2, n // 50)                                          # generated(): each with a positive supply, so each on an artificial arc
                size = lambda m: footprint(m + n + sources, n + 1)
                m = n - sources
                if size(m) <= limit:
                    break
            assert size(m) <= limit, (limit, "below the smallest workspace of both families")
            while size(m + 1) <= limit:
                m += 1
            for arcs, fits in ((m, True), (m + 1, False)):
                p = generated(5000 + len(out), n, arcs)
                assert footprint_of(p) == size(arcs) and (size(arcs) <= limit) == fits
                out.append((p, size(arcs), limit, fits))
    assert len(out) == 24 and sum(p.n == 400 for p, *_ in out) >= 8 and max(p.m for p, *_ in out) < 5000
    return tuple(out)


PADDED_NODES = 4500      # 37 bytes per node: above the larger of LDS_LIMITS whatever the arcs


@functools.lru_cache(maxsize=None)
def padded_fuzz(rule):
    """((problem, supply type, (oracle, status, trace)) ...): fuzz instances above one stride with isolated zero-supply nodes appended up
    to PADDED_NODES, so that the workspace fits no LDS limit and the solve runs in place in global memory.  Still valid input with a
    defined answer; the root links of the added nodes join the search range.  The six largest instances per status of the unpadded reference, half
    of them with 64-bit costs; what is asserted is what the oracle answers on the padded ones: every status at least twice, once with
    costs above 2^32, and a LEQ instance among them."""
    picked = {st: [[], []] for st in (O.OPTIMAL, O.INFEASIBLE, O.UNBOUNDED)}
    for (p, stype), (o, st, _) in reversed(list(zip(fuzz_cases(), fuzz_reference(rule)))):          # the largest first
        if p.m + p.n <= 64 or bound_infeasible(p):
            continue
        wide = int(np.abs(p.cost).max() > 1 << 32)
        if len(picked[st][wide]) < 3:
            picked[st][wide].append((p, stype))
    out = []
    seen = {st: [0, 0] for st in picked}
    for p, stype in (c for st in picked for half in picked[st] for c in half):
        q = O.Problem(PADDED_NODES, p.m, p.src, p.tgt, p.lower, p.upper, p.cost, np.concatenate([p.supply, np.zeros(PADDED_NODES - p.n, np.int64)]))
        assert footprint_of(q, stype) > max(LDS_LIMITS)
        o, st, tr = oracle_of(q, rule, stype, trace_cap=1 << 14)
        assert o.n_pivots < 1 << 14
        if st == O.OPTIMAL:
            assert o.total_cost == sum(int(f) * int(c) for f, c in zip(o.flow(), q.cost))
            assert max(abs(int(v)) for v in o.potential()) < 1 << 62
        seen[st][0] += 1
        seen[st][1] += int(np.abs(q.cost).max() > 1 << 32)
        out.append((q, stype, (o, st, tr)))
    print(f"padded fuzz, rule {rule}: {len(out)} instances, status -> [count, with 64-bit costs] {seen}, longest solve {max(r[0].n_pivots for _, _, r in out)} pivots")
    assert len(out) == 18 and all(n >= 2 and wide >= 1 for n, wide in seen.values()), seen
    assert any(stype == O.LEQ for _, stype, _ in out)
    return tuple(out)


def check_padded_fuzz(run, rule, **kw):
    b = M.BatchSolver(rule=RULES[rule], record_trace=1 << 14, **kw)
    for q, stype, _ in padded_fuzz(rule):
        b.add(q, supply_type=stype)
    run(b)
    for i, (_, _, (o, st, tr)) in enumerate(padded_fuzz(rule)):
        assert_equals_oracle(b, i, o, st, tr, f"padded fuzz instance {i}")
    return b


# ---- 1
@pytest.mark.parametrize("rule", [O.RULE_BLOCK, O.RULE_BEST, O.RULE_FIRST])
@pytest.mark.parametrize("name,path,want", fixtures(), ids=[f[0] for f in fixtures()])
def test_run_on_host_equals_the_oracle_on_every_fixture(name, path, want, rule):
    p = load(path)
    b = M.BatchSolver(rule=RULES[rule], record_trace=TRACE)
    if name in OVERSIZE:
        assert p.m > L.BATCH_MAX_ARCS
        with pytest.raises(M.McfError) as ei:
            b.add(p)
        assert ei.value.code == L.ERR_INVALID and "mcf_ns_solve" in str(ei.value)
        return
    if rule == O.RULE_FIRST and name in SLOW_FIRST_ELIGIBLE:
        assert p.m > 30000
        return      # left out on purpose (minutes on the CPU); the only two
    i = b.add(p)
    b.run_on_host()
    o, st, tr = oracle_of(p, rule)
    assert st == O.OPTIMAL
    assert_equals_oracle(b, i, o, st, tr, name)
    if want is not None:
        assert b.total_cost(i) == want


def test_the_fixture_matrix_is_complete():
    names = {f[0] for f in fixtures()}
    assert len(names) == 39 and OVERSIZE <= names and SLOW_FIRST_ELIGIBLE <= names


# ---- 2
@pytest.mark.parametrize("rule", [O.RULE_BLOCK, O.RULE_BEST, O.RULE_FIRST])
def test_known_answers_in_one_mixed_batch(rule):
    cases = mixed_cases()
    b = M.BatchSolver(rule=RULES[rule], record_trace=4096)
    for k, (_, p, stype, *_rest) in enumerate(cases):
        assert b.add(p, supply_type=stype) == k
    b.run_on_host()
    check_mixed_batch(b, cases, rule)
    st = b.stats()
    assert st["instances"] == len(cases) and st["total_pivots"] == sum(b.pivots(i) for i in range(len(cases)))


# ---- 3
def test_results_do_not_depend_on_the_composition_of_the_batch():
    p = generated(7)
    others = [generated(100 + k, 60 + 3 * k, 200 + 7 * k) for k in range(49)]
    alone = M.BatchSolver(record_trace=1 << 14)
    alone.add(p)
    alone.run_on_host()
    first = M.BatchSolver(record_trace=1 << 14)
    first.add(p)
    for q in others:
        first.add(q)
    first.run_on_host()
    last = M.BatchSolver(record_trace=1 << 14)
    for q in others:
        last.add(q)
    k = last.add(p)
    last.run_on_host()
    assert k == 49 and alone.pivots(0) > 100
    for b, i in ((first, 0), (last, 49)):
        assert b.status(i) == alone.status(0) == M.SolverStatus.Optimal
        assert np.array_equal(b.trace(i), alone.trace(0))
        assert np.array_equal(b.flows(i), alone.flows(0)) and np.array_equal(b.potentials(i), alone.potentials(0))


# ---- 4
@pytest.mark.parametrize("rule", [O.RULE_BLOCK, O.RULE_BEST, O.RULE_FIRST])
def test_pivot_limit(rule):
    p = generated(11)
    full = M.BatchSolver(rule=RULES[rule], record_trace=1 << 14)
    full.add(p)
    full.run_on_host()
    total = full.pivots(0)
    assert full.status(0) == M.SolverStatus.Optimal and total > 50
    for k in (1, 17, total - 1):
        b = M.BatchSolver(rule=RULES[rule], pivot_limit=k, record_trace=1 << 14)
        b.add(p)
        b.add(load("transport_2x3"))                 # finishes well inside the limit... except k = 1
        b.run_on_host()
        assert b.status(0) == M.SolverStatus.NotSolved and b.pivots(0) == k
        assert np.array_equal(b.trace(0), full.trace(0)[:k])
        assert b.status(1) == (M.SolverStatus.Optimal if k >= 6 else M.SolverStatus.NotSolved)
    # a limit of exactly the pivot count is not hit: the search after the last pivot finds nothing
    b = M.BatchSolver(rule=RULES[rule], pivot_limit=total, record_trace=1 << 14)
    b.add(p)
    b.run_on_host()
    assert b.status(0) == M.SolverStatus.Optimal and b.pivots(0) == total
    # the default: 64 * (m + 2 n) + 1024, far above any fixture's count
    assert total < 64 * (p.m + 2 * p.n) + 1024


# ---- 5
def test_argument_and_order_errors(have_gpu):
    lib = L.lib()
    p = load("transport_2x3")
    h = C.c_void_p()
    d = L.BatchDesc(0, L.RULE_BLOCK_SEARCH, L.SEM_PLAIN, 0, 0, 0, 0, 0)
    assert lib.mcf_batch_create(None, C.byref(d)) == L.ERR_INVALID
    assert lib.mcf_batch_create(C.byref(h), None) == L.ERR_INVALID
    lib.mcf_batch_destroy(None)
    # refused rules / semantics / sharding, each with a message that says so
    for kw, word in ((dict(rule=M.PivotRule.CandidateList), "list rules"), (dict(rule=M.PivotRule.AlteringList), "list rules"), (dict(rule=9), "pivot rule"),
                     (dict(semantics=L.SEM_OPTIMIZED), "MCF_SEM_OPTIMIZED"), (dict(flags=L.BATCH_SHARDED), "sharding"), (dict(pivot_limit=-1), "negative"),
                     (dict(record_trace=-1), "negative")):
        with pytest.raises(M.McfError) as ei:
            M.BatchSolver(**kw)
        assert ei.value.code == L.ERR_INVALID and word in str(ei.value), kw
    b = M.BatchSolver(record_trace=64)
    keep = []

    def i32(a):
        keep.append(np.ascontiguousarray(a, np.int32))      # the pointer must outlive the call
        return keep[-1].ctypes.data
    # null arguments and bad graphs
    assert lib.mcf_batch_add(None, 2, 1, i32([0]), i32([1]), None, None, None, None, 0, None) == L.ERR_INVALID
    assert lib.mcf_batch_add(b._h, 2, 1, None, None, None, None, None, None, 0, None) == L.ERR_INVALID
    assert lib.mcf_batch_add(b._h, -1, 0, None, None, None, None, None, None, 0, None) == L.ERR_INVALID
    assert lib.mcf_batch_add(b._h, 2, 1, i32([0]), i32([2]), None, None, None, None, 0, None) == L.ERR_INVALID       # end point out of range
    assert lib.mcf_batch_add(b._h, 2, 1, i32([-1]), i32([1]), None, None, None, None, 0, None) == L.ERR_INVALID
    assert lib.mcf_batch_add(b._h, 2, 1, i32([0]), i32([1]), None, None, None, None, 7, None) == L.ERR_INVALID       # supply type
    # oversize: arcs, nodes
    big = np.zeros(L.BATCH_MAX_ARCS + 1, np.int32)
    assert lib.mcf_batch_add(b._h, 2, L.BATCH_MAX_ARCS + 1, big.ctypes.data, big.ctypes.data, None, None, None, None, 0, None) == L.ERR_INVALID
    assert b"mcf_ns_solve" in lib.mcf_last_error()
    assert lib.mcf_batch_add(b._h, L.BATCH_MAX_NODES + 1, 0, None, None, None, None, None, None, 0, None) == L.ERR_INVALID
    assert len(b) == 0 and b.stats()["instances"] == 0
    # all-default arrays are accepted (0 / unbounded / 0 / 0)
    idx = C.c_int32(-1)
    assert lib.mcf_batch_add(b._h, 2, 1, i32([0]), i32([1]), None, None, None, None, 0, C.byref(idx)) == 0 and idx.value == 0
    b._problems.append((2, 1))
    assert b.add(p) == 1
    # getters before a solve; index out of range
    st, v, n = C.c_int32(), C.c_int64(), C.c_int64()
    out = np.zeros(16, np.int64)
    assert lib.mcf_batch_get_status(b._h, 0, C.byref(st)) == L.ERR_STATE
    assert lib.mcf_batch_get_total_cost(b._h, 0, C.byref(v)) == L.ERR_STATE
    assert lib.mcf_batch_get_flows(b._h, 0, out.ctypes.data) == L.ERR_STATE
    assert lib.mcf_batch_get_potentials(b._h, 0, out.ctypes.data) == L.ERR_STATE
    assert lib.mcf_batch_get_pivots(b._h, 0, C.byref(v)) == L.ERR_STATE
    assert lib.mcf_batch_get_trace(b._h, 0, None, 0, C.byref(n)) == L.ERR_STATE
    assert lib.mcf_batch_get_status(b._h, 2, C.byref(st)) == L.ERR_INVALID
    assert lib.mcf_batch_get_status(b._h, -1, C.byref(st)) == L.ERR_INVALID
    assert lib.mcf_batch_get_stats(b._h, None) == L.ERR_INVALID and lib.mcf_batch_get_stats(None, C.byref(L.BatchStats())) == L.ERR_INVALID
    assert lib.mcf_batch_solve(None) == L.ERR_INVALID and lib.mcf_batch_run_on_host(None) == L.ERR_INVALID
    # no device: the solver proper refuses, the hook is no way round it for mcf_ns_solve (test_no_cpu_search_path_without_device)
    if not have_gpu:
        with pytest.raises(M.McfError) as ei:
            b.solve()
        assert ei.value.code == L.ERR_NO_DEVICE
    b.run_on_host()
    assert b.status(0) == M.SolverStatus.Optimal and b.status(1) == M.SolverStatus.Optimal
    for bad in (2, -1, 1 << 20):
        for getter in (b.status, b.total_cost, b.flows, b.potentials, b.pivots, b.trace):
            with pytest.raises(M.McfError) as ei:
                getter(bad)
            assert ei.value.code == L.ERR_INVALID
    assert lib.mcf_batch_get_status(b._h, 0, None) == L.ERR_INVALID and lib.mcf_batch_get_flows(b._h, 0, None) == L.ERR_INVALID
    assert lib.mcf_batch_get_trace(b._h, 1, None, 4, C.byref(n)) == L.ERR_INVALID and lib.mcf_batch_get_trace(b._h, 1, None, 0, None) == L.ERR_INVALID
    # single-shot, like Solve(); nothing is added to a solved batch
    for again in (b.run_on_host, b.solve, lambda: b.add(p)):
        with pytest.raises(M.McfError) as ei:
            again()
        assert ei.value.code == L.ERR_STATE
    # a short trace buffer gets the first entries, the length is the recorded one
    short = np.zeros(2, np.int32)
    assert lib.mcf_batch_get_trace(b._h, 1, short.ctypes.data, 2, C.byref(n)) == 0 and n.value == b.pivots(1) > 2
    assert np.array_equal(short, b.trace(1)[:2])


@pytest.mark.skipif(M.device_count() > 0, reason="a GPU is present")
def test_batch_solve_without_a_device():
    b = M.BatchSolver()
    b.add(load("transport_2x3"))
    with pytest.raises(M.McfError) as ei:
        b.solve()
    assert ei.value.code == L.ERR_NO_DEVICE
    b.run_on_host()                       # the refused call left the batch unsolved
    assert b.status(0) == M.SolverStatus.Optimal


# ---- 6
def test_batch_structs_have_the_layout_of_the_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void){printf("%%zu %%zu %%zu %%zu %%zu\\n", sizeof(mcf_batch_desc), sizeof(mcf_batch_stats),'
                   ' offsetof(mcf_batch_desc, pivot_limit), offsetof(mcf_batch_desc, flags), offsetof(mcf_batch_stats, kernel_ns));return 0;}\n'
                   % os.path.join(ROOT, "include", "mcf_hip.h"))
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(L.BatchDesc), C.sizeof(L.BatchStats), L.BatchDesc.pivot_limit.offset, L.BatchDesc.flags.offset, L.BatchStats.kernel_ns.offset]
    header = open(os.path.join(ROOT, "include", "mcf_hip.h")).read()
    for name, value in (("MCF_BATCH_MAX_ARCS", L.BATCH_MAX_ARCS), ("MCF_BATCH_MAX_NODES", L.BATCH_MAX_NODES), ("MCF_BATCH_MAX_INSTANCES", L.BATCH_MAX_INSTANCES)):
        assert f"#define {name} {value}" in header


# ---- 13
@pytest.mark.parametrize("rule", [O.RULE_BLOCK, O.RULE_BEST, O.RULE_FIRST])
def test_adversarial_batch_on_the_host(rule):
    """All outcomes at every search-range size round the wave's strides, 64-bit costs, ties, LEQ, lower bounds, infinite and zero
    capacities (tests/adversarial.py): the pivot code with one lane equals the oracle on every instance."""
    b = fuzz_solver(rule).run_on_host()
    assert_fuzz_equals_oracle(b, rule)
    assert b.stats()["total_pivots"] == sum(o.n_pivots for o, _, _ in fuzz_reference(rule))
    check_padded_fuzz(lambda q: q.run_on_host(), rule)


# ---- 14
def test_the_ladder_straddles_every_class_limit():
    steps = ladder()
    assert {limit for _, _, limit, _ in steps} == {L // d for L in LDS_LIMITS for d in LDS_DIVISORS}
    for (p, size, limit, fits), (q, size_q, limit_q, fits_q) in zip(steps[::2], steps[1::2]):
        assert limit == limit_q and fits and not fits_q and q.m == p.m + 1 and q.n == p.n
        assert size <= limit < size_q
    for L in LDS_LIMITS:                                   # the tier edge itself is made of the 400-node family
        assert [p.n for p, _, limit, _ in steps if limit == L] == [400, 400]


def short_trace_problems():
    return [generated(21), generated(22, 120, 500), generated(23, 260, 700)]


def check_short_and_absent_traces(run, **kw):
    """run: BatchSolver -> solved BatchSolver.  Half of the smallest pivot count as the capacity: every trace is the prefix of its own full
    trace (nobody's pivots are recorded in a neighbour's), the pivot counts are the full ones; capacity 0: no trace, the same solve."""
    problems = short_trace_problems()
    full = M.BatchSolver(record_trace=1 << 13)
    for p in problems:
        full.add(p)
    full.run_on_host()
    counts = [full.pivots(i) for i in range(3)]
    assert all(full.status(i) == M.SolverStatus.Optimal and 100 < counts[i] < 1 << 13 for i in range(3)) and len(set(counts)) == 3
    for cap in (min(counts) // 2, 0):
        b = M.BatchSolver(record_trace=cap, **kw)
        for p in problems:
            b.add(p)
        run(b)
        for i in range(3):
            assert b.status(i) == M.SolverStatus.Optimal and b.pivots(i) == counts[i], (cap, i)
            assert len(b.trace(i)) == cap and np.array_equal(b.trace(i), full.trace(i)[:cap]), (cap, i)
            assert b.total_cost(i) == full.total_cost(i), (cap, i)
            assert np.array_equal(b.flows(i), full.flows(i)) and np.array_equal(b.potentials(i), full.potentials(i)), (cap, i)
        assert b.stats()["total_pivots"] == sum(counts)
    return full


# ---- 15
def test_short_and_absent_traces_on_the_host():
    check_short_and_absent_traces(lambda b: b.run_on_host())


def only_bound_infeasible():
    """Valid input with a defined answer: Infeasible by an arc whose upper bound is below its lower bound (NS.cs:227-231)."""
    p = load("transport_2x3")
    q = generated(31, 60, 200)
    out = []
    for base, arc in ((p, 0), (q, 17), (p, p.m - 1)):
        upper = base.upper.copy()
        upper[arc] = base.lower[arc] - 1
        out.append(O.Problem(base.n, base.m, base.src, base.tgt, base.lower, upper, base.cost, base.supply))
    return out


def check_nothing_to_run(run):
    b = M.BatchSolver(record_trace=64)
    run(b)
    st = b.stats()
    assert len(b) == 0 and st["instances"] == 0 and st["launches"] == 0 and st["workspace_bytes"] == 0 and st["total_pivots"] == 0
    assert st["lds_instances"] == 0 and st["global_instances"] == 0
    with pytest.raises(M.McfError) as ei:
        b.status(0)
    assert ei.value.code == L.ERR_INVALID
    b = M.BatchSolver(record_trace=64)
    problems = only_bound_infeasible()
    for p in problems:
        b.add(p)
    run(b)
    st = b.stats()
    assert st["instances"] == 3 and st["launches"] == 0 and st["workspace_bytes"] == 0 and st["total_pivots"] == 0
    assert st["lds_instances"] == 0 and st["global_instances"] == 0
    for i, p in enumerate(problems):
        o, st_o, tr = oracle_of(p, O.RULE_BLOCK)
        assert st_o == O.INFEASIBLE and o.n_pivots == 0
        assert_equals_oracle(b, i, o, st_o, tr)


# ---- 16
def test_nothing_to_run_on_the_host():
    check_nothing_to_run(lambda b: b.run_on_host())

