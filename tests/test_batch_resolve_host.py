"""Re-solving a solved batch with new arc costs (mcf_batch_set_costs / mcf_batch_resolve, DESIGN.md 3.14 "Re-solve") without a GPU:
mcf_batch_rerun_on_host runs the re-solve -- batch_reprice and the pivots of csrc/batch_step.hip.h -- with one lane on the CPU.

The check functions take `first` and `again` (BatchSolver -> BatchSolver): run_on_host / rerun_on_host here, solve / resolve in
test_batch_resolve_gpu.py.  The reference is the oracle's COLD solve of the instance with the new costs: a warm re-solve takes another
pivot path, so what is compared is the status, for Optimal the total cost (the optimum value is unique), and that the returned flows and
potentials are an optimal pair for the new costs (helpers.validate_solution: bounds, conservation, complementary slackness, dual = primal).
A cold re-solve (last status not Optimal) is compared with a fresh batch exactly, trace included."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import mincostflow_amd as M
from mincostflow_amd import _lib as L
from oracle import ns_oracle as O

from adversarial import BIG_COST, random_problem
from helpers import fixtures, load, validate_solution
from test_batch_host import ROOT, RULES, bound_infeasible, generated, oracle_of

ALL_RULES = [O.RULE_BLOCK, O.RULE_BEST, O.RULE_FIRST]
HOST = (lambda b: b.run_on_host(), lambda b: b.rerun_on_host())
TRACE = 1 << 15
SEED = 20261018
SIZES = (63, 64, 65, 129, 257, 640, 1000)      # m + n: round one, two and four strides of the wave, ten strides, no multiple
PER_SIZE = 12
MODES = ("redraw 5 %", "full redraw", "sign flips", "2^40 + jitter")


def snapshot(b, i):
    st = b.status(i)
    out = [st, b.pivots(i), b.trace(i).tobytes()]
    if st == M.SolverStatus.Optimal:
        out += [b.total_cost(i), b.flows(i).tobytes(), b.potentials(i).tobytes()]
    return out


def with_cost(p, cost):
    return O.Problem(p.n, p.m, p.src, p.tgt, p.lower, p.upper, cost, p.supply)


# ---- the family of item 2: every arc has a finite, positive capacity after the lower-bound shift, so status and optimum do not depend on
# the pivot path (the limit documented in include/mcf_hip.h)
@functools.lru_cache(maxsize=None)
def family():
    """((problem, supply type) ...): kinds balanced / negative / excess by k % 3, LEQ every fifth, lower bounds on 15 % of the arcs."""
    rng = np.random.default_rng(SEED)
    out = []
    for size in SIZES:
        for _ in range(PER_SIZE):
            k = len(out)
            n = int(rng.integers(2, min(size, 60)))
            p = random_problem(rng, n, size - n, ("balanced", "negative", "excess")[k % 3], zero_capacity=False, inf_fraction=0.0)
            assert np.all(p.upper > p.lower) and np.all(p.upper < O.INF_CAP)
            out.append((p, O.LEQ if k % 5 == 4 else O.GEQ))
    assert any(np.any(p.lower != 0) for p, _ in out)
    return tuple(out)


def new_cost(p, k, step):
    """The costs of instance k at re-solve `step`: the mode moves on by one per step, so every instance meets all four."""
    rng = np.random.default_rng([SEED, k, step])
    mode = (k + step) % 4
    m = p.m
    if mode == 0:
        hit = rng.random(m) < 0.05
        hit[int(rng.integers(0, m))] = True
        return np.where(hit, rng.integers(-6, 20, m), p.cost).astype(np.int64)
    if mode == 1:
        return rng.integers(-6, 20, m).astype(np.int64)
    if mode == 2:
        return np.where(rng.random(m) < 0.5, -p.cost, p.cost).astype(np.int64)
    return (rng.integers(-6, 20, m) * np.int64(BIG_COST) + rng.integers(-3, 4, m)).astype(np.int64)


def cold_reference(p, stype, rule):
    """(status, total cost or None, exact) of the oracle's cold solve; its numbers did not overflow.  exact is None when the oracle's own
    flows and potentials pass validate_solution.  They cannot where the reference answers Optimal to supplies it cannot place -- a surplus
    under GEQ: it looks at the root links only and leaves the surplus on an artificial arc (asserted: only with unbalanced supplies, and
    only by the conservation check).  Which node keeps the surplus depends on the pivot path, so the library re-solves such an instance
    cold, and exact = (flows, potentials, pivots, trace) is what it must then give, bit for bit."""
    o, st, tr = oracle_of(p, rule, stype, trace_cap=TRACE)
    if st != O.OPTIMAL:
        return st, None, None
    assert o.total_cost == sum(int(f) * int(c) for f, c in zip(o.flow(), p.cost))
    assert max((abs(int(v)) for v in o.potential()), default=0) < 1 << 62
    try:
        validate_solution(p, o.flow(), o.potential(), stype)
    except AssertionError as e:
        assert "conservation" in str(e) and int(p.supply.sum()) != 0 and o.n_pivots < TRACE
        return st, o.total_cost, (o.flow(), o.potential(), o.n_pivots, tr)
    return st, o.total_cost, None


def warm_after(ref):
    """Whether an instance whose last solve gave `ref` is re-solved from its basis."""
    return ref[-3] == O.OPTIMAL and ref[-1] is None


@functools.lru_cache(maxsize=None)
def original_reference(rule):
    return tuple(cold_reference(p, stype, rule) for p, stype in family())


STEPS = 4


@functools.lru_cache(maxsize=None)
def family_reference(rule):
    """per step ((cost, status, total cost, exact) per instance).  Asserted on the oracle's answers alone: at least 10 Optimal and 10 Infeasible in
    every step, no Unbounded."""
    out = []
    for step in range(STEPS):
        row = []
        for k, (p, stype) in enumerate(family()):
            cost = new_cost(p, k, step)
            row.append((cost,) + cold_reference(with_cost(p, cost), stype, rule))
        count = {st: sum(r[1] == st for r in row) for st in (O.OPTIMAL, O.INFEASIBLE, O.UNBOUNDED)}
        print(f"re-solve family, rule {rule}, step {step}: {count}")
        assert count[O.OPTIMAL] >= 10 and count[O.INFEASIBLE] >= 10 and count[O.UNBOUNDED] == 0 and sum(count.values()) == len(row), count
        assert sum(warm_after(r) for r in row) >= 10
        out.append(tuple(row))
    return tuple(out)


def assert_matches_cold(b, i, p, stype, cost, st, total, exact, what):
    assert b.status(i) == st, (what, b.status(i), st)
    if st == O.OPTIMAL:
        assert b.total_cost(i) == total, (what, b.total_cost(i), total)
        if exact is None:
            assert validate_solution(with_cost(p, cost), b.flows(i), b.potentials(i), stype) == total, what
        else:
            assert np.array_equal(b.flows(i), exact[0]) and np.array_equal(b.potentials(i), exact[1]), what
            assert b.pivots(i) == exact[2] and np.array_equal(b.trace(i), exact[3]), what


def family_solver(rule, **kw):
    b = M.BatchSolver(rule=RULES[rule], record_trace=TRACE, **kw)
    for p, stype in family():
        b.add(p, supply_type=stype)
    return b


def run_family_steps(b, rule, again, steps=STEPS):
    """b: the family, solved.  Every step gives every instance new costs, re-solves and compares with the cold reference."""
    refs = family_reference(rule)
    for step in range(steps):
        last = refs[step - 1] if step else original_reference(rule)
        warm = sum(warm_after(r) for r in last)
        for i, (cost, *_rest) in enumerate(refs[step]):
            b.set_costs(i, cost)
        again(b)
        st = b.resolve_stats()
        assert (st["warm_instances"], st["cold_instances"], st["untouched_instances"]) == (warm, len(b) - warm, 0), (step, st)
        assert st["total_pivots"] == sum(b.pivots(i) for i in range(len(b)))
        for i, ((p, stype), (cost, st_o, total, exact)) in enumerate(zip(family(), refs[step])):
            assert_matches_cold(b, i, p, stype, cost, st_o, total, exact, f"step {step}, instance {i}, {MODES[(i + step) % 4]}")
    return b


# ---- 1
def unchanged_inputs():
    out = [(name, load(path), O.GEQ) for name, path, _ in fixtures()]
    out = [(name, p, stype) for name, p, stype in out if p.m <= 5000]
    names = {name for name, _, _ in out}
    assert {"circulation_100_0_10", "SimpleProblemIllustration"} <= names and len(out) >= 20
    out += [(f"generated_{seed}", generated(seed, 200, 600), O.GEQ) for seed in range(41, 49)]
    out += [(f"family_{k}", p, stype) for k, (p, stype) in enumerate(family()) if k % 4 == 0]      # lower bounds, LEQ, Infeasible ones
    assert any(stype == O.LEQ and np.any(p.lower != 0) for _, p, stype in out)
    return out


def check_unchanged_costs(first, again, rule):
    cases = unchanged_inputs()
    b = M.BatchSolver(rule=RULES[rule], record_trace=TRACE)
    for _, p, stype in cases:
        b.add(p, supply_type=stype)
    first(b)
    before = [snapshot(b, i) for i in range(len(cases))]
    optimal = [warm_after(cold_reference(p, stype, rule)) for _, p, stype in cases]          # re-solved warm
    assert sum(optimal) >= 40 and not all(optimal) and all(s[0] == M.SolverStatus.Optimal for s, o in zip(before, optimal) if o)
    for i, (_, p, _) in enumerate(cases):
        b.set_costs(i, p.cost)
    again(b)
    for i, (name, _, _) in enumerate(cases):
        after = snapshot(b, i)
        if optimal[i]:                                      # warm: nothing is eligible under the potentials of the same basis
            assert after[1] == 0 and after[2] == b"", (name, after[1])
            assert after[0] == before[i][0] and after[3:] == before[i][3:], name
        else:                                               # cold: the same solve again
            assert after == before[i], name
    st = b.resolve_stats()
    assert st["warm_instances"] == sum(optimal) and st["untouched_instances"] == 0 and st["total_pivots"] == sum(s[1] for s, o in zip(before, optimal) if not o)


@pytest.mark.parametrize("rule", ALL_RULES)
def test_unchanged_costs_need_no_pivot_on_the_host(rule):
    check_unchanged_costs(*HOST, rule)


# ---- 2
@pytest.mark.parametrize("rule", ALL_RULES)
def test_new_costs_against_a_cold_solve_on_the_host(rule):
    run_family_steps(HOST[0](family_solver(rule)), rule, HOST[1])


# ---- 3
def check_chains(first, again, rule):
    """Costs A -> B -> A -> B on the instances with lower bounds: every step the cold answer, the third the first's total cost, and flows
    inside the ORIGINAL bounds with the ORIGINAL supplies (validate_solution), which a lower-bound shift applied twice or not at all breaks."""
    picked = [(k, p, stype) for k, (p, stype) in enumerate(family()) if np.any(p.lower != 0)]
    assert len(picked) >= 20
    b = M.BatchSolver(rule=RULES[rule], record_trace=TRACE)
    for _, p, stype in picked:
        b.add(p, supply_type=stype)
    first(b)
    costs = {"A": [p.cost for _, p, _ in picked], "B": [new_cost(p, k, 1) for k, p, _ in picked]}
    refs = {w: [cold_reference(with_cost(p, c), stype, rule) for (_, p, stype), c in zip(picked, costs[w])] for w in "AB"}
    assert sum(warm_after(r) for r in refs["A"]) >= 8 and sum(warm_after(r) for r in refs["B"]) >= 8
    totals = []
    for step, w in enumerate("ABAB"):
        if step:
            for i, c in enumerate(costs[w]):
                b.set_costs(i, c)
            again(b)
        for i, (k, p, stype) in enumerate(picked):
            assert_matches_cold(b, i, p, stype, costs[w][i], *refs[w][i], f"chain step {step} ({w}), family instance {k}")
        totals.append([b.total_cost(i) if b.status(i) == M.SolverStatus.Optimal else None for i in range(len(picked))])
    assert totals[2] == totals[0] and totals[3] == totals[1]


@pytest.mark.parametrize("rule", ALL_RULES)
def test_chains_do_not_drift_on_the_host(rule):
    check_chains(*HOST, rule)


# ---- 4
@functools.lru_cache(maxsize=None)
def art_cost_cases(rule):
    """Family instances whose first solve ends Optimal with an artificial arc still in the basis (at zero flow: Optimal means none carries
    any), read off the oracle's State[] -- the batch's first solve takes the oracle's pivots -- and the Infeasible ones."""
    basic, infeasible = [], []
    for k, (p, stype) in enumerate(family()):
        o, st, _ = oracle_of(p, rule, stype, trace_cap=0)
        state = o.internal_arrays()["state"]
        if st == O.OPTIMAL and np.any(state[p.m + p.n:o.all_arc_num] == L.STATE_TREE) and warm_after(original_reference(rule)[k]):
            basic.append(k)
        elif st == O.INFEASIBLE and not bound_infeasible(p):
            infeasible.append(k)
    print(f"art_cost cases, rule {rule}: {len(basic)} Optimal with a basic artificial arc, {len(infeasible)} Infeasible")
    assert len(basic) >= 5 and len(infeasible) >= 5
    return tuple(basic + infeasible)


def check_art_cost_moves(first, again, rule):
    """Costs x 2^20 and back.  An artificial arc that keeps its old cost is then far cheaper than a real arc (or far dearer): flow would go
    round through the root, and the recomputed potentials would be those of another problem."""
    picked = [(k,) + family()[k] for k in art_cost_cases(rule)]
    b = M.BatchSolver(rule=RULES[rule], record_trace=TRACE)
    for _, p, stype in picked:
        b.add(p, supply_type=stype)
    first(b)
    for scale in (1 << 20, 1, 1 << 20):
        refs = []
        for i, (_, p, stype) in enumerate(picked):
            cost = p.cost * np.int64(scale)
            refs.append((cost,) + cold_reference(with_cost(p, cost), stype, rule))
            b.set_costs(i, cost)
        again(b)
        for i, ((k, p, stype), (cost, st, total, exact)) in enumerate(zip(picked, refs)):
            assert_matches_cold(b, i, p, stype, cost, st, total, exact, f"costs x {scale}, family instance {k}")


@pytest.mark.parametrize("rule", ALL_RULES)
def test_art_cost_follows_the_costs_on_the_host(rule):
    check_art_cost_moves(*HOST, rule)


# ---- 5
PIVOT_LIMIT = 5


@functools.lru_cache(maxsize=None)
def mixed_parts(rule):
    """[(role, problem, supply type, new cost or None)] for one batch with a pivot limit of 5: tiny instances that end Optimal inside it
    (untouched and warm ones), one infeasible by its bounds, one Infeasible after pivots and one that hits the limit."""
    rng = np.random.default_rng(SEED + 1)
    small = []
    while len(small) < 8:
        p = random_problem(rng, 4, 6, "balanced", zero_capacity=False, inf_fraction=0.0)
        o, st, _ = oracle_of(p, rule, trace_cap=0)
        o2, st2, _ = oracle_of(with_cost(p, new_cost(p, len(small), 1)), rule, trace_cap=0)
        if st == st2 == O.OPTIMAL and 0 < o.n_pivots <= PIVOT_LIMIT and o2.n_pivots <= PIVOT_LIMIT:
            small.append(p)
    by_bounds = O.Problem(2, 1, [0], [1], [3], [2], [4], [1, -1])
    stuck = O.Problem(3, 2, [0, 1], [1, 2], [0, 0], [1, 1], [2, 3], [2, 0, -2])          # one unit gets through: Infeasible after pivots
    o, st, _ = oracle_of(stuck, rule, trace_cap=0)
    assert st == O.INFEASIBLE and 0 < o.n_pivots <= PIVOT_LIMIT
    long = generated(11)
    parts = []
    for k, p in enumerate(small):
        parts.append(("untouched" if k % 2 else "warm", p, O.GEQ, None if k % 2 else new_cost(p, k, 1)))
    parts.insert(2, ("by bounds", by_bounds, O.GEQ, np.array([7], np.int64)))
    parts.insert(5, ("stuck", stuck, O.GEQ, np.array([5, 1], np.int64)))
    parts.append(("limit", long, O.GEQ, new_cost(long, 99, 1)))
    parts.append(("untouched", generated(12, 60, 200), O.GEQ, None))                      # NotSolved at the limit, and left alone
    return tuple(parts)


def check_mixed_batch(first, again, rule, **kw):
    parts = mixed_parts(rule)
    b = M.BatchSolver(rule=RULES[rule], pivot_limit=PIVOT_LIMIT, record_trace=64, **kw)
    for _, p, stype, _ in parts:
        b.add(p, supply_type=stype)
    first(b)
    before = [snapshot(b, i) for i in range(len(parts))]
    for i, (role, p, _, cost) in enumerate(parts):
        want = {"untouched": None, "warm": M.SolverStatus.Optimal, "by bounds": M.SolverStatus.Infeasible, "stuck": M.SolverStatus.Infeasible,
                "limit": M.SolverStatus.NotSolved}[role]
        assert want is None or b.status(i) == want, (role, b.status(i))
        if role == "stuck":
            assert b.pivots(i) > 0
        if role == "limit":
            assert b.pivots(i) == PIVOT_LIMIT
        if cost is not None:
            b.set_costs(i, np.zeros(p.m, np.int64))          # the last call wins
            b.set_costs(i, cost)
    again(b)
    fresh = M.BatchSolver(rule=RULES[rule], pivot_limit=PIVOT_LIMIT, record_trace=64, **kw)
    for _, p, stype, cost in parts:
        fresh.add(p if cost is None else with_cost(p, cost), supply_type=stype)
    first(fresh)
    for i, (role, p, stype, cost) in enumerate(parts):
        if role == "untouched":
            assert snapshot(b, i) == before[i], i
        elif role == "warm":
            st, total, exact = cold_reference(with_cost(p, cost), stype, rule)
            assert st == O.OPTIMAL and exact is None
            assert_matches_cold(b, i, p, stype, cost, st, total, exact, f"mixed batch, instance {i}")
            assert b.pivots(i) <= PIVOT_LIMIT and len(b.trace(i)) == b.pivots(i)
        else:                                               # cold: a fresh batch, pivot for pivot
            assert snapshot(b, i) == snapshot(fresh, i), (role, i)
            if role == "by bounds":
                assert b.pivots(i) == 0
    st = b.resolve_stats()
    roles = [r for r, *_ in parts]
    assert st["warm_instances"] == roles.count("warm") and st["cold_instances"] == 3 and st["untouched_instances"] == roles.count("untouched"), st
    assert st["total_pivots"] == sum(b.pivots(i) for i, r in enumerate(roles) if r != "untouched")
    return b


@pytest.mark.parametrize("rule", ALL_RULES)
def test_mixed_batch_on_the_host(rule):
    b = check_mixed_batch(*HOST, rule)
    st = b.resolve_stats()
    assert st["launches"] == 0 and st["bytes_uploaded"] == 0 and st["bytes_downloaded"] == 0


# ---- 6
def check_errors_and_order(first, again_name):
    lib = L.lib()
    p = load("transport_2x3")
    b = M.BatchSolver(record_trace=64)
    b.add(p)
    b.add(generated(5, 40, 120))
    cost = np.ascontiguousarray(p.cost[::-1].copy())
    stats = L.BatchResolveStats()
    # before a solve: costs come with add
    assert lib.mcf_batch_set_costs(b._h, 0, cost.ctypes.data) == L.ERR_STATE
    assert lib.mcf_batch_resolve(b._h) == L.ERR_STATE and lib.mcf_batch_rerun_on_host(b._h) == L.ERR_STATE
    assert lib.mcf_batch_get_resolve_stats(b._h, C.byref(stats)) == L.ERR_STATE
    # null arguments and bad indices, before and after
    for _ in range(2):
        assert lib.mcf_batch_set_costs(None, 0, cost.ctypes.data) == L.ERR_INVALID and lib.mcf_batch_set_costs(b._h, 0, None) == L.ERR_INVALID
        assert lib.mcf_batch_set_costs(b._h, 2, cost.ctypes.data) == L.ERR_INVALID and lib.mcf_batch_set_costs(b._h, -1, cost.ctypes.data) == L.ERR_INVALID
        assert lib.mcf_batch_resolve(None) == L.ERR_INVALID and lib.mcf_batch_rerun_on_host(None) == L.ERR_INVALID
        assert lib.mcf_batch_get_resolve_stats(None, C.byref(stats)) == L.ERR_INVALID and lib.mcf_batch_get_resolve_stats(b._h, None) == L.ERR_INVALID
        if not b_solved(b):
            first(b)
    with pytest.raises(ValueError):
        b.set_costs(0, cost[:-1])
    before = [snapshot(b, i) for i in range(2)]
    # nothing changed: MCF_OK, nothing runs -- with or without a device
    for name in ("resolve", "rerun_on_host"):
        getattr(b, name)()
        st = b.resolve_stats()
        assert st["launches"] == 0 and st["untouched_instances"] == 2 and st["warm_instances"] + st["cold_instances"] + st["total_pivots"] + st["bytes_uploaded"] == 0
        assert [snapshot(b, i) for i in range(2)] == before
    # the single-shot calls stay refused, before and after a re-solve
    for _ in range(2):
        for refused in (b.run_on_host, b.solve, lambda: b.add(p)):
            with pytest.raises(M.McfError) as ei:
                refused()
            assert ei.value.code == L.ERR_STATE
        held = snapshot(b, 0)
        b.set_costs(0, cost)
        assert snapshot(b, 0) == held                       # the old results until the re-solve
        getattr(b, again_name)()
        assert b.status(0) == M.SolverStatus.Optimal and b.total_cost(0) == cold_reference(with_cost(p, cost), O.GEQ, O.RULE_BLOCK)[1]
        assert snapshot(b, 1) == before[1]


def b_solved(b):
    return L.lib().mcf_batch_get_status(b._h, 0, C.byref(C.c_int32())) != L.ERR_STATE


def test_errors_and_order_on_the_host():
    check_errors_and_order(HOST[0], "rerun_on_host")


@pytest.mark.skipif(M.device_count() > 0, reason="a GPU is present")
def test_resolve_without_a_device_leaves_the_batch_as_it_was():
    p = load("transport_2x3")
    b = M.BatchSolver(record_trace=64)
    b.add(p)
    b.run_on_host()
    before = snapshot(b, 0)
    cost = p.cost[::-1].copy()
    b.set_costs(0, cost)
    with pytest.raises(M.McfError) as ei:
        b.resolve()
    assert ei.value.code == L.ERR_NO_DEVICE
    assert snapshot(b, 0) == before
    b.rerun_on_host()                                       # the new costs are still waiting
    assert b.resolve_stats()["warm_instances"] == 1
    assert b.total_cost(0) == cold_reference(with_cost(p, cost), O.GEQ, O.RULE_BLOCK)[1]


def test_resolve_stats_have_the_layout_of_the_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void){printf("%%zu %%zu %%zu\\n", sizeof(mcf_batch_resolve_stats),'
                   ' offsetof(mcf_batch_resolve_stats, bytes_uploaded), offsetof(mcf_batch_resolve_stats, kernel_ns));return 0;}\n'
                   % os.path.join(ROOT, "include", "mcf_hip.h"))
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(L.BatchResolveStats), L.BatchResolveStats.bytes_uploaded.offset, L.BatchResolveStats.kernel_ns.offset]
