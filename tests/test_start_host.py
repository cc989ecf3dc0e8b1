"""Starting placed batches from a basis the caller supplies (mcf_ubatch_solve_from / mcf_rbatch_solve_from, DESIGN.md 3.14 "Start from a
given basis") without a GPU: the hooks run the device's own start step -- the walk over the forest, the hanging, flows, potentials and the
class -- its dual and primal pivots and its fallback with one lane on the CPU.

The rows come from cost_ranges_on_host() after a first solve of the re-data family (test_redata_host.py).  References: the oracle's cold
solve on whatever data the start is given (status always, for Optimal the total cost and validate_solution on flows and potentials; for
every row that went cold the oracle's fresh solve bit for bit, trace included) and start_oracle.classify(), which predicts the class of
every row from the problem and the row alone.  test_start_gpu.py imports the cases and the checkers from here."""
import functools

import numpy as np
import pytest

import mincostflow_amd as M
from mincostflow_amd import _lib as L
from oracle import ns_oracle as O

import start_oracle as S
from helpers import validate_solution
from test_batch_resolve_host import cold_reference, new_cost, with_cost
from test_redata_host import LIMIT, PADDED_NODES, STEPS, assert_row_is_fresh, chain, chain_reference, padded_chain, padded_reference, redata_family
from test_uniform_host import ALL_RULES, NOT_SOLVED, TRACE, answer_of, assert_row_matches_cold, step_costs, to_numpy, uniform_of

DATA_STEPS = ("a", "b", "c", "e")       # the chain steps test 3 starts on; with the first solve's rows they force dual starts
FROM_HOST = lambda u, rows, a, stype: u.run_from_on_host(rows, supply_type=stype, **a)
SOLVE_HOST = lambda u, a, stype: u.run_on_host(supply_type=stype, **a)
RANGES_HOST = lambda u: u.cost_ranges_on_host(costs=False)


@functools.lru_cache(maxsize=None)
def first_solve(rule):
    """per graph of the family: (rows of a fresh run_on_host, ranged, arc_state) -- the basis every test here starts from.  The floors on
    the family are asserted here, on code that was there before solve_from and on numpy alone."""
    out = []
    spanning = forest = cold = 0
    for t, stype in redata_family():
        u = uniform_of(t, rule)
        r = to_numpy(u.run_on_host(supply_type=stype, **t.arrays()))
        g = u.cost_ranges_on_host(costs=False)
        ranged, rows = np.asarray(g.ranged).astype(bool), np.asarray(g.arc_state)
        assert rows.dtype == np.int8 and rows.shape == (t.count, t.m)
        trees = (rows == S.TREE).sum(axis=1)
        assert np.all(trees[ranged] <= t.n - 1) and not rows[~ranged].any()
        spanning += int((ranged & (trees == t.n - 1)).sum())
        forest += int((ranged & (trees < t.n - 1)).sum())
        cold += int((~ranged).sum())                # all zero = all TREE: more than n - 1 tree arcs
        assert all(S.classify(p, stype, rows[k]).kind == S.COLD for k, p in enumerate(t.variants) if not ranged[k])
        out.append((r, ranged, rows))
    print(f"first solve, rule {rule}: {spanning} spanning ranged rows, {forest} forest rows, {cold} rows cold by rule")
    assert spanning >= 24 and forest >= 1 and cold >= 20, (spanning, forest, cold)
    return tuple(out)


def is_spanning(t, ranged, rows, k):
    return bool(ranged[k]) and S.count_tree(rows[k]) == t.n - 1


def assert_start(r, problems, stype, rows, refs, stats, what):
    """One start of `problems` from `rows` against the oracle: every row as assert_row_matches_cold; rows cold by rule, and accepted rows
    that cannot have stood, are the fresh solve's bit for bit; the statistics count the classes start_oracle predicts.
    refs: per problem (cold_reference(), answer_of()).  Returns the predictions."""
    kinds = [S.classify(p, stype, rows[k]).kind for k, p in enumerate(problems)]
    for k, (p, (ref, answer)) in enumerate(zip(problems, refs)):
        assert_row_matches_cold(r, k, p, stype, ref, what)
        if kinds[k] == S.COLD or ref[0] != O.OPTIMAL:
            assert_row_is_fresh(r, k, answer, what)
        assert r["pivots"][k] <= TRACE
    count = {kind: kinds.count(kind) for kind in (S.PRIMAL, S.DUAL, S.COLD)}
    assert (stats["primal_starts"], stats["dual_starts"], stats["cold_instances"]) == (count[S.PRIMAL], count[S.DUAL], count[S.COLD]), (what, stats, count)
    must_fall_back = sum(kind != S.COLD and ref[0] != O.OPTIMAL for kind, (ref, _) in zip(kinds, refs))
    assert must_fall_back <= stats["fallback_instances"] <= count[S.PRIMAL] + count[S.DUAL], (what, stats)
    assert stats["dual_pivots"] >= 0 and stats["primal_pivots"] >= 0 and stats["dual_pivots"] + stats["primal_pivots"] >= int(r["pivots"].sum()), (what, stats)
    assert (stats["dual_pivots"] > 0) <= (count[S.DUAL] > 0), (what, stats)
    return kinds


@functools.lru_cache(maxsize=None)
def recost_cases(rule):
    """per graph: (topology with the costs of step_costs(t, j, 1), references per variant)"""
    out = []
    for j, (t, stype) in enumerate(redata_family()):
        cost = step_costs(t, j, 1)
        top = type(t)(t.n, t.src, t.tgt, [with_cost(p, cost[k]) for k, p in enumerate(t.variants)], t.zero_capacity)
        out.append((top, tuple((cold_reference(q, stype, rule), answer_of(q, rule, stype)) for q in top.variants)))
    return tuple(out)


# ---- 1: the round trip
def check_round_trip(solve, start, ranges, rule, **kw):
    for j, ((t, stype), (r0, ranged, rows)) in enumerate(zip(redata_family(), first_solve(rule))):
        a = t.arrays()
        refs = tuple((cold_reference(p, stype, rule), answer_of(p, rule, stype)) for p in t.variants) if j == 3 else chain_reference(rule)[j][0]
        v = uniform_of(t, rule, **kw)
        r = to_numpy(start(v, rows, a, stype))
        kinds = assert_start(r, t.variants, stype, rows, refs, v.start_stats(), f"round trip, graph {j}")
        back = np.asarray(to_numpy_rows(ranges(v).arc_state))
        for k, p in enumerate(t.variants):
            if is_spanning(t, ranged, rows, k):
                assert kinds[k] == S.PRIMAL and r["pivots"][k] == 0 and not r["trace"][k].any() and r["status"][k] == O.OPTIMAL, (j, k, kinds[k], r["pivots"][k])
                assert r["total_cost"][k] == r0["total_cost"][k] and np.array_equal(r["flows"][k], r0["flows"][k]), (j, k)
                assert validate_solution(p, r["flows"][k], r["potentials"][k], stype) == r0["total_cost"][k]
                assert np.array_equal(back[k], rows[k]), (j, k)
            if kinds[k] == S.COLD:
                for name in r:
                    assert np.array_equal(r[name][k], r0[name][k]), (j, k, name)


def to_numpy_rows(a):
    return a if isinstance(a, np.ndarray) else a.cpu().numpy()


@pytest.mark.parametrize("rule", ALL_RULES)
def test_round_trip_on_the_host(rule):
    check_round_trip(SOLVE_HOST, FROM_HOST, RANGES_HOST, rule)


# ---- 2: new costs on a kept basis
def check_new_costs(start, rule, **kw):
    seen = []
    for j, ((t, stype), (_, _, rows), (top, refs)) in enumerate(zip(redata_family(), first_solve(rule), recost_cases(rule))):
        v = uniform_of(t, rule, **kw)
        r = to_numpy(start(v, rows, top.arrays(), stype))
        seen += assert_start(r, top.variants, stype, rows, refs, v.start_stats(), f"new costs, graph {j}")
    return seen


@pytest.mark.parametrize("rule", ALL_RULES)
def test_new_costs_on_a_kept_basis_on_the_host(rule):
    check_new_costs(FROM_HOST, rule)


# ---- 3: new data on a kept basis
def check_new_data(start, rule, **kw):
    seen = []
    dual = dict.fromkeys(DATA_STEPS, 0)
    for j, (((t, steps), (_, stype)), (_, _, rows), refs) in enumerate(zip(zip(chain(), redata_family()), first_solve(rule), chain_reference(rule))):
        for name in DATA_STEPS:
            s = STEPS.index(name)
            v = uniform_of(t, rule, **kw)
            r = to_numpy(start(v, rows, steps[s].arrays(), stype))
            st = v.start_stats()
            kinds = assert_start(r, steps[s].variants, stype, rows, refs[s + 1], st, f"new data, graph {j}, step {name}")
            if S.DUAL in kinds:
                assert st["dual_starts"] > 0 and st["dual_pivots"] > 0, (j, name, st)
                dual[name] += st["dual_pivots"]
            seen += kinds
    print(f"rule {rule}: dual pivots per step {dual}")
    assert all(dual[name] > 0 for name in DATA_STEPS), dual
    return seen


@pytest.mark.parametrize("rule", ALL_RULES)
def test_new_data_on_a_kept_basis_on_the_host(rule):
    check_new_data(FROM_HOST, rule)


def test_every_class_is_predicted():
    """Over the cases of this file each of the three classes is predicted at least 3 times -- from the oracle and the rows alone."""
    rule = O.RULE_BLOCK
    kinds = []
    for j, ((t, stype), (_, _, rows), (top, _)) in enumerate(zip(redata_family(), first_solve(rule), recost_cases(rule))):
        kinds += [S.classify(p, stype, rows[k]).kind for k, p in enumerate(t.variants)]
        kinds += [S.classify(q, stype, rows[k]).kind for k, q in enumerate(top.variants)]
        for name in DATA_STEPS:
            kinds += [S.classify(p, stype, rows[k]).kind for k, p in enumerate(chain()[j][1][STEPS.index(name)].variants)]
    count = {kind: kinds.count(kind) for kind in (S.PRIMAL, S.DUAL, S.COLD)}
    print(count)
    assert min(count.values()) >= 3, count


# ---- 4: one shared row
COPIES = 7


def shared_case(rule, j=2):
    """A handle of COPIES instances of graph j that share the supplies and bounds of its first spanning variant and differ in costs."""
    (t, stype), (_, ranged, rows) = redata_family()[j], first_solve(rule)[j]
    k = next(k for k in range(t.count) if is_spanning(t, ranged, rows, k))
    p = t.variants[k]
    cost = np.stack([p.cost] + [new_cost(p, 1000 + c, c % 3) for c in range(1, COPIES)])
    top = type(t)(t.n, t.src, t.tgt, [with_cost(p, c) for c in cost], [False] * COPIES)
    return top, stype, dict(cost=cost, supply=p.supply, lower=p.lower, upper=p.upper), rows[k]


def check_shared_row(start, rule, **kw):
    top, stype, a, row = shared_case(rule)
    u, v = uniform_of(top, rule, **kw), uniform_of(top, rule, **kw)
    shared = to_numpy(start(u, row, a, stype))
    tiled = to_numpy(start(v, np.ascontiguousarray(np.tile(row, (COPIES, 1))), a, stype))
    for name in shared:
        assert np.array_equal(shared[name], tiled[name]), name
    su, sv = u.start_stats(), v.start_stats()
    for name in ("primal_starts", "dual_starts", "cold_instances", "fallback_instances", "dual_pivots", "primal_pivots"):
        assert su[name] == sv[name], name
    refs = tuple((cold_reference(q, stype, rule), answer_of(q, rule, stype)) for q in top.variants)
    assert_start(shared, top.variants, stype, [row] * COPIES, refs, su, "one shared row")
    assert shared["pivots"][0] == 0 and su["primal_starts"] == COPIES          # the row's own costs: optimal as it stands; the others: primal pivots


def test_one_shared_row_on_the_host():
    check_shared_row(FROM_HOST, O.RULE_BLOCK)


# ---- 5: hostile rows
def hostile_case(rule, j=0):
    """(topology of one problem per hostile row, supply type, arrays, rows, names): graph j's first spanning variant and its good row, spoilt."""
    (t, stype), (_, ranged, rows) = redata_family()[j], first_solve(rule)[j]
    k = next(k for k in range(t.count) if is_spanning(t, ranged, rows, k))
    p, good = t.variants[k], rows[k]
    assert int(p.supply.sum()) == 0 and np.any(p.supply != 0)
    src, tgt = t.src, t.tgt
    ends = [frozenset((int(a), int(b))) for a, b in zip(src, tgt)]
    loop = next(e for e in range(t.m) if src[e] == tgt[e])
    pair = next((e, f) for e in range(t.m) for f in range(e + 1, t.m) if len(ends[e]) == 2 and ends[e] == ends[f])
    triangle = next((e, f, g) for e in range(t.m) for f in range(e + 1, t.m) for g in range(f + 1, t.m)
                    if len(ends[e]) == len(ends[f]) == len(ends[g]) == 2 and len({ends[e], ends[f], ends[g]}) == 3 and len(ends[e] | ends[f] | ends[g]) == 3)
    lower_only = np.full(t.m, S.LOWER, np.int8)

    def only(*arcs):
        row = lower_only.copy()
        row[list(arcs)] = S.TREE
        return row

    def spoilt(e, value):
        row = good.copy()
        row[e] = value
        return row

    off_tree = next(e for e in range(t.m) if good[e] != S.TREE and len(ends[e]) == 2)
    r0 = first_solve(rule)[j][0]
    carrying = next(e for e in range(t.m) if good[e] == S.TREE and r0["flows"][k][e] != p.lower[e])
    at_upper = next((e for e in range(t.m) if good[e] == S.UPPER), off_tree)
    free = p.upper.copy()
    free[at_upper] = O.INF_CAP
    cases = [("a tree cycle among few arcs", only(*triangle), p), ("two parallel tree arcs", only(*pair), p), ("a tree self loop", only(loop), p),
             ("a cycle closed in a spanning tree", spoilt(off_tree, S.TREE), p), ("the value 2", spoilt(off_tree, 2), p), ("the value -2", spoilt(off_tree, -2), p),
             ("UPPER on an arc made uncapacitated", spoilt(at_upper, S.UPPER), O.Problem(p.n, p.m, p.src, p.tgt, p.lower, free, p.cost, p.supply)),
             ("all LOWER with supplies", lower_only, p), ("all TREE", np.zeros(t.m, np.int8), p),
             ("a forest whose components do not balance", spoilt(carrying, S.LOWER), p)]
    top = type(t)(t.n, t.src, t.tgt, [q for _, _, q in cases], [False] * len(cases))
    return top, stype, np.ascontiguousarray(np.stack([row for _, row, _ in cases])), [name for name, _, _ in cases]


def check_hostile_rows(solve, start, rule, **kw):
    top, stype, rows, names = hostile_case(rule)
    for k, (p, name) in enumerate(zip(top.variants, names)):
        assert S.classify(p, stype, rows[k]).kind == S.COLD, name
    a = top.arrays()
    fresh = to_numpy(solve(uniform_of(top, rule, **kw), a, stype))
    u = uniform_of(top, rule, **kw)
    r = to_numpy(start(u, rows, a, stype))
    st = u.start_stats()
    assert st["cold_instances"] == top.count and st["primal_starts"] == st["dual_starts"] == st["fallback_instances"] == st["dual_pivots"] == 0, st
    for name in r:
        assert np.array_equal(r[name], fresh[name]), name
    assert (fresh["status"] == O.OPTIMAL).all() and fresh["pivots"].min() > 0


def test_hostile_rows_are_cold_by_rule_on_the_host():
    check_hostile_rows(SOLVE_HOST, FROM_HOST, O.RULE_BLOCK)


# ---- 6: three graphs in one handle, flat rows
@functools.lru_cache(maxsize=None)
def padded_first(rule):
    """(rows of a fresh run_on_host of the padded mix, ranged, the flat arc_state)"""
    base, _ = padded_chain()
    h = base.handle(rule)
    r = base.split(h.run_on_host(supply_type=O.GEQ, **base.arrays()))
    g = h.cost_ranges_on_host(costs=False)
    assert g.arc_state.shape == (int(base.arc_rows[-1]),)
    return to_numpy(r), np.asarray(g.ranged).astype(bool), np.asarray(g.arc_state)


def check_ragged(start, ranges, rule, **kw):
    base, steps = padded_chain()
    refs = padded_reference(rule)
    r0, ranged, flat = padded_first(rule)
    per_row = [flat[base.arc_rows[i]:base.arc_rows[i + 1]] for i in range(base.count)]
    wide = [i for i in range(base.count) if base.n[i] == PADDED_NODES]
    assert len(wide) == 12 and any(ranged[i] and S.count_tree(per_row[i]) < PADDED_NODES - 1 for i in wide)     # forests of thousands of components
    seen = []
    for s, mix in ((None, base), (STEPS.index("b"), steps[STEPS.index("b")])):
        h = base.handle(rule, **kw)
        r = to_numpy(mix.split(start(h, flat, mix.arrays(), O.GEQ)))
        seen += assert_start(r, mix.problems(), O.GEQ, per_row, refs[0 if s is None else s + 1], h.start_stats(), f"three graphs, step {s}")
        if s is None:
            back = to_numpy_rows(ranges(h).arc_state)
            for i in range(base.count):
                if ranged[i] and S.count_tree(per_row[i]) == base.n[i] - 1:
                    assert r["pivots"][i] == 0 and np.array_equal(r["flows"][i], r0["flows"][i]) and np.array_equal(back[base.arc_rows[i]:base.arc_rows[i + 1]], per_row[i]), i
    assert S.DUAL in seen and S.PRIMAL in seen and S.COLD in seen
    return h


def test_three_graphs_in_one_handle_on_the_host():
    check_ragged(FROM_HOST, RANGES_HOST, O.RULE_BLOCK)


# ---- 7: mixed with the other calls, under a limit, refusals, layout
RECOST_HOST = lambda u, a, stype: u.rerun_on_host(supply_type=stype, **a)
REDATA_HOST = lambda u, a, stype: u.rerun_data_on_host(supply_type=stype, **a)


def check_mixed(start, recost, redata, ranges, rule, **kw):
    """solve_from -> resolve -> resolve_data -> cost_ranges, each against the oracle's cold solve of what holds then"""
    for j, (((t, steps), (_, stype)), (_, _, rows)) in enumerate(zip(zip(chain(), redata_family()), first_solve(rule))):
        u = uniform_of(t, rule, **kw)
        cost_1, cost_2, data = step_costs(t, j, 1), step_costs(t, j, 0), steps[1]
        calls = ((lambda u, a, stype: start(u, rows, a, stype), t, cost_1), (recost, t, cost_2), (redata, data, cost_2))
        for c, (call, top, cost) in enumerate(calls):
            r = to_numpy(call(u, dict(top.arrays(), cost=cost), stype))
            held = [with_cost(p, cost[k]) for k, p in enumerate(top.variants)]
            last = [cold_reference(q, stype, rule) for q in held]
            for k, q in enumerate(held):
                assert_row_matches_cold(r, k, q, stype, last[k], f"graph {j}, call {c}")
        g = ranges(u)
        got, state = to_numpy_rows(g.ranged).astype(bool), to_numpy_rows(g.arc_state)
        for k, q in enumerate(held):
            assert got[k] == (last[k][0] == O.OPTIMAL and last[k][2] is None), (j, k)
            if got[k]:
                assert np.all(r["flows"][k][state[k] == S.LOWER] == q.lower[state[k] == S.LOWER]) and np.all(r["flows"][k][state[k] == S.UPPER] == q.upper[state[k] == S.UPPER])
                assert S.classify(q, stype, state[k]).kind == S.PRIMAL


def test_mixed_with_the_other_calls_on_the_host():
    check_mixed(FROM_HOST, RECOST_HOST, REDATA_HOST, RANGES_HOST, O.RULE_BLOCK)


def check_under_a_limit(solve, start, redata, rule, **kw):
    """With a limit of 5 pivots: a stopped instance reports Not Solved with zero rows, a finished one answers as the oracle does, and the
    next re-solve with new data starts every stopped one cold -- its row is then a fresh solve's under the same limit."""
    stopped_then_cold = 0
    for j, (((t, steps), (_, stype)), (_, _, rows)) in enumerate(zip(zip(chain(), redata_family()), first_solve(rule))):
        u = uniform_of(t, rule, pivot_limit=LIMIT, **kw)
        r = to_numpy(start(u, rows, steps[0].arrays(), stype))
        stopped = r["status"] == NOT_SOLVED
        for k, p in enumerate(steps[0].variants):
            if stopped[k]:
                assert r["pivots"][k] == LIMIT and r["total_cost"][k] == 0 and not r["flows"][k].any() and not r["potentials"][k].any(), (j, k)
            else:
                assert_row_matches_cold(r, k, p, stype, cold_reference(p, stype, rule), f"graph {j}, limit")
        top = steps[2]
        again = to_numpy(redata(u, top.arrays(), stype))
        st = u.resolve_data_stats()
        assert st["cold_instances"] >= stopped.sum() and st["warm_instances"] <= (~stopped).sum(), (j, st)
        fresh = to_numpy(solve(uniform_of(t, rule, pivot_limit=LIMIT, **kw), top.arrays(), stype))
        for k in np.flatnonzero(stopped):
            stopped_then_cold += 1
            for name in again:
                assert np.array_equal(again[name][k], fresh[name][k]), (j, k, name)
    assert stopped_then_cold >= 10, stopped_then_cold


def test_under_a_pivot_limit_on_the_host():
    check_under_a_limit(SOLVE_HOST, FROM_HOST, REDATA_HOST, O.RULE_BLOCK)


def test_refusals_and_their_error_codes():
    rule = O.RULE_BLOCK
    (t, stype), (_, _, rows) = redata_family()[0], first_solve(rule)[0]
    a = t.arrays()
    u = uniform_of(t, rule)

    def refused(io_change=None, basis_change=None, fn="mcf_ubatch_run_from_on_host"):
        import ctypes as C
        from test_uniform_host import io_of
        io = io_of(t, a)
        basis = L.UBatchBasisIo(L.MEM_HOST, 0, rows.ctypes.data, t.m)
        if io_change:
            io_change(io)
        if callable(basis_change):
            basis_change(basis)
        rc = getattr(L.lib(), fn)(u._h, C.byref(io), None if basis_change == "null" else C.byref(basis))
        return rc, L.lib().mcf_last_error().decode()

    def set_to(name, value):
        return lambda s: setattr(s, name, value)

    rc, msg = refused(basis_change=set_to("arc_state", None))
    assert rc == L.ERR_INVALID and "arc_state" in msg
    rc, msg = refused(basis_change=set_to("memory", L.MEM_DEVICE))
    assert rc == L.ERR_INVALID and "memory" in msg
    rc, msg = refused(basis_change=set_to("state_stride", -1))
    assert rc == L.ERR_INVALID and "stride" in msg
    mask = np.ones(t.count, np.uint8)
    rc, msg = refused(io_change=set_to("changed", mask.ctypes.data))
    assert rc == L.ERR_INVALID and "changed" in msg
    rc, msg = refused(io_change=set_to("memory", L.MEM_DEVICE), basis_change=set_to("memory", L.MEM_DEVICE))
    assert rc == L.ERR_INVALID and "host" in msg
    rc, msg = refused(basis_change="null")
    assert rc == L.ERR_INVALID and "null" in msg
    # nothing of that touched the handle: it has not been solved
    with pytest.raises(M.McfError) as e:
        u.rerun_on_host(supply_type=stype, **a)
    assert e.value.code == L.ERR_STATE
    # bad arrays never reach the library
    for bad in (rows.astype(np.int64), rows[:, :-1], rows[:-1], np.ascontiguousarray(rows.T).T, None):
        with pytest.raises(ValueError):
            u.run_from_on_host(bad, supply_type=stype, **a)
    with pytest.raises(M.McfError) as e:
        u.rerun_on_host(supply_type=stype, **a)
    assert e.value.code == L.ERR_STATE
    # and a start is a solve: afterwards the re-solves go on from it
    u.run_from_on_host(rows, supply_type=stype, **a)
    assert not to_numpy(u.rerun_on_host(supply_type=stype, **a))["pivots"][first_solve(rule)[0][1]].any()
    assert M.UniformBatch.start_stats is M.RaggedBatch.start_stats and M.UniformBatch.solve_from is M.RaggedBatch.solve_from


@pytest.mark.skipif(M.device_count() > 0, reason="a GPU is present")
def test_without_a_device_the_handle_stays_as_it_was():
    rule = O.RULE_BLOCK
    (t, stype), (r0, ranged, rows) = redata_family()[0], first_solve(rule)[0]
    a = t.arrays()
    u = uniform_of(t, rule)
    u.run_from_on_host(rows, supply_type=stype, **a)
    before = u.start_stats()
    with pytest.raises(M.McfError) as e:
        u.solve_from(rows, supply_type=stype, **a)
    assert e.value.code == L.ERR_NO_DEVICE
    after = u.start_stats()
    assert all(after[name] == before[name] for name in before)
    assert not to_numpy(u.rerun_on_host(supply_type=stype, **a))["pivots"][ranged].any()


def test_start_structs_have_the_layout_of_the_header(tmp_path):
    import ctypes as C
    import os
    import subprocess
    from test_batch_host import ROOT
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void){printf("%%zu %%zu %%zu %%zu %%zu %%zu %%zu %%zu %%zu\\n", '
                   'sizeof(mcf_ubatch_basis_io), offsetof(mcf_ubatch_basis_io, arc_state), offsetof(mcf_ubatch_basis_io, state_stride), '
                   'sizeof(mcf_rbatch_basis_io), sizeof(mcf_ubatch_start_stats), offsetof(mcf_ubatch_start_stats, dual_pivots), '
                   'offsetof(mcf_ubatch_start_stats, kernel_ns), sizeof(mcf_ubatch_io), sizeof(mcf_rbatch_io));return 0;}\n' % os.path.join(ROOT, "include", "mcf_hip.h"))
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(L.UBatchBasisIo), L.UBatchBasisIo.arc_state.offset, L.UBatchBasisIo.state_stride.offset, C.sizeof(L.RBatchBasisIo),
                   C.sizeof(L.UBatchStartStats), L.UBatchStartStats.dual_pivots.offset, L.UBatchStartStats.kernel_ns.offset, 128, 96]
    assert C.sizeof(L.UBatchIo) == 128 and C.sizeof(L.RBatchIo) == 96          # the solve calls' structs keep their layout
