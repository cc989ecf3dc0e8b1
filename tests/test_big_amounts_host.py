"""Supplies, bounds and flows beyond 32 bits (DESIGN.md 3.14 "Amounts beyond 32 bits") through the batch solvers without a GPU: the
families of big_amounts.py through the *_on_host hooks, which run the device's own steps with one lane on the CPU.

Three kinds of check, all exact:
  the oracle     every solve call's rows against the oracle's solve of the same (scaled or irregular) data, bit for bit, as the checkers
                 of test_uniform_host.py, test_redata_host.py and test_start_host.py state it
  the law        a problem whose amounts are multiplied by k is the same problem in another unit: status, pivots, trace, potentials, the
                 counted statistics and the cost ranges are the unscaled run's; flows, total cost, the finite rooms of data_ranges(),
                 violation and unmet of diagnose(), objective and dual cost of validate() are k times the unscaled run's.  A value cut to
                 32 bits breaks it: with K_HIGH such a value IS the unscaled one
  independent    data_ranges_oracle.py and ranges_oracle.py on the oracle's basis, certificate_oracle.py on every cut, oracle/validator.py
                 on every row, and the meaning of the data ranges through resolve_data

Every checker takes its calls as an argument and returns what they gave -- [(kind, rows, counted statistics) ...] --;
test_big_amounts_gpu.py runs the same checkers with the device's calls and compares that record with the hooks' bit for bit."""
import collections
import functools

import numpy as np
import pytest

import mincostflow_amd as M
from oracle import ns_oracle as O
from oracle import validator as V

import big_amounts as B
import certificate_oracle as K
import data_ranges_oracle as D
import ranges_oracle as R
import wide_graphs as W
from test_batch_host import RULES
from test_batch_resolve_host import cold_reference, new_cost, with_cost
from test_data_ranges_host import assert_equals_reference, check_meaning, data_rows
from test_diagnose_host import COUNTS as DIAGNOSE_COUNTED
from test_diagnose_host import FlatNodes, check_instance, diag_rows
from test_ragged_host import Mix
from test_ranges_host import range_rows
from test_redata_host import assert_step
from test_start_host import assert_start
from test_uniform_host import TRACE, Topology, assert_equals_answers, assert_row_matches_cold, batch_answers, to_numpy, uniform_of
from test_uniform_validate_host import Case, assert_equals_oracle, mapped_upper, rows_of
from test_wide_host import RANGE_COUNTED, RAGGED_GRAPHS, REDATA_COUNTED, START_COUNTED

RULE = O.RULE_BLOCK
SOLVE_COUNTED = ("instances", "total_pivots")
DATA_RANGE_COUNTED = ("instances", "ranged", "walks", "hops")
VD = M.Verdict

Calls = collections.namedtuple("Calls", "first again recost start ranges data_ranges diagnose validate batch")
HOST = Calls(first=lambda u, a, stype: u.run_on_host(supply_type=stype, **a),
             again=lambda u, a, stype: u.rerun_data_on_host(supply_type=stype, **a),
             recost=lambda u, a, stype: u.rerun_on_host(supply_type=stype, **a),
             start=lambda u, rows, a, stype: u.run_from_on_host(rows, supply_type=stype, **a),
             ranges=lambda u: u.cost_ranges_on_host(),
             data_ranges=lambda u, pairs: u.data_ranges_on_host(pairs=pairs),
             diagnose=lambda u: u.diagnose_on_host(),
             validate=lambda u, r, a, stype: u.validate_on_host(r, supply_type=stype, **a),
             batch=lambda b: b.run_on_host())


def counted(stats, fields):
    return {f: stats[f] for f in fields}


# ---- what the law says of two records
def times(a, k):
    return a * np.int64(k)


def assert_law(base, big, k, outside, what):
    """base, big: the records of the same calls on the unscaled and on the scaled data.  outside: per pair of an instance's list (or
    per ship row) whether an id is out of range: there a -1 is a mark and no amount.  MCF_RANGE_INF is above every finite room, so it is
    told by its value; nothing else is: a finite -1 is possible in unmet."""
    assert [kind for kind, _, _ in base] == [kind for kind, _, _ in big], what
    for c, ((kind, a, sa), (_, b, sb)) in enumerate(zip(base, big)):
        where = (what, c, kind)
        assert sa == sb, (where, sa, sb)
        same, scaled, marked = {"solve": (("status", "pivots", "trace", "potentials"), ("total_cost", "flows"), ()),
                                "cost_ranges": (("ranged", "arc_state", "cost_down", "cost_up"), (), ()),
                                "data_ranges": (("ranged", "arc_state"), (), ("flow_down", "flow_up", "ship_forth", "ship_back")),
                                "diagnose": (("verdict", "set_size", "side"), ("violation", "unmet"), ()),
                                "validate": (("valid", "errors", "first"), ("objective", "dual_cost"), ())}[kind if kind in ("cost_ranges", "data_ranges", "diagnose", "validate") else "solve"]
        assert set(a) == set(b) == set(same + scaled + marked), where
        for name in same:
            assert a[name].dtype == b[name].dtype and np.array_equal(a[name], b[name]), (where, name)
        for name in scaled:
            differ = np.flatnonzero((b[name] != times(a[name], k)).reshape(-1))
            assert a[name].dtype == b[name].dtype and not len(differ), (where, name, differ[:4], b[name].reshape(-1)[differ[:4]], a[name].reshape(-1)[differ[:4]])
        for name in marked:
            mark = a[name] == D.INF
            if name.startswith("ship"):
                mark |= np.resize(outside, len(a[name])) & (a[name] == -1)
            differ = np.flatnonzero(b[name] != np.where(mark, a[name], times(a[name], k)))
            assert not len(differ), (where, name, differ[:4], b[name][differ[:4]], a[name][differ[:4]])


# ---- the queries of the kept state, each against its independent oracle
TRUTH = {}


def truth_of(p, stype):
    key = (id(p), stype)
    if key not in TRUTH:
        TRUTH[key] = (p, K.feasible(p, stype))
    return TRUTH[key][1]


def queries(calls, u, top, stype, result, pairs, what, truth, oracles=None, data_reference=None):
    """cost_ranges, data_ranges, diagnose and validate of the state the last solve call left on the uniform handle u.
    oracles: per variant (oracle, status) where the kept basis is the oracle's own (after a cold solve): then the cost ranges are held
    to the brute force; data_reference: data_ranges_oracle.reference_rows() of those.  truth: certificate_oracle.feasible() per variant
    (None: this diagnosis is held to the law and the hooks only); every cut is checked by certificate_oracle.check_cut, every row by
    oracle/validator.py."""
    log = []
    r = to_numpy(result)
    g = calls.ranges(u)
    rows = range_rows(g)
    if oracles is not None:
        ranged, state, down, up, _ = R.reference_rows([(p,) + o for p, o in zip(top.variants, oracles)])
        assert np.array_equal(rows["ranged"], ranged), what
        for name, ref in (("arc_state", state), ("cost_down", down), ("cost_up", up)):
            assert np.array_equal(rows[name].reshape(-1), ref), (what, name)
    log.append(("cost_ranges", rows, counted(u.range_stats(), RANGE_COUNTED)))
    g = calls.data_ranges(u, pairs)
    if data_reference is not None:
        assert_equals_reference(g, data_reference, top.variants, [pairs] * top.count, u.data_range_stats(), what)
    assert np.array_equal(data_rows(g)["ranged"], rows["ranged"]), what
    log.append(("data_ranges", data_rows(g), counted(u.data_range_stats(), DATA_RANGE_COUNTED)))
    d = diag_rows(calls.diagnose(u))
    for v, p in enumerate(top.variants if truth is not None else ()):
        assert (d["verdict"][v] == VD.NoVerdict) == (r["status"][v] == O.UNBOUNDED)
        check_instance(p, stype, int(r["status"][v]), int(d["verdict"][v]), int(d["violation"][v]), int(d["set_size"][v]), d["side"][v], d["unmet"][v], truth[v], (what, v))
    log.append(("diagnose", d, counted(u.diagnose_stats(), DIAGNOSE_COUNTED)))
    check = calls.validate(u, result, top.arrays(), stype)
    assert_equals_oracle(check, Case(str(what), top.n, top.src, top.tgt, top.arrays(), {name: r[name] for name in ("status", "total_cost", "flows", "potentials")}, stype), what)
    got = rows_of(check)
    fine = (r["status"] == O.OPTIMAL) & (rows["ranged"] == 1)                  # Optimal with every supply met: nothing to complain about
    assert np.all(got["valid"][fine] == 1) and not got["errors"][fine].any(), what
    log.append(("validate", got, {}))
    return log


# ---- 1: a uniform handle through every kind of solve call, every query after each
def run_chain(calls, t, steps, stype, refs, pairs, what, shared_row, cost_tag, truths, data_reference=None, rule=RULE, handles=None, **kw):
    """first solve -> steps (resolve_data) -> new costs (resolve) on one handle, solve_from(shared_row) on another; every row against the
    oracle, every query after every call.  refs: per topology per variant (cold_reference(), answer_of()); truths: per topology
    certificate_oracle.feasible() per variant, or None.  handles: a list that receives the two handles."""
    log = []
    u = uniform_of(t, rule, **kw)
    res = calls.first(u, t.arrays(), stype)
    assert_equals_answers(res, [answer for _, answer in refs[0]], what)
    log.append(("solve", to_numpy(res), counted(u.stats(), SOLVE_COUNTED)))
    oracles = [B.oracle_of(p, rule, stype, trace_cap=0)[:2] for p in t.variants]
    log += queries(calls, u, t, stype, res, pairs, (what, "solve"), truths[0], oracles, data_reference)
    dual = 0
    for s, top in enumerate(steps):
        res = calls.again(u, top.arrays(), stype)
        d, _ = assert_step(to_numpy(res), top.variants, stype, refs[s], refs[s + 1], u.resolve_data_stats(), (what, "step", s))
        dual += d
        log.append(("resolve_data", to_numpy(res), counted(u.resolve_data_stats(), REDATA_COUNTED)))
        log += queries(calls, u, top, stype, res, pairs, (what, "step", s), truths[s + 1])
    assert dual > 0, what
    last = steps[-1]
    cost = cost_step(last, cost_tag)
    recosted = Topology(last.n, last.src, last.tgt, [with_cost(p, cost[v]) for v, p in enumerate(last.variants)], last.zero_capacity)
    res = calls.recost(u, recosted.arrays(), stype)
    for v, q in enumerate(recosted.variants):
        assert_row_matches_cold(to_numpy(res), v, q, stype, cold_reference(q, stype, rule), (what, "new costs"))
    log.append(("resolve", to_numpy(res), {}))
    log += queries(calls, u, recosted, stype, res, pairs, (what, "new costs"), truths[-1])
    w = uniform_of(t, rule, **kw)
    res = calls.start(w, shared_row, t.arrays(), stype)
    assert_start(to_numpy(res), t.variants, stype, [shared_row] * t.count, refs[0], w.start_stats(), (what, "start"))
    log.append(("solve_from", to_numpy(res), counted(w.start_stats(), START_COUNTED)))
    log += queries(calls, w, t, stype, res, pairs, (what, "start"), truths[0])
    if handles is not None:
        handles += [u, w]
    return log


def cost_step(top, tag):
    """new costs per variant by test_batch_resolve_host.new_cost in its modes 0 to 2 by v % 3 (5 % redrawn, all redrawn, sign flips); its
    fourth mode draws costs of 2^40, whose product with a flow of 2^37 no int64 holds"""
    return np.stack([new_cost(p, 4 * (100 * tag + v) + v % 3 + 3, 1) for v, p in enumerate(top.variants)])


def outside_of(pairs, n):
    return ~np.all((pairs >= 0) & (pairs < n), axis=1)


@functools.lru_cache(maxsize=None)
def wide_truth(g):
    """certificate_oracle.feasible() per topology of graph g's chain and variant, from the unscaled data: whether a flow exists does not
    depend on the unit (big_amounts.cut_truth() asserts that on its family under both factors).  On the big grid, where one answer takes
    0.2 s, for the first solve's data and the last step's only."""
    t, steps, stype = B.wide(1)[g]
    tops = (t,) + steps
    return tuple(None if g == W.BIG and 0 < s < len(steps) else tuple(K.feasible(p, stype) for p in top.variants) for s, top in enumerate(tops))


def wide_chain_log(calls, g, k, **kw):
    """graph g of the wide family with every amount times k; the shared row of the start is the UNSCALED first variant's exported basis"""
    t, steps, stype = B.wide(k)[g]
    return run_chain(calls, t, steps, stype, B.wide_reference(k)[g], D.wide_pairs()[g], f"{W.NAMES[g]} times {k}", W.shared_row(g, RULE), g, wide_truth(g),
                     data_reference=B.wide_data_rows(k)[g], **kw)


@functools.lru_cache(maxsize=None)
def hook_log(check, *args):
    """what the hooks give under the checker `check`, computed once"""
    return tuple(CHECKS[check](HOST, *args))


def check_wide_law(calls, g, k, **kw):
    log = wide_chain_log(calls, g, k, **kw)
    assert_law(hook_log("wide chain", g, 1), log, k, outside_of(D.wide_pairs()[g], W.shapes()[g][0]), (W.NAMES[g], k))
    return log


def test_the_floors_of_the_families():
    """what big_amounts.py asserts on the oracles and the data alone, printed"""
    for k in B.FACTORS:
        B.wide_reference(k)
        B.wide_data_rows(k)
        B.structured_reference(k)
        B.structured_data_rows(k)
        B.cut_truth(k)
        for rule in B.ALL_RULES:
            B.adversarial_reference(k, rule)
            B.adversarial_data_rows(k, rule)
    B.irregular_reference()
    B.irregular_data_rows()


@pytest.mark.parametrize("k", B.FACTORS, ids=("K_HIGH", "K_SIGN"))
@pytest.mark.parametrize("g", range(len(W.NAMES)), ids=W.NAMES)
def test_wide_graphs_follow_the_oracle_and_the_law_on_the_host(g, k):
    check_wide_law(HOST, g, k)


# ---- 2: the structured graph: infinite sides, and what the data ranges mean at this magnitude
def structured_log(calls, k, **kw):
    """the chorded path with uncapacitated chords and self loops: the first solve and its queries"""
    t, stype = B.structured(k)
    pairs = B.structured_pairs()
    u = uniform_of(t, RULE, **kw)
    res = calls.first(u, t.arrays(), stype)
    assert_equals_answers(res, B.structured_reference(k), f"structured times {k}")
    oracles = [B.oracle_of(p, RULE, stype, trace_cap=0)[:2] for p in t.variants]
    truth = [truth_of(p, stype) for p in t.variants]
    return [("solve", to_numpy(res), counted(u.stats(), SOLVE_COUNTED))] + queries(calls, u, t, stype, res, pairs, f"structured times {k}", truth, oracles, B.structured_data_rows(k))


def check_structured_law(calls, k, **kw):
    log = structured_log(calls, k, **kw)
    t, _ = B.structured(1)
    assert_law(hook_log("structured", 1), log, k, outside_of(B.structured_pairs(), t.n), ("structured", k))
    infinite = sum(int(np.sum(rows[name] == D.INF)) for kind, rows, _ in log if kind == "data_ranges" for name in ("flow_down", "flow_up"))
    assert infinite >= 100, infinite
    return log


@pytest.mark.parametrize("k", B.FACTORS, ids=("K_HIGH", "K_SIGN"))
def test_the_structured_graph_follows_the_oracle_and_the_law_on_the_host(k):
    check_structured_law(HOST, k)


def meaning_case():
    """the first ranged variant of the chorded path, times K_HIGH: a probe moves a datum by its whole range, an amount above 2^32"""
    t, _, stype = B.wide(B.K_HIGH)[W.PATH]
    return t.variants[int(np.flatnonzero(B.wide_data_rows(B.K_HIGH)[W.PATH]["ranged"])[0])], stype


def test_a_datum_moved_by_its_range_keeps_the_basis_and_one_past_it_does_not_on_the_host():
    check_meaning(HOST.first, HOST.again, lambda u, pairs, **kw: u.data_ranges_on_host(pairs=pairs, **kw), meaning_case())


# ---- 3: cuts wider than a wave with a violation above 2^32
def cuts_log(calls, k, **kw):
    log = []
    wide_cuts = 0
    for i, (g, t) in enumerate(zip(B.CUT_GRAPHS, B.cut_family(k))):
        u = uniform_of(t, RULE, **kw)
        res = calls.first(u, t.arrays(), O.GEQ)
        r = to_numpy(res)
        d = diag_rows(calls.diagnose(u))
        for v, p in enumerate(t.variants):
            check_instance(p, O.GEQ, int(r["status"][v]), int(d["verdict"][v]), int(d["violation"][v]), int(d["set_size"][v]), d["side"][v], d["unmet"][v],
                           B.cut_truth(k)[i][v], (W.NAMES[g], k, v))
        wide_cuts += int(np.sum((d["verdict"] == VD.Cut) & (d["set_size"] > W.WAVE) & (d["violation"] > B.WORD)))
        log += [("solve", r, counted(u.stats(), SOLVE_COUNTED)), ("diagnose", d, counted(u.diagnose_stats(), DIAGNOSE_COUNTED))]
    print(f"cuts times {k}: {wide_cuts} cuts of more than {W.WAVE} nodes with a violation above 2^32, each checked by certificate_oracle.check_cut")
    assert k == 1 or wide_cuts >= 4, wide_cuts
    return log


def check_cuts_law(calls, k, **kw):
    log = cuts_log(calls, k, **kw)
    assert_law(hook_log("cuts", 1), log, k, None, ("cuts", k))
    return log


@pytest.mark.parametrize("k", B.FACTORS, ids=("K_HIGH", "K_SIGN"))
def test_cuts_wider_than_a_wave_follow_the_oracle_and_the_law_on_the_host(k):
    check_cuts_law(HOST, k)


# ---- 4: the adversarial family in one ragged handle, and in a BatchSolver
@functools.lru_cache(maxsize=None)
def adversarial_flat(k):
    return FlatNodes([p for p, _ in B.adversarial(k)])


def split_flat(flat, r):
    rows = dict(r)
    for name, at in (("flows", flat.arc_rows), ("potentials", flat.node_rows)):
        cut = np.empty(flat.count, object)
        for i in range(flat.count):
            cut[i] = r[name][at[i]:at[i + 1]]
        rows[name] = cut
    return rows


def assert_answer(rows, i, answer, what):
    st, pivots, tr, total, flows, potentials = answer
    assert rows["status"][i] == st and rows["pivots"][i] == pivots, (what, i, rows["status"][i], st, rows["pivots"][i], pivots)
    assert np.array_equal(rows["trace"][i][:pivots], tr) and not rows["trace"][i][pivots:].any(), (what, i)
    if st == O.OPTIMAL:
        assert rows["total_cost"][i] == total and np.array_equal(rows["flows"][i], flows) and np.array_equal(rows["potentials"][i], potentials), (what, i)
    else:
        assert rows["total_cost"][i] == 0 and not np.any(rows["flows"][i]) and not np.any(rows["potentials"][i]), (what, i)


def adversarial_log(calls, k, rule, **kw):
    """One ragged handle holds the 318 instances; a call has one supply type, so the handle is solved under each and every instance is
    held to the oracles under its own."""
    cases, refs, flat = B.adversarial(k), B.adversarial_reference(k, rule), adversarial_flat(k)
    pair_lists = list(B.adversarial_pairs())
    cost_ref, data_ref = R.reference_rows([(p, o, st) for (p, _), (o, st, _) in zip(cases, refs)]), B.adversarial_data_rows(k, rule)
    h = flat.handle(rule, record_trace=TRACE, **kw)
    log = []
    for stype in (O.GEQ, O.LEQ):
        what = ("adversarial", k, rule, stype)
        own = [i for i, (_, s) in enumerate(cases) if s == stype]
        res = calls.first(h, flat.arrays, stype)
        r = to_numpy(res)
        rows = split_flat(flat, r)
        for i in own:
            assert_answer(rows, i, refs[i][2], what)
        log.append(("solve", r, counted(h.stats(), SOLVE_COUNTED)))
        cr = range_rows(calls.ranges(h))
        for i in own:
            lo, hi = flat.arc_rows[i], flat.arc_rows[i + 1]
            assert cr["ranged"][i] == cost_ref[0][i], (what, i)
            for name, ref in (("arc_state", cost_ref[1]), ("cost_down", cost_ref[2]), ("cost_up", cost_ref[3])):
                assert np.array_equal(cr[name][lo:hi], ref[lo:hi]), (what, i, name)
        log.append(("cost_ranges", cr, counted(h.range_stats(), RANGE_COUNTED)))
        g = calls.data_ranges(h, pair_lists)
        assert_equals_reference(g, data_ref, flat.problems, pair_lists, h.data_range_stats(), what, only=set(own))
        log.append(("data_ranges", data_rows(g), counted(h.data_range_stats(), DATA_RANGE_COUNTED)))
        d = diag_rows(calls.diagnose(h))
        for i in own:
            p = cases[i][0]
            lo, hi = flat.node_rows[i], flat.node_rows[i + 1]
            assert (d["verdict"][i] == VD.NoVerdict) == (r["status"][i] == O.UNBOUNDED), (what, i)
            check_instance(p, stype, int(r["status"][i]), int(d["verdict"][i]), int(d["violation"][i]), int(d["set_size"][i]), d["side"][lo:hi], d["unmet"][lo:hi],
                           truth_of(p, stype), (what, i))
        log.append(("diagnose", d, counted(h.diagnose_stats(), DIAGNOSE_COUNTED)))
        got = rows_of(calls.validate(h, res, flat.arrays, stype))
        for i in own:
            if r["status"][i] != O.OPTIMAL:
                assert got["valid"][i] == 0 and got["errors"][i].sum() == 1, (what, i)
                continue
            p = cases[i][0]
            v = V.validate(p.n, p.src, p.tgt, p.lower, mapped_upper(p.upper), p.cost, p.supply, stype, rows["flows"][i], rows["potentials"][i], r["total_cost"][i])
            assert (got["valid"][i], got["objective"][i], got["dual_cost"][i]) == (v["valid"], v["objective"], v["dual_cost"]), (what, i)
            assert [int(e) for e in got["errors"][i]] == [v["errors"][name] for name in V.KINDS] and [int(e) for e in got["first"][i]] == [v["first"][name] for name in V.KINDS], (what, i)
        log.append(("validate", got, {}))
    return log


def adversarial_outside():
    return np.concatenate([outside_of(pairs, p.n) for pairs, (p, _) in zip(B.adversarial_pairs(), B.adversarial())])


def check_adversarial_law(calls, k, rule, **kw):
    log = adversarial_log(calls, k, rule, **kw)
    assert_law(hook_log("adversarial", 1, rule), log, k, adversarial_outside(), ("adversarial", k, rule))
    return log


@pytest.mark.parametrize("k", B.FACTORS, ids=("K_HIGH", "K_SIGN"))
@pytest.mark.parametrize("rule", B.ALL_RULES)
def test_the_adversarial_family_follows_the_oracle_and_the_law_on_the_host(rule, k):
    check_adversarial_law(HOST, k, rule)


def check_batch_solver(run, k, rule, **kw):
    """BatchSolver: every instance under its own supply type in one batch, bit for bit the oracle's"""
    cases, refs = B.adversarial(k), B.adversarial_reference(k, rule)
    b = M.BatchSolver(rule=RULES[rule], record_trace=TRACE, **kw)
    for p, stype in cases:
        b.add(p, supply_type=stype)
    run(b)
    got = batch_answers(b, len(cases))
    for i, (mine, (_, _, answer)) in enumerate(zip(got, refs)):
        assert mine[0] == answer[0] and mine[1] == answer[1] and np.array_equal(mine[2][:answer[1]], answer[2]), ("BatchSolver", k, rule, i)
        if answer[0] == O.OPTIMAL:
            assert mine[3] == answer[3] and np.array_equal(mine[4], answer[4]) and np.array_equal(mine[5], answer[5]), ("BatchSolver", k, rule, i)
    return got


@pytest.mark.parametrize("k", B.FACTORS, ids=("K_HIGH", "K_SIGN"))
@pytest.mark.parametrize("rule", B.ALL_RULES)
def test_the_adversarial_family_in_a_batch_solver_on_the_host(rule, k):
    check_batch_solver(HOST.batch, k, rule)


# ---- 5: the three GEQ wide graphs, big grid included, in one ragged handle
@functools.lru_cache(maxsize=None)
def ragged_mixes(k):
    """(mix of the first solve, of step a, of step c) as test_wide_host.ragged_mixes, every amount times k"""
    chains = [B.wide(k)[g] for g in RAGGED_GRAPHS]
    order = [(i, v) for v in range(W.PER) for i, (t, _, _) in enumerate(chains) if v < t.count]
    assert all(stype == O.GEQ for _, _, stype in chains)
    return Mix([t for t, _, _ in chains], order), Mix([steps[0] for _, steps, _ in chains], order), Mix([steps[2] for _, steps, _ in chains], order)


def ragged_queries(calls, h, mix, res, pair_lists):
    """the four queries on the ragged handle; here they are held to the law and to the hooks, the oracles have them on the uniform handles"""
    return [("cost_ranges", range_rows(calls.ranges(h)), counted(h.range_stats(), RANGE_COUNTED)),
            ("data_ranges", data_rows(calls.data_ranges(h, pair_lists)), counted(h.data_range_stats(), DATA_RANGE_COUNTED)),
            ("diagnose", diag_rows(calls.diagnose(h)), counted(h.diagnose_stats(), DIAGNOSE_COUNTED)),
            ("validate", rows_of(calls.validate(h, res, mix.arrays(), O.GEQ)), {})]


def ragged_log(calls, k, **kw):
    base, mix_a, mix_c = ragged_mixes(k)
    refs = [base.pick([B.wide_reference(k)[g][s] for g in RAGGED_GRAPHS]) for s in (0, 1, 3)]
    pair_lists = [D.wide_pairs()[g] for g in RAGGED_GRAPHS]
    h = base.handle(RULE, **kw)
    res = calls.first(h, base.arrays(), O.GEQ)
    assert_equals_answers(base.split(res), [answer for _, answer in refs[0]], ("ragged", k))
    log = [("solve", to_numpy(res), counted(h.stats(), SOLVE_COUNTED))] + ragged_queries(calls, h, base, res, pair_lists)
    for s, mix in ((1, mix_a), (2, mix_c)):
        res = calls.again(h, mix.arrays(), O.GEQ)
        assert_step(to_numpy(mix.split(res)), mix.problems(), O.GEQ, refs[s - 1], refs[s], h.resolve_data_stats(), ("ragged", k, s))
        log.append(("resolve_data", to_numpy(res), counted(h.resolve_data_stats(), REDATA_COUNTED)))
        log += ragged_queries(calls, h, mix, res, pair_lists)
    return log, h


def ragged_outside():
    base, _, _ = ragged_mixes(1)
    return np.concatenate([outside_of(D.wide_pairs()[RAGGED_GRAPHS[i]], base.tops[i].n) for i, _ in base.order])


def check_ragged_law(calls, k, **kw):
    log, h = ragged_log(calls, k, **kw)
    assert_law(hook_log("ragged", 1), log, k, ragged_outside(), ("ragged", k))
    return log, h


@pytest.mark.parametrize("k", B.FACTORS, ids=("K_HIGH", "K_SIGN"))
def test_one_ragged_handle_over_both_tiers_follows_the_oracle_and_the_law_on_the_host(k):
    check_ragged_law(HOST, k)


# ---- 6: the irregular family: no law, the oracles alone
def irregular_log(calls, i, **kw):
    g = B.SMALL_GRAPHS[i]
    t, steps, stype = B.irregular_family()[i]
    row = np.ascontiguousarray(B.oracle_of(t.variants[0], RULE, stype, trace_cap=0)[0].internal_arrays()["state"][:t.m].astype(np.int8))
    truths = [[truth_of(p, stype) for p in top.variants] for top in (t,) + steps]
    return run_chain(calls, t, steps, stype, B.irregular_reference()[i], B.irregular_pairs()[i], f"irregular {W.NAMES[g]}", row, 10 + g, truths,
                     data_reference=B.irregular_data_rows()[i], **kw)


@pytest.mark.parametrize("i", range(len(B.SMALL_GRAPHS)), ids=[W.NAMES[g] for g in B.SMALL_GRAPHS])
def test_the_irregular_family_follows_the_oracles_on_the_host(i):
    hook_log("irregular", i)


def irregular_ragged_log(calls, **kw):
    """the GEQ graphs of the irregular family (grid and hub) in one ragged handle: the first solve and both steps against the oracle"""
    picked = [i for i, (_, _, stype) in enumerate(B.irregular_family()) if stype == O.GEQ]
    chains = [B.irregular_family()[i] for i in picked]
    mixes = [Mix([((t,) + steps)[s] for t, steps, _ in chains]) for s in range(3)]
    refs = [mixes[0].pick([B.irregular_reference()[i][s] for i in picked]) for s in range(3)]
    h = mixes[0].handle(RULE, **kw)
    res = calls.first(h, mixes[0].arrays(), O.GEQ)
    assert_equals_answers(mixes[0].split(res), [answer for _, answer in refs[0]], "irregular, ragged")
    log = [("solve", to_numpy(res), counted(h.stats(), SOLVE_COUNTED))]
    for s in (1, 2):
        res = calls.again(h, mixes[s].arrays(), O.GEQ)
        assert_step(to_numpy(mixes[s].split(res)), mixes[s].problems(), O.GEQ, refs[s - 1], refs[s], h.resolve_data_stats(), ("irregular, ragged", s))
        log.append(("resolve_data", to_numpy(res), counted(h.resolve_data_stats(), REDATA_COUNTED)))
    return log


def test_the_irregular_family_in_one_ragged_handle_on_the_host():
    hook_log("irregular ragged")


CHECKS = {"wide chain": wide_chain_log, "structured": structured_log, "cuts": cuts_log, "adversarial": adversarial_log, "ragged": lambda calls, k: ragged_log(calls, k)[0],
          "irregular": irregular_log, "irregular ragged": irregular_ragged_log}


# ---- 7: the single-solve path (its entering-arc search exists on the device only: test_big_amounts_gpu.py runs this)
SINGLE = ("netgen_8_08a", "transport_40x30")


def check_single_solve(name, configure):
    """NetworkSimplex on a fixture and on the fixture times K_HIGH: the same pivots, flows and cost times K_HIGH, the same potentials,
    and the reference's validator passes both.  configure(ns) chooses where the searches run."""
    from helpers import load
    p = load(name)
    q = B.scaled(p, B.K_HIGH)
    runs = []
    for problem in (p, q):
        ns = configure(M.NetworkSimplex(problem.n, problem.src, problem.tgt).set_problem(problem.lower, problem.upper, problem.cost, problem.supply).set_pivot_rule(M.PivotRule.BlockSearch).enable_optimized_pivot(True)).record_trace(1 << 20)
        assert ns.solve() == O.OPTIMAL
        v = ns.validate()
        assert v["valid"] == 1 and not any(v["errors"].values()), (name, v)
        runs.append((ns.trace(), ns.flows(), ns.potentials(), ns.get_total_cost(), v))
    (tr, flows, pi, total, v), (tr_k, flows_k, pi_k, total_k, v_k) = runs
    assert len(tr) > 0 and np.array_equal(tr, tr_k) and np.array_equal(pi, pi_k), name
    assert np.array_equal(flows_k, times(flows, B.K_HIGH)) and total_k == total * B.K_HIGH < 1 << 62, name
    assert total_k == sum(int(f) * int(c) for f, c in zip(flows_k, q.cost)) and B.carried_high(flows_k), name
    assert (v_k["objective"], v_k["dual_cost"]) == (v["objective"] * B.K_HIGH, v["dual_cost"] * B.K_HIGH), name
    o, st, _ = B.oracle_of(q, RULE, O.GEQ, trace_cap=0)
    assert st == O.OPTIMAL and o.total_cost == total_k, name
    return len(tr), int(flows_k.max())
