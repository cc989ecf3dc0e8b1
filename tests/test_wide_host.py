"""Warm re-solves, cost ranges and given starts (DESIGN.md 3.14 "Re-solve with new data", "Cost ranges of the kept basis", "Start from a given
basis") on the graphs of wide_graphs.py without a GPU: connected graphs of 130 to 841 nodes with supplies on nodes >= 64 only, so that the
node-strided loops find their answer past the first stride of a wave, the trees are deeper than a wave is wide, and the big grid puts a
connected tree of hundreds of nodes into the global tier.  The hooks run the device's own steps with one lane on the CPU.

The references are those of test_redata_host.py, test_ranges_host.py and test_start_host.py, and so are the checkers where they take a
family: the oracle's cold solve, the brute force of ranges_oracle.py on the oracle's basis, start_oracle.classify().  The floors on the
graphs are asserted in wide_graphs.py on the oracle alone and printed from there.  Every checker here takes its calls as an argument and
runs under a recorder; test_wide_gpu.py runs the same checkers with the device's calls and compares what was recorded bit for bit."""
import collections
import functools

import numpy as np
import pytest

from oracle import ns_oracle as O

import start_oracle as S
import wide_graphs as W
from test_ragged_host import Mix
from test_ranges_host import FIELDS, INF, check_meaning, range_rows, redata
from test_redata_host import assert_step, check_mixed_with_new_costs
from test_start_host import assert_start
from test_uniform_host import assert_equals_answers, assert_rows_equal, to_numpy, uniform_of

RULE = O.RULE_BLOCK
SMALL_GRAPHS = (W.PATH, W.GRID, W.HUB)
RAGGED_GRAPHS = (W.HUB, W.GRID, W.BIG)         # in this order in the handle; all of supply type GEQ
REDATA_COUNTED = ("warm_instances", "cold_instances", "fallback_instances", "untouched_instances", "dual_pivots", "primal_pivots")
START_COUNTED = ("primal_starts", "dual_starts", "cold_instances", "fallback_instances", "dual_pivots", "primal_pivots")
RANGE_COUNTED = ("instances", "ranged", "tree_arcs", "cycle_hops")
BIG_SHARED_DATA = (0, 1, 3)                    # the big grid's shared row meets the first solve's data and steps a and c only: its cold rows are solves of 2 000 pivots

Calls = collections.namedtuple("Calls", "first again recost ranges start")
HOST = Calls(first=lambda u, a, stype: u.run_on_host(supply_type=stype, **a),
             again=lambda u, a, stype, **kw: u.rerun_data_on_host(supply_type=stype, **a, **kw),
             recost=lambda u, a, stype, **kw: u.rerun_on_host(supply_type=stype, **a, **kw),
             ranges=lambda u, **kw: u.cost_ranges_on_host(**kw),
             start=lambda u, rows, a, stype: u.run_from_on_host(rows, supply_type=stype, **a))


class Recorded:
    """Calls that keep what every call returned and counted: log = [(kind, rows, counted statistics) ...]"""

    def __init__(self, calls):
        self.calls, self.log = calls, []

    def note(self, kind, rows, stats=None, fields=()):
        self.log.append((kind, rows, {f: stats[f] for f in fields}))

    def first(self, u, a, stype):
        r = self.calls.first(u, a, stype)
        self.note("solve", to_numpy(r))
        return r

    def again(self, u, a, stype, **kw):
        r = self.calls.again(u, a, stype, **kw)
        self.note("resolve_data", to_numpy(r), u.resolve_data_stats(), REDATA_COUNTED)
        return r

    def recost(self, u, a, stype, **kw):
        r = self.calls.recost(u, a, stype, **kw)
        self.note("resolve", to_numpy(r))
        return r

    def ranges(self, u, **kw):
        g = self.calls.ranges(u, **kw)
        self.note("cost_ranges", range_rows(g), u.range_stats(), RANGE_COUNTED if kw.get("costs", True) else RANGE_COUNTED[:2])
        return g

    def start(self, u, rows, a, stype):
        r = self.calls.start(u, rows, a, stype)
        self.note("solve_from", to_numpy(r), u.start_stats(), START_COUNTED)
        return r


def assert_same_log(mine, theirs, what=""):
    assert [kind for kind, _, _ in mine] == [kind for kind, _, _ in theirs], what
    for c, ((kind, a, sa), (_, b, sb)) in enumerate(zip(mine, theirs)):
        assert a.keys() == b.keys()
        for name in a:
            assert (a[name] is None) == (b[name] is None), (what, c, kind, name)
            assert a[name] is None or (a[name].dtype == b[name].dtype and np.array_equal(a[name], b[name])), (what, c, kind, name)
        assert sa == sb, (what, c, kind, sa, sb)


def graph(g):
    (t, steps), (_, stype) = W.wide_chain()[g], W.wide_family()[g]
    return t, steps, stype, W.wide_reference(RULE)[g]


def test_the_floors_of_the_graphs():
    """what wide_graphs.py asserts on the oracle and the data alone, printed: warm candidates and forced dual pivots per step, first leaving
    nodes on both sides of node 64, tree depths, crossing arcs, tiers, the ranges' tally and the classes of the shared row"""
    assert len(W.wide_reference(RULE)) == len(W.wide_ranges(RULE)) == len(W.start_classes(RULE)) == len(W.NAMES)
    W.hostile_case()
    W.meaning_problem()


# ---- 1: first solve, ranges of the oracle's basis, the four steps, ranges of a warm basis, the round trip
def assert_ranges_of_first_solve(g, got, stats, t):
    """every row against the brute force on the oracle's basis, none left out"""
    ranged, state, down, up, _ = W.wide_ranges(RULE)[g]
    rows = range_rows(got)
    assert rows["arc_state"].shape == rows["cost_down"].shape == rows["cost_up"].shape == (t.count, t.m) and rows["ranged"].shape == (t.count,)
    assert rows["ranged"].dtype == np.int32 and rows["arc_state"].dtype == np.int8 and rows["cost_down"].dtype == rows["cost_up"].dtype == np.int64
    assert np.array_equal(rows["ranged"], ranged), W.NAMES[g]
    for name, ref in (("arc_state", state), ("cost_down", down), ("cost_up", up)):
        differ = np.flatnonzero(rows[name].reshape(-1) != ref)
        assert not len(differ), (W.NAMES[g], name, differ[:8] // t.m, differ[:8] % t.m)
    assert stats["instances"] == t.count and stats["ranged"] == int(ranged.sum()) and stats["cycle_hops"] > 0, stats
    assert stats["tree_arcs"] == int(np.sum(state.reshape(t.count, t.m)[ranged == 1] == S.TREE)), stats


def assert_ranges_of_a_warm_basis(got, r, problems, stype, refs, what):
    """The basis is the batch's own: ranged exactly where the oracle's cold solve is Optimal and conserves flow; there the states agree
    with the flows, the row is a primal start for start_oracle, a non-tree arc's range is its reduced cost under the returned potentials
    on one side and unbounded on the other, and a tree arc's sides are not negative.  Rows that are not ranged are zero."""
    rows = range_rows(got)
    for k, (p, (ref, _)) in enumerate(zip(problems, refs)):
        state, down, up = rows["arc_state"][k], rows["cost_down"][k], rows["cost_up"][k]
        assert bool(rows["ranged"][k]) == (ref[0] == O.OPTIMAL and ref[2] is None), (what, k)
        if not rows["ranged"][k]:
            assert not state.any() and not down.any() and not up.any(), (what, k)
            continue
        flows, pi = r["flows"][k], r["potentials"][k]
        assert np.all(flows[state == S.LOWER] == p.lower[state == S.LOWER]) and np.all(flows[state == S.UPPER] == p.upper[state == S.UPPER]), (what, k)
        assert S.classify(p, stype, state).kind == S.PRIMAL, (what, k)
        rc = p.cost + pi[p.src] - pi[p.tgt]
        assert np.all(rc[state == S.TREE] == 0), (what, k)
        assert np.all(down[state == S.LOWER] == rc[state == S.LOWER]) and np.all(up[state == S.LOWER] == INF), (what, k)
        assert np.all(up[state == S.UPPER] == -rc[state == S.UPPER]) and np.all(down[state == S.UPPER] == INF), (what, k)
        assert np.all(down >= 0) and np.all(up >= 0), (what, k)


def check_steps(calls, g, **kw):
    t, steps, stype, refs = graph(g)
    u = uniform_of(t, RULE, **kw)
    r = calls.first(u, t.arrays(), stype)
    assert_equals_answers(r, [answer for _, answer in refs[0]], f"{W.NAMES[g]}, first solve")
    got = calls.ranges(u)
    assert_ranges_of_first_solve(g, got, u.range_stats(), t)
    assert np.array_equal(range_rows(got)["arc_state"][0], W.shared_row(g, RULE))
    dual = {}
    for s, name in enumerate(W.STEPS):
        what = f"{W.NAMES[g]}, step {name}"
        r = to_numpy(calls.again(u, steps[s].arrays(), stype))
        dual[name], _ = assert_step(r, steps[s].variants, stype, refs[s], refs[s + 1], u.resolve_data_stats(), what)
        if name in ("a", W.STEPS[-1]):
            assert_ranges_of_a_warm_basis(calls.ranges(u), r, steps[s].variants, stype, refs[s + 1], what)
    print(f"{W.NAMES[g]}: dual pivots per step {dual}")
    assert all(d > 0 for d in dual.values()), (W.NAMES[g], dual)
    # the round trip: the basis the last step left, exported, starts a fresh handle on the same data with no pivot
    export = calls.ranges(u, costs=False)
    ranged, rows = range_rows(export)["ranged"].astype(bool), range_rows(export)["arc_state"]
    v = uniform_of(t, RULE, **kw)
    back = to_numpy(calls.start(v, export.arc_state, steps[-1].arrays(), stype))
    assert_start(back, steps[-1].variants, stype, rows, refs[-1], v.start_stats(), f"{W.NAMES[g]}, round trip")
    spanning = [k for k in np.flatnonzero(ranged) if S.count_tree(rows[k]) == t.n - 1]
    print(f"{W.NAMES[g]}: round trip of {int(ranged.sum())} ranged rows, {len(spanning)} of them spanning trees")
    assert len(spanning) >= 1
    for k in np.flatnonzero(ranged):
        assert back["status"][k] == r["status"][k] == O.OPTIMAL and back["total_cost"][k] == r["total_cost"][k], (W.NAMES[g], k)
        if k in spanning:               # a forest is hung on artificial arcs anew: its potentials, and so its pivots, may differ
            assert back["pivots"][k] == 0 and not back["trace"][k].any() and np.array_equal(back["flows"][k], r["flows"][k]), (W.NAMES[g], k, back["pivots"][k])
    assert np.array_equal(range_rows(calls.ranges(v, costs=False))["arc_state"][spanning], rows[spanning])
    return u


@functools.lru_cache(maxsize=None)
def hook_log(check, *args):
    """what the hooks return and count under the checker `check`, computed once"""
    rec = Recorded(HOST)
    CHECKS[check](rec, *args)
    return tuple(rec.log)


@pytest.mark.parametrize("g", range(len(W.NAMES)), ids=W.NAMES)
def test_steps_ranges_and_round_trip_on_the_host(g):
    hook_log("steps", g)


# ---- 2: the cost step
def check_cost_step(calls, g, **kw):
    t, steps, stype, _ = graph(g)
    check_mixed_with_new_costs(calls.first, calls.again, calls.recost, RULE, graphs=(((t, steps), stype),), **kw)


@pytest.mark.parametrize("g", range(len(W.NAMES)), ids=W.NAMES)
def test_mixed_with_new_costs_on_the_host(g):
    hook_log("cost step", g)


# ---- 3: what the ranges mean, on a circulation over the grid of 12 x 12
def check_meaning_on_the_grid(calls, reference=None):
    solve, resolve = (lambda u, a: calls.first(u, a, O.GEQ)), (lambda u, a: calls.recost(u, a, O.GEQ))
    check_meaning(solve, resolve, calls.ranges, reference=reference, problem=W.meaning_problem())
    check_meaning(solve, resolve, calls.ranges, between=redata(lambda u, a: calls.again(u, a, O.GEQ)), reference=reference, problem=W.meaning_problem())


def test_a_cost_inside_its_range_makes_no_pivot_and_one_past_it_does_on_the_host():
    check_meaning_on_the_grid(HOST)


# ---- 4: one shared row for all variants, and hostile rows on the chorded path
def check_shared_row(calls, g, **kw):
    t, steps, stype, refs = graph(g)
    row, classes = W.shared_row(g, RULE), W.start_classes(RULE)[g]
    for s, top in enumerate((t,) + steps):
        if g == W.BIG and s not in BIG_SHARED_DATA:
            continue
        u, last = uniform_of(t, RULE, **kw), top
        r = to_numpy(calls.start(u, row, top.arrays(), stype))
        kinds = assert_start(r, top.variants, stype, [row] * t.count, refs[s], u.start_stats(), f"{W.NAMES[g]}, shared row, data {s}")
        assert tuple(kinds) == classes[s]
        if s == 0:
            assert r["pivots"][0] == 0 and np.array_equal(r["flows"][0], refs[0][0][1][4])
    # a row each gives what the shared row gives
    tiled = uniform_of(t, RULE, **kw)
    assert_rows_equal(calls.start(tiled, np.ascontiguousarray(np.tile(row, (t.count, 1))), last.arrays(), stype), u._last, "a row each")


@pytest.mark.parametrize("g", range(len(W.NAMES)), ids=W.NAMES)
def test_one_shared_row_on_the_host(g):
    hook_log("shared row", g)


def check_hostile_rows(calls, **kw):
    from test_batch_resolve_host import cold_reference
    from test_uniform_host import answer_of
    top, stype, cycle, forward = W.hostile_case()
    refs = tuple((cold_reference(p, stype, RULE), answer_of(p, RULE, stype)) for p in top.variants)
    for name, row in (("a cycle of more than 64 arcs", cycle), ("the forward path", forward)):
        u = uniform_of(top, RULE, **kw)
        r = to_numpy(calls.start(u, row, top.arrays(), stype))
        kinds = assert_start(r, top.variants, stype, [row] * top.count, refs, u.start_stats(), name)
        assert (kinds.count(S.COLD) == top.count) if row is cycle else (kinds[-1] == S.PRIMAL), (name, kinds)


def test_hostile_rows_on_the_chorded_path_on_the_host():
    hook_log("hostile rows")


# ---- 5: one ragged handle over the hub, the grid of 12 x 12 and the big grid
@functools.lru_cache(maxsize=None)
def ragged_mixes():
    """(mix of the first solve, of step a, of step c): every variant of the three graphs, interleaved while a graph has variants left"""
    chains = [W.wide_chain()[g] for g in RAGGED_GRAPHS]
    order = [(i, v) for v in range(W.PER) for i, (t, _) in enumerate(chains) if v < t.count]
    assert all(W.wide_family()[g][1] == O.GEQ for g in RAGGED_GRAPHS)
    return Mix([t for t, _ in chains], order), Mix([steps[0] for _, steps in chains], order), Mix([steps[2] for _, steps in chains], order)


def check_ragged(calls, **kw):
    """first solve -> step a -> ranges -> step c -> solve_from of its own export: the oracle per step, and row for row what a uniform handle
    per graph gives for the same calls.  Returns the handles of the steps and of the start."""
    base, mix_a, mix_c = ragged_mixes()
    refs = [base.pick([W.wide_reference(RULE)[g][s] for g in RAGGED_GRAPHS]) for s in (0, 1, 3)]
    h = base.handle(RULE, **kw)
    got = [calls.first(h, base.arrays(), O.GEQ)]
    got.append(calls.again(h, mix_a.arrays(), O.GEQ))
    assert_step(to_numpy(mix_a.split(got[-1])), mix_a.problems(), O.GEQ, refs[0], refs[1], h.resolve_data_stats(), "ragged, step a")
    ranges = range_rows(calls.ranges(h))
    got.append(calls.again(h, mix_c.arrays(), O.GEQ))
    assert_step(to_numpy(mix_c.split(got[-1])), mix_c.problems(), O.GEQ, refs[1], refs[2], h.resolve_data_stats(), "ragged, step c")
    export = calls.ranges(h, costs=False)
    h2 = base.handle(RULE, **kw)
    got.append(calls.start(h2, export.arc_state, mix_c.arrays(), O.GEQ))
    flat = range_rows(export)["arc_state"]
    assert_start(to_numpy(mix_c.split(got[-1])), mix_c.problems(), O.GEQ, [flat[base.arc_rows[i]:base.arc_rows[i + 1]] for i in range(base.count)], refs[2],
                 h2.start_stats(), "ragged, start")
    for i, g in enumerate(RAGGED_GRAPHS):
        t, steps, stype, _ = graph(g)
        u = uniform_of(t, RULE, **kw)
        mine = [calls.first(u, t.arrays(), stype), calls.again(u, steps[0].arrays(), stype)]
        uniform_ranges = range_rows(calls.ranges(u))
        mine.append(calls.again(u, steps[2].arrays(), stype))
        uniform_export = calls.ranges(u, costs=False)
        mine.append(calls.start(uniform_of(t, RULE, **kw), uniform_export.arc_state, steps[2].arrays(), stype))
        for c, (ragged, uniform) in enumerate(zip(got, mine)):
            assert_rows_equal(base.of_graph(ragged, i), uniform, (W.NAMES[g], "call", c))
        at = sorted((v, k) for k, (gg, v) in enumerate(base.order) if gg == i)
        for v, k in at:
            lo, hi = base.arc_rows[k], base.arc_rows[k + 1]
            assert ranges["ranged"][k] == uniform_ranges["ranged"][v], (W.NAMES[g], v)
            for name in FIELDS[1:]:
                assert np.array_equal(ranges[name][lo:hi], uniform_ranges[name][v]), (W.NAMES[g], v, name)
            assert np.array_equal(flat[lo:hi], range_rows(uniform_export)["arc_state"][v]), (W.NAMES[g], v)
    return h, h2


def test_one_ragged_handle_equals_the_uniform_handles_on_the_host():
    hook_log("ragged")


CHECKS = {"steps": check_steps, "cost step": check_cost_step, "shared row": check_shared_row, "hostile rows": check_hostile_rows, "ragged": check_ragged}
