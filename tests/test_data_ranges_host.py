"""Supply and bound ranges of the kept basis (mcf_ubatch_data_ranges_on_host / mcf_rbatch_data_ranges_on_host, DESIGN.md 3.14 "Supply and
bound ranges of the kept basis") without a GPU: the hooks run the device's own step (csrc/data_ranges_step.hip.h) with one lane on the CPU.

Every comparison is exact.  The reference is data_ranges_oracle.py on the oracle's own basis (its floors are asserted there); what the
numbers MEAN is checked through the existing re-solve with new data: a datum moved by exactly its range makes no pivot and keeps the
basis, one moved one unit further does not keep it.  test_data_ranges_gpu.py imports the batches and the checkers from here."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mincostflow_amd as M
from mincostflow_amd import _lib as L
from oracle import ns_oracle as O

import data_ranges_oracle as D
import wide_graphs as W
from helpers import validate_solution
from test_batch_host import ROOT, RULES, fuzz_cases
from test_batch_resolve_host import cold_reference
from test_ranges_host import Flat, fuzz_flat, small_case
from test_redata_host import PADDED_NODES, redata_family
from test_uniform_host import ALL_RULES, TRACE, assert_row_matches_cold, to_numpy, uniform_of

INF = M.RANGE_INF
FIELDS = ("ranged", "arc_state", "flow_down", "flow_up", "ship_forth", "ship_back")
DTYPES = dict(ranged=np.int32, arc_state=np.int8, flow_down=np.int64, flow_up=np.int64, ship_forth=np.int64, ship_back=np.int64)
PROBLEM_FIELDS = ("cost", "supply", "lower", "upper")


def data_rows(g):
    """a result's rows as flat numpy arrays, wherever they are"""
    get = lambda a: None if a is None else (a if isinstance(a, np.ndarray) else a.cpu().numpy()).reshape(-1)
    return {name: get(getattr(g, name)) for name in FIELDS}


def assert_same_data_ranges(a, b, what=""):
    a, b = data_rows(a), data_rows(b)
    for name in FIELDS:
        assert (a[name] is None) == (b[name] is None), (what, name)
        assert a[name] is None or (a[name].dtype == b[name].dtype and np.array_equal(a[name], b[name])), (what, name)


def assert_equals_reference(g, ref, problems, pair_lists, stats, what, only=None):
    """A result against data_ranges_oracle.reference_rows(): every row exact for the instances `only` (default: all), zero rows where
    not ranged, the ship rows of every third arc equal to that arc's flow rows where it is not in the tree, the statistics counted anew."""
    rows = data_rows(g)
    arc_rows = np.concatenate([[0], np.cumsum([p.m for p in problems])])
    ship_rows = ref["ship_rows"]
    assert rows["ranged"].shape == (len(problems),) and rows["arc_state"].shape == rows["flow_down"].shape == rows["flow_up"].shape == (arc_rows[-1],), what
    assert rows["ship_forth"].shape == rows["ship_back"].shape == (ship_rows[-1],), what
    walks = 0
    for name in FIELDS:
        assert rows[name].dtype == DTYPES[name], (what, name)
    for i, (p, pairs) in enumerate(zip(problems, pair_lists)):
        arcs, ships = slice(arc_rows[i], arc_rows[i + 1]), slice(ship_rows[i], ship_rows[i + 1])
        if not rows["ranged"][i]:
            assert not any(rows[name][arcs].any() for name in FIELDS[1:4]) and not any(rows[name][ships].any() for name in FIELDS[4:]), (what, i)
        else:
            inside = np.all((pairs >= 0) & (pairs < p.n), axis=1)
            walks += int(np.sum(rows["arc_state"][arcs] != 0)) + int(inside.sum())
            third, at = D.third_arcs(p.m)
            off_tree = rows["arc_state"][arcs][third] != 0
            assert np.array_equal(rows["ship_forth"][ships][at][off_tree], rows["flow_down"][arcs][third][off_tree]), (what, i)
            assert np.array_equal(rows["ship_back"][ships][at][off_tree], rows["flow_up"][arcs][third][off_tree]), (what, i)
            same = pairs[:, 0] == pairs[:, 1]
            assert np.all(rows["ship_forth"][ships][~inside] == -1) and np.all(rows["ship_back"][ships][~inside] == -1), (what, i)
            assert np.all(rows["ship_forth"][ships][same & inside] == INF) and np.all(rows["ship_back"][ships][same & inside] == INF), (what, i)
        if only is not None and i not in only:
            continue
        assert rows["ranged"][i] == ref["ranged"][i], (what, i)
        for name in FIELDS[1:4]:
            assert np.array_equal(rows[name][arcs], ref[name][arcs]), (what, i, name)
        for name in FIELDS[4:]:
            assert np.array_equal(rows[name][ships], ref[name][ships]), (what, i, name)
    assert stats["instances"] == len(problems) and stats["ranged"] == int(rows["ranged"].sum()) and stats["walks"] == walks, (what, stats, walks)
    assert (stats["hops"] > 0) == (walks > 0), (what, stats)
    return rows


HOST_SOLVE = lambda h, a, stype: h.run_on_host(supply_type=stype, **a)
HOST_RANGES = lambda h, pairs, **kw: h.data_ranges_on_host(pairs=pairs, **kw)
HOST_ONLY = lambda st: st["lds_instances"] == st["global_instances"] == st["bytes_up"] == st["bytes_down"] == 0


# ---- 1: the rows against the reference
def uniform_cases(rule):
    """((topology, supply type, pairs, reference rows, name) ...): the re-data family, the wide family and the structured graph"""
    out = [(t, stype, pairs, rows, f"re-data graph {j}") for j, ((t, stype), (pairs, rows)) in enumerate(zip(redata_family(), D.redata_rows(rule)))]
    out += [(t, stype, D.wide_pairs()[g], rows, W.NAMES[g]) for g, ((t, stype), rows) in enumerate(zip(W.wide_family(), D.wide_rows(rule)))]
    out.append(D.structured_family() + D.structured_rows(rule) + ("chorded path without chord capacities",))
    return out


def check_uniform_families(solve, ranges, rule, check_stats=lambda st: True, **kw):
    for t, stype, pairs, ref, name in uniform_cases(rule):
        u = uniform_of(t, rule, **kw)
        solve(u, t.arrays(), stype)
        g = ranges(u, pairs)
        assert tuple(g.flow_down.shape) == (t.count, t.m) and tuple(g.ship_forth.shape) == (t.count, len(pairs))
        st = u.data_range_stats()
        rows = assert_equals_reference(g, ref, t.variants, [pairs] * t.count, st, (name, rule))
        assert check_stats(st), st
        lower, upper = t.stack("lower").reshape(-1), t.stack("upper").reshape(-1)
        want = D.bounds_table(ref, lower, upper)
        for got, row in zip(g.bounds(t.stack("lower"), t.stack("upper")), want):
            got = got if isinstance(got, np.ndarray) else got.cpu().numpy()
            assert got.dtype == np.int64 and np.array_equal(got.reshape(-1), row), (name, rule)
        yield u, t, stype, pairs, g, rows


@pytest.mark.parametrize("rule", ALL_RULES)
def test_uniform_families_equal_the_reference_on_the_host(rule):
    for _ in check_uniform_families(HOST_SOLVE, HOST_RANGES, rule, HOST_ONLY):
        pass


def check_adversarial_batch(solve, ranges, rule, check_stats=lambda st: True):
    """One ragged handle holds every instance, each with its own pair list; a call has one supply type, so the handle is solved under
    each and every instance is compared under its own."""
    flat, ref, pair_lists = fuzz_flat(), D.fuzz_rows(rule), list(D.fuzz_pairs())
    stypes = [s for _, s in fuzz_cases()]
    h = flat.handle(rule)
    for stype in (O.GEQ, O.LEQ):
        solve(h, flat.arrays, stype)
        g = ranges(h, pair_lists)
        st = h.data_range_stats()
        assert_equals_reference(g, ref, flat.problems, pair_lists, st, ("adversarial", rule, stype), only={k for k, s in enumerate(stypes) if s == stype})
        assert check_stats(st), st
        assert np.array_equal(g.ship_rows, ref["ship_rows"]) and len(g.ships(3)[0]) == len(pair_lists[3]) and len(g.arcs(3)[1]) == flat.problems[3].m
        want = D.bounds_table(dict(ref, **{k: v for k, v in data_rows(g).items() if k in ("arc_state", "flow_down", "flow_up")},
                                   ranged_arcs=np.repeat(data_rows(g)["ranged"] != 0, [p.m for p in flat.problems])), flat.arrays["lower"], flat.arrays["upper"])
        for got, row in zip(g.bounds(flat.arrays["lower"], flat.arrays["upper"]), want):
            got = got if isinstance(got, np.ndarray) else got.cpu().numpy()
            assert np.array_equal(got, row), (rule, stype)
        yield h, g


@pytest.mark.parametrize("rule", ALL_RULES)
def test_adversarial_batch_equals_the_reference_on_the_host(rule):
    for _ in check_adversarial_batch(HOST_SOLVE, HOST_RANGES, rule, HOST_ONLY):
        pass


def three_graphs(rule):
    """(Flat of the 12 x 12 grid's, the hub's and the big grid's variants -- the graphs of wide_graphs that share GEQ --, graphs, graph_of,
    pair lists per graph, reference rows)"""
    graphs = (W.GRID, W.HUB, W.BIG)
    tops = [W.wide_family()[g][0] for g in graphs]
    problems = [p for t in tops for p in t.variants]
    rows = [D.wide_rows(rule)[g] for g in graphs]
    ref = {name: np.concatenate([r[name] for r in rows]) for name in FIELDS + ("ranged_arcs",)}
    ref["ship_rows"] = np.concatenate([[0], np.cumsum([len(D.wide_pairs()[g]) for g, t in zip(graphs, tops) for _ in t.variants])])
    return Flat(problems), [(t.n, t.src, t.tgt) for t in tops], np.repeat(np.arange(3), [t.count for t in tops]).astype(np.int32), [D.wide_pairs()[g] for g in graphs], ref


def two_tiers():
    """three_graphs() and a graph of 9 nodes padded to PADDED_NODES isolated ones: (Flat, graphs, graph_of, pair lists per graph).  On the
    device 16 of the 24 instances are solved in LDS, the rest in place."""
    flat, graphs, graph_of, pair_lists, _ = three_graphs(O.RULE_BLOCK)
    t, stype = redata_family()[3]
    assert stype == O.GEQ
    small = [O.Problem(PADDED_NODES, p.m, p.src, p.tgt, p.lower, p.upper, p.cost, np.concatenate([p.supply, np.zeros(PADDED_NODES - p.n, np.int64)])) for p in t.variants[:4]]
    pairs = np.ascontiguousarray(np.concatenate([D.pairs_of((8,), t.n, t.src, t.tgt), [[PADDED_NODES - 1, 0], [PADDED_NODES, 0]]]).astype(np.int32))
    return (Flat(flat.problems + tuple(small)), graphs + [(PADDED_NODES, t.src, t.tgt)], np.concatenate([graph_of, np.full(4, 3, np.int32)]).astype(np.int32),
            pair_lists + [pairs])


def check_three_graphs(solve, ranges, rule=O.RULE_BLOCK, **kw):
    flat, graphs, graph_of, pair_lists, ref = three_graphs(rule)
    h = M.RaggedBatch(graphs, graph_of=graph_of, rule=RULES[rule], **kw)
    solve(h, flat.arrays, O.GEQ)
    g = ranges(h, pair_lists)
    assert_equals_reference(g, ref, flat.problems, [pair_lists[k] for k in graph_of], h.data_range_stats(), "three graphs in one handle")
    return h, g


def test_three_graphs_in_one_ragged_handle_on_the_host():
    check_three_graphs(HOST_SOLVE, HOST_RANGES)


# ---- 2: what the numbers mean
def moved(p, what, e, d):
    """problem p with one datum moved by d: a bound of arc e, or d units of supply from node e[1] to node e[0]"""
    lower, upper, supply = p.lower.copy(), p.upper.copy(), p.supply.copy()
    if what == "lower":
        lower[e] += d
    elif what == "upper":
        upper[e] += d
    else:
        supply[e[0]] += d
        supply[e[1]] -= d
    return O.Problem(p.n, p.m, p.src, p.tgt, lower, upper, p.cost, supply)


def probes_of(p, state, down, up, pairs, forth, back):
    """((what, arc or pair, sign, range) ...): both sides of the bound every non-tree arc sits at, the two finite sides of every tree
    arc's bounds, both directions of the pairs; the table of include/mcf_hip.h by hand"""
    out = []
    for e in range(p.m):
        cap = int(p.upper[e] - p.lower[e])
        assert p.upper[e] != O.INF_CAP
        if state[e] == 1:
            out += [("lower", e, -1, int(down[e])), ("lower", e, 1, min(int(up[e]), cap))]
        elif state[e] == -1:
            out += [("upper", e, -1, min(int(down[e]), cap)), ("upper", e, 1, int(up[e]))]
        else:
            out += [("lower", e, 1, int(down[e])), ("upper", e, -1, int(up[e]))]
    for (a, b), f, k in zip(pairs.tolist(), forth.tolist(), back.tolist()):
        out += [("supply", (a, b), 1, f), ("supply", (a, b), -1, k)]
    return out


def meaning_cases(rule=O.RULE_BLOCK):
    """(problem, supply type) twice: the first ranged variant of the re-data family's graph of 9 nodes and 54 arcs, and of the chorded path"""
    out = []
    for (t, stype), ranged in ((redata_family()[3], D.redata_rows(rule)[3][1]["ranged"]), (W.wide_family()[W.PATH], D.wide_rows(rule)[W.PATH]["ranged"])):
        out.append((t.variants[int(np.flatnonzero(ranged)[0])], stype))
    return out


def check_meaning(solve, resolve_data, ranges, case, rule=O.RULE_BLOCK, reference=None, **kw):
    """A UniformBatch of identical instances, one per probe, solved once.  Inside: instance k moves its one datum by exactly its range.
    Outside: from a freshly solved handle, by one unit more, for every finite probe that does not invert the arc's bounds."""
    p, stype = case
    pairs = np.ascontiguousarray(np.random.default_rng([D.PAIR_SEED, 9, p.n]).integers(0, p.n, (20, 2)).astype(np.int32))
    base = {f: getattr(p, f) for f in PROBLEM_FIELDS}
    probes = None
    seen = dict(inside=0, outside=0, zero=0, without_capacity=0)
    for past in (0, 1):
        count = 1 if probes is None else len(probes)
        for attempt in range(2 if probes is None else 1):             # the first handle only tells how many probes there are
            u = M.UniformBatch(p.n, p.src, p.tgt, count, rule=RULES[rule], record_trace=TRACE, **kw)
            r0 = to_numpy(solve(u, base, stype))
            assert np.all(r0["status"] == O.OPTIMAL)
            g = ranges(u, pairs)
            rows = data_rows(g)
            assert rows["ranged"].all()
            if probes is None:
                state, down, up = (rows[name][:p.m] for name in FIELDS[1:4])
                probes = probes_of(p, state, down, up, pairs, rows["ship_forth"][:len(pairs)], rows["ship_back"][:len(pairs)])
                count = len(probes)
        for name in FIELDS[1:]:
            assert np.all(rows[name].reshape(count, -1) == rows[name].reshape(count, -1)[0]), name
        if reference is not None:
            assert_same_data_ranges(g, reference(u, pairs), "against the hook")
        problems, live = [], np.zeros(count, bool)
        for k, (what, e, sign, room) in enumerate(probes):
            d = room + past if room != INF else (0 if past else 1000)
            q = moved(p, what, e, sign * d) if room >= 0 else p
            live[k] = room >= 0 and not (past and (room == INF or np.any(q.upper < q.lower)))
            problems.append(q if live[k] else p)
            seen["zero"] += live[k] and room == 0 and not past
        arrays = {f: np.ascontiguousarray(np.stack([getattr(q, f) for q in problems])) for f in PROBLEM_FIELDS}
        r = to_numpy(resolve_data(u, arrays, stype))
        st = u.resolve_data_stats()
        after = data_rows(ranges(u, None, flows=False))
        same_basis = (after["ranged"] == 1) & np.all(after["arc_state"].reshape(count, p.m) == state, axis=1)
        refs = {}
        for k, q in enumerate(problems):
            key = probes[k] if live[k] else None
            if key not in refs:
                refs[key] = cold_reference(q, stype, rule)
            if np.all(q.upper > q.lower) or r["status"][k] != O.OPTIMAL:
                assert_row_matches_cold(r, k, q, stype, refs[key], (probes[k], past))
            else:
                # The probe leaves an arc without capacity (a bound moved by the arc's whole capacity), which is outside the limit stated at
                # mcf_batch_resolve: there the reference may answer Unbounded on a path the warm start never takes.  Optimal is then checked
                # by what it means: the returned flows and potentials are an optimal pair of the moved problem at the returned cost.
                seen["without_capacity"] += 1
                assert validate_solution(q, r["flows"][k], r["potentials"][k], stype) == r["total_cost"][k], (probes[k], past)
                assert refs[key][0] != O.OPTIMAL or refs[key][1] == r["total_cost"][k], (probes[k], past)
        if not past:
            assert not r["pivots"].any(), [probes[k] for k in np.flatnonzero(r["pivots"])]
            assert st["warm_instances"] == count and st["dual_pivots"] == st["primal_pivots"] == st["fallback_instances"] == st["cold_instances"] == 0, st
            assert same_basis.all(), [probes[k] for k in np.flatnonzero(~same_basis)]
            seen["inside"] = int(live.sum())
        else:
            assert not same_basis[live].any(), [probes[k] for k in np.flatnonzero(same_basis & live)]
            assert same_basis[~live].all() and not r["pivots"][~live].any()
            seen["outside"] = int(live.sum())
    print(f"meaning on {p.n} nodes / {p.m} arcs: {len(probes)} probes, {seen}")
    assert seen["inside"] >= p.m and seen["outside"] >= p.m // 2 and seen["zero"] >= 1, seen


HOST_REDATA = lambda u, a, stype: u.rerun_data_on_host(supply_type=stype, **a)


@pytest.mark.parametrize("which", (0, 1))
def test_a_datum_moved_by_its_range_keeps_the_basis_and_one_past_it_does_not_on_the_host(which):
    check_meaning(HOST_SOLVE, HOST_REDATA, HOST_RANGES, meaning_cases()[which])


# ---- 3: a call changes nothing
def check_solves_do_not_see_it(solve, resolve, resolve_data, ranges, cost_ranges):
    """After a data_ranges, cost_ranges, resolve and resolve_data give what they give without it, and the solve's statistics are as they were."""
    t, a = small_case()
    pairs = D.pairs_of((5,), t.n, t.src, t.tgt)
    other = dict(a, cost=np.ascontiguousarray(a["cost"][::-1]))
    supply = a["supply"].copy()
    supply[:, [0, -1]] = supply[:, [-1, 0]]
    moved_data = dict(other, supply=supply)
    with_it, without = uniform_of(t, O.RULE_BLOCK), uniform_of(t, O.RULE_BLOCK)
    for step, (run, arrays) in enumerate(((solve, a), (resolve, other), (resolve_data, moved_data), (resolve, dict(moved_data, cost=a["cost"])))):
        r1, r2 = run(with_it, arrays), run(without, arrays)
        for name, v in to_numpy(r1).items():
            assert np.array_equal(v, to_numpy(r2)[name]), (step, name)
        stats, redata_stats, range_stats = with_it.stats(), with_it.resolve_data_stats(), with_it.range_stats()
        first = ranges(with_it, pairs)
        assert with_it.stats() == stats and with_it.resolve_data_stats() == redata_stats and with_it.range_stats() == range_stats
        assert_same_data_ranges(ranges(with_it, pairs), first, step)
        c1, c2 = cost_ranges(with_it), cost_ranges(without)
        for name in ("ranged", "arc_state", "cost_down", "cost_up"):
            get = lambda x: x if isinstance(x, np.ndarray) else x.cpu().numpy()
            assert np.array_equal(get(getattr(c1, name)), get(getattr(c2, name))), (step, name)
        for key in ("total_pivots", "launches", "instances"):
            assert stats[key] == without.stats()[key], (step, key)


def test_solve_calls_and_cost_ranges_do_not_see_a_data_ranges_call_on_the_host():
    plain = lambda name: (lambda u, a: getattr(u, name)(**a))
    check_solves_do_not_see_it(plain("run_on_host"), plain("rerun_on_host"), plain("rerun_data_on_host"), HOST_RANGES, lambda u: u.cost_ranges_on_host())


# ---- 4: the contract
def data_range_io(cls, memory=L.MEM_HOST, pair_count=None, **arrays):
    io = cls()
    io.memory = memory
    if pair_count is not None:
        io.pair_count = pair_count
    for name, a in arrays.items():
        setattr(io, name, None if a is None else a.ctypes.data)
    return io


def check_contract(solve, name, host_only):
    """solve(handle, arrays) -> result; name: the C entry point's name behind the handle's prefix."""
    lib = L.lib()
    t, a = small_case()
    flat = Flat(t.variants)
    pairs = D.pairs_of((6,), t.n, t.src, t.tgt)
    k = len(pairs)
    pair_row = np.arange(t.count + 1, dtype=np.int64) * k
    for handle, io_cls, arrays, arcs, tables in ((uniform_of(t, O.RULE_BLOCK), L.UBatchDataRangeIo, a, t.count * t.m, dict(pair_count=k, pairs=pairs)),
                                                 (flat.handle(), L.RBatchDataRangeIo, flat.arrays, int(flat.arc_rows[-1]),
                                                  dict(pairs=np.ascontiguousarray(np.tile(pairs, (t.count, 1))), pair_row=pair_row, ship_row=pair_row))):
        uniform = io_cls is L.UBatchDataRangeIo
        call = getattr(lib, f"{handle._PREFIX}_{name}")
        out = dict(ranged=np.full(t.count, 7, np.int32), arc_state=np.full(arcs, 7, np.int8), flow_down=np.full(arcs, 7, np.int64), flow_up=np.full(arcs, 7, np.int64),
                   ship_forth=np.full(t.count * k, 7, np.int64), ship_back=np.full(t.count * k, 7, np.int64))
        untouched = lambda: all(np.all(v == 7) for v in out.values())
        # before a solve of either kind
        assert call(handle._h, C.byref(data_range_io(io_cls, **tables, **out))) == L.ERR_STATE and untouched()
        solve(handle, arrays)
        assert call(handle._h, None) == L.ERR_INVALID and call(None, C.byref(data_range_io(io_cls, **tables, **out))) == L.ERR_INVALID
        assert call(handle._h, C.byref(data_range_io(io_cls, memory=5, **tables, **out))) == L.ERR_INVALID
        if host_only:
            assert call(handle._h, C.byref(data_range_io(io_cls, memory=L.MEM_DEVICE, **tables, **out))) == L.ERR_INVALID
        # half a pair of outputs
        for alone in ("flow_down", "flow_up", "ship_forth", "ship_back"):
            assert call(handle._h, C.byref(data_range_io(io_cls, **tables, **{n: v for n, v in out.items() if n != alone}))) == L.ERR_INVALID, alone
        # ship rows without pairs, a negative count, tables that do not fit
        assert call(handle._h, C.byref(data_range_io(io_cls, **out))) == L.ERR_INVALID
        if uniform:
            assert call(handle._h, C.byref(data_range_io(io_cls, **dict(tables, pair_count=-1), **out))) == L.ERR_INVALID
            assert call(handle._h, C.byref(data_range_io(io_cls, pair_count=k, **out))) == L.ERR_INVALID                  # a count without a list
        else:
            assert call(handle._h, C.byref(data_range_io(io_cls, **dict(tables, ship_row=None), **out))) == L.ERR_INVALID
            assert call(handle._h, C.byref(data_range_io(io_cls, **dict(tables, pair_row=pair_row[::-1].copy()), **out))) == L.ERR_INVALID
            assert call(handle._h, C.byref(data_range_io(io_cls, **dict(tables, ship_row=pair_row + 1), **out))) == L.ERR_INVALID
            short = pair_row.copy()
            short[-1] -= 1
            assert call(handle._h, C.byref(data_range_io(io_cls, **dict(tables, ship_row=short), **out))) == L.ERR_INVALID
        assert untouched()
        assert call(handle._h, C.byref(data_range_io(io_cls, **tables, **out))) == 0
        full = {n: v.copy() for n, v in out.items()}
        assert 0 < full["ranged"].sum() < t.count and np.any(full["flow_up"] == INF) and np.any(full["ship_forth"] == -1) and np.any(full["ship_forth"] == INF)
        stats = L.UBatchDataRangeStats()
        getter = getattr(lib, f"{handle._PREFIX}_get_data_range_stats")
        assert getter(handle._h, C.byref(stats)) == 0 and stats.ranged == full["ranged"].sum() and stats.hops > 0 and stats.walks > 0
        for present in ((), ("ranged",), ("arc_state",), ("flow_down", "flow_up"), ("ship_forth", "ship_back"), ("ranged", "flow_down", "flow_up", "ship_forth", "ship_back")):
            part = {n: np.full_like(v, 7) for n, v in out.items() if n in present}
            with_pairs = tables if "ship_forth" in present else {}
            assert call(handle._h, C.byref(data_range_io(io_cls, **with_pairs, **part))) == 0, present
            for n, v in part.items():
                assert np.array_equal(v, full[n]), (present, n)
            assert getter(handle._h, C.byref(stats)) == 0 and stats.ranged == full["ranged"].sum()
            assert (stats.walks > 0) == ("flow_down" in present or "ship_forth" in present), present
        assert getter(handle._h, None) == L.ERR_INVALID and getter(None, C.byref(stats)) == L.ERR_INVALID
        ranges = handle.data_ranges_on_host if host_only else handle.data_ranges
        g = ranges(flows=False)
        assert g.flow_down is None and g.ship_forth is None and np.array_equal(data_rows(g)["arc_state"], full["arc_state"])
        with pytest.raises(ValueError):
            g.bounds(None, None)
        with pytest.raises(ValueError):
            ranges(pairs=np.zeros((3, 3), np.int32) if uniform else [pairs])


def test_contract_on_the_host():
    check_contract(lambda h, a: h.run_on_host(**a), "data_ranges_on_host", True)


def test_without_a_device_the_handle_is_unchanged(have_gpu):
    # no GPU: device 0 is missing; with one, device 99 is
    t, a = small_case()
    pairs = D.pairs_of((6,), t.n, t.src, t.tgt)
    u = uniform_of(t, O.RULE_BLOCK, device=99 if have_gpu else 0)
    r = u.run_on_host(**a)
    before, stats, range_stats = u.data_ranges_on_host(pairs=pairs), u.stats(), u.data_range_stats()
    with pytest.raises(M.McfError) as ei:
        u.data_ranges(pairs=pairs, tensors=False)
    assert ei.value.code == L.ERR_NO_DEVICE
    assert u.stats() == stats and u.data_range_stats() == range_stats
    assert_same_data_ranges(u.data_ranges_on_host(pairs=pairs), before)
    again = u.rerun_data_on_host(**a)
    assert np.array_equal(again.flows, r.flows) and before.ranged.any() and not again.pivots[before.ranged == 1].any()       # the warm starts


def test_data_range_structs_have_the_layout_of_the_header(tmp_path):
    src = tmp_path / "sz.c"
    u_fields = ("pair_count", "pairs", "ranged", "arc_state", "flow_down", "flow_up", "ship_forth", "ship_back")
    r_fields = ("pairs", "pair_row", "ship_row", "ranged", "arc_state", "flow_down", "flow_up", "ship_forth", "ship_back")
    s_fields = ("instances", "ranged", "lds_instances", "global_instances", "walks", "hops", "kernel_ns", "bytes_up", "bytes_down")
    line = lambda struct, fields: 'printf("%zu' + " %zu" * len(fields) + '\\n", sizeof(%s)' % struct + "".join(", offsetof(%s, %s)" % (struct, f) for f in fields) + ");"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void){' % os.path.join(ROOT, "include", "mcf_hip.h")
                   + line("mcf_ubatch_data_range_io", u_fields) + line("mcf_rbatch_data_range_io", r_fields) + line("mcf_ubatch_data_range_stats", s_fields)
                   + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", str(src), "-o", str(exe)])
    got = [[int(x) for x in row.split()] for row in subprocess.check_output([str(exe)]).decode().splitlines()]
    for cls, fields, row in zip((L.UBatchDataRangeIo, L.RBatchDataRangeIo, L.UBatchDataRangeStats), (u_fields, r_fields, s_fields), got):
        assert row == [C.sizeof(cls)] + [getattr(cls, f).offset for f in fields], cls
        assert cls.memory.offset == 0 if hasattr(cls, "memory") else True


# ---- 5: instances that are not ranged
def check_not_ranged(solve, ranges, limited):
    """Zero rows after a pivot limit, for an Infeasible instance and for one that ends Optimal with a surplus."""
    t, stype = redata_family()[0]
    pairs = D.pairs_of((7,), t.n, t.src, t.tgt)
    refs = [cold_reference(p, stype, O.RULE_BLOCK) for p in t.variants]
    surplus = [k for k, ref in enumerate(refs) if ref[0] == O.OPTIMAL and ref[2] is not None]
    infeasible = [k for k, ref in enumerate(refs) if ref[0] == O.INFEASIBLE]
    ranged = [k for k, ref in enumerate(refs) if ref[0] == O.OPTIMAL and ref[2] is None]
    assert surplus and infeasible and ranged
    u = uniform_of(t, O.RULE_BLOCK)
    solve(u, t.arrays(), stype)
    rows = data_rows(ranges(u, pairs))
    assert np.array_equal(np.flatnonzero(rows["ranged"]), ranged)
    for k in surplus + infeasible:
        assert not any(rows[name].reshape(t.count, -1)[k].any() for name in FIELDS[1:]), k
    for k in ranged:
        assert rows["flow_up"].reshape(t.count, -1)[k].any() and rows["ship_forth"].reshape(t.count, -1)[k].any(), k
    u = uniform_of(t, O.RULE_BLOCK, pivot_limit=1)
    r = to_numpy(limited(u, t.arrays(), stype))
    stopped = np.flatnonzero(r["status"] == M.SolverStatus.NotSolved)
    assert len(stopped) >= 3
    rows = data_rows(ranges(u, pairs))
    assert not rows["ranged"][stopped].any() and not any(rows[name].reshape(t.count, -1)[stopped].any() for name in FIELDS[1:])
    st = u.data_range_stats()
    assert st["ranged"] == int(rows["ranged"].sum())


def test_instances_that_are_not_ranged_give_zero_rows_on_the_host():
    check_not_ranged(HOST_SOLVE, HOST_RANGES, HOST_SOLVE)
