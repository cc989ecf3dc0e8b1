"""Cost ranges of the kept basis (mcf_ubatch_cost_ranges_on_host / mcf_rbatch_cost_ranges_on_host, DESIGN.md 3.14 "Cost ranges of the kept
basis") without a GPU: the hooks run the device's own step (csrc/ranges_step.hip.h) with one lane on the CPU.

Every comparison is exact.  The reference is the brute force of ranges_oracle.py on the oracle's own basis (its floors are asserted
there); what the numbers MEAN is checked through the existing re-solve: a cost inside its range makes no pivot and keeps the flows, a
cost one past it makes at least one.  test_ranges_gpu.py imports the batches and the checkers from here."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import mincostflow_amd as M
from mincostflow_amd import _lib as L
from oracle import ns_oracle as O

import ranges_oracle as R
from adversarial import random_problem
from test_batch_host import ROOT, RULES, fuzz_cases, oracle_of, padded_fuzz
from test_uniform_host import ALL_RULES, family, to_numpy, uniform_of

INF = M.RANGE_INF
FIELDS = ("ranged", "arc_state", "cost_down", "cost_up")
PROBLEM_FIELDS = ("cost", "supply", "lower", "upper")


def range_rows(g):
    get = lambda a: a if a is None or isinstance(a, np.ndarray) else a.cpu().numpy()
    return {name: get(getattr(g, name)) for name in FIELDS}


def assert_same_ranges(a, b, what=""):
    a, b = range_rows(a), range_rows(b)
    for name in FIELDS:
        assert a[name].dtype == b[name].dtype and np.array_equal(a[name], b[name]), (what, name)


class Flat:
    """Problems of any graphs in one RaggedBatch, instance i = problem i."""

    def __init__(self, problems):
        self.problems = tuple(problems)
        self.count = len(self.problems)
        self.arc_rows = np.concatenate([[0], np.cumsum([p.m for p in self.problems])]).astype(np.int64)
        self.arrays = {f: np.ascontiguousarray(np.concatenate([getattr(p, f) for p in self.problems])) for f in PROBLEM_FIELDS}

    def handle(self, rule=O.RULE_BLOCK, **kw):
        return M.RaggedBatch([(p.n, p.src, p.tgt) for p in self.problems], rule=RULES[rule], **kw)


@functools.lru_cache(maxsize=None)
def fuzz_flat():
    return Flat([p for p, _ in fuzz_cases()])


@functools.lru_cache(maxsize=None)
def padded_flat(rule):
    return Flat([q for q, _, _ in padded_fuzz(rule)])


def assert_zero_where_not_ranged(rows, arc_rows):
    for i in np.flatnonzero(rows["ranged"] == 0):
        lo, hi = arc_rows[i], arc_rows[i + 1]
        assert not rows["arc_state"][lo:hi].any() and not rows["cost_down"][lo:hi].any() and not rows["cost_up"][lo:hi].any(), i
    assert set(np.unique(rows["ranged"])) <= {0, 1}


def check_against_brute_force(solve, ranges, flat, stypes, want, rule):
    """One handle holds every instance; a call has one supply type, so the handle is solved under each, and every instance is compared
    under its own.  want: ranges_oracle.reference_rows.  Yields (supply type, handle, the call's rows) for what the caller adds."""
    ranged, state, down, up, _ = want
    h = flat.handle(rule)
    compared = 0
    for stype in (O.GEQ, O.LEQ):
        solve(h, flat.arrays, stype)
        g = ranges(h)
        rows = range_rows(g)
        assert rows["ranged"].shape == (flat.count,) and rows["arc_state"].shape == rows["cost_down"].shape == rows["cost_up"].shape == (flat.arc_rows[-1],)
        assert rows["ranged"].dtype == np.int32 and rows["arc_state"].dtype == np.int8 and rows["cost_down"].dtype == rows["cost_up"].dtype == np.int64
        assert_zero_where_not_ranged(rows, flat.arc_rows)
        for i in (k for k, s in enumerate(stypes) if s == stype):
            lo, hi = flat.arc_rows[i], flat.arc_rows[i + 1]
            assert rows["ranged"][i] == ranged[i], (i, stype)
            for name, ref in (("arc_state", state), ("cost_down", down), ("cost_up", up)):
                assert np.array_equal(rows[name][lo:hi], ref[lo:hi]), (i, stype, name)
            a, d, u = g.arcs(i)
            assert len(a) == len(d) == len(u) == hi - lo
            compared += 1
        st = h.range_stats()
        assert st["instances"] == flat.count and st["ranged"] == int(rows["ranged"].sum()), st
        assert st["tree_arcs"] == sum(int(np.sum(rows["arc_state"][flat.arc_rows[i]:flat.arc_rows[i + 1]] == 0)) for i in np.flatnonzero(rows["ranged"])), st
        assert st["cycle_hops"] > 0
        yield stype, h, g
    assert compared == flat.count


HOST_SOLVE = lambda h, a, stype: h.run_on_host(supply_type=stype, **a)
HOST_RANGES = lambda h: h.cost_ranges_on_host()


# ---- 1: the adversarial batch against the brute force
@pytest.mark.parametrize("rule", ALL_RULES)
def test_adversarial_batch_equals_the_brute_force_on_the_host(rule):
    for stype, h, g in check_against_brute_force(HOST_SOLVE, HOST_RANGES, fuzz_flat(), [s for _, s in fuzz_cases()], R.fuzz_ranges(rule), rule):
        st = h.range_stats()
        assert st["lds_instances"] == st["global_instances"] == st["bytes_up"] == st["bytes_down"] == 0, st


def test_padded_instances_equal_the_brute_force_on_the_host():
    rule = O.RULE_BLOCK
    for _ in check_against_brute_force(HOST_SOLVE, HOST_RANGES, padded_flat(rule), [s for _, s, _ in padded_fuzz(rule)], R.padded_ranges(rule), rule):
        pass


# ---- 2: a handle of one graph
def check_one_graph(solve_ragged, solve_uniform, ranges):
    t = family("A")[4]
    a = t.arrays()
    flat = Flat(t.variants)
    for stype in (O.GEQ, O.LEQ):
        h, u = flat.handle(), uniform_of(t, O.RULE_BLOCK)
        solve_ragged(h, flat.arrays, stype)
        solve_uniform(u, a, stype)
        gh, gu = range_rows(ranges(h)), range_rows(ranges(u))
        assert gu["arc_state"].shape == gu["cost_down"].shape == gu["cost_up"].shape == (t.count, t.m)
        assert 0 < gu["ranged"].sum() < t.count
        for name in FIELDS:
            assert gh[name].dtype == gu[name].dtype and np.array_equal(gh[name].reshape(-1), gu[name].reshape(-1)), (stype, name)
        sh, su = h.range_stats(), u.range_stats()
        for field in ("instances", "ranged", "lds_instances", "global_instances", "tree_arcs", "cycle_hops"):
            assert sh[field] == su[field], (field, sh, su)


def test_one_graph_equals_the_uniform_batch_on_the_host():
    check_one_graph(HOST_SOLVE, HOST_SOLVE, HOST_RANGES)


# ---- 3: what the numbers mean
@functools.lru_cache(maxsize=None)
def meaning_problem():
    """A ranged instance of 20 nodes and 60 arcs drawn as the families' negative-cost variants are, every capacity finite, made a
    circulation (supplies and lower bounds 0): the first seed the oracle solves to Optimal after at least 10 pivots.
    A circulation because "every other cost fixed" must hold in the re-solve that checks a range.  A re-solve derives the artificial arcs'
    cost anew from the largest |cost| (art_cost = (max |cost| + 1) n), and of 3 000 balanced instances drawn with supplies every ranged
    one kept an artificial arc in its tree at flow 0 -- the root hangs by it -- so the slack of every root link, and with it every range
    a root link limits, is about art_cost: moving a cost that far moves art_cost along, a second cost.  Without supplies no node needs
    an artificial arc, the root hangs by root links of cost 0, and nothing but the one arc's cost changes."""
    zeros = np.zeros(60, np.int64)
    for seed in range(64):
        q = random_problem(np.random.default_rng([20261120, seed]), 20, 60, "negative", zero_capacity=False, inf_fraction=0.0)
        p = O.Problem(q.n, q.m, q.src, q.tgt, zeros, q.upper - q.lower, q.cost, np.zeros(q.n, np.int64))
        o, st, _ = oracle_of(p, O.RULE_BLOCK)
        if R.is_ranged(o, st, p) and o.n_pivots >= 10:
            assert np.all(p.upper < O.INF_CAP) and o.all_arc_num == p.m + p.n
            return p, o
    raise AssertionError("no ranged instance among 64 seeds")


def recosted(u, base, r0, resolve):
    """the state a resolve() with other costs leaves"""
    base = dict(base, cost=base["cost"] + np.arange(len(base["cost"])) % 5)
    return base, resolve(u, base)


def redata(resolve_data):
    def between(u, base, r0, resolve):
        """the state a warm resolve_data() leaves: the arc that carries the most flow loses one unit of capacity, so a tree arc or an
        arc at its upper bound has to give way"""
        flows = to_numpy(r0)["flows"][0]
        e = int(np.argmax(flows))
        assert flows[e] >= 2
        upper = base["upper"].copy()
        upper[e] = flows[e] - 1
        base = dict(base, upper=upper)
        r = resolve_data(u, base)
        st = u.resolve_data_stats()
        assert st["warm_instances"] == len(u) and st["fallback_instances"] == st["cold_instances"] == 0, st
        assert np.all(to_numpy(r)["flows"][:, e] == flows[e] - 1)
        return base, r
    return between


def check_meaning(solve, resolve, ranges, between=None, reference=None, problem=None):
    """solve / resolve(handle, arrays) -> result with one shared row per array but the costs.  problem: (a ranged circulation, its
    oracle), by default meaning_problem()."""
    p, o = problem or meaning_problem()
    m, count = p.m, 4 * p.m
    u = M.UniformBatch(p.n, p.src, p.tgt, count)
    base = {f: getattr(p, f) for f in PROBLEM_FIELDS}
    r0 = solve(u, base)
    if between:
        base, r0 = between(u, base, r0, resolve)
    r0 = to_numpy(r0)
    assert np.all(r0["status"] == O.OPTIMAL)
    g = range_rows(ranges(u))
    assert g["ranged"].all()
    for name in FIELDS[1:]:
        assert np.all(g[name] == g[name][0]), name
    state, down, up = g["arc_state"][0], g["cost_down"][0], g["cost_up"][0]
    if not between:
        ref_state, ref_down, ref_up, _ = R.brute_force(o, p)
        assert np.array_equal(state, ref_state) and np.array_equal(down, ref_down) and np.array_equal(up, ref_up)
    if reference is not None:
        assert_same_ranges(Rows(g), reference(u), "against the hook")
    assert np.all(down >= 0) and np.all(up >= 0) and np.all((state != 1) | (up == INF)) and np.all((state != -1) | (down == INF))
    cost = np.ascontiguousarray(np.tile(base["cost"], (count, 1)))
    kind = np.zeros(count, np.int8)          # 1 = inside its range, 2 = one past it, 0 = the skipped outside of an infinite side: costs unchanged
    for e in range(m):
        for k, (side, sign, past) in enumerate(((down, -1, 0), (down, -1, 1), (up, 1, 0), (up, 1, 1))):
            i = 4 * e + k
            if side[e] == INF:
                if not past:
                    cost[i, e] += sign * (1 << 20)
                    kind[i] = 1
            else:
                cost[i, e] += sign * (int(side[e]) + past)
                kind[i] = 1 + past
    r1 = to_numpy(resolve(u, dict(base, cost=cost)))
    outside = kind == 2
    assert outside.sum() >= m, outside.sum()
    assert np.all(r1["status"][~outside] == O.OPTIMAL)
    assert np.all(r1["pivots"][~outside] == 0), np.flatnonzero((r1["pivots"] != 0) & ~outside)
    assert np.all(r1["flows"][~outside] == r0["flows"][0])
    assert np.all(r1["pivots"][outside] >= 1), np.flatnonzero((r1["pivots"] == 0) & outside)
    return u


class Rows:
    def __init__(self, rows):
        self.__dict__.update(rows)


HOST_UNIFORM = (lambda u, a: u.run_on_host(**a), lambda u, a: u.rerun_on_host(**a), lambda u, a: u.rerun_data_on_host(**a))


def test_a_cost_inside_its_range_makes_no_pivot_and_one_past_it_does_on_the_host():
    check_meaning(HOST_UNIFORM[0], HOST_UNIFORM[1], HOST_RANGES)


def test_ranges_after_a_resolve_and_after_a_warm_resolve_data_on_the_host():
    check_meaning(HOST_UNIFORM[0], HOST_UNIFORM[1], HOST_RANGES, between=recosted)
    check_meaning(HOST_UNIFORM[0], HOST_UNIFORM[1], HOST_RANGES, between=redata(HOST_UNIFORM[2]))


# ---- 4: the contract
def range_io(cls, memory=L.MEM_HOST, **arrays):
    io = cls()
    io.memory = memory
    for name, a in arrays.items():
        setattr(io, name, a.ctypes.data)
    return io


def small_case():
    t = family("A")[3]
    return t, t.arrays()


def check_contract(solve, ranges_name, host_only, have_gpu):
    """solve(handle, arrays) -> result; ranges_name: the C entry point's name behind the handle's prefix."""
    lib = L.lib()
    t, a = small_case()
    flat = Flat(t.variants)
    for handle, io_cls, arrays, arcs in ((uniform_of(t, O.RULE_BLOCK), L.UBatchRangeIo, a, t.count * t.m), (flat.handle(), L.RBatchRangeIo, flat.arrays, int(flat.arc_rows[-1]))):
        call = getattr(lib, f"{handle._PREFIX}_{ranges_name}")
        out = dict(ranged=np.full(t.count, 7, np.int32), arc_state=np.full(arcs, 7, np.int8), cost_down=np.full(arcs, 7, np.int64), cost_up=np.full(arcs, 7, np.int64))
        # before a solve of either kind
        assert call(handle._h, C.byref(range_io(io_cls, **out))) == L.ERR_STATE
        assert all(np.all(v == 7) for v in out.values())
        solve(handle, arrays)
        assert call(handle._h, None) == L.ERR_INVALID and call(None, C.byref(range_io(io_cls, **out))) == L.ERR_INVALID
        assert call(handle._h, C.byref(range_io(io_cls, memory=5, **out))) == L.ERR_INVALID
        if host_only:
            assert call(handle._h, C.byref(range_io(io_cls, memory=L.MEM_DEVICE, **out))) == L.ERR_INVALID
        # one of the two cost rows alone is refused; everything else may be absent
        for alone in ("cost_down", "cost_up"):
            assert call(handle._h, C.byref(range_io(io_cls, **{k: v for k, v in out.items() if k != alone}))) == L.ERR_INVALID
        assert all(np.all(v == 7) for v in out.values())
        assert call(handle._h, C.byref(range_io(io_cls, **out))) == 0
        full = {k: v.copy() for k, v in out.items()}
        assert 0 < full["ranged"].sum() < t.count and np.any(full["cost_down"] == INF) and np.any(full["cost_up"] == INF)
        stats = L.UBatchRangeStats()
        getter = getattr(lib, f"{handle._PREFIX}_get_range_stats")
        assert getter(handle._h, C.byref(stats)) == 0 and stats.ranged == full["ranged"].sum() and stats.cycle_hops > 0
        for present in ((), ("ranged",), ("arc_state",), ("cost_down", "cost_up"), ("ranged", "cost_down", "cost_up")):
            part = {k: np.full_like(v, 7) for k, v in out.items() if k in present}
            assert call(handle._h, C.byref(range_io(io_cls, **part))) == 0, present
            for k, v in part.items():
                assert np.array_equal(v, full[k]), (present, k)
            assert getter(handle._h, C.byref(stats)) == 0 and stats.ranged == full["ranged"].sum()
            assert (stats.cycle_hops > 0) == ("cost_down" in present) and (stats.tree_arcs > 0) == ("cost_down" in present)
        assert getter(handle._h, None) == L.ERR_INVALID and getter(None, C.byref(stats)) == L.ERR_INVALID
        g = handle.cost_ranges_on_host(costs=False) if host_only else handle.cost_ranges(costs=False)
        assert g.cost_down is None and g.cost_up is None and np.array_equal(range_rows(g)["arc_state"].reshape(-1), full["arc_state"])


def test_contract_on_the_host(have_gpu):
    check_contract(lambda h, a: h.run_on_host(**a), "cost_ranges_on_host", True, have_gpu)


def test_without_a_device_the_handle_is_unchanged(have_gpu):
    # no GPU: device 0 is missing; with one, device 99 is
    t, a = small_case()
    u = uniform_of(t, O.RULE_BLOCK, device=99 if have_gpu else 0)
    r = u.run_on_host(**a)
    before, stats, range_stats = u.cost_ranges_on_host(), u.stats(), u.range_stats()
    with pytest.raises(M.McfError) as ei:
        u.cost_ranges()
    assert ei.value.code == L.ERR_NO_DEVICE
    assert u.stats() == stats and u.range_stats() == range_stats
    assert_same_ranges(u.cost_ranges_on_host(), before)
    again = u.rerun_on_host(**a)
    assert np.array_equal(again.flows, r.flows) and before.ranged.any() and not again.pivots[before.ranged == 1].any()     # the warm starts


def check_empty_and_infeasible(solve_uniform, solve_ragged, ranges):
    t, a = small_case()
    # no instance at all
    u = M.UniformBatch(t.n, t.src, t.tgt, 0)
    solve_uniform(u, {k: v[:0] for k, v in a.items()})
    g = range_rows(ranges(u))
    assert g["ranged"].shape == (0,) and g["cost_down"].shape == (0, t.m)
    assert u.range_stats()["instances"] == u.range_stats()["ranged"] == 0
    h = M.RaggedBatch([])
    solve_ragged(h, {k: np.zeros(0, np.int64) for k in PROBLEM_FIELDS})
    g = range_rows(ranges(h))
    assert g["ranged"].shape == g["arc_state"].shape == g["cost_up"].shape == (0,)
    # every instance infeasible by its bounds: nothing was ever set up
    bad = dict(a, upper=np.ascontiguousarray(a["lower"] - 1))
    u = uniform_of(t, O.RULE_BLOCK)
    r = solve_uniform(u, bad)
    assert np.all(to_numpy(r)["status"] == O.INFEASIBLE) and not to_numpy(r)["pivots"].any()
    g = range_rows(ranges(u))
    assert not any(g[name].any() for name in FIELDS)
    st = u.range_stats()
    assert st["instances"] == t.count and st["ranged"] == st["tree_arcs"] == st["cycle_hops"] == 0, st


def test_empty_and_infeasible_batches_on_the_host():
    check_empty_and_infeasible(lambda u, a: u.run_on_host(**a), lambda h, a: h.run_on_host(**a), HOST_RANGES)


def check_solves_do_not_see_it(solve, resolve, resolve_data, ranges):
    """After a cost_ranges, resolve and resolve_data give the rows they give without it, and the solve's statistics are as they were."""
    t, a = small_case()
    other = dict(a, cost=np.ascontiguousarray(a["cost"][::-1]))
    supply = a["supply"].copy()
    supply[:, [0, -1]] = supply[:, [-1, 0]]
    moved = dict(other, supply=supply)
    with_it, without = uniform_of(t, O.RULE_BLOCK), uniform_of(t, O.RULE_BLOCK)
    for step, (run, arrays) in enumerate(((solve, a), (resolve, other), (resolve_data, moved), (resolve, dict(moved, cost=a["cost"])))):
        r1, r2 = run(with_it, arrays), run(without, arrays)
        for name, v in to_numpy(r1).items():
            assert np.array_equal(v, to_numpy(r2)[name]), (step, name)
        stats, redata_stats = with_it.stats(), with_it.resolve_data_stats()
        first = ranges(with_it)
        assert with_it.stats() == stats and with_it.resolve_data_stats() == redata_stats
        assert_same_ranges(ranges(with_it), first, step)
        for key in ("total_pivots", "launches", "instances"):
            assert stats[key] == without.stats()[key], (step, key)


def test_solve_calls_do_not_see_a_ranges_call_on_the_host():
    check_solves_do_not_see_it(HOST_UNIFORM[0], HOST_UNIFORM[1], HOST_UNIFORM[2], HOST_RANGES)


def test_range_structs_have_the_layout_of_the_header(tmp_path):
    src = tmp_path / "sz.c"
    names = ("ubatch_range_io", "rbatch_range_io")
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void){' % os.path.join(ROOT, "include", "mcf_hip.h")
                   + "".join('printf("%%zu %%zu %%zu %%zu %%zu\\n", sizeof(mcf_%s), offsetof(mcf_%s, ranged), offsetof(mcf_%s, arc_state), offsetof(mcf_%s, cost_down), '
                             'offsetof(mcf_%s, cost_up));' % ((n,) * 5) for n in names)
                   + 'printf("%zu %zu %zu %zu %zu\\n", sizeof(mcf_ubatch_range_stats), offsetof(mcf_ubatch_range_stats, global_instances), offsetof(mcf_ubatch_range_stats, cycle_hops), '
                     'offsetof(mcf_ubatch_range_stats, kernel_ns), offsetof(mcf_ubatch_range_stats, bytes_down));'
                   + 'printf("%lld\\n", (long long)MCF_RANGE_INF);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", str(src), "-o", str(exe)])
    got = [[int(x) for x in line.split()] for line in subprocess.check_output([str(exe)]).decode().splitlines()]
    for cls, row in zip((L.UBatchRangeIo, L.RBatchRangeIo), got):
        assert row == [C.sizeof(cls), cls.ranged.offset, cls.arc_state.offset, cls.cost_down.offset, cls.cost_up.offset]
    S = L.UBatchRangeStats
    assert got[2] == [C.sizeof(S), S.global_instances.offset, S.cycle_hops.offset, S.kernel_ns.offset, S.bytes_down.offset]
    assert got[3] == [L.RANGE_INF] and M.RANGE_INF == np.iinfo(np.int64).max == R.INF
