"""The ragged batch (mcf_rbatch_*, RaggedBatch, DESIGN.md 3.14 "Ragged batch") without a GPU: mcf_rbatch_run_on_host / _rerun_on_host /
_validate_on_host run the device's own steps (csrc/uniform_step.hip.h) on views formed from the handle's tables (ragged_view), and its pivot
code, with one lane on the CPU.

One handle holds a whole family of test_uniform_host.py, INTERLEAVED: instance k is variant k // G of graph k % G, so consecutive rows have
different lengths and no row offset is a multiple of 64 by accident.  Every comparison is exact.  The references are the oracle
(reference() of test_uniform_host.py, whose floors are asserted there), BatchSolver.add + run_on_host for the same instances in the same
order, UniformBatch for a handle of one graph, and oracle/validator.validate for the validation.  test_ragged_gpu.py imports the mixes and
the checkers from here."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import mincostflow_amd as M
from mincostflow_amd import _lib as L
from oracle import ns_oracle as O
from oracle import validator as V

from test_batch_host import ROOT, RULES, bound_infeasible
from test_batch_resolve_host import cold_reference, with_cost
from test_uniform_host import (ALL_RULES, CLASSES, KINDS, LIMIT_RUNS, NOT_SOLVED, STEPS, SUPPLY_TYPES, TRACE, answer_of, assert_equals_answers, assert_limit_floors,
                               assert_matches_cold, assert_rows_equal, batch_answers, check_chain_under_a_limit, check_unchanged_costs_and_mask_under_a_limit, draw_topology,
                               family, limited_chain, limited_reference, limited_validation_cases, reference, resolve_family, step_costs, stride_of, to_numpy, uniform_of)
from test_uniform_validate_host import EQ, OUT_NAMES, PROBLEM_NAMES, ROW_NAMES, corrupted_cases, rows_of, solved_cases


class Rows:
    """A dict of rows with the attributes of a result, so that the checkers of test_uniform_host.py take it."""

    def __init__(self, rows):
        self.__dict__.update(rows)


class Mix:
    """Instances of several graphs in one handle.  tops: the Topology of every graph; order: per instance (graph, variant), by default
    interleaved -- instance k is variant k // G of graph k % G."""

    def __init__(self, tops, order=None):
        self.tops = tuple(tops)
        G = len(self.tops)
        self.order = tuple(order) if order is not None else tuple((k % G, k // G) for k in range(G * self.tops[0].count))
        self.count = len(self.order)
        self.graph_of = np.array([g for g, _ in self.order], np.int32)
        self.graphs = [(t.n, t.src, t.tgt) for t in self.tops]
        self.m = np.array([self.tops[g].m for g, _ in self.order], np.int64)
        self.n = np.array([self.tops[g].n for g, _ in self.order], np.int64)
        self.arc_rows = np.concatenate([[0], np.cumsum(self.m)]).astype(np.int64)
        self.node_rows = np.concatenate([[0], np.cumsum(self.n)]).astype(np.int64)

    def problems(self):
        return [self.tops[g].variants[v] for g, v in self.order]

    def handle(self, rule=O.RULE_BLOCK, **kw):
        h = M.RaggedBatch(self.graphs, self.graph_of, rule=RULES[rule], record_trace=kw.pop("record_trace", TRACE), **kw)
        assert np.array_equal(h.arc_rows, self.arc_rows) and np.array_equal(h.node_rows, self.node_rows) and len(h) == self.count
        assert h.arc_rows.dtype == h.node_rows.dtype == np.int64
        return h

    def flat(self, per_graph):
        """per_graph[g][name] = [variants, m or n] (or None) -> name: the instances' rows one after the other"""
        out = {}
        for name in per_graph[0]:
            if per_graph[0][name] is None:
                out[name] = None
                continue
            parts = [np.asarray(per_graph[g][name][v]).reshape(-1) for g, v in self.order]
            out[name] = np.ascontiguousarray(np.concatenate(parts)) if parts else np.zeros(0, np.int64)
        return out

    def arrays(self):
        return self.flat([t.arrays() for t in self.tops])

    def pick(self, per_graph):
        """per_graph[g][v] -> per instance"""
        return [per_graph[g][v] for g, v in self.order]

    def batch_solver(self, rule, stype, **kw):
        b = M.BatchSolver(rule=RULES[rule], record_trace=kw.pop("record_trace", TRACE), **kw)
        for p in self.problems():
            b.add(p, supply_type=stype)
        return b

    def split(self, r):
        """A ragged result as the checkers read it: flows[i] and potentials[i] are instance i's slices"""
        rows = to_numpy(r)
        for name, rows_of_name in (("flows", self.arc_rows), ("potentials", self.node_rows)):
            cut = np.empty(self.count, object)
            for i in range(self.count):
                cut[i] = rows[name][rows_of_name[i]:rows_of_name[i + 1]]
            rows[name] = cut
        return Rows(rows)

    def of_graph(self, r, g):
        """The instances of graph g, in the order of their variants, as a uniform result's 2-D rows"""
        s = to_numpy(self.split(r))
        at = sorted((v, i) for i, (gg, v) in enumerate(self.order) if gg == g)
        idx = [i for _, i in at]
        return Rows({name: (np.stack([s[name][i] for i in idx]) if name in ("flows", "potentials") else s[name][idx]) for name in s})


def footprints(mix):
    return sum(stride_of(mix.tops[g]) for g, _ in mix.order)


@functools.lru_cache(maxsize=None)
def family_mix(name):
    return Mix(family(name))


# ---- 1
def check_families(run, name, rule, **kw):
    """run(handle, arrays, stype) -> result"""
    mix = family_mix(name)
    a = mix.arrays()
    for stype in SUPPLY_TYPES:
        answers = mix.pick(reference(name, rule, stype))
        h = mix.handle(rule, **kw)
        r = run(h, a, stype)
        what = f"family {name}, supply type {stype}"
        assert to_numpy(r)["flows"].shape == (mix.arc_rows[-1],) and to_numpy(r)["potentials"].shape == (mix.node_rows[-1],)
        assert to_numpy(r)["trace"].shape == (mix.count, TRACE)
        assert_equals_answers(mix.split(r), answers, what)
        for i in (0, 1, mix.count - 1):
            assert np.array_equal(_cpu(r.arcs(i)), to_numpy(r)["flows"][mix.arc_rows[i]:mix.arc_rows[i + 1]]) and len(r.arcs(i)) == mix.m[i]
            assert np.array_equal(_cpu(r.nodes(i)), to_numpy(r)["potentials"][mix.node_rows[i]:mix.node_rows[i + 1]]) and len(r.nodes(i)) == mix.n[i]
        b = mix.batch_solver(rule, stype).run_on_host()
        assert_equals_answers(mix.split(r), batch_answers(b, mix.count), what + ", BatchSolver")
        st = h.stats()
        assert st["instances"] == mix.count and st["total_pivots"] == sum(x[1] for x in answers) and st["workspace_bytes"] == footprints(mix), st
        yield stype, h, r, st


def _cpu(a):
    return a if isinstance(a, np.ndarray) else a.cpu().numpy()


HOST = (lambda h, a, stype: h.run_on_host(supply_type=stype, **a), lambda h, a, stype, **kw: h.rerun_on_host(supply_type=stype, **a, **kw))


@pytest.mark.parametrize("rule", ALL_RULES)
@pytest.mark.parametrize("name", ["A", "B"])
def test_families_in_one_handle_on_the_host(name, rule):
    for stype, h, r, st in check_families(HOST[0], name, rule):
        assert st["launches"] == st["bytes_up"] == st["bytes_down"] == st["lds_instances"] == st["global_instances"] == 0


# ---- 2
ONE_GRAPH = (("A", 4), ("B", 4))        # 129 search arcs; 65 nodes


def check_one_graph(run_ragged, run_uniform):
    for name, index in ONE_GRAPH:
        t = family(name)[index]
        assert (t.m + t.n == 129) if name == "A" else (t.n == 65)
        for stype in SUPPLY_TYPES:
            mix = Mix([t], [(0, v) for v in range(t.count)])
            h, u = mix.handle(), uniform_of(t, O.RULE_BLOCK)
            r, ru = to_numpy(run_ragged(h, mix.arrays(), stype)), to_numpy(run_uniform(u, t.arrays(), stype))
            for field in r:
                assert r[field].dtype == ru[field].dtype and np.array_equal(r[field].reshape(-1), ru[field].reshape(-1)), (name, stype, field)
            sh, su = h.stats(), u.stats()
            for field in ("instances", "lds_instances", "global_instances", "launches", "total_pivots", "workspace_bytes", "lds_bytes_max", "bytes_up", "bytes_down"):
                assert sh[field] == su[field], (field, sh, su)


def test_one_graph_equals_the_uniform_batch_on_the_host():
    check_one_graph(HOST[0], lambda u, a, stype: u.run_on_host(supply_type=stype, **a))


# ---- 3
def check_graph_of(run):
    tops = family("A")
    G = len(tops)
    # None with count == graph_count is the identity
    one_each = Mix(tops, [(g, 2) for g in range(G)])
    a = one_each.arrays()
    implicit = M.RaggedBatch(one_each.graphs, None, record_trace=TRACE)
    assert len(implicit) == G and np.array_equal(implicit.arc_rows, one_each.arc_rows)
    first = run(implicit, a, O.GEQ)
    assert_rows_equal(first, run(one_each.handle(), a, O.GEQ), "identity")
    assert_equals_answers(one_each.split(first), one_each.pick(reference("A", O.RULE_BLOCK, O.GEQ)), "identity")
    # a permutation of the instances permutes the rows and nothing else
    straight = family_mix("A")
    rows = straight.split(run(straight.handle(), straight.arrays(), O.GEQ))
    perm = np.random.default_rng(20261103).permutation(straight.count)
    assert not np.array_equal(perm, np.arange(straight.count))
    shuffled = Mix(tops, [straight.order[k] for k in perm])
    got = to_numpy(shuffled.split(run(shuffled.handle(), shuffled.arrays(), O.GEQ)))
    want = to_numpy(rows)
    for field in got:
        for i, k in enumerate(perm):
            assert np.array_equal(got[field][i], want[field][k]), (field, i, k)
    # two instances of one graph with equal data get equal rows, whatever lies between them
    twice = Mix(tops, [(5, 3), (0, 1), (5, 3), (7, 0), (5, 3)])
    s = to_numpy(twice.split(run(twice.handle(), twice.arrays(), O.GEQ)))
    assert s["pivots"][0] > 0
    for field in s:
        assert np.array_equal(s[field][0], s[field][2]) and np.array_equal(s[field][0], s[field][4]), field


def test_graph_of_on_the_host():
    check_graph_of(HOST[0])


# ---- 3b: graphs that the sizes alone do not tell apart
@functools.lru_cache(maxsize=None)
def sibling_mixes():
    """Four graphs of 40 nodes drawn as the families' are: one of 60 arcs and three of 89.  (mix of the three equal ones, mix of the small one
    in front of two of them.)  Equal sizes mean equal rows, workspaces and layouts: only the end points, the incidence lists and -- where
    the arc counts differ -- the slot templates (search range, block size, default pivot limit) tell the instances' graphs apart."""
    tops = [draw_topology(5, index, 40, m).subset(range(8)) for index, m in enumerate((60, 89, 89, 89))]
    assert len({(t.n, t.m) for t in tops[1:]}) == 1 and not np.array_equal(tops[1].src, tops[2].src)
    return Mix(tops[1:]), Mix(tops[:3])


def check_siblings(run, validate, which):
    for mix in (sibling_mixes()[which],):
        a = mix.arrays()
        for rule in ALL_RULES:
            for stype in SUPPLY_TYPES:
                answers = [answer_of(p, rule, stype) for p in mix.problems()]
                assert sum(x[1] > 0 for x in answers) >= mix.count // 2
                r = run(mix.handle(rule), a, stype)
                assert_equals_answers(mix.split(r), answers, (rule, stype))
        # and the validation, which is the only reader of the incidence lists: arbitrary flows and potentials on feasible-looking rows
        rng = np.random.default_rng(20261105)
        rows = dict(status=np.full(mix.count, O.OPTIMAL, np.int32), total_cost=rng.integers(-9, 9, mix.count), flows=rng.integers(0, 9, mix.arc_rows[-1]),
                    potentials=rng.integers(-9, 1, mix.node_rows[-1]))
        want = [V.validate(p.n, p.src, p.tgt, p.lower, np.where(p.upper == O.INF_CAP, np.iinfo(np.int64).max // 2, p.upper), p.cost, p.supply, O.GEQ,
                           rows["flows"][lo:hi], rows["potentials"][nlo:nhi], rows["total_cost"][i])
                for i, (p, lo, hi, nlo, nhi) in enumerate(zip(mix.problems(), mix.arc_rows[:-1], mix.arc_rows[1:], mix.node_rows[:-1], mix.node_rows[1:]))]
        got = rows_of(validate(mix.handle(), rows, a))
        for i, w in enumerate(want):
            assert got["valid"][i] == w["valid"] and got["objective"][i] == w["objective"] and got["dual_cost"][i] == w["dual_cost"], i
            assert [int(x) for x in got["errors"][i]] == [w["errors"][k] for k in V.KINDS] and [int(x) for x in got["first"][i]] == [w["first"][k] for k in V.KINDS], i
        assert any(w["errors"]["conservation"] for w in want)


def test_graphs_of_equal_size_on_the_host():
    check_siblings(HOST[0], lambda h, rows, a: h.validate_on_host(rows, **a), 0)


def test_graphs_of_equal_node_count_on_the_host():
    check_siblings(HOST[0], lambda h, rows, a: h.validate_on_host(rows, **a), 1)


# ---- 4: re-solve
@functools.lru_cache(maxsize=None)
def resolve_mix():
    """The three re-solve graphs of test_uniform_host.py in one handle, interleaved.  A call has one supply type, so the handle runs the
    chain under each (the single-graph chain gives the middle graph LEQ and the others GEQ)."""
    return Mix([t for t, _ in resolve_family()])


def mix_costs(mix, step):
    return mix.flat([dict(cost=step_costs(t, j, step)) for j, t in enumerate(mix.tops)])["cost"]


@functools.lru_cache(maxsize=None)
def mix_resolve_reference(rule, stype):
    """per step, per graph: cold_reference per variant.  Asserted on the oracle alone: over the chain, instances re-solved warm, Optimal
    with a surplus (re-solved cold) and Infeasible all occur."""
    mix = resolve_mix()
    kinds = {"warm": 0, "surplus": 0, "infeasible": 0}
    out = []
    for step in range(STEPS):
        per_graph = []
        for j, t in enumerate(mix.tops):
            cost = step_costs(t, j, step)
            refs = tuple(cold_reference(with_cost(p, cost[k]), stype, rule) for k, p in enumerate(t.variants))
            assert all(st != O.UNBOUNDED for st, _, _ in refs)
            kinds["warm"] += sum(st == O.OPTIMAL and exact is None for st, _, exact in refs)
            kinds["surplus"] += sum(exact is not None for _, _, exact in refs)
            kinds["infeasible"] += sum(st == O.INFEASIBLE for st, _, _ in refs)
            per_graph.append(refs)
        out.append(tuple(per_graph))
    print(f"ragged re-solve chain, rule {rule}, supply type {stype}: {kinds}")
    assert kinds["warm"] >= 10 and kinds["infeasible"] >= 10 and (stype == O.LEQ or kinds["surplus"] >= 10), kinds
    return tuple(out)


def check_resolve_chain(first, again, rule, stypes=SUPPLY_TYPES, **kw):
    """Four re-solves, every variant meeting all four cost modes: the oracle's cold solve on status and cost, validate_solution on flows and
    potentials (assert_matches_cold per graph), BatchSolver.set_costs + rerun_on_host bit for bit."""
    mix = resolve_mix()
    a = mix.arrays()
    for stype in stypes:
        h = mix.handle(rule, **kw)
        r = first(h, a, stype)
        b = mix.batch_solver(rule, stype).run_on_host()
        assert_equals_answers(mix.split(r), batch_answers(b, mix.count), f"supply type {stype}, first solve")
        for step, per_graph in enumerate(mix_resolve_reference(rule, stype)):
            cost = mix_costs(mix, step)
            r = again(h, dict(a, cost=cost), stype)
            for j, t in enumerate(mix.tops):
                assert_matches_cold(mix.of_graph(r, j), t, stype, step_costs(t, j, step), per_graph[j], f"supply type {stype}, graph {j}, step {step}")
                assert all(KINDS[k % 3] == "excess" for k, (_, _, exact) in enumerate(per_graph[j]) if exact is not None)
            for i in range(mix.count):
                b.set_costs(i, cost[mix.arc_rows[i]:mix.arc_rows[i + 1]])
            b.rerun_on_host()
            assert_equals_answers(mix.split(r), batch_answers(b, mix.count), f"supply type {stype}, step {step}, BatchSolver")


@pytest.mark.parametrize("rule", ALL_RULES)
def test_resolve_chain_on_the_host(rule):
    check_resolve_chain(*HOST, rule)


def warm_rows(mix, rule, stype):
    return np.array([(lambda ref: ref[0] == O.OPTIMAL and ref[2] is None)(cold_reference(p, stype, rule)) for p in mix.problems()])


def check_unchanged_costs_and_mask(first, again, rule, **kw):
    mix = resolve_mix()
    a = mix.arrays()
    stype = O.GEQ
    warm = warm_rows(mix, rule, stype)
    assert warm.sum() >= 6 and not warm.all()
    # unchanged costs: nothing is eligible under the potentials of the same basis
    h = mix.handle(rule, **kw)
    before = to_numpy(first(h, a, stype))
    after = to_numpy(again(h, a, stype))
    assert not after["pivots"][warm].any() and not after["trace"][warm].any()
    assert np.array_equal(after["pivots"][~warm], before["pivots"][~warm]) and np.array_equal(after["trace"][~warm], before["trace"][~warm])
    for name in ("status", "total_cost", "flows", "potentials"):
        assert np.array_equal(after[name], before[name]), name
    # the mask: rows it leaves out keep their last outputs, the marked ones equal an unmasked re-solve's
    cost = mix_costs(mix, 1)
    mask = np.arange(mix.count) % 3 != 1
    h = mix.handle(rule, **kw)
    before = to_numpy(mix.split(first(h, a, stype)))
    masked = to_numpy(mix.split(again(h, dict(a, cost=cost), stype, changed=mask)))
    v = mix.handle(rule, **kw)
    first(v, a, stype)
    whole = to_numpy(mix.split(again(v, dict(a, cost=cost), stype)))
    for name in before:
        for i in range(mix.count):
            assert np.array_equal(masked[name][i], (whole if mask[i] else before)[name][i]), (name, i)
    assert not np.array_equal(whole["total_cost"][~mask], before["total_cost"][~mask])
    back = to_numpy(again(h, a, stype, changed=~mask))
    assert np.array_equal(back["total_cost"][~mask], before["total_cost"][~mask]) and np.array_equal(back["total_cost"][mask], masked["total_cost"][mask])
    assert (warm & ~mask).any() and not back["pivots"][warm & ~mask].any()
    assert h.stats()["total_pivots"] == back["pivots"][~mask].sum()


@pytest.mark.parametrize("rule", ALL_RULES)
def test_unchanged_costs_and_the_changed_mask_on_the_host(rule):
    check_unchanged_costs_and_mask(*HOST, rule)


# ---- 5: validation
class MixCase:
    """Cases of test_uniform_validate_host.py (one per graph, equal counts) in one handle, interleaved; expected: their oracle rows likewise."""

    def __init__(self, cases):
        self.cases = tuple(cases)
        c0 = self.cases[0]
        assert all(c.count == c0.count and c.stype == c0.stype for c in self.cases)
        self.stype, self.label = c0.stype, " + ".join(c.label for c in self.cases)
        G = len(self.cases)
        self.order = tuple((k % G, k // G) for k in range(G * c0.count))
        self.count = len(self.order)
        self.graphs = [(c.n, c.src, c.tgt) for c in self.cases]
        self.graph_of = np.array([g for g, _ in self.order], np.int32)
        cat = lambda rows: np.ascontiguousarray(np.concatenate([np.asarray(r).reshape(-1) for r in rows]))
        self.arrays = {name: (None if c0.arrays[name] is None else cat(self.cases[g].arrays[name][v] for g, v in self.order)) for name in PROBLEM_NAMES}
        self.rows = {name: cat(self.cases[g].rows[name][v] for g, v in self.order) for name in ROW_NAMES}
        self.expected = {name: np.stack([self.cases[g].expected[name][v] for g, v in self.order]) for name in OUT_NAMES}

    def handle(self):
        return M.RaggedBatch(self.graphs, self.graph_of)


def assert_equals_oracle(v, c, what=""):
    got, want = rows_of(v), c.expected
    for name in OUT_NAMES:
        assert got[name].dtype == want[name].dtype and got[name].shape == want[name].shape, (c.label, what, name)
        if not np.array_equal(got[name], want[name]):
            i = int(np.flatnonzero((got[name] != want[name]).reshape(c.count, -1).any(axis=1))[0])
            raise AssertionError((c.label, what, name, "instance", i, "graph", c.order[i], "got", got[name][i].tolist(), "expected", want[name][i].tolist()))
    invalid = np.flatnonzero(want["valid"] == 0)
    s = v.summary
    assert (s["instances"], s["invalid"], s["first_invalid"]) == (c.count, len(invalid), int(invalid[0]) if len(invalid) else -1), (c.label, what, s)


@functools.lru_cache(maxsize=None)
def solved_mix_cases(name):
    """per supply type: the solved rows of the whole family (Block Search), interleaved.  solved_cases() asserts its floors."""
    cases = solved_cases(name)
    G = len(family(name))
    return tuple(MixCase(cases[k * G:(k + 1) * G]) for k in range(2))


@functools.lru_cache(maxsize=None)
def corrupted_mix_cases(check_as=None):
    """per supply type: the corrupted rows of B's graphs of 65, 129 and 300 nodes in ONE handle.  Instance k of a graph is corrupted at
    position set k // 8 of arc_positions / node_positions: sets 0 and 2 hold the first and the last arc and node of the instance's row,
    so an off-by-one in a row offset reads the neighbour -- an instance of another graph."""
    cases = corrupted_cases(check_as)
    return tuple(MixCase(cases[k * 3:(k + 1) * 3]) for k in range(2))


def validate_on_host(c, **kw):
    return c.handle().validate_on_host(c.rows, supply_type=c.stype, **dict(c.arrays, **kw))


@pytest.mark.parametrize("name", ["A", "B"])
def test_solved_families_validate_on_the_host(name):
    mix = family_mix(name)
    for c in solved_mix_cases(name):
        r = to_numpy(mix.handle().run_on_host(supply_type=c.stype, **mix.arrays()))
        for field in ROW_NAMES:                         # the rows under validation are this handle's own
            assert np.array_equal(r[field], c.rows[field]), field
        v = validate_on_host(c)
        assert_equals_oracle(v, c)
        assert isinstance(v.valid, np.ndarray) and v.summary["bytes_up"] == v.summary["bytes_down"] == 0


def test_corruptions_validate_on_the_host():
    for c in corrupted_mix_cases() + corrupted_mix_cases(EQ):
        assert [n for n, _, _ in c.graphs] == [65, 129, 300]
        assert_equals_oracle(validate_on_host(c), c)
    c = corrupted_mix_cases()[0]
    assert c.expected["errors"][:, :9].any(axis=0).all()


# ---- 6: edges
def io_of(a, memory=L.MEM_HOST, stype=O.GEQ, **outputs):
    io = L.RBatchIo()
    io.memory, io.supply_type = memory, stype
    for name in PROBLEM_NAMES:
        if a.get(name) is not None:
            setattr(io, name, a[name].ctypes.data)
    for name, arr in outputs.items():
        setattr(io, name, arr.ctypes.data)
    return io


@functools.lru_cache(maxsize=None)
def small_mix():
    """family A's graphs of 63, 64 and 129 search arcs, every variant"""
    return Mix([family("A")[k] for k in (1, 2, 4)])


def check_empty_handles(run):
    for h in (M.RaggedBatch([], None, record_trace=8), M.RaggedBatch([], [], record_trace=8), M.RaggedBatch(small_mix().graphs, [], record_trace=8)):
        assert len(h) == 0 and h.arc_rows.tolist() == [0] and h.node_rows.tolist() == [0]
        r = run(h, np.zeros(0, np.int64), np.zeros(0, np.int64))
        st = h.stats()
        assert st["instances"] == st["launches"] == st["total_pivots"] == st["workspace_bytes"] == 0
        assert {k: v.shape for k, v in to_numpy(r).items()} == dict(status=(0,), pivots=(0,), total_cost=(0,), flows=(0,), potentials=(0,), trace=(0, 8))


def test_empty_handles_on_the_host():
    check_empty_handles(lambda h, cost, supply: h.run_on_host(cost, supply))
    h = M.RaggedBatch([], None)
    v = h.validate_on_host((np.zeros(0, np.int32), np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64)), np.zeros(0, np.int64), np.zeros(0, np.int64))
    assert (v.summary["instances"], v.summary["invalid"], v.summary["first_invalid"]) == (0, 0, -1)


def check_an_unused_graph(run):
    """A graph no instance names changes nothing, wherever it stands among the graphs"""
    mix = small_mix()
    want = run(mix.handle(), mix.arrays(), O.GEQ)
    spare = family("B")[6]
    for at in (0, 1, 3):
        tops = list(mix.tops)
        tops.insert(at, spare)
        other = Mix(tops, [(g + (g >= at), v) for g, v in mix.order])
        assert at not in other.graph_of
        assert_rows_equal(run(other.handle(), other.arrays(), O.GEQ), want, at)


def test_a_graph_no_instance_uses_on_the_host():
    check_an_unused_graph(HOST[0])


def check_nothing_runs(run):
    """Every instance infeasible by its bounds: nothing runs, every output is written."""
    mix = small_mix()
    a = mix.arrays()
    arcs = mix.arc_rows[:-1] + np.random.default_rng(20261104).integers(0, mix.m)
    a["upper"] = a["upper"].copy()
    a["upper"][arcs] = a["lower"][arcs] - 1
    h = mix.handle(record_trace=8)
    r = to_numpy(run(h, a))
    st = h.stats()
    assert st["launches"] == 0 and st["total_pivots"] == 0 and st["instances"] == mix.count
    assert np.all(r["status"] == O.INFEASIBLE) and r["status"].dtype == np.int32
    for name in ("pivots", "total_cost", "flows", "potentials", "trace"):
        assert not r[name].any(), name


def test_a_handle_infeasible_by_its_bounds_on_the_host():
    check_nothing_runs(lambda h, a: h.run_on_host(**a))


def check_absent_arrays(run):
    mix = small_mix()
    a = mix.arrays()
    zeros, inf = np.zeros_like(a["lower"]), np.full_like(a["upper"], O.INF_CAP)
    cost = np.abs(a["cost"])            # uncapacitated everywhere: no negative cycles
    for kw in (dict(lower=None, upper=a["upper"]), dict(lower=a["lower"], upper=None), dict(lower=None, upper=None)):
        full = dict(lower=zeros if kw["lower"] is None else kw["lower"], upper=inf if kw["upper"] is None else kw["upper"])
        r1 = run(mix.handle(), dict(cost=cost, supply=a["supply"], **kw))
        assert_rows_equal(r1, run(mix.handle(), dict(cost=cost, supply=a["supply"], **full)), tuple(kw))
        problems = [O.Problem(p.n, p.m, p.src, p.tgt, full["lower"][lo:hi], full["upper"][lo:hi], cost[lo:hi], p.supply)
                    for p, lo, hi in zip(mix.problems(), mix.arc_rows[:-1], mix.arc_rows[1:])]
        assert_equals_answers(mix.split(r1), [answer_of(p, O.RULE_BLOCK, O.GEQ) for p in problems], tuple(kw))
    # no cost and no supply: every instance Optimal at once
    r = to_numpy(run(mix.handle(), dict(cost=None, supply=None, lower=None, upper=a["upper"])))
    keep = ~np.array([bound_infeasible(p) for p in mix.problems()])
    assert np.all(r["status"][keep] == O.OPTIMAL) and not r["pivots"].any() and not r["flows"].any()


def test_absent_arrays_on_the_host():
    check_absent_arrays(lambda h, a: h.run_on_host(**a))


def check_null_outputs(call, memory=L.MEM_HOST):
    mix = small_mix()
    a = mix.arrays()
    full = to_numpy(mix.handle().run_on_host(**a))
    for name in full:
        h = mix.handle()
        out = np.full_like(full[name], -7)
        assert call(h._h, C.byref(io_of(a, memory, **{name: out}))) == 0
        assert np.array_equal(out, full[name]), name
    h = mix.handle()
    assert call(h._h, C.byref(io_of(a, memory))) == 0                   # no output at all
    assert h.stats()["total_pivots"] == full["pivots"].sum()
    status = np.full(mix.count, -7, np.int32)
    assert call(h._h, C.byref(io_of({}, memory, status=status))) == 0 and np.all(status == O.OPTIMAL) and h.stats()["total_pivots"] == 0


def test_null_output_pointers_on_the_host():
    check_null_outputs(L.lib().mcf_rbatch_run_on_host)


def check_short_and_absent_traces(run):
    graphs = (5, 7, 8)                  # family B's graphs of 127, 129 and 300 nodes: no solve of theirs that pivots at all ends after one pivot
    mix = Mix([family("B")[k] for k in graphs])
    answers = mix.pick([reference("B", O.RULE_BLOCK, O.GEQ)[k] for k in graphs])
    smallest = min(x[1] for x in answers if x[1] > 0)
    assert smallest >= 2
    for cap in (smallest // 2, 0):
        r = run(mix.handle(record_trace=cap), mix.arrays())
        assert to_numpy(r)["trace"].shape == (mix.count, cap)
        assert_equals_answers(mix.split(r), answers, f"trace capacity {cap}", trace_cap=cap)


def test_short_and_absent_traces_on_the_host():
    check_short_and_absent_traces(lambda h, a: h.run_on_host(**a))


def check_solve_twice(run):
    """A second solve on the same handle, with other supplies and the other supply type, equals two fresh handles."""
    mix = Mix([family("B")[k] for k in (3, 5, 6)])
    a = mix.arrays()
    other = dict(a, supply=np.ascontiguousarray(-a["supply"]))
    h = mix.handle()
    first, second, third = run(h, a, O.GEQ), run(h, other, O.LEQ), run(h, a, O.GEQ)
    assert_rows_equal(first, run(mix.handle(), a, O.GEQ), "first")
    assert_rows_equal(second, run(mix.handle(), other, O.LEQ), "second")
    assert_rows_equal(third, first, "third")
    assert not np.array_equal(to_numpy(first)["pivots"], to_numpy(second)["pivots"])
    problems = [O.Problem(p.n, p.m, p.src, p.tgt, p.lower, p.upper, p.cost, -p.supply) for p in mix.problems()]
    assert_equals_answers(mix.split(second), [answer_of(p, O.RULE_BLOCK, O.LEQ) for p in problems])


def test_solve_twice_on_the_host():
    check_solve_twice(lambda h, a, stype: h.run_on_host(supply_type=stype, **a))


def desc_of(graphs, graph_of, count=None, **kw):
    """(RBatchDesc, what keeps its arrays alive)"""
    node_count = np.array([n for n, _, _ in graphs], np.int32)
    arc_start = np.concatenate([[0], np.cumsum([len(s) for _, s, _ in graphs])]).astype(np.int64) if "arc_start" not in kw else np.asarray(kw.pop("arc_start"), np.int64)
    src = np.concatenate([np.asarray(s, np.int32) for _, s, _ in graphs] + [np.zeros(0, np.int32)]).astype(np.int32)
    tgt = np.concatenate([np.asarray(t, np.int32) for _, _, t in graphs] + [np.zeros(0, np.int32)]).astype(np.int32)
    of = None if graph_of is None else np.asarray(graph_of, np.int32)
    d = L.RBatchDesc(0, kw.pop("rule", L.RULE_BLOCK_SEARCH), kw.pop("semantics", L.SEM_PLAIN), 0, kw.pop("pivot_limit", 0), 0, kw.pop("record_trace", 0), kw.pop("flags", 0),
                     len(graphs), (len(graphs) if of is None else len(of)) if count is None else count, node_count.ctypes.data, arc_start.ctypes.data,
                     src.ctypes.data, tgt.ctypes.data, None if of is None else of.ctypes.data)
    assert not kw
    return d, (node_count, arc_start, src, tgt, of)


def refused(d):
    h = C.c_void_p()
    rc = L.lib().mcf_rbatch_create(C.byref(h), C.byref(d[0]))
    assert not h.value
    return rc, L.lib().mcf_last_error().decode()


def test_refusals_and_their_error_codes(have_gpu):
    lib = L.lib()
    mix = small_mix()
    a = mix.arrays()
    two = [(2, [0], [1]), (3, [0, 1], [1, 2])]
    for kw, word in ((dict(rule=M.PivotRule.CandidateList), "list rules"), (dict(rule=M.PivotRule.AlteringList), "list rules"), (dict(rule=9), "pivot rule"),
                     (dict(semantics=L.SEM_OPTIMIZED), "MCF_SEM_OPTIMIZED"), (dict(flags=L.BATCH_SHARDED), "sharding"), (dict(pivot_limit=-1), "negative"),
                     (dict(record_trace=-1), "negative")):
        with pytest.raises(M.McfError) as ei:
            M.RaggedBatch(two, [0, 1, 1], **kw)
        assert ei.value.code == L.ERR_INVALID and word in str(ei.value), word
    for d, word in ((desc_of(two, [0, 2]), "graph_of[1]"), (desc_of(two, [-1, 0]), "graph_of[0]"), (desc_of(two, None, count=3), "must equal graph_count"),
                    (desc_of(two, None, count=1), "must equal graph_count"), (desc_of(two, [0, 1], arc_start=[0, 2, 1]), "monotone"),
                    (desc_of(two, [0, 1], arc_start=[0, 3, 3]), "end point"),          # graph 0 reaches into graph 1's arcs: node 2 is not one of its two
                    (desc_of([(2, [0], [2]), two[1]], [0, 1]), "end point"), (desc_of([two[0], (3, [0, -1], [1, 2])], [0, 1]), "end point"),
                    (desc_of([two[0], (3, [0, 3], [1, 2])], [1]), "end point"),         # in a graph's own range, not in the sum of them
                    (desc_of([two[0], (-1, [], [])], [0]), "graph must not be null"),   # a negative node count: refused before any table is sized by it
                    (desc_of([(-3, [0], [0]), two[1]], [1, 1]), "graph must not be null"),
                    (desc_of(two, [0], count=-1), "negative"), (desc_of([], None, count=L.BATCH_MAX_INSTANCES + 1), "at most"),
                    (desc_of([(L.BATCH_MAX_NODES + 1, [], [])], [0]), "mcf_ns_solve"),
                    (desc_of([(2, np.zeros(L.BATCH_MAX_ARCS + 1, np.int32), np.zeros(L.BATCH_MAX_ARCS + 1, np.int32))], [0]), "mcf_ns_solve")):
        rc, message = refused(d)
        assert rc == L.ERR_INVALID and word in message, (word, message)
    d = desc_of(two, [0, 1])[0]
    d.graph_count = -1
    assert refused((d,))[0] == L.ERR_INVALID
    d, keep = desc_of(two, [0, 1])
    d.source = None
    assert refused((d,))[0] == L.ERR_INVALID                                            # arcs without end points
    d, keep = desc_of(two, [0, 1])
    d.node_count = None
    assert refused((d,))[0] == L.ERR_INVALID
    h = C.c_void_p()
    assert lib.mcf_rbatch_create(None, C.byref(d)) == L.ERR_INVALID and lib.mcf_rbatch_create(C.byref(h), None) == L.ERR_INVALID
    lib.mcf_rbatch_destroy(None)
    assert lib.mcf_rbatch_get_rows(None, None, None) == L.ERR_INVALID
    u = mix.handle()
    assert lib.mcf_rbatch_get_rows(u._h, None, None) == 0
    calls = (lib.mcf_rbatch_solve, lib.mcf_rbatch_resolve, lib.mcf_rbatch_run_on_host, lib.mcf_rbatch_rerun_on_host)
    for call in calls:
        assert call(None, C.byref(io_of(a))) == L.ERR_INVALID and call(u._h, None) == L.ERR_INVALID
        assert call(u._h, C.byref(io_of(a, stype=7))) == L.ERR_INVALID
        assert call(u._h, C.byref(io_of(a, stype=EQ))) == L.ERR_INVALID
        assert call(u._h, C.byref(io_of(a, memory=2))) == L.ERR_INVALID
    assert lib.mcf_rbatch_get_stats(None, C.byref(L.UBatchStats())) == L.ERR_INVALID and lib.mcf_rbatch_get_stats(u._h, None) == L.ERR_INVALID
    for call in calls[2:]:                              # the hooks read host memory only
        assert call(u._h, C.byref(io_of(a, memory=L.MEM_DEVICE))) == L.ERR_INVALID
    for call in (lib.mcf_rbatch_resolve, lib.mcf_rbatch_rerun_on_host):                 # a re-solve needs a solve
        assert call(u._h, C.byref(io_of(a))) == L.ERR_STATE
    for again in (u.resolve, u.rerun_on_host):
        with pytest.raises(M.McfError) as ei:
            again(**a)
        assert ei.value.code == L.ERR_STATE
        with pytest.raises(M.McfError) as ei:
            again(changed=np.ones(mix.count, bool), **a)
        assert ei.value.code == L.ERR_STATE
    # the validation's refusals
    rows = to_numpy(u.run_on_host(**a))
    summary = L.UBatchCheckSummary()

    def check_io(memory=L.MEM_HOST, stype=O.GEQ, **drop):
        io = L.RBatchCheckIo()
        io.memory, io.supply_type = memory, stype
        for name in PROBLEM_NAMES:
            setattr(io, name, a[name].ctypes.data)
        for name in ROW_NAMES:
            if name not in drop:
                setattr(io, name, rows[name].ctypes.data)
        return io
    for call in (lib.mcf_rbatch_validate, lib.mcf_rbatch_validate_on_host):
        assert call(None, C.byref(check_io()), C.byref(summary)) == L.ERR_INVALID and call(u._h, None, C.byref(summary)) == L.ERR_INVALID
        assert call(u._h, C.byref(check_io()), None) == L.ERR_INVALID
        assert call(u._h, C.byref(check_io(stype=3)), C.byref(summary)) == L.ERR_INVALID and call(u._h, C.byref(check_io(memory=2)), C.byref(summary)) == L.ERR_INVALID
        for name in ROW_NAMES:
            assert call(u._h, C.byref(check_io(**{name: True})), C.byref(summary)) == L.ERR_INVALID, name
    assert lib.mcf_rbatch_validate_on_host(u._h, C.byref(check_io(memory=L.MEM_DEVICE)), C.byref(summary)) == L.ERR_INVALID
    assert lib.mcf_rbatch_validate_on_host(u._h, C.byref(check_io(stype=EQ)), C.byref(summary)) == 0 and summary.instances == mix.count
    if not have_gpu:
        assert lib.mcf_rbatch_validate(u._h, C.byref(check_io()), C.byref(summary)) == L.ERR_NO_DEVICE
    # shapes, dtypes, contiguity, and numpy where the hooks are asked for lists of the wrong length
    for kw in (dict(a, cost=a["cost"][:-1]), dict(a, supply=a["supply"].astype(np.int32)), dict(a, cost=np.tile(a["cost"], 2)[::2]),
               dict(a, cost=a["cost"].reshape(1, -1)), dict(a, upper=a["upper"].astype(np.float64))):
        with pytest.raises(ValueError):
            u.run_on_host(**kw)
        with pytest.raises(ValueError):
            u.validate_on_host(rows, **kw)
    with pytest.raises(ValueError):
        u.rerun_on_host(changed=np.ones(mix.count + 1, bool), **a)
    with pytest.raises(ValueError):
        u.validate_on_host(dict(rows, flows=rows["flows"][:-1]), **a)
    with pytest.raises(ValueError):
        M.RaggedBatch([(2, [0, 1], [1])], [0])


def test_rbatch_structs_have_the_layout_of_the_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void){printf("%%zu %%zu %%zu %%zu %%zu %%zu %%zu %%zu %%zu %%zu %%zu\\n", '
                   'sizeof(mcf_rbatch_desc), sizeof(mcf_rbatch_io), sizeof(mcf_rbatch_check_io), offsetof(mcf_rbatch_desc, graph_count), offsetof(mcf_rbatch_desc, count), '
                   'offsetof(mcf_rbatch_desc, node_count), offsetof(mcf_rbatch_desc, graph_of), offsetof(mcf_rbatch_io, changed), offsetof(mcf_rbatch_io, trace), '
                   'offsetof(mcf_rbatch_check_io, status), offsetof(mcf_rbatch_check_io, dual_cost));return 0;}\n' % os.path.join(ROOT, "include", "mcf_hip.h"))
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(L.RBatchDesc), C.sizeof(L.RBatchIo), C.sizeof(L.RBatchCheckIo), L.RBatchDesc.graph_count.offset, L.RBatchDesc.count.offset,
                   L.RBatchDesc.node_count.offset, L.RBatchDesc.graph_of.offset, L.RBatchIo.changed.offset, L.RBatchIo.trace.offset,
                   L.RBatchCheckIo.status.offset, L.RBatchCheckIo.dual_cost.offset]
    assert [name for name, _ in L.RBatchDesc._fields_[:9]] == [name for name, _ in L.UBatchDesc._fields_[:8]] + ["graph_count"]


@pytest.mark.skipif(M.device_count() > 0, reason="a GPU is present")
def test_solve_without_a_device_leaves_the_handle_as_it_was():
    mix = resolve_mix()
    a = mix.arrays()
    h = mix.handle()
    for refused_call in (h.solve, h.resolve):           # an unsolved handle stays unsolved
        with pytest.raises(M.McfError) as ei:
            refused_call(**a)
        assert ei.value.code == (L.ERR_NO_DEVICE if refused_call == h.solve else L.ERR_STATE)
    with pytest.raises(M.McfError) as ei:
        h.rerun_on_host(**a)
    assert ei.value.code == L.ERR_STATE
    before = h.run_on_host(**a)
    stats = h.stats()
    cost = mix_costs(mix, 0)
    for refused_call in (h.solve, h.resolve):
        with pytest.raises(M.McfError) as ei:
            refused_call(**dict(a, cost=cost))
        assert ei.value.code == L.ERR_NO_DEVICE
    assert h.stats() == stats
    v = mix.handle()
    assert_rows_equal(v.run_on_host(**a), before)
    assert_rows_equal(h.rerun_on_host(**dict(a, cost=cost)), v.rerun_on_host(**dict(a, cost=cost)))


# ---- 7: the pivot limit (the references, floors and checkers of test_uniform_host.py on one handle)
def check_families_under_a_limit(run, name, rule, k, cap, **kw):
    """run(handle, arrays, stype) -> result.  Every row against the oracle's limited answer; the limit changes nothing of the statistics
    but the pivots."""
    mix = family_mix(name)
    a = mix.arrays()
    for stype in SUPPLY_TYPES:
        answers = mix.pick(limited_reference(name, rule, stype, k))
        h = mix.handle(rule, pivot_limit=k, record_trace=cap, **kw)
        r = run(h, a, stype)
        assert to_numpy(r)["trace"].shape == (mix.count, cap)
        assert_equals_answers(mix.split(r), answers, (f"family {name}, supply type {stype}, limit {k}, trace capacity {cap}", kw), trace_cap=cap)
        st = h.stats()
        assert st["instances"] == mix.count and st["total_pivots"] == sum(x[1] for x in answers) and st["workspace_bytes"] == footprints(mix), st
        yield stype, answers, h, r, st


@pytest.mark.parametrize("k, cap", LIMIT_RUNS)
@pytest.mark.parametrize("rule", ALL_RULES)
@pytest.mark.parametrize("name", ["A", "B"])
def test_families_under_a_pivot_limit_on_the_host(name, rule, k, cap):
    for stype, answers, h, r, st in check_families_under_a_limit(HOST[0], name, rule, k, cap):
        assert st["launches"] == st["bytes_up"] == st["bytes_down"] == st["lds_instances"] == st["global_instances"] == 0


MIX_RESOLVE_LIMIT = {O.RULE_BLOCK: 16, O.RULE_BEST: 10, O.RULE_FIRST: 23}     # per rule the smallest limit in 8..64 at which mix_limited_chain_reference() meets every class


def mix_cost_rows(mix, step):
    cost = mix_costs(mix, step)
    return cost, tuple(cost[lo:hi] for lo, hi in zip(mix.arc_rows[:-1], mix.arc_rows[1:]))


@functools.lru_cache(maxsize=None)
def mix_limited_chain_reference(rule):
    """per supply type: (the flat cost array and the cost rows of every step, limited_chain() of resolve_mix()).  Asserted on the references
    alone: summed over both supply types every class of CLASSES occurs."""
    mix = resolve_mix()
    k = MIX_RESOLVE_LIMIT[rule]
    costs = tuple(mix_cost_rows(mix, step) for step in range(STEPS))
    out = tuple((costs, limited_chain(mix.problems(), stype, rule, k, [rows for _, rows in costs])) for stype in SUPPLY_TYPES)
    classes = sum(ref[2] for _, ref in out)
    print(f"ragged re-solve chain under a pivot limit of {k}, rule {rule}: {dict(zip(CLASSES, classes.tolist()))}")
    assert classes.min() >= 1, classes
    return out


def check_resolve_chain_under_a_limit(first, again, rule, **kw):
    mix = resolve_mix()
    a = mix.arrays()
    k = MIX_RESOLVE_LIMIT[rule]
    for stype, (costs, ref) in zip(SUPPLY_TYPES, mix_limited_chain_reference(rule)):
        h = mix.handle(rule, pivot_limit=k, **kw)
        check_chain_under_a_limit(ref, mix.problems(), stype, k, [rows for _, rows in costs], lambda: first(h, a, stype), lambda step: again(h, dict(a, cost=costs[step][0]), stype),
                                  lambda: first(mix.handle(rule, pivot_limit=k, **kw), dict(a, cost=costs[-1][0]), stype), mix.split, (f"supply type {stype}", kw))


@pytest.mark.parametrize("rule", ALL_RULES)
def test_resolve_chain_under_a_pivot_limit_on_the_host(rule):
    check_resolve_chain_under_a_limit(*HOST, rule)


def check_unchanged_costs_and_mask_under_a_limit_mix(first, again, rule, **kw):
    mix = resolve_mix()
    a = mix.arrays()
    k = MIX_RESOLVE_LIMIT[rule]
    seen = [check_unchanged_costs_and_mask_under_a_limit(
        mix.problems(), stype, rule, k, lambda: mix.handle(rule, pivot_limit=k, **kw), lambda h: first(h, a, stype),
        lambda h, cost, changed: again(h, a if cost is None else dict(a, cost=cost), stype, **({} if changed is None else dict(changed=changed))),
        mix_costs(mix, 1), mix.split, (f"supply type {stype}", kw)) for stype in SUPPLY_TYPES]
    assert_limit_floors(seen, f"ragged handle under a pivot limit of {k}, rule {rule}")


@pytest.mark.parametrize("rule", ALL_RULES)
def test_unchanged_costs_and_the_changed_mask_under_a_pivot_limit_on_the_host(rule):
    check_unchanged_costs_and_mask_under_a_limit_mix(*HOST, rule)


@functools.lru_cache(maxsize=None)
def limited_mix_cases(name, k=16):
    """per supply type: limited_validation_cases() of the whole family -- the oracle's answers under the limit as solution rows -- interleaved"""
    cases = limited_validation_cases(name, k)
    G = len(family(name))
    return tuple(MixCase(cases[j * G:(j + 1) * G]) for j in range(2))


def check_validation_under_a_limit(first, validate, again, name="B", k=16):
    """first(h, arrays, stype), validate(h, result, arrays, stype), again(h, arrays, stype).  The result goes into the validation as it lies;
    the re-solve behind it equals one that no validation preceded.  Yields (case, validation)."""
    mix = family_mix(name)
    a = mix.arrays()
    for c in limited_mix_cases(name, k):
        h, w = mix.handle(pivot_limit=k), mix.handle(pivot_limit=k)
        r = first(h, a, c.stype)
        rows = to_numpy(r)
        for field in ROW_NAMES:                         # the rows under validation are this handle's own
            assert np.array_equal(rows[field], c.rows[field]), (c.label, field)
        assert (rows["status"] == NOT_SOLVED).sum() >= 10
        stats = h.stats()
        v = validate(h, r, a, c.stype)
        assert_equals_oracle(v, c)
        assert h.stats() == stats
        yield c, v
        HOST[0](w, a, c.stype)
        assert_rows_equal(again(h, a, c.stype), HOST[1](w, a, c.stype), (c.label, "the validation left the state alone"))


def test_validation_of_limit_stopped_results_on_the_host():
    for c, v in check_validation_under_a_limit(HOST[0], lambda h, r, a, stype: h.validate_on_host(r, supply_type=stype, **a), HOST[1]):
        assert isinstance(v.valid, np.ndarray) and v.summary["bytes_up"] == v.summary["bytes_down"] == 0
