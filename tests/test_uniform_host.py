"""The uniform batch (mcf_ubatch_*, UniformBatch, DESIGN.md 3.14 "Uniform batch") without a GPU: mcf_ubatch_run_on_host / _rerun_on_host run
the device's own set-up, re-cost and finish steps (csrc/uniform_step.hip.h) and its pivot code with one lane on the CPU.

Every comparison is exact.  The references are the CPU oracle as test_batch_host.py builds it (status, pivot count, whole trace, and for
Optimal cost, flows and potentials) and the same instances put through BatchSolver.add + run_on_host.  test_uniform_gpu.py imports the
families and the checkers from here."""
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
from helpers import validate_solution
from test_batch_host import ROOT, RULES, bound_infeasible, footprint, oracle_of
from test_batch_resolve_host import cold_reference, new_cost, warm_after, with_cost

ALL_RULES = [O.RULE_BLOCK, O.RULE_BEST, O.RULE_FIRST]
SUPPLY_TYPES = [O.GEQ, O.LEQ]
SEED = 20261020          # chosen on the CPU: the first seed from 20261019 on at which the oracle meets the floors of reference() without overflow
PER = 24                 # variants per topology
TRACE = 4096             # above the longest solve of both families (asserted in reference())
A_SIZES = (3, 63, 64, 65, 129, 257, 640, 1000)          # m + n: the strides of the searches
B_NODES = (1, 2, 63, 64, 65, 127, 128, 129, 300)        # n, with m = 2 n: the strides of the prefix count and of the node-indexed writes
KINDS = ("balanced", "negative", "excess")
BY_BOUNDS = 13           # the variant of every topology that is infeasible by its bounds


class Topology:
    """One graph and its variants: problems that differ in costs, supplies and bounds only."""

    def __init__(self, n, src, tgt, variants, zero_capacity):
        self.n, self.m, self.src, self.tgt = n, len(src), src, tgt
        self.variants = tuple(variants)
        self.zero_capacity = tuple(zero_capacity)
        self.count = len(variants)

    def stack(self, field):
        return np.ascontiguousarray(np.stack([getattr(p, field) for p in self.variants]))

    def arrays(self):
        return dict(cost=self.stack("cost"), supply=self.stack("supply"), lower=self.stack("lower"), upper=self.stack("upper"))

    def subset(self, keep):
        return Topology(self.n, self.src, self.tgt, [self.variants[k] for k in keep], [self.zero_capacity[k] for k in keep])


def on_topology(p, src, tgt):
    return O.Problem(p.n, p.m, src, tgt, p.lower, p.upper, p.cost, p.supply)


def shifted_supply(p):
    s = p.supply.copy()
    np.subtract.at(s, p.src, p.lower)
    np.add.at(s, p.tgt, p.lower)
    return s


def draw_topology(tag, index, n, m, big_cost=True):
    """24 variants of one random graph, each from a seed of its own, the generator's src / tgt replaced by the shared pair (its other draws
    do not depend on them).  By the running index g over the family: kind g % 3; costs plain / ties / BIG_COST / plain by g % 4; zero
    capacities allowed every 11th; variant BY_BOUNDS infeasible by its bounds.  Uncapacitated arcs as adversarial_batch: 0.1 of them, none
    in seven of eight negative-cost variants and none above 257 search arcs."""
    rng = np.random.default_rng([SEED, tag, index])
    src, tgt = rng.integers(0, n, m).astype(np.int32), rng.integers(0, n, m).astype(np.int32)
    variants, zero = [], []
    for k in range(PER):
        g = index * PER + k
        kind, mode = KINDS[g % 3], g % 4
        inf_fraction = 0.0 if kind == "negative" and ((g // 3) % 8 != 0 or m + n > 257) else 0.1
        zero.append(g % 11 == 5)
        p = random_problem(np.random.default_rng([SEED, tag, index, k]), n, m, kind, cost_scale=BIG_COST if mode == 2 and big_cost else 1, ties=mode == 1,
                           zero_capacity=zero[-1], inf_fraction=inf_fraction, bound_infeasible=k == BY_BOUNDS)
        variants.append(on_topology(p, src, tgt))
    return Topology(n, src, tgt, variants, zero)


@functools.lru_cache(maxsize=None)
def family(name):
    """A: one topology per search range m + n of A_SIZES, n <= 60.  B: one per node count of B_NODES with m = 2 n, no BIG_COST above 129
    nodes (art_cost = (max |cost| + 1) n stays far inside int64); in variants 1 and 4 mod 6 the largest positive (negative) supplies are
    moved onto nodes 63, 64 and n - 1, so that under GEQ (LEQ) the nodes that need an artificial arc lie on both sides of every multiple of
    the wave -- asserted on the shifted supplies."""
    out = []
    if name == "A":
        rng = np.random.default_rng([SEED, 0])
        for index, size in enumerate(A_SIZES):
            n = int(rng.integers(1, min(size - 1, 60) + 1))
            out.append(draw_topology(1, index, n, size - n))
    else:
        for index, n in enumerate(B_NODES):
            t = draw_topology(2, index, n, 2 * n, big_cost=n <= 129)
            if n >= 64:
                spots = sorted({spot for spot in (63, 64, n - 1) if spot < n})
                variants = list(t.variants)
                for k in range(PER):
                    sign = {1: 1, 4: -1}.get(k % 6)
                    if sign is None or k == BY_BOUNDS:
                        continue
                    p = variants[k]
                    supply = p.supply.copy()
                    for spot in spots:
                        shifted = shifted_supply(O.Problem(p.n, p.m, p.src, p.tgt, p.lower, p.upper, p.cost, supply))
                        shifted[spots] = 0                      # not one of the spots themselves
                        donor = int(np.argmax(sign * shifted))
                        supply[spot], supply[donor] = supply[donor], supply[spot]
                    variants[k] = O.Problem(p.n, p.m, p.src, p.tgt, p.lower, p.upper, p.cost, supply)
                t = Topology(t.n, t.src, t.tgt, variants, t.zero_capacity)
                for stype, hung in ((O.GEQ, lambda s: s > 0), (O.LEQ, lambda s: s < 0)):
                    for spot in spots:
                        assert any(hung(shifted_supply(p))[spot] for p in t.variants if not bound_infeasible(p)), (n, stype, spot)
            out.append(t)
    assert all(t.count == PER and sum(bound_infeasible(p) for p in t.variants) == 1 for t in out)
    return tuple(out)


def answer_of(p, rule, stype, trace_cap=TRACE):
    """(status, pivots, trace, total cost, flows, potentials) of the oracle, the last three None unless Optimal; its numbers did not overflow."""
    o, st, tr = oracle_of(p, rule, stype, trace_cap=trace_cap)
    assert trace_cap < TRACE or (o.n_pivots < trace_cap and len(tr) == o.n_pivots)
    if st != O.OPTIMAL:
        return st, o.n_pivots, np.array(tr, np.int32), None, None, None
    assert o.total_cost == sum(int(f) * int(c) for f, c in zip(o.flow(), p.cost))
    assert max((abs(int(v)) for v in o.potential()), default=0) < 1 << 62
    return st, o.n_pivots, np.array(tr, np.int32), o.total_cost, o.flow().copy(), o.potential().copy()


@functools.lru_cache(maxsize=None)
def reference(name, rule, stype):
    """Per topology of family(name) a tuple of answer_of() per variant.  The floors are asserted here, on the oracle's answers alone: at
    least 10 Optimal and 10 Infeasible after pivots, and in family A at least 3 Unbounded among the zero-capacity variants."""
    out = []
    optimal = infeasible = unbounded = 0
    for t in family(name):
        row = tuple(answer_of(p, rule, stype) for p in t.variants)
        for p, zero, a in zip(t.variants, t.zero_capacity, row):
            optimal += a[0] == O.OPTIMAL
            infeasible += a[0] == O.INFEASIBLE and a[1] > 0
            unbounded += a[0] == O.UNBOUNDED and zero
            if bound_infeasible(p):
                assert a[0] == O.INFEASIBLE and a[1] == 0
        out.append(row)
    print(f"family {name}, rule {rule}, supply type {stype}: Optimal {optimal}, Infeasible after pivots {infeasible}, Unbounded by zero capacities {unbounded}, "
          f"longest solve {max(a[1] for row in out for a in row)} pivots")
    assert optimal >= 10 and infeasible >= 10, (optimal, infeasible)
    assert name != "A" or unbounded >= 3, unbounded
    return tuple(out)


def to_numpy(r):
    """A UniformResult's rows as numpy arrays, wherever they are."""
    get = lambda a: a if isinstance(a, np.ndarray) else a.cpu().numpy()
    return {name: get(getattr(r, name)) for name, _, _ in M.UniformResult.FIELDS}


def assert_rows_equal(a, b, what=""):
    a, b = to_numpy(a), to_numpy(b)
    for name in a:
        assert a[name].dtype == b[name].dtype and np.array_equal(a[name], b[name]), (what, name)


def assert_equals_answers(r, answers, what="", trace_cap=TRACE):
    """Every row of the result against answer_of()'s tuple, none left out; rows that are not Optimal are zero."""
    r = to_numpy(r)
    assert len(r["status"]) == len(answers)
    for i, (st, pivots, tr, total, flows, potentials) in enumerate(answers):
        where = (what, i)
        assert r["status"][i] == st, (where, r["status"][i], st)
        assert r["pivots"][i] == pivots, (where, r["pivots"][i], pivots)
        kept = min(pivots, trace_cap)
        assert np.array_equal(r["trace"][i][:kept], tr[:kept]) and not r["trace"][i][kept:].any(), where
        if st == O.OPTIMAL:
            assert r["total_cost"][i] == total, where
            assert np.array_equal(r["flows"][i], flows) and np.array_equal(r["potentials"][i], potentials), where
        else:
            assert r["total_cost"][i] == 0 and not r["flows"][i].any() and not r["potentials"][i].any(), where


def batch_answers(b, count):
    """answer_of()'s tuples read off a solved BatchSolver."""
    out = []
    for i in range(count):
        st = b.status(i)
        optimal = st == M.SolverStatus.Optimal
        out.append((st, b.pivots(i), b.trace(i), b.total_cost(i) if optimal else None, b.flows(i) if optimal else None, b.potentials(i) if optimal else None))
    return out


def batch_solver_of(t, rule, stype, **kw):
    b = M.BatchSolver(rule=RULES[rule], record_trace=kw.pop("record_trace", TRACE), **kw)
    for p in t.variants:
        b.add(p, supply_type=stype)
    return b


def uniform_of(t, rule, **kw):
    return M.UniformBatch(t.n, t.src, t.tgt, t.count, rule=RULES[rule], record_trace=kw.pop("record_trace", TRACE), **kw)


def stride_of(t):
    """The workspace of DESIGN.md 3.14 for an instance whose every node needs an artificial arc."""
    return footprint(t.m + 2 * t.n, t.n + 1)


# ---- 1
@pytest.mark.parametrize("rule", ALL_RULES)
@pytest.mark.parametrize("name", ["A", "B"])
def test_families_on_the_host(name, rule):
    for stype in SUPPLY_TYPES:
        refs = reference(name, rule, stype)
        for t, answers in zip(family(name), refs):
            u = uniform_of(t, rule)
            r = u.run_on_host(supply_type=stype, **t.arrays())
            assert_equals_answers(r, answers, f"family {name}, n {t.n}, m {t.m}, supply type {stype}")
            b = batch_solver_of(t, rule, stype).run_on_host()
            assert_equals_answers(r, batch_answers(b, t.count), "BatchSolver")
            st = u.stats()
            assert st["instances"] == t.count and st["total_pivots"] == sum(a[1] for a in answers) and st["workspace_bytes"] == t.count * stride_of(t)
            assert st["launches"] == st["bytes_up"] == st["bytes_down"] == 0


def picked(name="A", size_index=4):
    return family(name)[size_index]


# ---- 2
def test_shared_arrays_equal_the_same_data_tiled():
    t = picked()
    a = t.arrays()
    for shared in (("cost",), ("supply",), ("lower", "upper"), ("cost", "supply", "lower", "upper")):
        one = {k: (v[3].copy() if k in shared else v) for k, v in a.items()}
        tiled = {k: (np.ascontiguousarray(np.tile(v[3], (t.count, 1))) if k in shared else v) for k, v in a.items()}
        r1 = uniform_of(t, O.RULE_BLOCK).run_on_host(**one)
        r2 = uniform_of(t, O.RULE_BLOCK).run_on_host(**tiled)
        assert_rows_equal(r1, r2, shared)
        assert len(set(to_numpy(r1)["status"])) > 1 or shared != ("cost",)
    # strided views: rows of a wider array, and a row repeated by a zero stride
    wide = np.zeros((t.count, t.m + 5), np.int64)
    wide[:, :t.m] = a["cost"]
    r3 = uniform_of(t, O.RULE_BLOCK).run_on_host(**dict(a, cost=wide[:, :t.m]))
    assert_rows_equal(r3, uniform_of(t, O.RULE_BLOCK).run_on_host(**a), "row stride above m")
    with pytest.raises(ValueError):
        uniform_of(t, O.RULE_BLOCK).run_on_host(**dict(a, cost=np.asfortranarray(a["cost"])))
    with pytest.raises(ValueError):
        uniform_of(t, O.RULE_BLOCK).run_on_host(**dict(a, cost=a["cost"][:, :-1]))
    with pytest.raises(ValueError):
        uniform_of(t, O.RULE_BLOCK).run_on_host(**dict(a, supply=a["supply"].astype(np.int32)))


# ---- 3
def test_absent_bounds_are_zero_and_uncapacitated():
    t = picked()
    a = t.arrays()
    zeros, inf = np.zeros_like(a["lower"]), np.full_like(a["upper"], O.INF_CAP)
    cost = np.abs(a["cost"])            # uncapacitated everywhere: no negative cycles
    for kw in (dict(lower=None, upper=a["upper"]), dict(lower=a["lower"], upper=None), dict(lower=None, upper=None)):
        full = dict(lower=zeros if kw["lower"] is None else kw["lower"], upper=inf if kw["upper"] is None else kw["upper"])
        r1 = uniform_of(t, O.RULE_BLOCK).run_on_host(cost, a["supply"], **kw)
        r2 = uniform_of(t, O.RULE_BLOCK).run_on_host(cost, a["supply"], **full)
        assert_rows_equal(r1, r2, kw.keys())
        variants = [O.Problem(p.n, p.m, p.src, p.tgt, full["lower"][k], full["upper"][k], cost[k], p.supply) for k, p in enumerate(t.variants)]
        assert_equals_answers(r1, [answer_of(p, O.RULE_BLOCK, O.GEQ) for p in variants])


# ---- 4
def check_empty_batch(run):
    t = picked()
    u = M.UniformBatch(t.n, t.src, t.tgt, 0, record_trace=8)
    r = run(u, np.zeros((0, t.m), np.int64), np.zeros((0, t.n), np.int64))
    st = u.stats()
    assert st["instances"] == st["launches"] == st["total_pivots"] == st["workspace_bytes"] == 0
    assert {k: v.shape for k, v in to_numpy(r).items()} == dict(status=(0,), pivots=(0,), total_cost=(0,), flows=(0, t.m), potentials=(0, t.n), trace=(0, 8))


def test_an_empty_batch_on_the_host():
    check_empty_batch(lambda u, cost, supply: u.run_on_host(cost, supply))


# ---- 5
def by_bounds_only():
    t = picked()
    a = t.arrays()
    arcs = np.random.default_rng(SEED).integers(0, t.m, t.count)
    a["upper"] = a["upper"].copy()
    a["upper"][np.arange(t.count), arcs] = a["lower"][np.arange(t.count), arcs] - 1
    return t, a


def check_nothing_runs(run):
    """Every variant infeasible by its bounds: nothing runs, every output is written."""
    t, a = by_bounds_only()
    u = uniform_of(t, O.RULE_BLOCK, record_trace=8)
    r = to_numpy(run(u, a))
    st = u.stats()
    assert st["launches"] == 0 and st["total_pivots"] == 0 and st["instances"] == t.count
    assert np.all(r["status"] == O.INFEASIBLE) and r["status"].dtype == np.int32
    for name in ("pivots", "total_cost", "flows", "potentials", "trace"):
        assert not r[name].any(), name


def test_a_batch_infeasible_by_its_bounds_on_the_host():
    check_nothing_runs(lambda u, a: u.run_on_host(**a))


# ---- 6
def io_of(t, a, memory=L.MEM_HOST, **outputs):
    io = L.UBatchIo()
    io.memory, io.supply_type = memory, O.GEQ
    for name in ("cost", "supply", "lower", "upper"):
        setattr(io, name, a[name].ctypes.data)
        setattr(io, name + "_stride", a[name].shape[1])
    for name, arr in outputs.items():
        setattr(io, name, arr.ctypes.data)
    return io


def test_null_output_pointers():
    t = picked()
    a = t.arrays()
    lib = L.lib()
    full = to_numpy(uniform_of(t, O.RULE_BLOCK).run_on_host(**a))
    for name in full:
        u = uniform_of(t, O.RULE_BLOCK)
        out = np.full_like(full[name], -7)
        assert lib.mcf_ubatch_run_on_host(u._h, C.byref(io_of(t, a, **{name: out}))) == 0
        assert np.array_equal(out, full[name]), name
    u = uniform_of(t, O.RULE_BLOCK)
    assert lib.mcf_ubatch_run_on_host(u._h, C.byref(io_of(t, a))) == 0            # no output at all
    assert u.stats()["total_pivots"] == full["pivots"].sum()
    # null inputs: costs and supplies 0, every variant Optimal at once
    io = L.UBatchIo()
    status = np.full(t.count, -7, np.int32)
    io.status = status.ctypes.data
    assert lib.mcf_ubatch_run_on_host(u._h, C.byref(io)) == 0 and np.all(status == O.OPTIMAL) and u.stats()["total_pivots"] == 0


# ---- 7
def check_short_and_absent_traces(run, name="A"):
    t = picked(name)
    answers = reference(name, O.RULE_BLOCK, O.GEQ)[family(name).index(t)]
    smallest = min(a[1] for a in answers if a[1] > 0)
    assert smallest >= 2
    for cap in (smallest // 2, 0):
        r = run(uniform_of(t, O.RULE_BLOCK, record_trace=cap), t.arrays())
        assert to_numpy(r)["trace"].shape == (t.count, cap)
        assert_equals_answers(r, answers, f"trace capacity {cap}", trace_cap=cap)


def test_short_and_absent_traces_on_the_host():
    check_short_and_absent_traces(lambda u, a: u.run_on_host(**a))


# ---- 8
def test_refusals_and_their_error_codes(have_gpu):
    lib = L.lib()
    t = picked()
    a = t.arrays()
    for kw, word in ((dict(rule=M.PivotRule.CandidateList), "list rules"), (dict(rule=M.PivotRule.AlteringList), "list rules"), (dict(rule=9), "pivot rule"),
                     (dict(semantics=L.SEM_OPTIMIZED), "MCF_SEM_OPTIMIZED"), (dict(flags=L.BATCH_SHARDED), "sharding"), (dict(pivot_limit=-1), "negative"),
                     (dict(record_trace=-1), "negative"), (dict(count=-1), "negative instance count"), (dict(count=L.BATCH_MAX_INSTANCES + 1), "at most")):
        with pytest.raises(M.McfError) as ei:
            M.UniformBatch(t.n, t.src, t.tgt, kw.pop("count", 4), **kw)
        assert ei.value.code == L.ERR_INVALID and word in str(ei.value), word
    for src, tgt in (([0, t.n], [0, 0]), ([0, -1], [0, 0]), ([0, 0], [t.n, 0])):
        with pytest.raises(M.McfError) as ei:
            M.UniformBatch(t.n, src, tgt, 4)
        assert ei.value.code == L.ERR_INVALID and "end point" in str(ei.value)
    with pytest.raises(M.McfError) as ei:
        M.UniformBatch(2, np.zeros(L.BATCH_MAX_ARCS + 1, np.int32), np.zeros(L.BATCH_MAX_ARCS + 1, np.int32), 1)
    assert ei.value.code == L.ERR_INVALID and "mcf_ns_solve" in str(ei.value)
    with pytest.raises(M.McfError) as ei:
        M.UniformBatch(L.BATCH_MAX_NODES + 1, [], [], 1)
    assert ei.value.code == L.ERR_INVALID
    h = C.c_void_p()
    d = L.UBatchDesc(0, L.RULE_BLOCK_SEARCH, L.SEM_PLAIN, 0, 0, 0, 0, 0, 2, 1, 1, None, None)
    assert lib.mcf_ubatch_create(C.byref(h), C.byref(d)) == L.ERR_INVALID          # arcs without end points
    assert lib.mcf_ubatch_create(None, C.byref(d)) == L.ERR_INVALID and lib.mcf_ubatch_create(C.byref(h), None) == L.ERR_INVALID
    lib.mcf_ubatch_destroy(None)
    u = uniform_of(t, O.RULE_BLOCK)
    calls = (lib.mcf_ubatch_solve, lib.mcf_ubatch_resolve, lib.mcf_ubatch_run_on_host, lib.mcf_ubatch_rerun_on_host)
    for call in calls:
        assert call(None, C.byref(io_of(t, a))) == L.ERR_INVALID and call(u._h, None) == L.ERR_INVALID
        io = io_of(t, a)
        io.supply_type = 7
        assert call(u._h, C.byref(io)) == L.ERR_INVALID
        io = io_of(t, a, memory=2)
        assert call(u._h, C.byref(io)) == L.ERR_INVALID
        io = io_of(t, a)
        io.cost_stride = -1
        assert call(u._h, C.byref(io)) == L.ERR_INVALID
    assert lib.mcf_ubatch_get_stats(None, C.byref(L.UBatchStats())) == L.ERR_INVALID and lib.mcf_ubatch_get_stats(u._h, None) == L.ERR_INVALID
    # the hooks read host memory only
    for call in calls[2:]:
        assert call(u._h, C.byref(io_of(t, a, memory=L.MEM_DEVICE))) == L.ERR_INVALID
    # a re-solve needs a solve
    for call in (lib.mcf_ubatch_resolve, lib.mcf_ubatch_rerun_on_host):
        assert call(u._h, C.byref(io_of(t, a))) == L.ERR_STATE
    for again in (u.resolve, u.rerun_on_host):
        with pytest.raises(M.McfError) as ei:
            again(**a)
        assert ei.value.code == L.ERR_STATE
        with pytest.raises(M.McfError) as ei:
            again(changed=np.ones(t.count, bool), **a)
        assert ei.value.code == L.ERR_STATE
    if not have_gpu:
        with pytest.raises(M.McfError) as ei:
            u.solve(**a)
        assert ei.value.code == L.ERR_NO_DEVICE
        assert lib.mcf_ubatch_rerun_on_host(u._h, C.byref(io_of(t, a))) == L.ERR_STATE      # the refused call left the handle unsolved
    r = u.run_on_host(**a)
    if not have_gpu:
        with pytest.raises(M.McfError) as ei:
            u.resolve(**a)
        assert ei.value.code == L.ERR_NO_DEVICE
        assert_rows_equal(u.rerun_on_host(**a), rerun_reference(t, a, r), "after a refused resolve")
    # shapes, and numpy where the hooks are asked for tensors or lists of the wrong length
    with pytest.raises(ValueError):
        u.run_on_host(a["cost"][:-1], a["supply"])
    with pytest.raises(ValueError):
        u.rerun_on_host(changed=np.ones(t.count + 1, bool), **a)


def rerun_reference(t, a, first):
    """What a re-solve with unchanged costs gives after `first`: warm rows with 0 pivots, cold ones again."""
    u = uniform_of(t, O.RULE_BLOCK)
    assert_rows_equal(u.run_on_host(**a), first)
    return u.rerun_on_host(**a)


def test_ubatch_structs_have_the_layout_of_the_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void){printf("%%zu %%zu %%zu %%zu %%zu %%zu %%zu %%zu\\n", sizeof(mcf_ubatch_desc), '
                   'sizeof(mcf_ubatch_io), sizeof(mcf_ubatch_stats), offsetof(mcf_ubatch_desc, node_count), offsetof(mcf_ubatch_desc, source), offsetof(mcf_ubatch_io, changed), '
                   'offsetof(mcf_ubatch_io, trace), offsetof(mcf_ubatch_stats, bytes_up));return 0;}\n' % os.path.join(ROOT, "include", "mcf_hip.h"))
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(L.UBatchDesc), C.sizeof(L.UBatchIo), C.sizeof(L.UBatchStats), L.UBatchDesc.node_count.offset, L.UBatchDesc.source.offset,
                   L.UBatchIo.changed.offset, L.UBatchIo.trace.offset, L.UBatchStats.bytes_up.offset]
    header = open(os.path.join(ROOT, "include", "mcf_hip.h")).read()
    assert f"#define MCF_MEM_HOST {L.MEM_HOST}" in header and f"#define MCF_MEM_DEVICE {L.MEM_DEVICE}" in header


# ---- 9
def check_solve_twice(run):
    """A second solve on the same handle, with other supplies and the other supply type, equals two fresh handles."""
    t = picked("B", 5)
    a = t.arrays()
    other = dict(a, supply=np.ascontiguousarray(-a["supply"][::-1]))
    u = uniform_of(t, O.RULE_BLOCK)
    first = run(u, a, O.GEQ)
    second = run(u, other, O.LEQ)
    third = run(u, a, O.GEQ)
    assert_rows_equal(first, run(uniform_of(t, O.RULE_BLOCK), a, O.GEQ), "first")
    assert_rows_equal(second, run(uniform_of(t, O.RULE_BLOCK), other, O.LEQ), "second")
    assert_rows_equal(third, first, "third")
    assert not np.array_equal(to_numpy(first)["pivots"], to_numpy(second)["pivots"])
    assert_equals_answers(second, [answer_of(O.Problem(p.n, p.m, p.src, p.tgt, p.lower, p.upper, p.cost, other["supply"][k]), O.RULE_BLOCK, O.LEQ)
                                   for k, p in enumerate(t.variants)])


def test_solve_twice_on_the_host():
    check_solve_twice(lambda u, a, stype: u.run_on_host(supply_type=stype, **a))


# ---- 10: re-solve
RESOLVE_SIZES = (3, 5, 7)            # indices into A_SIZES: 65, 257 and 1000 search arcs
RESOLVE_PER = 12
STEPS = 4


@functools.lru_cache(maxsize=None)
def resolve_family():
    """((topology, supply type) ...): family A's graphs of 65, 257 and 1000 search arcs with 12 variants of finite, positive capacity each (the
    family of test_batch_resolve_host.py on shared graphs: status and optimum do not depend on the pivot path); kinds by k % 3, so a third
    are the "excess" kind, which ends Optimal with a surplus on an artificial arc and is re-solved cold; the last variant is infeasible by
    its bounds.  LEQ for the middle graph."""
    out = []
    for j, index in enumerate(RESOLVE_SIZES):
        t = family("A")[index]
        variants = []
        for k in range(RESOLVE_PER):
            p = random_problem(np.random.default_rng([SEED, 3, index, k]), t.n, t.m, KINDS[k % 3], zero_capacity=False, inf_fraction=0.0,
                               bound_infeasible=k == RESOLVE_PER - 1)
            assert k == RESOLVE_PER - 1 or (np.all(p.upper > p.lower) and np.all(p.upper < O.INF_CAP))
            variants.append(on_topology(p, t.src, t.tgt))
        assert any(np.any(p.lower != 0) for p in variants)
        out.append((Topology(t.n, t.src, t.tgt, variants, [False] * RESOLVE_PER), O.LEQ if j == 1 else O.GEQ))
    return tuple(out)


def step_costs(t, j, step):
    return np.stack([new_cost(p, 100 * j + k, step) for k, p in enumerate(t.variants)])


@functools.lru_cache(maxsize=None)
def resolve_reference(rule):
    """per graph, per step: (cost rows, (status, total cost, exact) of the oracle's cold solve per variant).  Asserted on the oracle alone: every
    step of every graph has Optimal answers that conserve flow (re-solved warm), and over the chain Infeasible ones and Optimal ones with a
    surplus (re-solved cold) occur."""
    out = []
    kinds = {"warm": 0, "surplus": 0, "infeasible": 0}
    for j, (t, stype) in enumerate(resolve_family()):
        steps = []
        for step in range(STEPS):
            cost = step_costs(t, j, step)
            refs = tuple(cold_reference(with_cost(p, cost[k]), stype, rule) for k, p in enumerate(t.variants))
            assert sum(st == O.OPTIMAL and exact is None for st, _, exact in refs) >= 2 and all(st != O.UNBOUNDED for st, _, _ in refs)
            kinds["warm"] += sum(st == O.OPTIMAL and exact is None for st, _, exact in refs)
            kinds["surplus"] += sum(exact is not None for _, _, exact in refs)
            kinds["infeasible"] += sum(st == O.INFEASIBLE for st, _, _ in refs)
            steps.append((cost, refs))
        out.append(tuple(steps))
    print(f"re-solve chain, rule {rule}: {kinds}")
    assert min(kinds.values()) >= 10, kinds
    return tuple(out)


def assert_row_matches_cold(r, k, p, stype, ref, what):
    """Row k of to_numpy()'s rows against cold_reference()'s tuple for the problem p (the new costs in it)."""
    st, total, exact = ref
    assert r["status"][k] == st, (what, k, r["status"][k], st)
    if st == O.OPTIMAL:
        assert r["total_cost"][k] == total, (what, k)
        if exact is None:
            assert validate_solution(p, r["flows"][k], r["potentials"][k], stype) == total, (what, k)
        else:                       # cold although Optimal: the oracle's own solve, bit for bit
            assert np.array_equal(r["flows"][k], exact[0]) and np.array_equal(r["potentials"][k], exact[1]) and r["pivots"][k] == exact[2], (what, k)
            assert np.array_equal(r["trace"][k][:exact[2]], exact[3]), (what, k)


def assert_matches_cold(r, t, stype, cost, refs, what):
    r = to_numpy(r)
    for k, (p, ref) in enumerate(zip(t.variants, refs)):
        assert_row_matches_cold(r, k, with_cost(p, cost[k]), stype, ref, what)


def check_resolve_chain(first, again, rule, **kw):
    """first(u, arrays, stype), again(u, arrays, stype) -> result.  Four re-solves, every variant meeting all four cost modes: the oracle's cold
    solve on status and cost, validate_solution on flows and potentials, BatchSolver.set_costs + rerun_on_host bit for bit."""
    for j, ((t, stype), steps) in enumerate(zip(resolve_family(), resolve_reference(rule))):
        a = t.arrays()
        u = uniform_of(t, rule, **kw)
        r = first(u, a, stype)
        b = batch_solver_of(t, rule, stype).run_on_host()
        assert_equals_answers(r, batch_answers(b, t.count), f"graph {j}, first solve")
        for step, (cost, refs) in enumerate(steps):
            r = again(u, dict(a, cost=cost), stype)
            what = f"graph {j}, step {step}"
            assert_matches_cold(r, t, stype, cost, refs, what)
            for k in range(t.count):
                b.set_costs(k, cost[k])
            b.rerun_on_host()
            assert_equals_answers(r, batch_answers(b, t.count), what + ", BatchSolver")
            cold = [k for k, (st, _, exact) in enumerate(refs) if exact is not None]
            # the "excess" kind goes cold: pivot for pivot the oracle's fresh solve (assert_matches_cold), never 0 pivots from a kept basis
            assert all(KINDS[k % 3] == "excess" for k in cold), cold


HOST = (lambda u, a, stype: u.run_on_host(supply_type=stype, **a), lambda u, a, stype, **kw: u.rerun_on_host(supply_type=stype, **a, **kw))


@pytest.mark.parametrize("rule", ALL_RULES)
def test_resolve_chain_on_the_host(rule):
    check_resolve_chain(*HOST, rule)


# ---- 11
def check_unchanged_costs(first, again, rule):
    for j, (t, stype) in enumerate(resolve_family()):
        a = t.arrays()
        u = uniform_of(t, rule)
        before = to_numpy(first(u, a, stype))
        after = to_numpy(again(u, a, stype))
        refs = [cold_reference(p, stype, rule) for p in t.variants]
        warm = np.array([st == O.OPTIMAL and exact is None for st, _, exact in refs])
        assert warm.sum() >= 2 and not warm.all()
        assert not after["pivots"][warm].any() and not after["trace"][warm].any()                   # nothing is eligible under the potentials of the same basis
        assert np.array_equal(after["pivots"][~warm], before["pivots"][~warm]) and np.array_equal(after["trace"][~warm], before["trace"][~warm])
        for name in ("status", "total_cost", "flows", "potentials"):
            assert np.array_equal(after[name], before[name]), (j, name)


@pytest.mark.parametrize("rule", ALL_RULES)
def test_unchanged_costs_need_no_pivot_on_the_host(rule):
    check_unchanged_costs(*HOST, rule)


# ---- 12
def check_changed_mask(first, again, rule, **kw):
    """Rows the mask leaves out keep their last outputs; the marked ones equal an unmasked re-solve's."""
    j = 1
    t, stype = resolve_family()[j]
    a = t.arrays()
    cost = step_costs(t, j, 1)
    mask = np.arange(t.count) % 3 != 1
    u = uniform_of(t, rule, **kw)
    before = to_numpy(first(u, a, stype))
    masked = to_numpy(again(u, dict(a, cost=cost), stype, changed=mask))
    v = uniform_of(t, rule, **kw)
    first(v, a, stype)
    whole = to_numpy(again(v, dict(a, cost=cost), stype))
    for name in before:
        assert np.array_equal(masked[name][~mask], before[name][~mask]), name
        assert np.array_equal(masked[name][mask], whole[name][mask]), name
    assert not np.array_equal(whole["total_cost"][~mask], before["total_cost"][~mask])
    # the left-out rows go on from their own last state: marked alone now, with their first costs again -> 0 pivots where warm
    back = to_numpy(again(u, a, stype, changed=~mask))
    assert np.array_equal(back["total_cost"][~mask], before["total_cost"][~mask]) and np.array_equal(back["total_cost"][mask], masked["total_cost"][mask])
    warm = np.array([st == O.OPTIMAL and exact is None for st, _, exact in (cold_reference(p, stype, rule) for p in t.variants)])
    assert (warm & ~mask).any() and not back["pivots"][warm & ~mask].any()
    assert u.stats()["total_pivots"] == back["pivots"][~mask].sum()


@pytest.mark.parametrize("rule", ALL_RULES)
def test_changed_mask_on_the_host(rule):
    check_changed_mask(*HOST, rule)


@pytest.mark.skipif(M.device_count() > 0, reason="a GPU is present")
def test_solve_without_a_device_leaves_the_handle_as_it_was():
    t, stype = resolve_family()[0]
    a = t.arrays()
    u = uniform_of(t, O.RULE_BLOCK)
    before = u.run_on_host(supply_type=stype, **a)
    stats = u.stats()
    cost = step_costs(t, 0, 0)
    for refused in (u.solve, u.resolve):
        with pytest.raises(M.McfError) as ei:
            refused(supply_type=stype, **dict(a, cost=cost))
        assert ei.value.code == L.ERR_NO_DEVICE
    assert u.stats() == stats
    v = uniform_of(t, O.RULE_BLOCK)
    assert_rows_equal(v.run_on_host(supply_type=stype, **a), before)
    assert_rows_equal(u.rerun_on_host(supply_type=stype, **dict(a, cost=cost)), v.rerun_on_host(supply_type=stype, **dict(a, cost=cost)))


# ---- 13: the pivot limit.  An instance that reaches it reports NotSolved with zero rows, `limit` pivots and `limit` trace entries
NOT_SOLVED = M.SolverStatus.NotSolved
LIMIT_RUNS = ((1, TRACE), (16, TRACE), (16, 16), (16, 17), (16, 8))      # (pivot_limit, record_trace): at 17 the entering arc of the refused pivot would lie inside the row
LONG_TRACE = 1 << 15     # for the oracle's solves with the re-solves' costs


class Rows:
    """to_numpy()'s dict with the attributes of a result, so that the checkers take it."""

    def __init__(self, rows):
        self.__dict__.update(rows)


def limited(answer, k):
    """answer_of()'s tuple under a pivot limit of k, derived from the unlimited answer: a solve of at most k pivots is not touched by the
    limit; a longer one stops behind its first k pivots and reports nothing else."""
    if answer[1] <= k:
        return answer
    return NOT_SOLVED, k, answer[2][:k], None, None, None


@functools.lru_cache(maxsize=None)
def limited_reference(name, rule, stype, k):
    """reference() under a pivot limit of k.  The floors are asserted here, on the oracle's answers alone: at least 10 instances are stopped,
    and at k = 16 at least 10 finish below the limit."""
    refs = reference(name, rule, stype)
    pivots = np.array([a[1] for row in refs for a in row])
    stopped, below, exact = int((pivots > k).sum()), int((pivots < k).sum()), int((pivots == k).sum())
    print(f"family {name}, rule {rule}, supply type {stype}, pivot limit {k}: stopped {stopped}, finished below the limit {below}, solves of exactly {k} pivots {exact}")
    assert stopped >= 10 and (k != 16 or below >= 10), (stopped, below)
    return tuple(tuple(limited(a, k) for a in row) for row in refs)


def test_some_solves_take_exactly_the_limit():
    """Such a solve meets the limit's test with pivots == limit and must end as if there were no limit: limited() leaves it as it is."""
    for k in sorted({k for k, _ in LIMIT_RUNS}):
        exact = {(name, rule, stype): sum(a[1] == k for row in reference(name, rule, stype) for a in row) for name in "AB" for rule in ALL_RULES for stype in SUPPLY_TYPES}
        print(f"solves of exactly {k} pivots by (family, rule, supply type): {exact}")
        assert sum(exact.values()) >= 1, k


def check_families_under_a_limit(run, name, rule, k, cap, **kw):
    """run(handle, arrays, stype) -> result.  Every row against the oracle's limited answer; the limit changes nothing of the statistics
    but the pivots."""
    for stype in SUPPLY_TYPES:
        for t, answers in zip(family(name), limited_reference(name, rule, stype, k)):
            u = uniform_of(t, rule, pivot_limit=k, record_trace=cap, **kw)
            r = run(u, t.arrays(), stype)
            assert to_numpy(r)["trace"].shape == (t.count, cap)
            assert_equals_answers(r, answers, (f"family {name}, n {t.n}, m {t.m}, supply type {stype}, limit {k}, trace capacity {cap}", kw), trace_cap=cap)
            st = u.stats()
            assert st["instances"] == t.count and st["total_pivots"] == sum(a[1] for a in answers) and st["workspace_bytes"] == t.count * stride_of(t), st
            yield t, stype, answers, u, r, st


@pytest.mark.parametrize("k, cap", LIMIT_RUNS)
@pytest.mark.parametrize("rule", ALL_RULES)
@pytest.mark.parametrize("name", ["A", "B"])
def test_families_under_a_pivot_limit_on_the_host(name, rule, k, cap):
    for t, stype, answers, u, r, st in check_families_under_a_limit(HOST[0], name, rule, k, cap):
        assert st["launches"] == st["bytes_up"] == st["bytes_down"] == st["lds_instances"] == st["global_instances"] == 0


# ---- 14: re-solves round the limit
RESOLVE_LIMIT = {O.RULE_BLOCK: 21, O.RULE_BEST: 11, O.RULE_FIRST: 23}     # per rule the smallest limit in 8..64 at which limited_chain_reference() meets every class
CLASSES = ("stopped -> stopped", "stopped -> finished", "Optimal -> warm and finished", "Optimal -> warm and stopped", "after warm and stopped -> finished",
           "after warm and stopped -> stopped")


def same_answer(a, b):
    return a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2]) and (a[0] != O.OPTIMAL or (a[3] == b[3] and np.array_equal(a[4], b[4]) and np.array_equal(a[5], b[5])))


def limited_chain(problems, stype, rule, k, costs):
    """The reference of a chain of re-solves under a pivot limit of k; costs[step][i] is the cost row of instance i.
    -> (first, steps, classes).  first: the limited oracle answers of the first solve.  steps: per step `expected` (an answer per instance),
    `warm` (re-solved from the kept basis: the last solve ended Optimal and conserves flow), `stopped`, and `cold` (cold_reference() of the
    new costs).  classes: how often each of CLASSES occurs.
    A row re-solved cold -- its last solve was stopped, Infeasible or left a surplus -- has the oracle's cold solve under the limit as its
    reference.  No oracle knows a warm pivot path: there the reference is BatchSolver (set_costs + rerun_on_host, the same limit), and
    wherever the oracle speaks BatchSolver is asserted to say the same."""
    n = len(problems)
    b = M.BatchSolver(rule=RULES[rule], pivot_limit=k, record_trace=TRACE)
    for p in problems:
        b.add(p, supply_type=stype)
    b.run_on_host()
    last = batch_answers(b, n)
    first = tuple(limited(answer_of(p, rule, stype), k) for p in problems)
    assert all(same_answer(x, y) for x, y in zip(last, first))
    conserves = [warm_after(cold_reference(p, stype, rule)) for p in problems]
    after_warm_and_stopped = np.zeros(n, bool)
    classes = np.zeros(len(CLASSES), np.int64)
    steps = []
    for cost in costs:
        for i in range(n):
            b.set_costs(i, cost[i])
        b.rerun_on_host()
        now = batch_answers(b, n)
        was_stopped = np.array([a[0] == NOT_SOLVED for a in last])
        warm = np.array([a[0] == O.OPTIMAL and c for a, c in zip(last, conserves)])
        stopped = np.array([a[0] == NOT_SOLVED for a in now])
        cold = tuple(cold_reference(with_cost(p, cost[i]), stype, rule) for i, p in enumerate(problems))
        expected = list(now)
        for i in np.flatnonzero(~warm):
            expected[i] = limited(answer_of(with_cost(problems[i], cost[i]), rule, stype, trace_cap=LONG_TRACE), k)
            assert same_answer(now[i], expected[i]), i
        assert all(a[1] <= k for a in now) and all(a[1] == k for a in now if a[0] == NOT_SOLVED)
        classes += [(was_stopped & stopped).sum(), (was_stopped & ~stopped).sum(), (warm & ~stopped).sum(), (warm & stopped).sum(),
                    (after_warm_and_stopped & ~stopped).sum(), (after_warm_and_stopped & stopped).sum()]
        steps.append(dict(expected=tuple(expected), warm=warm, stopped=stopped, cold=cold))
        after_warm_and_stopped = warm & stopped
        last, conserves = now, [warm_after(ref) for ref in cold]
    return first, tuple(steps), classes


def check_chain_under_a_limit(ref, problems, stype, k, costs, solve, resolve, fresh, rows_of, what):
    """solve() / resolve(step) / fresh() -> result: the handle's first solve, its re-solve with costs[step], and a fresh handle's first solve
    with the last costs.  rows_of(result): the rows per instance."""
    first, steps, _ = ref
    assert_equals_answers(rows_of(solve()), first, (what, "first solve"))
    for step, s in enumerate(steps):
        r = rows_of(resolve(step))
        assert_equals_answers(r, s["expected"], (what, "step", step))
        rows = to_numpy(r)
        for i in np.flatnonzero(s["warm"]):
            if s["stopped"][i]:                 # its workspace holds a half-repriced basis now: the next step starts it cold
                assert rows["status"][i] == NOT_SOLVED and rows["pivots"][i] == k, (what, step, i)
            else:
                assert rows["pivots"][i] <= k, (what, step, i)
                assert_row_matches_cold(rows, i, with_cost(problems[i], costs[step][i]), stype, s["cold"][i], (what, "step", step))
    # what the last step re-solved cold is what a fresh handle gives for the same costs
    again = to_numpy(rows_of(fresh()))
    cold = np.flatnonzero(~steps[-1]["warm"])
    assert len(cold)
    for name in rows:
        for i in cold:
            assert np.array_equal(rows[name][i], again[name][i]), (what, "fresh handle", name, i)


@functools.lru_cache(maxsize=None)
def limited_chain_reference(rule):
    """per graph of resolve_family(): (the cost rows of every step, limited_chain()).  Asserted on the references alone: over the graphs
    every class of CLASSES occurs."""
    k = RESOLVE_LIMIT[rule]
    out = []
    classes = np.zeros(len(CLASSES), np.int64)
    for j, (t, stype) in enumerate(resolve_family()):
        costs = tuple(step_costs(t, j, step) for step in range(STEPS))
        ref = limited_chain(t.variants, stype, rule, k, costs)
        classes += ref[2]
        out.append((costs, ref))
    print(f"re-solve chain under a pivot limit of {k}, rule {rule}: {dict(zip(CLASSES, classes.tolist()))}")
    assert classes.min() >= 1, classes
    return tuple(out)


def check_resolve_chain_under_a_limit(first, again, rule, **kw):
    k = RESOLVE_LIMIT[rule]
    for j, ((t, stype), (costs, ref)) in enumerate(zip(resolve_family(), limited_chain_reference(rule))):
        a = t.arrays()
        u = uniform_of(t, rule, pivot_limit=k, **kw)
        check_chain_under_a_limit(ref, t.variants, stype, k, costs, lambda: first(u, a, stype), lambda step: again(u, dict(a, cost=costs[step]), stype),
                                  lambda: first(uniform_of(t, rule, pivot_limit=k, **kw), dict(a, cost=costs[-1]), stype), lambda r: r, (f"graph {j}", kw))


@pytest.mark.parametrize("rule", ALL_RULES)
def test_resolve_chain_under_a_pivot_limit_on_the_host(rule):
    check_resolve_chain_under_a_limit(*HOST, rule)


def check_unchanged_costs_and_mask_under_a_limit(problems, stype, rule, k, make, first, again, cost, rows_of, what):
    """make() -> a fresh handle with the limit; first(handle), again(handle, cost, changed) -> result (cost None: the first costs again).
    -> (stopped, warm, mask) per instance, from the oracle, for the caller's floors."""
    n = len(problems)
    answers = [limited(answer_of(p, rule, stype), k) for p in problems]
    stopped = np.array([a[0] == NOT_SOLVED for a in answers])
    warm = np.array([a[0] == O.OPTIMAL and warm_after(cold_reference(p, stype, rule)) for a, p in zip(answers, problems)])
    fields = lambda r: to_numpy(rows_of(r))
    # unchanged costs: a stopped row starts cold and is stopped again behind the same pivots; nothing is eligible where the basis was kept
    h = make()
    before = fields(first(h))
    assert_equals_answers(Rows(before), answers, what)
    after = fields(again(h, None, None))
    for i in range(n):
        for name in before:
            if warm[i] and name in ("pivots", "trace"):
                assert not np.any(after[name][i]), (what, "unchanged costs", name, i)
            else:
                assert np.array_equal(after[name][i], before[name][i]), (what, "unchanged costs", name, i)
    assert np.all(after["pivots"][stopped] == k) and np.all(after["status"][stopped] == NOT_SOLVED)
    assert h.stats()["total_pivots"] == after["pivots"].sum()
    # the mask: rows it leaves out keep their last outputs and are not counted, the marked ones equal an unmasked re-solve's
    mask = np.arange(n) % 3 != 1
    h, v = make(), make()
    first(h)
    first(v)
    masked, whole = fields(again(h, cost, mask)), fields(again(v, cost, None))
    assert h.stats()["total_pivots"] == masked["pivots"][mask].sum()
    for i in range(n):
        for name in before:
            assert np.array_equal(masked[name][i], (whole if mask[i] else before)[name][i]), (what, "mask", name, i)
    # the left-out rows go on from their own last state, stopped ones included: marked alone now, with their first costs again
    back = fields(again(h, None, ~mask))
    assert h.stats()["total_pivots"] == back["pivots"][~mask].sum()
    for i in range(n):
        for name in before:
            assert np.array_equal(back[name][i], (masked if mask[i] else after)[name][i]), (what, "mask, the rest", name, i)
    return stopped, warm, mask


def assert_limit_floors(seen, what):
    """seen: check_unchanged_costs_and_mask_under_a_limit()'s returns.  Stopped rows lie on both sides of the mask, and a row is kept warm."""
    inside, outside, warm = (sum(int(f(*s).sum()) for s in seen) for f in (lambda st, w, m: st & m, lambda st, w, m: st & ~m, lambda st, w, m: w))
    print(f"{what}: stopped rows marked {inside}, stopped rows left out {outside}, rows kept warm {warm}")
    assert inside >= 1 and outside >= 1 and warm >= 1, (inside, outside, warm)


def check_unchanged_costs_and_mask_under_a_limit_uniform(first, again, rule, **kw):
    k = RESOLVE_LIMIT[rule]
    seen = []
    for j, (t, stype) in enumerate(resolve_family()):
        a = t.arrays()
        seen.append(check_unchanged_costs_and_mask_under_a_limit(
            t.variants, stype, rule, k, lambda: uniform_of(t, rule, pivot_limit=k, **kw), lambda u: first(u, a, stype),
            lambda u, cost, changed: again(u, a if cost is None else dict(a, cost=cost), stype, **({} if changed is None else dict(changed=changed))),
            step_costs(t, j, 1), lambda r: r, (f"graph {j}", kw)))
    assert_limit_floors(seen, f"uniform handles under a pivot limit of {k}, rule {rule}")


@pytest.mark.parametrize("rule", ALL_RULES)
def test_unchanged_costs_and_the_changed_mask_under_a_pivot_limit_on_the_host(rule):
    check_unchanged_costs_and_mask_under_a_limit_uniform(*HOST, rule)


# ---- 15: the validation of limit-stopped results
def rows_from_answers(answers, m, n):
    """The four rows a validation reads, as the answers say them: zeros where an instance is not Optimal."""
    zeros = lambda length: np.zeros(length, np.int64)
    return dict(status=np.array([a[0] for a in answers], np.int32), total_cost=np.array([a[3] or 0 for a in answers], np.int64),
                flows=np.stack([zeros(m) if a[4] is None else np.asarray(a[4], np.int64) for a in answers]),
                potentials=np.stack([zeros(n) if a[5] is None else np.asarray(a[5], np.int64) for a in answers]))


@functools.lru_cache(maxsize=None)
def limited_validation_cases(name, k=16):
    """per supply type, per graph of family(name): the Case of test_uniform_validate_host.py whose solution rows are the oracle's answers under
    a pivot limit of k (Block Search), its expected rows the oracle validator's.  Asserted on those alone: a stopped row has the status error
    and nothing else, objective and dual cost 0."""
    from test_uniform_validate_host import KINDS, Case, K
    out = []
    stopped = 0
    for stype in SUPPLY_TYPES:
        for t, answers in zip(family(name), limited_reference(name, O.RULE_BLOCK, stype, k)):
            c = Case(f"family {name}, n {t.n}, m {t.m}, supply type {stype}, pivot limit {k}", t.n, t.src, t.tgt, t.arrays(), rows_from_answers(answers, t.m, t.n), stype)
            bad = c.rows["status"] == NOT_SOLVED
            stopped += int(bad.sum())
            e = c.expected
            assert np.all(e["errors"][bad, K["status"]] == 1) and np.all(e["errors"][bad].sum(axis=1) == 1) and not e["valid"][bad].any()
            assert not e["objective"][bad].any() and not e["dual_cost"][bad].any() and e["errors"].shape[1] == len(KINDS)
            out.append(c)
    valid = sum(int(c.expected["valid"].sum()) for c in out)
    print(f"family {name} under a pivot limit of {k}: stopped rows {stopped}, valid rows {valid}")
    assert stopped >= 10 and valid >= 10, (stopped, valid)
    return tuple(out)


def check_validation_under_a_limit(first, validate, again, name, k=16):
    """first(u, arrays, stype), validate(u, result, arrays, stype), again(u, arrays, stype).  The result goes into the validation as it lies;
    the re-solve behind it equals one that no validation preceded.  Yields (case, validation)."""
    from test_uniform_validate_host import ROW_NAMES, assert_equals_oracle
    tops = family(name)
    for j, c in enumerate(limited_validation_cases(name, k)):
        t = tops[j % len(tops)]
        a = t.arrays()
        u, w = uniform_of(t, O.RULE_BLOCK, pivot_limit=k), uniform_of(t, O.RULE_BLOCK, pivot_limit=k)
        r = first(u, a, c.stype)
        rows = to_numpy(r)
        for field in ROW_NAMES:                         # the rows under validation are this handle's own
            assert np.array_equal(rows[field], c.rows[field]), (c.label, field)
        stats = u.stats()
        v = validate(u, r, a, c.stype)
        assert_equals_oracle(v, c)
        assert u.stats() == stats
        yield c, v
        HOST[0](w, a, c.stype)
        assert_rows_equal(again(u, a, c.stype), HOST[1](w, a, c.stype), (c.label, "the validation left the state alone"))


@pytest.mark.parametrize("name", ["A", "B"])
def test_validation_of_limit_stopped_results_on_the_host(name):
    for c, v in check_validation_under_a_limit(HOST[0], lambda u, r, a, stype: u.validate_on_host(r, supply_type=stype, **a), HOST[1], name):
        assert isinstance(v.valid, np.ndarray) and v.summary["bytes_up"] == v.summary["bytes_down"] == 0
