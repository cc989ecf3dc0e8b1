"""The uniform batch on the MI355X (mcf_ubatch_solve / _resolve, UniformBatch, DESIGN.md 3.14 "Uniform batch"): set-up, pivots and finish
on the device, torch tensors in and out.

Every comparison is exact: against the host hook's outputs bit for bit and against the oracle (families, references and checkers of
test_uniform_host.py)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import mincostflow_amd as M
from mincostflow_amd import _lib as L
from oracle import ns_oracle as O

from test_batch_host import LDS_LIMITS, PADDED_NODES, bound_infeasible
from test_uniform_host import (ALL_RULES, HOST, LIMIT_RUNS, NOT_SOLVED, PER, RESOLVE_LIMIT, STEPS, SUPPLY_TYPES, Topology, answer_of, assert_equals_answers, assert_rows_equal,
                               check_changed_mask, check_empty_batch, check_families_under_a_limit, check_nothing_runs, check_resolve_chain,
                               check_resolve_chain_under_a_limit, check_short_and_absent_traces, check_solve_twice, check_unchanged_costs,
                               check_unchanged_costs_and_mask_under_a_limit_uniform, check_validation_under_a_limit, family, limited, picked, reference, resolve_family,
                               step_costs, stride_of, to_numpy, uniform_of)

pytestmark = pytest.mark.gpu
SLOT_BYTES = 104 + C.sizeof(L.BlockConfig)           # BatchSlot of csrc/batch_layout.hip.h, which has no padding


def tensors(a):
    return {k: (torch.from_numpy(np.ascontiguousarray(v)).cuda() if isinstance(v, np.ndarray) else v) for k, v in a.items()}


DEVICE = (lambda u, a, stype: u.solve(supply_type=stype, **tensors(a)), lambda u, a, stype, **kw: u.resolve(supply_type=stype, **tensors(a), **tensors(kw)))
DEVICE_NUMPY = (lambda u, a, stype: u.solve(supply_type=stype, **a), lambda u, a, stype, **kw: u.resolve(supply_type=stype, **a, **kw))


@functools.lru_cache(maxsize=None)
def hook_results(name, rule, stype):
    return tuple(to_numpy(uniform_of(t, rule).run_on_host(supply_type=stype, **t.arrays())) for t in family(name))


class Rows:
    """to_numpy()'s dict with the attributes of a UniformResult, so that the checkers take it."""

    def __init__(self, rows):
        self.__dict__.update(rows)


# ---- 1
@pytest.mark.parametrize("rule", ALL_RULES)
@pytest.mark.parametrize("name", ["A", "B"])
def test_families_on_the_device(name, rule):
    """Torch in, whole and in slices of 3 pivots; numpy in (MCF_MEM_HOST) equals torch in.  Every graph of both families is an LDS-tier batch."""
    for stype in SUPPLY_TYPES:
        for t, answers, hook in zip(family(name), reference(name, rule, stype), hook_results(name, rule, stype)):
            what = f"family {name}, n {t.n}, m {t.m}, supply type {stype}"
            a = tensors(t.arrays())
            for kw in ({}, dict(pivots_per_launch=3)):
                u = uniform_of(t, rule, **kw)
                r = u.solve(supply_type=stype, **a)
                assert all(v.is_cuda for v in (r.status, r.pivots, r.total_cost, r.flows, r.potentials, r.trace))
                assert_rows_equal(r, Rows(hook), (what, kw))
                assert_equals_answers(r, answers, (what, kw))
                st = u.stats()
                assert st["instances"] == st["lds_instances"] == t.count and st["global_instances"] == 0, st
                assert st["workspace_bytes"] == t.count * stride_of(t) and st["total_pivots"] == sum(x[1] for x in answers)
                assert st["launches"] >= 1 and st["lds_bytes_max"] == stride_of(t), (st, stride_of(t))
                if kw:
                    assert st["launches"] >= -(-max(x[1] for x in answers) // 3)
            for kw in ({}, dict(pivots_per_launch=3)):
                r = uniform_of(t, rule, **kw).solve(supply_type=stype, **t.arrays())
                assert isinstance(r.flows, np.ndarray)
                assert_rows_equal(r, Rows(hook), (what, "numpy in", kw))


# ---- 2: the global tier
def padded(t, keep):
    variants = [O.Problem(PADDED_NODES, p.m, p.src, p.tgt, p.lower, p.upper, p.cost, np.concatenate([p.supply, np.zeros(PADDED_NODES - p.n, np.int64)]))
                for p in (t.variants[k] for k in keep)]
    return Topology(PADDED_NODES, t.src, t.tgt, variants, [t.zero_capacity[k] for k in keep])


@functools.lru_cache(maxsize=None)
def padded_family(rule):
    """((topology, supply type, answers) ...): the six largest family A variants per outcome (largest graph first; none infeasible by its
    bounds), grouped by their graph and padded with isolated zero-supply nodes to 4 500 nodes as padded_fuzz does: the stride fits no LDS
    limit.  Picked under GEQ and run under GEQ, the two largest graphs also under LEQ.  The root links of the added nodes join the search
    range, so the oracle answers the padded instances."""
    left = {O.OPTIMAL: 6, O.INFEASIBLE: 6, O.UNBOUNDED: 6}
    out = []
    for t, answers in reversed(list(zip(family("A"), reference("A", rule, O.GEQ)))):
        keep = []
        for k in reversed(range(t.count)):
            st = answers[k][0]
            if t.m + t.n > 64 and not bound_infeasible(t.variants[k]) and left.get(st, 0) > 0:
                left[st] -= 1
                keep.append(k)
        if keep:
            q = padded(t, sorted(keep))
            assert stride_of(q) > max(LDS_LIMITS)
            for stype in (O.GEQ, O.LEQ) if len(out) < 4 else (O.GEQ,):
                out.append((q, stype, tuple(answer_of(p, rule, stype, trace_cap=1 << 14) for p in q.variants)))
    assert not any(left.values()), left
    seen = {st: sum(a[0] == st for _, stype, answers in out for a in answers if stype == O.GEQ) for st in left}
    print(f"padded family, rule {rule}: {[(q.m, q.count, stype) for q, stype, _ in out]}, under GEQ {seen}")
    assert all(v >= 2 for v in seen.values()), seen
    assert any(stype == O.LEQ and any(a[1] > 0 for a in answers) for _, stype, answers in out)
    return tuple(out)


@pytest.mark.parametrize("rule", ALL_RULES)
def test_global_tier_whole_and_in_slices(rule):
    for q, stype, answers in padded_family(rule):
        hook = uniform_of(q, rule, record_trace=1 << 14).run_on_host(supply_type=stype, **q.arrays())
        assert_equals_answers(hook, answers, "hook", trace_cap=1 << 14)
        for kw in ({}, dict(pivots_per_launch=7)):
            u = uniform_of(q, rule, record_trace=1 << 14, **kw)
            r = u.solve(supply_type=stype, **tensors(q.arrays()))
            assert_rows_equal(r, hook, (kw, stype))
            st = u.stats()
            assert st["global_instances"] == q.count and st["lds_instances"] == 0 and st["lds_bytes_max"] == 0 and st["launches"] >= 1, st
            assert st["workspace_bytes"] == q.count * stride_of(q)


# ---- 3: re-solve
@functools.lru_cache(maxsize=None)
def hook_chain(rule):
    """per graph of resolve_family(): the hook's rows after the first solve and after each of the four re-solves"""
    out = []
    for j, (t, stype) in enumerate(resolve_family()):
        a = t.arrays()
        u = uniform_of(t, rule)
        rows = [to_numpy(HOST[0](u, a, stype))]
        for step in range(STEPS):
            rows.append(to_numpy(HOST[1](u, dict(a, cost=step_costs(t, j, step)), stype)))
        out.append(tuple(rows))
    return tuple(out)


@pytest.mark.parametrize("rule", ALL_RULES)
def test_resolve_chain_on_the_device(rule):
    check_resolve_chain(*DEVICE, rule)


@pytest.mark.parametrize("slices", [1, 3])
@pytest.mark.parametrize("rule", ALL_RULES)
def test_resolve_chain_and_mask_in_slices_equal_the_hook(rule, slices):
    for j, ((t, stype), rows) in enumerate(zip(resolve_family(), hook_chain(rule))):
        a = t.arrays()
        u = uniform_of(t, rule, pivots_per_launch=slices)
        assert_rows_equal(DEVICE[0](u, a, stype), Rows(rows[0]), (j, "first solve"))
        for step in range(STEPS):
            assert_rows_equal(DEVICE[1](u, dict(a, cost=step_costs(t, j, step)), stype), Rows(rows[step + 1]), (j, step))
    check_changed_mask(*DEVICE, rule, pivots_per_launch=slices)


@pytest.mark.parametrize("rule", ALL_RULES)
def test_unchanged_costs_need_no_pivot_on_the_device(rule):
    check_unchanged_costs(*DEVICE, rule)


@pytest.mark.parametrize("rule", ALL_RULES)
def test_the_device_equals_the_hook_in_any_order(rule):
    """solve -> resolve, hook solve -> resolve, solve -> hook re-solve -> resolve: the state moves between host and device with the calls."""
    orders = ((DEVICE[0], DEVICE[1], DEVICE[1]), (HOST[0], DEVICE[1], DEVICE[1]), (DEVICE[0], HOST[1], DEVICE[1]), (DEVICE_NUMPY[0], DEVICE[1], HOST[1]))
    for j, ((t, stype), rows) in enumerate(zip(resolve_family(), hook_chain(rule))):
        a = t.arrays()
        for order in orders:
            u = uniform_of(t, rule)
            assert_rows_equal(order[0](u, a, stype), Rows(rows[0]), j)
            assert_rows_equal(order[1](u, dict(a, cost=step_costs(t, j, 0)), stype), Rows(rows[1]), j)
            assert_rows_equal(order[2](u, dict(a, cost=step_costs(t, j, 1)), stype), Rows(rows[2]), j)


# ---- 4: the edges of test_uniform_host.py on the device
def test_an_empty_batch_on_the_device():
    check_empty_batch(lambda u, cost, supply: u.solve(torch.from_numpy(cost).cuda(), torch.from_numpy(supply).cuda()))
    check_empty_batch(lambda u, cost, supply: u.solve(cost, supply))


def test_a_batch_infeasible_by_its_bounds_on_the_device():
    check_nothing_runs(lambda u, a: u.solve(**tensors(a)))
    check_nothing_runs(lambda u, a: u.solve(**a))


def test_short_and_absent_traces_on_the_device():
    check_short_and_absent_traces(lambda u, a: u.solve(**tensors(a)))


def test_solve_twice_on_the_device():
    check_solve_twice(lambda u, a, stype: u.solve(supply_type=stype, **tensors(a)))


# ---- 5
def test_device_in_moves_slots_and_ids_only():
    """30 instances from tensors: up go the slot template and the ids of the one round of launches, down come the slots after the set-up and
    after the round; nothing of it changes when the graph has twice the arcs."""
    t = picked("A", 6)
    keep = [k for k in range(PER) if not bound_infeasible(t.variants[k])] + [0, 1, 2, 3, 4, 5, 6]
    assert len(keep) == 30
    q = t.subset(keep)
    src2, tgt2 = np.concatenate([q.src, q.src]), np.concatenate([q.tgt, q.tgt])
    double = Topology(q.n, src2, tgt2, [O.Problem(p.n, 2 * p.m, src2, tgt2, np.tile(p.lower, 2), np.tile(p.upper, 2), np.tile(p.cost, 2), p.supply) for p in q.variants],
                      q.zero_capacity)
    seen = []
    for g in (q, double):
        u = uniform_of(g, O.RULE_BLOCK)
        r = u.solve(**tensors(g.arrays()))
        st = u.stats()
        assert st["launches"] == 1 and int(r.pivots.max()) > 0, st
        assert st["bytes_up"] == SLOT_BYTES + 4 * 30, st
        assert st["bytes_down"] == 2 * 30 * SLOT_BYTES, st
        seen.append((st["bytes_up"], st["bytes_down"]))
        # numpy in: the arrays as well, one copy each
        v = uniform_of(g, O.RULE_BLOCK)
        v.solve(**g.arrays())
        sv = v.stats()
        assert sv["bytes_up"] == st["bytes_up"] + 8 * 30 * (3 * g.m + g.n), sv
        assert sv["bytes_down"] == st["bytes_down"] + 30 * (4 + 8 + 8 + 8 * g.m + 8 * g.n + 4 * u.record_trace), sv
    assert seen[0] == seen[1]


# ---- 6
def test_bad_tensors_are_refused_before_anything_is_launched():
    t = picked()
    a = t.arrays()
    good = tensors(a)
    u = uniform_of(t, O.RULE_BLOCK)
    wide = torch.zeros((t.m, t.count), dtype=torch.int64, device="cuda")
    bad = (dict(good, cost=torch.from_numpy(a["cost"])),                           # on the CPU
           dict(good, supply=good["supply"].to(torch.int32)),                      # dtype
           dict(good, cost=wide.t()),                                              # not contiguous in the last dimension
           dict(good, upper=good["upper"].to(torch.float64)),
           dict(good, lower=a["lower"]),                                           # a mix
           dict(a, cost=good["cost"]),
           dict(good, cost=good["cost"][:, :-1]))                                  # shape
    if torch.cuda.device_count() > 1:
        bad += (dict(good, cost=good["cost"].to("cuda:1")),)
    for kw in bad:
        with pytest.raises(ValueError):
            u.solve(**kw)
        with pytest.raises(ValueError):
            u.resolve(**kw)
    with pytest.raises(ValueError):
        u.run_on_host(**good)
    st = u.stats()
    assert st["instances"] == 0 and st["launches"] == 0 and st["bytes_up"] == 0
    with pytest.raises(M.McfError) as ei:
        u.resolve(**good)                                                          # and still unsolved
    assert ei.value.code == L.ERR_STATE
    # a view with a row stride above m is fine: the strides come from the tensor
    padded_cost = torch.zeros((t.count, t.m + 3), dtype=torch.int64, device="cuda")
    padded_cost[:, :t.m] = good["cost"]
    assert_rows_equal(u.solve(**dict(good, cost=padded_cost[:, :t.m])), uniform_of(t, O.RULE_BLOCK).run_on_host(**a))
    # one row for all, as a 1-D tensor and as an expanded one (stride 0)
    shared = uniform_of(t, O.RULE_BLOCK).run_on_host(**dict(a, cost=a["cost"][2]))
    assert_rows_equal(u.solve(**dict(good, cost=good["cost"][2])), shared)
    assert_rows_equal(u.solve(**dict(good, cost=good["cost"][2].expand(t.count, t.m))), shared)


# ---- 7: the pivot limit.  On the device the search that meets the limit may be the first thing of a launch of its own, on a slot read
# back with pivots == limit, and the entering arc it found lies in the device's trace buffer behind the `limit` kept ones
LAUNCH_BUDGETS = {1: (0, 1), 16: (0, 1, 4, 16, 17)}      # pivots_per_launch per limit: the default, 1, a divisor of the limit, the limit, one more


@functools.lru_cache(maxsize=None)
def limited_hook_results(name, rule, stype, k, cap):
    return tuple(to_numpy(uniform_of(t, rule, pivot_limit=k, record_trace=cap).run_on_host(supply_type=stype, **t.arrays())) for t in family(name))


@pytest.mark.parametrize("k, cap", LIMIT_RUNS)
@pytest.mark.parametrize("rule", ALL_RULES)
@pytest.mark.parametrize("name", ["A", "B"])
def test_families_under_a_pivot_limit_on_the_device(name, rule, k, cap):
    tops = family(name)
    for budget in LAUNCH_BUDGETS[k]:
        for t, stype, answers, u, r, st in check_families_under_a_limit(DEVICE[0], name, rule, k, cap, pivots_per_launch=budget):
            what = (name, t.n, t.m, stype, k, cap, budget)
            hook = Rows(limited_hook_results(name, rule, stype, k, cap)[tops.index(t)])
            assert all(v.is_cuda for v in (r.status, r.pivots, r.total_cost, r.flows, r.potentials, r.trace))
            assert_rows_equal(r, hook, what)
            assert st["lds_instances"] == t.count and st["global_instances"] == 0 and st["lds_bytes_max"] == (stride_of(t) if st["launches"] else 0), st
            if budget == k and any(a[0] == NOT_SOLVED for a in answers):
                assert st["launches"] >= 2, st          # the refused search is a launch of its own
            if budget in (0, k):
                numpy_in = DEVICE_NUMPY[0](uniform_of(t, rule, pivot_limit=k, record_trace=cap, pivots_per_launch=budget), t.arrays(), stype)
                assert isinstance(numpy_in.flows, np.ndarray) and isinstance(numpy_in.trace, np.ndarray)
                assert_rows_equal(numpy_in, hook, (what, "numpy in"))


def test_global_tier_under_a_pivot_limit():
    rule, k, cap = O.RULE_BLOCK, 16, 32
    stopped = finished = 0
    for q, stype, answers in padded_family(rule):
        want = tuple(limited(a, k) for a in answers)
        stopped += sum(a[0] == NOT_SOLVED for a in want)
        finished += sum(a[0] != NOT_SOLVED and a[1] > 0 for a in want)
        hook = uniform_of(q, rule, pivot_limit=k, record_trace=cap).run_on_host(supply_type=stype, **q.arrays())
        assert_equals_answers(hook, want, "hook", trace_cap=cap)
        for budget in LAUNCH_BUDGETS[k]:
            u = uniform_of(q, rule, pivot_limit=k, record_trace=cap, pivots_per_launch=budget)
            r = u.solve(supply_type=stype, **tensors(q.arrays()))
            assert_rows_equal(r, hook, (budget, stype))
            st = u.stats()
            assert st["global_instances"] == q.count and st["lds_instances"] == 0 and st["lds_bytes_max"] == 0, st
            assert st["workspace_bytes"] == q.count * stride_of(q) and st["total_pivots"] == sum(a[1] for a in want)
            assert budget != k or not any(a[0] == NOT_SOLVED for a in want) or st["launches"] >= 2, st
    print(f"padded family under a pivot limit of {k}: stopped {stopped}, finished after pivots {finished}")
    assert stopped >= 2 and finished >= 2, (stopped, finished)


@pytest.mark.parametrize("rule", ALL_RULES)
def test_resolve_chain_under_a_pivot_limit_on_the_device(rule):
    check_resolve_chain_under_a_limit(*DEVICE, rule)


@functools.lru_cache(maxsize=None)
def limited_hook_chain(rule):
    """hook_chain() under the rule's limit of RESOLVE_LIMIT"""
    out = []
    for j, (t, stype) in enumerate(resolve_family()):
        a = t.arrays()
        u = uniform_of(t, rule, pivot_limit=RESOLVE_LIMIT[rule])
        rows = [to_numpy(HOST[0](u, a, stype))]
        for step in range(STEPS):
            rows.append(to_numpy(HOST[1](u, dict(a, cost=step_costs(t, j, step)), stype)))
        out.append(tuple(rows))
    return tuple(out)


@pytest.mark.parametrize("slices", [0, 3])
@pytest.mark.parametrize("rule", ALL_RULES)
def test_resolve_chain_and_mask_under_a_pivot_limit_equal_the_hook(rule, slices):
    for j, ((t, stype), rows) in enumerate(zip(resolve_family(), limited_hook_chain(rule))):
        a = t.arrays()
        u = uniform_of(t, rule, pivot_limit=RESOLVE_LIMIT[rule], pivots_per_launch=slices)
        assert_rows_equal(DEVICE[0](u, a, stype), Rows(rows[0]), (j, "first solve"))
        for step in range(STEPS):
            assert_rows_equal(DEVICE[1](u, dict(a, cost=step_costs(t, j, step)), stype), Rows(rows[step + 1]), (j, step))
    check_unchanged_costs_and_mask_under_a_limit_uniform(*DEVICE, rule, pivots_per_launch=slices)


@pytest.mark.parametrize("rule", ALL_RULES)
def test_the_device_equals_the_hook_in_any_order_under_a_pivot_limit(rule):
    """The orders of test_the_device_equals_the_hook_in_any_order: slab and slots of limit-stopped instances move whole between host and device."""
    orders = ((DEVICE[0], DEVICE[1], DEVICE[1]), (HOST[0], DEVICE[1], DEVICE[1]), (DEVICE[0], HOST[1], DEVICE[1]), (DEVICE_NUMPY[0], DEVICE[1], HOST[1]))
    for j, ((t, stype), rows) in enumerate(zip(resolve_family(), limited_hook_chain(rule))):
        a = t.arrays()
        assert (rows[0]["status"] == NOT_SOLVED).any() and (rows[1]["status"] == NOT_SOLVED).any()
        for order in orders:
            u = uniform_of(t, rule, pivot_limit=RESOLVE_LIMIT[rule])
            assert_rows_equal(order[0](u, a, stype), Rows(rows[0]), j)
            assert_rows_equal(order[1](u, dict(a, cost=step_costs(t, j, 0)), stype), Rows(rows[1]), j)
            assert_rows_equal(order[2](u, dict(a, cost=step_costs(t, j, 1)), stype), Rows(rows[2]), j)


@pytest.mark.parametrize("name", ["A", "B"])
def test_validation_of_limit_stopped_results_as_they_lie(name):
    """solve()'s tensors under a limit go into validate() as they are: 16 bytes up (the two summary words) and 16 down."""
    def validate(u, r, a, stype):
        assert r.status.is_cuda and r.flows.is_cuda
        return u.validate(r, supply_type=stype, **tensors(a))
    for c, v in check_validation_under_a_limit(DEVICE[0], validate, DEVICE[1], name):
        assert v.valid.is_cuda and v.errors.is_cuda and v.summary["bytes_up"] == 16 and v.summary["bytes_down"] == 16, v.summary
