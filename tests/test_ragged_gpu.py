"""The ragged batch on the MI355X (mcf_rbatch_solve / _resolve / _validate, RaggedBatch, DESIGN.md 3.14 "Ragged batch"): set-up, pivots,
finish and validation on the device, every block finding its instance's graph, rows and workspace in the handle's tables; flat torch
tensors in and out.

Every comparison is exact: against the host hook's rows bit for bit, and against the oracle, BatchSolver and UniformBatch as
test_ragged_host.py does (its mixes and checkers are imported)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import mincostflow_amd as M
from mincostflow_amd import _lib as L
from oracle import ns_oracle as O

from test_batch_host import LDS_LIMITS, bound_infeasible
from test_ragged_host import (HOST, MIX_RESOLVE_LIMIT, Mix, assert_equals_oracle, check_absent_arrays, check_an_unused_graph, check_empty_handles, check_families,
                              check_families_under_a_limit, check_graph_of, check_nothing_runs, check_null_outputs, check_one_graph, check_resolve_chain,
                              check_resolve_chain_under_a_limit, check_short_and_absent_traces, check_siblings, check_solve_twice, check_unchanged_costs_and_mask,
                              check_unchanged_costs_and_mask_under_a_limit_mix, check_validation_under_a_limit, corrupted_mix_cases, family_mix, footprints, mix_costs,
                              resolve_mix, small_mix, solved_mix_cases, validate_on_host)
from test_uniform_gpu import LAUNCH_BUDGETS, padded
from test_uniform_host import (ALL_RULES, LIMIT_RUNS, NOT_SOLVED, STEPS, SUPPLY_TYPES, Rows, Topology, answer_of, assert_equals_answers, assert_rows_equal, family, limited, stride_of,
                               to_numpy)
from test_uniform_validate_host import OUT_NAMES, assert_same_rows

pytestmark = pytest.mark.gpu
SLOT_BYTES = 104 + C.sizeof(L.BlockConfig)           # BatchSlot of csrc/batch_layout.hip.h, which has no padding


def tensors(a):
    return {k: (torch.from_numpy(np.ascontiguousarray(v)).cuda() if isinstance(v, np.ndarray) else v) for k, v in a.items()}


DEVICE = (lambda h, a, stype: h.solve(supply_type=stype, **tensors(a)), lambda h, a, stype, **kw: h.resolve(supply_type=stype, **tensors(a), **tensors(kw)))
DEVICE_NUMPY = (lambda h, a, stype: h.solve(supply_type=stype, **a), lambda h, a, stype, **kw: h.resolve(supply_type=stype, **a, **kw))


# ---- 1
@pytest.mark.parametrize("rule", ALL_RULES)
@pytest.mark.parametrize("name", ["A", "B"])
def test_families_in_one_handle_on_the_device(name, rule):
    """Torch in: the oracle, BatchSolver, and the hook bit for bit; every graph of both families is in the LDS tier, in several classes."""
    mix = family_mix(name)
    for stype, h, r, st in check_families(DEVICE[0], name, rule):
        assert all(v.is_cuda for v in (r.status, r.pivots, r.total_cost, r.flows, r.potentials, r.trace))
        assert_rows_equal(r, HOST[0](mix.handle(rule), mix.arrays(), stype), (name, stype, "against the hook"))
        assert st["lds_instances"] == mix.count and st["global_instances"] == 0 and st["launches"] >= 2, st
        assert st["lds_bytes_max"] == max(stride_of(t) for t in mix.tops), st


@pytest.mark.parametrize("name", ["A", "B"])
def test_numpy_in_equals_torch_in_whole_and_in_slices(name):
    mix = family_mix(name)
    a = mix.arrays()
    want = DEVICE[0](mix.handle(), a, O.LEQ)
    for kw in ({}, dict(pivots_per_launch=5)):
        h = mix.handle(**kw)
        r = DEVICE_NUMPY[0](h, a, O.LEQ)
        assert isinstance(r.flows, np.ndarray) and isinstance(r.trace, np.ndarray)
        assert_rows_equal(r, want, kw)
        assert_rows_equal(DEVICE[0](mix.handle(**kw), a, O.LEQ), want, kw)
        if kw:
            assert h.stats()["launches"] >= -(-int(to_numpy(want)["pivots"].max()) // 5)


# ---- 2, 3
def test_one_graph_equals_the_uniform_batch_on_the_device():
    check_one_graph(DEVICE[0], lambda u, a, stype: u.solve(supply_type=stype, **tensors(a)))


def test_graph_of_on_the_device():
    check_graph_of(DEVICE[0])


def test_graphs_of_equal_size_on_the_device():
    check_siblings(DEVICE[0], lambda h, rows, a: h.validate(tensors(rows), **tensors(a)), 0)


def test_graphs_of_equal_node_count_on_the_device():
    check_siblings(DEVICE[0], lambda h, rows, a: h.validate(tensors(rows), **tensors(a)), 1)


# ---- mixed tiers: the case the per-instance footprint exists for
MIXED_PER = 6
MIXED_TRACE = 1 << 14


@functools.lru_cache(maxsize=None)
def mixed_tiers():
    """family A's two largest graphs padded with plain nodes to 4 500 nodes (their workspace fits no LDS limit), interleaved with its three
    smallest, which stay in LDS; six variants of each."""
    keep = list(range(MIXED_PER))
    tops = [padded(family("A")[7], keep), family("A")[0].subset(keep), padded(family("A")[6], keep), family("A")[1].subset(keep), family("A")[2].subset(keep)]
    assert all(not bound_infeasible(p) for t in tops for p in t.variants)
    assert all((stride_of(t) > max(LDS_LIMITS)) == (g in (0, 2)) for g, t in enumerate(tops))
    return Mix(tops)


@functools.lru_cache(maxsize=None)
def mixed_answers(stype):
    return tuple(answer_of(p, O.RULE_BLOCK, stype, trace_cap=MIXED_TRACE) for p in mixed_tiers().problems())


def test_lds_and_global_tier_in_one_handle():
    mix = mixed_tiers()
    a = mix.arrays()
    for stype in (O.GEQ, O.LEQ):
        answers = mixed_answers(stype)
        assert any(x[1] > 0 for x, (g, _) in zip(answers, mix.order) if g in (0, 2)) and any(x[1] > 0 for x, (g, _) in zip(answers, mix.order) if g not in (0, 2))
        hook = HOST[0](mix.handle(record_trace=MIXED_TRACE), a, stype)
        assert_equals_answers(mix.split(hook), answers, "hook", trace_cap=MIXED_TRACE)
        for kw in ({}, dict(pivots_per_launch=11)):
            h = mix.handle(record_trace=MIXED_TRACE, **kw)
            r = DEVICE[0](h, a, stype)
            assert_rows_equal(r, hook, (stype, kw))
            st = h.stats()
            assert st["lds_instances"] == 3 * MIXED_PER and st["global_instances"] == 2 * MIXED_PER, st
            assert st["workspace_bytes"] == footprints(mix) and 0 < st["lds_bytes_max"] == max(stride_of(mix.tops[g]) for g in (1, 3, 4)), st
    # and a re-solve across both tiers
    cost = np.ascontiguousarray(np.abs(a["cost"][::-1]) // 2)      # no negative cost: nothing depends on a pivot limit
    h, v = mix.handle(record_trace=MIXED_TRACE), mix.handle(record_trace=MIXED_TRACE)
    DEVICE[0](h, a, O.GEQ)
    HOST[0](v, a, O.GEQ)
    assert_rows_equal(DEVICE[1](h, dict(a, cost=cost), O.GEQ), HOST[1](v, dict(a, cost=cost), O.GEQ), "re-solve")


# ---- 4: re-solve
@pytest.mark.parametrize("rule", ALL_RULES)
def test_resolve_chain_on_the_device(rule):
    check_resolve_chain(*DEVICE, rule)


@pytest.mark.parametrize("rule", ALL_RULES)
def test_unchanged_costs_and_the_changed_mask_on_the_device(rule):
    check_unchanged_costs_and_mask(*DEVICE, rule)
    check_unchanged_costs_and_mask(*DEVICE, rule, pivots_per_launch=3)


def test_the_device_equals_the_hook_in_any_order():
    """solve -> resolve, hook solve -> resolve, solve -> hook re-solve -> resolve, numpy solve -> resolve -> hook re-solve: the state moves
    whole between host and device with the calls."""
    mix = resolve_mix()
    a = mix.arrays()
    costs = [dict(a, cost=mix_costs(mix, step)) for step in range(2)]
    for stype in (O.GEQ, O.LEQ):
        u = mix.handle()
        rows = [HOST[0](u, a, stype), HOST[1](u, costs[0], stype), HOST[1](u, costs[1], stype)]
        for order in ((DEVICE[0], DEVICE[1], DEVICE[1]), (HOST[0], DEVICE[1], DEVICE[1]), (DEVICE[0], HOST[1], DEVICE[1]), (DEVICE_NUMPY[0], DEVICE[1], HOST[1])):
            h = mix.handle()
            assert_rows_equal(order[0](h, a, stype), rows[0], stype)
            assert_rows_equal(order[1](h, costs[0], stype), rows[1], stype)
            assert_rows_equal(order[2](h, costs[1], stype), rows[2], stype)


# ---- 5: validation
def check_validation_on_device(c):
    v = c.handle().validate(tensors(c.rows), supply_type=c.stype, **tensors(c.arrays))
    assert all(getattr(v, name).is_cuda for name in OUT_NAMES), c.label
    assert_equals_oracle(v, c, "tensors in")
    assert_same_rows(v, validate_on_host(c), (c.label, "against the hook"))
    assert v.summary["bytes_up"] == 16 and v.summary["bytes_down"] == 16, v.summary
    w = c.handle().validate(c.rows, supply_type=c.stype, **c.arrays)
    assert all(isinstance(getattr(w, name), np.ndarray) for name in OUT_NAMES), c.label
    assert_equals_oracle(w, c, "numpy in")


def test_solved_families_and_corruptions_validate_on_the_device():
    for c in solved_mix_cases("A") + solved_mix_cases("B") + corrupted_mix_cases():
        check_validation_on_device(c)


def test_validation_of_the_tensors_of_solve_as_they_lie():
    """solve()'s result goes into validate() as it is: 16 bytes up (the two summary words) and 16 down, whatever the handle holds."""
    mix = family_mix("B")
    a = tensors(mix.arrays())
    c = solved_mix_cases("B")[0]
    h = mix.handle()
    r = h.solve(supply_type=c.stype, **a)
    stats = h.stats()
    v = h.validate(r, supply_type=c.stype, **a)
    assert_equals_oracle(v, c)
    assert v.summary["bytes_up"] == 16 and v.summary["bytes_down"] == 16 and h.stats() == stats
    assert_rows_equal(h.resolve(supply_type=c.stype, **a), HOST[1](_solved_on_host(mix, c.stype), mix.arrays(), c.stype), "the validation left the state alone")


def _solved_on_host(mix, stype):
    h = mix.handle()
    HOST[0](h, mix.arrays(), stype)
    return h


# ---- 6: the edges of test_ragged_host.py on the device
def test_empty_handles_on_the_device():
    check_empty_handles(lambda h, cost, supply: h.solve(torch.from_numpy(cost).cuda(), torch.from_numpy(supply).cuda()))
    check_empty_handles(lambda h, cost, supply: h.solve(cost, supply))
    h = M.RaggedBatch([], None)
    empty = lambda dtype: torch.zeros(0, dtype=dtype, device="cuda")
    v = h.validate((empty(torch.int32), empty(torch.int64), empty(torch.int64), empty(torch.int64)), empty(torch.int64), empty(torch.int64))
    assert (v.summary["instances"], v.summary["invalid"], v.summary["first_invalid"]) == (0, 0, -1)


def test_a_graph_no_instance_uses_on_the_device():
    check_an_unused_graph(DEVICE[0])


def test_a_handle_infeasible_by_its_bounds_on_the_device():
    check_nothing_runs(lambda h, a: h.solve(**tensors(a)))
    check_nothing_runs(lambda h, a: h.solve(**a))


def test_absent_arrays_on_the_device():
    check_absent_arrays(lambda h, a: h.solve(**tensors(a)))


def test_null_output_pointers_on_the_device():
    check_null_outputs(L.lib().mcf_rbatch_solve)         # MCF_MEM_HOST: staged


def test_short_and_absent_traces_on_the_device():
    check_short_and_absent_traces(lambda h, a: h.solve(**tensors(a)))


def test_solve_twice_on_the_device():
    check_solve_twice(lambda h, a, stype: h.solve(supply_type=stype, **tensors(a)))


# ---- what moves
def test_device_in_moves_templates_slots_and_ids_only():
    """30 instances over 3 graphs from tensors: up go the three slot templates and the ids of the one round of launches, down come the slots
    after the set-up and after the round; nothing of it changes when every graph has twice the arcs."""
    keep = list(range(10))
    tops = [family("A")[k].subset(keep) for k in (4, 5, 6)]
    assert not any(bound_infeasible(p) for t in tops for p in t.variants)

    def doubled(q):
        src2, tgt2 = np.concatenate([q.src, q.src]), np.concatenate([q.tgt, q.tgt])
        return Topology(q.n, src2, tgt2, [O.Problem(p.n, 2 * p.m, src2, tgt2, np.tile(p.lower, 2), np.tile(p.upper, 2), np.tile(p.cost, 2), p.supply) for p in q.variants],
                        q.zero_capacity)
    seen = []
    for mix in (Mix(tops), Mix([doubled(t) for t in tops])):
        assert mix.count == 30
        a = mix.arrays()
        h = mix.handle()
        r = h.solve(**tensors(a))
        st = h.stats()
        assert 1 <= st["launches"] <= 3 and int(r.pivots.max()) > 0, st                 # one round: a launch per class of footprint
        assert st["bytes_up"] == 3 * SLOT_BYTES + 4 * 30, st
        assert st["bytes_down"] == 2 * 30 * SLOT_BYTES, st
        seen.append((st["bytes_up"], st["bytes_down"]))
        # numpy in: the arrays as well, one copy each
        v = mix.handle()
        v.solve(**a)
        sv = v.stats()
        arcs, nodes = int(mix.arc_rows[-1]), int(mix.node_rows[-1])
        assert sv["bytes_up"] == st["bytes_up"] + 8 * (3 * arcs + nodes), sv
        assert sv["bytes_down"] == st["bytes_down"] + 30 * (4 + 8 + 8 + 4 * h.record_trace) + 8 * arcs + 8 * nodes, sv
    assert seen[0] == seen[1]


def test_bad_tensors_are_refused_before_anything_is_launched():
    mix = small_mix()
    a = mix.arrays()
    good = tensors(a)
    h = mix.handle()
    bad = (dict(good, cost=torch.from_numpy(a["cost"])),                           # on the CPU
           dict(good, supply=good["supply"].to(torch.int32)),                      # dtype
           dict(good, upper=good["upper"].to(torch.float64)),
           dict(good, cost=torch.cat([good["cost"], good["cost"]])[::2]),          # not contiguous
           dict(good, lower=a["lower"]),                                           # a mix
           dict(a, cost=good["cost"]),
           dict(good, cost=good["cost"][:-1]),                                     # length
           dict(good, supply=good["supply"].reshape(1, -1)))                       # not flat
    if torch.cuda.device_count() > 1:
        bad += (dict(good, cost=good["cost"].to("cuda:1")),)
    for kw in bad:
        with pytest.raises(ValueError):
            h.solve(**kw)
        with pytest.raises(ValueError):
            h.resolve(**kw)
    with pytest.raises(ValueError):
        h.run_on_host(**good)
    with pytest.raises(ValueError):
        h.resolve(changed=torch.ones(mix.count + 1, dtype=torch.bool, device="cuda"), **good)
    st = h.stats()
    assert st["instances"] == 0 and st["launches"] == 0 and st["bytes_up"] == 0
    with pytest.raises(M.McfError) as ei:
        h.resolve(**good)                                                          # and still unsolved
    assert ei.value.code == L.ERR_STATE
    r = h.solve(**good)
    assert_rows_equal(r, HOST[0](mix.handle(), a, O.GEQ))
    rows = (r.status, r.total_cost, r.flows, r.potentials)
    for wrong in ((r.status.to(torch.int64),) + rows[1:], rows[:2] + (r.flows[:-1],) + rows[3:], rows[:3] + (r.potentials.cpu(),), rows[:3]):
        with pytest.raises(ValueError):
            h.validate(wrong, **good)


# ---- 7: the pivot limit (references, floors and checkers of test_uniform_host.py and test_ragged_host.py)
@functools.lru_cache(maxsize=None)
def limited_hook_rows(name, rule, stype, k, cap):
    mix = family_mix(name)
    return to_numpy(HOST[0](mix.handle(rule, pivot_limit=k, record_trace=cap), mix.arrays(), stype))


@pytest.mark.parametrize("k, cap", LIMIT_RUNS)
@pytest.mark.parametrize("rule", ALL_RULES)
@pytest.mark.parametrize("name", ["A", "B"])
def test_families_under_a_pivot_limit_on_the_device(name, rule, k, cap):
    mix = family_mix(name)
    for budget in LAUNCH_BUDGETS[k]:
        for stype, answers, h, r, st in check_families_under_a_limit(DEVICE[0], name, rule, k, cap, pivots_per_launch=budget):
            what = (name, stype, k, cap, budget)
            hook = Rows(limited_hook_rows(name, rule, stype, k, cap))
            assert all(v.is_cuda for v in (r.status, r.pivots, r.total_cost, r.flows, r.potentials, r.trace))
            assert_rows_equal(r, hook, what)
            assert st["lds_instances"] == mix.count and st["global_instances"] == 0 and st["lds_bytes_max"] == max(stride_of(t) for t in mix.tops), st
            if budget == k:
                assert any(a[0] == NOT_SOLVED for a in answers) and st["launches"] >= 2, st           # the refused search is a launch of its own
            if budget in (0, k):
                numpy_in = DEVICE_NUMPY[0](mix.handle(rule, pivot_limit=k, record_trace=cap, pivots_per_launch=budget), mix.arrays(), stype)
                assert isinstance(numpy_in.flows, np.ndarray) and isinstance(numpy_in.trace, np.ndarray)
                assert_rows_equal(numpy_in, hook, (what, "numpy in"))


def test_lds_and_global_tier_under_a_pivot_limit():
    """One pivot_limit goes into every graph's slot template: instances of both tiers are stopped in the same round."""
    mix = mixed_tiers()
    a = mix.arrays()
    k = 16
    for stype in SUPPLY_TYPES:
        answers = [limited(x, k) for x in mixed_answers(stype)]
        stopped = [sum(x[0] == NOT_SOLVED for x, (g, _) in zip(answers, mix.order) if (g in (0, 2)) == in_global) for in_global in (True, False)]
        print(f"mixed tiers under a pivot limit of {k}, supply type {stype}: stopped in the global tier {stopped[0]}, in LDS {stopped[1]}")
        assert min(stopped) >= 1, stopped
        hook = HOST[0](mix.handle(pivot_limit=k, record_trace=MIXED_TRACE), a, stype)
        assert_equals_answers(mix.split(hook), answers, "hook", trace_cap=MIXED_TRACE)
        for kw in ({}, dict(pivots_per_launch=11)):
            h = mix.handle(pivot_limit=k, record_trace=MIXED_TRACE, **kw)
            assert_rows_equal(DEVICE[0](h, a, stype), hook, (stype, kw))
            st = h.stats()
            assert st["lds_instances"] == 3 * MIXED_PER and st["global_instances"] == 2 * MIXED_PER and st["workspace_bytes"] == footprints(mix), st
            assert st["total_pivots"] == sum(x[1] for x in answers), st


@pytest.mark.parametrize("rule", ALL_RULES)
def test_resolve_chain_under_a_pivot_limit_on_the_device(rule):
    check_resolve_chain_under_a_limit(*DEVICE, rule)


@functools.lru_cache(maxsize=None)
def limited_hook_chain(rule, stype):
    """the hook's rows under the rule's limit of MIX_RESOLVE_LIMIT: after the first solve and after each of the four re-solves"""
    mix = resolve_mix()
    a = mix.arrays()
    h = mix.handle(rule, pivot_limit=MIX_RESOLVE_LIMIT[rule])
    return (to_numpy(HOST[0](h, a, stype)),) + tuple(to_numpy(HOST[1](h, dict(a, cost=mix_costs(mix, step)), stype)) for step in range(STEPS))


@pytest.mark.parametrize("slices", [0, 3])
@pytest.mark.parametrize("rule", ALL_RULES)
def test_resolve_chain_and_mask_under_a_pivot_limit_equal_the_hook(rule, slices):
    mix = resolve_mix()
    a = mix.arrays()
    for stype in SUPPLY_TYPES:
        rows = limited_hook_chain(rule, stype)
        h = mix.handle(rule, pivot_limit=MIX_RESOLVE_LIMIT[rule], pivots_per_launch=slices)
        assert_rows_equal(DEVICE[0](h, a, stype), Rows(rows[0]), (stype, "first solve"))
        for step in range(STEPS):
            assert_rows_equal(DEVICE[1](h, dict(a, cost=mix_costs(mix, step)), stype), Rows(rows[step + 1]), (stype, step))
    check_unchanged_costs_and_mask_under_a_limit_mix(*DEVICE, rule, pivots_per_launch=slices)


@pytest.mark.parametrize("rule", ALL_RULES)
def test_the_device_equals_the_hook_in_any_order_under_a_pivot_limit(rule):
    """The orders of test_the_device_equals_the_hook_in_any_order: slab and slots of limit-stopped instances move whole between host and device."""
    mix = resolve_mix()
    a = mix.arrays()
    costs = [dict(a, cost=mix_costs(mix, step)) for step in range(2)]
    for stype in SUPPLY_TYPES:
        rows = limited_hook_chain(rule, stype)
        assert (rows[0]["status"] == NOT_SOLVED).any() and (rows[1]["status"] == NOT_SOLVED).any()
        for order in ((DEVICE[0], DEVICE[1], DEVICE[1]), (HOST[0], DEVICE[1], DEVICE[1]), (DEVICE[0], HOST[1], DEVICE[1]), (DEVICE_NUMPY[0], DEVICE[1], HOST[1])):
            h = mix.handle(rule, pivot_limit=MIX_RESOLVE_LIMIT[rule])
            assert_rows_equal(order[0](h, a, stype), Rows(rows[0]), stype)
            assert_rows_equal(order[1](h, costs[0], stype), Rows(rows[1]), stype)
            assert_rows_equal(order[2](h, costs[1], stype), Rows(rows[2]), stype)


def test_validation_of_limit_stopped_results_as_they_lie():
    """solve()'s tensors under a limit go into validate() as they are: 16 bytes up (the two summary words) and 16 down."""
    def validate(h, r, a, stype):
        assert r.status.is_cuda and r.flows.is_cuda
        return h.validate(r, supply_type=stype, **tensors(a))
    for c, v in check_validation_under_a_limit(DEVICE[0], validate, DEVICE[1]):
        assert v.valid.is_cuda and v.errors.is_cuda and v.summary["bytes_up"] == 16 and v.summary["bytes_down"] == 16, v.summary
