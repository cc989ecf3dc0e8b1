"""Starting placed batches from a basis the caller supplies on the MI355X (mcf_ubatch_solve_from / mcf_rbatch_solve_from, DESIGN.md 3.14
"Start from a given basis"): the start launch in both tiers, the rounds of batch_dual_kernel, the settle launch and the fallback.

The cases, the references and the checkers are test_start_host.py's: the oracle's cold solve and start_oracle's predicted classes.  On top
of them the device is compared with the one-lane hook bit for bit -- the counts, the sums and the class are combined over 64 lanes and
the walk runs between two barriers, which the hook cannot see."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import mincostflow_amd as M
from mincostflow_amd import _lib as L
from oracle import ns_oracle as O

from test_redata_host import PADDED_NODES, SMALL, STEPS, chain, padded_chain, redata_family
from test_start_host import (COPIES, DATA_STEPS, FROM_HOST, REDATA_HOST, RECOST_HOST, check_hostile_rows, check_mixed, check_new_costs,
                             check_new_data, check_ragged, check_round_trip, check_shared_row, check_under_a_limit, first_solve, is_spanning, padded_first,
                             recost_cases, shared_case)
from test_uniform_host import assert_rows_equal, step_costs, to_numpy, uniform_of

pytestmark = pytest.mark.gpu
SLOT_BYTES = 104 + C.sizeof(L.BlockConfig)           # BatchSlot of csrc/batch_layout.hip.h, which has no padding
COUNTED = ("primal_starts", "dual_starts", "cold_instances", "fallback_instances", "dual_pivots", "primal_pivots")


def tensor(v):
    return torch.from_numpy(np.ascontiguousarray(v)).cuda() if isinstance(v, np.ndarray) else v


def tensors(a):
    return {k: tensor(v) for k, v in a.items()}


FROM_DEVICE = lambda u, rows, a, stype: u.solve_from(tensor(rows), supply_type=stype, **tensors(a))
FROM_DEVICE_NUMPY = lambda u, rows, a, stype: u.solve_from(rows, supply_type=stype, **a)
SOLVE_DEVICE = lambda u, a, stype: u.solve(supply_type=stype, **tensors(a))
RECOST_DEVICE = lambda u, a, stype: u.resolve(supply_type=stype, **tensors(a))
REDATA_DEVICE = lambda u, a, stype: u.resolve_data(supply_type=stype, **tensors(a))
RANGES_DEVICE = lambda u: u.cost_ranges(costs=False)


class Rows:
    """to_numpy()'s dict with the attributes of a result, so that the checkers take it."""

    def __init__(self, rows):
        self.__dict__.update(rows)


# ---- 1: the checkers of the host file, on the device
def test_round_trip_on_the_device():
    check_round_trip(SOLVE_DEVICE, FROM_DEVICE, RANGES_DEVICE, O.RULE_BLOCK)


def test_new_costs_and_new_data_on_the_device():
    check_new_costs(FROM_DEVICE, O.RULE_BLOCK)
    check_new_data(FROM_DEVICE, O.RULE_BLOCK)


def test_hostile_rows_are_cold_by_rule_on_the_device():
    check_hostile_rows(SOLVE_DEVICE, FROM_DEVICE, O.RULE_BLOCK)


def test_mixed_with_the_other_calls_and_under_a_limit_on_the_device():
    check_mixed(FROM_DEVICE, RECOST_DEVICE, REDATA_DEVICE, RANGES_DEVICE, O.RULE_BLOCK)
    check_under_a_limit(SOLVE_DEVICE, FROM_DEVICE, REDATA_DEVICE, O.RULE_BLOCK, pivots_per_launch=2)


# ---- 2: the device equals the hook
def start_cases(rule):
    """per graph: ((name, arrays) ...): the first solve's data (the round trip), its new costs, and the data after steps a, b, c and e"""
    out = []
    for j, ((t, steps), (top, _)) in enumerate(zip(chain(), recost_cases(rule))):
        out.append((("round trip", t.arrays()), ("new costs", top.arrays())) + tuple((f"step {name}", steps[STEPS.index(name)].arrays()) for name in DATA_STEPS))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def hook_starts(rule):
    """per graph, per case: (the hook's rows, its start statistics), each on a fresh handle"""
    out = []
    for (t, stype), (_, _, rows), cases in zip(redata_family(), first_solve(rule), start_cases(rule)):
        per_case = []
        for _, a in cases:
            u = uniform_of(t, rule)
            per_case.append((to_numpy(FROM_HOST(u, rows, a, stype)), u.start_stats()))
        out.append(tuple(per_case))
    return tuple(out)


@pytest.mark.parametrize("slices", [0, 1, 3])
def test_the_device_equals_the_hook(slices):
    """status, pivots, total cost, flows, potentials, trace and the counted statistics of every case, whole and in slices of 1 and 3 pivots
    (a slice boundary inside the dual phase, at its hand-over, inside a primal start's pivots and inside a fallback's cold solve)"""
    rule = O.RULE_BLOCK
    for j, ((t, stype), (_, _, rows), cases, hook) in enumerate(zip(redata_family(), first_solve(rule), start_cases(rule), hook_starts(rule))):
        for (name, a), (theirs, their_stats) in zip(cases, hook):
            u = uniform_of(t, rule, pivots_per_launch=slices)
            r = FROM_DEVICE(u, rows, a, stype)
            assert r.status.is_cuda and r.flows.is_cuda and r.trace.is_cuda
            assert_rows_equal(r, Rows(theirs), (j, name, slices))
            mine = u.start_stats()
            for field in COUNTED:
                assert mine[field] == their_stats[field], (j, name, field, mine, their_stats)
            if slices:
                assert mine["launches"] >= -(-int(theirs["pivots"].max()) // slices)


# ---- 3: both tiers in one ragged call
def test_three_graphs_in_both_tiers():
    """Flat rows over three graphs, the padded one in the global tier with n > 64 (every ballot loop takes more than one stride), the small
    ones on either side of one wave (m + n = 63 and 65): against the oracle, and bit for bit the hook's"""
    base, steps = padded_chain()
    assert {(t.n, t.m) for t in base.tops} >= {(PADDED_NODES, SMALL[1]), (9, 56)} and SMALL == (9, 54)
    _, _, flat = padded_first(O.RULE_BLOCK)
    for slices in (0, 7):
        h = check_ragged(FROM_DEVICE, RANGES_DEVICE, O.RULE_BLOCK, pivots_per_launch=slices)
        st = h.stats()
        assert st["lds_instances"] == 2 * st["global_instances"] > 0, st
    mix = steps[STEPS.index("b")]
    host = base.handle(O.RULE_BLOCK)
    theirs = FROM_HOST(host, flat, mix.arrays(), O.GEQ)
    assert_rows_equal(h._last, theirs, "three graphs")
    mine, their_stats = h.start_stats(), host.start_stats()
    assert all(mine[field] == their_stats[field] for field in COUNTED), (mine, their_stats)


# ---- 4: device and hook calls in four orders on one handle
def order_calls(j, rule):
    """start, re-solve with new data, start on other data, re-solve with new costs: (device call, hook call, arrays) each"""
    (t, steps), (_, _, rows) = chain()[j], first_solve(rule)[j]
    later = steps[STEPS.index("c")]
    start_d = lambda u, a, stype: FROM_DEVICE(u, rows, a, stype)
    start_numpy = lambda u, a, stype: FROM_DEVICE_NUMPY(u, rows, a, stype)
    start_h = lambda u, a, stype: FROM_HOST(u, rows, a, stype)
    return ((start_d, start_h, t.arrays()), (REDATA_DEVICE, REDATA_HOST, steps[0].arrays()), (start_numpy, start_h, later.arrays()),
            (RECOST_DEVICE, RECOST_HOST, dict(later.arrays(), cost=step_costs(t, j, 1))))


@functools.lru_cache(maxsize=None)
def hook_orders(rule):
    out = []
    for j, (t, stype) in enumerate(redata_family()):
        u = uniform_of(t, rule)
        out.append(tuple(to_numpy(hook(u, a, stype)) for _, hook, a in order_calls(j, rule)))
    return tuple(out)


@pytest.mark.parametrize("order", ["dhdh", "hdhd", "ddhh", "hhdd"])
def test_any_order_of_device_and_hook(order):
    """every call by the device (tensors, the second start with numpy arrays) or by the hook: the state moves whole, the rows are the hook's"""
    rule = O.RULE_BLOCK
    for j, ((t, stype), hook) in enumerate(zip(redata_family(), hook_orders(rule))):
        u = uniform_of(t, rule)
        for c, (who, (device, host, a)) in enumerate(zip(order, order_calls(j, rule))):
            assert_rows_equal((device if who == "d" else host)(u, a, stype), Rows(hook[c]), (j, c, order))


# ---- 5: tensors, one shared row and one row each
def test_a_shared_row_and_a_row_each_as_tensors():
    check_shared_row(FROM_DEVICE, O.RULE_BLOCK)
    top, stype, a, row = shared_case(O.RULE_BLOCK)
    u, v = uniform_of(top, O.RULE_BLOCK), uniform_of(top, O.RULE_BLOCK)
    assert_rows_equal(FROM_DEVICE(u, row, a, stype), FROM_HOST(v, row, a, stype), "a shared row")
    wide = tensor(np.tile(row, (COPIES, 1)))
    assert tuple(wide.shape) == (COPIES, top.m) and wide.dtype == torch.int8
    assert_rows_equal(u.solve_from(wide, supply_type=stype, **tensors(a)), v._last, "a row each")


# ---- 6: what crosses the bus
def test_traffic_of_a_start_with_tensors():
    """A call whose every instance is a primal start that needs no pivot: up the slot template and the ids of the one round; down the slots
    three times -- after the start launch, after the round and after the settle launch.  Nothing scales with arcs, nodes or the rows of
    states: two graphs, the same bytes per instance."""
    rule = O.RULE_BLOCK
    per_instance = []
    for j in (0, 2):
        (t, stype), (_, ranged, rows) = redata_family()[j], first_solve(rule)[j]
        keep = [k for k in range(t.count) if is_spanning(t, ranged, rows, k)]
        assert len(keep) >= 4
        t, rows = t.subset(keep), np.ascontiguousarray(rows[keep])
        u = uniform_of(t, rule)
        r = FROM_DEVICE(u, rows, t.arrays(), stype)
        st, ss = u.stats(), u.start_stats()
        assert ss["primal_starts"] == t.count and ss["launches"] == 1 and not to_numpy(r)["pivots"].any(), ss
        assert st["bytes_up"] == ss["bytes_up"] == SLOT_BYTES + 4 * t.count, st
        assert st["bytes_down"] == ss["bytes_down"] == 3 * t.count * SLOT_BYTES, st
        per_instance.append((st["bytes_up"] - SLOT_BYTES) // t.count + st["bytes_down"] // t.count)
        # numpy in: the arrays as well, one copy each, the rows of states at one byte per arc
        v = uniform_of(t, rule)
        FROM_DEVICE_NUMPY(v, rows, t.arrays(), stype)
        sv = v.stats()
        assert sv["bytes_up"] == st["bytes_up"] + 8 * t.count * (3 * t.m + t.n) + t.count * t.m, sv
        assert sv["bytes_down"] == st["bytes_down"] + t.count * (4 + 8 + 8 + 8 * t.m + 8 * t.n + 4 * u.record_trace), sv
    assert per_instance[0] == per_instance[1]


# ---- 7: refusals
def test_bad_tensors_are_refused_before_anything_is_launched():
    rule = O.RULE_BLOCK
    (t, stype), (_, ranged, rows) = redata_family()[0], first_solve(rule)[0]
    good, state = tensors(t.arrays()), tensor(rows)
    u = uniform_of(t, rule)
    first = to_numpy(u.solve(supply_type=stype, **good))
    before = u.stats()
    bad = (state.cpu(), state.to(torch.int64), state[:, :-1], state[:-1], state.t().contiguous().t(), rows, None)
    for arc_state in bad:
        with pytest.raises(ValueError):
            u.solve_from(arc_state, supply_type=stype, **good)
    with pytest.raises(ValueError):
        u.solve_from(state, supply_type=stype, **dict(good, supply=good["supply"].cpu()))
    with pytest.raises(ValueError):
        u.run_from_on_host(state, supply_type=stype, **good)
    with pytest.raises(M.McfError) as e:
        u.solve_from(state, supply_type=7, **good)
    assert e.value.code == L.ERR_INVALID
    assert u.stats() == before and u.start_stats()["launches"] == 0
    # and the handle is as it was: the same costs again need no pivot where the first solve left an optimal basis
    again = to_numpy(u.resolve(supply_type=stype, **good))
    assert not again["pivots"][ranged].any()
    for name in ("status", "total_cost", "flows", "potentials"):
        assert np.array_equal(again[name], first[name]), name
