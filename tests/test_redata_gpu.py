"""Re-solving placed batches with new supplies and bounds on the MI355X (mcf_ubatch_resolve_data / mcf_rbatch_resolve_data, DESIGN.md 3.14
"Re-solve with new data"): the re-data launch, the dual pivots of batch_dual_kernel in both tiers, the settle launch and the fallback.

The family, the references and the checkers are test_redata_host.py's: the oracle's cold solve on the new data.  On top of them the device
is compared with the one-lane hook bit for bit -- the leaving-arc search and the ratio test combine 64 lanes, which the hook cannot see."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import mincostflow_amd as M
from mincostflow_amd import _lib as L
from oracle import ns_oracle as O

from test_redata_host import (HOST, STEPS, chain, check_back_and_forth, check_chain, check_changed_mask, check_mixed_with_new_costs, check_padded_chain,
                              check_unchanged_data, check_under_a_limit, expected_warm, padded_chain, redata_family)
from test_batch_resolve_host import cold_reference
from test_uniform_host import ALL_RULES, assert_rows_equal, to_numpy, uniform_of

pytestmark = pytest.mark.gpu
SLOT_BYTES = 104 + C.sizeof(L.BlockConfig)           # BatchSlot of csrc/batch_layout.hip.h, which has no padding


def tensors(a):
    return {k: (torch.from_numpy(np.ascontiguousarray(v)).cuda() if isinstance(v, np.ndarray) else v) for k, v in a.items()}


DEVICE = (lambda u, a, stype: u.solve(supply_type=stype, **tensors(a)), lambda u, a, stype, **kw: u.resolve_data(supply_type=stype, **tensors(a), **tensors(kw)))
DEVICE_NUMPY = (lambda u, a, stype: u.solve(supply_type=stype, **a), lambda u, a, stype, **kw: u.resolve_data(supply_type=stype, **a, **kw))
RECOST = lambda u, a, stype, **kw: u.resolve(supply_type=stype, **tensors(a), **tensors(kw))


class Rows:
    """to_numpy()'s dict with the attributes of a result, so that the checkers take it."""

    def __init__(self, rows):
        self.__dict__.update(rows)


# ---- 1
@pytest.mark.parametrize("rule", ALL_RULES)
def test_chain_on_the_device(rule):
    check_chain(*DEVICE, rule)


# ---- 2: the device equals the hook
@functools.lru_cache(maxsize=None)
def hook_chain(rule):
    """per graph: the hook's rows after the first solve and after every step"""
    out = []
    for (t, steps), (_, stype) in zip(chain(), redata_family()):
        u = uniform_of(t, rule)
        rows = [to_numpy(HOST[0](u, t.arrays(), stype))]
        rows += [to_numpy(HOST[1](u, top.arrays(), stype)) for top in steps]
        out.append(tuple(rows))
    return tuple(out)


@pytest.mark.parametrize("slices", [0, 1, 3])
def test_the_device_equals_the_hook(slices):
    """status, pivots, total cost, flows, potentials and trace of every step, whole and in slices of 1 and 3 pivots (a slice boundary inside
    the dual phase, at its hand-over and inside a fallback's cold solve)"""
    rule = O.RULE_BLOCK
    for j, (((t, steps), (_, stype)), hook) in enumerate(zip(zip(chain(), redata_family()), hook_chain(rule))):
        u = uniform_of(t, rule, pivots_per_launch=slices)
        assert_rows_equal(DEVICE[0](u, t.arrays(), stype), Rows(hook[0]), (j, "first solve"))
        host = uniform_of(t, rule)
        HOST[0](host, t.arrays(), stype)
        for s, name in enumerate(STEPS):
            r = DEVICE[1](u, steps[s].arrays(), stype)
            assert r.status.is_cuda and r.flows.is_cuda and r.trace.is_cuda
            assert_rows_equal(r, Rows(hook[s + 1]), (j, name, slices))
            HOST[1](host, steps[s].arrays(), stype)
            mine, theirs = u.resolve_data_stats(), host.resolve_data_stats()
            for field in ("warm_instances", "cold_instances", "fallback_instances", "untouched_instances", "dual_pivots", "primal_pivots"):
                assert mine[field] == theirs[field], (j, name, field, mine, theirs)
            if slices:
                assert mine["launches"] >= -(-int(to_numpy(r)["pivots"].max()) // slices)


@pytest.mark.parametrize("order", ["dhdhdhd", "hdhdhdh", "ddhhddh", "hhdddhh"])
def test_any_order_of_device_and_hook(order):
    """every step by the device (tensors, or numpy at every other device step) or by the hook: the state moves whole, the rows are the hook's"""
    rule = O.RULE_BLOCK
    for j, (((t, steps), (_, stype)), hook) in enumerate(zip(zip(chain(), redata_family()), hook_chain(rule))):
        u = uniform_of(t, rule)
        (DEVICE[0] if order[0] == "h" else HOST[0])(u, t.arrays(), stype)       # the first solve by the other side
        for s, (name, who) in enumerate(zip(STEPS, order)):
            again = HOST[1] if who == "h" else (DEVICE[1], DEVICE_NUMPY[1])[s % 2]
            assert_rows_equal(again(u, steps[s].arrays(), stype), Rows(hook[s + 1]), (j, name, order))


# ---- 3: the checkers of the host file, on the device
def test_unchanged_data_need_no_pivot_on_the_device():
    check_unchanged_data(*DEVICE, O.RULE_BLOCK)


def test_back_and_forth_on_the_device():
    check_back_and_forth(*DEVICE, O.RULE_BLOCK)


def test_changed_mask_on_the_device():
    check_changed_mask(*DEVICE, O.RULE_BLOCK)
    check_changed_mask(*DEVICE_NUMPY, O.RULE_BLOCK, pivots_per_launch=2)


def test_mixed_with_new_costs_on_the_device():
    check_mixed_with_new_costs(*DEVICE, RECOST, O.RULE_BLOCK)


def test_under_a_pivot_limit_on_the_device():
    check_under_a_limit(*DEVICE, O.RULE_BLOCK)
    check_under_a_limit(*DEVICE, O.RULE_BLOCK, pivots_per_launch=2)


# ---- 4: both tiers in one call
@functools.lru_cache(maxsize=None)
def padded_hook():
    base, steps = padded_chain()
    h = base.handle(O.RULE_BLOCK)
    rows = [to_numpy(HOST[0](h, base.arrays(), O.GEQ))]
    rows += [to_numpy(HOST[1](h, mix.arrays(), O.GEQ)) for mix in steps]
    return tuple(rows)


@pytest.mark.parametrize("slices", [0, 7])
def test_three_graphs_in_both_tiers(slices):
    """the chain over three graphs in one handle, the padded one in the global tier: against the oracle, and bit for bit the hook's"""
    seen = []

    def again(h, a, stype):
        r = DEVICE[1](h, a, stype)
        st = h.stats()
        assert st["lds_instances"] == 2 * st["global_instances"] > 0, st
        seen.append(to_numpy(r))
        return r
    check_padded_chain(DEVICE[0], again, O.RULE_BLOCK, pivots_per_launch=slices)
    for s, (mine, theirs) in enumerate(zip(seen, padded_hook()[1:])):
        assert_rows_equal(Rows(mine), Rows(theirs), (STEPS[s], slices))


# ---- 5: what crosses the bus
def test_traffic_of_a_warm_call_with_tensors():
    """A call whose every instance is warm: up the slot template and the ids of the one round; down the slots three times -- after the
    re-data launch, after the round and after the settle launch.  Nothing scales with arcs or nodes: two graphs, the same bytes per instance."""
    per_instance = []
    for j in (0, 2):
        (t, steps), (_, stype) = chain()[j], redata_family()[j]
        keep = [k for k, p in enumerate(steps[0].variants)
                if expected_warm(cold_reference(t.variants[k], stype, O.RULE_BLOCK), p) and cold_reference(p, stype, O.RULE_BLOCK)[0] == O.OPTIMAL]
        assert len(keep) >= 4
        t, new = t.subset(keep), steps[0].subset(keep)
        u = uniform_of(t, O.RULE_BLOCK)
        u.solve(supply_type=stype, **tensors(t.arrays()))
        u.resolve_data(supply_type=stype, **tensors(new.arrays()))
        st, rs = u.stats(), u.resolve_data_stats()
        assert rs["warm_instances"] == t.count and rs["cold_instances"] == rs["fallback_instances"] == 0 and rs["dual_pivots"] > 0 and rs["launches"] == 1, rs
        assert st["bytes_up"] == rs["bytes_up"] == SLOT_BYTES + 4 * t.count, st
        assert st["bytes_down"] == rs["bytes_down"] == 3 * t.count * SLOT_BYTES, st
        per_instance.append((st["bytes_up"] - SLOT_BYTES) // t.count + st["bytes_down"] // t.count)
        # numpy in: the arrays as well, one copy each
        v = uniform_of(t, O.RULE_BLOCK)
        v.solve(supply_type=stype, **t.arrays())
        v.resolve_data(supply_type=stype, **new.arrays())
        sv = v.stats()
        assert sv["bytes_up"] == st["bytes_up"] + 8 * t.count * (3 * t.m + t.n), sv
        assert sv["bytes_down"] == st["bytes_down"] + t.count * (4 + 8 + 8 + 8 * t.m + 8 * t.n + 4 * u.record_trace), sv
    assert per_instance[0] == per_instance[1]


# ---- 6: refusals
def test_bad_tensors_are_refused_before_anything_is_launched():
    t, stype = redata_family()[0]
    good = tensors(t.arrays())
    u = uniform_of(t, O.RULE_BLOCK)
    with pytest.raises(M.McfError) as e:
        u.resolve_data(supply_type=stype, **good)                                  # before any solve
    assert e.value.code == L.ERR_STATE
    first = to_numpy(u.solve(supply_type=stype, **good))
    before = u.stats()
    bad = (dict(good, supply=good["supply"].cpu()), dict(good, upper=good["upper"].to(torch.int32)), dict(good, lower=good["lower"][:, :-1]),
           dict(good, cost=good["cost"].t().contiguous().t()), dict(good, supply=t.arrays()["supply"]))
    for kw in bad:
        with pytest.raises(ValueError):
            u.resolve_data(supply_type=stype, **kw)
    with pytest.raises(ValueError):
        u.rerun_data_on_host(supply_type=stype, **good)
    with pytest.raises(M.McfError) as e:
        u.resolve_data(supply_type=O.LEQ if stype == O.GEQ else O.GEQ, **good)
    assert e.value.code == L.ERR_INVALID
    assert u.stats() == before and u.resolve_data_stats()["launches"] == 0
    # and the handle is as it was: the same data again, no pivot where warm, the same rows
    again = to_numpy(u.resolve_data(supply_type=stype, **good))
    assert u.resolve_data_stats()["dual_pivots"] == 0
    for name in ("status", "total_cost", "flows", "potentials"):
        assert np.array_equal(again[name], first[name]), name
