"""Supply and bound ranges of the kept basis on the MI355X (mcf_ubatch_data_ranges / mcf_rbatch_data_ranges, DESIGN.md 3.14 "Supply and
bound ranges of the kept basis"): one wave per instance, every lane walks the tree path of one non-tree arc or one pair and gathers the
rooms on it into two registers -- in LDS where the instance is solved in LDS, in place otherwise.

Every comparison is exact: against the host hook's rows bit for bit, against data_ranges_oracle.py, and through the existing
resolve_data() for what the numbers mean.  The batches and the checkers are test_data_ranges_host.py's.  Each test is a few launches
over at most 408 tiny instances, 28 wide ones or a handful padded into the global tier."""
import numpy as np
import pytest
import torch

import mincostflow_amd as M
from oracle import ns_oracle as O

import data_ranges_oracle as D
import wide_graphs as W
from test_batch_host import RULES
from test_data_ranges_host import (FIELDS, HOST_RANGES, HOST_REDATA, HOST_SOLVE, assert_same_data_ranges, check_adversarial_batch, check_contract, check_meaning,
                                   check_not_ranged, check_solves_do_not_see_it, check_three_graphs, check_uniform_families, data_rows, meaning_cases, three_graphs, two_tiers)
from test_ranges_host import fuzz_flat, small_case
from test_uniform_host import ALL_RULES, uniform_of

pytestmark = pytest.mark.gpu
COUNTED = ("instances", "ranged", "walks", "hops")


def tensors(a):
    return {k: (torch.from_numpy(np.ascontiguousarray(v)).cuda() if isinstance(v, np.ndarray) else v) for k, v in a.items()}


SOLVE = lambda h, a, stype: h.solve(supply_type=stype, **tensors(a))
SOLVE_NUMPY = lambda h, a, stype: h.solve(supply_type=stype, **a)
REDATA = lambda h, a, stype: h.resolve_data(supply_type=stype, **tensors(a))
RANGES = lambda h, pairs, **kw: h.data_ranges(pairs=pairs, **kw)
RANGES_NUMPY = lambda h, pairs, **kw: h.data_ranges(pairs=pairs, tensors=False, **kw)


def same_counts(a, b):
    return {k: a[k] for k in COUNTED} == {k: b[k] for k in COUNTED}


# ---- 1: every family against the hook and the reference
@pytest.mark.parametrize("rule", ALL_RULES)
def test_uniform_families_equal_the_hook_and_the_reference_on_the_device(rule):
    for u, t, stype, pairs, g, _ in check_uniform_families(SOLVE, RANGES, rule):
        assert all(getattr(g, name).is_cuda for name in FIELDS)
        st = u.data_range_stats()
        in_lds = u.stats()["lds_instances"]
        assert st["lds_instances"] == in_lds and st["global_instances"] == t.count - in_lds and (t.n < 800) == (in_lds == t.count), st
        assert st["bytes_down"] == 24 and st["bytes_up"] == 24 + 4 * t.count, st                # the summary words; the table of instances with the first call
        host = uniform_of(t, rule)
        HOST_SOLVE(host, t.arrays(), stype)
        hook = HOST_RANGES(host, pairs)
        assert_same_data_ranges(g, hook, (rule, t.n))
        assert same_counts(st, host.data_range_stats()), (st, host.data_range_stats())
        # numpy out of the same state: pairs up and rows down through the staging buffer
        gn = RANGES_NUMPY(u, pairs)
        assert isinstance(gn.flow_down, np.ndarray) and isinstance(gn.ship_back, np.ndarray)
        assert_same_data_ranges(gn, hook, (rule, t.n, "numpy"))
        stn = u.data_range_stats()
        assert stn["bytes_up"] == 24 + 8 * len(pairs) and stn["bytes_down"] == 24 + 4 * t.count + 17 * t.count * t.m + 16 * t.count * len(pairs), stn
        assert same_counts(stn, st)


@pytest.mark.parametrize("rule", ALL_RULES)
def test_adversarial_batch_equals_the_hook_and_the_reference_on_the_device(rule):
    flat, pair_lists = fuzz_flat(), list(D.fuzz_pairs())
    host = flat.handle(rule)
    calls = 0
    for h, g in check_adversarial_batch(SOLVE, RANGES, rule):
        stype = O.GEQ if calls == 0 else O.LEQ
        calls += 1
        HOST_SOLVE(host, flat.arrays, stype)
        assert_same_data_ranges(g, HOST_RANGES(host, pair_lists), (rule, stype))
        st = h.data_range_stats()
        assert st["lds_instances"] == flat.count and st["global_instances"] == 0 and same_counts(st, host.data_range_stats()), st
        assert st["bytes_down"] == 24 and st["bytes_up"] == 24 + (4 * flat.count if calls == 1 else 0), st


# ---- 2: both tiers in one ragged call
def test_both_tiers_in_one_ragged_call():
    """The 12 x 12 grid, the hub, the big grid and a graph of 9 nodes padded to PADDED_NODES isolated ones: 16 instances in LDS, the rest in place."""
    flat, graphs, graph_of, pair_lists = two_tiers()
    dev, host = (M.RaggedBatch(graphs, graph_of=graph_of, rule=RULES[O.RULE_BLOCK]) for _ in range(2))
    SOLVE(dev, flat.arrays, O.GEQ)
    HOST_SOLVE(host, flat.arrays, O.GEQ)
    g, hook = RANGES(dev, pair_lists), HOST_RANGES(host, pair_lists)
    assert_same_data_ranges(g, hook, "four graphs")
    st = dev.data_range_stats()
    assert st["lds_instances"] == 16 and st["global_instances"] == 8 and same_counts(st, host.data_range_stats()), st
    rows = data_rows(g)
    assert rows["ranged"][:20].all() and rows["ranged"][20:].any()
    check_three_graphs(SOLVE, RANGES)               # and the three wide graphs against the reference


# ---- 3: the state moves between host and device
def test_four_orders_of_device_and_hook_calls():
    t, a = small_case()
    pairs = D.pairs_of((6,), t.n, t.src, t.tgt)
    want = None
    for solve_on_device, first_on_device in ((True, True), (True, False), (False, True), (False, False)):
        u = uniform_of(t, O.RULE_BLOCK)
        (SOLVE_NUMPY if solve_on_device else HOST_SOLVE)(u, a, O.GEQ)
        order = (RANGES_NUMPY, HOST_RANGES) if first_on_device else (HOST_RANGES, RANGES_NUMPY)
        for ranges in order + order:
            g = ranges(u, pairs)
            want = want or g
            assert_same_data_ranges(g, want, (solve_on_device, first_on_device))
    assert data_rows(want)["ranged"].sum() > 0


def test_rows_after_a_resolve_and_after_a_resolve_data_equal_the_hook_on_the_same_state():
    t, stype = W.wide_family()[W.GRID]
    pairs = D.wide_pairs()[W.GRID]
    a = t.arrays()
    u = uniform_of(t, O.RULE_BLOCK)
    SOLVE(u, a, stype)
    recost = dict(a, cost=a["cost"] + np.arange(t.m) % 5)
    u.resolve(supply_type=stype, **tensors(recost))
    g = RANGES(u, pairs)
    assert_same_data_ranges(g, u.data_ranges_on_host(pairs=pairs), "after resolve()")
    assert data_rows(g)["ranged"].sum() >= 5
    step = W.wide_chain()[W.GRID][1][0].arrays()
    u.resolve_data(supply_type=stype, **tensors(dict(step, cost=recost["cost"])))
    assert u.resolve_data_stats()["warm_instances"] >= 5
    g = RANGES(u, pairs)
    assert_same_data_ranges(g, u.data_ranges_on_host(pairs=pairs), "after resolve_data()")
    assert data_rows(g)["ranged"].sum() > 0


# ---- 4: what the numbers mean
def test_a_datum_moved_by_its_range_keeps_the_basis_and_one_past_it_does_not_on_the_device():
    check_meaning(SOLVE, REDATA, RANGES, meaning_cases()[1], reference=lambda u, pairs: u.data_ranges_on_host(pairs=pairs))


# ---- 5: the contract
def test_contract_on_the_device():
    check_contract(lambda h, a: h.solve(**a), "data_ranges", False)


def test_solve_calls_and_cost_ranges_do_not_see_a_data_ranges_call_on_the_device():
    on = lambda name: (lambda u, a: getattr(u, name)(**tensors(a)))
    check_solves_do_not_see_it(on("solve"), on("resolve"), on("resolve_data"), RANGES, lambda u: u.cost_ranges())


def test_instances_that_are_not_ranged_give_zero_rows_on_the_device():
    check_not_ranged(SOLVE, RANGES, SOLVE)


def test_bytes_of_a_call_on_tensors():
    """MCF_MEM_DEVICE: the three summary words up and down, and with the handle's first call the table of instance ids; pairs, rows and
    the ragged tables never cross in the library."""
    flat, graphs, graph_of, pair_lists, _ = three_graphs(O.RULE_BLOCK)
    h = M.RaggedBatch(graphs, graph_of=graph_of, rule=RULES[O.RULE_BLOCK])
    SOLVE(h, flat.arrays, O.GEQ)
    on_device = [torch.from_numpy(p).cuda() for p in pair_lists]
    for call in range(3):
        g = h.data_ranges(pairs=on_device, tensors=True, flows=call != 1)
        st = h.data_range_stats()
        assert st["bytes_down"] == 24 and st["bytes_up"] == 24 + (4 * flat.count if call == 0 else 0), (call, st)
        assert (g.flow_down is None) == (call == 1) and g.ship_forth.is_cuda
    cost_first = h.cost_ranges()
    assert h.range_stats()["bytes_up"] == 24 + 4 * flat.count               # the cost ranges' own table, by its own classes


def test_bad_tensors_are_refused_before_anything_is_launched():
    t, a = small_case()
    pairs = D.pairs_of((6,), t.n, t.src, t.tgt)
    u = uniform_of(t, O.RULE_BLOCK)
    SOLVE(u, a, O.GEQ)
    good = RANGES(u, pairs)
    stats = u.data_range_stats()
    for bad in (torch.from_numpy(pairs), torch.from_numpy(pairs.astype(np.int64)).cuda(), torch.from_numpy(pairs).cuda().reshape(-1), torch.from_numpy(pairs).cuda()[:, :1]):
        with pytest.raises(ValueError):
            u.data_ranges(pairs=bad, tensors=True)
    with pytest.raises(ValueError):
        u.data_ranges(pairs=torch.from_numpy(pairs).cuda(), tensors=False)
    assert u.data_range_stats() == stats
    assert_same_data_ranges(RANGES(u, torch.from_numpy(pairs).cuda()[::2]), RANGES(u, pairs[::2]), "a strided tensor is made contiguous")
    assert_same_data_ranges(RANGES(u, pairs), good)
