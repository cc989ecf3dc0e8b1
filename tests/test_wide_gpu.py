"""Warm re-solves, cost ranges and given starts on the graphs of wide_graphs.py on the MI355X: graphs of 130 to 841 connected nodes whose
supplies lie on nodes >= 64, so that batch_find_violated's answer, the supply sums and the set-up loops of the start, and the tree flows
lie past the first stride of the wave; trees deeper than 64; and the big grid, a connected tree of 841 nodes in the global tier.

The checkers are test_wide_host.py's, run with the device's calls on tensors: the oracle's cold solve, the brute force on the oracle's
basis and start_oracle's classes.  Each runs under the recorder of that file, and what the device returned and counted -- status, pivots,
total cost, flows, potentials, trace, and the counted statistics of every call -- is compared with what the hooks recorded, bit for bit."""
import numpy as np
import pytest
import torch

import wide_graphs as W
from test_wide_host import (HOST, RULE, SMALL_GRAPHS, Calls, Recorded, assert_same_log, check_cost_step, check_hostile_rows, check_meaning_on_the_grid, check_ragged,
                            check_shared_row, check_steps, graph, hook_log)
from test_uniform_host import uniform_of

pytestmark = pytest.mark.gpu


def tensor(v):
    return torch.from_numpy(np.ascontiguousarray(v)).cuda() if isinstance(v, np.ndarray) else v


def tensors(a):
    return {k: tensor(v) for k, v in a.items()}


DEVICE = Calls(first=lambda u, a, stype: u.solve(supply_type=stype, **tensors(a)),
               again=lambda u, a, stype, **kw: u.resolve_data(supply_type=stype, **tensors(a), **tensors(kw)),
               recost=lambda u, a, stype, **kw: u.resolve(supply_type=stype, **tensors(a), **tensors(kw)),
               ranges=lambda u, **kw: u.cost_ranges(**kw),
               start=lambda u, rows, a, stype: u.solve_from(tensor(rows), supply_type=stype, **tensors(a)))
# whole and in slices of 1 and 3 pivots on the LDS graphs; of 7 on the big grid, whose solves run a few thousand pivots
SLICED = [(g, slices) for g in SMALL_GRAPHS for slices in (0, 1, 3)] + [(W.BIG, 0), (W.BIG, 7)]
SLICED_IDS = [f"{W.NAMES[g]}-{slices}" for g, slices in SLICED]


def on_device(check, *args, **kw):
    """the checker with the device's calls; what it recorded equals the hooks' record"""
    rec = Recorded(DEVICE)
    out = check(rec, *args, **kw)
    names = {check_steps: "steps", check_cost_step: "cost step", check_shared_row: "shared row", check_hostile_rows: "hostile rows", check_ragged: "ragged"}
    assert_same_log(rec.log, hook_log(names[check], *args), (names[check], args, kw))
    return out


# ---- 1: first solve, ranges, the four steps, ranges of warm bases, the round trip
@pytest.mark.parametrize("g, slices", SLICED, ids=SLICED_IDS)
def test_steps_ranges_and_round_trip_on_the_device(g, slices):
    u = on_device(check_steps, g, pivots_per_launch=slices)
    st, rs = u.stats(), u.range_stats()
    tier, other = ("global_instances", "lds_instances") if g == W.BIG else ("lds_instances", "global_instances")
    assert st[tier] > 0 and st[other] == 0, st
    assert rs[tier] > 0 and rs[other] == 0, rs
    if slices:                          # the last step ran in slices: no fewer launches than its longest row needs
        last = [rows for kind, rows, _ in hook_log("steps", g) if kind == "resolve_data"][-1]
        assert u.resolve_data_stats()["launches"] >= -(-int(last["pivots"].max()) // slices), u.resolve_data_stats()


# ---- 2: the cost step
@pytest.mark.parametrize("g", range(len(W.NAMES)), ids=W.NAMES)
def test_mixed_with_new_costs_on_the_device(g):
    on_device(check_cost_step, g)


# ---- 3: what the ranges mean
def test_a_cost_inside_its_range_makes_no_pivot_and_one_past_it_does_on_the_device():
    check_meaning_on_the_grid(DEVICE, reference=lambda u: u.cost_ranges_on_host())


# ---- 4: starts
@pytest.mark.parametrize("g, slices", SLICED, ids=SLICED_IDS)
def test_one_shared_row_on_the_device(g, slices):
    on_device(check_shared_row, g, pivots_per_launch=slices)


@pytest.mark.parametrize("slices", [0, 1])
def test_hostile_rows_on_the_chorded_path_on_the_device(slices):
    on_device(check_hostile_rows, pivots_per_launch=slices)


# ---- 5: both tiers in one ragged handle
@pytest.mark.parametrize("slices", [0, 7])
def test_one_ragged_handle_in_both_tiers(slices):
    h, started = on_device(check_ragged, pivots_per_launch=slices)
    for st in (h.stats(), h.range_stats(), started.stats()):            # the steps, the ranges, and the handle of the start
        assert st["lds_instances"] > 0 and st["global_instances"] > 0, st


# ---- 6: any order of device and hook
@pytest.mark.parametrize("g", [W.GRID, W.BIG], ids=[W.NAMES[W.GRID], W.NAMES[W.BIG]])
@pytest.mark.parametrize("order", ["dhdh", "hdhd"])
def test_any_order_of_device_and_hook(order, g):
    """first solve, step a, ranges, step c, each by the device or by the hook: the state moves whole, the rows and the counts are the hook's"""
    t, steps, stype, _ = graph(g)
    sequence = (lambda c, u: c.first(u, t.arrays(), stype), lambda c, u: c.again(u, steps[0].arrays(), stype), lambda c, u: c.ranges(u),
                lambda c, u: c.again(u, steps[2].arrays(), stype))
    want = Recorded(HOST)
    u = uniform_of(t, RULE)
    for call in sequence:
        call(want, u)
    mixed = {"d": Recorded(DEVICE), "h": Recorded(HOST)}
    mixed["h"].log = mixed["d"].log
    u = uniform_of(t, RULE)
    for who, call in zip(order, sequence):
        call(mixed[who], u)
    assert_same_log(mixed["d"].log, want.log, (W.NAMES[g], order))
