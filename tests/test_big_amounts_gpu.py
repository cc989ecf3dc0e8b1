"""Supplies, bounds and flows beyond 32 bits on the MI355X (DESIGN.md 3.14 "Amounts beyond 32 bits"): the families of big_amounts.py
through the device's calls on tensors.  On the device an amount passes through code the one-lane hooks replace by the identity: the
64-bit lane sums of the supply totals and of diagnose()'s violation, the 64-bit atomics on shifted[] and flow[] in LDS and in global
memory, the lane maximum of batch_find_violated, the two rooms a walk of data_ranges() gathers in registers, the 16-byte copies of flow
and upper into LDS, and the batch validator's objective.

The checkers are test_big_amounts_host.py's: the oracle bit for bit, the scaling law against the hooks' unscaled record, the independent
oracles on every query.  What the device returned and counted in every call is then compared with the hooks' record of the same calls,
bit for bit."""
import numpy as np
import pytest
import torch

import big_amounts as B
import wide_graphs as W
from test_big_amounts_host import (SINGLE, Calls, check_adversarial_law, check_batch_solver, check_cuts_law, check_ragged_law, check_single_solve,
                                   check_structured_law, check_wide_law, hook_log, irregular_log, irregular_ragged_log, meaning_case)
from test_data_ranges_host import check_meaning
from test_wide_host import assert_same_log

pytestmark = pytest.mark.gpu


def tensor(v):
    return torch.from_numpy(np.ascontiguousarray(v)).cuda() if isinstance(v, np.ndarray) else v


def tensors(a):
    return {k: tensor(v) for k, v in a.items()}


DEVICE = Calls(first=lambda u, a, stype: u.solve(supply_type=stype, **tensors(a)),
               again=lambda u, a, stype: u.resolve_data(supply_type=stype, **tensors(a)),
               recost=lambda u, a, stype: u.resolve(supply_type=stype, **tensors(a)),
               start=lambda u, rows, a, stype: u.solve_from(tensor(rows), supply_type=stype, **tensors(a)),
               ranges=lambda u: u.cost_ranges(),
               data_ranges=lambda u, pairs: u.data_ranges(pairs=pairs),
               diagnose=lambda u: u.diagnose(),
               validate=lambda u, r, a, stype: u.validate(r, supply_type=stype, **tensors(a)),
               batch=lambda b: b.solve())
FACTOR_IDS = ("K_HIGH", "K_SIGN")


def in_tier(handles, tier):
    other = {"lds_instances": "global_instances", "global_instances": "lds_instances"}[tier]
    for h in handles:
        for st in (h.stats(), h.range_stats(), h.data_range_stats(), h.diagnose_stats()):
            assert st[tier] > 0 and st[other] == 0, st


# ---- 1: the LDS tier: the three small graphs whole, and the grid of 12 x 12 in slices of 1 and 3 pivots per launch
@pytest.mark.parametrize("k", B.FACTORS, ids=FACTOR_IDS)
@pytest.mark.parametrize("g", B.SMALL_GRAPHS, ids=[W.NAMES[g] for g in B.SMALL_GRAPHS])
def test_small_wide_graphs_in_lds(g, k):
    handles = []
    assert_same_log(check_wide_law(DEVICE, g, k, handles=handles), hook_log("wide chain", g, k), (W.NAMES[g], k))
    in_tier(handles, "lds_instances")


@pytest.mark.parametrize("slices", [1, 3])
def test_the_grid_in_slices(slices):
    assert_same_log(check_wide_law(DEVICE, W.GRID, B.K_HIGH, pivots_per_launch=slices), hook_log("wide chain", W.GRID, B.K_HIGH), ("slices", slices))


# ---- 2: the global tier: the big grid, a connected tree of 841 nodes whose flows and shifted supplies lie in global memory
@pytest.mark.parametrize("k", B.FACTORS, ids=FACTOR_IDS)
def test_the_big_grid_in_the_global_tier(k):
    handles = []
    assert_same_log(check_wide_law(DEVICE, W.BIG, k, handles=handles), hook_log("wide chain", W.BIG, k), ("big grid", k))
    in_tier(handles, "global_instances")


# ---- 3: both tiers in one ragged call
@pytest.mark.parametrize("k", B.FACTORS, ids=FACTOR_IDS)
def test_both_tiers_in_one_ragged_handle(k):
    log, h = check_ragged_law(DEVICE, k)
    assert_same_log(log, hook_log("ragged", k), ("ragged", k))
    for st in (h.stats(), h.range_stats(), h.data_range_stats(), h.diagnose_stats()):
        assert st["lds_instances"] > 0 and st["global_instances"] > 0, st


# ---- 4: the structured graph (infinite sides), the cuts wider than a wave, what the data ranges mean
@pytest.mark.parametrize("k", B.FACTORS, ids=FACTOR_IDS)
def test_the_structured_graph_on_the_device(k):
    assert_same_log(check_structured_law(DEVICE, k), hook_log("structured", k), ("structured", k))


@pytest.mark.parametrize("k", B.FACTORS, ids=FACTOR_IDS)
def test_cuts_wider_than_a_wave_on_the_device(k):
    assert_same_log(check_cuts_law(DEVICE, k), hook_log("cuts", k), ("cuts", k))


def test_a_datum_moved_by_its_range_keeps_the_basis_and_one_past_it_does_not_on_the_device():
    check_meaning(DEVICE.first, DEVICE.again, lambda u, pairs, **kw: u.data_ranges(pairs=pairs, **kw), meaning_case(),
                  reference=lambda u, pairs: u.data_ranges_on_host(pairs=pairs))


# ---- 5: the adversarial family: one ragged handle under every rule, and BatchSolver.solve()
@pytest.mark.parametrize("k", B.FACTORS, ids=FACTOR_IDS)
@pytest.mark.parametrize("rule", B.ALL_RULES)
def test_the_adversarial_family_in_one_ragged_handle(rule, k):
    assert_same_log(check_adversarial_law(DEVICE, k, rule), hook_log("adversarial", k, rule), ("adversarial", k, rule))


@pytest.mark.parametrize("rule", B.ALL_RULES)
def test_the_adversarial_family_in_a_batch_solver(rule):
    check_batch_solver(DEVICE.batch, B.K_HIGH, rule)


# ---- 6: the irregular family
@pytest.mark.parametrize("i", range(len(B.SMALL_GRAPHS)), ids=[W.NAMES[g] for g in B.SMALL_GRAPHS])
def test_the_irregular_family_on_the_device(i):
    assert_same_log(irregular_log(DEVICE, i), hook_log("irregular", i), ("irregular", i))


def test_the_irregular_family_in_one_ragged_handle_on_the_device():
    assert_same_log(irregular_ragged_log(DEVICE), hook_log("irregular ragged"), "irregular ragged")


# ---- 7: the single-solve path
@pytest.mark.parametrize("name", SINGLE)
def test_a_single_solve_follows_the_law(name):
    pivots, largest = check_single_solve(name, lambda ns: ns.set_device(0))
    print(f"{name} times K_HIGH: {pivots} pivots, largest flow {largest}")
