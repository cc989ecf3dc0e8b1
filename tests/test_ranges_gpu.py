"""Cost ranges of the kept basis on the MI355X (mcf_ubatch_cost_ranges / mcf_rbatch_cost_ranges, DESIGN.md 3.14 "Cost ranges of the kept
basis"): one wave per instance walks the cycles of the instance's non-tree arcs, in LDS where the instance is solved in LDS, in place
otherwise.

Every comparison is exact: against the host hook's rows bit for bit, against the brute force of ranges_oracle.py, and through the
existing resolve() for what the numbers mean.  The batches and the checkers are test_ranges_host.py's.  Each test is a few launches over
at most 408 tiny instances or 18 padded ones."""
import numpy as np
import pytest
import torch

import mincostflow_amd as M
from oracle import ns_oracle as O

import ranges_oracle as R
from test_batch_host import fuzz_cases, padded_fuzz
from test_ranges_host import (FIELDS, HOST_RANGES, HOST_SOLVE, HOST_UNIFORM, assert_same_ranges, check_against_brute_force, check_contract, check_empty_and_infeasible,
                              check_meaning, check_one_graph, check_solves_do_not_see_it, fuzz_flat, padded_flat, range_rows, recosted, redata, small_case)
from test_uniform_host import ALL_RULES, uniform_of

pytestmark = pytest.mark.gpu


def tensors(a):
    return {k: (torch.from_numpy(np.ascontiguousarray(v)).cuda() if isinstance(v, np.ndarray) else v) for k, v in a.items()}


SOLVE = lambda h, a, stype: h.solve(supply_type=stype, **tensors(a))
SOLVE_NUMPY = lambda h, a, stype: h.solve(supply_type=stype, **a)
RANGES = lambda h: h.cost_ranges()
UNIFORM = (lambda u, a: u.solve(**tensors(a)), lambda u, a: u.resolve(**tensors(a)), lambda u, a: u.resolve_data(**tensors(a)))
UNIFORM_NUMPY = (lambda u, a: u.solve(**a), lambda u, a: u.resolve(**a), lambda u, a: u.resolve_data(**a))


def hook_rows(flat, rule):
    """per supply type the host hook's rows of the whole handle"""
    h = flat.handle(rule)
    out = {}
    for stype in (O.GEQ, O.LEQ):
        HOST_SOLVE(h, flat.arrays, stype)
        out[stype] = HOST_RANGES(h)
    return out


# ---- 1: the adversarial batch, every instance in the LDS tier
@pytest.mark.parametrize("rule", ALL_RULES)
def test_adversarial_batch_equals_the_hook_and_the_brute_force_on_the_device(rule):
    flat = fuzz_flat()
    hook = hook_rows(flat, rule)
    for stype, h, g in check_against_brute_force(SOLVE, RANGES, flat, [s for _, s in fuzz_cases()], R.fuzz_ranges(rule), rule):
        assert all(getattr(g, name).is_cuda for name in FIELDS)
        assert_same_ranges(g, hook[stype], (rule, stype))
        st = h.range_stats()
        print(f"rule {rule}, supply type {stype}: {st}")
        assert st["lds_instances"] == flat.count and st["global_instances"] == 0, st
        assert st["bytes_down"] == 24 and st["bytes_up"] in (24, 24 + 4 * flat.count), st          # the summary words; the table of instances once
        # numpy out of the same state: the rows come down through the staging buffer
        gn = h.cost_ranges(tensors=False)
        assert isinstance(gn.cost_down, np.ndarray)
        assert_same_ranges(gn, hook[stype], (rule, stype, "numpy"))
        stn = h.range_stats()
        assert stn["bytes_up"] == 24 and stn["bytes_down"] == 24 + 4 * flat.count + 17 * int(flat.arc_rows[-1]), stn
        assert {k: stn[k] for k in ("ranged", "tree_arcs", "cycle_hops")} == {k: st[k] for k in ("ranged", "tree_arcs", "cycle_hops")}


# ---- 2: the global tier
@pytest.mark.parametrize("rule", ALL_RULES)
def test_padded_instances_in_the_global_tier(rule):
    flat = padded_flat(rule)
    hook = hook_rows(flat, rule)
    for stype, h, g in check_against_brute_force(SOLVE, RANGES, flat, [s for _, s, _ in padded_fuzz(rule)], R.padded_ranges(rule), rule):
        assert_same_ranges(g, hook[stype], (rule, stype))
        st = h.range_stats()
        print(f"rule {rule}, supply type {stype}: {st}")
        assert st["global_instances"] == flat.count == 18 and st["lds_instances"] == 0, st
        assert h.stats()["global_instances"] == flat.count


# ---- 3
def test_one_graph_equals_the_uniform_batch_on_the_device():
    check_one_graph(SOLVE, SOLVE, RANGES)


# ---- 4: what the numbers mean
def test_a_cost_inside_its_range_makes_no_pivot_and_one_past_it_does_on_the_device():
    u = check_meaning(UNIFORM[0], UNIFORM[1], RANGES, reference=lambda u: u.cost_ranges_on_host())
    assert u.range_stats()["instances"] == len(u)
    check_meaning(UNIFORM_NUMPY[0], UNIFORM_NUMPY[1], RANGES)


def test_ranges_after_a_resolve_and_after_a_warm_resolve_data_on_the_device():
    """The bases a re-solve leaves are the batch's own: the references are the hook on the same state, and the re-solve itself."""
    check_meaning(UNIFORM[0], UNIFORM[1], RANGES, between=recosted, reference=lambda u: u.cost_ranges_on_host())
    check_meaning(UNIFORM[0], UNIFORM[1], RANGES, between=redata(UNIFORM[2]), reference=lambda u: u.cost_ranges_on_host())


# ---- 5: the contract
def test_contract_on_the_device(have_gpu):
    check_contract(lambda h, a: h.solve(**a), "cost_ranges", False, have_gpu)


def test_empty_and_infeasible_batches_on_the_device():
    check_empty_and_infeasible(lambda u, a: u.solve(**a), lambda h, a: h.solve(**a), RANGES)


def test_solve_calls_do_not_see_a_ranges_call_on_the_device():
    check_solves_do_not_see_it(UNIFORM[0], UNIFORM[1], UNIFORM[2], RANGES)


def test_the_state_moves_between_host_and_device():
    """Hook after a device solve, device after a hook's solve, and a device re-solve after both: the same rows every way."""
    t, a = small_case()
    dev, host = uniform_of(t, O.RULE_BLOCK), uniform_of(t, O.RULE_BLOCK)
    r_dev, r_host = UNIFORM_NUMPY[0](dev, a), HOST_UNIFORM[0](host, a)
    want = host.cost_ranges_on_host()
    assert_same_ranges(dev.cost_ranges_on_host(), want, "hook after a device solve")
    assert_same_ranges(host.cost_ranges(tensors=False), want, "device after a hook's solve")
    assert_same_ranges(dev.cost_ranges(tensors=False), want, "device after the hook read the device's state")
    other = dict(a, cost=np.ascontiguousarray(a["cost"][::-1]))
    r1, r2 = UNIFORM_NUMPY[1](dev, other), HOST_UNIFORM[1](host, other)
    for name in ("status", "pivots", "total_cost", "flows", "potentials"):
        assert np.array_equal(getattr(r1, name), getattr(r2, name)), name
    assert_same_ranges(dev.cost_ranges(tensors=False), host.cost_ranges_on_host(), "after the re-solves")
    assert range_rows(want)["ranged"].sum() > 0
