"""Re-solving a solved batch with new arc costs on the MI355X (mcf_batch_resolve, DESIGN.md 3.14 "Re-solve"): the state of every
instance stays in device memory, a warm instance gets its new cost array and its slot, batch_reprice recomputes its potentials on the
device and the pivots go on from the kept basis.

Items 1 to 6 are the check functions of test_batch_resolve_host.py with solve / resolve in the place of the host hooks (reference: the
oracle's cold solve with the new costs).  The others compare the device with mcf_batch_rerun_on_host bit for bit.  Durations on an
MI355X: DESIGN.md 3.14."""
import ctypes as C

import numpy as np
import pytest

import mincostflow_amd as M
from mincostflow_amd import _lib as L
from oracle import ns_oracle as O

from test_batch_host import LDS_LIMITS, PADDED_NODES, RULES, footprint_of
from test_batch_resolve_host import (ALL_RULES, HOST, STEPS, TRACE, check_art_cost_moves, check_chains, check_errors_and_order, check_mixed_batch,
                                     check_unchanged_costs, family, family_reference, family_solver, original_reference, run_family_steps,
                                     snapshot, warm_after)

pytestmark = pytest.mark.gpu

DEVICE = (lambda b: b.solve(), lambda b: b.resolve())
UP16 = lambda x: (x + 15) // 16 * 16
SLOT_BYTES = 2 * 8 + 3 * 8 + 12 * 4 + 2 * 8 + C.sizeof(L.BlockConfig)      # BatchSlot of csrc/batch.hip, restated: 104 bytes and the block configuration


def assert_same(a, b, count=None):
    for i in range(len(a) if count is None else count):
        assert snapshot(a, i) == snapshot(b, i), i


# ---- 1 to 6 on the device
@pytest.mark.parametrize("rule", ALL_RULES)
def test_unchanged_costs_need_no_pivot_on_the_device(rule):
    check_unchanged_costs(*DEVICE, rule)


@pytest.mark.parametrize("rule", ALL_RULES)
def test_new_costs_against_a_cold_solve_on_the_device(rule):
    run_family_steps(DEVICE[0](family_solver(rule)), rule, DEVICE[1])


@pytest.mark.parametrize("rule", ALL_RULES)
def test_chains_do_not_drift_on_the_device(rule):
    check_chains(*DEVICE, rule)


@pytest.mark.parametrize("rule", ALL_RULES)
def test_art_cost_follows_the_costs_on_the_device(rule):
    check_art_cost_moves(*DEVICE, rule)


@pytest.mark.parametrize("rule", ALL_RULES)
def test_mixed_batch_on_the_device(rule):
    b = check_mixed_batch(*DEVICE, rule)
    st = b.resolve_stats()
    assert st["launches"] >= 1 and 0 < st["bytes_uploaded"] and 0 < st["bytes_downloaded"]
    check_mixed_batch(*DEVICE, rule, pivots_per_launch=2)


def test_errors_and_order_on_the_device():
    check_errors_and_order(DEVICE[0], "resolve")


# ---- 7, 8: the device equals the hook, whatever came first
def stepped(rule, calls, steps=2, **kw):
    """The family solved by calls[0] and re-solved with the costs of step 0, 1, ... by calls[1], calls[2], ..."""
    b = getattr(family_solver(rule, **kw), calls[0])()
    refs = family_reference(rule)
    for step in range(steps):
        for i, (cost, *_rest) in enumerate(refs[step]):
            b.set_costs(i, cost)
        getattr(b, calls[1 + step])()
    return b


@pytest.mark.parametrize("rule", ALL_RULES)
def test_the_device_equals_the_hook_in_any_order(rule):
    """Status, pivot count, whole trace, flows and potentials of the second re-solve, bit for bit: the device all the way; the hook all
    the way; no slab when the first re-solve comes (everything is packed from the host's copies, core_reopen included); a slab that the
    hook made stale (dropped and packed again)."""
    hook = stepped(rule, ("run_on_host", "rerun_on_host", "rerun_on_host"))
    dev = stepped(rule, ("solve", "resolve", "resolve"))
    assert_same(dev, hook)
    warm = sum(warm_after(r) for r in family_reference(rule)[0])
    st = dev.resolve_stats()
    assert st["warm_instances"] == warm >= 10 and st["launches"] >= 1 and st["total_pivots"] == hook.resolve_stats()["total_pivots"] > 0
    assert_same(stepped(rule, ("run_on_host", "resolve", "resolve")), hook)
    assert_same(stepped(rule, ("solve", "rerun_on_host", "resolve")), hook)
    assert_same(stepped(rule, ("run_on_host", "rerun_on_host", "resolve")), hook)
    assert_same(stepped(rule, ("solve", "resolve", "rerun_on_host")), hook)


# ---- 9
@pytest.mark.parametrize("rule", ALL_RULES)
def test_slices_reprice_once(rule):
    """pivots_per_launch 1 and 3: the potentials are recomputed in the first slice only (a second time would still be right after a
    pivot -- but the slot's flag must be gone, and the traces must be the default's)."""
    whole = stepped(rule, ("solve", "resolve"), steps=1)
    for ppl in (1, 3):
        sliced = stepped(rule, ("solve", "resolve"), steps=1, pivots_per_launch=ppl)
        assert sliced.resolve_stats()["launches"] > whole.resolve_stats()["launches"]
        assert sliced.resolve_stats()["launches"] >= max(sliced.pivots(i) for i in range(len(sliced))) // ppl
        assert_same(whole, sliced)


# ---- 10
def padded(p):
    return O.Problem(PADDED_NODES, p.m, p.src, p.tgt, p.lower, p.upper, p.cost, np.concatenate([p.supply, np.zeros(PADDED_NODES - p.n, np.int64)]))


@pytest.mark.parametrize("rule", ALL_RULES)
def test_both_tiers_in_one_resolve(rule):
    """Six warm and three cold instances padded with isolated zero-supply nodes to 4 500 nodes (no LDS limit holds them: batch_reprice and
    the pivots run in place), with LDS-tier neighbours between them."""
    orig = original_reference(rule)
    big = [k for k in range(len(family()) - 1, -1, -1) if family()[k][0].m + family()[k][0].n >= 257]          # the largest first
    warm = [k for k in big if warm_after(orig[k])][:6]
    cold = [k for k in big if orig[k][0] == O.INFEASIBLE][:3]
    small = [k for k in range(len(family())) if warm_after(orig[k])][:4]
    assert len(warm) == 6 and len(cold) == 3 and len(small) == 4
    order = [(k, True) for k in warm[:3]] + [(small[0], False), (cold[0], True), (small[1], False)] + [(k, True) for k in warm[3:]] + \
            [(cold[1], True), (small[2], False), (cold[2], True), (small[3], False)]
    dev = M.BatchSolver(rule=RULES[rule], record_trace=TRACE)
    hook = M.BatchSolver(rule=RULES[rule], record_trace=TRACE)
    for k, pad in order:
        p, stype = family()[k]
        q = padded(p) if pad else p
        assert (footprint_of(q, stype) > max(LDS_LIMITS)) == pad
        dev.add(q, supply_type=stype)
        hook.add(q, supply_type=stype)
    dev.solve()
    hook.run_on_host()
    assert dev.stats()["global_instances"] == 9 and dev.stats()["lds_instances"] == 4
    assert_same(dev, hook)
    for step in range(2):
        for i, (k, _) in enumerate(order):
            for b in (dev, hook):
                b.set_costs(i, family_reference(rule)[step][k][0])
        dev.resolve()
        hook.rerun_on_host()
        st = dev.resolve_stats()
        assert st["warm_instances"] == 10 and st["cold_instances"] == 3 and st["launches"] >= 2, st
        assert_same(dev, hook)
        for i, (k, _) in enumerate(order):
            ref = family_reference(rule)[step][k]
            assert dev.status(i) == ref[1] and (ref[1] != O.OPTIMAL or dev.total_cost(i) == ref[2]), (step, i)


def test_a_warm_resolve_uploads_costs_and_slots_only():
    """A batch of warm instances only: what goes up is, per instance, its cost array over all its arcs (8 A bytes, rounded up to 16 as
    the workspace layout does) and its slot -- restated here -- and far less than the workspaces."""
    rule = O.RULE_BLOCK
    picked = [k for k, r in enumerate(original_reference(rule)) if warm_after(r) and warm_after(family_reference(rule)[0][k])]
    assert len(picked) >= 10
    b = M.BatchSolver(rule=RULES[rule], record_trace=64)
    arcs = []
    for k in picked:
        p, stype = family()[k]
        b.add(p, supply_type=stype)
        s = p.supply.copy()
        np.subtract.at(s, p.src, p.lower)
        np.add.at(s, p.tgt, p.lower)
        arcs.append(p.m + p.n + int(np.sum(s > 0) if stype == O.GEQ else np.sum(s < 0)))     # as footprint_of counts them
    b.solve()
    for i, k in enumerate(picked):
        b.set_costs(i, family_reference(rule)[0][k][0])
    b.resolve()
    st = b.resolve_stats()
    print(st, b.stats()["workspace_bytes"])
    assert st["warm_instances"] == len(picked) and st["cold_instances"] == 0
    assert st["bytes_uploaded"] == sum(UP16(8 * A) for A in arcs) + len(picked) * SLOT_BYTES
    assert st["bytes_uploaded"] < b.stats()["workspace_bytes"]
    assert 0 < st["bytes_downloaded"]
    for i, k in enumerate(picked):
        ref = family_reference(rule)[0][k]
        assert b.status(i) == ref[1] == O.OPTIMAL and b.total_cost(i) == ref[2]
