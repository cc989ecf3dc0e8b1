"""Unbounded or not, on the MI355X (mcf_ubatch_rays / mcf_rbatch_rays, DESIGN.md 3.14 "Unbounded or not: a negative cycle or labels from
the kept data"): one wave per instance runs a level-synchronous Bellman-Ford over the uncapacitated arcs -- costs, capacities, labels,
marks and frontiers in LDS where the instance is solved in LDS, the working arrays in a buffer of the handle's otherwise.

Every comparison is exact: against the host hook bit for bit (verdict, cycle_cost, cycle_length, on_cycle, label and the work counts of the
stats) and against ray_oracle.py.  The batches and the checkers are test_rays_host.py's.  Each test is a few launches over at most 204
tiny instances, 64 of 161 nodes or 12 padded into the global tier."""
import numpy as np
import pytest
import torch

import mincostflow_amd as M
from oracle import ns_oracle as O

import ray_oracle as R
from test_diagnose_host import FlatNodes, diag_rows
from test_rays_host import (CYCLE_NODES, FIELDS, HOST_RAYS, HOST_SOLVE, Ray, assert_same_rays, check_answers, check_by_bounds_between_neighbours, check_contract,
                            check_edges, check_family, check_kept_data, check_long_cycles, check_one_graph, check_padded, check_the_hazard, check_untouched, family_flat,
                            padded_family, ray_rows, ray_topology, same_counts)
from test_batch_host import PADDED_NODES
from test_uniform_host import Topology, uniform_of

pytestmark = pytest.mark.gpu
SUMMARY_BYTES = 8 * 8           # four verdict counts and four work counts


def tensors(a):
    return {k: (torch.from_numpy(np.ascontiguousarray(v)).cuda() if isinstance(v, np.ndarray) else v) for k, v in a.items()}


SOLVE = lambda h, a, stype: h.solve(supply_type=stype, **tensors(a))
SOLVE_NUMPY = lambda h, a, stype: h.solve(supply_type=stype, **a)
RESOLVE = lambda h, a, stype: h.resolve(supply_type=stype, **tensors(a))
RAYS = lambda h: h.rays()
RAYS_NUMPY = lambda h: h.rays(tensors=False)


# ---- 1: the family, from device tensors to device tensors: the LDS tier
def test_family_equals_the_hook_and_the_oracle_on_the_device():
    flat = family_flat()
    host = flat.handle()
    calls = []

    def rays(h):
        d = h.rays()
        assert all(getattr(d, name).is_cuda for name in FIELDS)
        stype = O.GEQ if not calls else O.LEQ
        HOST_SOLVE(host, flat.arrays, stype)
        assert_same_rays(d, HOST_RAYS(host), stype)
        st = h.ray_stats()
        assert st["lds_instances"] == flat.count and st["global_instances"] == 0 and same_counts(st, host.ray_stats()), (st, host.ray_stats())
        # MCF_MEM_DEVICE moves the summary words and nothing else; the table of instances goes up with the first call
        assert st["bytes_down"] == SUMMARY_BYTES and st["bytes_up"] == SUMMARY_BYTES + (0 if calls else 4 * flat.count), st
        calls.append(stype)
        return d

    check_family(SOLVE, rays)
    assert calls == [O.GEQ, O.LEQ]


# ---- 2: the global tier: a node sweep of 71 strides per round
def test_padded_instances_in_the_global_tier():
    flat = FlatNodes(padded_family())
    host = flat.handle()
    HOST_SOLVE(host, flat.arrays, O.GEQ)
    want = HOST_RAYS(host)

    def stats_check(st):
        assert st["global_instances"] == flat.count == 12 and st["lds_instances"] == 0 and same_counts(st, host.ray_stats()), (st, host.ray_stats())
        assert st["bytes_down"] == SUMMARY_BYTES, st

    h, d, u, st = check_padded(SOLVE, RAYS, stats_check)
    assert d.label.is_cuda
    assert_same_rays(d, want, "padded")
    assert st["global_instances"] == len(u) == 3 and st["lds_instances"] == 0 and st["bytes_down"] == SUMMARY_BYTES, st       # the uniform handle


# ---- 3: a frontier wider than a wave: the ballot prefix is carried across strides
HUB_COUNT = 64
HUB_LEAVES = 160


def hub_batch():
    """A hub (node 0) with 160 leaves 64 times: an uncapacitated arc of cost -1 .. -5 out to every leaf and one of cost 5 .. 9 back, so every
    leaf's label falls in round 1 and the frontier of round 2 holds all 160 -- three strides of the collect step.  Even variants stop
    there (no way round is negative: BOUNDED); in the odd ones one arc back costs 0, which closes a negative cycle through the hub: the
    hub falls, then every leaf again, in turn until round k + 1 = 162."""
    n, leaves = HUB_LEAVES + 1, np.arange(1, HUB_LEAVES + 1)
    src = np.concatenate([np.zeros(HUB_LEAVES, np.int64), leaves]).astype(np.int32)
    tgt = np.concatenate([leaves, np.zeros(HUB_LEAVES, np.int64)]).astype(np.int32)
    m = len(src)
    variants = []
    for k in range(HUB_COUNT):
        rng = np.random.default_rng([R.SEED, 9, k])
        cost = np.concatenate([-rng.integers(1, 6, HUB_LEAVES), rng.integers(5, 10, HUB_LEAVES)]).astype(np.int64)
        if k % 2:
            cost[HUB_LEAVES + int(rng.integers(0, HUB_LEAVES))] = 0
        supply = np.zeros(n, np.int64)
        ends = rng.choice(leaves, 8, replace=False)
        supply[ends[:4]] += 2
        supply[ends[4:]] -= 2
        variants.append(O.Problem(n, m, src, tgt, np.zeros(m, np.int64), np.full(m, O.INF_CAP, np.int64), cost, supply))
    return Topology(n, src, tgt, variants, [False] * HUB_COUNT)


def test_a_frontier_wider_than_a_wave():
    t = hub_batch()
    sizes = [R.jacobi_frontiers(p) for p in t.variants]
    truth = [R.has_negative_cycle(p) for p in t.variants]
    assert truth == [bool(k % 2) for k in range(HUB_COUNT)]
    # restated from the data: the second frontier of every instance spans three strides; a cyclic one alternates between the leaves and the hub
    assert all(s[:2] == [HUB_LEAVES + 1, HUB_LEAVES] for s in sizes) and all(len(s) == (HUB_LEAVES + 2 if c else 2) for s, c in zip(sizes, truth))
    assert all(max(s[2:]) > 128 and min(s[2:]) == 1 for s, c in zip(sizes, truth) if c) and HUB_LEAVES > 2 * 64
    a = t.arrays()
    dev, host = uniform_of(t, O.RULE_BLOCK), uniform_of(t, O.RULE_BLOCK)
    SOLVE(dev, a, O.GEQ)
    HOST_SOLVE(host, a, O.GEQ)
    d = RAYS(dev)
    assert d.on_cycle.shape == (HUB_COUNT, t.m) and d.label.shape == (HUB_COUNT, t.n) and d.on_cycle.is_cuda
    assert_same_rays(d, HOST_RAYS(host), "hub")
    st = dev.ray_stats()
    assert st["lds_instances"] == HUB_COUNT and same_counts(st, host.ray_stats()), (st, host.ray_stats())
    assert st["bytes_down"] == SUMMARY_BYTES and st["bytes_up"] == SUMMARY_BYTES + 4 * HUB_COUNT, st
    assert st["rounds"] == sum(len(s) for s in sizes) and st["frontier_nodes"] == sum(sum(s) for s in sizes), st
    rows = ray_rows(d)
    assert list(rows["verdict"]) == [Ray.Cycle if c else Ray.Bounded for c in truth] and st["cycle_arcs"] == 2 * (HUB_COUNT // 2)
    for k, p in enumerate(t.variants):
        if truth[k]:
            R.check_cycle(p, rows["on_cycle"][k], rows["cycle_cost"][k], rows["cycle_length"][k])
        else:
            R.check_labels(p, rows["label"][k])


# ---- 4: depth: 301 rounds with a frontier of one node each, in LDS and in place in global memory
def test_a_cycle_of_300_arcs_and_its_zero_cost_twin_on_the_device():
    st = check_long_cycles(SOLVE, RAYS)
    assert st["lds_instances"] == 1 and st["global_instances"] == 0, st


def test_the_same_cycles_padded_into_the_global_tier():
    st = check_long_cycles(SOLVE, RAYS, CYCLE_NODES, PADDED_NODES)
    assert st["lds_instances"] == 0 and st["global_instances"] == 1, st


# ---- 5: both tiers in one handle, and the buffer the global tier shares with diagnose()
def test_two_tiers_in_one_handle_in_turn_with_diagnose():
    problems = [p for p, _ in R.ray_family()][-30:] + list(padded_family())
    flat = FlatNodes(problems)
    dev, host = flat.handle(), flat.handle()
    SOLVE(dev, flat.arrays, O.GEQ)
    HOST_SOLVE(host, flat.arrays, O.GEQ)
    want_rays, want_diag = HOST_RAYS(host), diag_rows(host.diagnose_on_host())
    ray_counts = host.ray_stats()
    for turn in range(2):
        diag = diag_rows(dev.diagnose())
        for name, row in want_diag.items():
            assert np.array_equal(diag[name], row), (turn, name)
        d = RAYS(dev)
        assert_same_rays(d, want_rays, turn)
        st = dev.ray_stats()
        assert st["lds_instances"] == 30 and st["global_instances"] == 12 and same_counts(st, ray_counts), (st, ray_counts)
    check_answers(problems, flat, d, st, "two tiers")


# ---- 6: nothing to walk
def test_no_instances_all_by_their_bounds_and_numpy_rows_from_a_device_solve():
    t = ray_topology()
    a = t.arrays()
    bad = dict(a, upper=np.ascontiguousarray(a["lower"] - 1))
    u = uniform_of(t, O.RULE_BLOCK)
    SOLVE(u, bad, O.GEQ)
    for d in (RAYS(u), RAYS_NUMPY(u), HOST_RAYS(u), RAYS(u)):
        rows = ray_rows(d)
        assert np.all(rows["verdict"] == Ray.Bounds) and not rows["cycle_cost"].any() and not rows["cycle_length"].any() and not rows["on_cycle"].any() and not rows["label"].any()
        st = u.ray_stats()
        assert st["bounds"] == t.count == st["instances"] and st["rounds"] == st["frontier_nodes"] == st["inc_entries"] == st["cycle_arcs"] == 0, st
    u = M.UniformBatch(t.n, t.src, t.tgt, 0)
    SOLVE(u, {k: v[:0] for k, v in a.items()}, O.GEQ)
    d = RAYS(u)
    assert d.verdict.shape == (0,) and d.on_cycle.shape == (0, t.m) and d.label.shape == (0, t.n) and u.ray_stats()["instances"] == 0
    # a handle solved from tensors, asked for numpy rows: the arrays cross the bus, the answers are the same
    u, host = uniform_of(t, O.RULE_BLOCK), uniform_of(t, O.RULE_BLOCK)
    SOLVE(u, a, O.GEQ)
    HOST_SOLVE(host, a, O.GEQ)
    d = RAYS_NUMPY(u)
    assert isinstance(d.on_cycle, np.ndarray) and isinstance(d.label, np.ndarray)
    assert_same_rays(d, HOST_RAYS(host), "numpy rows")
    st = u.ray_stats()
    assert st["bytes_down"] == SUMMARY_BYTES + t.count * (4 + 8 + 4) + t.count * t.m + 8 * t.count * t.n and st["bytes_up"] == SUMMARY_BYTES + 4 * t.count, st


def test_the_state_moving_between_host_and_device():
    t = ray_topology()
    a = t.arrays()
    want = None
    for solve_on_device, first_on_device in ((True, True), (True, False), (False, True), (False, False)):
        u = uniform_of(t, O.RULE_BLOCK)
        (SOLVE_NUMPY if solve_on_device else HOST_SOLVE)(u, a, O.GEQ)
        order = (RAYS_NUMPY, HOST_RAYS) if first_on_device else (HOST_RAYS, RAYS_NUMPY)
        for rays in order + order:
            d = rays(u)
            assert isinstance(d.label, np.ndarray)
            want = want or d
            assert_same_rays(d, want, (solve_on_device, first_on_device))
    assert Ray.Cycle in ray_rows(want)["verdict"]


# ---- 7: the rest of the host file on the device
def test_contract_on_the_device():
    check_contract(lambda h, a: h.solve(**a), "rays", False)


def test_hand_made_edges_on_the_device():
    check_edges(SOLVE, RAYS)
    check_the_hazard(SOLVE, RAYS)
    check_by_bounds_between_neighbours(SOLVE, RAYS)


def test_one_graph_equals_the_uniform_batch_on_the_device():
    check_one_graph(SOLVE, RAYS, lambda h, arcs, labels: h.rays(arcs=arcs, labels=labels))


def test_the_answer_follows_every_kind_of_solve_call_on_the_device():
    check_kept_data(SOLVE, RESOLVE, lambda h, a, s: h.resolve_data(supply_type=s, **tensors(a)),
                    lambda h, states, a, s: h.solve_from(torch.from_numpy(states).cuda(), supply_type=s, **tensors(a)), RAYS)


def test_the_kept_state_is_untouched_on_the_device():
    check_untouched(SOLVE, RESOLVE, RAYS, (lambda h: h.cost_ranges(), lambda h: h.data_ranges(), lambda h: h.diagnose()))
