"""Unbounded or not (mcf_ubatch_rays_on_host / mcf_rbatch_rays_on_host, DESIGN.md 3.14 "Unbounded or not: a negative cycle or labels from
the kept data") without a GPU: the hooks run the device's own step (csrc/rays_step.hip.h) with one lane on the CPU.

Every comparison is exact.  The reference is ray_oracle.py: an arc-list Bellman-Ford for the truth and exact-integer checks of every
cycle and every row of labels, on the caller's own numbers and sharing nothing with the code under test.  test_rays_gpu.py imports the
batches and the checkers from here."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import mincostflow_amd as M
from mincostflow_amd import _lib as L
from oracle import ns_oracle as O

import certificate_oracle as K
import ray_oracle as R
from adversarial import random_problem
from test_batch_host import LDS_LIMITS, PADDED_NODES, ROOT, footprint_of
from test_diagnose_host import FlatNodes, diag_rows, problem
from test_ranges_host import small_case
from test_uniform_host import Topology, on_topology, stride_of, to_numpy, uniform_of

Ray = M.Ray
FIELDS = ("verdict", "cycle_cost", "cycle_length", "on_cycle", "label")
COUNTS = ("instances", "none", "bounded", "cycle", "bounds", "rounds", "frontier_nodes", "inc_entries", "cycle_arcs")      # what host and device must agree on


def ray_rows(d):
    get = lambda a: a if a is None or isinstance(a, np.ndarray) else a.cpu().numpy()
    return {name: get(getattr(d, name)) for name in FIELDS}


def assert_same_rays(a, b, what=""):
    a, b = ray_rows(a), ray_rows(b)
    for name in FIELDS:
        assert a[name].dtype == b[name].dtype and np.array_equal(a[name].reshape(-1), b[name].reshape(-1)), (what, name)


def query_rows(result):
    """Every row another query answered with; None where it was not asked for"""
    get = lambda a: a if a is None or isinstance(a, np.ndarray) else a.cpu().numpy()
    return {name: get(getattr(result, name)) for name, _, _ in type(result).FIELDS}


def same_counts(a, b):
    return all(a[f] == b[f] for f in COUNTS)


def bound_infeasible(p):
    return bool(np.any(p.upper < p.lower))


def check_row(p, verdict, cycle_cost, cycle_length, on_cycle, label, what):
    """One answered row against the independent oracle"""
    assert on_cycle.shape == (p.m,) and label.shape == (p.n,), what
    if bound_infeasible(p):
        assert verdict == Ray.Bounds and not on_cycle.any() and not label.any() and cycle_cost == 0 and cycle_length == 0, (what, verdict)
        return
    assert verdict == (Ray.Cycle if R.has_negative_cycle(p) else Ray.Bounded), (what, verdict)
    if verdict == Ray.Cycle:
        R.check_cycle(p, on_cycle, cycle_cost, cycle_length)
        assert not label.any(), what
    else:
        R.check_labels(p, label)
        assert not on_cycle.any() and cycle_cost == 0 and cycle_length == 0, what


def work_of(problems):
    """(rounds, frontier nodes) of the documented rounds over all problems that are answered, restated from the data"""
    sizes = [R.jacobi_frontiers(p) for p in problems if not bound_infeasible(p)]
    return sum(len(s) for s in sizes), sum(sum(s) for s in sizes)


@functools.lru_cache(maxsize=None)
def family_flat():
    return FlatNodes([p for p, _ in R.ray_family()])


@functools.lru_cache(maxsize=None)
def family_truth():
    """has_negative_cycle per instance of the family.  The floors are asserted here, on the oracles' answers alone -- conditions on the
    inputs, before anything of the library is compared."""
    cases = R.ray_family()
    truth = tuple(R.has_negative_cycle(p) for p, _ in cases)
    rounds = [R.jacobi_rounds(p) for p, _ in cases]
    hazard = 0
    for (p, stype), cyclic in zip(cases, truth):
        assert not bound_infeasible(p)
        if not cyclic:
            continue
        lemon = O.Oracle(p, O.SEM_LEMON, O.RULE_BLOCK, supply_type=stype).solve()[0]
        assert lemon == (O.UNBOUNDED if K.feasible(p, stype) else lemon) and lemon in (O.UNBOUNDED, O.INFEASIBLE)
        if K.feasible(p, stype) and O.Oracle(p, O.SEM_CSHARP, O.RULE_BLOCK, supply_type=stype, auto_config=True).solve()[0] == O.OPTIMAL:
            hazard += 1
    floors = dict(cycle=sum(truth), none=len(truth) - sum(truth), optimal_although_unbounded=hazard,
                  two_arcs_or_more=sum(c and not R.only_loops_are_negative(p) for (p, _), c in zip(cases, truth)),
                  bounded_in_two_rounds_or_more=sum(r is not None and r >= 2 for r in rounds),
                  cycle_above_a_stride=sum(c and p.m + p.n > 64 for (p, _), c in zip(cases, truth)))
    print(f"ray family: {len(cases)} instances, {floors}, most rounds of a bounded one {max(r for r in rounds if r)}")
    assert len(cases) == 204 and floors["cycle"] >= 30 and floors["none"] >= 100 and floors["optimal_although_unbounded"] >= 20, floors
    assert floors["two_arcs_or_more"] >= 10 and floors["bounded_in_two_rounds_or_more"] >= 20 and floors["cycle_above_a_stride"] >= 25, floors
    return truth


def check_answers(problems, flat, d, st, what=""):
    """Every instance of a flat handle's answer against the oracle, none left out, and the statistics against the tally"""
    rows = ray_rows(d)
    assert rows["verdict"].shape == rows["cycle_cost"].shape == rows["cycle_length"].shape == (flat.count,)
    assert rows["on_cycle"].shape == (flat.arc_rows[-1],) and rows["label"].shape == (flat.node_rows[-1],)
    assert rows["verdict"].dtype == rows["cycle_length"].dtype == np.int32 and rows["cycle_cost"].dtype == rows["label"].dtype == np.int64 and rows["on_cycle"].dtype == np.int8
    for i, p in enumerate(problems):
        on_cycle, label = d.arcs(i), d.nodes(i)
        to_np = lambda a: a if isinstance(a, np.ndarray) else a.cpu().numpy()
        assert np.array_equal(to_np(on_cycle), rows["on_cycle"][flat.arc_rows[i]:flat.arc_rows[i + 1]])
        check_row(p, int(rows["verdict"][i]), int(rows["cycle_cost"][i]), int(rows["cycle_length"][i]), to_np(on_cycle), to_np(label), (what, i))
    assert st["instances"] == flat.count, st
    for name, verdict in (("none", Ray.NoVerdict), ("bounded", Ray.Bounded), ("cycle", Ray.Cycle), ("bounds", Ray.Bounds)):
        assert st[name] == int(np.sum(rows["verdict"] == verdict)), (name, st)
    assert st["cycle_arcs"] == int(rows["cycle_length"].sum()) == int(rows["on_cycle"].sum()), st
    assert (st["rounds"], st["frontier_nodes"]) == work_of(problems), (st, work_of(problems))
    return rows


def check_family(solve, rays, stats_check=None):
    """The family in one ragged handle, solved under each supply type: the answer is the data's and must be the same under both"""
    cases, flat, truth = R.ray_family(), family_flat(), family_truth()
    h = flat.handle()
    out = {}
    for stype in (O.GEQ, O.LEQ):
        solve(h, flat.arrays, stype)
        d = rays(h)
        st = h.ray_stats()
        rows = check_answers([p for p, _ in cases], flat, d, st, stype)
        assert [v == Ray.Cycle for v in rows["verdict"]] == list(truth) and st["cycle"] == sum(truth) and st["bounded"] == len(truth) - sum(truth), st
        if stats_check:
            stats_check(st)
        out[stype] = rows
    for name in FIELDS:
        assert np.array_equal(out[O.GEQ][name], out[O.LEQ][name]), name
    return out


HOST_SOLVE = lambda h, a, stype: h.run_on_host(supply_type=stype, **a)
HOST_RAYS = lambda h: h.rays_on_host()


def host_stats(st):
    assert st["lds_instances"] == st["global_instances"] == st["bytes_up"] == st["bytes_down"] == 0, st


# ---- 1: the family against the independent oracle
def test_family_on_the_host():
    check_family(HOST_SOLVE, HOST_RAYS, host_stats)


# ---- 2: hand-made edges
def one(p, stype=O.GEQ, solve=HOST_SOLVE, rays=HOST_RAYS):
    """(verdict, cycle cost, the marked arcs, labels, the solve's result, handle) of p alone in a ragged handle, checked against the oracle"""
    flat = FlatNodes([p])
    h = flat.handle()
    r = to_numpy(solve(h, flat.arrays, stype))
    rows = check_answers([p], flat, rays(h), h.ray_stats(), "hand-made")
    return int(rows["verdict"][0]), int(rows["cycle_cost"][0]), [int(e) for e in np.flatnonzero(rows["on_cycle"])], [int(x) for x in rows["label"]], r, h


TRIANGLE = [(0, 1, 0, None, -1), (1, 2, 0, None, -1), (2, 0, 0, None, -1)]


def edge_cases():
    """(name, problem, verdict, cycle cost, the cycle's arcs or None where several serve, labels or None)"""
    return (("a negative self loop", problem(2, [(0, 1, 0, 4, 1), (1, 1, 0, None, -2)], [1, -1]), Ray.Cycle, -2, [1], None),
            ("two parallel arcs out and one back: only the cheaper pair is negative", problem(2, [(0, 1, 0, None, 3), (0, 1, 0, None, 1), (1, 0, 0, None, -2)], [0, 0]),
             Ray.Cycle, -1, [1, 2], None),
            ("the same with the cheaper arc first", problem(2, [(0, 1, 0, None, 1), (0, 1, 0, None, 3), (1, 0, 0, None, -2)], [0, 0]), Ray.Cycle, -1, [0, 2], None),
            ("a negative cycle with one capacitated arc", problem(3, [(0, 1, 0, None, -1), (1, 2, 0, 7, -1), (2, 0, 0, None, -1)], [0, 0, 0]), Ray.Bounded, 0, [], [-1, -2, 0]),
            ("a zero-cost cycle", problem(3, [(0, 1, 0, None, -2), (1, 2, 0, None, 1), (2, 0, 0, None, 1)], [0, 0, 0]), Ray.Bounded, 0, [], [0, -2, -1]),
            ("a lower bound on an uncapacitated arc of the cycle", problem(3, [(0, 1, 2, None, -1), (1, 2, 0, None, -1), (2, 0, 0, None, -1)], [0, 0, 0]), Ray.Cycle, -3,
             [0, 1, 2], None),
            ("one node with no arcs", problem(1, [], [0]), Ray.Bounded, 0, [], [0]),
            ("no uncapacitated arc at all", problem(3, [(0, 1, 0, 5, -4), (1, 0, 0, 5, -4)], [0, 0, 0]), Ray.Bounded, 0, [], [0, 0, 0]),
            # what the rounds' end must get right: a path of k arcs whose labels all fall in round k is no cycle ...
            ("a negative path, every label falling up to round k", problem(4, [(0, 1, 0, None, -1), (1, 2, 0, None, -1), (2, 3, 0, None, -1)], [0, 0, 0, 0]), Ray.Bounded, 0, [],
             [0, -1, -2, -3]),
            # ... and the lowest node that still falls need not lie on the cycle: node 0 hangs off it
            ("a tail off the cycle at the lowest node", problem(6, [(3, 4, 0, None, -1), (4, 5, 0, None, -1), (5, 3, 0, None, -1), (5, 1, 0, None, 0), (1, 0, 0, None, 0)],
                                                                 [0] * 6), Ray.Cycle, -3, [0, 1, 2], None),
            # equal labels: a label is taken only when strictly below
            ("a zero-cost self loop and a zero-cost pair", problem(2, [(0, 0, 0, None, 0), (0, 1, 0, None, 0), (1, 0, 0, None, 0)], [0, 0]), Ray.Bounded, 0, [], [0, 0]))


def check_edges(solve, rays):
    for name, p, verdict, cost, arcs, labels in edge_cases():
        got = one(p, O.GEQ, solve, rays)
        assert got[:3] == (verdict, cost, arcs), (name, got[:4])
        assert labels is None or got[3] == labels, (name, got[3])


def test_hand_made_edges_on_the_host():
    check_edges(HOST_SOLVE, HOST_RAYS)


def check_the_hazard(solve, rays):
    """What the call is for: the status says Optimal and the objective is garbage"""
    for supply, extra, cost in (([0, 0, 0], [], 4611686018427387907), ([2, 0, -2, 0], [(0, 2, 0, 5, 3)], None)):
        p = problem(len(supply), TRIANGLE + extra, supply)
        assert O.Oracle(p, O.SEM_LEMON, O.RULE_BLOCK).solve()[0] == O.UNBOUNDED and K.feasible(p, O.GEQ)
        verdict, cycle_cost, arcs, _, r, h = one(p, O.GEQ, solve, rays)
        assert (verdict, cycle_cost, arcs) == (Ray.Cycle, -3, [0, 1, 2])
        assert r["status"][0] == O.OPTIMAL                                  # the hazard, pinned: nothing but rays() says so
        assert cost is None or r["total_cost"][0] == cost
        assert int(r["flows"][0:3].min()) >= (1 << 62) - 3
        assert to_numpy_verdicts(h.diagnose_on_host() if rays is HOST_RAYS else h.diagnose()) == [M.Verdict.Feasible]


def to_numpy_verdicts(d):
    return [int(v) for v in diag_rows(d)["verdict"]]


def test_optimal_although_unbounded_is_caught():
    check_the_hazard(HOST_SOLVE, HOST_RAYS)


def test_upper_none_and_costs_not_negative_take_one_round():
    t, a = small_case()
    u = uniform_of(t, O.RULE_BLOCK)
    u.run_on_host(cost=np.ascontiguousarray(np.abs(a["cost"])), supply=a["supply"])
    d = u.rays_on_host()
    st = u.ray_stats()
    assert np.all(d.verdict == Ray.Bounded) and not d.label.any() and not d.on_cycle.any()
    assert st["rounds"] == st["instances"] == t.count and st["frontier_nodes"] == t.count * t.n and st["cycle_arcs"] == 0, st


def check_by_bounds_between_neighbours(solve, rays):
    good, bad = problem(3, TRIANGLE, [0, 0, 0]), problem(3, [(0, 1, 3, 2, -1), (1, 2, 0, None, -1), (2, 0, 0, None, -1)], [0, 0, 0])
    flat = FlatNodes([good, bad, problem(3, [(0, 1, 0, None, 1)], [1, -1, 0])])
    h = flat.handle()
    solve(h, flat.arrays, O.GEQ)
    rows = check_answers(flat.problems, flat, rays(h), h.ray_stats())
    assert list(rows["verdict"]) == [Ray.Cycle, Ray.Bounds, Ray.Bounded] and h.ray_stats()["bounds"] == 1


def test_infeasible_by_its_bounds_between_two_that_are_not():
    check_by_bounds_between_neighbours(HOST_SOLVE, HOST_RAYS)


# ---- 3: long cycles
CYCLE_NODES = 300


def long_cycle(total, nodes=CYCLE_NODES, pad_to=None):
    """A directed cycle of `nodes` nodes numbered against the walk (v -> v - 1), every arc costing 1 but the one out of node 0, which makes
    the cycle cost `total`; a shipment of 1 from node 2 to node 1 so that the solve has something to do.  pad_to: isolated nodes appended."""
    n = nodes
    src = np.arange(n, dtype=np.int32)
    tgt = ((src - 1) % n).astype(np.int32)
    cost = np.ones(n, np.int64)
    cost[0] = total - (n - 1)
    supply = np.zeros(pad_to or n, np.int64)
    supply[2], supply[1] = 1, -1
    return O.Problem(pad_to or n, n, src, tgt, np.zeros(n, np.int64), np.full(n, O.INF_CAP, np.int64), cost, supply)


def check_long_cycles(solve, rays, nodes=CYCLE_NODES, pad_to=None):
    n = nodes
    extra = (pad_to or n) - n
    verdict, cost, arcs, _, _, h = one(long_cycle(-1, n, pad_to), O.GEQ, solve, rays)
    st = h.ray_stats()
    assert (verdict, cost, arcs) == (Ray.Cycle, -1, list(range(n))) and st["cycle_arcs"] == n
    # round 1 starts from every node; after it one label falls per round, the last in round k + 1 = n + 1
    assert st["rounds"] == n + 1 and st["frontier_nodes"] == n + extra + n and st["inc_entries"] == 2 * 2 * n + n * 4, st
    verdict, cost, arcs, labels, _, h = one(long_cycle(0, n, pad_to), O.GEQ, solve, rays)
    st = h.ray_stats()
    assert (verdict, cost, arcs) == (Ray.Bounded, 0, []) and labels[:n] == [-v for v in range(n)] and not any(labels[n:])
    assert st["rounds"] == n and st["frontier_nodes"] == n + extra + n - 1 and st["cycle_arcs"] == 0, st
    return st


def test_a_cycle_of_300_arcs_and_its_zero_cost_twin_on_the_host():
    check_long_cycles(HOST_SOLVE, HOST_RAYS)


# ---- 4: one graph, many instances: the uniform handle, and what the kept data say after every kind of solve call
RAY_GRAPH = (30, 90)          # m + n = 120: two strides of the arcs
RAY_VARIANTS = 24
BY_BOUNDS = 13


@functools.lru_cache(maxsize=None)
def ray_topology():
    """24 variants of one random graph of 30 nodes and 90 arcs: kinds and shares of uncapacitated arcs as the family's, variant 13
    infeasible by its bounds.  Asserted on the oracle's answers: both verdicts at least five times."""
    n, m = RAY_GRAPH
    rng = np.random.default_rng([R.SEED, 7])
    src, tgt = rng.integers(0, n, m).astype(np.int32), rng.integers(0, n, m).astype(np.int32)
    variants = []
    for k in range(RAY_VARIANTS):
        p = random_problem(np.random.default_rng([R.SEED, 7, k]), n, m, ("negative", "balanced", "negative", "excess")[k % 4], ties=k % 5 == 2, zero_capacity=False,
                           inf_fraction=(0.3, 0.6, 1.0, 1.0)[(k // 4) % 4], bound_infeasible=k == BY_BOUNDS)
        variants.append(on_topology(p, src, tgt))
    t = Topology(n, src, tgt, variants, [False] * RAY_VARIANTS)
    truth = [R.has_negative_cycle(p) for k, p in enumerate(variants) if k != BY_BOUNDS]
    assert sum(truth) >= 5 and len(truth) - sum(truth) >= 5, truth
    return t


def check_one_graph(solve, rays, rays_bare):
    t = ray_topology()
    a = t.arrays()
    flat = FlatNodes(t.variants)
    for shared in (False, True):
        ua, ra, problems = dict(a), dict(flat.arrays), t.variants
        if shared:                                                          # one cost row for all: a row with a cycle in most variants' capacities
            row = t.variants[2].cost
            ua["cost"], ra["cost"] = np.ascontiguousarray(row), np.ascontiguousarray(np.tile(row, t.count))
            problems = [O.Problem(p.n, p.m, p.src, p.tgt, p.lower, p.upper, row, p.supply) for p in t.variants]
        h, u = flat.handle(), uniform_of(t, O.RULE_BLOCK)
        solve(h, ra, O.GEQ)
        solve(u, ua, O.GEQ)
        dh, du = rays(h), rays(u)
        rh, ru = check_answers(problems, flat, dh, h.ray_stats(), shared), ray_rows(du)
        assert ru["on_cycle"].shape == (t.count, t.m) and ru["label"].shape == (t.count, t.n) and ru["verdict"].shape == (t.count,)
        assert set(ru["verdict"]) == {Ray.Bounded, Ray.Cycle, Ray.Bounds} and ru["verdict"][BY_BOUNDS] == Ray.Bounds
        assert_same_rays(dh, du, shared)
        assert same_counts(h.ray_stats(), u.ray_stats()), (h.ray_stats(), u.ray_stats())
        for arcs, labels in ((False, True), (True, False), (False, False)):
            bare = ray_rows(rays_bare(u, arcs, labels))
            assert (bare["on_cycle"] is None) == (not arcs) and (bare["label"] is None) == (not labels)
            for name in FIELDS:
                assert bare[name] is None or np.array_equal(bare[name], ru[name]), name
            assert same_counts(h.ray_stats(), u.ray_stats())                # without the rows the rounds still run


def test_one_graph_equals_the_uniform_batch_on_the_host():
    check_one_graph(HOST_SOLVE, HOST_RAYS, lambda h, arcs, labels: h.rays_on_host(arcs=arcs, labels=labels))


def check_kept_data(solve, resolve, resolve_data, solve_from, rays):
    """The answer follows the data the last solve call of any kind left"""
    arcs = lambda costs, cap: [(0, 1, 0, None, costs[0]), (1, 2, 0, cap, costs[1]), (2, 0, 0, None, costs[2]), (0, 2, 0, 9, 4)]
    make = lambda costs, cap=None: FlatNodes([problem(3, arcs(costs, cap), [2, 0, -2])])
    plain, cyclic, capped = make([1, 1, 1]), make([1, -3, 1]), make([1, -3, 1], 6)
    answer = lambda h, flat: int(check_answers(flat.problems, flat, rays(h), h.ray_stats())["verdict"][0])
    h = plain.handle()
    solve(h, plain.arrays, O.GEQ)
    assert answer(h, plain) == Ray.Bounded
    resolve(h, cyclic.arrays, O.GEQ)                                        # new costs create the cycle ...
    assert answer(h, cyclic) == Ray.Cycle
    resolve(h, plain.arrays, O.GEQ)                                         # ... and take it away again
    assert answer(h, plain) == Ray.Bounded
    resolve(h, cyclic.arrays, O.GEQ)
    resolve_data(h, capped.arrays, O.GEQ)                                   # a capacity on the cycle
    assert answer(h, capped) == Ray.Bounded
    resolve_data(h, cyclic.arrays, O.GEQ)
    assert answer(h, cyclic) == Ray.Cycle
    g = plain.handle()                                                      # from a given basis, on a handle that has never solved
    states = np.array([0, 0, 1, 1], np.int8)
    solve_from(g, states, cyclic.arrays, O.GEQ)
    assert answer(g, cyclic) == Ray.Cycle
    solve_from(g, states, plain.arrays, O.GEQ)
    assert answer(g, plain) == Ray.Bounded


def test_the_answer_follows_every_kind_of_solve_call_on_the_host():
    check_kept_data(HOST_SOLVE, lambda h, a, s: h.rerun_on_host(supply_type=s, **a), lambda h, a, s: h.rerun_data_on_host(supply_type=s, **a),
                    lambda h, states, a, s: h.run_from_on_host(states, supply_type=s, **a), HOST_RAYS)


def check_untouched(solve, resolve, rays, queries):
    """Bit for bit round a call: what the other queries read of the kept state, every other statistic, and a resolve() afterwards.
    queries: (cost_ranges, data_ranges, diagnose) of a handle."""
    t = ray_topology()
    a = t.arrays()
    new_cost = np.ascontiguousarray(a["cost"][::-1])
    others = lambda h: (h.stats(), h.range_stats(), h.data_range_stats(), h.diagnose_stats(), h.resolve_data_stats(), h.start_stats())
    strip = lambda s: {k: v for k, v in s.items() if not k.endswith("_ns") and not k.startswith("bytes_")}     # a query's first device call takes its table up
    for stype in (O.GEQ, O.LEQ):
        with_call, without = uniform_of(t, O.RULE_BLOCK), uniform_of(t, O.RULE_BLOCK)
        solve(with_call, a, stype)
        solve(without, a, stype)
        before = [query_rows(q(with_call)) for q in queries]
        stats = others(with_call)
        d = ray_rows(rays(with_call))
        assert set(d["verdict"]) == {Ray.Bounded, Ray.Cycle, Ray.Bounds}
        again = ray_rows(rays(with_call))
        for name in FIELDS:
            assert np.array_equal(d[name], again[name]), name
        assert others(with_call) == stats
        after = [query_rows(q(with_call)) for q in queries]
        for x, y in zip(before, after):
            for name in x:
                assert np.array_equal(x[name], y[name]), name
        assert [strip(s) for s in others(with_call)] == [strip(s) for s in stats]        # the second calls count what the first counted
        ra, rb = to_numpy(resolve(with_call, dict(a, cost=new_cost), stype)), to_numpy(resolve(without, dict(a, cost=new_cost), stype))
        for name in ra:
            assert np.array_equal(ra[name], rb[name]), (stype, name)
        assert strip(with_call.stats()) == strip(without.stats())


def test_the_kept_state_is_untouched_on_the_host():
    check_untouched(HOST_SOLVE, lambda h, a, stype: h.rerun_on_host(supply_type=stype, **a), HOST_RAYS,
                    (lambda h: h.cost_ranges_on_host(), lambda h: h.data_ranges_on_host(), lambda h: h.diagnose_on_host()))


# ---- 5: the global tier's instances (run here with one lane; test_rays_gpu.py runs them in place in global memory)
@functools.lru_cache(maxsize=None)
def padded_family():
    """The six largest family instances of each verdict with isolated zero-supply nodes appended up to 4 500, so that the workspace fits
    no LDS limit: node sweeps of 71 strides; k stays at most 60, so the rounds stay few."""
    picked = {True: [], False: []}
    for (p, stype), cyclic in reversed(list(zip(R.ray_family(), family_truth()))):
        if len(picked[cyclic]) < 6:
            picked[cyclic].append((p, stype))
    out = []
    for p, stype in picked[True] + picked[False]:
        q = O.Problem(PADDED_NODES, p.m, p.src, p.tgt, p.lower, p.upper, p.cost, np.concatenate([p.supply, np.zeros(PADDED_NODES - p.n, np.int64)]))
        assert footprint_of(q, stype) > max(LDS_LIMITS) and PADDED_NODES > 70 * 64
        out.append(q)
    assert len(out) == 12 and sum(R.has_negative_cycle(q) for q in out) == 6 and max(len(R.jacobi_frontiers(q)) for q in out) <= 61
    return tuple(out)


@functools.lru_cache(maxsize=None)
def padded_topology():
    """Three variants of ray_topology() padded the same way, for one uniform handle in the global tier: the first with a negative cycle,
    the first without and the one that is infeasible by its bounds."""
    t = ray_topology()
    cyclic = [k != BY_BOUNDS and R.has_negative_cycle(p) for k, p in enumerate(t.variants)]
    keep = (cyclic.index(True), min(k for k in range(t.count) if not cyclic[k] and k != BY_BOUNDS), BY_BOUNDS)
    variants = [O.Problem(PADDED_NODES, p.m, p.src, p.tgt, p.lower, p.upper, p.cost, np.concatenate([p.supply, np.zeros(PADDED_NODES - p.n, np.int64)]))
                for p in (t.variants[k] for k in keep)]
    padded = Topology(PADDED_NODES, t.src, t.tgt, variants, [False] * len(variants))
    assert stride_of(padded) > max(LDS_LIMITS)              # a uniform handle is one class: its stride decides the tier
    return padded


def check_padded(solve, rays, stats_check):
    """-> the ragged handle and its answers; the uniform handle and the statistics of its call"""
    flat = FlatNodes(padded_family())
    h = flat.handle()
    solve(h, flat.arrays, O.GEQ)
    d = rays(h)
    rows = check_answers(flat.problems, flat, d, h.ray_stats(), "padded")
    assert {Ray.Cycle, Ray.Bounded} == set(rows["verdict"])
    stats_check(h.ray_stats())
    # one uniform handle of the same tier: bit for bit what the same handle's hook says of the same state
    t = padded_topology()
    u = uniform_of(t, O.RULE_BLOCK)
    solve(u, t.arrays(), O.GEQ)
    du = rays(u)
    st = u.ray_stats()
    assert list(ray_rows(du)["verdict"]) == [Ray.Cycle, Ray.Bounded, Ray.Bounds] and ray_rows(du)["label"].shape == (t.count, PADDED_NODES)
    assert_same_rays(du, HOST_RAYS(u), "padded, uniform")
    assert st["instances"] == t.count and same_counts(st, u.ray_stats()), (st, u.ray_stats())
    return h, d, u, st


def test_padded_instances_on_the_host():
    check_padded(HOST_SOLVE, HOST_RAYS, host_stats)


# ---- 6: the contract
def rays_io(cls, memory=L.MEM_HOST, **arrays):
    io = cls()
    io.memory = memory
    for name, a in arrays.items():
        setattr(io, name, a.ctypes.data)
    return io


def check_contract(solve, name, host_only):
    lib = L.lib()
    t = ray_topology()
    a = t.arrays()
    flat = FlatNodes(t.variants)
    for handle, io_cls, arrays in ((uniform_of(t, O.RULE_BLOCK), L.UBatchRaysIo, a), (flat.handle(), L.RBatchRaysIo, flat.arrays)):
        call = getattr(lib, f"{handle._PREFIX}_{name}")
        out = dict(verdict=np.full(t.count, 7, np.int32), cycle_cost=np.full(t.count, 7, np.int64), cycle_length=np.full(t.count, 7, np.int32),
                   on_cycle=np.full(t.count * t.m, 7, np.int8), label=np.full(t.count * t.n, 7, np.int64))
        untouched = lambda: all(np.all(v == 7) for v in out.values())
        assert call(handle._h, C.byref(rays_io(io_cls, **out))) == L.ERR_STATE and untouched()
        solve(handle, arrays)
        assert call(handle._h, None) == L.ERR_INVALID and call(None, C.byref(rays_io(io_cls, **out))) == L.ERR_INVALID
        assert call(handle._h, C.byref(rays_io(io_cls, memory=5, **out))) == L.ERR_INVALID
        if host_only:
            assert call(handle._h, C.byref(rays_io(io_cls, memory=L.MEM_DEVICE, **out))) == L.ERR_INVALID
        assert untouched()
        assert call(handle._h, C.byref(rays_io(io_cls, **out))) == 0
        full = {k: v.copy() for k, v in out.items()}
        assert set(full["verdict"]) == {Ray.Bounded, Ray.Cycle, Ray.Bounds} and full["on_cycle"].any() and full["label"].any() and full["cycle_cost"].any()
        stats = L.UBatchRaysStats()
        getter = getattr(lib, f"{handle._PREFIX}_get_rays_stats")
        assert getter(handle._h, C.byref(stats)) == 0 and stats.cycle == np.sum(full["verdict"] == Ray.Cycle) > 0 and stats.rounds > 0
        counts = stats.as_dict()
        for present in ((), ("verdict",), ("cycle_cost", "cycle_length"), ("on_cycle",), ("label",), ("verdict", "label")):
            part = {k: np.full_like(v, 7) for k, v in out.items() if k in present}
            assert call(handle._h, C.byref(rays_io(io_cls, **part))) == 0, present
            for k, v in part.items():
                assert np.array_equal(v, full[k]), (present, k)
            assert getter(handle._h, C.byref(stats)) == 0 and same_counts(stats.as_dict(), counts), present
        assert getter(handle._h, None) == L.ERR_INVALID and getter(None, C.byref(stats)) == L.ERR_INVALID


def test_contract_on_the_host():
    check_contract(lambda h, a: h.run_on_host(**a), "rays_on_host", True)


def test_rays_before_a_solve_is_refused_and_tensors_by_the_hook():
    t = ray_topology()
    for h in (uniform_of(t, O.RULE_BLOCK), FlatNodes(t.variants).handle()):
        for call in (h.rays_on_host, lambda: h.rays(tensors=False)):
            with pytest.raises(M.McfError) as ei:
                call()
            assert ei.value.code == L.ERR_STATE
        assert h.ray_stats() == {name: 0 for name, _ in L.UBatchRaysStats._fields_}


def test_without_a_device_the_handle_is_unchanged(have_gpu):
    # no GPU: device 0 is missing; with one, device 99 is
    t = ray_topology()
    a = t.arrays()
    u = uniform_of(t, O.RULE_BLOCK, device=99 if have_gpu else 0)
    r = u.run_on_host(**a)
    before, stats, ray_stats = u.rays_on_host(), u.stats(), u.ray_stats()
    with pytest.raises(M.McfError) as ei:
        u.rays(tensors=False)
    assert ei.value.code == L.ERR_NO_DEVICE
    assert u.stats() == stats and u.ray_stats() == ray_stats
    assert_same_rays(u.rays_on_host(), before)
    again = u.rerun_on_host(**a)
    assert np.array_equal(again.flows, r.flows) and np.array_equal(again.status, r.status)


def test_rays_structs_have_the_layout_of_the_header(tmp_path):
    src = tmp_path / "sz.c"
    io_fields = ("memory", "verdict", "cycle_cost", "cycle_length", "on_cycle", "label")
    s_fields = tuple(name for name, _ in L.UBatchRaysStats._fields_)
    line = lambda struct, fields: 'printf("%zu' + " %zu" * len(fields) + '\\n", sizeof(%s)' % struct + "".join(", offsetof(%s, %s)" % (struct, f) for f in fields) + ");"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void){' % os.path.join(ROOT, "include", "mcf_hip.h")
                   + line("mcf_ubatch_rays_io", io_fields) + line("mcf_rbatch_rays_io", io_fields) + line("mcf_ubatch_rays_stats", s_fields)
                   + 'printf("%d %d %d %d\\n", MCF_RAY_NONE, MCF_RAY_BOUNDED, MCF_RAY_CYCLE, MCF_RAY_BOUNDS);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", str(src), "-o", str(exe)])
    got = [[int(x) for x in row.split()] for row in subprocess.check_output([str(exe)]).decode().splitlines()]
    for cls, fields, row in zip((L.UBatchRaysIo, L.RBatchRaysIo, L.UBatchRaysStats), (io_fields, io_fields, s_fields), got):
        assert row == [C.sizeof(cls)] + [getattr(cls, f).offset for f in fields], cls
    assert got[3] == [Ray.NoVerdict, Ray.Bounded, Ray.Cycle, Ray.Bounds] == [0, 1, 2, 3]


def test_the_ray_oracle_on_answers_it_must_refuse():
    """check_cycle and check_labels are the judges: a wrong sum, a capacitated arc, two cycles, a path, labels that break an arc"""
    p = problem(4, [(0, 1, 0, None, -2), (1, 0, 0, None, 1), (2, 3, 0, None, -1), (3, 2, 0, None, -1), (1, 2, 0, 5, -9), (0, 0, 0, None, 3)], [0] * 4)
    R.check_cycle(p, [1, 1, 0, 0, 0, 0], -1, 2)
    R.check_cycle(p, [0, 0, 1, 1, 0, 0], -2, 2)
    for marks, cost, length in (([1, 1, 0, 0, 0, 0], -2, 2), ([1, 1, 0, 0, 0, 0], -1, 3), ([1, 1, 1, 1, 0, 0], -3, 4), ([1, 0, 0, 0, 0, 0], -2, 1), ([0, 0, 0, 0, 0, 1], 3, 1),
                               ([0, 0, 0, 0, 0, 0], 0, 0), ([1, 0, 0, 0, 1, 0], -11, 2)):
        with pytest.raises(AssertionError):
            R.check_cycle(p, marks, cost, length)
    assert R.has_negative_cycle(p) and R.jacobi_rounds(p) is None
    q = problem(3, [(0, 1, 0, None, -2), (1, 2, 0, None, 1), (2, 0, 0, None, 1), (0, 2, 0, 4, -7)], [0] * 3)
    assert not R.has_negative_cycle(q) and R.jacobi_rounds(q) == 3 and R.jacobi_frontiers(q) == [3, 1, 1]
    R.check_labels(q, [0, -2, -1])
    R.check_labels(q, [5, 3, 4])
    for labels in ([0, 0, 0], [-1, -2, 0], [-1, -3, -1]):
        with pytest.raises(AssertionError):
            R.check_labels(q, labels)
