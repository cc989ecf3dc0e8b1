"""CPU tests of the host driver's thread-break bitmap and of the run walker that reads it (thread_breaks.h): after the first relabelling every
walk of 48 nodes and more takes its run ends from one bit per node (set where Thread[a] != a + 1), which the re-hanging keeps current.  The
node counts put the root id n and the sentinel words before, on and behind a 64-bit word boundary.  No device involved."""
import functools

import numpy as np
import pytest

import mincostflow_amd as M
from oracle import ns_oracle as O

SIZES = [63, 64, 65, 127, 128, 129, 1000]


@functools.lru_cache(maxsize=None)
def _instance(n):
    """A NETGEN-like instance with n nodes and the oracle's Best Eligible run on it: (problem, entering arcs, oracle), computed once."""
    g = M.netgen_like(4200 + n, n, 4 * n, n // 10, n // 10)
    p = O.Problem(g.node_count, g.arc_count, g.source, g.target, g.lower, g.upper, g.cost, g.supply)
    o = O.Oracle(p, O.SEM_CSHARP, O.RULE_BEST)
    assert o.init()
    arcs = []
    while True:
        f, e = o.find_entering()
        if not f:
            break
        assert o.apply_pivot(e) != O.UNBOUNDED
        arcs.append(e)
    assert o.finish() == O.OPTIMAL and len(arcs) > n // 2
    return p, np.array(arcs, np.int32), o


def _solver(p):
    ns = M.NetworkSimplex(p.n, p.src, p.tgt).set_problem(p.lower, p.upper, p.cost, p.supply)
    assert ns.begin() != M.SolverStatus.Infeasible
    return ns


def _assert_equals_oracle(ns, o):
    it, oa = ns.internal(), o.internal_arrays()
    assert np.array_equal(it["state"][: o.all_arc_num], oa["state"][: o.all_arc_num])
    assert np.array_equal(it["pi"], oa["pi"])
    assert ns.finish() == O.OPTIMAL
    assert ns.get_total_cost() == o.total_cost
    assert np.array_equal(ns.flows(), o.flow()) and np.array_equal(ns.potentials(), o.potential())


@pytest.mark.parametrize("smaller_side", [False, True], ids=["subtree", "smaller-side"])
@pytest.mark.parametrize("renumber_every", [0.1, 1.0, 4.0])
@pytest.mark.parametrize("n", SIZES)
def test_replay_with_the_break_bitmap(n, renumber_every, smaller_side):
    """The oracle's pivot sequence through mcf_ns_replay, relabelled every 0.1, 1 and 4 n walked nodes: states, flows and potentials are the
    oracle's, and the bitmap that the last relabelling left (rebuilt for the caller's ids when they were restored) is current."""
    p, arcs, o = _instance(n)
    ns = _solver(p)
    ns.replay(arcs, smaller_side=smaller_side, renumber_every=renumber_every)
    assert ns.get_metrics()["iterations"] == len(arcs)
    if renumber_every < 1.0:
        assert ns.replay_relabellings >= 2
    assert ns.check_thread_breaks() == 0
    _assert_equals_oracle(ns, o)


@pytest.mark.parametrize("smaller_side", [False, True], ids=["subtree", "smaller-side"])
@pytest.mark.parametrize("n", SIZES)
def test_pivot_by_pivot_keeps_the_bitmap_current(n, smaller_side):
    """Pivot by pivot through mcf_ns_apply_pivot.  Without a relabelling there is no bitmap and nothing to report; a replayed stretch with
    relabellings leaves one (over the caller's ids again, so the thread list leaves the id order almost everywhere), and from then on every
    re-hanging has to keep it current: checked after every pivot, twice over (a second replayed stretch relabels again in between)."""
    p, arcs, o = _instance(n)
    ns = _solver(p)
    k = len(arcs)
    cuts = [k // 8, k // 4, k // 2, 5 * k // 8]
    for e in arcs[: cuts[0]]:
        assert not ns.apply_pivot(int(e))
        assert ns.check_thread_breaks() == 0
    ns.replay(arcs[cuts[0]: cuts[1]], smaller_side=smaller_side, renumber_every=0.1)
    assert ns.replay_relabellings >= 1 and ns.check_thread_breaks() == 0
    for e in arcs[cuts[1]: cuts[2]]:
        assert not ns.apply_pivot(int(e))
        assert ns.check_thread_breaks() == 0
    before = ns.replay_relabellings
    ns.replay(arcs[cuts[2]: cuts[3]], smaller_side=smaller_side, renumber_every=0.1)
    assert ns.replay_relabellings > before and ns.check_thread_breaks() == 0
    for e in arcs[cuts[3]:]:
        assert not ns.apply_pivot(int(e))
        assert ns.check_thread_breaks() == 0
    _assert_equals_oracle(ns, o)


@functools.lru_cache(maxsize=None)
def _big_instance():
    """3 000 nodes / 12 000 arcs, large enough for walks of 512 nodes and more (the run form): (problem, the oracle's Best Eligible trace)."""
    g = M.netgen_like(13502460, 3000, 12000, 40, 40)
    p = O.Problem(g.node_count, g.arc_count, g.source, g.target, g.lower, g.upper, g.cost, g.supply)
    st, trace = O.Oracle(p, O.SEM_CSHARP_OPT, O.RULE_BEST).solve(trace_cap=1 << 20)
    assert st == O.OPTIMAL
    return p, np.asarray(trace, np.int32)


@pytest.mark.parametrize("renumber_every", [0.1, 0.0], ids=["relabelled", "control"])
def test_last_pivot_lists_the_nodes_that_moved(renumber_every):
    """mcf_ns_last_pivot after a replayed first half (32 relabellings at renumber_every=0.1, so the second half's walks of 512 nodes and more
    are written down as runs of consecutive ids): after every pivot of the second half the returned list is exactly the set of nodes whose
    potential changed, and each of them changed by sigma.  The control never relabels (no bitmap, no runs)."""
    p, trace = _big_instance()
    ns = _solver(p)
    k = len(trace) // 2
    ns.replay(trace[:k], smaller_side=False, renumber_every=renumber_every)
    assert (ns.replay_relabellings >= 10) if renumber_every else (ns.replay_relabellings == 0)
    pi = ns.internal()["pi"]
    big = 0
    for i, e in enumerate(trace[k:]):
        assert not ns.apply_pivot(int(e))
        lp, now = ns.last_pivot(), ns.internal()["pi"]
        if lp["sigma"] != 0:
            changed = np.nonzero(now != pi)[0]
            assert lp["count"] == len(changed), i
            assert np.array_equal(np.sort(lp["nodes"]), changed), (i, len(changed))
            assert np.all(now[changed] - pi[changed] == lp["sigma"]), i
            big += len(changed) >= 512
        pi = now
    assert big >= 100, big
    assert ns.finish() == O.OPTIMAL
