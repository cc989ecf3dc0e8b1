"""GPU tests of the walks that take their run ends from the thread-break bitmap (thread_breaks.h) inside real solves: with relabelling forced
often, runs of consecutive ids, node lists and runs cut by a piece hand-over all reach the default engine, and the pivots stay the oracle's."""
import functools

import numpy as np
import pytest

import mincostflow_amd as M
from oracle import ns_oracle as O


@functools.lru_cache(maxsize=None)
def _case(n, m):
    g = M.netgen_like(13502460, n, m, 40, 40)
    p = O.Problem(g.node_count, g.arc_count, g.source, g.target, g.lower, g.upper, g.cost, g.supply)
    o = O.Oracle(p, O.SEM_CSHARP_OPT, O.RULE_BEST)
    st_o, tr_o = o.solve(trace_cap=1 << 20)
    assert st_o == O.OPTIMAL
    return g, p, o, np.asarray(tr_o, np.int32)


# 3 000 / 12 000: walks of 48 .. 3 000 nodes (node lists below 512, runs above); 9 000 / 27 000 adds walks long enough to be handed over
# in pieces, whose boundaries cut runs
@pytest.mark.gpu
@pytest.mark.parametrize("n,m", [(3000, 12000), (9000, 27000)])
def test_solve_with_frequent_relabelling_is_the_oracles(n, m, monkeypatch):
    monkeypatch.setenv("MCF_NS_RENUMBER", "0.5")
    g, p, o, tr_o = _case(n, m)
    ns = M.NetworkSimplex.from_problem(g).set_pivot_rule(M.PivotRule.BestEligible).enable_optimized_pivot(True).record_trace(1 << 20)
    assert ns.solve() == M.SolverStatus.Optimal
    tr = ns.trace()
    assert len(tr) == len(tr_o)
    assert np.array_equal(tr, tr_o), int(np.argmax(tr != tr_o))
    assert ns.get_total_cost() == o.total_cost
    assert np.array_equal(ns.flows(), o.flow()) and np.array_equal(ns.potentials(), o.potential())
    e = ns.get_metrics()["engine"]
    assert e["renumberings"] >= 5, e["renumberings"]
    assert ns.check_thread_breaks() == 0


@pytest.mark.gpu
def test_stepwise_pivots_on_the_device_keep_the_bitmap_current():
    """The stepwise path: the device searches (a raw engine with the default flags), mcf_ns_apply_pivot carries each pivot out.  A replayed first
    half with relabellings leaves a bitmap; from then on the entering arcs are the oracle's and the break check reports 0 between pivots."""
    g, p, o, tr_o = _case(3000, 12000)
    ns = M.NetworkSimplex(p.n, p.src, p.tgt).set_problem(p.lower, p.upper, p.cost, p.supply)
    assert ns.begin() != M.SolverStatus.Infeasible
    k = len(tr_o) // 2
    ns.replay(tr_o[:k], smaller_side=False, renumber_every=0.1)
    assert ns.replay_relabellings >= 10 and ns.check_thread_breaks() == 0
    it = ns.internal()
    eng = M.PivotEngine(p.n + 1, it["arc_capacity"], it["search_arc_num"], rule=M.PivotRule.BestEligible, optimized=True)
    eng.upload(it["source"], it["target"], it["cost"], it["state"], it["pi"])
    pi = it["pi"]
    for i in range(k, len(tr_o) + 1):
        found, arc, _ = eng.find_entering()
        if i == len(tr_o):
            assert not found
            break
        assert found and arc == tr_o[i], i
        assert not ns.apply_pivot(arc)
        assert ns.check_thread_breaks() == 0, i
        lp = ns.last_pivot()
        eng.patch_state(lp["state_arcs"], lp["state_values"])
        now = ns.internal()["pi"]
        moved = np.nonzero(now != pi)[0].astype(np.int32)
        if lp["sigma"] != 0:
            assert np.array_equal(np.sort(lp["nodes"]), moved), i
        if len(moved):
            eng.set_potential(moved, now[moved])
        pi = now
    assert ns.finish() == O.OPTIMAL
    assert ns.get_total_cost() == o.total_cost
    assert np.array_equal(ns.flows(), o.flow()) and np.array_equal(ns.potentials(), o.potential())
