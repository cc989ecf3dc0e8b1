"""The candidate cache's heap keeps only the touched arcs that can still win (candidate_cache.hip.h: INVARIANT, cand_admit_all): an arc whose
key is not below the list's threshold is not kept, unless a refresh is in flight, and every install sweeps the heap.  None of that may change
a pivot: whole solves against the oracle's trace, and an engine-level round against the oracle's scan."""
import numpy as np
import pytest

import mincostflow_amd as M
from oracle import ns_oracle as O

pytestmark = pytest.mark.gpu

EPOCH_NEAR_WRAP = 0xFFFFFF00 - 300

_cache = {}


def _oracle_run():
    """The instance and the oracle's solve of it: computed once, shared by the variants, left unchanged."""
    if not _cache:
        g = M.netgen_like(13502460, 3000, 12000, 50, 50)
        p = O.Problem(g.node_count, g.arc_count, g.source, g.target, g.lower, g.upper, g.cost, g.supply)
        o = O.Oracle(p, O.SEM_CSHARP_OPT, O.RULE_BEST)
        st_o, tr_o = o.solve(trace_cap=4_000_000)
        _cache.update(p=p, o=o, st=st_o, trace=tr_o)
    return _cache


@pytest.mark.parametrize("env", [pytest.param({}, id="default"), pytest.param({"MCF_HIP_CAND_HEAP_COMPACT": "1"}, id="sweep-above-1"),
                                 pytest.param({"MCF_HIP_CAND_EPOCH0": str(EPOCH_NEAR_WRAP)}, id="epoch-near-wrap")])
def test_filtered_heap_takes_the_oracles_pivots(env, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    r = _oracle_run()
    p = r["p"]
    ns = M.NetworkSimplex(p.n, p.src, p.tgt).set_problem(p.lower, p.upper, p.cost, p.supply)
    ns.set_pivot_rule(M.PivotRule.BestEligible).enable_optimized_pivot(True).set_device(0, 0, 0, 0).record_trace(4_000_000)
    st = ns.solve()
    assert st == r["st"] == O.OPTIMAL
    tr = ns.trace()
    assert np.array_equal(tr, r["trace"]), int(np.argmax(tr[: len(r["trace"])] != r["trace"][: len(tr)]))
    assert ns.get_total_cost() == r["o"].total_cost
    assert np.array_equal(ns.flows(), r["o"].flow()) and np.array_equal(ns.potentials(), r["o"].potential())
    e = ns.get_metrics()["engine"]
    print({k: e[k] for k in ("candidates", "host_decided", "async_refreshes", "heap_compactions", "resident_requests")})
    # without these the run proves nothing about the filter
    assert e["candidates"] == 1, e
    assert e["host_decided"] > 0, e
    assert e["async_refreshes"] > 0, e
    assert e["heap_compactions"] > 0, e


def test_engine_round_with_rising_thresholds():
    """300 searches on random arrays against the oracle's scan.  Every winner leaves (state 0), so keys are consumed and each list's threshold
    lies above the last one's; between searches 1-8 nodes move, never a big list, so refreshes stay asynchronous and arcs are touched while
    one is in flight."""
    rng = np.random.default_rng(29)
    m_s, n = 9001, 1200
    a = dict(src=rng.integers(0, n, m_s, dtype=np.int32), tgt=rng.integers(0, n, m_s, dtype=np.int32),
             cost=rng.integers(-50, 51, m_s, dtype=np.int64), state=rng.integers(-1, 2, m_s, dtype=np.int8),
             pi=rng.integers(-1000, 1, n, dtype=np.int64))
    eng = M.PivotEngine(n, m_s, m_s, rule=M.PivotRule.BestEligible, flags=0)
    eng.upload(a["src"], a["tgt"], a["cost"], a["state"], a["pi"])
    for it in range(300):
        want = O.scan_best(m_s, a["state"], a["cost"], a["src"], a["tgt"], a["pi"])
        assert eng.find_entering() == want, it
        assert want[0], it          # 9 001 random arcs do not run out of eligible ones in 300 searches
        a["state"][want[1]] = 0
        eng.patch_state([want[1]], [0])
        nodes = rng.choice(n, size=int(rng.integers(1, 9)), replace=False).astype(np.int32)
        sigma = int(rng.integers(-40, 41))
        a["pi"][nodes] += sigma
        eng.update_potential(nodes, sigma)
    st = eng.stats()
    print({k: st[k] for k in ("candidates", "host_decided", "async_refreshes", "heap_compactions", "resident_requests")})
    assert st["candidates"] == 1 and st["host_decided"] > 0 and st["async_refreshes"] > 0 and st["heap_compactions"] > 0, st
    assert np.array_equal(eng.download_pi(), a["pi"]) and np.array_equal(eng.download_state()[:m_s], a["state"][:m_s])
