"""LEMON's Candidate List and Altering List rules (PivotRule 3 / 4): the literal restatement (lemon_list_literal.py) against the golden
fixtures on the CPU, the public surface, and on the GPU the device primitive (mcf_engine_collect_eligible) against a numpy statement of
both stop rules and whole solves against the restatement, pivot for pivot."""
import numpy as np
import pytest

import mincostflow_amd as M
from mincostflow_amd import _lib as L
import lemon_list_literal as LL
from helpers import fixtures, load, validate_solution

RULES = [pytest.param(M.PivotRule.CandidateList, id="candidate"), pytest.param(M.PivotRule.AlteringList, id="altering")]


def _ns(p):
    if isinstance(p, M.Problem):               # generated instances
        return M.NetworkSimplex.from_problem(p)
    return M.NetworkSimplex(p.n, p.src, p.tgt).set_problem(p.lower, p.upper, p.cost, p.supply)


# ------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("name,path,want", fixtures(), ids=[f[0] for f in fixtures()])
def test_literal_rules_solve_every_fixture(name, path, want, rule):
    """The restatement, driven through begin / apply_pivot / finish, reaches Optimal with the .sol cost and a valid solution."""
    p = load(path)
    ns = _ns(p)
    st, trace, r = LL.solve_literal(ns, rule)
    assert st == M.SolverStatus.Optimal, (name, st)
    assert ns.get_total_cost() == want
    validate_solution(p, ns.flows(), ns.potentials())
    assert r.majors >= 1 and len(trace) > 0


def test_partial_sort_is_libstdcxx():
    """A hand-checked case of libstdc++'s heap-select + sort-heap with ties: heapq or sorted() would keep the first of equal keys in front."""
    key = {10: -5, 11: -7, 12: -5, 13: -7, 14: -1, 15: -7}
    a = [10, 11, 12, 13, 14, 15]
    LL.partial_sort(a, 0, 3, len(a), lambda l, r: key[l] < key[r])
    assert sorted(key[x] for x in a[:3]) == [-7, -7, -7]
    assert a == [15, 11, 13, 12, 14, 10]          # what g++'s std::partial_sort leaves


def test_set_list_pivot_rule_accepts_3_and_4_only():
    p = load("grid_2x2")
    ns = _ns(p)
    ns.set_list_pivot_rule(M.PivotRule.CandidateList)
    ns.set_list_pivot_rule(M.PivotRule.AlteringList)
    for bad in (-1, 0, 1, 2, 5):
        with pytest.raises(M.McfError) as ei:
            ns.set_list_pivot_rule(bad)
        assert ei.value.code == L.ERR_INVALID
    # set_pivot_rule keeps refusing the list rules (NS.cs:884) and replaces a list rule set before
    for r in (M.PivotRule.CandidateList, M.PivotRule.AlteringList):
        with pytest.raises(M.McfError) as ei:
            ns.set_pivot_rule(r)
        assert ei.value.code == L.ERR_INVALID
    ns.set_pivot_rule(M.PivotRule.BlockSearch)


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("shard", ["rccl", "host", "group"])
def test_list_rules_refuse_sharding_at_prepare(rule, shard):
    p = load("grid_2x2")
    ns = _ns(p).set_list_pivot_rule(rule)
    if shard == "rccl":
        ns.set_sharding(np.zeros(128, np.uint8), 0, 1)
    elif shard == "host":
        ns.set_sharding_host("/mcf_list_rule_test", 0, 1)
    else:
        ns.set_shard_group([0, 0])
    with pytest.raises(M.McfError) as ei:
        ns.prepare()
    assert ei.value.code == L.ERR_INVALID


@pytest.mark.parametrize("rule", RULES)
def test_list_rule_solve_without_a_device_fails_like_the_others(rule):
    # no GPU: device 0 is missing; with one, device 99 is
    ns = _ns(load("grid_2x2")).set_list_pivot_rule(rule).set_device(99 if M.device_count() > 0 else 0)
    with pytest.raises(M.McfError) as ei:
        ns.solve()
    assert ei.value.code == L.ERR_NO_DEVICE


def _collect_loop(src, tgt, cost, state, pi, m_s, next_arc, limit=0, B=0, h=0, s=0):
    """LEMON's major loops (ns.h:478-507, :583-610) arc by arc: (arcs, costs, end, scanned)."""
    out, cs, scanned = [], [], 0
    cnt, lim = B, h
    for k in range(m_s):
        e = (next_arc + k) % m_s
        scanned += 1
        c = int(state[e]) * (int(cost[e]) + int(pi[src[e]]) - int(pi[tgt[e]]))
        if c < 0:
            out.append(e); cs.append(c)
            if limit and len(out) == limit:
                return out, cs, e, scanned
        if not limit:
            cnt -= 1
            if cnt == 0:
                if s + len(out) > lim:
                    return out, cs, e, scanned
                lim, cnt = 0, B
    return out, cs, next_arc, scanned


def _collect_numpy(src, tgt, cost, state, pi, m_s, next_arc, limit=0, B=0, h=0, s=0):
    """The same as a statement about positions p = (arc - next_arc) mod m_s: FIRST_N stops at the limit-th eligible arc; BLOCKS after block 1
    if s + c1 > h, after block 2 if s + c1 > 0, else after the block of the first eligible position >= B; a stop beyond the cycle returns all."""
    arcs = (next_arc + np.arange(m_s, dtype=np.int64)) % m_s
    c = state[arcs].astype(np.int64) * (cost[arcs].astype(np.int64) + pi[src[arcs]].astype(np.int64) - pi[tgt[arcs]].astype(np.int64))
    elig = np.flatnonzero(c < 0)
    if limit:
        if len(elig) >= limit:
            sel = elig[:limit]
            return arcs[sel], c[sel], int(arcs[sel[-1]]), int(sel[-1]) + 1
        return arcs[elig], c[elig], next_arc, m_s
    c1 = int((elig < B).sum())
    beyond = elig[elig >= B]
    if s + c1 > h:
        p_end = B - 1
    elif s + c1 > 0:
        p_end = 2 * B - 1
    elif len(beyond):
        p_end = (int(beyond[0]) // B + 1) * B - 1
    else:
        p_end = 1 << 62
    p_lim = min(p_end, m_s - 1)
    sel = elig[elig <= p_lim]
    return arcs[sel], c[sel], int(arcs[p_end]) if p_end < m_s else next_arc, p_lim + 1


def _random_soa(rng, m_s, n, frac_eligible, width=64):
    big = 1 << 20 if width == 32 else 1 << 40
    src = rng.integers(0, n, m_s).astype(np.int32)
    tgt = rng.integers(0, n, m_s).astype(np.int32)
    pi = rng.integers(-big, big, n).astype(np.int64)
    state = rng.choice(np.array([-1, 1] if frac_eligible >= 1 else [-1, 0, 1], np.int8), m_s)
    # cost chosen so that c = state * (cost + pi[s] - pi[t]) has the wanted sign: eligible with probability frac_eligible
    base = pi[src] - pi[tgt]
    mag = rng.integers(1, 50, m_s)
    want_neg = rng.random(m_s) < frac_eligible
    sign = np.where(state == 0, 1, state).astype(np.int64)
    red = np.where(want_neg, -mag, mag) * sign          # state * red < 0 exactly when want_neg (state != 0)
    if frac_eligible < 1:
        red[(rng.random(m_s) < 0.05)] = 0               # some ties at zero
    cost = (red - base).astype(np.int64)
    return src, tgt, cost, state, pi


def _collect_cases():
    # (m_s, next_arc, limit, B, h, s): FIRST_N when limit > 0
    return [(1000, 0, 25, 0, 0, 0), (1000, 997, 25, 0, 0, 0), (1000, 500, 2000, 0, 0, 0), (37, 36, 5, 0, 0, 0),
            (1000, 0, 0, 31, 3, 0), (1000, 990, 0, 31, 3, 2), (1000, 977, 0, 31, 3, 0), (1000, 999, 0, 31, 3, 3),
            (25, 7, 0, 31, 3, 0), (25, 7, 0, 31, 3, 3), (1001, 400, 0, 100, 3, 0), (5000, 4990, 0, 70, 3, 0)]


@pytest.mark.parametrize("frac", [0.0, 0.02, 0.5, 1.0])
def test_numpy_statement_of_the_stop_rules_is_lemons_loop(frac):
    """Pins the numpy statement the GPU test uses to LEMON's loops, on the same cases."""
    rng = np.random.default_rng(int(frac * 100) + 5)
    for m_s, na, limit, B, h, s in _collect_cases():
        a = _random_soa(rng, m_s, 50, frac)
        x = _collect_loop(*a, m_s, na, limit, B, h, s)
        y = _collect_numpy(*a, m_s, na, limit, B, h, s)
        assert list(y[0]) == x[0] and list(y[1]) == x[1] and y[2:] == x[2:], (m_s, na, limit, B, h, s)


# ------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("width", [32, 64])
def test_collect_eligible_matches_the_stop_rules(width):
    rng = np.random.default_rng(width)
    cases = [(m_s, na, limit, B, h, s, frac) for frac in (0.0, 0.02, 0.5, 1.0) for (m_s, na, limit, B, h, s) in _collect_cases()]
    cases += [(2_000_003, 1_999_990, 300, 0, 0, 0, 0.0001), (2_000_003, 1_000_000, 0, 1414, 14, 0, 0.00001),
              (2_000_003, 5, 0, 1414, 14, 3, 0.001), (2_000_003, 77, 4000, 0, 0, 0, 0.001)]
    soa = {}
    for m_s, na, limit, B, h, s, frac in cases:
        n = 4000
        key = (m_s, frac)
        if key not in soa:
            a = _random_soa(rng, m_s, n, frac, width)
            eng = M.PivotEngine(n, m_s, m_s, rule=M.PivotRule.CandidateList if limit else M.PivotRule.AlteringList, int_width=width)
            eng.upload(*a)
            soa[key] = (a, eng)
        a, eng = soa[key]
        want = _collect_numpy(*a, m_s, na, limit, B, h, s)
        cap = limit if limit else h + B
        got = eng.collect_eligible(na, limit=limit, block_size=B, head_length=h, survivors=s, capacity=max(cap, len(want[0])))
        assert np.array_equal(got[0], want[0].astype(np.int32)), (m_s, na, limit, B, h, s, frac)
        assert np.array_equal(got[1], want[1]), (m_s, na, limit, B, h, s, frac)
        assert got[2:] == want[2:], (m_s, na, limit, B, h, s, frac, got[2:], want[2:])


@pytest.mark.gpu
def test_collect_applies_queued_patches_of_several_pivots_in_order():
    """Host-answered pivots queue their state writes and potential lists (a node repeated across them) before the next device call."""
    rng = np.random.default_rng(3)
    m_s, n = 20000, 3000
    a = list(_random_soa(rng, m_s, n, 0.05))
    eng = M.PivotEngine(n, m_s, m_s, rule=M.PivotRule.AlteringList, int_width=64)
    eng.upload(*a)
    src, tgt, cost, state, pi = a
    for rnd in range(6):
        for _ in range(int(rng.integers(1, 40))):           # many "pivots" without a device call
            arcs = rng.choice(m_s, size=2, replace=False).astype(np.int32)
            vals = rng.integers(-1, 2, 2).astype(np.int8)
            state[arcs] = vals
            eng.patch_state(arcs, vals)
            nodes = rng.choice(n, size=int(rng.integers(1, 300)), replace=False).astype(np.int32)
            sigma = int(rng.integers(-40, 41))
            pi[nodes] += sigma
            eng.shift_potential(nodes, pi[nodes].copy(), sigma)
        na = int(rng.integers(0, m_s))
        want = _collect_numpy(src, tgt, cost, state, pi, m_s, na, 0, 141, 3, 0)
        got = eng.collect_eligible(na, block_size=141, head_length=3, survivors=0, capacity=m_s)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2:] == want[2:], rnd
    assert np.array_equal(eng.download_pi(), pi)
    assert np.array_equal(eng.download_state()[:m_s], state)
    with pytest.raises(M.McfError) as ei:
        eng.find_entering()
    assert ei.value.code == L.ERR_STATE


def _device_solve(p, rule, supply_type=M.SupplyType.Geq, int_width=0, share=0):
    ns = _ns(p).set_supply_type(supply_type).set_list_pivot_rule(rule).set_device(0, int_width, 0, 0).record_trace(4 << 20)
    if share:
        ns.set_device_share(share)
    st = ns.solve()
    return ns, st


def _check_against_literal(p, rule, supply_type=M.SupplyType.Geq, int_width=0, share=0):
    ns, st = _device_solve(p, rule, supply_type, int_width, share)
    ref = _ns(p).set_supply_type(supply_type)
    st_r, tr_r, r = LL.solve_literal(ref, rule)
    assert st == st_r
    assert np.array_equal(ns.trace(), tr_r)
    ls = ns.list_rule_stats()
    assert ls["rule"] == rule and ls["searches"] == ls["major_scans"] + ls["host_answered"]
    assert ls["searches"] == len(tr_r) + (0 if st == M.SolverStatus.Unbounded else 1)      # the last search found nothing
    assert ls["major_scans"] == r.majors and ls["host_answered"] == r.minors
    if st == M.SolverStatus.Optimal:
        assert ns.get_total_cost() == ref.get_total_cost()
        assert np.array_equal(ns.flows(), ref.flows()) and np.array_equal(ns.potentials(), ref.potentials())
        assert ns.validate()["valid"] == 1
        assert ns.check_reduced_costs() == 0
    return ns


@pytest.mark.gpu
@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("name", ["assignment_50x50", "circulation_100_0_10", "AURV19V6", "netgen_8_10a", "transport_400x300", "grid_5x5",
                                  "SimpleProblemIllustration2NonSparse"])
def test_device_solve_is_the_literal_rule_pivot_for_pivot(name, rule):
    _check_against_literal(load(name), rule)


@pytest.mark.gpu
@pytest.mark.parametrize("rule", RULES)
def test_device_solve_on_generated_instances(rule):
    g = M.netgen_like(13502460, 10_000, 30_000, 100, 100)
    ns = _check_against_literal(g, rule)
    m = ns.get_metrics()
    assert m["iterations"] == len(ns.trace()) and m["total_arcs_checked"] == 0
    _check_against_literal(M.assignment(5, 100, 1, 10), rule)                   # tie-heavy: costs 1 .. 10
    _check_against_literal(M.netgen_like(77, 2000, 8000, 40, 40), rule, int_width=32)
    _check_against_literal(M.netgen_like(78, 3000, 9000, 40, 40), rule, share=32)
    _check_against_literal(M.netgen_like(79, 1500, 6000, 30, 30), rule, supply_type=M.SupplyType.Leq)    # balanced, LEQ start basis
