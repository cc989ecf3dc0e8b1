"""Re-solving placed batches with new supplies and bounds from the kept basis (mcf_ubatch_resolve_data / mcf_rbatch_resolve_data, DESIGN.md
3.14 "Re-solve with new data") without a GPU: the hooks run the device's own re-data step, its dual pivots and its fallback with one
lane on the CPU.

The reference for everything is the oracle's cold solve on the new data: status always, for Optimal the total cost and validate_solution
on the returned flows and potentials, and for every row that went cold -- by rule or by fallback -- the oracle's fresh solve bit for bit,
trace included.  test_redata_gpu.py imports the family and the checkers from here."""
import functools

import numpy as np
import pytest

import mincostflow_amd as M
from mincostflow_amd import _lib as L
from oracle import ns_oracle as O

from adversarial import random_problem
from test_batch_host import bound_infeasible
from test_batch_resolve_host import cold_reference, warm_after, with_cost
from test_ragged_host import Mix
from test_uniform_host import (ALL_RULES, KINDS, NOT_SOLVED, RESOLVE_PER, SEED, TRACE, Topology, answer_of, assert_row_matches_cold, on_topology,
                               resolve_family, step_costs, to_numpy, uniform_of)

STEPS = ("a", "b", "c", "d", "e", "f", "g")
DUAL_STEPS = ("a", "b", "c", "e")       # the old optimum violates the new data: dual pivots are forced
CUT = (0, 4, 7)                         # the variants whose cut step (f) makes infeasible; none of the "excess" kind
SURPLUS = (3, 9)                        # the balanced variants that step (g) gives a surplus: cold by rule
SMALL = (9, 54)                         # n, m of the graph with m + n = 63: every search is one stride of the wave, not a full one
PADDED_NODES = 4500                     # above the LDS tier whatever the arcs: 37 bytes per node alone exceed 160 KiB


@functools.lru_cache(maxsize=None)
def redata_family():
    """resolve_family() of test_uniform_host.py (65, 257 and 1000 search arcs, LEQ on the middle graph, 12 variants of finite, positive
    capacity with lower bounds, the last infeasible by its bounds) and one graph more with m + n = 63, drawn the same way: 9 nodes as the
    graph of 65 has, since family A's own graph of 63 search arcs has 10 arcs on 53 nodes and no feasible variant."""
    n, m = SMALL
    rng = np.random.default_rng([SEED, 5])
    src, tgt = rng.integers(0, n, m).astype(np.int32), rng.integers(0, n, m).astype(np.int32)
    variants = []
    for k in range(RESOLVE_PER):
        p = random_problem(np.random.default_rng([SEED, 5, k]), n, m, KINDS[k % 3], zero_capacity=False, inf_fraction=0.0, bound_infeasible=k == RESOLVE_PER - 1)
        variants.append(on_topology(p, src, tgt))
    return resolve_family() + ((Topology(n, src, tgt, variants, [False] * RESOLVE_PER), O.GEQ),)


def with_data(p, supply, lower, upper):
    return O.Problem(p.n, p.m, p.src, p.tgt, lower.astype(np.int64), upper.astype(np.int64), p.cost, supply.astype(np.int64))


def cut_off(p, rng):
    """Capacity 1 on every arc that leaves the node with the largest supply (self loops left alone), while that keeps what can leave it
    below its supply."""
    supply, lower, upper = p.supply, p.lower.copy(), p.upper.copy()
    for v in np.argsort(-supply, kind="stable"):
        out = np.flatnonzero((p.src == v) & (p.tgt != v))
        into = np.flatnonzero((p.tgt == v) & (p.src != v))
        if supply[v] > 0 and int((lower[out] + 1).sum()) - int(lower[into].sum()) < supply[v]:
            upper[out] = lower[out] + 1
            break
    return with_data(p, supply, lower, upper)


def next_data(p, name, k, rng, pool=None):
    """The problem after the step `name` of the chain; an arc whose upper bound lies below its lower bound keeps both.  pool: the nodes whose
    supplies steps b and g may redraw, by default every node."""
    supply, lower, upper = p.supply.copy(), p.lower.copy(), p.upper.copy()
    live = upper > lower
    cap = upper - lower
    if name == "a":                     # delta units from one supply node to one demand node
        pos, neg = np.flatnonzero(supply > 0), np.flatnonzero(supply < 0)
        if len(pos) and len(neg):
            delta = int(rng.integers(1, 4))
            supply[rng.choice(pos)] -= delta
            supply[rng.choice(neg)] += delta
    elif name == "b":                   # 5 % of the supplies redrawn, at least two, their sum kept
        nodes = np.arange(p.n) if pool is None else np.asarray(pool)
        hit = rng.random(len(nodes)) < 0.05
        hit[rng.choice(len(nodes), min(2, len(nodes)), replace=False)] = True
        at = nodes[np.flatnonzero(hit)]
        new = rng.integers(-8, 9, len(at))
        new[-1] += supply[at].sum() - new.sum()
        supply[at] = new
    elif name == "c":                   # capacities halved, rounded up
        upper = np.where(live, lower + (cap + 1) // 2, upper)
    elif name == "d":                   # capacities doubled
        upper = np.where(live, lower + 2 * cap, upper)
    elif name == "e":                   # lower bounds redrawn within the capacities
        drawn = np.where(rng.random(p.m) < 0.15, rng.integers(0, 4, p.m), 0)
        lower = np.where(live, np.minimum(drawn, upper - 1), lower)
    elif name == "f":                   # a cut below the supply behind it
        if k in CUT:
            return cut_off(p, rng)
    elif name == "g":                   # supplies redrawn as in b, in the variants SURPLUS with a surplus
        supply = next_data(p, "b", k, rng, pool).supply
        if k in SURPLUS:
            supply[rng.integers(0, p.n)] += 3
    return with_data(p, supply, lower, upper)


@functools.lru_cache(maxsize=None)
def chain():
    """per graph: (topology with the data of the first solve, (topology after step a, ... after step g)); every step starts from the data the
    one before it left."""
    out = []
    for j, (t, stype) in enumerate(redata_family()):
        steps, now = [], t
        for s, name in enumerate(STEPS):
            now = Topology(t.n, t.src, t.tgt, [next_data(p, name, k, np.random.default_rng([SEED, 6, j, k, s])) for k, p in enumerate(now.variants)], now.zero_capacity)
            steps.append(now)
        out.append((t, tuple(steps)))
    return tuple(out)


def expected_warm(before, p):
    """The warm rule of mcf_ubatch_resolve_data, from the oracle's answer to the data before and the new data alone."""
    return warm_after(before) and int(p.supply.sum()) == 0 and not bound_infeasible(p)


def violates(p, flow):
    net = np.zeros(p.n, np.int64)
    np.add.at(net, p.src, flow)
    np.subtract.at(net, p.tgt, flow)
    return bool(np.any(flow < p.lower) or np.any(flow > p.upper) or not np.array_equal(net, p.supply))


def references(tops, stype, rule):
    """per topology of a chain (the first solve's, then every step's): per variant (cold_reference(), answer_of())"""
    return tuple(tuple((cold_reference(p, stype, rule), answer_of(p, rule, stype)) for p in t.variants) for t in tops)


@functools.lru_cache(maxsize=None)
def chain_reference(rule):
    """per graph: references() of its chain.  The conditions on the family are asserted here, on the oracle's answers and the data alone:
    in every step at least 10 instances are Optimal and flow-conserving before and after (the warm candidates); in steps a, b, c and e at
    least 5 of those have an old optimum that violates the new data; Infeasible answers and answers with a surplus occur at least 3 times
    each; nothing is Unbounded."""
    out = tuple(references((t,) + steps, stype, rule) for (t, steps), (_, stype) in zip(chain(), redata_family()))
    infeasible = surplus = 0
    for s, name in enumerate(STEPS):
        candidates = forced = 0
        for (t, steps), refs in zip(chain(), out):
            for k, p in enumerate(steps[s].variants):
                (before, answer_before), (after, _) = refs[s][k], refs[s + 1][k]
                assert after[0] != O.UNBOUNDED
                infeasible += after[0] == O.INFEASIBLE and not bound_infeasible(p)
                surplus += after[2] is not None
                if expected_warm(before, p) and warm_after(after):
                    candidates += 1
                    forced += violates(p, answer_before[4])
        print(f"re-data chain, rule {rule}, step {name}: {candidates} warm candidates, {forced} with a violated old optimum")
        assert candidates >= 10 and (name not in DUAL_STEPS or forced >= 5), (name, candidates, forced)
    assert infeasible >= 3 and surplus >= 3, (infeasible, surplus)
    return out


def assert_row_is_fresh(r, k, answer, what):
    """Row k of to_numpy()'s rows is the oracle's fresh solve bit for bit."""
    st, pivots, tr, total, flows, potentials = answer
    assert r["status"][k] == st and r["pivots"][k] == pivots, (what, k, r["status"][k], st, r["pivots"][k], pivots)
    assert np.array_equal(r["trace"][k][:pivots], tr) and not r["trace"][k][pivots:].any(), (what, k)
    if st == O.OPTIMAL:
        assert r["total_cost"][k] == total and np.array_equal(r["flows"][k], flows) and np.array_equal(r["potentials"][k], potentials), (what, k)
    else:
        assert r["total_cost"][k] == 0 and not np.any(r["flows"][k]) and not np.any(r["potentials"][k]), (what, k)


def assert_step(r, problems, stype, before, after, stats, what):
    """One re-solve of `problems` against the oracle: every row as assert_row_matches_cold; rows cold by rule, and rows that cannot have
    stood warm, are the fresh solve's bit for bit; the statistics count what the warm rule predicts.  Returns (dual pivots, fallbacks)."""
    warm = [expected_warm(b[0], p) for b, p in zip(before, problems)]
    for k, (p, (ref, answer)) in enumerate(zip(problems, after)):
        assert_row_matches_cold(r, k, p, stype, ref, what)
        if not warm[k] or ref[0] != O.OPTIMAL:
            assert_row_is_fresh(r, k, answer, what)
        assert r["pivots"][k] <= TRACE
    must_fall_back = sum(w and ref[0] != O.OPTIMAL for w, (ref, _) in zip(warm, after))
    assert stats["warm_instances"] == sum(warm) and stats["cold_instances"] == len(warm) - sum(warm) and stats["untouched_instances"] == 0, (what, stats, sum(warm))
    assert must_fall_back <= stats["fallback_instances"] <= sum(warm), (what, stats)
    assert stats["dual_pivots"] >= 0 and stats["primal_pivots"] >= 0 and stats["dual_pivots"] + stats["primal_pivots"] >= int(r["pivots"].sum()), (what, stats)
    return stats["dual_pivots"], stats["fallback_instances"]


def assert_chain_floors(dual, fallback, what):
    assert all(dual[name] > 0 for name in DUAL_STEPS) and fallback["f"] > 0, (what, dual, fallback)


# ---- 1: the chain
def check_chain(first, again, rule, **kw):
    """first(u, arrays, stype), again(u, arrays, stype, **kw) -> result: a solve, then the seven steps as re-solves with new data."""
    dual, fallback = dict.fromkeys(STEPS, 0), dict.fromkeys(STEPS, 0)
    for j, (((t, steps), (_, stype)), refs) in enumerate(zip(zip(chain(), redata_family()), chain_reference(rule))):
        u = uniform_of(t, rule, **kw)
        first(u, t.arrays(), stype)
        for s, name in enumerate(STEPS):
            r = to_numpy(again(u, steps[s].arrays(), stype))
            d, f = assert_step(r, steps[s].variants, stype, refs[s], refs[s + 1], u.resolve_data_stats(), f"graph {j}, step {name}")
            dual[name] += d
            fallback[name] += f
    print(f"rule {rule}: dual pivots per step {dual}, fallbacks per step {fallback}")
    assert_chain_floors(dual, fallback, rule)


HOST = (lambda u, a, stype: u.run_on_host(supply_type=stype, **a), lambda u, a, stype, **kw: u.rerun_data_on_host(supply_type=stype, **a, **kw))
RECOST_ON_HOST = lambda u, a, stype, **kw: u.rerun_on_host(supply_type=stype, **a, **kw)


@pytest.mark.parametrize("rule", ALL_RULES)
def test_chain_on_the_host(rule):
    check_chain(*HOST, rule)


# ---- 2: unchanged data, and A -> B -> A -> B
def check_unchanged_data(first, again, rule):
    for j, (t, stype) in enumerate(redata_family()):
        a = t.arrays()
        u = uniform_of(t, rule)
        before = to_numpy(first(u, a, stype))
        after = to_numpy(again(u, a, stype))
        warm = np.array([expected_warm(cold_reference(p, stype, rule), p) for p in t.variants])
        assert warm.sum() >= 2 and not warm.all()
        st = u.resolve_data_stats()
        assert st["warm_instances"] == warm.sum() and st["fallback_instances"] == 0 and st["dual_pivots"] == 0, st
        assert not after["pivots"][warm].any() and not after["trace"][warm].any()           # the recomputed tree flows are the kept ones: nothing is violated
        assert np.array_equal(after["pivots"][~warm], before["pivots"][~warm]) and np.array_equal(after["trace"][~warm], before["trace"][~warm])
        for name in ("status", "total_cost", "flows", "potentials"):
            assert np.array_equal(after[name], before[name]), (j, name)


@pytest.mark.parametrize("rule", ALL_RULES)
def test_unchanged_data_need_no_pivot_on_the_host(rule):
    check_unchanged_data(*HOST, rule)


def check_back_and_forth(first, again, rule, **kw):
    """A -> B -> A -> B with B = the data after steps a to c: every visit answers as the oracle does, the second round as the first."""
    for j, (((t, steps), (_, stype)), refs) in enumerate(zip(zip(chain(), redata_family()), chain_reference(rule))):
        u = uniform_of(t, rule, **kw)
        first(u, t.arrays(), stype)
        seen = {}
        for visit, s in enumerate((3, 0, 3, 0)):                # indices into (t,) + steps
            top = ((t,) + steps)[s]
            r = to_numpy(again(u, top.arrays(), stype))
            for k, p in enumerate(top.variants):
                assert_row_matches_cold(r, k, p, stype, refs[s][k][0], f"graph {j}, visit {visit}")
            if s in seen:
                assert np.array_equal(r["status"], seen[s]["status"]) and np.array_equal(r["total_cost"], seen[s]["total_cost"]), (j, visit)
            seen[s] = r


def test_back_and_forth_on_the_host():
    check_back_and_forth(*HOST, O.RULE_BLOCK)


# ---- 3: the mask
def check_changed_mask(first, again, rule, **kw):
    """Rows the mask leaves out keep their last outputs and their state; the marked ones equal an unmasked re-solve's."""
    j = 1
    (t, steps), (_, stype) = chain()[j], redata_family()[j]
    a, new = t.arrays(), steps[2].arrays()
    mask = np.arange(t.count) % 3 != 1
    u = uniform_of(t, rule, **kw)
    before = to_numpy(first(u, a, stype))
    masked = to_numpy(again(u, new, stype, changed=mask))
    assert u.resolve_data_stats()["untouched_instances"] == (~mask).sum()
    v = uniform_of(t, rule, **kw)
    first(v, a, stype)
    whole = to_numpy(again(v, new, stype))
    for name in before:
        assert np.array_equal(masked[name][~mask], before[name][~mask]), name
        assert np.array_equal(masked[name][mask], whole[name][mask]), name
    assert not np.array_equal(whole["total_cost"][~mask], before["total_cost"][~mask])
    # the left-out rows go on from their own last state: marked alone now, with their first data again -> 0 pivots where warm
    back = to_numpy(again(u, a, stype, changed=~mask))
    assert np.array_equal(back["total_cost"][~mask], before["total_cost"][~mask]) and np.array_equal(back["total_cost"][mask], masked["total_cost"][mask])
    warm = np.array([expected_warm(cold_reference(p, stype, rule), p) for p in t.variants])
    assert (warm & ~mask).any() and not back["pivots"][warm & ~mask].any()
    assert u.stats()["total_pivots"] == back["pivots"][~mask].sum()


def test_changed_mask_on_the_host():
    check_changed_mask(*HOST, O.RULE_BLOCK)


# ---- 4: mixed with re-solves with new costs
def check_mixed_with_new_costs(first, again, recost, rule, graphs=None, **kw):
    """new costs, then new data under those costs, then new costs under those data: each against the oracle's cold solve of what holds then.
    graphs: ((topology, its steps), supply type) per graph, by default the chain's."""
    graphs = tuple((c, stype) for c, (_, stype) in zip(chain(), redata_family())) if graphs is None else graphs
    for j, ((t, steps), stype) in enumerate(graphs):
        u = uniform_of(t, rule, **kw)
        first(u, t.arrays(), stype)
        cost_1, cost_2, data = step_costs(t, j, 1), step_costs(t, j, 0), steps[1]
        calls = ((recost, t, cost_1), (again, data, cost_1), (recost, data, cost_2))
        for c, (call, top, cost) in enumerate(calls):
            r = to_numpy(call(u, dict(top.arrays(), cost=cost), stype))
            for k, p in enumerate(top.variants):
                q = with_cost(p, cost[k])
                assert_row_matches_cold(r, k, q, stype, cold_reference(q, stype, rule), f"graph {j}, call {c}")


def test_mixed_with_new_costs_on_the_host():
    check_mixed_with_new_costs(*HOST, RECOST_ON_HOST, O.RULE_BLOCK)


# ---- 5: three graphs in one handle, one of them in the global tier
@functools.lru_cache(maxsize=None)
def padded_chain():
    """(mix of the first solve, (mix per step)): the graphs of 65 and 1000 search arcs and the small one, the last padded with isolated
    nodes of supply 0 to PADDED_NODES nodes; supply type GEQ for all (one call, one supply type)."""
    picked = [g for g, (_, stype) in enumerate(redata_family()) if stype == O.GEQ]
    assert len(picked) == 3

    def pad(t):
        def wide(p):
            return O.Problem(PADDED_NODES, p.m, p.src, p.tgt, p.lower, p.upper, p.cost, np.concatenate([p.supply, np.zeros(PADDED_NODES - p.n, np.int64)]))
        return Topology(PADDED_NODES, t.src, t.tgt, [wide(p) for p in t.variants], t.zero_capacity)

    def mix_of(tops):
        return Mix(tops[:-1] + [pad(tops[-1])])

    return mix_of([chain()[g][0] for g in picked]), tuple(mix_of([chain()[g][1][s] for g in picked]) for s in range(len(STEPS)))


@functools.lru_cache(maxsize=None)
def padded_reference(rule):
    base, steps = padded_chain()
    return tuple(tuple((cold_reference(p, O.GEQ, rule), answer_of(p, rule, O.GEQ)) for p in mix.problems()) for mix in (base,) + steps)


def check_padded_chain(first, again, rule, **kw):
    base, steps = padded_chain()
    refs = padded_reference(rule)
    h = base.handle(rule, **kw)
    first(h, base.arrays(), O.GEQ)
    dual, fallback = dict.fromkeys(STEPS, 0), dict.fromkeys(STEPS, 0)
    for s, name in enumerate(STEPS):
        r = to_numpy(steps[s].split(again(h, steps[s].arrays(), O.GEQ)))
        dual[name], fallback[name] = assert_step(r, steps[s].problems(), O.GEQ, refs[s], refs[s + 1], h.resolve_data_stats(), f"three graphs, step {name}")
    assert_chain_floors(dual, fallback, "three graphs")
    return h


def test_three_graphs_in_one_handle_on_the_host():
    check_padded_chain(*HOST, O.RULE_BLOCK)


# ---- 6: under a pivot limit
LIMIT = 5


def check_under_a_limit(first, again, rule, **kw):
    """With a limit of 5 pivots: a stopped instance reports Not Solved with zero rows, a finished one answers as the oracle does, and the
    next re-solve with new data starts every stopped one cold -- its row is then a fresh solve's under the same limit."""
    stopped_then_cold = 0
    for j, ((t, steps), (_, stype)) in enumerate(zip(chain(), redata_family())):
        u = uniform_of(t, rule, pivot_limit=LIMIT, **kw)
        r = to_numpy(first(u, t.arrays(), stype))
        for s in (0, 2):
            stopped = r["status"] == NOT_SOLVED
            top = steps[s]
            r = to_numpy(again(u, top.arrays(), stype))
            st = u.resolve_data_stats()
            assert st["cold_instances"] >= stopped.sum() and st["warm_instances"] <= (~stopped).sum(), (j, s, st)
            fresh = to_numpy(first(uniform_of(t, rule, pivot_limit=LIMIT, **kw), top.arrays(), stype))
            for k, p in enumerate(top.variants):
                if r["status"][k] == NOT_SOLVED:
                    assert r["pivots"][k] == LIMIT and r["total_cost"][k] == 0 and not r["flows"][k].any() and not r["potentials"][k].any(), (j, s, k)
                else:
                    assert_row_matches_cold(r, k, p, stype, cold_reference(p, stype, rule), f"graph {j}, step {s}, limit")
                if stopped[k]:
                    stopped_then_cold += 1
                    for name in r:
                        assert np.array_equal(r[name][k], fresh[name][k]), (j, s, k, name)
    assert stopped_then_cold >= 10, stopped_then_cold


def test_under_a_pivot_limit_on_the_host():
    check_under_a_limit(*HOST, O.RULE_BLOCK)


# ---- 7: refusals
def test_refusals_and_their_error_codes():
    t, stype = redata_family()[0]
    a = t.arrays()
    u = uniform_of(t, O.RULE_BLOCK)
    with pytest.raises(M.McfError) as e:
        u.rerun_data_on_host(supply_type=stype, **a)
    assert e.value.code == L.ERR_STATE
    with pytest.raises(M.McfError) as e:
        u.resolve_data(supply_type=stype, **a)
    assert e.value.code == L.ERR_STATE
    u.run_on_host(supply_type=stype, **a)
    other = O.LEQ if stype == O.GEQ else O.GEQ
    for call in (u.rerun_data_on_host, u.resolve_data):
        with pytest.raises(M.McfError) as e:
            call(supply_type=other, **a)
        assert e.value.code == L.ERR_INVALID and "supply type" in str(e.value)
    # bad arrays never reach the library
    with pytest.raises(ValueError):
        u.rerun_data_on_host(supply_type=stype, **dict(a, supply=a["supply"][:, :-1]))
    with pytest.raises(ValueError):
        u.rerun_data_on_host(supply_type=stype, **dict(a, upper=a["upper"].astype(np.int32)))
    with pytest.raises(ValueError):
        u.rerun_data_on_host(supply_type=stype, changed=np.ones(t.count + 1, bool), **a)
    # the handle is as it was: the same data again need no pivot where the instance is warm
    again = to_numpy(u.rerun_data_on_host(supply_type=stype, **a))
    assert u.resolve_data_stats()["dual_pivots"] == 0 and u.resolve_data_stats()["warm_instances"] >= 2
    assert np.array_equal(again["status"], to_numpy(uniform_of(t, O.RULE_BLOCK).run_on_host(supply_type=stype, **a))["status"])
    assert M.UniformBatch.resolve_data_stats is M.RaggedBatch.resolve_data_stats


def test_redata_stats_struct_has_the_layout_of_the_header(tmp_path):
    import ctypes as C
    import os
    import subprocess
    from test_batch_host import ROOT
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void){printf("%%zu %%zu %%zu\\n", sizeof(mcf_ubatch_redata_stats), '
                   'offsetof(mcf_ubatch_redata_stats, dual_pivots), offsetof(mcf_ubatch_redata_stats, kernel_ns));return 0;}\n' % os.path.join(ROOT, "include", "mcf_hip.h"))
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(L.UBatchRedataStats), L.UBatchRedataStats.dual_pivots.offset, L.UBatchRedataStats.kernel_ns.offset]
