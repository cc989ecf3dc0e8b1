"""The batch solver on the MI355X (mcf_batch_solve): one workgroup per instance, whole pivots on the device.

Every comparison is exact: status, pivot count, the whole entering-arc trace, and for optimal instances cost, flows and potentials.
References: the CPU oracle in SEM_CSHARP (auto-configured Block Search, see test_batch_host.py), mcf_batch_run_on_host, and
mcf_ns_solve with the same rule and enable_optimized_pivot(False).  Device time of the whole file on an MI355X: see DESIGN.md 3.14."""
import numpy as np
import pytest

import mincostflow_amd as M
from oracle import ns_oracle as O

from helpers import fixtures, load
from test_batch_host import (LDS_LIMITS, RULES, assert_equals_oracle, assert_fuzz_equals_oracle, bound_infeasible, check_mixed_batch,
                             check_nothing_to_run, check_padded_fuzz, check_short_and_absent_traces, footprint_of, fuzz_cases,
                             fuzz_reference, fuzz_solver, generated, ladder, mixed_cases, oracle_of, padded_fuzz)

pytestmark = pytest.mark.gpu


def assert_equals_single_solve(b, i, p, rule, what=""):
    ns = M.NetworkSimplex(p.n, p.src, p.tgt).set_problem(p.lower, p.upper, p.cost, p.supply)
    ns.set_pivot_rule(RULES[rule]).enable_optimized_pivot(False).record_trace(1 << 18)
    st = ns.solve()
    assert b.status(i) == st, what
    assert np.array_equal(b.trace(i), ns.trace()), what
    if st == M.SolverStatus.Optimal:
        assert b.total_cost(i) == ns.get_total_cost(), what
        assert np.array_equal(b.flows(i), ns.flows()) and np.array_equal(b.potentials(i), ns.potentials()), what


def assert_same_results(a, b, count):
    for i in range(count):
        assert a.status(i) == b.status(i) and a.pivots(i) == b.pivots(i), i
        assert np.array_equal(a.trace(i), b.trace(i)), i
        if a.status(i) == M.SolverStatus.Optimal:
            assert np.array_equal(a.flows(i), b.flows(i)) and np.array_equal(a.potentials(i), b.potentials(i)), i


# ---- 7
@pytest.mark.parametrize("rule", [O.RULE_BLOCK, O.RULE_BEST, O.RULE_FIRST])
def test_every_small_fixture_in_one_batch(rule):
    problems = [(name, load(path)) for name, path, _ in fixtures()]
    problems = [(name, p) for name, p in problems if p.m <= 8192]
    assert len(problems) == 34
    b = M.BatchSolver(rule=RULES[rule], record_trace=1 << 15)
    for _, p in problems:
        b.add(p)
    b.solve()
    st = b.stats()
    print(f"rule {rule}: {st}")
    assert st["instances"] == 34 and st["lds_instances"] >= 1 and st["global_instances"] >= 1 and st["launches"] >= 1
    assert st["lds_instances"] + st["global_instances"] == 34
    for i, (name, p) in enumerate(problems):
        o, st_o, tr = oracle_of(p, rule)
        assert st_o == O.OPTIMAL
        assert_equals_oracle(b, i, o, st_o, tr, name)
        assert_equals_single_solve(b, i, p, rule, name)


# ---- 8
def test_large_instances_run_in_place_and_in_slices():
    names = ["AURV19V6", "netgen_8_13a"]
    problems = [load(n) for n in names]
    b = M.BatchSolver(rule=M.PivotRule.BlockSearch, record_trace=1 << 17, pivots_per_launch=1000)
    for p in problems:
        b.add(p)
    b.solve()
    st = b.stats()
    print(st)
    assert st["global_instances"] == 2 and st["lds_instances"] == 0
    assert st["launches"] > 1 and st["launches"] >= max(b.pivots(0), b.pivots(1)) // 1000
    for i, p in enumerate(problems):
        o, st_o, tr = oracle_of(p, O.RULE_BLOCK)
        assert st_o == O.OPTIMAL
        assert_equals_oracle(b, i, o, st_o, tr, names[i])
        assert_equals_single_solve(b, i, p, O.RULE_BLOCK, names[i])


# ---- 9
def test_a_thousand_generated_instances():
    problems = [generated(seed) for seed in range(1, 1025)]
    dev = M.BatchSolver(record_trace=2048)
    host = M.BatchSolver(record_trace=2048)
    for p in problems:
        dev.add(p)
        host.add(p)
    dev.solve()
    host.run_on_host()
    st = dev.stats()
    print(st, f"{st['kernel_ns'] / max(st['total_pivots'], 1):.1f} ns of launch time per pivot of the batch")
    assert st["lds_instances"] == 1024 and st["total_pivots"] == host.stats()["total_pivots"]
    assert all(dev.status(i) == M.SolverStatus.Optimal for i in range(1024))
    assert max(dev.pivots(i) for i in range(1024)) < 2048            # the traces are whole
    assert_same_results(dev, host, 1024)
    for i in np.random.default_rng(20251016).choice(1024, 32, replace=False):
        o, st_o, tr = oracle_of(problems[i], O.RULE_BLOCK)
        assert_equals_oracle(dev, int(i), o, st_o, tr, f"seed {i + 1}")


# ---- 10
@pytest.mark.parametrize("rule", [O.RULE_BLOCK, O.RULE_BEST, O.RULE_FIRST])
def test_mixed_statuses_on_the_device(rule):
    cases = mixed_cases()
    b = M.BatchSolver(rule=RULES[rule], record_trace=4096)
    for _, p, stype, *_rest in cases:
        b.add(p, supply_type=stype)
    b.solve()
    check_mixed_batch(b, cases, rule)


# ---- 11
@pytest.mark.parametrize("rule", [O.RULE_BLOCK, O.RULE_BEST, O.RULE_FIRST])
def test_slicing_leaves_no_mark(rule):
    """The state survives the round trip through the workspace at any pivot: slices of 1, of 7 and the default give the same solve."""
    problems = [generated(3), generated(4, 80, 300), load("netgen_8_08a"), load("grid_5x5"), load("SimpleProblemIllustration2NonSparse")]
    solved = []
    for ppl in (0, 7, 1):
        if ppl == 1:
            problems = problems[:4]          # one launch per pivot: leave the 2 500-pivot global-tier instance to the slices of 7
        b = M.BatchSolver(rule=RULES[rule], record_trace=1 << 13, pivots_per_launch=ppl)
        for p in problems:
            b.add(p)
        b.solve()
        solved.append(b)
    whole, by7, by1 = solved
    assert whole.stats()["global_instances"] >= 1 and whole.stats()["lds_instances"] >= 2
    assert by7.stats()["launches"] > whole.stats()["launches"] and by1.stats()["launches"] >= max(by1.pivots(i) for i in range(4))
    assert_same_results(whole, by7, 5)
    assert_same_results(whole, by1, 4)
    o, st_o, tr = oracle_of(problems[0], rule)
    assert_equals_oracle(by1, 0, o, st_o, tr)


# ---- 12
def test_pivot_limit_on_the_device():
    p, q = generated(11), load("netgen_8_10a")           # LDS tier, global tier
    full = M.BatchSolver(record_trace=1 << 14)
    full.add(p)
    full.add(q)
    full.solve()
    assert full.status(0) == full.status(1) == M.SolverStatus.Optimal
    for k, ppl in ((1, 0), (17, 5), (300, 0), (300, 100)):
        b = M.BatchSolver(pivot_limit=k, record_trace=1 << 14, pivots_per_launch=ppl)
        b.add(p)
        b.add(q)
        b.add(load("transport_2x3"))
        b.solve()
        for i in (0, 1):
            want = min(k, full.pivots(i))
            assert b.pivots(i) == want and np.array_equal(b.trace(i), full.trace(i)[:want])
            assert b.status(i) == (M.SolverStatus.NotSolved if k < full.pivots(i) else M.SolverStatus.Optimal)
        assert b.status(2) == (M.SolverStatus.Optimal if k >= 4 else M.SolverStatus.NotSolved)


# ---- 17
@pytest.mark.parametrize("rule", [O.RULE_BLOCK, O.RULE_BEST, O.RULE_FIRST])
def test_adversarial_batch_on_the_device(rule):
    """The fuzz of test_adversarial_batch_on_the_host with 64 lanes: Infeasible and Unbounded endings, LEQ, lower bounds, infinite and zero
    capacities, ties and costs above 2^32 where the lanes' minima are combined over up to 16 strides, search ranges of 63 / 64 / 65 ...
    257 arcs, instances that never reach the device between ones that do.  Slices of 3 pivots end solves of every kind in the middle of a
    sequence of launches.  Every workspace here fits LDS; the global tier's share is test_adversarial_instances_in_the_global_tier."""
    count = len(fuzz_cases())
    dev = fuzz_solver(rule).solve()
    assert_fuzz_equals_oracle(dev, rule)
    host = fuzz_solver(rule).run_on_host()
    assert_same_results(dev, host, count)
    st = dev.stats()
    print(f"rule {rule}: {st}")
    by_bounds = sum(bound_infeasible(p) for p, _ in fuzz_cases())
    assert st["lds_instances"] + st["global_instances"] == count - by_bounds and st["total_pivots"] == host.stats()["total_pivots"]
    assert st["workspace_bytes"] == sum(footprint_of(p, stype) for p, stype in fuzz_cases())
    by3 = fuzz_solver(rule, pivots_per_launch=3).solve()
    assert by3.stats()["launches"] >= max(o.n_pivots for o, _, _ in fuzz_reference(rule)) // 3
    assert_same_results(dev, by3, count)
    assert_fuzz_equals_oracle(by3, rule)


# ---- 18
@pytest.mark.parametrize("rule", [O.RULE_BLOCK, O.RULE_BEST, O.RULE_FIRST])
def test_adversarial_instances_in_the_global_tier(rule):
    """The fuzz batch above fits LDS on every device (its largest workspace is 37 KB), so batch_kernel<false> sees none of it.  Here the
    largest instances of every outcome, padded with isolated nodes until no LDS limit holds them, run in place: whole, and in slices of 7."""
    count = len(padded_fuzz(rule))
    whole = check_padded_fuzz(lambda b: b.solve(), rule)
    st = whole.stats()
    print(f"rule {rule}: {st}")
    assert st["global_instances"] == count and st["lds_instances"] == 0 and st["lds_bytes_max"] == 0
    assert st["workspace_bytes"] == sum(footprint_of(q, stype) for q, stype, _ in padded_fuzz(rule))
    by7 = check_padded_fuzz(lambda b: b.solve(), rule, pivots_per_launch=7)
    assert by7.stats()["launches"] >= max(r[0].n_pivots for _, _, r in padded_fuzz(rule)) // 7
    assert_same_results(whole, by7, count)


# ---- 19
def test_footprint_ladder_across_the_classes_and_the_tier_edge():
    """One batch with, for every class limit L / d (L = 160 KiB and 64 KiB, d = 16, 8, 4, 3, 2, 1), the last workspace that fits and the
    first that does not: the classes hold mixed footprints, and whatever L this device gives, its two neighbours are here."""
    steps = ladder()
    count = len(steps)
    dev = M.BatchSolver(record_trace=1 << 14)
    host = M.BatchSolver(record_trace=1 << 14)
    for p, *_ in steps:
        dev.add(p)
        host.add(p)
    dev.solve()
    host.run_on_host()
    st = dev.stats()
    sizes = sorted(size for _, size, _, _ in steps)
    assert st["workspace_bytes"] == sum(sizes)                       # Layout (batch.hip) against the restatement of DESIGN.md 3.14
    j = st["lds_instances"]
    assert j + st["global_instances"] == count and 0 < j < count
    fitting = [L for L in LDS_LIMITS if st["lds_bytes_max"] <= L]
    assert fitting
    L = min(fitting)
    print(f"LDS limit found: {L} bytes; {st}")
    assert all(size <= st["lds_bytes_max"] for size in sizes[:j]) and sizes[j] > L
    assert sizes[j - 1] == st["lds_bytes_max"] and sizes[j - 1] <= L
    assert all(dev.status(i) == M.SolverStatus.Optimal and dev.pivots(i) < 1 << 14 for i in range(count))
    assert_same_results(dev, host, count)
    edge = [i for i, (_, size, _, _) in enumerate(steps) if size in (sizes[j - 1], sizes[j])]
    assert len(edge) == 2
    for i in edge:
        o, st_o, tr = oracle_of(steps[i][0], O.RULE_BLOCK)
        assert_equals_oracle(dev, i, o, st_o, tr, f"ladder step {i}")


# ---- 20
@pytest.mark.parametrize("pivots_per_launch", [0, 5])
def test_short_and_absent_traces_on_the_device(pivots_per_launch):
    """All traces of a batch share one device buffer: with a capacity below every pivot count each instance's entries are its own first
    pivots.  Capacity 0: the kernel gets no trace pointer."""
    check_short_and_absent_traces(lambda b: b.solve(), pivots_per_launch=pivots_per_launch)


# ---- 21
def test_nothing_to_run_on_the_device():
    check_nothing_to_run(lambda b: b.solve())
