"""Amounts beyond 32 bits (DESIGN.md 3.14 "Amounts beyond 32 bits"): supplies, lower bounds, capacities and so flows, the rooms of
data_ranges() and unmet / violation of diagnose() whose upper word is not zero.  Every other solver family draws amounts of at most 40
units, so a 32-bit shuffle, an int temporary or a uint32_t cast on an amount's way through the device passed the whole suite.

  scaled(p, k)    supply, lower and finite upper times k; MCF_INF_CAP and the costs stay
  K_HIGH          2^33 + 1: both words of every amount are non-zero, and an amount cut to its low word is the UNSCALED amount
  K_SIGN          2^31 + 1: one unit fits uint32 but not int32; larger amounts cross 2^32 by the carry alone

A scaled problem is the same linear program in another unit: the oracle must go through the same pivots to the same potentials, with flows
and cost k times the unscaled ones.  That law is asserted here on the oracle for every instance of every scaled family, and so is that the
oracle did not overflow (answer_of's checks); the host and device tests then hold the library to the oracle bit for bit and to the law.

The families (Block Search unless a rule is named):
  wide            wide_graphs.wide_family() / wide_chain(), all four graphs, the first solve's data and steps a, b, c, e
  adversarial     the 318 of adversarial_batch()'s 408 instances with max |cost| < BIG_COST / 4, under all three rules
  structured      the chorded path of data_ranges_oracle.structured_family(): uncapacitated chords and self loops, where infinite sides come from
  cuts            the hub and the grid of 12 x 12 with the supplies of test_diagnose_gpu.hub_batch(): feasible, 5 units too many on one
                  node, one node asked for more than its arcs carry; 16 variants each
  irregular       the three small wide graphs with amounts no scaling law covers: see irregular_family()

Measured on the oracle (printed by the functions below; Block Search where no rule is named):
  overflow        none, in any instance of any family under either factor, nor in the irregular family; the law holds for every instance
  wide            Optimal solves over the chain 40 / 37 / 35 / 20 (path / grid / hub / big grid); 2^32 or more on at least half of the
                  flow-carrying arcs in all of them under K_HIGH, in 40 / 35 / 35 / 20 under K_SIGN; largest flow 180 388 626 453
                  data-range sides both finite and above 2^32: 1 173 / 1 176 / 2 480 / 3 121 (K_SIGN 845 / 550 / 1 668 / 1 513), zero 1 474 / 1 906 / 2 640 / 6 511
  adversarial     per rule Optimal 165..168, Infeasible 136..137, Unbounded 13..16, scaled as unscaled; 116..120 Optimal with high flows;
                  sides both finite above 2^32: 10 656..11 674 (K_SIGN 2 906..3 694), zero 11 455..12 320, infinite 3 925..4 107
  structured      8 of 8 Optimal; sides both finite above 2^32: 836 (K_SIGN 465), zero 1 816, infinite 104
  cuts            8 of 16 infeasible on either graph, scaled or not; the hooks find 13 cuts of more than 64 nodes with a violation above
                  2^32 under either factor (asserted in test_big_amounts_host.cuts_log, each through certificate_oracle.check_cut)
  irregular       8 of 8 Optimal first solves per graph, largest flow 120 895 530 286; 8 warm candidates per graph and step, 5..8 of them
                  with a violated old optimum; first dual pivots whose two largest violations differ below bit 32 only: 5, from bit 32 up
                  only: 3, in both words: 9; sides both finite above 2^32: 1 056 / 864 / 2 233, zero 476 / 1 321 / 2 186"""
import functools

import numpy as np

from oracle import ns_oracle as O

import certificate_oracle as K
import data_ranges_oracle as D
import start_oracle as S
import wide_graphs as W
from adversarial import BIG_COST
from test_batch_host import fuzz_cases, oracle_of
from test_batch_resolve_host import cold_reference, warm_after
from test_redata_host import expected_warm, violates
from test_uniform_host import TRACE, Topology, answer_of

K_HIGH = 2 ** 33 + 1
K_SIGN = 2 ** 31 + 1
FACTORS = (K_HIGH, K_SIGN)
WORD = 1 << 32
ALL_RULES = (O.RULE_BLOCK, O.RULE_BEST, O.RULE_FIRST)
KEPT = 318                              # adversarial instances without 64-bit costs
SMALL_GRAPHS = (W.PATH, W.GRID, W.HUB)


def scaled(p, k):
    """supply, lower and finite upper times k; MCF_INF_CAP stays, costs are untouched"""
    k = np.int64(k)
    assert max(int(np.abs(p.supply).max(initial=0)), int(np.abs(p.lower).max(initial=0)), int(np.abs(np.where(p.upper == O.INF_CAP, 0, p.upper)).max(initial=0))) * int(k) < 1 << 61
    return O.Problem(p.n, p.m, p.src, p.tgt, p.lower * k, np.where(p.upper == O.INF_CAP, O.INF_CAP, p.upper * k).astype(np.int64), p.cost, p.supply * k)


def scaled_topology(t, k):
    return t if k == 1 else Topology(t.n, t.src, t.tgt, [scaled(p, k) for p in t.variants], t.zero_capacity)


def assert_law(unscaled, answer, k, what):
    """answer_of()'s tuples: the scaled problem's is the unscaled one's with flows and cost times k"""
    (st, pivots, tr, total, flows, pi), (st_k, pivots_k, tr_k, total_k, flows_k, pi_k) = unscaled, answer
    assert st == st_k and pivots == pivots_k and np.array_equal(tr, tr_k), (what, st, st_k, pivots, pivots_k)
    if st == O.OPTIMAL:
        assert total_k == total * k and np.array_equal(flows_k, flows * np.int64(k)) and np.array_equal(pi_k, pi), what


def carried_high(flows):
    """whether at least half of the flow-carrying arcs carry 2^32 or more"""
    carrying = flows != 0
    return bool(carrying.any() and 2 * int(np.sum(np.abs(flows) >= WORD)) >= int(carrying.sum()))


# ---- the wide family and its chain
@functools.lru_cache(maxsize=None)
def wide(k):
    """per graph (topology with the first solve's data, (topology after step a, b, c, e), supply type), every amount times k"""
    return tuple((scaled_topology(t, k), tuple(scaled_topology(s, k) for s in steps), stype) for (t, steps), (_, stype) in zip(W.wide_chain(), W.wide_family()))


@functools.lru_cache(maxsize=None)
def wide_reference(k, rule=O.RULE_BLOCK):
    """per graph, per topology of its chain, per variant (cold_reference(), answer_of()) of the scaled data: W.wide_reference()'s shape.
    Asserted on the oracle alone: no overflow (inside answer_of), the scaling law against the unscaled answers, and flows at or above
    2^32 on at least half of the flow-carrying arcs of at least 5 Optimal instances per graph (3 on the big grid)."""
    base = W.wide_reference(rule)
    if k == 1:
        return base
    out = []
    for g, (t, steps, stype) in enumerate(wide(k)):
        refs = tuple(tuple((cold_reference(p, stype, rule), answer_of(p, rule, stype, trace_cap=TRACE)) for p in top.variants) for top in (t,) + steps)
        optimal = high = 0
        for s, row in enumerate(refs):
            for v, (_, answer) in enumerate(row):
                assert_law(base[g][s][v][1], answer, k, (W.NAMES[g], s, v, k))
                assert base[g][s][v][0][0] == refs[s][v][0][0] and (base[g][s][v][0][2] is None) == (refs[s][v][0][2] is None)
                if answer[0] == O.OPTIMAL:
                    optimal += 1
                    high += carried_high(answer[4])
        largest = max((int(np.abs(a[4]).max()) for row in refs for _, a in row if a[0] == O.OPTIMAL), default=0)
        print(f"{W.NAMES[g]} times {k}, rule {rule}: {optimal} Optimal solves over the chain, {high} with 2^32 or more on at least half of the flow-carrying arcs; largest flow {largest}")
        assert high >= (3 if g == W.BIG else 5), (W.NAMES[g], k, high)
        out.append(refs)
    return tuple(out)


# ---- the adversarial batch without its 64-bit costs
@functools.lru_cache(maxsize=None)
def adversarial(k=1):
    """((problem, supply type) ...): the instances of adversarial_batch() with max |cost| < BIG_COST / 4, every amount times k"""
    kept = tuple((p if k == 1 else scaled(p, k), stype) for p, stype in fuzz_cases() if int(np.abs(p.cost).max(initial=0)) < BIG_COST // 4)
    assert len(kept) == KEPT, len(kept)
    return kept


@functools.lru_cache(maxsize=None)
def adversarial_reference(k, rule):
    """((oracle, status, answer_of()) per instance of adversarial(k)).  Asserted on the oracle alone: no overflow, the scaling law, at
    least 130 Infeasible and 10 Unbounded, and Optimal instances with 2^32 or more on at least half of their flow-carrying arcs."""
    out = []
    for i, (p, stype) in enumerate(adversarial(k)):
        o, st, _ = oracle_of(p, rule, stype, trace_cap=0)
        out.append((o, st, answer_of(p, rule, stype)))
    count = {st: sum(s == st for _, s, _ in out) for st in (O.OPTIMAL, O.INFEASIBLE, O.UNBOUNDED)}
    high = sum(carried_high(a[4]) for _, st, a in out if st == O.OPTIMAL)
    if k != 1:
        for i, ((_, _, a), (_, _, b)) in enumerate(zip(adversarial_reference(1, rule), out)):
            assert_law(a, b, k, ("adversarial", i, k, rule))
    print(f"adversarial times {k}, rule {rule}: Optimal {count[O.OPTIMAL]}, Infeasible {count[O.INFEASIBLE]}, Unbounded {count[O.UNBOUNDED]}; "
          f"{high} Optimal with 2^32 or more on at least half of the flow-carrying arcs")
    assert sum(count.values()) == KEPT and count[O.INFEASIBLE] >= 130 and count[O.UNBOUNDED] >= 10, count
    assert k == 1 or high >= 50, high
    return tuple(out)


# ---- the structured graph: uncapacitated chords and self loops
@functools.lru_cache(maxsize=None)
def structured(k=1):
    t, stype = D.structured_family()
    return scaled_topology(t, k), stype


def structured_pairs():
    t, _ = D.structured_family()
    return D.pairs_of((4,), t.n, t.src, t.tgt)


@functools.lru_cache(maxsize=None)
def structured_reference(k, rule=O.RULE_BLOCK):
    """answer_of() per variant; the scaling law and no overflow"""
    t, stype = structured(k)
    out = tuple(answer_of(p, rule, stype) for p in t.variants)
    if k != 1:
        for v, (a, b) in enumerate(zip(structured_reference(1, rule), out)):
            assert_law(a, b, k, ("structured", v, k))
        high = sum(carried_high(a[4]) for a in out if a[0] == O.OPTIMAL)
        print(f"structured times {k}: {sum(a[0] == O.OPTIMAL for a in out)} Optimal, {high} with 2^32 or more on at least half of the flow-carrying arcs")
        assert high >= 5, high
    return out


# ---- the sides of the data ranges
SIDES = ("both_finite_above_a_word", "zero", "infinite")


def sides_of(rows):
    """what the non-tree arcs of data_ranges_oracle.reference_rows() cover: both sides finite and above 2^32, a side zero, a side infinite"""
    off = (rows["arc_state"] != 0) & rows["ranged_arcs"]
    down, up = rows["flow_down"][off], rows["flow_up"][off]
    finite = (down != D.INF) & (up != D.INF)
    return dict(both_finite_above_a_word=int(np.sum(finite & (down > WORD) & (up > WORD))), zero=int(np.sum((down == 0) | (up == 0))),
                infinite=int(np.sum((down == D.INF) | (up == D.INF))))


def assert_scaled_rows(base, rows, k, what):
    """the law on data_ranges_oracle's rows: ranged and arc_state kept, finite entries times k, INF and the -1 of a pair out of range kept"""
    assert np.array_equal(base["ranged"], rows["ranged"]) and np.array_equal(base["arc_state"], rows["arc_state"]), what
    for name in ("flow_down", "flow_up", "ship_forth", "ship_back"):
        sentinel = (base[name] == D.INF) | (base[name] == -1)          # the oracle gives -1 for a pair out of range only: its finite rooms are >= 0
        assert np.array_equal(rows[name], np.where(sentinel, base[name], base[name] * np.int64(k))), (what, name)


@functools.lru_cache(maxsize=None)
def wide_data_rows(k, rule=O.RULE_BLOCK):
    """per graph data_ranges_oracle.reference_rows() of the first solve of the scaled data, with D.wide_pairs(); floors per graph: sides
    both finite and above 2^32, and sides equal to zero"""
    out = []
    for g, (t, _, stype) in enumerate(wide(k)):
        rows = D.reference_rows([(p,) + oracle_of(p, rule, stype, trace_cap=0)[:2] + (D.wide_pairs()[g],) for p in t.variants])
        if k != 1:
            assert_scaled_rows(D.wide_rows(rule)[g], rows, k, (W.NAMES[g], k))
            sides = sides_of(rows)
            print(f"data ranges, {W.NAMES[g]} times {k}: {sides}")
            assert sides["both_finite_above_a_word"] > 0 and sides["zero"] > 0, (W.NAMES[g], sides)
        out.append(rows)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def structured_data_rows(k, rule=O.RULE_BLOCK):
    t, stype = structured(k)
    rows = D.reference_rows([(p,) + oracle_of(p, rule, stype, trace_cap=0)[:2] + (structured_pairs(),) for p in t.variants])
    if k != 1:
        assert_scaled_rows(D.structured_rows(rule)[1], rows, k, ("structured", k))
        sides = sides_of(rows)
        print(f"data ranges, structured times {k}: {sides}")
        assert min(sides.values()) > 0, sides
    return rows


@functools.lru_cache(maxsize=None)
def adversarial_pairs():
    return tuple(D.pairs_of((5, i), p.n, p.src, p.tgt) for i, (p, _) in enumerate(adversarial()))


@functools.lru_cache(maxsize=None)
def adversarial_data_rows(k, rule):
    rows = D.reference_rows([(p, o, st, pairs) for (p, _), (o, st, _), pairs in zip(adversarial(k), adversarial_reference(k, rule), adversarial_pairs())])
    if k != 1:
        assert_scaled_rows(adversarial_data_rows(1, rule), rows, k, ("adversarial", k, rule))
        sides = sides_of(rows)
        print(f"data ranges, adversarial times {k}, rule {rule}: {sides}")
        assert min(sides.values()) > 0, sides
    return rows


# ---- cuts wider than a wave with a violation above 2^32
CUT_GRAPHS = (W.HUB, W.GRID)
CUT_COUNT = 16


@functools.lru_cache(maxsize=None)
def cut_family(k=1):
    """per graph of CUT_GRAPHS a topology of 16 variants under GEQ, the supplies of test_diagnose_gpu.hub_batch() by v % 4: balanced
    (feasible), 5 units too many on one node (nobody takes them: S is everything the node reaches), one node asked to ship 200 units
    more than its outgoing arcs carry (S is small), balanced again.  No lower bounds; every amount times k."""
    out = []
    for g in CUT_GRAPHS:
        n, src, tgt, _, cap_range, _, _ = W.shapes()[g]
        m = len(src)
        variants = []
        for v in range(CUT_COUNT):
            rng = np.random.default_rng([W.SEED, 10, g, v])
            cap = rng.integers(cap_range[0], cap_range[1]).astype(np.int64)
            supply = np.zeros(n, np.int64)
            amount = rng.integers(1, 7, 12)
            nodes = rng.choice(np.arange(1, n), 24, replace=False)
            supply[nodes[:12]] += amount
            supply[nodes[12:]] -= amount
            if v % 4 == 1:
                supply[nodes[0]] += 5
            if v % 4 == 2:
                supply[nodes[0]] += 200
                supply[nodes[12]] -= 200
            p = O.Problem(n, m, src, tgt, np.zeros(m, np.int64), cap, rng.integers(1, 20, m).astype(np.int64), supply)
            variants.append(p if k == 1 else scaled(p, k))
        out.append(Topology(n, src, tgt, variants, [False] * CUT_COUNT))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def cut_truth(k=1):
    """certificate_oracle.feasible() per graph and variant; scaling changes no answer, and about half are infeasible"""
    truth = tuple(tuple(K.feasible(p, O.GEQ) for p in t.variants) for t in cut_family(k))
    for g, row in zip(CUT_GRAPHS, truth):
        infeasible = sum(f is False for f in row)
        print(f"cuts, {W.NAMES[g]} times {k}: {infeasible} of {len(row)} infeasible by the max-flow test")
        assert None not in row and CUT_COUNT * 3 // 8 <= infeasible <= CUT_COUNT * 5 // 8, (W.NAMES[g], row)
    assert k == 1 or truth == cut_truth(1)
    return truth


# ---- the irregular family: amounts that are no multiple of anything
IRREGULAR_SEED = 20261106               # chosen on the CPU: the first seed from 20261101 on at which the oracle meets every floor of irregular_reference()
IRREGULAR_PER = 8
IRREGULAR_STEPS = ("shift", "halve")
LOW = WORD - 1


def irregular_amounts(rng, mode, small, jitter_bits=20):
    """an amount per entry of `small` (small integers): mode 0 -- drawn in [2^33, 2^36) whatever `small` is; mode 1 -- small * K_HIGH + a
    jitter below 2^20, so that entries with equal `small` differ below bit 32 only; mode 2 -- small * 2^32: the low words are all equal"""
    small = np.asarray(small, np.int64)
    if mode == 0:
        return rng.integers(1 << 33, 1 << 36, small.shape).astype(np.int64)
    if mode == 1:
        return small * np.int64(K_HIGH) + rng.integers(0, 1 << jitter_bits, small.shape)
    return small * np.int64(WORD)


@functools.lru_cache(maxsize=None)
def irregular_family(seed=IRREGULAR_SEED):
    """per graph of SMALL_GRAPHS (topology of the first solve, (topology after "shift", after "halve"), supply type): 8 variants each.
      capacities    small * K_HIGH + jitter, small from the graph's capacity range of wide_graphs.shapes(), jitter in [0, 2^20)
      lower bounds  on about 15 % of the arcs, in [0, 2^34), below the capacity
      supplies      per pair of nodes >= 64 an amount in [2^33, 2^36)
    in the variants v % 4 in (0, 1).  With these alone no two violations ever share a low word, so two variants in four draw otherwise:
    v % 4 == 2 draws the supplies as small * K_HIGH + jitter too (small in 1..6: equal high parts are common, and the jitter settles
    them), v % 4 == 3 makes every amount a multiple of 2^32 (the low words are all zero, and the high words settle everything).
    "shift" moves an amount of the variant's kind from one supply node to one demand node, "halve" halves the capacities (in v % 4 == 3
    rounded down to a multiple of 2^32, at least 2^32) -- the steps a and c of test_redata_host.next_data at this magnitude."""
    out = []
    for g in SMALL_GRAPHS:
        n, src, tgt, cost_range, cap_range, pairs, _ = W.shapes()[g]
        m = len(src)
        first, shifted, halved = [], [], []
        for v in range(IRREGULAR_PER):
            rng = np.random.default_rng([seed, 5, g, v])
            kind = v % 4
            mode = {0: 0, 1: 0, 2: 1, 3: 2}[kind]
            cost = rng.integers(cost_range[0], cost_range[1]).astype(np.int64)
            cap = irregular_amounts(rng, 2 if kind == 3 else 1, rng.integers(cap_range[0], cap_range[1]))
            drawn = rng.integers(0, 1 << 34, m) if kind != 3 else rng.integers(0, 4, m) * np.int64(WORD)
            lower = np.minimum(np.where(rng.random(m) < 0.15, drawn, 0), cap - 1).astype(np.int64)
            if kind == 3:
                lower &= ~np.int64(LOW)
            amount = irregular_amounts(rng, mode, rng.integers(1, 7, pairs))
            supply = np.zeros(n, np.int64)
            supply[rng.choice(W.pool_of(n), pairs, replace=False)] += amount
            supply[rng.choice(W.pool_of(n), pairs, replace=False)] -= rng.permutation(amount)
            assert np.all(cap >= 1) and np.all(lower >= 0) and supply.sum() == 0
            p = O.Problem(n, m, src, tgt, lower, lower + cap, cost, supply)
            first.append(p)
            pos, neg = np.flatnonzero(supply > 0), np.flatnonzero(supply < 0)
            delta = int(irregular_amounts(rng, mode, rng.integers(1, 4, 1))[0]) >> (2 if mode == 0 else 0)
            moved = supply.copy()
            moved[rng.choice(pos)] -= delta
            moved[rng.choice(neg)] += delta
            q = O.Problem(n, m, src, tgt, lower, p.upper, cost, moved)
            shifted.append(q)
            half = (cap + 1) // 2 if kind != 3 else np.maximum((cap // 2) & ~np.int64(LOW), WORD)
            halved.append(O.Problem(n, m, src, tgt, lower, lower + half, cost, moved))
        tops = [Topology(n, src, tgt, variants, [False] * IRREGULAR_PER) for variants in (first, shifted, halved)]
        out.append((tops[0], (tops[1], tops[2]), O.LEQ if g == W.PATH else O.GEQ))
    return tuple(out)


def two_largest(o, p, q, stype):
    """The two largest violations max(-flow, flow - capacity) among the tree arcs when the basis the oracle `o` ended with on p meets the
    data of q, from the tree flows start_oracle derives (as wide_graphs.first_leaving() does); None unless two arcs are violated."""
    row = o.internal_arrays()["state"][:p.m]
    if S.count_tree(row) != p.n - 1:
        return None
    start = S.classify(q, stype, row)
    if start.kind != S.DUAL:
        return None
    found = sorted((max(-int(start.flow[e]), int(start.flow[e]) - int(q.upper[e] - q.lower[e])) for e in np.flatnonzero(row == S.TREE)), reverse=True)[:2]
    return found if len(found) == 2 and found[1] > 0 else None


@functools.lru_cache(maxsize=None)
def irregular_reference(seed=IRREGULAR_SEED, rule=O.RULE_BLOCK):
    """per graph, per topology of its chain, per variant (cold_reference(), answer_of()).  Asserted on the oracle and the data alone:
    no overflow (inside answer_of and cold_reference); per graph at least 5 Optimal first solves, each with 2^32 or more on at least
    half of its flow-carrying arcs; per step at least 3 warm candidates per graph whose old optimum violates the new data; and over
    the family at least 3 first dual pivots whose two largest violations differ below bit 32 only, and at least 3 where they differ
    from bit 32 up only."""
    out = []
    low_only = high_only = both = 0
    for g, (t, steps, stype) in zip(SMALL_GRAPHS, irregular_family(seed)):
        tops = (t,) + steps
        refs = tuple(tuple((cold_reference(p, stype, rule), answer_of(p, rule, stype, trace_cap=TRACE)) for p in top.variants) for top in tops)
        optimal = [a for _, a in refs[0] if a[0] == O.OPTIMAL]
        assert len(optimal) >= 5 and all(carried_high(a[4]) for a in optimal), (W.NAMES[g], len(optimal))
        assert max(a[1] for row in refs for _, a in row) < TRACE
        for s, name in enumerate(IRREGULAR_STEPS):
            candidates = forced = 0
            for v, q in enumerate(steps[s].variants):
                (before, answer_before), (after, _) = refs[s][v], refs[s + 1][v]
                assert after[0] != O.UNBOUNDED
                if expected_warm(before, q) and warm_after(after):
                    candidates += 1
                    forced += violates(q, answer_before[4])
                    o, st, _ = oracle_of(tops[s].variants[v], rule, stype, trace_cap=0)
                    pair = two_largest(o, tops[s].variants[v], q, stype)
                    if pair is not None and pair[0] != pair[1]:
                        same_high, same_low = pair[0] >> 32 == pair[1] >> 32, pair[0] & LOW == pair[1] & LOW
                        low_only += same_high
                        high_only += same_low
                        both += not same_high and not same_low
            print(f"irregular, {W.NAMES[g]}, step {name}: {candidates} warm candidates, {forced} with a violated old optimum")
            assert forced >= 3, (W.NAMES[g], name, candidates, forced)
        largest = max(int(np.abs(a[4]).max()) for row in refs for _, a in row if a[0] == O.OPTIMAL)
        print(f"irregular, {W.NAMES[g]}: {len(optimal)} Optimal first solves, largest flow {largest}")
        out.append(refs)
    print(f"irregular: first dual pivots whose two largest violations differ below bit 32 only: {low_only}, from bit 32 up only: {high_only}, in both words: {both}")
    assert low_only >= 3 and high_only >= 3, (low_only, high_only, both)
    return tuple(out)


def irregular_pairs():
    return tuple(D.wide_pairs()[g] for g in SMALL_GRAPHS)


@functools.lru_cache(maxsize=None)
def irregular_data_rows(rule=O.RULE_BLOCK):
    out = []
    for g, (t, _, stype), pairs in zip(SMALL_GRAPHS, irregular_family(), irregular_pairs()):
        rows = D.reference_rows([(p,) + oracle_of(p, rule, stype, trace_cap=0)[:2] + (pairs,) for p in t.variants])
        sides = sides_of(rows)
        print(f"data ranges, irregular {W.NAMES[g]}: {sides}")
        assert sides["both_finite_above_a_word"] > 0 and sides["zero"] > 0, sides
        out.append(rows)
    return tuple(out)
