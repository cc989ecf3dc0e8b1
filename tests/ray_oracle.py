"""What an answer of rays() (mcf_*batch_rays, DESIGN.md 3.14 "Unbounded or not: a negative cycle or labels from the kept data") must satisfy,
stated without the code under test: Python integers on the caller's own src / tgt / upper / cost.

  check_cycle         the marked arcs are ONE simple directed cycle of uncapacitated arcs whose costs sum to the claimed cost < 0
  check_labels        label[tgt] <= label[src] + cost on every uncapacitated arc: summed round any cycle of such arcs, its cost is >= 0
  has_negative_cycle  the truth: an arc-list Bellman-Ford over the uncapacitated arcs, n full passes and one more
  jacobi_rounds       how many rounds a Jacobi Bellman-Ford from all-zero labels makes before one changes nothing (None: there is a cycle)
and the family the tests run on: ray_family(), a fixed-seed fuzz with uncapacitated arcs."""
import functools

import numpy as np

from oracle import ns_oracle as O

from adversarial import BIG_COST, SEARCH_ARCS, random_problem

INF_CAP = int(O.INF_CAP)


def open_arcs(p):
    """(tail, head, cost, arc) of every uncapacitated arc"""
    return [(int(p.src[e]), int(p.tgt[e]), int(p.cost[e]), e) for e in range(p.m) if int(p.upper[e]) == INF_CAP]


def check_cycle(p, on_cycle, cycle_cost, cycle_length):
    marked = [e for e in range(p.m) if on_cycle[e]]
    assert set(int(x) for x in on_cycle) <= {0, 1} and len(on_cycle) == p.m
    assert marked and len(marked) == int(cycle_length), (marked, cycle_length)
    out_of, into = {}, {}
    for e in marked:
        assert int(p.upper[e]) == INF_CAP, f"arc {e} on the cycle is capacitated"
        a, b = int(p.src[e]), int(p.tgt[e])
        assert a not in out_of and b not in into, f"two marked arcs leave {a} or enter {b}"
        out_of[a], into[b] = e, e
    assert set(out_of) == set(into)                                          # every touched node: exactly one in, one out
    for start in marked:
        e, used = start, []
        for _ in range(len(marked)):
            used.append(e)
            e = out_of[int(p.tgt[e])]
        assert e == start and sorted(used) == marked, f"the marks are not one cycle from arc {start}"
    total = sum(int(p.cost[e]) for e in marked)
    assert total == int(cycle_cost) and total < 0, (total, int(cycle_cost))


def check_labels(p, label):
    assert len(label) == p.n
    for a, b, c, e in open_arcs(p):
        assert int(label[b]) <= int(label[a]) + c, f"arc {e}: label[{b}] = {int(label[b])} > label[{a}] + cost = {int(label[a]) + c}"


def has_negative_cycle(p):
    arcs = open_arcs(p)
    d = [0] * p.n
    for _ in range(p.n + 1):
        changed = False
        for a, b, c, _ in arcs:                                              # in place: Gauss-Seidel, the answer is the same
            if d[a] + c < d[b]:
                d[b] = d[a] + c
                changed = True
        if not changed:
            return False
    return True


def jacobi_rounds(p):
    if has_negative_cycle(p):
        return None
    arcs = open_arcs(p)
    d, rounds = [0] * p.n, 0
    while True:
        rounds += 1
        new = list(d)
        for a, b, c, _ in arcs:
            new[b] = min(new[b], d[a] + c)
        if new == d:
            return rounds
        d = new


def jacobi_frontiers(p):
    """The sizes of the frontiers of the documented rounds, restated from the data: round 1 starts from every node; a round's frontier is
    what fell in the round before; with k nodes that have an uncapacitated arc coming in, a fall in round k + 1 ends the rounds."""
    arcs = open_arcs(p)
    k = len({b for _, b, _, _ in arcs})
    d, sizes, frontier = [0] * p.n, [], p.n
    while frontier:
        sizes.append(frontier)
        new = list(d)
        for a, b, c, _ in arcs:
            new[b] = min(new[b], d[a] + c)
        frontier = sum(x != y for x, y in zip(new, d))
        d = new
        if frontier and len(sizes) == k + 1:
            break
    return sizes


def only_loops_are_negative(p):
    """Whether taking the negative self loops away leaves no negative cycle: if not, the instance holds one of two or more arcs"""
    keep = np.array([not (int(p.upper[e]) == INF_CAP and p.src[e] == p.tgt[e] and p.cost[e] < 0) for e in range(p.m)], bool)
    q = O.Problem(p.n, int(keep.sum()), p.src[keep], p.tgt[keep], p.lower[keep], p.upper[keep], p.cost[keep], p.supply)
    return not has_negative_cycle(q)


SEED = 20261021
PER_SIZE = 12


@functools.lru_cache(maxsize=None)
def ray_family():
    """[(problem, supply type)]: 12 instances for every size m + n of adversarial.SEARCH_ARCS, n in [1, min(m + n, 60)], no zero
    capacities (so that Unbounded by a zero capacity stays out of the way).  By the running index k: kind negative / balanced / negative /
    excess (k % 4); share of uncapacitated arcs 0.05 / 0.15 / 0.4 / 1.0 by (k // 4) % 4, and 0.02 / 0.05 / 0.1 / 0.2 above 257 search
    arcs, where a dense graph of at most 60 nodes would otherwise always hold a cycle; costs -1 / 0 / 1 where k % 5 == 2, times BIG_COST
    where k % 5 == 4; LEQ every sixth."""
    rng = np.random.default_rng(SEED)
    out = []
    for size in SEARCH_ARCS:
        for _ in range(PER_SIZE):
            k = len(out)
            n = int(rng.integers(1, min(size, 60) + 1))
            kind = ("negative", "balanced", "negative", "excess")[k % 4]
            share = ((0.05, 0.15, 0.4, 1.0) if size <= 257 else (0.02, 0.05, 0.1, 0.2))[(k // 4) % 4]
            p = random_problem(rng, n, size - n, kind, cost_scale=BIG_COST if k % 5 == 4 else 1, ties=k % 5 == 2, zero_capacity=False, inf_fraction=share)
            out.append((p, O.LEQ if k % 6 == 5 else O.GEQ))
    return tuple(out)
