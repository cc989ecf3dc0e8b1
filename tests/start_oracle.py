"""What a start from a given basis must come to (mcf_*batch_solve_from, DESIGN.md 3.14 "Start from a given basis"), restated in plain numpy
and Python integers from the problem and the row of arc states alone -- no walk order, no thread list, no workspace:

  forest or not (union-find over the TREE arcs), the components, the non-tree flows by state, the tree flows by solving conservation on
  the forest leaf by leaf, the potentials with the hanging rule (each component's lowest node hangs on the root by an artificial arc of
  cost art_cost, so it gets -art_cost under GEQ and +art_cost under LEQ), and from those the class.

classify() predicts the class the library must count; the tests compare it with start_stats() and with how each row came out."""
import numpy as np

from oracle import ns_oracle as O

LOWER, TREE, UPPER = 1, 0, -1
COLD, PRIMAL, DUAL = "cold", "primal", "dual"


class Start:
    """kind: COLD / PRIMAL / DUAL; why: the rule that made it cold; for an accepted start also components, flow (standard form) and pi."""

    def __init__(self, kind, why="", components=0, flow=None, pi=None):
        self.kind, self.why, self.components, self.flow, self.pi = kind, why, components, flow, pi


def art_cost_of(p):
    return (max((abs(int(c)) for c in p.cost), default=0) + 1) * p.n


def classify(p, stype, row):
    n, m = p.n, p.m
    row = [int(s) for s in row]
    src, tgt = [int(v) for v in p.src], [int(v) for v in p.tgt]
    lower, cost, supply = [int(v) for v in p.lower], [int(v) for v in p.cost], [int(v) for v in p.supply]
    capped = [int(u) != O.INF_CAP for u in p.upper]
    cap = [int(u) - lo if c else None for u, lo, c in zip(p.upper, lower, capped)]      # None: uncapacitated
    if any(c is not None and c < 0 for c in cap):
        return Start(COLD, "an upper bound below its lower bound")
    if any(s not in (LOWER, TREE, UPPER) for s in row):
        return Start(COLD, "a value that is no state")
    if any(s == UPPER and c is None for s, c in zip(row, cap)):
        return Start(COLD, "UPPER on an uncapacitated arc")
    if sum(supply) != 0:
        return Start(COLD, "the supplies do not sum to zero")
    if n == 0:
        return Start(COLD, "no node")
    # the forest: union-find, lowest node as the representative
    rep = list(range(n))

    def find(v):
        while rep[v] != v:
            rep[v] = rep[rep[v]]
            v = rep[v]
        return v

    near = [[] for _ in range(n)]       # per node (arc, other end, node is the arc's tail)
    for e in range(m):
        if row[e] != TREE:
            continue
        a, b = find(src[e]), find(tgt[e])
        if a == b:
            return Start(COLD, "the tree arcs hold a cycle")
        rep[max(a, b)] = min(a, b)
        near[src[e]].append((e, tgt[e], True))
        near[tgt[e]].append((e, src[e], False))
    roots = sorted({find(v) for v in range(n)})
    # the excess every node must send away through tree arcs: shifted supply minus what its non-tree arcs carry
    flow = [0] * m
    excess = list(supply)
    for e in range(m):
        moved = lower[e]
        if row[e] != TREE:
            flow[e] = cap[e] if row[e] == UPPER else 0
            moved += flow[e]
        excess[src[e]] -= moved
        excess[tgt[e]] += moved
    art = art_cost_of(p)
    pi = [None] * n
    for r in roots:
        pi[r] = -art if stype == O.GEQ else art
        order, above = [r], {r: None}
        for u in order:                 # breadth first: parents before children
            for e, v, u_is_tail in near[u]:
                if v in above:
                    continue
                above[v] = (e, u, not u_is_tail)
                pi[v] = pi[u] + cost[e] if u_is_tail else pi[u] - cost[e]      # cost + pi[tail] - pi[head] = 0
                order.append(v)
        for v in reversed(order[1:]):   # children before parents
            e, u, v_is_tail = above[v]
            flow[e] = excess[v] if v_is_tail else -excess[v]
            excess[u] += excess[v]
        if excess[r] != 0:
            return Start(COLD, "a component does not balance by itself")
    inside = all(0 <= flow[e] and (cap[e] is None or flow[e] <= cap[e]) for e in range(m) if row[e] == TREE)
    if inside:
        return Start(PRIMAL, components=len(roots), flow=flow, pi=pi)
    if all(row[e] * (cost[e] + pi[src[e]] - pi[tgt[e]]) >= 0 for e in range(m)):     # the root links: LOWER, reduced cost -/+ pi[v] >= 0 always
        assert all((-v if stype == O.GEQ else v) >= 0 for v in pi)
        return Start(DUAL, components=len(roots), flow=flow, pi=pi)
    return Start(COLD, "neither primal nor dual feasible")


def count_tree(row):
    return int(np.count_nonzero(np.asarray(row) == TREE))
