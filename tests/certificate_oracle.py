"""What a diagnosis (mcf_*batch_diagnose, DESIGN.md 3.14 "Why infeasible: a cut from the kept flow") must satisfy, stated without the code
under test: Python integers on the caller's own lower / upper / supply.

  check_cut   a node set S and a claimed violation: recomputes the cut inequality and requires that it equals the claim, that the claim
              is positive, and that no uncapacitated arc crosses S in the bounding direction.  Such a cut proves infeasibility on its own:
                GEQ  every flow has  sum of net outflow over S = flow(leaving S) - flow(entering S) <= upper(leaving) - lower(entering),
                     and the constraints ask for at least supply(S);
                LEQ  ... >= lower(leaving) - upper(entering), and the constraints ask for at most supply(S).
  feasible    whether ANY flow satisfies the constraints: a plain augmenting-path max-flow on the standard form (lower bounds shifted into
              the supplies).  GEQ: every positive shifted supply must be shipped, demands may absorb up to their size -- a node may always send
              more than its supply, which helps nobody.  LEQ: mirrored.  None where an arc has upper < lower (infeasible by its bounds)."""
from collections import deque

from oracle import ns_oracle as O

INF_CAP = int(O.INF_CAP)


def check_cut(p, supply_type, side, violation):
    """Asserts that `side` ([n], nonzero = in S) is a cut of problem p that is violated by exactly `violation` > 0."""
    inside = [bool(s) for s in side]
    assert len(inside) == p.n and any(inside)
    supply = sum(int(b) for b, s in zip(p.supply, inside) if s)
    lower_out = upper_out = lower_in = upper_in = 0
    for e in range(p.m):
        a, b = inside[int(p.src[e])], inside[int(p.tgt[e])]
        if a == b:
            continue
        lo, up = int(p.lower[e]), int(p.upper[e])
        bounding = a if supply_type == O.GEQ else b        # GEQ is bounded by the capacity that leaves S, LEQ by the capacity that enters it
        assert not (bounding and up == INF_CAP), f"uncapacitated arc {e} crosses the cut in the bounding direction"
        if a:
            lower_out += lo; upper_out += up
        else:
            lower_in += lo; upper_in += up
    value = supply - (upper_out - lower_in) if supply_type == O.GEQ else (lower_out - upper_in) - supply
    assert value == int(violation), (value, int(violation))
    assert value > 0, value


def max_flow(nodes, arcs, s, t):
    """arcs: [(tail, head, capacity)], capacity None = unbounded.  Breadth-first augmenting paths, each pushed to its bottleneck."""
    head, cap, first = [], [], [[] for _ in range(nodes)]
    for a, b, c in arcs:
        first[a].append(len(head)); head.append(b); cap.append(c)
        first[b].append(len(head)); head.append(a); cap.append(0)
    total = 0
    while True:
        via = [-1] * nodes
        via[s] = -2
        queue = deque([s])
        while queue and via[t] == -1:
            u = queue.popleft()
            for k in first[u]:
                if via[head[k]] == -1 and (cap[k] is None or cap[k] > 0):
                    via[head[k]] = k
                    queue.append(head[k])
        if via[t] == -1:
            return total
        push, v = None, t
        while v != s:
            k = via[v]
            if cap[k] is not None and (push is None or cap[k] < push):
                push = cap[k]
            v = head[k ^ 1]
        assert push is not None          # the arcs at s and t are capacitated
        v = t
        while v != s:
            k = via[v]
            if cap[k] is not None:
                cap[k] -= push
            if cap[k ^ 1] is not None:
                cap[k ^ 1] += push
            v = head[k ^ 1]
        total += push


def feasible(p, supply_type):
    """True / False; None where the problem is infeasible by an arc's bounds."""
    shifted = [int(b) for b in p.supply]
    arcs = []
    for e in range(p.m):
        lo, up = int(p.lower[e]), int(p.upper[e])
        if up < lo:
            return None
        a, b = int(p.src[e]), int(p.tgt[e])
        shifted[a] -= lo
        shifted[b] += lo
        arcs.append((a, b, None if up == INF_CAP else up - lo))
    s, t = p.n, p.n + 1
    # GEQ: what must leave a node is the source's, what may arrive is the sink's; LEQ: what must arrive is the sink's, what may leave the source's
    must = 0
    for v, b in enumerate(shifted):
        if b > 0:
            arcs.append((s, v, b))
            must += b if supply_type == O.GEQ else 0
        elif b < 0:
            arcs.append((v, t, -b))
            must += -b if supply_type == O.LEQ else 0
    return max_flow(p.n + 2, arcs, s, t) == must
