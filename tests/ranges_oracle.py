"""Cost ranges by brute force from the oracle's own basis: the reference of test_ranges_host.py and test_ranges_gpu.py.

Independent of the library: it reads only oracle.ns_oracle.Oracle after a solve.  The oracle is pivot-for-pivot identical to the batch
solver, so Oracle.internal_arrays() sliced to all_arc_num is the basis the batch keeps: standard form, arcs [0, m) the caller's,
[m, m + n) the root links, the rules scan [0, search_arc_num); rc_f = cost_f + pi[src_f] - pi[tgt_f]; state LOWER = +1, TREE = 0,
UPPER = -1.

The definition, applied arc by arc.  A non-tree arc at LOWER may rise for ever and fall by rc; at UPPER it may fall for ever and rise
by -rc.  A tree arc e is taken out of the tree: the nodes the root no longer reaches are the set S.  Raising cost_e by d while e keeps
reduced cost 0 and the root keeps its potential shifts pi on S by -d where e's source lies in S, by +d where its target does.  An arc f
with exactly one end in S then has rc_f changed by that shift times ([src_f in S] - [tgt_f in S]); the basis stays optimal while
state_f * rc_f >= 0.  up[e] is the smallest state_f * rc_f among the arcs a raise pushes toward 0, down[e] among those a fall pushes."""
import functools

import numpy as np

from oracle import ns_oracle as O

from test_batch_host import fuzz_cases, fuzz_reference, padded_fuzz

INF = np.iinfo(np.int64).max          # MCF_RANGE_INF


def is_ranged(o, st, p):
    """Optimal, with every supply met exactly: no flow is left on a root link (that is Optimal) nor on an artificial arc."""
    if st != O.OPTIMAL:
        return False
    net = np.zeros(p.n, np.int64)
    f = o.flow()
    np.add.at(net, p.src, f)
    np.subtract.at(net, p.tgt, f)
    return bool(np.array_equal(net, p.supply))


def brute_force(o, p):
    """(arc_state[m] int8, down[m], up[m] int64) of the basis oracle `o` ended with on problem `p`."""
    n, m = p.n, p.m
    A, S = o.all_arc_num, o.search_arc_num
    a = o.internal_arrays()
    src, tgt, cost, state, pi = a["src"][:A].astype(np.int64), a["tgt"][:A].astype(np.int64), a["cost"][:A], a["state"][:A], a["pi"]
    tree = np.flatnonzero(state == 0)
    assert len(tree) == n, (len(tree), n)
    # the tree from the root: every node's depth-first entry and exit time, from the tree arcs alone
    adj = [[] for _ in range(n + 1)]
    for e in tree:
        adj[src[e]].append((int(tgt[e]), int(e)))
        adj[tgt[e]].append((int(src[e]), int(e)))
    tin, tout, below = np.full(n + 1, -1, np.int64), np.zeros(n + 1, np.int64), {}
    clock, stack = 0, [(n, iter(adj[n]))]
    tin[n] = 0
    while stack:
        v, it = stack[-1]
        for w, e in it:
            if tin[w] < 0:
                clock += 1
                tin[w] = clock
                below[e] = w                 # the end of tree arc e that loses the root when e is removed
                stack.append((w, iter(adj[w])))
                break
        else:
            tout[v] = clock
            stack.pop()
    assert np.all(tin >= 0), "the arcs with state 0 do not span the nodes"
    rc = cost + pi[src] - pi[tgt]
    slack = state.astype(np.int64) * rc
    search = np.arange(A) < S
    down, up = np.empty(m, np.int64), np.empty(m, np.int64)
    for e in range(m):
        if state[e] == 1:
            down[e], up[e] = rc[e], INF
        elif state[e] == -1:
            down[e], up[e] = INF, -rc[e]
        else:
            w = below[e]
            in_s = (tin >= tin[w]) & (tin <= tout[w])                       # flooding from the root without e reaches everything else
            assert in_s[w] and not in_s[n] and in_s[src[e]] != in_s[tgt[e]]
            shift = -1 if in_s[src[e]] else 1                               # of pi on S, per unit the cost is raised
            crossing = search & (state != 0) & (in_s[src] != in_s[tgt])
            move = state.astype(np.int64) * shift * (in_s[src].astype(np.int64) - in_s[tgt].astype(np.int64))     # of state * rc per unit raised
            toward_up, toward_down = crossing & (move < 0), crossing & (move > 0)
            up[e] = slack[toward_up].min() if toward_up.any() else INF
            down[e] = slack[toward_down].min() if toward_down.any() else INF
    return state[:m].astype(np.int8), down, up, bool(np.all(slack[search] >= 0))


def reference_rows(cases):
    """cases: ((problem, oracle, status) ...) -> (ranged [count] int32, arc_state, down, up flat over all instances' arcs, tally)"""
    ranged, states, downs, ups = [], [], [], []
    tally = dict(ranged=0, above_one_stride=0, both_finite=0, one_infinite=0)
    for p, o, st in cases:
        r = is_ranged(o, st, p)
        ranged.append(int(r))
        if not r:
            states.append(np.zeros(p.m, np.int8)); downs.append(np.zeros(p.m, np.int64)); ups.append(np.zeros(p.m, np.int64))
            continue
        s, d, u, feasible = brute_force(o, p)
        assert feasible and np.all(d >= 0) and np.all(u >= 0)
        states.append(s); downs.append(d); ups.append(u)
        tree = s == 0
        tally["ranged"] += 1
        tally["above_one_stride"] += int(o.search_arc_num > 64)
        tally["both_finite"] += int(np.sum(tree & (d != INF) & (u != INF)))
        tally["one_infinite"] += int(np.sum(tree & ((d == INF) | (u == INF))))
    cat = lambda parts, dtype: np.concatenate(parts).astype(dtype) if parts else np.zeros(0, dtype)
    return np.array(ranged, np.int32), cat(states, np.int8), cat(downs, np.int64), cat(ups, np.int64), tally


@functools.lru_cache(maxsize=None)
def fuzz_ranges(rule):
    """The adversarial batch's rows per rule, computed once and left unchanged; the floors are asserted here, on the oracle's side alone."""
    rows = reference_rows([(p, o, st) for (p, _), (o, st, _) in zip(fuzz_cases(), fuzz_reference(rule))])
    tally = rows[4]
    print(f"ranges, rule {rule}: {tally}")
    assert tally["ranged"] >= 100 and tally["above_one_stride"] >= 60 and tally["both_finite"] >= 1000 and tally["one_infinite"] >= 5, tally
    return rows


@functools.lru_cache(maxsize=None)
def padded_ranges(rule):
    """The same for the padded global-tier instances of test_batch_host.padded_fuzz.  The oracle finds 4 of the 18 ranged under every
    rule, with 127 tree arcs finite on both sides; the floors only say that the global tier's test is not empty."""
    rows = reference_rows([(q, o, st) for q, _, (o, st, _) in padded_fuzz(rule)])
    print(f"padded ranges, rule {rule}: {rows[4]}")
    assert rows[4]["ranged"] >= 1 and rows[4]["both_finite"] >= 10, rows[4]
    return rows
