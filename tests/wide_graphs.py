"""Structured, connected graphs of more than 64 nodes for the three newest steps of the placed batches (resolve_data, cost_ranges, solve_from;
DESIGN.md 3.14): every other family of these steps has at most 60 nodes that matter, so no node-strided lane loop ever had its answer past
the first stride, no tree was deeper than a wave is wide, and the global tier never held a connected tree.

  chorded path   130 nodes, 258 path arcs (both ways, cost 0..2, capacity 20..39) and 200 chords (cost 30..59): the optimal tree is nearly the path
  grid 12 x 12   144 nodes, 528 arcs (4-neighbour, both directions)
  hub            161 nodes: node 0 and 160 leaves, four arcs between the hub and every leaf and a ring over the leaves, 800 arcs
  big grid       29 x 29, 841 nodes, 3248 arcs: the smallest square grid whose workspace exceeds every LDS limit with no artificial arc

8 variants each (4 on the big grid): finite positive capacities, lower bounds on about 15 % of the arcs, supplies and demands on nodes >= 64
only; variant 1 has variant 0's costs, so that variant 0's basis is dual feasible for it.  Per graph the data of the first solve and of the
steps a, b, c, e of test_redata_host.next_data, each from what the step before left, step b's supplies redrawn on nodes >= 64 too.

Everything a test needs of these graphs is asserted in wide_reference(), on the oracle's answers and the data alone.  Measured there
(Block Search; depth of the oracle's tree after the first solve per variant, the most non-tree search arcs across the cut of one tree arc among the caller's arcs, and
the first leaving node of the warm candidates over all steps):

  chorded path   depth 50..85 (above 64 in 4 variants), 157..183 crossing arcs, first leaving node >= 64 in 6 of 9; longest solve 544 pivots
  grid 12 x 12   depth 36..48, 148..163 crossing arcs, first leaving node >= 64 in 23 of 27; longest solve 405 pivots
  hub            depth 4, 165 crossing arcs, one node with 153..158 children, first leaving node >= 64 in 19 of 22; longest solve 421 pivots
  big grid       depth 126..147, 849..886 crossing arcs, first leaving node >= 64 in 11 of 12; longest solve 2 316 pivots; 174 176..175 360 bytes

(The first leaving node is counted where the oracle's basis has n - 1 tree arcs among the caller's arcs: 9, 27, 22 and 12 of the 32, 29, 27
and 16 warm candidates.)  The three small graphs take 25 360..39 552 bytes and lie in the LDS tier.  The shared row of the starts is a
primal start 5 times, a dual start 35 times and cold 100 times over the family."""
import functools

import numpy as np

from oracle import ns_oracle as O

import start_oracle as S
from test_batch_host import LDS_LIMITS, footprint, footprint_of, oracle_of
from test_batch_resolve_host import cold_reference, warm_after
from test_redata_host import expected_warm, next_data, violates
from test_uniform_host import TRACE, Topology, answer_of

SEED = 20261041                         # chosen on the CPU: the first seed from 20261021 on at which the oracle meets every floor of wide_reference()
WAVE = 64
STEPS = ("a", "b", "c", "e")            # the steps of test_redata_host.next_data that force dual pivots
PER, BIG_PER = 8, 4
NAMES = ("chorded path", "grid 12 x 12", "hub", "big grid")
PATH, GRID, HUB, BIG = range(4)
PATH_NODES, CHORDS, HUB_LEAVES = 130, 200, 160


def grid_arcs(side):
    """4-neighbour, both directions: 4 side (side - 1) arcs"""
    at = np.arange(side * side).reshape(side, side)
    pairs = np.concatenate([np.stack([at[:, :-1].ravel(), at[:, 1:].ravel()], 1), np.stack([at[:-1].ravel(), at[1:].ravel()], 1)])
    return side * side, np.concatenate([pairs[:, 0], pairs[:, 1]]).astype(np.int32), np.concatenate([pairs[:, 1], pairs[:, 0]]).astype(np.int32)


def big_side():
    """the smallest side at which a grid with a root link per node and not one artificial arc is above every LDS limit"""
    side = 2
    while footprint(4 * side * (side - 1) + side * side, side * side + 1) <= max(LDS_LIMITS):
        side += 1
    assert side in (29, 30)
    return side


def shapes():
    """per graph (n, src, tgt, (low, high) of the costs per arc, (low, high) of the capacities per arc, pairs of supply and demand nodes, variants)"""
    rng = np.random.default_rng([SEED, 0])
    n = PATH_NODES
    i = np.arange(n - 1)
    chords = set()
    while len(chords) < CHORDS:
        a, b = (int(v) for v in rng.integers(0, n, 2))
        if abs(a - b) > 1:
            chords.add((a, b))
    chords = np.array(sorted(chords), np.int32)
    src, tgt = np.concatenate([i, i + 1, chords[:, 0]]).astype(np.int32), np.concatenate([i + 1, i, chords[:, 1]]).astype(np.int32)
    on_path = np.arange(len(src)) < 2 * (n - 1)
    out = [(n, src, tgt, (np.where(on_path, 0, 30), np.where(on_path, 3, 60)), (np.where(on_path, 20, 4), np.where(on_path, 40, 12)), 10, PER)]
    n, src, tgt = grid_arcs(12)
    assert (n, len(src)) == (144, 528)
    out.append((n, src, tgt, (np.zeros(528, int), np.full(528, 20)), (np.full(528, 6), np.full(528, 16)), 12, PER))
    # four arcs between node 0 and every leaf, two each way (star() of test_uniform_validate_host.py), and a ring over the leaves
    spokes = 4 * HUB_LEAVES
    leaf = (np.arange(spokes) % HUB_LEAVES + 1).astype(np.int32)
    outward = (np.arange(spokes) // HUB_LEAVES) % 2 == 0
    ring = np.arange(HUB_LEAVES, dtype=np.int32)
    src = np.concatenate([np.where(outward, 0, leaf), ring + 1]).astype(np.int32)
    tgt = np.concatenate([np.where(outward, leaf, 0), (ring + 1) % HUB_LEAVES + 1]).astype(np.int32)
    spoke = np.arange(len(src)) < spokes
    assert len(src) == 800
    out.append((HUB_LEAVES + 1, src, tgt, (np.where(spoke, 1, 8), np.where(spoke, 10, 30)), (np.where(spoke, 10, 4), np.where(spoke, 24, 10)), 12, PER))
    side = big_side()
    n, src, tgt = grid_arcs(side)
    out.append((n, src, tgt, (np.zeros(len(src), int), np.full(len(src), 20)), (np.full(len(src), 10), np.full(len(src), 30)), 24, BIG_PER))
    return out


def pool_of(n):
    return np.arange(WAVE, n)


@functools.lru_cache(maxsize=None)
def wide_family():
    """((topology, supply type) ...) in the order of NAMES; LEQ on the chorded path, GEQ on the three graphs that share a ragged handle"""
    out = []
    for g, (n, src, tgt, cost_range, cap_range, pairs, count) in enumerate(shapes()):
        m = len(src)
        variants = []
        for k in range(count):
            rng = np.random.default_rng([SEED, 1, g, k])
            cost = np.random.default_rng([SEED, 2, g, 0 if k == 1 else k]).integers(cost_range[0], cost_range[1]).astype(np.int64)
            cap = rng.integers(cap_range[0], cap_range[1]).astype(np.int64)
            lower = np.minimum(np.where(rng.random(m) < 0.15, rng.integers(0, 4, m), 0), cap - 1).astype(np.int64)
            supply = np.zeros(n, np.int64)
            amount = rng.integers(1, 7, pairs)
            supply[rng.choice(pool_of(n), pairs, replace=False)] += amount
            supply[rng.choice(pool_of(n), pairs, replace=False)] -= rng.permutation(amount)
            assert np.all(cap >= 1) and np.all(lower >= 0) and not supply[:WAVE].any() and supply.sum() == 0
            variants.append(O.Problem(n, m, src, tgt, lower, lower + cap, cost, supply))
        out.append((Topology(n, src, tgt, variants, [False] * count), O.LEQ if g == PATH else O.GEQ))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def wide_chain():
    """per graph: (topology with the data of the first solve, (topology after step a, b, c, e)); every step starts from the data the one
    before it left"""
    out = []
    for g, (t, _) in enumerate(wide_family()):
        steps, now = [], t
        for s, name in enumerate(STEPS):
            now = Topology(t.n, t.src, t.tgt, [next_data(p, name, k, np.random.default_rng([SEED, 3, g, k, s]), pool=pool_of(t.n)) for k, p in enumerate(now.variants)],
                           now.zero_capacity)
            assert all(not (q.supply[:WAVE] != p.supply[:WAVE]).any() for p, q in zip(t.variants, now.variants))
            steps.append(now)
        out.append((t, tuple(steps)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def solved(g, s, k, rule):
    """(oracle, status) of variant k of graph g on the data of the first solve (s = 0) or after step s - 1"""
    (t, steps), (_, stype) = wide_chain()[g], wide_family()[g]
    o, st, _ = oracle_of(((t,) + steps)[s].variants[k], rule, stype, trace_cap=0)
    return o, st


def tree_of(o, p):
    """(parent[n + 1], depth[n + 1], child end per tree arc {arc: node}) of the oracle's tree; the root is node n"""
    par = o.parent()
    a = o.internal_arrays()
    A = o.all_arc_num
    src, tgt, state = a["src"][:A], a["tgt"][:A], a["state"][:A]
    depth = np.zeros(p.n + 1, np.int64)
    for v in range(p.n):
        u, d = v, 0
        while u != p.n:
            u, d = int(par[u]), d + 1
            assert d <= p.n
        depth[v] = d
    child = {}
    for e in np.flatnonzero(state == S.TREE):
        u, v = int(src[e]), int(tgt[e])
        assert par[u] == v or par[v] == u
        child[int(e)] = u if par[u] == v else v
    assert len(child) == p.n and sorted(child.values()) == list(range(p.n))
    return par, depth, child


def most_crossing(o, p):
    """the largest number of non-tree arcs of the search range across the cut of one tree arc among the caller's arcs (those get a range)"""
    par, depth, child = tree_of(o, p)
    a = o.internal_arrays()
    A, search = o.all_arc_num, o.search_arc_num
    src, tgt, state = a["src"][:A].astype(np.int64), a["tgt"][:A].astype(np.int64), a["state"][:A]
    off_tree = (np.arange(A) < search) & (state != S.TREE)
    # below[v, w]: w lies in the subtree of v -- the deepest nodes first, every node hands its set to its parent
    below = np.eye(p.n + 1, dtype=bool)
    for v in np.argsort(-depth[:p.n], kind="stable"):
        below[par[v]] |= below[v]
    return max(int(np.count_nonzero(off_tree & (below[c][src] != below[c][tgt]))) for e, c in child.items() if e < p.m)


def first_leaving(o, p, q, stype):
    """The node above which the first dual pivot's leaving arc lies when the basis the oracle `o` ended with on p meets the data of q:
    the largest violation max(-flow, flow - capacity) of the tree flows start_oracle derives, the lowest child node among equals.
    None: the basis has fewer than n - 1 tree arcs among the caller's arcs, or nothing is violated."""
    row = o.internal_arrays()["state"][:p.m]
    if S.count_tree(row) != p.n - 1:
        return None
    start = S.classify(q, stype, row)
    assert start.kind in (S.PRIMAL, S.DUAL), start.why
    _, _, child = tree_of(o, p)
    worst, at = 0, None
    for e in np.flatnonzero(row == S.TREE):
        f = start.flow[e]
        violation = max(-f, f - int(q.upper[e] - q.lower[e]))
        if violation > worst or (violation == worst and violation > 0 and child[int(e)] < at):
            worst, at = violation, child[int(e)]
    return at


@functools.lru_cache(maxsize=None)
def wide_reference(rule):
    """per graph, per topology of its chain (the first solve's, then every step's), per variant: (cold_reference(), answer_of()).
    The floors are asserted here, on the oracle's answers and the data alone; see the module's docstring for what they are."""
    out = []
    for g, ((t, steps), (_, stype)) in enumerate(zip(wide_chain(), wide_family())):
        tops = (t,) + steps
        refs = tuple(tuple((cold_reference(p, stype, rule), answer_of(p, rule, stype, trace_cap=TRACE)) for p in top.variants) for top in tops)
        longest = max(a[1] for row in refs for _, a in row)
        floor = 3 if g == BIG else 5
        leaving = []
        for s, name in enumerate(STEPS):
            candidates = forced = 0
            for k, q in enumerate(steps[s].variants):
                (before, answer_before), (after, _) = refs[s][k], refs[s + 1][k]
                assert after[0] != O.UNBOUNDED
                if expected_warm(before, q) and warm_after(after):
                    candidates += 1
                    forced += violates(q, answer_before[4])
                    o, st = solved(g, s, k, rule)
                    assert st == O.OPTIMAL
                    leaving.append(first_leaving(o, tops[s].variants[k], q, stype))
            print(f"{NAMES[g]}, rule {rule}, step {name}: {candidates} warm candidates, {forced} with a violated old optimum")
            assert candidates >= floor and forced >= 3, (NAMES[g], name, candidates, forced)
        known = [v for v in leaving if v is not None]
        high, low = sum(v >= WAVE for v in known), sum(v < WAVE for v in known)
        depths, crossing, children = [], [], []
        for k, p in enumerate(t.variants):
            o, st = solved(g, 0, k, rule)
            if st == O.OPTIMAL:
                depths.append(int(tree_of(o, p)[1].max()))
                children.append(int(np.bincount(tree_of(o, p)[0][:p.n]).max()))
                crossing.append(most_crossing(o, p))
        prints = [footprint_of(p, stype) for top in tops for p in top.variants]
        print(f"{NAMES[g]}, rule {rule}: longest solve {longest} pivots; tree depth {min(depths)}..{max(depths)} (above {WAVE} in {sum(d > WAVE for d in depths)} variants); "
              f"crossing arcs {min(crossing)}..{max(crossing)}; most children of one node {min(children)}..{max(children)}; first leaving node >= {WAVE} in {high} of {len(known)} (of {len(leaving)} warm candidates); "
              f"workspace {min(prints)}..{max(prints)} bytes")
        assert longest < TRACE
        assert high >= 3 and low >= 1, (NAMES[g], high, low)
        assert min(crossing) >= WAVE, (NAMES[g], crossing)
        assert g != PATH or sum(d > WAVE for d in depths) >= 2, depths
        assert g != HUB or min(children) > 2 * WAVE, children
        assert g != BIG or (len(depths) == t.count and min(depths) > WAVE), depths
        if g == BIG:
            assert min(prints) > max(LDS_LIMITS) and footprint(t.m + t.n, t.n + 1) > max(LDS_LIMITS)
        else:
            assert 0 < min(prints) and max(prints) <= max(LDS_LIMITS), prints
        out.append(refs)
    return tuple(out)
    return tuple(out)


# ---- cost ranges
@functools.lru_cache(maxsize=None)
def wide_ranges(rule):
    """per graph ranges_oracle.reference_rows() of the first solve: the brute force on the oracle's own basis"""
    import ranges_oracle as R
    out = []
    for g, (t, _) in enumerate(wide_family()):
        rows = R.reference_rows([(p,) + solved(g, 0, k, rule) for k, p in enumerate(t.variants)])
        print(f"{NAMES[g]}, rule {rule}, ranges: {rows[4]}")
        assert rows[4]["ranged"] >= (3 if g == BIG else 5) and rows[4]["both_finite"] >= 100, rows[4]
        out.append(rows)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def meaning_problem():
    """test_ranges_host.meaning_problem() on the grid of 12 x 12: a circulation with costs from -6 and every capacity finite, the first
    seed the oracle solves to Optimal after at least 10 pivots"""
    import ranges_oracle as R
    n, src, tgt = grid_arcs(12)
    m = len(src)
    for seed in range(64):
        rng = np.random.default_rng([SEED, 4, seed])
        p = O.Problem(n, m, src, tgt, np.zeros(m, np.int64), rng.integers(1, 12, m), rng.integers(-6, 20, m), np.zeros(n, np.int64))
        o, st, _ = oracle_of(p, O.RULE_BLOCK)
        if R.is_ranged(o, st, p) and o.n_pivots >= 10:
            assert o.all_arc_num == p.m + p.n
            return p, o
    raise AssertionError("no ranged instance among 64 seeds")


# ---- starts from a given basis
@functools.lru_cache(maxsize=None)
def shared_row(g, rule):
    """the basis the oracle ends the first variant's first solve with, as cost_ranges exports it: one row for all variants of the graph"""
    import ranges_oracle as R
    p = wide_family()[g][0].variants[0]
    o, st = solved(g, 0, 0, rule)
    assert R.is_ranged(o, st, p)
    return np.ascontiguousarray(o.internal_arrays()["state"][:p.m].astype(np.int8))


@functools.lru_cache(maxsize=None)
def start_classes(rule):
    """per graph, per topology of its chain, per variant: the class start_oracle predicts for shared_row().  Asserted on that alone: over
    the family every class occurs, and variant 0 starts primal on its own data."""
    out = []
    for g, ((t, steps), (_, stype)) in enumerate(zip(wide_chain(), wide_family())):
        row = shared_row(g, rule)
        out.append(tuple(tuple(S.classify(p, stype, row).kind for p in top.variants) for top in (t,) + steps))
        assert out[-1][0][0] == S.PRIMAL
    kinds = [kind for graph in out for top in graph for kind in top]
    count = {kind: kinds.count(kind) for kind in (S.PRIMAL, S.DUAL, S.COLD)}
    print(f"starts from the first variant's basis, rule {rule}: {count}")
    assert min(count.values()) >= 1, count
    return tuple(out)


@functools.lru_cache(maxsize=None)
def hostile_case():
    """(topology, supply type, row with a cycle, row of the forward path) on the chorded path.  The forward path: every arc i -> i + 1
    TREE, all else LOWER -- one tree of depth 129 below node 0.  The cycle: the same with the chord that spans the most nodes TREE as
    well, which closes a cycle of more than 64 arcs.  The topology: the 8 variants and a ninth without lower bounds that ships 5 units
    from node 64 to node 129, which the forward path carries inside its bounds.  Asserted on start_oracle alone: the cycle is cold by
    its rule everywhere, the forward path is a primal start for the ninth."""
    t, stype = wide_family()[PATH]
    path_arcs = 2 * (PATH_NODES - 1)
    forward = np.full(t.m, S.LOWER, np.int8)
    forward[:PATH_NODES - 1] = S.TREE
    assert np.array_equal(t.src[:PATH_NODES - 1] + 1, t.tgt[:PATH_NODES - 1])
    chord = path_arcs + int(np.argmax(np.abs(t.src[path_arcs:] - t.tgt[path_arcs:])))
    assert abs(int(t.src[chord]) - int(t.tgt[chord])) + 1 > WAVE
    cycle = forward.copy()
    cycle[chord] = S.TREE
    p = t.variants[0]
    supply = np.zeros(t.n, np.int64)
    supply[WAVE], supply[t.n - 1] = 5, -5
    top = Topology(t.n, t.src, t.tgt, t.variants + (O.Problem(p.n, p.m, p.src, p.tgt, np.zeros(p.m, np.int64), p.upper - p.lower, p.cost, supply),), [False] * (t.count + 1))
    assert all(S.classify(q, stype, cycle).why == "the tree arcs hold a cycle" for q in top.variants)
    assert S.classify(top.variants[-1], stype, forward).kind == S.PRIMAL
    return top, stype, cycle, forward
