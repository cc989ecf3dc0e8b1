"""Supply and bound ranges by hand from the oracle's own basis: the reference of test_data_ranges_host.py and test_data_ranges_gpu.py.

Independent of the library, in the way ranges_oracle.py is: it reads only Oracle.internal_arrays(), Oracle.flow() and the problem's bounds
after a solve.  The arcs with state 0 are the tree; parents come from a breadth-first search from the root over those arcs alone; the
room of a node's tree arc comes from the oracle's flow and the CALLER's bounds (flow - lower to fall, upper - flow to rise, no limit
without an upper bound), 0 both ways for a root link or an artificial arc; a transfer climbs the two parent chains to their meeting
point, the deeper end first -- by depth, never by subtree sizes, so it does not share the rule of the walk it checks.

The definition (include/mcf_hip.h): T(a -> b) is the least room in the direction of travel over the tree path from a to b.  A tree arc
may fall and rise by its own rooms; a non-tree arc may fall by T(tail -> head) and rise by T(head -> tail), not clipped by its own
capacity; a pair (a, b) ships T(a -> b) forth and T(b -> a) back, INF twice where a == b, -1 twice where an id is out of range."""
import functools

import numpy as np

from oracle import ns_oracle as O

import ranges_oracle as R
import wide_graphs as W
from test_batch_host import fuzz_cases, fuzz_reference, oracle_of
from test_redata_host import redata_family
from test_uniform_host import Topology

INF = R.INF
WAVE = 64
DRAWN = 100                             # drawn pairs per graph
# chosen on the CPU: the first seed from 20261101 on at which the drawn pairs meet the floors of pairs_of() and structured_rows() on
# every graph (both of the first seed's lists already do)
PAIR_SEED = 20261101


def pairs_of(tag, n, src, tgt):
    """The pairs asked of one graph, int32 [k, 2]: DRAWN drawn pairs -- on a graph wider than a wave a quarter each with both ends below
    node 64, both from it on, and one end on either side --, one pair (a, a), one pair with an id out of range on either side, and both
    ends of every third arc (where such an arc is not in the tree its ship row must equal its flow row)."""
    rng = np.random.default_rng([PAIR_SEED] + list(tag))
    if n > WAVE:
        low, high = lambda k: rng.integers(0, WAVE, k), lambda k: rng.integers(WAVE, n, k)
        q = DRAWN // 4
        drawn = np.concatenate([np.stack([low(q), low(q)], 1), np.stack([high(q), high(q)], 1), np.stack([low(q), high(q)], 1), np.stack([high(q), low(q)], 1)])
        assert np.any((drawn[:, 0] < WAVE) & (drawn[:, 1] >= WAVE)) and np.any((drawn[:, 0] >= WAVE) & (drawn[:, 1] < WAVE))
    else:
        drawn = rng.integers(0, max(n, 1), (DRAWN, 2))
    same = int(rng.integers(0, max(n, 1)))
    special = np.array([[same, same], [n, 0], [0, -1]])
    third = np.stack([src[::3], tgt[::3]], 1) if len(src) else np.zeros((0, 2), np.int64)
    return np.ascontiguousarray(np.concatenate([drawn, special, third]).astype(np.int32))


def third_arcs(m):
    """(arc ids, their positions in pairs_of()'s list)"""
    arcs = np.arange(0, m, 3)
    return arcs, DRAWN + 3 + np.arange(len(arcs))


class Tree:
    """The oracle's basis as the definition needs it: parent, depth and the two rooms per node."""

    def __init__(self, o, p):
        n, m, A = p.n, p.m, o.all_arc_num
        a = o.internal_arrays()
        src, tgt, state = a["src"][:A].astype(np.int64), a["tgt"][:A].astype(np.int64), a["state"][:A]
        tree = np.flatnonzero(state == 0)
        assert len(tree) == n, (len(tree), n)
        flow = o.flow().astype(np.int64)
        fall = [int(v) for v in flow - p.lower]
        rise = [INF if int(u) == O.INF_CAP else int(u) - int(f) for u, f in zip(p.upper, flow)]
        assert all(v >= 0 for v in fall) and all(v >= 0 for v in rise)
        adj = [[] for _ in range(n + 1)]
        for e in tree:
            adj[src[e]].append((int(tgt[e]), int(e)))
            adj[tgt[e]].append((int(src[e]), int(e)))
        self.n, self.m = n, m
        self.parent, self.depth = [-1] * (n + 1), [-1] * (n + 1)
        self.out, self.into = [0] * (n + 1), [0] * (n + 1)
        self.by_root = [False] * (n + 1)                                    # the node's tree arc is a root link or an artificial arc
        self.depth[n] = 0
        queue = [n]
        for v in queue:
            for w, e in adj[v]:
                if self.depth[w] >= 0:
                    continue
                self.parent[w], self.depth[w] = v, self.depth[v] + 1
                if e < m:
                    leaves = int(src[e]) == w                               # the arc leaves w towards its parent
                    self.out[w], self.into[w] = (rise[e], fall[e]) if leaves else (fall[e], rise[e])
                else:
                    self.by_root[w] = True
                queue.append(w)
        assert min(self.depth) >= 0, "the arcs with state 0 do not span the nodes"
        self.state, self.src, self.tgt, self.fall, self.rise = state[:m].astype(np.int8), src[:m], tgt[:m], fall, rise

    def transfer(self, a, b):
        """(T(a -> b), T(b -> a), hops, the path passes a root link or an artificial arc)"""
        forth = back = INF
        hops, by_root = 0, False
        parent, depth, out, into = self.parent, self.depth, self.out, self.into
        while a != b:
            if depth[a] >= depth[b]:
                forth, back, by_root, a = min(forth, out[a]), min(back, into[a]), by_root or self.by_root[a], parent[a]
            else:
                forth, back, by_root, b = min(forth, into[b]), min(back, out[b]), by_root or self.by_root[b], parent[b]
            hops += 1
        return forth, back, hops, by_root


TALLY = ("ranged", "both_finite", "zero_by_a_tree_arc", "zero_by_the_root", "infinite", "own_capacity", "longest_walk")


def rows_of(o, p, pairs, tally):
    """(arc_state[m] int8, flow_down[m], flow_up[m], ship_forth[k], ship_back[k]) of the basis oracle `o` ended with on problem `p`"""
    t = Tree(o, p)
    down, up = np.empty(p.m, np.int64), np.empty(p.m, np.int64)
    for e in range(p.m):
        if t.state[e] == 0:
            down[e], up[e] = t.fall[e], t.rise[e]
            continue
        forth, back, hops, by_root = t.transfer(int(t.src[e]), int(t.tgt[e]))
        down[e], up[e] = forth, back
        tally["both_finite"] += 0 < forth < INF and 0 < back < INF
        if forth == 0 or back == 0:
            tally["zero_by_the_root" if by_root else "zero_by_a_tree_arc"] += 1
        tally["infinite"] += forth == INF or back == INF
        tally["own_capacity"] += t.state[e] == 1 and p.upper[e] != O.INF_CAP and int(p.upper[e] - p.lower[e]) < back
        tally["longest_walk"] = max(tally["longest_walk"], hops)
    forth, back = np.empty(len(pairs), np.int64), np.empty(len(pairs), np.int64)
    for k, (a, b) in enumerate(pairs.tolist()):
        if not (0 <= a < p.n and 0 <= b < p.n):
            forth[k] = back[k] = -1
            continue
        forth[k], back[k], hops, _ = t.transfer(a, b)
        tally["longest_walk"] = max(tally["longest_walk"], hops)
    return t.state, down, up, forth, back


def reference_rows(cases):
    """cases: ((problem, oracle, status, pairs) ...) -> dict of ranged [count], arc_state, flow_down, flow_up flat over the instances'
    arcs, ship_forth, ship_back flat over their pairs, ship_rows [count + 1], and the tally of what the non-tree arcs of the ranged
    instances cover"""
    parts = {name: [] for name in ("arc_state", "flow_down", "flow_up", "ship_forth", "ship_back")}
    ranged, ship_rows = [], [0]
    tally = dict.fromkeys(TALLY, 0)
    for p, o, st, pairs in cases:
        r = R.is_ranged(o, st, p)
        ranged.append(int(r))
        ship_rows.append(ship_rows[-1] + len(pairs))
        if r:
            tally["ranged"] += 1
            rows = rows_of(o, p, pairs, tally)
        else:
            rows = (np.zeros(p.m, np.int8),) + (np.zeros(p.m, np.int64),) * 2 + (np.zeros(len(pairs), np.int64),) * 2
        for name, row in zip(parts, rows):
            parts[name].append(row)
    out = {name: np.concatenate(v).astype(np.int8 if name == "arc_state" else np.int64) if v else np.zeros(0, np.int8 if name == "arc_state" else np.int64)
           for name, v in parts.items()}
    out["ranged"], out["ship_rows"], out["tally"] = np.array(ranged, np.int32), np.array(ship_rows, np.int64), tally
    out["ranged_arcs"] = np.repeat(out["ranged"] != 0, [c[0].m for c in cases]) if cases else np.zeros(0, bool)
    assert np.all(out["flow_down"] >= 0) and np.all(out["flow_up"] >= 0)
    return out


def assert_floors(tally, what, infinite=True):
    """What every family must cover, on the oracle's side alone.  A side equal to 0 comes about in two ways and the tally names each: a
    tree arc of the caller's on the path has no room that way (degenerate, or full), or the path passes the root."""
    print(f"data ranges, {what}: {tally}")
    assert tally["both_finite"] >= 20 and tally["zero_by_a_tree_arc"] + tally["zero_by_the_root"] >= 20 and tally["own_capacity"] >= 10, (what, tally)
    assert tally["zero_by_a_tree_arc"] >= 1 and tally["zero_by_the_root"] >= 1, (what, tally)
    assert not infinite or tally["infinite"] >= 10, (what, tally)


def bounds_table(rows, lower, upper):
    """The table of include/mcf_hip.h applied to reference rows, arc by arc: (lower may fall by, lower may rise by, upper may fall by,
    upper may rise by).  lower, upper: flat like the rows.  `ranged_arcs`: per arc whether its instance is ranged."""
    out = np.zeros((4, len(lower)), np.int64)
    for e, (st, d, u, lo, hi, r) in enumerate(zip(rows["arc_state"].tolist(), rows["flow_down"].tolist(), rows["flow_up"].tolist(), lower.tolist(), upper.tolist(),
                                                  rows["ranged_arcs"].tolist())):
        if not r:
            continue
        cap = INF if hi == O.INF_CAP else hi - lo
        out[:, e] = {1: (d, min(u, cap), cap, INF), -1: (INF, cap, min(d, cap), u), 0: (INF, d, u, INF)}[st]
    return out


# ---- the families
@functools.lru_cache(maxsize=None)
def redata_rows(rule):
    """per graph of test_redata_host.redata_family(): (pairs, reference_rows() of its variants' first solve); floors over the family"""
    out = []
    tally = dict.fromkeys(TALLY, 0)
    for j, (t, stype) in enumerate(redata_family()):
        pairs = pairs_of((1, j), t.n, t.src, t.tgt)
        rows = reference_rows([(p,) + oracle_of(p, rule, stype, trace_cap=0)[:2] + (pairs,) for p in t.variants])
        for k in TALLY:
            tally[k] = max(tally[k], rows["tally"][k]) if k == "longest_walk" else tally[k] + rows["tally"][k]
        out.append((pairs, rows))
    assert_floors(tally, f"re-data family, rule {rule}")
    assert all(0 < rows["ranged"].sum() < t.count for (t, _), (_, rows) in zip(redata_family(), out))        # not-ranged instances among them
    return tuple(out)


@functools.lru_cache(maxsize=None)
def fuzz_pairs():
    return tuple(pairs_of((2, i), p.n, p.src, p.tgt) for i, (p, _) in enumerate(fuzz_cases()))


@functools.lru_cache(maxsize=None)
def fuzz_rows(rule):
    """reference_rows() of the adversarial batch (every instance its own graph and supply type); its not-ranged instances give zero rows"""
    rows = reference_rows([(p, o, st, pairs) for (p, _), (o, st, _), pairs in zip(fuzz_cases(), fuzz_reference(rule), fuzz_pairs())])
    assert_floors(rows["tally"], f"adversarial batch, rule {rule}")
    assert rows["tally"]["ranged"] >= 100 and np.sum(rows["ranged"] == 0) >= 100
    return rows


@functools.lru_cache(maxsize=None)
def wide_pairs():
    return tuple(pairs_of((3, g), t.n, t.src, t.tgt) for g, (t, _) in enumerate(W.wide_family()))


@functools.lru_cache(maxsize=None)
def wide_rows(rule):
    """per graph of wide_graphs.wide_family(): reference_rows() of its variants' first solve.  Every capacity of this family is finite
    and no graph has a self loop, so no side of it is infinite: structured_rows() covers that floor on a graph of the same width."""
    out = []
    tally = dict.fromkeys(TALLY, 0)
    for g, (t, _) in enumerate(W.wide_family()):
        rows = reference_rows([(p,) + W.solved(g, 0, k, rule) + (wide_pairs()[g],) for k, p in enumerate(t.variants)])
        print(f"data ranges, {W.NAMES[g]}, rule {rule}: {rows['tally']}")
        assert rows["tally"]["ranged"] >= (3 if g == W.BIG else 5)
        assert g != W.PATH or rows["tally"]["longest_walk"] > WAVE, rows["tally"]
        for k in TALLY:
            tally[k] = max(tally[k], rows["tally"][k]) if k == "longest_walk" else tally[k] + rows["tally"][k]
        out.append(rows)
    assert_floors(tally, f"wide family, rule {rule}", infinite=False)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def structured_family():
    """(topology, supply type): the chorded path of wide_graphs with every chord UNCAPACITATED and a self loop on every tenth node, 8
    variants.  Added because the wide family cannot meet the floor of infinite sides: all its capacities are finite and it has no self
    loop, so every walk meets a finite room.  Here a chord in the tree has no limit to rise, and a self loop walks nothing."""
    t, stype = W.wide_family()[W.PATH]
    loops = np.arange(0, t.n, 10, dtype=np.int32)
    src, tgt = np.concatenate([t.src, loops]).astype(np.int32), np.concatenate([t.tgt, loops]).astype(np.int32)
    on_path = np.arange(t.m) < 2 * (W.PATH_NODES - 1)
    variants = []
    for k, p in enumerate(t.variants):
        rng = np.random.default_rng([PAIR_SEED, 4, k])
        lower = np.concatenate([p.lower, np.zeros(len(loops), np.int64)])
        upper = np.concatenate([np.where(on_path, p.upper, O.INF_CAP), rng.integers(1, 9, len(loops))]).astype(np.int64)
        cost = np.concatenate([np.where(on_path, p.cost, p.cost // 8), rng.integers(1, 9, len(loops))]).astype(np.int64)        # cheap chords: many enter the tree
        variants.append(O.Problem(t.n, len(src), src, tgt, lower, upper, cost, p.supply))
    return Topology(t.n, src, tgt, variants, [False] * len(variants)), stype


@functools.lru_cache(maxsize=None)
def structured_rows(rule):
    t, stype = structured_family()
    pairs = pairs_of((4,), t.n, t.src, t.tgt)
    rows = reference_rows([(p,) + oracle_of(p, rule, stype, trace_cap=0)[:2] + (pairs,) for p in t.variants])
    assert_floors(rows["tally"], f"chorded path without chord capacities, rule {rule}")
    assert rows["tally"]["ranged"] >= 5
    return pairs, rows
