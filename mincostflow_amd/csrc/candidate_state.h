// candidate_state.h -- the decision state of the resident engine's exact candidate cache and the pure functions on it: plain C++, no HIP, so
// that tools/candidate_state_check.cpp can run every rule of it on a CPU against a brute-force scan.  engine.hip derives mcf_engine from
// CandState and keeps what talks to the device (mailbox, sync and blind lists, posting, polling: candidate_cache.hip.h).  DESIGN.md 3.4.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

#include "common.h"

// Best Eligible picks argmin (c, arc) over ALL search arcs with the CURRENT potentials (NS.cs:1644-1667).  A pivot changes the
// potentials of one subtree and one or two states, so only arcs that touch those nodes change their key; every other arc keeps the key
// the last device search saw.  A device search returns a sorted candidate list that is COMPLETE below a threshold (every eligible arc
// with a smaller key is on it) as of the moment it was posted (its epoch).  The host keeps
//   * the list, and for every node / arc the epoch of its last change: a list entry is CLEAN when nothing of it changed after the list's epoch;
//   * a min-heap with the current keys of the arcs touched since that can still win (see INVARIANT; re-evaluated from the host mirrors when
//     they are touched; at most kCandMaxNodes nodes' adjacency per pivot -- a bigger subtree is not evaluated here, the device searches instead).
// Then, exactly:   min over untouched arcs = first clean list entry (all unlisted untouched arcs lie above the threshold)
//                  min over touched arcs   = top of the heap
// and the entering arc is the smaller of the two -- the reference's pivot, arc for arc (every parity test runs with the cache on and off).
//
// INVARIANT of the heap: after every push and every install it holds only eligible arcs touched after snap_at (current or outdated versions:
// deletion is lazy), and while no refresh is in flight each entry's key also lies below cand_thr in the (c, p) order of cand_key_less.  A
// touched arc that cannot beat the threshold is never kept: no decision would read it (cand_admit_all has the argument, cand_decide its use).
constexpr uint32_t kCandNone = 0xFFFFFFFFu;     // "no arc" in a key (kernels.hip.h: kNone)
constexpr int kCandMaxNodes = 256;              // sweep on config 3 (profiles/r03_cand_nodes_sweep.txt): 192-384 nodes evaluated on the host beat a device round trip
constexpr int64_t kCandDegreePerNode = 8;       // adjacency entries re-evaluated per pivot at most: this many per node of kCandMaxNodes

struct CandState {
    struct AdjEnt { int32_t arc; uint32_t other; int64_t cost; };  // other: the arc's second end point (bits 0-28), the arc's state + 1 (bits 29-30), bit 31 set when THIS node is the arc's target
    struct CandKey { int64_t c; uint32_t p; };
    // c, p: the key; at: the epoch of the touch that pushed it; u, v: the arc's end points.  An entry is CURRENT while nothing of its arc was
    // touched after `at` (arc_at[p], node_at[u], node_at[v] all <= at): a later touch either pushed a newer entry or was a skipped one, i.e. a
    // gap -- and no list older than a gap is ever judged against the heap (cand_decide).  (Rounds 1-2 kept a version counter per arc and
    // bumped it for every arc an evaluation looked at: 80 scattered read-modify-writes per pivot on the headline workload.)
    struct HeapEnt { int64_t c; uint32_t p; uint32_t at; int32_t u, v; };

    bool cand_valid = false;
    // every change carries the number of the search it precedes ("epoch"); a snapshot taken at epoch P knows all changes stamped <= P
    mcf::hvec<uint32_t> node_at, arc_at;        // epoch of the node's last potential change / the arc's last state change
    uint32_t cand_now = 1;                        // epoch of the changes that are arriving
    uint32_t snap_at = 0;                         // epoch the candidate list reflects
    uint32_t heap_gap = 0;                        // latest epoch whose changes were NOT evaluated into the heap (a subtree too big to evaluate here)
    std::vector<HeapEnt> heap;                    // min-heap of the keys of the arcs touched since that can still win (lazy deletion through the epochs)
    std::vector<int32_t> pivot_nodes, pivot_arcs; // touched since the last search: evaluated when the next search begins (all values final by then)
    int64_t pivot_degree = 0;
    bool pivot_overflow = false;
    std::vector<CandKey> cand_list;               // sorted; complete below cand_thr as of snap_at
    std::vector<int32_t> cand_ends;               // the end points of the listed arcs (2 per entry), looked up once when the list is installed
    size_t cand_ptr = 0;
    // what cand_decide found valid last time: the heap's top entry (tp_*) and the list's first clean entry (hd_*), remembered with their arc
    // and end points so that a touch of any of them (cand_note_node / cand_note_arc) can revoke it
    bool tp_ok = false, hd_ok = false;
    int32_t tp_a = -1, tp_u = -1, tp_v = -1, hd_a = -1, hd_u = -1, hd_v = -1;
    uint32_t tp_at = 0;
    size_t hd_ptr = 0;
    CandKey cand_thr{0, kCandNone};               // p == kCandNone: the list holds every eligible arc
    bool async_posted = false;                    // a refresh is on its way while the host keeps answering from the current list
    size_t heap_compact_above = 1u << 18;         // heap entries above which the stale ones are swept out (MCF_HIP_CAND_HEAP_COMPACT: tests)
    // push: eligible touched keys offered to the heap; admit: those it kept; sweeps: over a non-empty heap, at install or by size
    int64_t n_heap_push = 0, n_heap_admit = 0, n_heap_pop = 0, n_heap_sweeps = 0;
};

// what an evaluation reads: the engine's host mirrors of the search arcs, their lists per node, and the current potentials
struct CandGraph {
    const int32_t *adj_start;
    const CandState::AdjEnt *adj;
    const int32_t *src, *tgt;
    const int64_t *cost;
    const int8_t *state;
    const int64_t *pi;
};

inline bool cand_key_less(const CandState::CandKey &a, const CandState::CandKey &b) { return a.c < b.c || (a.c == b.c && a.p < b.p); }
struct CandHeapAfter {        // std::*_heap keep the LARGEST on top: order by "comes later"
    bool operator()(const CandState::HeapEnt &a, const CandState::HeapEnt &b) const { return b.c < a.c || (b.c == a.c && b.p < a.p); }
};

// a potential change of node u (the mirrors already hold the new value); true: its first in this epoch
inline bool cand_state_note_node(CandState *e, int u, const int32_t *adj_start)
{
    // what cand_decide verified last time stays verified until one of ITS nodes is touched (four compares here instead of six scattered loads there)
    if ((u == e->tp_u) | (u == e->tp_v)) e->tp_ok = false;
    if ((u == e->hd_u) | (u == e->hd_v)) e->hd_ok = false;
    if (e->node_at[u] == e->cand_now) return false;
    e->node_at[u] = e->cand_now;
    if (!e->pivot_overflow) {
        e->pivot_nodes.push_back(u);
        e->pivot_degree += adj_start[u + 1] - adj_start[u];
        if ((int)e->pivot_nodes.size() > kCandMaxNodes || e->pivot_degree > kCandDegreePerNode * kCandMaxNodes) e->pivot_overflow = true;
    }
    return true;
}
// a state change of arc a; true: its first in this epoch
inline bool cand_state_note_arc(CandState *e, int a)
{
    if (a == e->tp_a) e->tp_ok = false;
    if (a == e->hd_a) e->hd_ok = false;
    if (e->arc_at[a] == e->cand_now) return false;
    e->arc_at[a] = e->cand_now;
    e->pivot_arcs.push_back(a);
    return true;
}

inline bool cand_heap_current(const CandState *e, const CandState::HeapEnt &t)
{
    return ((int)(e->arc_at[t.p] <= t.at) & (int)(e->node_at[t.u] <= t.at) & (int)(e->node_at[t.v] <= t.at)) != 0;      // three independent loads: they miss together
}

// The admission rule.  cand_decide reads a heap entry in two ways only: against the first clean list entry, whose key lies below cand_thr, and
// against cand_thr itself once the list has run out.  A touched arc whose key is not below cand_thr can therefore not change a decision
// while that list is in force, and it is not kept.  Which list is that?  An entry pushed while no refresh is in flight carries an epoch <=
// the next post's, so the install of that post outdates it whatever its threshold is: the current threshold is the only one it ever
// meets.  An entry pushed while a refresh IS in flight (async_posted) outlives the install and will be judged under the coming list's
// threshold, which is not known yet and may be higher than this one: everything is admitted then, and the install sorts it out
// (cand_sweep_heap).  Without a list (cand_valid unset) or with a complete one (no threshold) there is nothing to filter against.
inline bool cand_admit_all(const CandState *e) { return e->async_posted || !e->cand_valid || e->cand_thr.p == kCandNone; }

// Sweeps the heap.  By size (cand_absorb_pivot): drops what lazy deletion left behind.  At install (cand_install, after snap_at and cand_thr
// are set): drops the entries the new list outdates (at <= snap_at) and those that cannot beat the new threshold.
inline void cand_sweep_heap(CandState *e, bool install)
{
    if (e->heap.empty()) return;
    size_t keep = 0;
    if (install) {
        const bool all = e->cand_thr.p == kCandNone;
        for (size_t i = 0; i < e->heap.size(); ++i) {
            const CandState::HeapEnt &t = e->heap[i];
            if (t.at > e->snap_at && (all || cand_key_less(CandState::CandKey{t.c, t.p}, e->cand_thr))) e->heap[keep++] = t;
        }
    } else {
        for (size_t i = 0; i < e->heap.size(); ++i)
            if (cand_heap_current(e, e->heap[i])) e->heap[keep++] = e->heap[i];
    }
    e->heap.resize(keep);
    std::make_heap(e->heap.begin(), e->heap.end(), CandHeapAfter());
    e->n_heap_sweeps += 1;
}

inline void cand_push(CandState *e, const CandGraph &g, int a)
{
    const int st = g.state[a];
    if (st == 0) return;
    const int64_t *pi = g.pi;
    const int32_t u = g.src[a], v = g.tgt[a];
    const int64_t d = g.cost[a] + pi[u] - pi[v];
    const int64_t rc = st > 0 ? d : -d;
    if (rc >= 0) return;
    e->n_heap_push += 1;
    if (!cand_admit_all(e) && !cand_key_less(CandState::CandKey{rc, (uint32_t)a}, e->cand_thr)) return;
    e->n_heap_admit += 1;
    e->heap.push_back(CandState::HeapEnt{rc, (uint32_t)a, e->cand_now, u, v});
    std::push_heap(e->heap.begin(), e->heap.end(), CandHeapAfter());
}

// all changes of the pivot are in: bring the heap up to date (or note that it is not)
inline void cand_absorb_pivot(CandState *e, const CandGraph &g)
{
    if (e->pivot_overflow) {
        e->heap_gap = e->cand_now;
        // arcs next to the moved nodes keep heap entries of older versions: they must not be taken for current ones
        // (entries are only trusted for snapshots taken at or after heap_gap, and those know the arcs' present keys -- see cand_decide)
    } else {
        const int64_t *pi = g.pi;
        const uint32_t now = e->cand_now;
        const bool admit_all = cand_admit_all(e);            // nothing here changes what the rule reads
        const CandState::CandKey thr = e->cand_thr;
        int64_t offered = 0, admitted = 0;
        // first the addresses the evaluation will miss on (version counters and far potentials live in arrays of the graph's size) ...
        for (int u : e->pivot_nodes)
            for (int i = g.adj_start[u], hi = g.adj_start[u + 1]; i < hi; ++i) {
                const CandState::AdjEnt &x = g.adj[i];
                __builtin_prefetch(&pi[x.other & 0x1FFFFFFFu]);
            }
        for (int u : e->pivot_nodes) {
            const int64_t pu = pi[u];
            // everything an evaluation needs sits in the entry except the other end's potential and the arc's version counter; an arc
            // between two moved nodes is evaluated twice (the second entry outdates the first), which is cheaper than remembering it
            for (int i = g.adj_start[u], hi = g.adj_start[u + 1]; i < hi; ++i) {
                const CandState::AdjEnt &x = g.adj[i];
                const int st = (int)((x.other >> 29) & 3u) - 1;
                if (st == 0) continue;
                const int32_t other = (int32_t)(x.other & 0x1FFFFFFFu);
                const int64_t po = pi[other];
                const int64_t d = (x.other >> 31) ? x.cost + po - pu : x.cost + pu - po;
                const int64_t rc = st > 0 ? d : -d;
                if (rc >= 0) continue;
                offered += 1;
                if (!admit_all && !cand_key_less(CandState::CandKey{rc, (uint32_t)x.arc}, thr)) continue;      // cannot change a decision (cand_admit_all)
                admitted += 1;
                e->heap.push_back(CandState::HeapEnt{rc, (uint32_t)x.arc, now, u, other});
                std::push_heap(e->heap.begin(), e->heap.end(), CandHeapAfter());
            }
        }
        e->n_heap_push += offered;
        e->n_heap_admit += admitted;
        for (int a : e->pivot_arcs) cand_push(e, g, a);
    }
    e->pivot_nodes.clear();
    e->pivot_arcs.clear();
    e->pivot_degree = 0;
    e->pivot_overflow = false;
    if (e->heap.size() > e->heap_compact_above) cand_sweep_heap(e, false);      // bounds the heap while a refresh is in flight
}

// true: *win holds the entering arc's key (p == kCandNone: the scan would find nothing either) without asking the device
inline bool cand_decide(CandState *e, CandState::CandKey *out)
{
    // the heap knows every change after snap_at only if none of them was skipped (heap_gap) -- and after a gap the entries of the arcs
    // next to the skipped nodes are outdated without being marked so; a snapshot at or after the gap makes all of that irrelevant:
    // an arc touched at or before snap_at is judged by the list (or lies above the threshold), whatever the heap says about it
    if (!e->cand_valid || e->snap_at < e->heap_gap) return false;
    CandState::CandKey best_d{0, kCandNone};
    while (!e->heap.empty()) {
        const CandState::HeapEnt &t = e->heap.front();
        const uint32_t a = t.p;
        // the entry that was found current last time, and none of its arc's three stamps has been touched since (cand_note_node / _arc)
        if (e->tp_ok && (int32_t)a == e->tp_a && t.at == e->tp_at) { best_d = CandState::CandKey{t.c, a}; break; }
        // current version, and touched after the snapshot (an arc last touched before it is the list's business).  While an entry is
        // current its own epoch is the arc's last touch: a later touch either pushed a newer entry or was a skipped one, i.e. a gap -- and
        // no list older than a gap gets here (above), so both the entry's epoch and the true one are <= snap_at then.
        const bool after = t.at > e->snap_at;
        if (after && cand_heap_current(e, t)) {
            e->tp_ok = true; e->tp_a = (int32_t)a; e->tp_at = t.at; e->tp_u = t.u; e->tp_v = t.v;
            best_d = CandState::CandKey{t.c, a};
            break;
        }
        std::pop_heap(e->heap.begin(), e->heap.end(), CandHeapAfter());
        e->heap.pop_back();
        e->n_heap_pop += 1;
    }
    // best_d is the smallest ADMITTED touched key; the smallest of all touched keys may be a rejected one, and the outcome is the same: with
    // a clean list entry, head < cand_thr <= any rejected key, so a rejected key never wins; with the list run out, a rejected key never
    // satisfied best_d < cand_thr anyway (and a complete list, or none, rejects nothing)
    while (e->cand_ptr < e->cand_list.size()) {
        if (e->hd_ok && e->hd_ptr == e->cand_ptr) break;     // verified clean last time, untouched since
        const uint32_t a = e->cand_list[e->cand_ptr].p;
        // three independent loads (no short circuit: they miss together), and the next entry's lines are asked for meanwhile
        if (e->cand_ptr + 1 < e->cand_list.size()) {
            __builtin_prefetch(&e->arc_at[e->cand_list[e->cand_ptr + 1].p]);
            __builtin_prefetch(&e->node_at[e->cand_ends[2 * e->cand_ptr + 2]]);
            __builtin_prefetch(&e->node_at[e->cand_ends[2 * e->cand_ptr + 3]]);
        }
        const uint32_t t_arc = e->arc_at[a], t_src = e->node_at[e->cand_ends[2 * e->cand_ptr]], t_tgt = e->node_at[e->cand_ends[2 * e->cand_ptr + 1]];
        if ((t_arc <= e->snap_at) & (t_src <= e->snap_at) & (t_tgt <= e->snap_at)) {
            e->hd_ok = true; e->hd_ptr = e->cand_ptr; e->hd_a = (int32_t)a; e->hd_u = e->cand_ends[2 * e->cand_ptr]; e->hd_v = e->cand_ends[2 * e->cand_ptr + 1];
            break;
        }
        e->cand_ptr++;
    }
    CandState::CandKey win{0, kCandNone};
    if (e->cand_ptr < e->cand_list.size()) {
        win = e->cand_list[e->cand_ptr];
        if (best_d.p != kCandNone && cand_key_less(best_d, win)) win = best_d;
    } else if (e->cand_thr.p == kCandNone) {
        win = best_d;                                   // the list was complete: nothing untouched is left
    } else if (best_d.p != kCandNone && cand_key_less(best_d, e->cand_thr)) {
        win = best_d;                                   // everything untouched and unlisted lies above the threshold
    } else {
        return false;
    }
    *out = win;
    return true;
}

// installs the answer of the device search posted at epoch `at`: its n records, and thr, the smallest key it did NOT report (none: it reported
// every eligible arc)
inline void cand_install(CandState *e, const CandGraph &g, const CandState::CandKey *rec, size_t n, CandState::CandKey thr, uint32_t at)
{
    e->cand_thr = thr;
    e->cand_list.clear();
    for (size_t i = 0; i < n; ++i)         // keep only what is provably complete: keys below the smallest unreported key
        if (thr.p == kCandNone || cand_key_less(rec[i], thr)) e->cand_list.push_back(rec[i]);
    std::sort(e->cand_list.begin(), e->cand_list.end(), cand_key_less);
    e->cand_ends.resize(2 * e->cand_list.size());
    for (size_t i = 0; i < e->cand_list.size(); ++i) { e->cand_ends[2 * i] = g.src[e->cand_list[i].p]; e->cand_ends[2 * i + 1] = g.tgt[e->cand_list[i].p]; }
    e->cand_ptr = 0;
    e->cand_valid = true;
    e->hd_ok = e->tp_ok = false;          // another list, another snapshot epoch: nothing verified yet
    e->snap_at = at;
    e->async_posted = false;
    // the heap's invariant under the new list: after a waited-for request nothing is left, after an asynchronous one the few arcs touched
    // during the flight that beat the new threshold
    cand_sweep_heap(e, true);
}

// forgets the list and the heap (upload, or the device state was changed behind the cache's back)
inline void cand_reset(CandState *e)
{
    e->cand_valid = false;
    e->cand_list.clear();
    e->cand_ptr = 0;
    e->hd_ok = e->tp_ok = false;
    e->heap.clear();
    e->pivot_nodes.clear(); e->pivot_arcs.clear(); e->pivot_degree = 0; e->pivot_overflow = false;
    e->heap_gap = e->cand_now;
}

// cand_now >= this and nothing in flight: the epochs start over before the next search
constexpr uint32_t kCandEpochWrap = 0xFFFFFF00u;
// the epoch counter is about to wrap (four billion searches): start over with nothing known -- the device searches next
inline void cand_restart_epochs(CandState *e)
{
    std::fill(e->node_at.begin(), e->node_at.end(), 0u);
    std::fill(e->arc_at.begin(), e->arc_at.end(), 0u);
    const bool overflow = e->pivot_overflow;
    const std::vector<int32_t> pn = e->pivot_nodes, pa = e->pivot_arcs;
    cand_reset(e);
    e->cand_now = 1;
    e->snap_at = 0;
    e->heap_gap = 1;
    e->pivot_overflow = overflow;                       // this pivot's changes are still to be shipped (the engine's sync lists are untouched)
    for (int u : pn) e->node_at[u] = 1;
    for (int a : pa) e->arc_at[a] = 1;
}

// node u becomes node new_of[u] (a permutation of the n nodes); the caller's graph is renumbered alike
inline void cand_renumber(CandState *e, const int32_t *new_of, int n)
{
    mcf::hvec<uint32_t> at((size_t)n);
    for (int u = 0; u < n; ++u) at[new_of[u]] = e->node_at[u];
    std::copy(at.begin(), at.end(), e->node_at.begin());
    for (size_t i = 0; i < e->cand_ends.size(); ++i) e->cand_ends[i] = new_of[e->cand_ends[i]];
    for (auto &h : e->heap) { h.u = new_of[h.u]; h.v = new_of[h.v]; }
    e->tp_ok = e->hd_ok = false;
    for (int32_t &u : e->pivot_nodes) u = new_of[u];
}
