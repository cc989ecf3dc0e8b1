// ranges_step.hip.h -- the cost ranges of a kept optimal basis (mcf_ubatch_cost_ranges, mcf_rbatch_cost_ranges; DESIGN.md 3.14 "Cost
// ranges of the kept basis"), stated once for host and device like the pivot in batch_step.hip.h.
//
// For every arc e of the caller's, how far its cost may fall (down[e]) and rise (up[e]) with every other cost fixed before the basis the
// last solve left stops being optimal; MCF_RANGE_INF where nothing bounds it.  Standard form as the workspace holds it: arcs [0, m) are
// the caller's, [m, m + n) the root links, the rules scan [0, search_arcs); rc_f = cost_f + pi[tail_f] - pi[head_f]; the basis is optimal
// while state_f * rc_f >= 0 for every non-tree arc f of the search range.
//   * a non-tree arc only moves its own reduced cost: at LOWER it may rise for ever and fall by rc, at UPPER the other way round;
//   * a tree arc e = par_arc[u] keeps reduced cost 0, so raising its cost by d shifts the potentials of u's subtree by -par_dir[u] * d
//     (batch_reprice: pi[u] = pi[parent] - par_dir[u] * cost).  That moves rc_f of an arc f across the cut by -par_dir[u] * d where f's
//     tail is the end below u, by +par_dir[u] * d where its head is.  With s = state_f * (tail below ? -par_dir[u] : par_dir[u]) the
//     slack state_f * rc_f changes by s * d: arcs with s < 0 bound the rise, arcs with s > 0 bound the fall, each by its slack.
// Instead of asking, per tree arc, which arcs cross its cut (a search over all arcs per tree arc), every non-tree arc f walks its own
// cycle as find_cycle does: the tree arcs on the path from tail_f up to the join node are exactly those that have tail_f below and
// head_f not, the ones on head_f's path the other way round.  Each lane takes one arc and folds its slack into the two minima of every
// tree arc it steps over: 64 independent chains of dependent loads per wave.  Minima do not depend on the order, so one lane and 64
// lanes give the same bits.
// Nothing here writes the workspace.
#pragma once

#include <stdint.h>

#include "batch_layout.hip.h"
#include "batch_step.hip.h"
#include "uniform_step.hip.h"

namespace mcf {

// what the step reads of an instance; the pointers point wherever the caller bound them (the workspace, LDS, host vectors)
struct RangeView {
    const int32_t *tail, *head;        // arcs [0, all_arcs)
    const int64_t *cost;
    const int8_t *state;
    const int64_t *pi;                 // nodes [0, n], n = the artificial root
    const int32_t *par, *par_arc, *sub;
    const int8_t *par_dir;
    int32_t n, m, search_arcs;
};

// ---- the LDS tier's copy: what RangeView names, and the two accumulators.  Every array starts on a 16-byte boundary and has the size
// it has in the workspace (Layout), rounded up likewise, so each is copied in whole 16-byte words; the accumulators are no larger than
// the workspace's upper[] and flow[], which are not copied: the footprint never exceeds the solve's.
//   tail[A] i32 | head[A] i32 | cost[A] i64 | state[A] i8 | pi[N] i64 | par, par_arc, sub [N] i32 each | par_dir[N] i8 | down[m], up[m] i64
// bytes = 17 A + 21 N + 16 m + padding (at most 15 per array)
struct RangeLayout {
    uint32_t tail, head, cost, state, pi, par, par_arc, sub, par_dir, down, up;
    uint32_t bytes;
};
MCF_HD inline RangeLayout range_layout_of(uint32_t A, uint32_t N, uint32_t m)
{
    RangeLayout r;
    uint32_t o = 0;
    r.tail = o; o = up16(o + 4 * A);
    r.head = o; o = up16(o + 4 * A);
    r.cost = o; o = up16(o + 8 * A);
    r.state = o; o = up16(o + A);
    r.pi = o; o = up16(o + 8 * N);
    r.par = o; o = up16(o + 4 * N);
    r.par_arc = o; o = up16(o + 4 * N);
    r.sub = o; o = up16(o + 4 * N);
    r.par_dir = o; o = up16(o + N);
    r.down = o; o = up16(o + 8 * m);
    r.up = o; o = up16(o + 8 * m);
    r.bytes = o;
    return r;
}

// *p = min(*p, v) where several lanes may meet on one p
MCF_HD inline void lanes_min_into_i64(int64_t *p, int64_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    atomicMin((long long *)p, (long long)v);
#else
    if (v < *p) *p = v;
#endif
}

struct RangeCount {
    uint64_t tree_arcs, hops;          // the caller's arcs in the tree; the steps of all cycle walks.  Summed over the lanes
};

// ---- down[0, m) and up[0, m) of the basis in w.  Order on the device, as uniform_begin explains it: plain stores, barrier, atomic minima
// on the same words, barrier.  A walk is bounded by count (n + 1 steps per side) and by the root, like batch_reprice: a tree that is not
// what rehang_subtree leaves cannot make it spin or step off the arrays.
MCF_HD inline RangeCount batch_cost_ranges(const RangeView &w, int64_t *down, int64_t *up, int lane, int lanes)
{
    const int n = w.n, m = w.m;
    RangeCount c{0, 0};
    for (int e = lane; e < m; e += lanes) {
        const int8_t st = w.state[e];
        const int64_t rc = w.cost[e] + w.pi[w.tail[e]] - w.pi[w.head[e]];
        down[e] = st == MCF_STATE_LOWER ? rc : MCF_RANGE_INF;
        up[e] = st == MCF_STATE_UPPER ? -rc : MCF_RANGE_INF;
        c.tree_arcs += st == MCF_STATE_TREE;
    }
    lanes_sync();
    for (int f = lane; f < w.search_arcs; f += lanes) {
        const int8_t st = w.state[f];
        if (st == MCF_STATE_TREE) continue;
        int a = w.tail[f], b = w.head[f];
        const int64_t slack = (int64_t)st * (w.cost[f] + w.pi[a] - w.pi[b]);
        int left_a = n + 1, left_b = n + 1;
        while (a != b) {                                                    // NS.cs:925-941
            const bool from_tail = w.sub[a] < w.sub[b];
            const int u = from_tail ? a : b;
            if ((unsigned)u >= (unsigned)n || (from_tail ? left_a-- : left_b--) <= 0) break;     // the root has no tree arc above it
            const int e = w.par_arc[u];
            if (e < m) {
                const int s = st * (from_tail ? -w.par_dir[u] : w.par_dir[u]);
                lanes_min_into_i64(s < 0 ? &up[e] : &down[e], slack);
            }
            if (from_tail) a = w.par[u]; else b = w.par[u];
            ++c.hops;
        }
    }
    lanes_sync();
    c.tree_arcs = lanes_sum_u64(c.tree_arcs);
    c.hops = lanes_sum_u64(c.hops);
    return c;
}

// the answers of a ranges call: rows like the solve's flows (instance i's at InstanceView::arc_row); any may be null, down and up together
struct RangeOutputs {
    int32_t *ranged;                   // [count]
    int8_t *arc_state;                 // per arc: MCF_STATE_LOWER / _TREE / _UPPER
    int64_t *cost_down, *cost_up;      // per arc
    int64_t *summary;                  // [3]: ranged instances, their tree arcs among the caller's, cycle hops
};

MCF_HD inline void range_summary_add(int64_t *summary, const RangeCount &c)
{
#if defined(__HIP_DEVICE_COMPILE__)
    atomicAdd((unsigned long long *)&summary[0], 1ull);
    atomicAdd((unsigned long long *)&summary[1], (unsigned long long)c.tree_arcs);
    atomicAdd((unsigned long long *)&summary[2], (unsigned long long)c.hops);
#else
    summary[0] += 1; summary[1] += (int64_t)c.tree_arcs; summary[2] += (int64_t)c.hops;
#endif
}

// dst[0, bytes) = src[0, bytes) in 16-byte words; both on 16-byte boundaries, bytes a multiple of 16
MCF_HD inline void lanes_copy16(unsigned char *dst, const unsigned char *src, uint32_t bytes, int lane, int lanes)
{
    struct alignas(16) Word { uint64_t lo, hi; };
    const Word *const from = (const Word *)src;
    Word *const to = (Word *)dst;
    for (uint32_t k = (uint32_t)lane; k < bytes / 16; k += (uint32_t)lanes) to[k] = from[k];
}

// ---- instance p's row of answers from its workspace and its slot, as its last solve call left them.  Ranged: uniform_kept_optimal;
// every other instance gets ranged = 0 and zero rows.  kLds false: walk the workspace in place and take the minima straight in the
// caller's rows.  kLds true (device only): lds is at least range_layout_of(slot.all_arcs, n + 1, m).bytes of LDS, into which what the
// step reads is copied; the minima are taken there and the rows are written out once, consecutive lanes on consecutive arcs.  A
// compile-time choice, so that every pointer the walk follows has one address space and the minima are LDS atomics, not flat ones.
template <bool kLds>
MCF_HD inline void uniform_ranges(const InstanceView &p, const RangeOutputs &o, const BatchSlot &slot, unsigned char *lds, int lane, int lanes)
{
    const int n = p.n, m = p.m;
    int8_t *const arc_state = o.arc_state ? o.arc_state + p.arc_row : nullptr;
    int64_t *const down = o.cost_down ? o.cost_down + p.arc_row : nullptr, *const up = o.cost_up ? o.cost_up + p.arc_row : nullptr;
    const bool ranged = uniform_kept_optimal(p, slot, lane, lanes);
    if (lane == 0 && o.ranged) o.ranged[p.i] = ranged ? 1 : 0;
    if (!ranged) {
        for (int e = lane; e < m; e += lanes) {
            if (arc_state) arc_state[e] = 0;
            if (down) { down[e] = 0; up[e] = 0; }
        }
        return;
    }
    const uint32_t A = (uint32_t)slot.all_arcs, N = (uint32_t)n + 1u;
    const Layout l = layout_of(A, N);
    if (arc_state) {
        const int8_t *const state = (const int8_t *)(p.home + l.state);
        for (int e = lane; e < m; e += lanes) arc_state[e] = state[e];
    }
    RangeCount c{0, 0};
    if (down) {
        const RangeLayout r = range_layout_of(A, N, (uint32_t)m);
        // one array of the workspace where the step reads it: in place, or its copy at [to, end) of the LDS
        const auto placed = [&](uint32_t from, uint32_t to, uint32_t end) -> const unsigned char * {
            if (!kLds) return p.home + from;
            lanes_copy16(lds + to, p.home + from, end - to, lane, lanes);
            return lds + to;
        };
        RangeView w;
        w.tail = (const int32_t *)placed(l.tail, r.tail, r.head); w.head = (const int32_t *)placed(l.head, r.head, r.cost);
        w.cost = (const int64_t *)placed(l.cost, r.cost, r.state); w.state = (const int8_t *)placed(l.state, r.state, r.pi);
        w.pi = (const int64_t *)placed(l.pi, r.pi, r.par); w.par = (const int32_t *)placed(l.par, r.par, r.par_arc);
        w.par_arc = (const int32_t *)placed(l.par_arc, r.par_arc, r.sub); w.sub = (const int32_t *)placed(l.sub, r.sub, r.par_dir);
        w.par_dir = (const int8_t *)placed(l.par_dir, r.par_dir, r.down);
        w.n = n; w.m = m; w.search_arcs = slot.search_arcs;
        if (kLds) {
            int64_t *const acc_down = (int64_t *)(lds + r.down), *const acc_up = (int64_t *)(lds + r.up);
            lanes_sync();
            c = batch_cost_ranges(w, acc_down, acc_up, lane, lanes);
            for (int e = lane; e < m; e += lanes) { down[e] = acc_down[e]; up[e] = acc_up[e]; }
        } else {
            c = batch_cost_ranges(w, down, up, lane, lanes);
        }
    }
    if (lane == 0) range_summary_add(o.summary, c);
}

}  // namespace mcf
