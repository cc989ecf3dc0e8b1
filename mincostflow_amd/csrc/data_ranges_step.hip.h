// data_ranges_step.hip.h -- the supply and bound ranges of a kept optimal basis (mcf_ubatch_data_ranges, mcf_rbatch_data_ranges;
// DESIGN.md 3.14 "Supply and bound ranges of the kept basis"), stated once for host and device like the cost ranges in ranges_step.hip.h,
// whose mirror image this is: classic right-hand-side ranging.
//
// How far the data may move before the basis the last solve call left stops being PRIMAL feasible, so that a mcf_*batch_resolve_data
// inside the range answers from the kept basis with no pivot and no fallback.  Standard form as the workspace holds it: arcs [0, m) are
// the caller's, [m, all_arcs) root links and artificial arcs; flow[e] is the flow above the lower bound, in [0, upper[e]] with upper[e]
// the capacity (upper - lower), upper[e] >= kInf = uncapacitated; par_dir[u] == kUp means par_arc[u] leaves u towards its parent
// (batch_reprice: pi[u] = pi[parent] - par_dir[u] * cost; uniform_tree_flows: flow[par_arc[u]] = par_dir[u] * the excess of u's subtree,
// so a positive supply ships towards the root through an arc that leaves its node).
//   * the ROOM of node u's tree arc e = par_arc[u]: fall = flow[e], rise = capacity - flow[e] (MCF_RANGE_INF without a capacity);
//     room_out[u], for flow travelling from u to its parent, is rise where the arc leaves u and fall otherwise; room_in[u] is the other.
//     An arc e >= m has no room either way: uniform_redata_settle lets no warm attempt stand that leaves flow on one;
//   * the TRANSFER T(a -> b) is the least room in the direction of travel over the tree path from a to b.  One walk, find_cycle's as
//     batch_cost_ranges walks it, gives T(a -> b) and T(b -> a): the side that climbs from a travels out of its nodes on the way forth
//     and into them on the way back, the side that climbs from b the other way round;
//   * a non-tree arc's flow may fall by T(tail -> head) (the units it no longer carries go through the tree) and rise by
//     T(head -> tail); a tree arc's by its own fall and rise; d units of supply may move from b to a (supply[a] + d, supply[b] - d)
//     while d <= T(a -> b).
// There the walk scatters one slack into the tree arcs it steps over, by atomic minima; here it gathers their rooms into two registers:
// no atomics, one answer pair per walk, so one lane and 64 lanes give the same bits.
// Nothing here writes the workspace.
#pragma once

#include <stdint.h>

#include "batch_layout.hip.h"
#include "batch_step.hip.h"
#include "ranges_step.hip.h"
#include "uniform_step.hip.h"

namespace mcf {

// what the step reads of an instance.  The walk's arrays point wherever the caller bound them (the workspace, LDS, host vectors); the
// four of the second line always into the workspace, where they are read once per node (the LDS tier) or once per hop (in place).
struct DataRangeView {
    const int32_t *tail, *head;        // arcs [0, m)
    const int8_t *state;
    const int32_t *par, *sub;          // nodes [0, n], n = the artificial root
    const int64_t *room_out, *room_in; // nodes [0, n): the LDS tier's; null where the walk runs in place
    const int32_t *par_arc;            // the workspace's
    const int8_t *par_dir;
    const int64_t *flow, *upper;
    int32_t n, m;
};

// ---- the LDS tier's copy: what the walk follows over the caller's arcs and the nodes, and the two room arrays.  Every array starts on a
// 16-byte boundary and is copied in whole 16-byte words.
//   tail[m] i32 | head[m] i32 | state[m] i8 | par[N] i32 | sub[N] i32 | room_out[N] i64 | room_in[N] i64
// bytes = 9 m + 24 N + padding (at most 15 per array).  Never more than the solve's (layout_of(A, N), A = all_arcs >= m): tail, head and
// state are no longer than its own, par and sub are its own, room_out is as long as its pi[N], and room_in (up16(8 N)) is no longer
// than its nxt[N] and prv[N] together (2 up16(4 N), a multiple of 16 that is at least 8 N) -- seven different arrays of that layout.
struct DataRangeLayout {
    uint32_t tail, head, state, par, sub, room_out, room_in;
    uint32_t bytes;
};
MCF_HD inline DataRangeLayout data_range_layout_of(uint32_t m, uint32_t N)
{
    DataRangeLayout r;
    uint32_t o = 0;
    r.tail = o; o = up16(o + 4 * m);
    r.head = o; o = up16(o + 4 * m);
    r.state = o; o = up16(o + m);
    r.par = o; o = up16(o + 4 * N);
    r.sub = o; o = up16(o + 4 * N);
    r.room_out = o; o = up16(o + 8 * N);
    r.room_in = o; o = up16(o + 8 * N);
    r.bytes = o;
    return r;
}

struct DataRangeCount {
    uint64_t walks, hops;              // the tree paths walked (one per non-tree arc, one per pair with both ids in range); their steps
};

// An uncapacitated arc's capacity in the workspace is kInf - lower (uniform_begin: uniform_upper() - lower), which lies below kInf where
// the lower bound is positive.  So a capacity from kInf / 2 on is read as none: that is every uncapacitated arc whose lower bound stays
// below 2^61 in size, and no capacity a flow could reach.
constexpr int64_t kNoCapacity = kInf / 2;

// how far the flow of arc e < m may fall and rise within its bounds
MCF_HD inline void arc_rooms(const DataRangeView &w, int e, int64_t *fall, int64_t *rise)
{
    const int64_t f = w.flow[e], cap = w.upper[e];
    *fall = f;
    *rise = cap >= kNoCapacity ? MCF_RANGE_INF : cap - f;
}
// the rooms of node u's tree arc, u < n
MCF_HD inline void node_rooms(const DataRangeView &w, int u, int64_t *out, int64_t *in)
{
    const int e = w.par_arc[u];
    if ((unsigned)e >= (unsigned)w.m) { *out = 0; *in = 0; return; }
    int64_t fall, rise;
    arc_rooms(w, e, &fall, &rise);
    const bool leaves = w.par_dir[u] == kUp;
    *out = leaves ? rise : fall;
    *in = leaves ? fall : rise;
}

// T(a -> b) and T(b -> a).  Bounded by count (n + 1 steps per side) and by the root, like batch_cost_ranges: a tree that is not what
// rehang_subtree leaves cannot make it spin or step off the arrays.  kRooms: the rooms were laid out per node (pass 0); otherwise each
// hop follows par_arc into the workspace.
template <bool kRooms>
MCF_HD inline void data_transfer(const DataRangeView &w, int a, int b, int64_t *forth_out, int64_t *back_out, DataRangeCount &c)
{
    const int n = w.n;
    int64_t forth = MCF_RANGE_INF, back = MCF_RANGE_INF;
    int left_a = n + 1, left_b = n + 1;
    while (a != b) {                                                        // NS.cs:925-941
        const bool from_a = w.sub[a] < w.sub[b];
        const int u = from_a ? a : b;
        if ((unsigned)u >= (unsigned)n || (from_a ? left_a-- : left_b--) <= 0) break;     // the root has no tree arc above it
        int64_t out, in;
        if (kRooms) { out = w.room_out[u]; in = w.room_in[u]; } else node_rooms(w, u, &out, &in);
        const int64_t ahead = from_a ? out : in, behind = from_a ? in : out;
        forth = ahead < forth ? ahead : forth;
        back = behind < back ? behind : back;
        if (from_a) a = w.par[u]; else b = w.par[u];
        ++c.hops;
    }
    ++c.walks;
    *forth_out = forth;
    *back_out = back;
}

// ---- the three passes.  rooms: where pass 0 lays room_out and room_in out (kRooms; w.room_out / w.room_in name the same words).
// down / up: the caller's rows [m], both or neither.  pairs: [pair_count][2] node ids, forth / back: the caller's rows [pair_count].
template <bool kRooms>
MCF_HD inline DataRangeCount batch_data_ranges(const DataRangeView &w, int64_t *room_out, int64_t *room_in, int64_t *down, int64_t *up, const int32_t *pairs,
                                               int64_t pair_count, int64_t *forth, int64_t *back, int lane, int lanes)
{
    const int n = w.n, m = w.m;
    DataRangeCount c{0, 0};
    if (kRooms) {
        for (int u = lane; u < n; u += lanes) {
            int64_t out, in;
            node_rooms(w, u, &out, &in);
            room_out[u] = out; room_in[u] = in;
        }
        lanes_sync();
    }
    if (down)
        for (int e = lane; e < m; e += lanes) {
            int64_t lo, hi;
            if (w.state[e] == MCF_STATE_TREE) arc_rooms(w, e, &lo, &hi);
            else data_transfer<kRooms>(w, w.tail[e], w.head[e], &lo, &hi, c);
            down[e] = lo; up[e] = hi;
        }
    if (forth)
        for (int64_t k = lane; k < pair_count; k += lanes) {
            const int a = pairs[2 * k], b = pairs[2 * k + 1];
            int64_t there = -1, here = -1;
            if ((unsigned)a < (unsigned)n && (unsigned)b < (unsigned)n) data_transfer<kRooms>(w, a, b, &there, &here, c);
            forth[k] = there; back[k] = here;
        }
    c.walks = lanes_sum_u64(c.walks);
    c.hops = lanes_sum_u64(c.hops);
    return c;
}

// the answers of a data-ranges call: per-arc rows like the solve's flows (instance i's at InstanceView::arc_row), ship rows where the
// instance's PairList says; any may be null, flow_down and flow_up together, ship_forth and ship_back together
struct DataRangeOutputs {
    int32_t *ranged;                   // [count]
    int8_t *arc_state;                 // per arc: MCF_STATE_LOWER / _TREE / _UPPER
    int64_t *flow_down, *flow_up;      // per arc
    int64_t *ship_forth, *ship_back;   // per pair
    int64_t *summary;                  // [3]: ranged instances, their walks, the walks' hops
};
// the pairs of one instance and where its answers to them begin
struct PairList {
    const int32_t *pairs;              // [count][2]
    int64_t count, ship_row;
};
// what a call says of its pairs: one list for every instance (uniform: pairs, pair_count) or one per graph by the caller's tables
// (ragged: pairs, pair_row[graphs + 1], ship_row[count + 1]); each kind of problem reads its own members
struct PairArgs {
    const int32_t *pairs;
    int64_t pair_count;
    const int64_t *pair_row, *ship_row;
};
MCF_HD inline PairList pairs_of(const UniformProblem &, const PairArgs &a, int64_t i) { return PairList{a.pairs, a.pairs ? a.pair_count : 0, i * a.pair_count}; }
MCF_HD inline PairList pairs_of(const RaggedProblem &r, const PairArgs &a, int64_t i)
{
    if (!a.pairs || !a.pair_row || !a.ship_row) return PairList{nullptr, 0, 0};
    const int32_t graph = r.graph_of[i];
    return PairList{a.pairs + 2 * a.pair_row[graph], a.pair_row[graph + 1] - a.pair_row[graph], a.ship_row[i]};
}

MCF_HD inline void data_range_summary_add(int64_t *summary, const DataRangeCount &c)
{
#if defined(__HIP_DEVICE_COMPILE__)
    atomicAdd((unsigned long long *)&summary[0], 1ull);
    atomicAdd((unsigned long long *)&summary[1], (unsigned long long)c.walks);
    atomicAdd((unsigned long long *)&summary[2], (unsigned long long)c.hops);
#else
    summary[0] += 1; summary[1] += (int64_t)c.walks; summary[2] += (int64_t)c.hops;
#endif
}

// ---- instance p's rows of answers from its workspace and its slot, as its last solve call left them.  Ranged: uniform_kept_optimal, as
// for the cost ranges; every other instance gets ranged = 0 and zero rows.  kLds false: the walks follow the workspace in place.  kLds
// true (device only): lds is at least data_range_layout_of(m, n + 1).bytes of LDS, into which what a hop reads is copied and the rooms
// are laid out; a hop is then sub[] followed by par[] with the two rooms riding along.  A compile-time choice, so that every pointer
// the walk follows has one address space.  The answers go from registers straight into the caller's rows, consecutive lanes on
// consecutive arcs or pairs.
template <bool kLds>
MCF_HD inline void uniform_data_ranges(const InstanceView &p, const DataRangeOutputs &o, const PairList &q, const BatchSlot &slot, unsigned char *lds, int lane, int lanes)
{
    const int n = p.n, m = p.m;
    int8_t *const arc_state = o.arc_state ? o.arc_state + p.arc_row : nullptr;
    int64_t *const down = o.flow_down ? o.flow_down + p.arc_row : nullptr, *const up = o.flow_up ? o.flow_up + p.arc_row : nullptr;
    int64_t *const forth = o.ship_forth && q.count > 0 ? o.ship_forth + q.ship_row : nullptr, *const back = forth ? o.ship_back + q.ship_row : nullptr;
    const bool ranged = uniform_kept_optimal(p, slot, lane, lanes);
    if (lane == 0 && o.ranged) o.ranged[p.i] = ranged ? 1 : 0;
    if (!ranged) {
        for (int e = lane; e < m; e += lanes) {
            if (arc_state) arc_state[e] = 0;
            if (down) { down[e] = 0; up[e] = 0; }
        }
        if (forth)
            for (int64_t k = lane; k < q.count; k += lanes) { forth[k] = 0; back[k] = 0; }
        return;
    }
    const uint32_t A = (uint32_t)slot.all_arcs, N = (uint32_t)n + 1u;
    const Layout l = layout_of(A, N);
    if (arc_state) {
        const int8_t *const state = (const int8_t *)(p.home + l.state);
        for (int e = lane; e < m; e += lanes) arc_state[e] = state[e];
    }
    DataRangeCount c{0, 0};
    if (down || forth) {
        const DataRangeLayout r = data_range_layout_of((uint32_t)m, N);
        // one array of the workspace where the walk reads it: in place, or its copy at [to, end) of the LDS
        const auto placed = [&](uint32_t from, uint32_t to, uint32_t end) -> const unsigned char * {
            if (!kLds) return p.home + from;
            lanes_copy16(lds + to, p.home + from, end - to, lane, lanes);
            return lds + to;
        };
        DataRangeView w;
        w.tail = (const int32_t *)placed(l.tail, r.tail, r.head); w.head = (const int32_t *)placed(l.head, r.head, r.state);
        w.state = (const int8_t *)placed(l.state, r.state, r.par);
        w.par = (const int32_t *)placed(l.par, r.par, r.sub); w.sub = (const int32_t *)placed(l.sub, r.sub, r.room_out);
        w.par_arc = (const int32_t *)(p.home + l.par_arc); w.par_dir = (const int8_t *)(p.home + l.par_dir);
        w.flow = (const int64_t *)(p.home + l.flow); w.upper = (const int64_t *)(p.home + l.upper);
        w.n = n; w.m = m;
        if (kLds) {
            int64_t *const room_out = (int64_t *)(lds + r.room_out), *const room_in = (int64_t *)(lds + r.room_in);
            w.room_out = room_out; w.room_in = room_in;
            c = batch_data_ranges<true>(w, room_out, room_in, down, up, q.pairs, q.count, forth, back, lane, lanes);      // its barrier covers the copies too
        } else {
            w.room_out = w.room_in = nullptr;
            c = batch_data_ranges<false>(w, nullptr, nullptr, down, up, q.pairs, q.count, forth, back, lane, lanes);
        }
    }
    if (lane == 0) data_range_summary_add(o.summary, c);
}

}  // namespace mcf
