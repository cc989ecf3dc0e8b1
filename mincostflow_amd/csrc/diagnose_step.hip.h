// diagnose_step.hip.h -- why an instance is infeasible, read from the flow its last solve left (mcf_ubatch_diagnose, mcf_rbatch_diagnose;
// DESIGN.md 3.14 "Why infeasible: a cut from the kept flow"), stated once for host and device like the ranges in ranges_step.hip.h.
//
// Standard form as the workspace holds it: arcs [0, m) are the caller's with 0 <= flow <= upper, [m, m + n) the root links (link m + v is
// node v's), [m + n, all_arcs) the artificial arcs, each between the root and ONE node.  A solve that ended with no entering arc left a
// flow that is extremal against the artificial cost; what it could not ship lies on the arcs >= m:
//   unmet[v] = what v sends to the root there - what it receives from it, so the caller's arcs carry nf(v) = b'(v) - unmet[v] out of v.
// GEQ asks nf >= b': v is VIOLATED where unmet > 0 and SLACK where unmet < 0; LEQ mirrors both.
//   * no violated node: the kept flow satisfies every constraint, whatever the status word says (MCF_DIAG_FEASIBLE);
//   * else S = what the violated nodes reach in the residual graph of the caller's arcs: GEQ tail -> head where flow < upper (an
//     uncapacitated arc is never saturated), head -> tail where flow > 0; LEQ both reversed (the nodes that still reach a violated one).
//     Every arc that leaves S in the walk's direction is saturated and every arc that enters it is empty, so summing nf over S gives
//       GEQ  sum of unmet over S = supply(S) - (upper(out of S) - lower(into S))
//       LEQ  sum of -unmet over S = (lower(out of S) - upper(into S)) - supply(S)
//     in the caller's own numbers.  With no slack node in S every term of the sum has one sign: it is the VIOLATION, > 0, and S is a cut
//     that proves the instance infeasible (MCF_DIAG_CUT).  A slack node in S would mean an augmenting path the solve left unused: no
//     certificate (MCF_DIAG_OPEN); the artificial cost (max |c| + 1) * n rules it out after a solve that found no entering arc.
// The walk is level synchronous and takes no atomics.  Per level each lane takes one frontier node, walks the node's incidence list
// (built at create, shared by all instances) and stores next[w] = 1 for every residual neighbour not reached yet: racing stores of one
// value.  Behind a barrier the lanes stride over the nodes; next && !reached becomes reached and joins the new frontier in ascending
// node id, placed by a ballot and the bits below the lane with the strides before as the running base (as uniform_begin numbers the
// artificial arcs).  The order is fixed, so one lane and 64 lanes give the same bits, the work counts included.
// Nothing here writes the workspace: marks, frontiers and unmet[] lie in room of their own (DiagLayout).
#pragma once

#include <stdint.h>

#include "batch_layout.hip.h"
#include "batch_step.hip.h"
#include "data_ranges_step.hip.h"
#include "ranges_step.hip.h"
#include "uniform_step.hip.h"

namespace mcf {

// ---- the room of one instance's diagnosis.  LDS tier (arcs = m): the copies of flow[0, m) and upper[0, m), each in whole 16-byte
// words, then the working arrays.  Global tier (arcs = 0): the working arrays alone, in the handle's buffer; flow and upper are read in
// place.  N = n + 1 as everywhere, though only n entries are used.
//   flow[arcs] i64 | upper[arcs] i64 | unmet[N] i64 | frontier, next frontier [N] i32 each | reached[N] i8 | next[N] i8
// bytes = 16 arcs + 18 N + padding (at most 15 per array): below the solve's 33 A + 37 N.
struct DiagLayout {
    uint32_t flow, upper, unmet, front, front_next, reached, next;
    uint32_t bytes;
};
MCF_HD inline DiagLayout diag_layout_of(uint32_t arcs, uint32_t N)
{
    DiagLayout d;
    uint32_t o = 0;
    d.flow = o; o = up16(o + 8 * arcs);
    d.upper = o; o = up16(o + 8 * arcs);
    d.unmet = o; o = up16(o + 8 * N);
    d.front = o; o = up16(o + 4 * N);
    d.front_next = o; o = up16(o + 4 * N);
    d.reached = o; o = up16(o + N);
    d.next = o; o = up16(o + N);
    d.bytes = o;
    return d;
}

// what the walk reads of an instance: the graph (global memory in both tiers) and the caller's arcs' flow and capacity where the tier has them
struct DiagView {
    const int32_t *source, *target;    // [m]
    const int32_t *inc_start, *inc;    // [n + 1], [2m]: arc << 1 | (the node is the arc's target)
    const int64_t *flow, *upper;       // [m]
    int32_t n, m;
    bool geq;
};

struct DiagCount {
    uint64_t levels, frontier, entries;     // levels walked, the nodes of all frontiers, incidence entries read
};

MCF_HD inline bool diag_violated(bool geq, int64_t unmet) { return geq ? unmet > 0 : unmet < 0; }
MCF_HD inline bool diag_slack(bool geq, int64_t unmet) { return geq ? unmet < 0 : unmet > 0; }

// One sweep over the nodes: those with take(v) are marked reached and appended to `out` in ascending id.  Returns how many.
template <class Take>
MCF_HD inline int32_t diag_collect(int n, int8_t *reached, int32_t *out, Take take, int lane, int lanes)
{
    int32_t count = 0;
    for (int base = 0; base < n; base += lanes) {
        const int v = base + lane;
        const bool add = v < n && take(v);
        const uint64_t mask = lanes_ballot(add);
        if (add) {
            reached[v] = 1;
            out[count + popcount64(mask & (((uint64_t)1 << lane) - 1))] = v;
        }
        count += popcount64(mask);
    }
    return count;
}

// ---- reached[v] = 1 exactly for the nodes of S.  unmet[0, n) is final; reached, next and the two frontiers are room for n entries each.
// Every lane leaves with the same counts.
MCF_HD inline DiagCount diag_reach(const DiagView &w, const int64_t *unmet, int8_t *reached, int8_t *next, int32_t *front, int32_t *front_next, int lane, int lanes)
{
    const int n = w.n;
    const bool geq = w.geq;
    DiagCount c{0, 0, 0};
    for (int v = lane; v < n; v += lanes) { reached[v] = 0; next[v] = 0; }
    lanes_sync();
    int32_t count = diag_collect(n, reached, front, [&](int v) { return diag_violated(geq, unmet[v]); }, lane, lanes);
    lanes_sync();
    while (count > 0) {
        ++c.levels;
        c.frontier += (uint64_t)count;
        for (int32_t k = lane; k < count; k += lanes) {
            const int v = front[k];
            const int32_t end = w.inc_start[v + 1];
            for (int32_t at = w.inc_start[v]; at < end; ++at) {
                const int32_t entry = w.inc[at], e = entry >> 1;
                const bool incoming = (entry & 1) != 0;                     // v is e's head: the other end is its tail
                const int64_t f = w.flow[e];
                // GEQ leaves v along e where e has room and against e where e carries flow; LEQ the other way round
                const bool along = geq ? !incoming : incoming;
                const bool open = along ? (w.upper[e] >= kNoCapacity || f < w.upper[e]) : f > 0;
                const int other = incoming ? w.source[e] : w.target[e];
                ++c.entries;
                if (open && !reached[other]) next[other] = 1;
            }
        }
        lanes_sync();
        count = diag_collect(n, reached, front_next, [&](int v) { return next[v] != 0 && reached[v] == 0; }, lane, lanes);
        lanes_sync();
        int32_t *const t = front; front = front_next; front_next = t;
    }
    c.entries = lanes_sum_u64(c.entries);
    return c;
}

// the answers of a diagnose call: one entry per instance, rows like the solve's potentials (instance i's at InstanceView::node_row); any may be null
struct DiagOutputs {
    int32_t *verdict;                  // [count] MCF_DIAG_*
    int64_t *violation;                // [count]
    int32_t *set_size;                 // [count]
    int8_t *side;                      // per node: 1 = in S
    int64_t *unmet;                    // per node
    int64_t *summary;                  // [MCF_DIAG_BOUNDS + 1] instances per verdict, then levels, frontier nodes, incidence entries
};
constexpr int kDiagSummaryWords = MCF_DIAG_BOUNDS + 4;

MCF_HD inline void diag_summary_add(int64_t *summary, int32_t verdict, const DiagCount &c)
{
#if defined(__HIP_DEVICE_COMPILE__)
    atomicAdd((unsigned long long *)&summary[verdict], 1ull);
    if (c.levels) {
        atomicAdd((unsigned long long *)&summary[MCF_DIAG_BOUNDS + 1], (unsigned long long)c.levels);
        atomicAdd((unsigned long long *)&summary[MCF_DIAG_BOUNDS + 2], (unsigned long long)c.frontier);
        atomicAdd((unsigned long long *)&summary[MCF_DIAG_BOUNDS + 3], (unsigned long long)c.entries);
    }
#else
    summary[verdict] += 1;
    summary[MCF_DIAG_BOUNDS + 1] += (int64_t)c.levels; summary[MCF_DIAG_BOUNDS + 2] += (int64_t)c.frontier; summary[MCF_DIAG_BOUNDS + 3] += (int64_t)c.entries;
#endif
}

// ---- instance p's answers from its workspace and its slot, as its last solve call left them; p.supply_type is that call's.  Diagnosed:
// the call ended with no entering arc.  By its bounds: MCF_DIAG_BOUNDS; anything else (Unbounded, a limit, never solved): MCF_DIAG_NONE;
// both with zero rows.  room: at least diag_layout_of(kLds ? m : 0, n + 1).bytes on a 16-byte boundary -- kLds true (device only): LDS,
// into which flow and upper of the caller's arcs are copied; kLds false: the instance's part of the handle's buffer (host: a vector),
// and the walk reads flow and upper in the workspace.  A compile-time choice, so that marks and frontiers have one address space.
template <bool kLds>
MCF_HD inline void uniform_diagnose(const InstanceView &p, const DiagOutputs &o, const BatchSlot &slot, unsigned char *room, int lane, int lanes)
{
    const int n = p.n, m = p.m;
    int8_t *const side = o.side ? o.side + p.node_row : nullptr;
    int64_t *const unmet_row = o.unmet ? o.unmet + p.node_row : nullptr;
    int32_t verdict = slot.run == kBatchByBounds ? MCF_DIAG_BOUNDS : MCF_DIAG_NONE;
    int64_t violation = 0;
    int32_t set_size = 0;
    DiagCount c{0, 0, 0};
    if (slot.run == kBatchNoEntering) {
        const bool geq = p.supply_type == MCF_SUPPLY_GEQ;
        const uint32_t A = (uint32_t)slot.all_arcs, N = (uint32_t)n + 1u;
        const Layout l = layout_of(A, N);
        const DiagLayout d = diag_layout_of(kLds ? (uint32_t)m : 0u, N);
        const int32_t *const tail = (const int32_t *)(p.home + l.tail), *const head = (const int32_t *)(p.home + l.head);
        const int64_t *const flow = (const int64_t *)(p.home + l.flow);
        int64_t *const unmet = (int64_t *)(room + d.unmet);
        int8_t *const reached = (int8_t *)(room + d.reached);
        DiagView w;
        w.source = p.source; w.target = p.target; w.inc_start = p.inc_start; w.inc = p.inc;
        w.n = n; w.m = m; w.geq = geq;
        if (kLds) {
            // flow[] and upper[] begin on 16-byte boundaries and hold all_arcs >= m entries: whole words up to up16(8 m) lie inside them
            lanes_copy16(room + d.flow, p.home + l.flow, d.upper - d.flow, lane, lanes);
            lanes_copy16(room + d.upper, p.home + l.upper, d.unmet - d.upper, lane, lanes);
            w.flow = (const int64_t *)(room + d.flow); w.upper = (const int64_t *)(room + d.upper);
        } else {
            w.flow = flow; w.upper = (const int64_t *)(p.home + l.upper);
        }
        // unmet: the link m + v is v's own; every artificial arc has one end that is not the root, and no node has two of them
        // (uniform_begin, uniform_start_try).  Plain stores, barrier, plain read-modify-write by the one lane that owns the arc.
        for (int v = lane; v < n; v += lanes) unmet[v] = geq ? -flow[m + v] : flow[m + v];
        lanes_sync();
        for (int e = m + n + lane; e < (int)A; e += lanes) {
            const int t = tail[e], h = head[e];
            const int v = t == n ? h : t;
            if ((unsigned)v < (unsigned)n) unmet[v] += t == v ? flow[e] : -flow[e];
        }
        lanes_sync();
        bool any = false;
        for (int v = lane; v < n; v += lanes) any |= diag_violated(geq, unmet[v]);
        if (!lanes_any(any)) {
            verdict = MCF_DIAG_FEASIBLE;
        } else {
            c = diag_reach(w, unmet, reached, (int8_t *)(room + d.next), (int32_t *)(room + d.front), (int32_t *)(room + d.front_next), lane, lanes);
            bool slack = false;
            uint64_t sum = 0, size = 0;
            for (int v = lane; v < n; v += lanes) {
                if (!reached[v]) continue;
                const int64_t u = unmet[v];
                slack |= diag_slack(geq, u);
                sum += (uint64_t)(u < 0 ? -u : u);
                ++size;
            }
            const bool open = lanes_any(slack);
            verdict = open ? MCF_DIAG_OPEN : MCF_DIAG_CUT;
            violation = open ? 0 : (int64_t)lanes_sum_u64(sum);
            set_size = (int32_t)lanes_sum_u64(size);
        }
        const bool walked = verdict != MCF_DIAG_FEASIBLE;
        for (int v = lane; v < n; v += lanes) {
            if (side) side[v] = walked ? reached[v] : 0;
            if (unmet_row) unmet_row[v] = unmet[v];
        }
    } else {
        for (int v = lane; v < n; v += lanes) {
            if (side) side[v] = 0;
            if (unmet_row) unmet_row[v] = 0;
        }
    }
    if (lane != 0) return;
    if (o.verdict) o.verdict[p.i] = verdict;
    if (o.violation) o.violation[p.i] = violation;
    if (o.set_size) o.set_size[p.i] = set_size;
    diag_summary_add(o.summary, verdict, c);
}

}  // namespace mcf
