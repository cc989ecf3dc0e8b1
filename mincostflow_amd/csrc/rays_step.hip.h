// rays_step.hip.h -- unbounded or not, read from the costs and capacities an instance's last solve call left in its workspace
// (mcf_ubatch_rays, mcf_rbatch_rays; DESIGN.md 3.14 "Unbounded or not: a negative cycle or labels from the kept data"), stated once for
// host and device like the diagnosis in diagnose_step.hip.h.
//
// The question is asked of the caller's arcs [0, m): cost_w[e] is the caller's cost, and e is UNCAPACITATED where upper_w[e] >= kNoCapacity
// (the workspace holds kInf - lower there).  A directed cycle of uncapacitated arcs with cost < 0 makes the objective unbounded below
// wherever the instance is feasible; the solve mirrors the reference and answers such an instance Optimal with a cost that wraps.
//   * MCF_RAY_CYCLE: on_cycle[] marks one simple such cycle, cycle_cost < 0 and cycle_length say what it sums to;
//   * MCF_RAY_BOUNDED: label[] with label[head] <= label[tail] + cost on every uncapacitated arc, which summed round a cycle proves its
//     cost >= 0.
// Bellman-Ford from all-zero labels, Jacobi (round r reads only what round r - 1 left: two label arrays) and level synchronous: a label
// can fall in round r only if an in-neighbour's fell in round r - 1, so each round PUSHES marks from the frontier -- the nodes that fell in
// the round before, every node in round 1 -- and PULLS at the marked nodes.  Per round each lane takes one frontier node v, brings the
// other label array up to date at v, walks v's incidence list (built at create, shared by all instances) and stores touched[head] = 1
// for every uncapacitated arc that leaves v: racing stores of one value.  Behind a barrier the lanes stride over the nodes; a touched
// node takes the minimum of old[tail] + cost over its uncapacitated arcs coming in, the first in incidence order among equals, keeps it
// and the arc (pred) only where it is strictly below its old label, and then joins the next frontier in ascending node id, placed by a
// ballot and the bits below the lane with the strides before as the running base (as diag_collect places a level).  No race decides
// anything and the order is fixed, so one lane and 64 lanes give the same bits, the work counts included.
// After round r a label is the cheapest walk of at most r uncapacitated arcs that ends there.  With k = the nodes that have such an arc
// coming in (the nodes round 1 marks) a simple path has at most k arcs, so without a negative cycle nothing falls after round k:
//   * an empty frontier: BOUNDED, and the labels are the certificate (nothing fell, so every arc's inequality holds);
//   * a label that falls in round k + 1: CYCLE.  Along every pred arc label[head] >= label[tail] + cost.  Did the chain of preds from that
//     node end at a node that never fell (label 0), it would be a simple path no cheaper than the label, which round k had then.  So the
//     chain runs into a cycle of the pred graph, behind at most k arcs: k + 1 steps from the lowest such node land on it, one more walk
//     round marks it and sums it.  Such a cycle is strictly negative: summing the inequality round it gives cost <= 0, and the arc that
//     follows the pred set last read a label that has fallen since.  One lane walks, at most 2k + 2 dependent steps.
// WORST CASE: k + 1 rounds where a cycle exists, each two barriers and one sweep over all n nodes -- in the global tier (10 000 nodes,
// thousands of rounds of dependent loads) that is slow, see the measurements in DESIGN.md.  Labels stay inside k * max |cost|, below the
// artificial cost (max |cost| + 1) * n the solve already requires to fit.
// Nothing here writes the workspace: labels, preds, marks and frontiers lie in room of their own (RaysLayout).
#pragma once

#include <stdint.h>

#include "batch_layout.hip.h"
#include "batch_step.hip.h"
#include "data_ranges_step.hip.h"
#include "ranges_step.hip.h"
#include "uniform_step.hip.h"

namespace mcf {

// ---- the room of one instance's query.  LDS tier (arcs = m): the copies of cost[0, m) and upper[0, m), each in whole 16-byte words,
// then the working arrays.  Global tier (arcs = 0): the working arrays alone, in the handle's buffer; cost and upper are read in place.
// N = n + 1 as everywhere, though only n entries are used.
//   cost[arcs] i64 | upper[arcs] i64 | label, other label [N] i64 each | pred, frontier, next frontier [N] i32 each | touched[N] i8
// bytes = 16 arcs + 29 N + padding (at most 15 per array, 7 arrays: 105) -- the solve's workspace is at least 33 (m + n) + 37 N, and
// 33 n >= 105 from n = 4 on; below that 16 m + 29 N + 105 <= 16 m + 250, far under the first LDS class.  The driver classes an
// instance's tier by the SOLVE's footprint (ensure_query_plan), so it is queried in LDS exactly when it is solved there.
struct RaysLayout {
    uint32_t cost, upper, label, label_next, pred, front, front_next, touched;
    uint32_t bytes;
};
MCF_HD inline RaysLayout rays_layout_of(uint32_t arcs, uint32_t N)
{
    RaysLayout d;
    uint32_t o = 0;
    d.cost = o; o = up16(o + 8 * arcs);
    d.upper = o; o = up16(o + 8 * arcs);
    d.label = o; o = up16(o + 8 * N);
    d.label_next = o; o = up16(o + 8 * N);
    d.pred = o; o = up16(o + 4 * N);
    d.front = o; o = up16(o + 4 * N);
    d.front_next = o; o = up16(o + 4 * N);
    d.touched = o; o = up16(o + N);
    d.bytes = o;
    return d;
}

// what the rounds read of an instance: the graph (global memory in both tiers) and the caller's arcs' cost and capacity where the tier has them
struct RaysView {
    const int32_t *source, *target;    // [m]
    const int32_t *inc_start, *inc;    // [n + 1], [2m]: arc << 1 | (the node is the arc's target)
    const int64_t *cost, *upper;       // [m]
    int32_t n, m;
};

struct RaysCount {
    uint64_t rounds, frontier, entries;     // rounds run, the nodes of all frontiers, incidence entries read
};

MCF_HD inline bool rays_open(const RaysView &w, int e) { return w.upper[e] >= kNoCapacity; }

// ---- the rounds.  Returns the nodes that still fell in round k + 1 (> 0: a negative cycle, *fell = those nodes in ascending id) or 0
// (bounded, *labels = the certificate).  label, other, pred, front, front_next and touched are room for n entries each.  Every lane
// leaves with the same counts and *k.
MCF_HD inline int32_t rays_rounds(const RaysView &w, int64_t *label, int64_t *other, int32_t *pred, int32_t *front, int32_t *front_next, int8_t *touched,
                                  RaysCount *c, int32_t *k, const int64_t **labels, const int32_t **fell, int lane, int lanes)
{
    const int n = w.n;
    for (int v = lane; v < n; v += lanes) { label[v] = 0; other[v] = 0; pred[v] = -1; touched[v] = 0; front[v] = v; }
    lanes_sync();
    int32_t count = n, reach = 0;
    uint64_t entries = 0;
    while (count > 0) {
        ++c->rounds;
        c->frontier += (uint64_t)count;
        for (int32_t at_front = lane; at_front < count; at_front += lanes) {
            const int v = front[at_front];
            other[v] = label[v];                                            // v fell in the round before: the array that round read is stale here
            const int32_t end = w.inc_start[v + 1];
            for (int32_t at = w.inc_start[v]; at < end; ++at) {
                const int32_t entry = w.inc[at], e = entry >> 1;
                ++entries;
                if ((entry & 1) == 0 && rays_open(w, e)) touched[w.target[e]] = 1;
            }
        }
        lanes_sync();
        // both arrays are equal now; `other` takes what falls
        int32_t next_count = 0, marked = 0;
        for (int base = 0; base < n; base += lanes) {
            const int v = base + lane;
            const bool pull = v < n && touched[v] != 0;
            bool falls = false;
            if (pull) {
                touched[v] = 0;
                int64_t best = label[v];
                int32_t best_arc = -1;
                const int32_t end = w.inc_start[v + 1];
                for (int32_t at = w.inc_start[v]; at < end; ++at) {
                    const int32_t entry = w.inc[at], e = entry >> 1;
                    ++entries;
                    if ((entry & 1) == 0 || !rays_open(w, e)) continue;
                    const int64_t through = label[w.source[e]] + w.cost[e];
                    if (through < best) { best = through; best_arc = e; }
                }
                falls = best_arc >= 0;
                if (falls) { other[v] = best; pred[v] = best_arc; }
            }
            const uint64_t mask = lanes_ballot(falls);
            if (falls) front_next[next_count + popcount64(mask & (((uint64_t)1 << lane) - 1))] = v;
            next_count += popcount64(mask);
            marked += popcount64(lanes_ballot(pull));
        }
        lanes_sync();
        if (c->rounds == 1) reach = marked;                                 // round 1 pushed from every node: the marked are the nodes with such an arc coming in
        { int64_t *const t = label; label = other; other = t; }
        { int32_t *const t = front; front = front_next; front_next = t; }
        count = next_count;
        if (count > 0 && c->rounds == (uint64_t)reach + 1u) break;
    }
    c->entries = lanes_sum_u64(entries);
    *k = reach;
    *labels = label;
    *fell = front;
    return count;
}

// the answers of a rays call: one entry per instance, rows like the solve's flows and potentials (instance i's at InstanceView::arc_row and
// ::node_row); any may be null
struct RaysOutputs {
    int32_t *verdict;                  // [count] MCF_RAY_*
    int64_t *cycle_cost;               // [count]
    int32_t *cycle_length;             // [count]
    int8_t *on_cycle;                  // per arc: 1 = on the cycle
    int64_t *label;                    // per node
    int64_t *summary;                  // [MCF_RAY_BOUNDS + 1] instances per verdict, then rounds, frontier nodes, incidence entries, cycle arcs
};
constexpr int kRaysSummaryWords = MCF_RAY_BOUNDS + 5;

MCF_HD inline void rays_summary_add(int64_t *summary, int32_t verdict, const RaysCount &c, int32_t cycle_arcs)
{
#if defined(__HIP_DEVICE_COMPILE__)
    atomicAdd((unsigned long long *)&summary[verdict], 1ull);
    if (c.rounds) {
        atomicAdd((unsigned long long *)&summary[MCF_RAY_BOUNDS + 1], (unsigned long long)c.rounds);
        atomicAdd((unsigned long long *)&summary[MCF_RAY_BOUNDS + 2], (unsigned long long)c.frontier);
        atomicAdd((unsigned long long *)&summary[MCF_RAY_BOUNDS + 3], (unsigned long long)c.entries);
    }
    if (cycle_arcs) atomicAdd((unsigned long long *)&summary[MCF_RAY_BOUNDS + 4], (unsigned long long)cycle_arcs);
#else
    summary[verdict] += 1;
    summary[MCF_RAY_BOUNDS + 1] += (int64_t)c.rounds; summary[MCF_RAY_BOUNDS + 2] += (int64_t)c.frontier; summary[MCF_RAY_BOUNDS + 3] += (int64_t)c.entries;
    summary[MCF_RAY_BOUNDS + 4] += cycle_arcs;
#endif
}

// ---- instance p's answers from its workspace and its slot, as its last solve call left them.  Stopped by its bounds: MCF_RAY_BOUNDS;
// a slot no solve call has placed (all_arcs below m + n): MCF_RAY_NONE; both with zero rows.  Everything else is answered: the data are
// in the workspace however the solve ended.  room: at least rays_layout_of(kLds ? m : 0, n + 1).bytes on a 16-byte boundary -- kLds true
// (device only): LDS, into which cost and upper of the caller's arcs are copied; kLds false: the instance's part of the handle's buffer
// (host: a vector), and the rounds read cost and upper in the workspace.  A compile-time choice, so that labels, marks and frontiers
// have one address space.
template <bool kLds>
MCF_HD inline void uniform_rays(const InstanceView &p, const RaysOutputs &o, const BatchSlot &slot, unsigned char *room, int lane, int lanes)
{
    const int n = p.n, m = p.m;
    int8_t *const on_cycle = o.on_cycle ? o.on_cycle + p.arc_row : nullptr;
    int64_t *const label_row = o.label ? o.label + p.node_row : nullptr;
    const bool placed = slot.all_arcs >= m + n && slot.n == n;
    int32_t verdict = slot.run == kBatchByBounds ? MCF_RAY_BOUNDS : MCF_RAY_NONE;
    int64_t cycle_cost = 0;
    int32_t cycle_length = 0;
    RaysCount c{0, 0, 0};
    const int64_t *labels = nullptr;
    if (on_cycle)
        for (int e = lane; e < m; e += lanes) on_cycle[e] = 0;
    if (placed && slot.run != kBatchByBounds) {
        const uint32_t N = (uint32_t)n + 1u;
        const Layout l = layout_of((uint32_t)slot.all_arcs, N);
        const RaysLayout d = rays_layout_of(kLds ? (uint32_t)m : 0u, N);
        RaysView w;
        w.source = p.source; w.target = p.target; w.inc_start = p.inc_start; w.inc = p.inc;
        w.n = n; w.m = m;
        if (kLds) {
            // cost[] and upper[] begin on 16-byte boundaries and hold all_arcs >= m entries: whole words up to up16(8 m) lie inside them
            lanes_copy16(room + d.cost, p.home + l.cost, d.upper - d.cost, lane, lanes);
            lanes_copy16(room + d.upper, p.home + l.upper, d.label - d.upper, lane, lanes);
            w.cost = (const int64_t *)(room + d.cost); w.upper = (const int64_t *)(room + d.upper);
        } else {
            w.cost = (const int64_t *)(p.home + l.cost); w.upper = (const int64_t *)(p.home + l.upper);
        }
        int32_t *const pred = (int32_t *)(room + d.pred);
        int32_t k = 0;
        const int32_t *fell = nullptr;
        const int32_t still = rays_rounds(w, (int64_t *)(room + d.label), (int64_t *)(room + d.label_next), pred, (int32_t *)(room + d.front),
                                          (int32_t *)(room + d.front_next), (int8_t *)(room + d.touched), &c, &k, &labels, &fell, lane, lanes);
        verdict = still > 0 ? MCF_RAY_CYCLE : MCF_RAY_BOUNDED;
        if (still > 0) {
            labels = nullptr;
            if (lane == 0) {                                                // behind the rounds' barriers: every pred is final and every zero above is stored
                int v = fell[0];
                for (int32_t step = 0; step <= k && pred[v] >= 0; ++step) v = w.source[pred[v]];
                const int first = v;
                for (int32_t step = 0; step <= k && pred[v] >= 0; ++step) {       // a cycle of the pred graph has at most k arcs
                    const int32_t e = pred[v];
                    if (on_cycle) on_cycle[e] = 1;
                    cycle_cost += w.cost[e];
                    ++cycle_length;
                    v = w.source[e];
                    if (v == first) break;
                }
            }
        }
    }
    if (label_row)
        for (int v = lane; v < n; v += lanes) label_row[v] = labels ? labels[v] : 0;
    if (lane != 0) return;
    if (o.verdict) o.verdict[p.i] = verdict;
    if (o.cycle_cost) o.cycle_cost[p.i] = cycle_cost;
    if (o.cycle_length) o.cycle_length[p.i] = cycle_length;
    rays_summary_add(o.summary, verdict, c, cycle_length);
}

}  // namespace mcf
