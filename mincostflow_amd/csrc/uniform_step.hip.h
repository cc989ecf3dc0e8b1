// uniform_step.hip.h -- the set-up and the end of a solve for a batch that shares ONE topology (mcf_ubatch_*, DESIGN.md 3.14 "Uniform
// batch"), stated once for host and device like the pivot in batch_step.hip.h.
//
// Three steps per instance, each over (lane, lanes): 64 lanes of one wave on the device, one "lane" on the host (the test hooks).
//   uniform_begin   bounds check, standard form, art_cost, the star start basis of start_basis (ns_core.cpp) and the instance's slot;
//   uniform_finish  the status (finish_instance + core_finish of batch.hip / ns_core.cpp) and the output rows;
//   uniform_recost  a re-solve with new costs: from the kept basis where the last solve ended Optimal, else uniform_begin again.
//   uniform_redata  a re-solve with new supplies and bounds: the kept basis with its tree flows recomputed, for batch_dual_run, else
//                   uniform_begin again; uniform_redata_settle judges the warm attempt and starts it again cold where it did not hold.
//   uniform_begin_from  a solve that starts from a basis the caller supplies, one state per arc: the forest of its TREE arcs is walked,
//                   hung on the root, given flows and potentials and classed; anything that is no basis: uniform_begin.
// The pivots between them are batch_run on the workspace these steps leave, unchanged.
// A fourth step stands apart from the solve: uniform_validate checks a solution in the caller's rows (mcf_ubatch_validate).
// Problem data are read straight from the caller's arrays, results are written straight into the caller's rows.  The steps never learn
// whether those pointers are device or host memory, nor how the rows were found: they work on an InstanceView, the instance PLACED.
// Two ways lead to a view.  uniform_view: one topology, rows at base + instance * stride (stride 0 = one array for all), workspaces at a
// fixed stride (mcf_ubatch_*).  ragged_view: a set of graphs, every instance names its own, rows and workspaces at running sums kept in
// per-handle tables (mcf_rbatch_*, DESIGN.md 3.14 "Ragged batch").  Code that serves both names neither: view_of and check_view_of
// take the problem of either kind.
// Nothing here depends on the order in which lanes add: the supply shift and the total cost are integer sums (they wrap, they commute),
// so one lane and 64 lanes give the same bits, and both give ns_core.cpp's.
#pragma once

#include <stdint.h>

#include "batch_layout.hip.h"
#include "batch_step.hip.h"

namespace mcf {

// one topology, `count` instances of it; every pointer points into the memory the step runs in
struct UniformProblem {
    int32_t n, m, supply_type, trace_cap;
    const int32_t *source, *target;                      // [m], validated by mcf_ubatch_create
    const int32_t *inc_start, *inc;                      // its incidence lists [n + 1], [2m]
    const int64_t *lower, *upper, *cost, *supply;        // null: 0 / uncapacitated / 0 / 0
    int64_t lower_stride, upper_stride, cost_stride, supply_stride;     // elements between instances, 0 = shared
    uint64_t stride;                                     // bytes between workspaces: layout_of(m + 2n, n + 1).bytes
    const uint8_t *changed;                              // re-solve: [count], null = all
    const int8_t *start_state;                           // uniform_begin_from: the caller's basis, [m] per instance ...
    int64_t start_stride;                                // ... elements between instances, 0 = one row for all
};
struct UniformOutputs {                                  // any may be null
    int32_t *status;
    int64_t *pivots, *total_cost, *flows, *potentials;   // [count], [count], [count * m], [count * n]
    int32_t *trace;                                      // [count * trace_cap]
};

// the solution and the answers of a validation: every array has one entry (or MCF_VAL_KINDS) per instance; the rows are in the view
struct UniformCheck {
    const int32_t *status;                               // the solution: [count], [count]
    const int64_t *total_cost;
    int32_t *valid, *errors, *first;                     // the answers, any may be null: [count], [count * MCF_VAL_KINDS] twice
    int64_t *objective, *dual_cost;                      // [count]
    int64_t *summary;                                    // [2]: invalid instances, the lowest invalid index (INT64_MAX while there is none)
};

// Instance i placed: its graph, its rows of the caller's arrays, its workspace, its output rows.  All the steps below see of a batch.
struct InstanceView {
    int64_t i;                                           // its entry of the per-instance arrays (status[i], changed[i], ...)
    int64_t arc_row;                                     // where its rows of the per-arc arrays begin, in elements
    int64_t node_row;                                    // ... and its rows of the per-node arrays
    int32_t n, m, supply_type, trace_cap;
    const int32_t *source, *target;                      // [m], validated at create
    const int32_t *inc_start, *inc;                      // the graph's incidence lists [n + 1], [2m]: uniform_validate and uniform_begin_from
    const int8_t *start_state;                           // uniform_begin_from: the instance's row of arc states [m]
    const int64_t *lower, *upper, *cost, *supply;        // the instance's rows; null: 0 / uncapacitated / 0 / 0
    unsigned char *home;                                 // its workspace = slab + workspace
    uint64_t workspace, trace;                           // what its slot says of where workspace and trace lie
    int64_t *flows, *potentials;                         // output rows [m], [n], null = not asked for
    int32_t *trace_row;                                  // [trace_cap]
    const int64_t *check_flows, *check_potentials;       // uniform_validate: the rows of the solution to check
};

// ---- a set of graphs, every instance one of them (mcf_rbatch_*).  The tables lie where the step runs.
struct RaggedGraph {
    int32_t n, m, tmpl, reserved;                        // tmpl: its slot template
    int64_t ends, inc_start, inc;                        // where its end points ([m]) and its incidence lists ([n + 1], [2m]) begin
};
struct RaggedProblem {
    int32_t supply_type, trace_cap;
    const int32_t *graph_of;                             // [count]
    const RaggedGraph *graphs;
    const int64_t *arc_row, *node_row;                   // [count + 1]: running sums of m and n
    const uint64_t *workspace;                           // [count]: running sums of layout_of(m + 2n, n + 1).bytes
    const int32_t *source, *target, *inc_start, *inc;    // every graph's, concatenated
    const int64_t *lower, *upper, *cost, *supply;        // [arc_row[count]] three times, [node_row[count]]; null as in the view
    const uint8_t *changed;                              // re-solve: [count], null = all
    const int8_t *start_state;                           // uniform_begin_from: [arc_row[count]]
};

// ---- what the lanes share (device: all 64 lanes of the wave call these together; host: one lane, the identity)
MCF_HD inline uint64_t lanes_ballot(bool p)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint64_t)__ballot(p ? 1 : 0);
#else
    return p ? 1u : 0u;
#endif
}
MCF_HD inline int popcount64(uint64_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __popcll(v);
#else
    return __builtin_popcountll(v);
#endif
}
MCF_HD inline bool lanes_any(bool p) { return lanes_ballot(p) != 0; }
MCF_HD inline uint64_t lanes_sum_u64(uint64_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    for (int d = 32; d > 0; d >>= 1) v += (uint64_t)__shfl_xor((int64_t)v, d, 64);
#endif
    return v;
}
// *p += v where several lanes may meet on one p
MCF_HD inline void lanes_add_i64(int64_t *p, int64_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    atomicAdd((unsigned long long *)p, (unsigned long long)v);
#else
    *p = (int64_t)((uint64_t)*p + (uint64_t)v);
#endif
}

MCF_HD inline const int64_t *uniform_row(const int64_t *base, int64_t stride, int64_t i) { return base ? base + i * stride : nullptr; }
MCF_HD inline int64_t *output_row(int64_t *base, int64_t offset) { return base ? base + offset : nullptr; }
// o: where a solve writes, c + solution rows + lists: what a validation reads; either may be absent
MCF_HD inline InstanceView uniform_view(const UniformProblem &p, const UniformOutputs *o, int64_t i, unsigned char *slab)
{
    InstanceView v{};
    v.i = i; v.n = p.n; v.m = p.m; v.supply_type = p.supply_type; v.trace_cap = p.trace_cap;
    v.source = p.source; v.target = p.target; v.inc_start = p.inc_start; v.inc = p.inc;
    v.lower = uniform_row(p.lower, p.lower_stride, i); v.upper = uniform_row(p.upper, p.upper_stride, i);
    v.cost = uniform_row(p.cost, p.cost_stride, i); v.supply = uniform_row(p.supply, p.supply_stride, i);
    v.arc_row = i * (int64_t)p.m; v.node_row = i * (int64_t)p.n;
    v.start_state = p.start_state ? p.start_state + i * p.start_stride : nullptr;
    v.workspace = (uint64_t)i * p.stride; v.trace = (uint64_t)i * (uint64_t)p.trace_cap;
    v.home = slab ? slab + v.workspace : nullptr;
    if (o) {
        v.flows = output_row(o->flows, i * (int64_t)p.m); v.potentials = output_row(o->potentials, i * (int64_t)p.n);
        v.trace_row = o->trace ? o->trace + i * (int64_t)p.trace_cap : nullptr;
    }
    return v;
}
MCF_HD inline InstanceView uniform_check_view(const UniformProblem &p, const int64_t *flows, const int64_t *potentials, int64_t i)
{
    InstanceView v = uniform_view(p, nullptr, i, nullptr);
    v.check_flows = flows + i * (int64_t)p.m; v.check_potentials = potentials + i * (int64_t)p.n;
    return v;
}
// the tables say where everything of instance i lies; *tmpl = the index of its graph's slot template
MCF_HD inline InstanceView ragged_view(const RaggedProblem &r, const UniformOutputs *o, int64_t i, unsigned char *slab, int32_t *tmpl)
{
    const RaggedGraph &g = r.graphs[r.graph_of[i]];
    const int64_t arcs = r.arc_row[i], nodes = r.node_row[i];
    InstanceView v{};
    v.i = i; v.arc_row = arcs; v.node_row = nodes; v.n = g.n; v.m = g.m; v.supply_type = r.supply_type; v.trace_cap = r.trace_cap;
    v.source = r.source + g.ends; v.target = r.target + g.ends;
    v.inc_start = r.inc_start + g.inc_start; v.inc = r.inc + g.inc;
    v.lower = r.lower ? r.lower + arcs : nullptr; v.upper = r.upper ? r.upper + arcs : nullptr;
    v.cost = r.cost ? r.cost + arcs : nullptr; v.supply = r.supply ? r.supply + nodes : nullptr;
    v.start_state = r.start_state ? r.start_state + arcs : nullptr;
    if (slab) { v.workspace = r.workspace[i]; v.home = slab + v.workspace; }
    v.trace = (uint64_t)i * (uint64_t)r.trace_cap;
    if (o) {
        v.flows = output_row(o->flows, arcs); v.potentials = output_row(o->potentials, nodes);
        v.trace_row = o->trace ? o->trace + i * (int64_t)r.trace_cap : nullptr;
    }
    if (tmpl) *tmpl = g.tmpl;
    return v;
}
MCF_HD inline InstanceView ragged_check_view(const RaggedProblem &r, const int64_t *flows, const int64_t *potentials, int64_t i)
{
    InstanceView v = ragged_view(r, nullptr, i, nullptr, nullptr);
    v.check_flows = flows + r.arc_row[i]; v.check_potentials = potentials + r.node_row[i];
    return v;
}
// one way from a problem of either kind to a view.  *tmpl = the index of the instance's slot template: a uniform handle holds one
MCF_HD inline InstanceView view_of(const UniformProblem &p, const UniformOutputs *o, int64_t i, unsigned char *slab, int32_t *tmpl)
{
    if (tmpl) *tmpl = 0;
    return uniform_view(p, o, i, slab);
}
MCF_HD inline InstanceView view_of(const RaggedProblem &r, const UniformOutputs *o, int64_t i, unsigned char *slab, int32_t *tmpl) { return ragged_view(r, o, i, slab, tmpl); }
MCF_HD inline InstanceView check_view_of(const UniformProblem &p, const int64_t *flows, const int64_t *potentials, int64_t i) { return uniform_check_view(p, flows, potentials, i); }
MCF_HD inline InstanceView check_view_of(const RaggedProblem &r, const int64_t *flows, const int64_t *potentials, int64_t i) { return ragged_check_view(r, flows, potentials, i); }
MCF_HD inline int64_t uniform_upper(const int64_t *upper, int e) { return !upper || upper[e] == MCF_INF_CAP ? kInf : upper[e]; }       // core_set_problem
MCF_HD inline int64_t uniform_art_cost(const int64_t *cost, int n, int m, int lane, int lanes)     // art_cost_of
{
    int64_t biggest = 0;
    if (cost)
        for (int e = lane; e < m; e += lanes) {
            const int64_t a = cost[e] < 0 ? -cost[e] : cost[e];
            biggest = a > biggest ? a : biggest;
        }
    return (lanes_max_i64(biggest) + 1) * (int64_t)n;
}
// the slot of instance i at the start of a solve: the handle's template, placed
MCF_HD inline void uniform_place_slot(BatchSlot &slot, const BatchSlot &tmpl, const InstanceView &p, int32_t all_arcs, int32_t run)
{
    slot = tmpl;
    slot.all_arcs = all_arcs;
    slot.workspace = p.workspace;
    slot.trace = p.trace;
    slot.run = run;
}

// ---- core_begin for the instance p on its workspace.  The slot says afterwards whether there is anything to run.
MCF_HD inline void uniform_begin(const InstanceView &p, const BatchSlot &tmpl, BatchSlot &slot, int lane, int lanes)
{
    const int n = p.n, m = p.m, root = n;
    unsigned char *const home = p.home;
    const int64_t *const lower = p.lower, *const upper = p.upper, *const cost = p.cost, *const supply = p.supply;
    // NS.cs:227-231
    bool inverted = false;
    for (int e = lane; e < m; e += lanes) inverted |= uniform_upper(upper, e) < (lower ? lower[e] : 0);
    if (lanes_any(inverted)) {
        lanes_sync();
        if (lane == 0) uniform_place_slot(slot, tmpl, p, m + n, kBatchByBounds);
        return;
    }
    // to_standard_form.  The supplies are not part of the workspace and all_arcs -- with it, where every array lies -- is known only once they
    // have been shifted by the lower bounds.  They are shifted where pi[] lies when every node needs an artificial arc (no layout of this
    // instance puts pi[] further back), then moved down to where pi[] does lie; the start basis below reads each and overwrites it.
    // Order on the device: plain stores of shifted[v], barrier, atomic adds on the same words (they meet in L2), barrier, plain loads by
    // other lanes.  It is the fence that comes with each lanes_sync() (a workgroup-scope release / acquire round the barrier) that puts
    // the stores before the atomics and the atomics before the loads; that covers every lane that touches the words only because the
    // workgroup is ONE wave on one CU.  Several workgroups on one instance would need agent-scope fences.
    int64_t *const shifted = (int64_t *)(home + layout_of((uint32_t)(m + 2 * n), (uint32_t)n + 1u).pi);
    for (int v = lane; v < n; v += lanes) shifted[v] = supply ? supply[v] : 0;
    lanes_sync();
    if (lower)
        for (int e = lane; e < m; e += lanes) {
            const int64_t lo = lower[e];
            if (lo == 0) continue;
            lanes_add_i64(&shifted[p.source[e]], -lo);
            lanes_add_i64(&shifted[p.target[e]], lo);
        }
    lanes_sync();
    const int64_t art_cost = uniform_art_cost(cost, n, m, lane, lanes);
    const bool geq = p.supply_type == MCF_SUPPLY_GEQ;
    int32_t hung = 0;               // nodes that cannot hang on their root link
    for (int base = 0; base < n; base += lanes) {
        const int v = base + lane;
        hung += popcount64(lanes_ballot(v < n && (geq ? shifted[v] > 0 : shifted[v] < 0)));
    }
    const int32_t all_arcs = m + n + hung;
    const Layout l = layout_of((uint32_t)all_arcs, (uint32_t)n + 1u);
    int32_t *const tail = (int32_t *)(home + l.tail), *const head = (int32_t *)(home + l.head);
    int64_t *const cost_w = (int64_t *)(home + l.cost), *const upper_w = (int64_t *)(home + l.upper);
    int64_t *const flow = (int64_t *)(home + l.flow), *const pi = (int64_t *)(home + l.pi);
    int32_t *const par = (int32_t *)(home + l.par), *const par_arc = (int32_t *)(home + l.par_arc), *const nxt = (int32_t *)(home + l.nxt);
    int32_t *const prv = (int32_t *)(home + l.prv), *const sub = (int32_t *)(home + l.sub), *const fin = (int32_t *)(home + l.fin);
    int8_t *const state = (int8_t *)(home + l.state), *const par_dir = (int8_t *)(home + l.par_dir);
    // pi <= shifted, both on 16-byte boundaries: moving up the array, an entry lands on entries that have been read
    if (pi != shifted)
        for (int base = 0; base < n; base += lanes) {
            const int v = base + lane;
            const int64_t s = v < n ? shifted[v] : 0;
            lanes_sync();
            if (v < n) pi[v] = s;
        }
    lanes_sync();
    // the arcs of the problem (start_basis: at their lower bound, which is 0 now)
    for (int e = lane; e < m; e += lanes) {
        tail[e] = p.source[e]; head[e] = p.target[e];
        cost_w[e] = cost ? cost[e] : 0;
        upper_w[e] = uniform_upper(upper, e) - (lower ? lower[e] : 0);
        flow[e] = 0;
        state[e] = MCF_STATE_LOWER;
    }
    // NS.cs:671-845, the star on the artificial root.  Node v's artificial arc is m + n + (nodes below v that need one): an exclusive prefix
    // count, per stride a ballot and the bits below the lane, with the strides before it as the running base.
    int32_t before = 0;
    for (int base = 0; base < n; base += lanes) {
        const int v = base + lane;
        const int64_t s = v < n ? pi[v] : 0;
        const bool plain = geq ? s <= 0 : s >= 0;
        const uint64_t mask = lanes_ballot(v < n && !plain);
        const int extra = m + n + before + popcount64(mask & (((uint64_t)1 << lane) - 1));
        before += popcount64(mask);
        if (v >= n) continue;
        const int link = m + v;
        const int lt = geq ? root : v, lh = geq ? v : root;         // the zero-cost link: GEQ root->v, LEQ v->root
        par[v] = root; sub[v] = 1; fin[v] = v;
        nxt[v] = v + 1 < n ? v + 1 : root;
        prv[v] = v > 0 ? v - 1 : root;
        tail[link] = lt; head[link] = lh; upper_w[link] = kInf; cost_w[link] = 0;
        if (plain) {
            par_dir[v] = geq ? kDown : kUp;
            pi[v] = 0;
            par_arc[v] = link;
            flow[link] = geq ? -s : s;
            state[link] = MCF_STATE_TREE;
        } else {
            par_dir[v] = geq ? kUp : kDown;
            pi[v] = geq ? -art_cost : art_cost;
            par_arc[v] = extra;
            tail[extra] = lh; head[extra] = lt;
            upper_w[extra] = kInf;
            flow[extra] = geq ? s : -s;
            cost_w[extra] = art_cost;
            state[extra] = MCF_STATE_TREE;
            flow[link] = 0;
            state[link] = MCF_STATE_LOWER;
        }
    }
    if (lane == 0) {
        par[root] = -1; par_arc[root] = -1; nxt[root] = n > 0 ? 0 : root; prv[root] = n > 0 ? n - 1 : root;
        sub[root] = n + 1; fin[root] = n - 1; par_dir[root] = 0; pi[root] = 0;
        uniform_place_slot(slot, tmpl, p, all_arcs, kBatchRunning);
    }
    lanes_sync();
}

// ---- finish_instance + core_finish + core_total_cost for instance i, into the caller's rows.  The flows in the workspace stay in standard
// form: the lower bounds are added into the output row only, so a re-solve goes on from the workspace as it is.
MCF_HD inline void uniform_finish(const InstanceView &p, const UniformOutputs &o, const BatchSlot &slot, const int32_t *traces, int lane, int lanes)
{
    const int n = p.n, m = p.m;
    const int64_t i = p.i;
    const unsigned char *const home = p.home;
    const Layout l = layout_of((uint32_t)slot.all_arcs, (uint32_t)n + 1u);
    const int64_t *const flow = (const int64_t *)(home + l.flow), *const pi = (const int64_t *)(home + l.pi), *const cost = (const int64_t *)(home + l.cost);
    const int64_t *const lower = p.lower;
    int32_t status = MCF_NOT_SOLVED;                                    // the pivot limit
    switch (slot.run) {
    case kBatchNoEntering: {
        // NS.cs:1272-1283 with difference D9: only the n root links
        bool left = false;
        for (int e = m + lane; e < m + n; e += lanes) left |= flow[e] != 0;
        status = lanes_any(left) ? MCF_INFEASIBLE : MCF_OPTIMAL;
        break;
    }
    case kBatchUnbounded: status = MCF_UNBOUNDED; break;
    case kBatchMaxIter: case kBatchByBounds: status = MCF_INFEASIBLE; break;
    default: break;
    }
    const int64_t pivots = slot.run == kBatchByBounds ? 0 : slot.pivots;
    const bool optimal = status == MCF_OPTIMAL;
    uint64_t total = 0;
    int64_t *const flows = p.flows, *const potentials = p.potentials;
    for (int e = lane; e < m; e += lanes) {
        const int64_t f = optimal ? (int64_t)((uint64_t)flow[e] + (uint64_t)(lower ? lower[e] : 0)) : 0;      // NS.cs:364-388
        if (optimal) total += (uint64_t)f * (uint64_t)cost[e];                                                // NS.cs:459-464, wrapping
        if (flows) flows[e] = f;
    }
    total = lanes_sum_u64(total);
    if (potentials)
        for (int v = lane; v < n; v += lanes) potentials[v] = optimal ? pi[v] : 0;
    if (p.trace_row) {
        const int64_t cap = p.trace_cap, len = pivots < cap ? pivots : cap;
        int32_t *const row = p.trace_row;
        for (int64_t k = lane; k < cap; k += lanes) row[k] = k < len ? traces[slot.trace + (uint64_t)k] : 0;
    }
    if (lane == 0) {
        if (o.status) o.status[i] = status;
        if (o.pivots) o.pivots[i] = pivots;
        if (o.total_cost) o.total_cost[i] = (int64_t)total;
    }
}

// ---- whether the last solve call of any kind left instance p with an optimal basis that is worth keeping: no entering arc, and no flow
// on a root link (Infeasible) or on an artificial arc (Optimal with a surplus whose place depends on the pivot path).  What a warm start
// with new costs demands (uniform_recost) and what makes the basis' cost ranges mean something (uniform_ranges of ranges_step.hip.h).
MCF_HD inline bool uniform_kept_optimal(const InstanceView &p, const BatchSlot &slot, int lane, int lanes)
{
    if (slot.run != kBatchNoEntering) return false;
    const int32_t all_arcs = slot.all_arcs;
    const int64_t *const flow = (const int64_t *)(p.home + layout_of((uint32_t)all_arcs, (uint32_t)p.n + 1u).flow);
    bool left = false;
    for (int e = p.m + lane; e < all_arcs; e += lanes) left |= flow[e] != 0;
    return !lanes_any(left);
}

// ---- prepare_resolve for instance i with the costs in p.  Warm as there: the last solve ended Optimal with no flow on an artificial arc.
MCF_HD inline void uniform_recost(const InstanceView &p, const BatchSlot &tmpl, BatchSlot &slot, int lane, int lanes)
{
    const int n = p.n, m = p.m;
    unsigned char *const home = p.home;
    const int32_t all_arcs = slot.all_arcs;
    if (!uniform_kept_optimal(p, slot, lane, lanes)) { uniform_begin(p, tmpl, slot, lane, lanes); return; }
    // core_recost: cost[0, m), art_cost as to_standard_form derives it, the artificial arcs; the root links keep 0
    const Layout l = layout_of((uint32_t)all_arcs, (uint32_t)n + 1u);
    int64_t *const cost_w = (int64_t *)(home + l.cost);
    const int64_t *const cost = p.cost;
    const int64_t art_cost = uniform_art_cost(cost, n, m, lane, lanes);
    for (int e = lane; e < m; e += lanes) cost_w[e] = cost ? cost[e] : 0;
    for (int e = m + n + lane; e < all_arcs; e += lanes) cost_w[e] = art_cost;
    lanes_sync();
    if (lane == 0) {                    // the rule starts as at a cold start, the count and the trace start again
        uniform_place_slot(slot, tmpl, p, all_arcs, kBatchRunning);
        slot.reprice = 1;
    }
    lanes_sync();
}

// ---- the flows of the basis that lies in p's workspace, under the lower, upper and supply in p: the new capacities go in, every non-tree
// arc's flow follows its state, and the tree flows are recomputed -- node v's excess is gathered into flow[par_arc[v]] (every node below
// the root owns one tree arc), folded root-ward up the reverse thread list, children before parents, and turned by par_dir.  The sums wrap
// and commute like uniform_begin's, so one lane and 64 lanes give the same bits.  scratch[] is cleared: no mark of an earlier dual phase
// is left (batch_dual_run).  Shared by uniform_redata (the kept basis) and uniform_begin_from (the caller's); lane 0 leaves with the
// flows written, the caller's lanes_sync() publishes them.
MCF_HD inline void uniform_tree_flows(const InstanceView &p, int32_t all_arcs, int lane, int lanes)
{
    const int n = p.n, m = p.m;
    unsigned char *const home = p.home;
    const int64_t *const lower = p.lower, *const upper = p.upper, *const supply = p.supply;
    const Layout l = layout_of((uint32_t)all_arcs, (uint32_t)n + 1u);
    int64_t *const upper_w = (int64_t *)(home + l.upper), *const flow = (int64_t *)(home + l.flow);
    const int32_t *const par = (const int32_t *)(home + l.par), *const par_arc = (const int32_t *)(home + l.par_arc), *const prv = (const int32_t *)(home + l.prv);
    int32_t *const scratch = (int32_t *)(home + l.scratch);
    const int8_t *const state = (const int8_t *)(home + l.state), *const par_dir = (const int8_t *)(home + l.par_dir);
    // plain stores, barrier, atomic adds on the same words, barrier, plain loads: the order uniform_begin explains
    for (int v = lane; v < n; v += lanes) flow[par_arc[v]] = supply ? supply[v] : 0;
    for (int v = lane; v < n + 2; v += lanes) scratch[v] = 0;
    lanes_sync();
    for (int e = lane; e < m; e += lanes) {
        const int64_t lo = lower ? lower[e] : 0, cap = uniform_upper(upper, e) - lo;
        upper_w[e] = cap;
        int64_t carried = lo;                                               // what the arc moves from its tail to its head, decided here
        if (state[e] != MCF_STATE_TREE) {
            const int64_t f = state[e] == MCF_STATE_UPPER ? cap : 0;
            flow[e] = f;
            carried = (int64_t)((uint64_t)carried + (uint64_t)f);
        }
        if (carried == 0) continue;
        lanes_add_i64(&flow[par_arc[p.source[e]]], -carried);
        lanes_add_i64(&flow[par_arc[p.target[e]]], carried);
    }
    for (int e = m + lane; e < all_arcs; e += lanes)
        if (state[e] != MCF_STATE_TREE) flow[e] = 0;
    lanes_sync();
    if (lane == 0) {
        // exactly n steps by count, like batch_reprice: the reverse thread list visits every node behind all of its subtree
        const int root = n;
        int u = prv[root];
        for (int i = 0; i < n && (unsigned)u < (unsigned)root; ++i) {
            const int e = par_arc[u], up = par[u];
            const int64_t below = flow[e];                                  // the excess of u's subtree: it leaves through u's tree arc
            if (up != root) flow[par_arc[up]] = (int64_t)((uint64_t)flow[par_arc[up]] + (uint64_t)below);
            flow[e] = par_dir[u] * below;
            u = prv[u];
        }
    }
}

// ---- a re-solve with new lower, upper and supply in p (costs and supply type are the last solve's).  The kept basis stays dual feasible:
// WARM where the last solve ended as uniform_recost asks, no non-tree arc at its upper bound has lost that bound, and the new supplies sum
// to zero (the lower bounds' shifts cancel in the sum; a surplus is answered by an artificial arc whose place depends on the pivot path).
// Warm: uniform_tree_flows above.
// The slot leaves with run = kBatchDual and reprice = 2: batch_dual_run goes first, and uniform_redata_settle judges the attempt.
// Anything else: uniform_begin with the new data, a fresh solve bit for bit.
MCF_HD inline void uniform_redata(const InstanceView &p, const BatchSlot &tmpl, BatchSlot &slot, int lane, int lanes)
{
    const int n = p.n, m = p.m;
    unsigned char *const home = p.home;
    const int64_t *const lower = p.lower, *const upper = p.upper, *const supply = p.supply;
    const int32_t all_arcs = slot.all_arcs;
    bool inverted = false;
    for (int e = lane; e < m; e += lanes) inverted |= uniform_upper(upper, e) < (lower ? lower[e] : 0);
    if (lanes_any(inverted)) { uniform_begin(p, tmpl, slot, lane, lanes); return; }         // kBatchByBounds, nothing runs
    bool warm = slot.run == kBatchNoEntering;
    if (warm) {
        const Layout l = layout_of((uint32_t)all_arcs, (uint32_t)n + 1u);
        const int64_t *const flow = (const int64_t *)(home + l.flow);
        const int8_t *const state = (const int8_t *)(home + l.state);
        bool cold = false;
        for (int e = m + lane; e < all_arcs; e += lanes) cold |= flow[e] != 0;
        for (int e = lane; e < m; e += lanes) cold |= state[e] == MCF_STATE_UPPER && uniform_upper(upper, e) >= kInf;
        uint64_t sum = 0;
        if (supply)
            for (int v = lane; v < n; v += lanes) sum += (uint64_t)supply[v];
        warm = !lanes_any(cold) && lanes_sum_u64(sum) == 0;
    }
    if (!warm) { uniform_begin(p, tmpl, slot, lane, lanes); return; }
    uniform_tree_flows(p, all_arcs, lane, lanes);
    if (lane == 0) {
        uniform_place_slot(slot, tmpl, p, all_arcs, kBatchDual);
        slot.reprice = 2;
    }
    lanes_sync();
}

// ---- the end of a warm attempt of uniform_redata (slot.reprice == 2, which this clears).  It stands when the dual phase handed over,
// the primal phase found no entering arc and no flow is left on a root link or an artificial arc; an instance stopped by the pivot limit
// stays stopped.  Anything else -- dual stuck, Unbounded, the iteration guard, flow left on [m, all_arcs) -- starts again cold with the
// same data: the slot says so (kBatchRunning) and the caller runs it.
MCF_HD inline void uniform_redata_settle(const InstanceView &p, const BatchSlot &tmpl, BatchSlot &slot, int lane, int lanes)
{
    if (slot.reprice != 2) return;
    const int n = p.n, m = p.m;
    const int32_t all_arcs = slot.all_arcs, run = slot.run;
    bool stands = run == kBatchLimit;
    if (run == kBatchNoEntering) {
        const int64_t *const flow = (const int64_t *)(p.home + layout_of((uint32_t)all_arcs, (uint32_t)n + 1u).flow);
        bool left = false;
        for (int e = m + lane; e < all_arcs; e += lanes) left |= flow[e] != 0;
        stands = !lanes_any(left);
    }
    lanes_sync();
    if (stands) {
        if (lane == 0) slot.reprice = 0;
        return;
    }
    uniform_begin(p, tmpl, slot, lane, lanes);
}

// ---- a solve that starts from a basis the caller supplies (mcf_*batch_solve_from, DESIGN.md 3.14 "Start from a given basis"):
// p.start_state holds one state per arc of the caller's, LOWER / TREE / UPPER, as uniform_ranges writes arc_state.  The TREE arcs must
// form a forest on the n nodes.  uniform_start_try builds the basis in the workspace and says whether it is one the pivots can go on
// from; false = COLD BY RULE, and nothing it wrote counts.  In this order:
//   1. what uniform_begin checks and derives (bounds, art_cost), the row's values, the supplies' sum, and the number of TREE arcs T: a
//      forest of T arcs has n - T components, which fixes all_arcs = m + n + (n - T) and with it where every array lies -- before the walk,
//      as uniform_begin counts `hung` before it places anything;
//   2. the arcs [0, m) in standard form with the row's states, the n root links at LOWER with flow 0;
//   3. the forest, on lane 0: a depth-first walk over the incidence lists (arc ids ascending per node), components by ascending lowest
//      node and rooted there.  It needs no stack: the way back is par[], and each node's cursor into its list lies in scratch[], which
//      uniform_tree_flows clears afterwards.  par[v] = -1 marks a node not reached yet.  A TREE arc that reaches a reached node -- a cycle,
//      the second of two parallel arcs, a self loop -- ends the walk: cold.  The walk writes par, par_arc, par_dir, nxt, prv, sub, fin in
//      preorder and is bounded by count: each step starts a component (<= n), moves a cursor (<= 2m) or leaves a node (<= n);
//   4. component k hangs on the root by the artificial arc m + n + k of its lowest node, directed and costed as uniform_begin's for a node
//      that cannot use its root link.  Not by the root link: that would give the node potential 0 and make the other nodes' root links
//      eligible, while after a real solve every potential lies beyond -/+ art_cost ("A limit that follows from the definition");
//   5. flows by uniform_tree_flows, potentials by batch_reprice;
//   6. the class.  Flow on an artificial arc (a component that does not balance by itself): cold.  Every caller's tree arc within its
//      bounds: a PRIMAL start, run = kBatchRunning.  Else every non-tree arc of [0, search_arcs) with state * reduced cost >= 0: a DUAL
//      start, run = kBatchDual.  Else cold.
// Both accepted kinds leave reprice = 2, so batch_run_after_dual runs them and uniform_redata_settle judges them as it judges a warm
// attempt of uniform_redata.  Cold by rule is uniform_begin on the same view: a fresh solve bit for bit.
MCF_HD inline bool uniform_start_try(const InstanceView &p, const BatchSlot &tmpl, BatchSlot &slot, int lane, int lanes)
{
    const int n = p.n, m = p.m, root = n;
    unsigned char *const home = p.home;
    const int64_t *const lower = p.lower, *const upper = p.upper, *const cost = p.cost, *const supply = p.supply;
    const int8_t *const row = p.start_state;
    bool bad = false;
    uint64_t trees = 0, sum = 0;
    for (int e = lane; e < m; e += lanes) {
        const int8_t st = row[e];
        const int64_t up = uniform_upper(upper, e);
        bad |= up < (lower ? lower[e] : 0) || st < MCF_STATE_UPPER || st > MCF_STATE_LOWER || (st == MCF_STATE_UPPER && up >= kInf);
        trees += st == MCF_STATE_TREE;
    }
    if (supply)
        for (int v = lane; v < n; v += lanes) sum += (uint64_t)supply[v];
    trees = lanes_sum_u64(trees);
    if (lanes_any(bad) || lanes_sum_u64(sum) != 0 || trees >= (uint64_t)n) return false;        // n = 0 too: nothing to hang
    const int32_t comps = n - (int32_t)trees, all_arcs = m + n + comps;
    const int64_t art_cost = uniform_art_cost(cost, n, m, lane, lanes);
    const bool geq = p.supply_type == MCF_SUPPLY_GEQ;
    const Layout l = layout_of((uint32_t)all_arcs, (uint32_t)n + 1u);
    int32_t *const tail = (int32_t *)(home + l.tail), *const head = (int32_t *)(home + l.head);
    int64_t *const cost_w = (int64_t *)(home + l.cost), *const upper_w = (int64_t *)(home + l.upper), *const flow = (int64_t *)(home + l.flow);
    int32_t *const par = (int32_t *)(home + l.par), *const par_arc = (int32_t *)(home + l.par_arc), *const nxt = (int32_t *)(home + l.nxt);
    int32_t *const prv = (int32_t *)(home + l.prv), *const sub = (int32_t *)(home + l.sub), *const fin = (int32_t *)(home + l.fin);
    int32_t *const cursor = (int32_t *)(home + l.scratch);
    int8_t *const state = (int8_t *)(home + l.state), *const par_dir = (int8_t *)(home + l.par_dir);
    for (int e = lane; e < m; e += lanes) {
        tail[e] = p.source[e]; head[e] = p.target[e];
        cost_w[e] = cost ? cost[e] : 0;
        upper_w[e] = uniform_upper(upper, e) - (lower ? lower[e] : 0);
        flow[e] = 0;
        state[e] = row[e];
    }
    for (int v = lane; v < n; v += lanes) {
        const int link = m + v;
        tail[link] = geq ? root : v; head[link] = geq ? v : root;   // the zero-cost link: GEQ root->v, LEQ v->root
        upper_w[link] = kInf; cost_w[link] = 0; flow[link] = 0; state[link] = MCF_STATE_LOWER;
        par[v] = -1; sub[v] = 1; cursor[v] = p.inc_start[v];
    }
    lanes_sync();
    int32_t forest = 1;
    if (lane == 0) {
        int last = root, u = -1, lowest = 0;
        int32_t k = 0;
        int64_t steps = 2 * (int64_t)m + 2 * (int64_t)n + 1;
        for (;;) {
            if (steps-- <= 0) { forest = 0; break; }
            if (u < 0) {                                            // the next component: the lowest node not reached yet
                while (lowest < n && par[lowest] != -1) ++lowest;
                if (lowest >= n) break;
                if (k >= comps) { forest = 0; break; }              // more components than a forest of `trees` arcs has: there is a cycle
                u = lowest;
                const int extra = m + n + k++;
                par[u] = root; par_arc[u] = extra; par_dir[u] = geq ? kUp : kDown;
                tail[extra] = geq ? u : root; head[extra] = geq ? root : u;
                upper_w[extra] = kInf; cost_w[extra] = art_cost; flow[extra] = 0; state[extra] = MCF_STATE_TREE;
                nxt[last] = u; prv[u] = last; last = u;
                continue;
            }
            const int32_t at = cursor[u];
            if (at >= p.inc_start[u + 1]) {                         // u's list is done: back up
                const int up = par[u];
                fin[u] = last;
                if (up != root) sub[up] += sub[u];
                u = up != root ? up : -1;
                continue;
            }
            cursor[u] = at + 1;
            const int32_t entry = p.inc[at], e = entry >> 1;
            if (row[e] != MCF_STATE_TREE || e == par_arc[u]) continue;
            const bool incoming = (entry & 1) != 0;                 // u is e's target: the other end is its tail
            const int v = incoming ? p.source[e] : p.target[e];
            if (par[v] != -1) { forest = 0; break; }
            par[v] = u; par_arc[v] = e; par_dir[v] = incoming ? kUp : kDown;
            nxt[last] = v; prv[v] = last; last = v;
            u = v;
        }
        if (k != comps) forest = 0;
        nxt[last] = root; prv[root] = last;                         // last = root where nothing was reached: n > 0 rules that out
        par[root] = -1; par_arc[root] = -1; sub[root] = n + 1; fin[root] = last; par_dir[root] = 0;
    }
    lanes_sync();
    if (!lanes_from_first(forest)) return false;
    uniform_tree_flows(p, all_arcs, lane, lanes);
    BatchWork w{};
    bind(w, home, l);
    w.n = n; w.search_arcs = tmpl.search_arcs;
    batch_reprice(w, lane, lanes);
    bool unbalanced = false, outside = false, eligible = false;
    for (int e = m + n + lane; e < all_arcs; e += lanes) unbalanced |= flow[e] != 0;
    for (int e = lane; e < m; e += lanes) outside |= state[e] == MCF_STATE_TREE && (flow[e] < 0 || flow[e] > upper_w[e]);
    for (int e = lane; e < w.search_arcs; e += lanes) eligible |= state[e] != MCF_STATE_TREE && batch_reduced_cost(w, e) < 0;
    if (lanes_any(unbalanced)) return false;
    const bool primal = !lanes_any(outside);
    if (!primal && lanes_any(eligible)) return false;
    if (lane == 0) {
        uniform_place_slot(slot, tmpl, p, all_arcs, primal ? kBatchRunning : kBatchDual);
        slot.reprice = 2;
    }
    lanes_sync();
    return true;
}
MCF_HD inline void uniform_begin_from(const InstanceView &p, const BatchSlot &tmpl, BatchSlot &slot, int lane, int lanes)
{
    if (uniform_start_try(p, tmpl, slot, lane, lanes)) return;
    lanes_sync();                       // what the attempt read in the workspace has been read
    uniform_begin(p, tmpl, slot, lane, lanes);
}

// ---- the reference's SolutionValidator (SolutionValidator.cs, restated in oracle/validator.py) for instance i of a solution that lies in
// rows as uniform_finish writes them.  It belongs to no solve: it reads the problem, the solution and the handle's incidence lists, and
// writes the instance's row of answers; slab and slots are not its business.
// The incidence lists (built once per graph at create): node v's entries are inc[inc_start[v], inc_start[v + 1]), each
// arc << 1 | (v is the arc's target), arc ids ascending.  With them a node sums its own arcs: no atomics, no scratch per instance.
// Every sum is an unsigned 64-bit add (C# long, unchecked), so one lane and 64 lanes give the same bits; `first` is a minimum.

// the two words every invalid instance meets on
MCF_HD inline void uniform_report_invalid(int64_t *summary, int64_t i)
{
#if defined(__HIP_DEVICE_COMPILE__)
    atomicAdd((unsigned long long *)&summary[0], 1ull);
    atomicMin((long long *)&summary[1], (long long)i);
#else
    summary[0] += 1;
    summary[1] = i < summary[1] ? i : summary[1];
#endif
}

MCF_HD inline void uniform_validate(const InstanceView &p, const UniformCheck &c, int lane, int lanes)
{
    const int n = p.n, m = p.m;
    const int64_t i = p.i;
    uint64_t count[MCF_VAL_KINDS] = {};                  // this lane's share, folded below
    uint32_t first[MCF_VAL_KINDS];
    for (int k = 0; k < MCF_VAL_KINDS; ++k) first[k] = kNoPos;              // (int32_t)kNoPos = -1
    uint64_t objective = 0, dual = 0;
    const bool optimal = c.status[i] == MCF_OPTIMAL;
    if (!optimal) {                                      // SolutionValidator.cs:28-33: nothing else is read
        count[MCF_VAL_STATUS] = 1;
        first[MCF_VAL_STATUS] = 0;
    } else {
        const int64_t *const lower = p.lower, *const upper = p.upper, *const cost = p.cost, *const supply = p.supply;
        const int64_t *const flow = p.check_flows, *const pi = p.check_potentials;
        const auto note = [&](int kind, bool failed, int id) {
            if (!failed) return;
            ++count[kind];
            first[kind] = (uint32_t)id < first[kind] ? (uint32_t)id : first[kind];
        };
        // the arcs: :104-124, :146-177, :232-255 and the arc terms of :276-331
        for (int e = lane; e < m; e += lanes) {
            const int64_t lo = lower ? lower[e] : 0, up = uniform_upper(upper, e), co = cost ? cost[e] : 0, f = flow[e];
            const int64_t rc = (int64_t)((uint64_t)co + (uint64_t)pi[p.source[e]] - (uint64_t)pi[p.target[e]]);
            note(MCF_VAL_LOWER, f < lo, e);
            note(MCF_VAL_UPPER, f > up, e);
            note(MCF_VAL_SLACK_POS, rc > 0 && f != lo, e);
            note(MCF_VAL_SLACK_NEG, rc < 0 && f != up, e);
            objective += (uint64_t)f * (uint64_t)co;
            dual += (uint64_t)lo * (uint64_t)co;
            if (rc < 0) dual -= ((uint64_t)up - (uint64_t)lo) * ((uint64_t)0 - (uint64_t)rc);
        }
        // the nodes: :62-99, :193-227 and the node terms of :276-331.  One lane per node walks the node's own arcs.
        for (int v = lane; v < n; v += lanes) {
            uint64_t net = 0, adj = 0;                   // flow out - flow in; the lower bounds' shift of the supply
            for (int32_t k = p.inc_start[v]; k < p.inc_start[v + 1]; ++k) {
                const int32_t entry = p.inc[k], e = entry >> 1;
                const bool incoming = (entry & 1) != 0;
                const uint64_t f = (uint64_t)flow[e], lo = lower ? (uint64_t)lower[e] : 0;
                net = incoming ? net - f : net + f;
                adj = incoming ? adj + lo : adj - lo;
            }
            const int64_t nf = (int64_t)net, sp = supply ? supply[v] : 0, pv = pi[v];
            note(MCF_VAL_CONSERVATION, p.supply_type == MCF_SUPPLY_GEQ ? nf < sp : (p.supply_type == MCF_SUPPLY_LEQ ? nf > sp : nf != sp), v);
            if (p.supply_type == MCF_SUPPLY_GEQ) {
                note(MCF_VAL_NODE_DUAL, pv > 0, v);
                note(MCF_VAL_NODE_SLACK, pv < 0 && nf != sp, v);
            } else if (p.supply_type == MCF_SUPPLY_LEQ) {
                note(MCF_VAL_NODE_DUAL, pv < 0, v);
                note(MCF_VAL_NODE_SLACK, pv > 0 && nf != sp, v);
            }
            dual -= ((uint64_t)sp + adj) * (uint64_t)pv;
        }
        objective = lanes_sum_u64(objective);
        dual = lanes_sum_u64(dual);
        for (int k = 0; k < MCF_VAL_OBJECTIVE; ++k) {
            count[k] = lanes_sum_u64(count[k]);
            first[k] = lanes_min_u32(first[k]);
        }
        const int64_t reported = c.total_cost[i];
        if ((int64_t)objective != reported) { count[MCF_VAL_OBJECTIVE] = 1; first[MCF_VAL_OBJECTIVE] = 0; }                // :257-262
        if ((int64_t)dual != reported) { count[MCF_VAL_DUAL_COST] = 1; first[MCF_VAL_DUAL_COST] = 0; }                     // :333-339
    }
    if (lane != 0) return;
    bool valid = true;
    for (int k = 0; k < MCF_VAL_KINDS; ++k) {
        valid &= count[k] == 0;
        if (c.errors) c.errors[i * MCF_VAL_KINDS + k] = (int32_t)count[k];
        if (c.first) c.first[i * MCF_VAL_KINDS + k] = (int32_t)first[k];
    }
    if (c.valid) c.valid[i] = valid ? 1 : 0;
    if (c.objective) c.objective[i] = (int64_t)objective;
    if (c.dual_cost) c.dual_cost[i] = (int64_t)dual;
    if (!valid) uniform_report_invalid(c.summary, i);
}

}  // namespace mcf
