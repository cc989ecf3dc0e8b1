// batch_step.hip.h -- ONE network-simplex pivot of the batch solver (batch.hip), stated once for host and device.
//
// The functions work on a BatchWork: the TreeView of tree_pivot.h, the other arrays mcf_ns keeps (ns_core.h) and the pivot rule's state.  They never learn
// where the pointers point: the kernel binds them to LDS or to the instance's workspace in global memory, mcf_batch_run_on_host binds
// them to host vectors.  Two halves per pivot:
//   * the entering-arc search is written over (lane, lanes): 64 lanes of one wave share it on the device, one "lane" runs it on the host.
//     What the lanes found is combined by lanes_min_* (a wave reduction on the device, the identity on the host), so every lane leaves
//     the search with the same answer and the same rule state.  Rules: First Eligible, Best Eligible and the plain Block Search of
//     NS.cs:1292-1668 (find_first / find_best / find_block_plain of oracle/ns_oracle.c), ties broken as there: the first arc in scan
//     order among equals.
//     A fourth search belongs to the dual phase (batch_dual_run): the leaving arc by the largest bound violation over the nodes, then the
//     ratio test over the arcs across the leaving arc's cut.
//   * join node, leaving arc, State[] writes, potentials of the subtree, flows round the cycle and the tree surgery are sequential:
//     batch_pivot calls the steps of tree_pivot.h (the ones mcf_ns calls) in the reference's order, with the plain walk over the subtree's
//     potentials between them.  Lane 0 runs it while the others wait.
// block_adapt_step is the arithmetic of mcf_block_adapt (NS.cs:1400-1438); util.cpp calls it, so there is one statement of it.
#pragma once

#include <stdint.h>

#include "../../include/mcf_hip.h"
#include "tree_pivot.h"

namespace mcf {

// how a slice of pivots ended (BatchWork::run)
enum BatchRun : int32_t {
    kBatchRunning = 0,     // the slice's budget ran out: relaunch
    kBatchNoEntering = 1,  // no eligible arc: the host finishes (feasibility, lower bounds)
    kBatchUnbounded = 2,   // NS.cs:321-325
    kBatchLimit = 3,       // the instance's pivot limit
    kBatchMaxIter = 4,     // the reference's own iteration guard (NS.cs:280, :311-317): Infeasible
    kBatchByBounds = 5,    // never ran: an upper bound below its lower bound (set by uniform_begin of uniform_step.hip.h only)
    kBatchDual = 6,        // a re-solve with new supplies or bounds: the dual phase is in progress (batch_dual_run): relaunch
    kBatchDualStuck = 7    // the dual phase found a violated tree arc and no arc across its cut to enter: the warm attempt is given up
};

struct BatchWork : TreeView {
    // arcs [0, all_arcs); the rules scan [0, search_arcs)
    const int64_t *cost;
    int8_t *state;
    // nodes [0, n], n = the artificial root
    int64_t *pi;
    int32_t *trace;                    // entering arc of every pivot, up to trace_cap (may be null)
    int32_t n, search_arcs, rule;
    // the rule's state
    int32_t next_arc, block_size, dyn_min;
    int32_t counters[2];               // _consecutiveLowHits, _consecutiveHighHits
    mcf_block_config cfg;
    int64_t pivots, pivot_limit, max_iter, trace_cap;
    int32_t run;                       // BatchRun
    int64_t dual_pivots;               // of `pivots`, those of the dual phase (batch_dual_run only; the slot keeps it in staged_out)
};

// ---- NS.cs:1400-1438, same doubles, same truncations (a product and a quotient each rounded once: nothing here can be contracted into an FMA)
MCF_HD inline void block_adapt_step(const mcf_block_config *c, int32_t dynamic_min, int64_t arcs_checked, int32_t *block_size, int32_t counters[2])
{
#pragma clang fp contract(off)
    if (!(c->flags & MCF_OPT_ADAPTIVE_BLOCK_SIZE)) return;
    const double hit_rate = arcs_checked > 0 ? 1.0 / (double)arcs_checked : 0;
    if (hit_rate < c->low_hit_rate_threshold) {
        counters[1] = 0;
        if (++counters[0] >= c->consecutive_hits_before_adapt) {
            const int smaller = (int)(*block_size * c->block_size_shrink_factor);
            *block_size = dynamic_min > smaller ? dynamic_min : smaller;
            counters[0] = 0;
        }
    } else if (hit_rate > c->high_hit_rate_threshold) {
        counters[0] = 0;
        if (++counters[1] >= c->consecutive_hits_before_adapt) {
            const int larger = (int)(*block_size * c->block_size_growth_factor);
            *block_size = c->max_block_size < larger ? c->max_block_size : larger;
            counters[1] = 0;
        }
    } else {
        counters[0] = counters[1] = 0;
    }
}

// ---- what the lanes of a search share.  Device: all 64 lanes of the wave call these together.
MCF_HD inline int64_t lanes_min_i64(int64_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    for (int d = 32; d > 0; d >>= 1) { const int64_t o = __shfl_xor(v, d, 64); v = o < v ? o : v; }
#endif
    return v;
}
MCF_HD inline int64_t lanes_max_i64(int64_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    for (int d = 32; d > 0; d >>= 1) { const int64_t o = __shfl_xor(v, d, 64); v = o > v ? o : v; }
#endif
    return v;
}
MCF_HD inline uint32_t lanes_min_u32(uint32_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    for (int d = 32; d > 0; d >>= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)v, d, 64); v = o < v ? o : v; }
#endif
    return v;
}
MCF_HD inline int32_t lanes_from_first(int32_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    v = __shfl(v, 0, 64);
#endif
    return v;
}
// what lane 0 wrote is visible to every lane behind this, and what the lanes read in front of it has been read (one wave per workgroup)
MCF_HD inline void lanes_sync()
{
#if defined(__HIP_DEVICE_COMPILE__)
    __syncthreads();
#endif
}

constexpr uint32_t kNoPos = 0xFFFFFFFFu;

MCF_HD inline int64_t batch_reduced_cost(const BatchWork &w, int e)      // NS.cs:1351-1352
{
    return (int64_t)w.state[e] * (w.cost[e] + w.pi[w.tail[e]] - w.pi[w.head[e]]);
}
// the arc at position p of a cyclic scan that starts at `from` (from <= m_s, p < m_s)
MCF_HD inline int batch_arc_at(int from, uint32_t p, int m_s)
{
    const int64_t e = (int64_t)from + (int64_t)p;
    return (int)(e >= m_s ? e - m_s : e);
}

// NS.cs:1644-1667: the most negative reduced cost, the lowest arc among equals
MCF_HD inline bool batch_find_best(BatchWork &w, int lane, int lanes, int32_t *in_arc)
{
    const int m_s = w.search_arcs;
    int64_t mine = 0;
    uint32_t at = kNoPos;
    for (int e = lane; e < m_s; e += lanes) {
        const int64_t c = batch_reduced_cost(w, e);
        if (c < mine) { mine = c; at = (uint32_t)e; }
    }
    const int64_t best = lanes_min_i64(mine);
    if (best >= 0) return false;
    *in_arc = (int32_t)lanes_min_u32(mine == best ? at : kNoPos);
    return true;
}

// NS.cs:1607-1636: the first eligible arc from _nextArc on, round the end; _nextArc = the arc behind it
MCF_HD inline bool batch_find_first(BatchWork &w, int lane, int lanes, int32_t *in_arc)
{
    const int m_s = w.search_arcs;
    for (uint32_t base = 0; base < (uint32_t)m_s; base += (uint32_t)lanes) {
        const uint32_t p = base + (uint32_t)lane;
        const bool hit = p < (uint32_t)m_s && batch_reduced_cost(w, batch_arc_at(w.next_arc, p, m_s)) < 0;
        const uint32_t first = lanes_min_u32(hit ? p : kNoPos);
        if (first != kNoPos) {
            const int e = batch_arc_at(w.next_arc, first, m_s);
            *in_arc = e;
            w.next_arc = e + 1;
            return true;
        }
    }
    return false;
}

// NS.cs:1339-1441: one cyclic scan from _nextArc in blocks of _blockSize arcs (the count runs on across the wrap); the scan stops at the
// first block end with an eligible arc seen so far, _nextArc = the LAST arc scanned; the minimum is kept over everything scanned.
// Then the adaptive block size.
MCF_HD inline bool batch_find_block(BatchWork &w, int lane, int lanes, int32_t *in_arc)
{
    const uint32_t m_s = (uint32_t)w.search_arcs;
    const uint32_t B = (uint32_t)(w.block_size > 0 ? w.block_size : 1);
    int64_t mine = 0;
    uint32_t at = kNoPos;
    uint32_t done = 0;              // positions scanned so far
    bool stopped = false;           // at a block end (else: the scan came round)
    while (done < m_s) {
        const uint32_t end = done + B < m_s ? done + B : m_s;
        for (uint32_t p = done + (uint32_t)lane; p < end; p += (uint32_t)lanes) {
            const int64_t c = batch_reduced_cost(w, batch_arc_at(w.next_arc, p, (int)m_s));
            if (c < mine) { mine = c; at = p; }
        }
        const bool full = end - done == B;
        done = end;
        if (full && lanes_min_i64(mine) < 0) { stopped = true; break; }
    }
    const int64_t best = lanes_min_i64(mine);
    if (best >= 0) return false;
    const uint32_t pos = lanes_min_u32(mine == best ? at : kNoPos);
    *in_arc = batch_arc_at(w.next_arc, pos, (int)m_s);
    if (stopped) w.next_arc = batch_arc_at(w.next_arc, done - 1, (int)m_s);     // else the scan ended where it began: _nextArc stays
    block_adapt_step(&w.cfg, w.dyn_min, (int64_t)done, &w.block_size, w.counters);
    return true;
}

MCF_HD inline bool batch_find_entering(BatchWork &w, int lane, int lanes, int32_t *in_arc)
{
    switch (w.rule) {
    case MCF_RULE_FIRST_ELIGIBLE: return batch_find_first(w, lane, lanes, in_arc);
    case MCF_RULE_BEST_ELIGIBLE: return batch_find_best(w, lane, lanes, in_arc);
    default: return batch_find_block(w, lane, lanes, in_arc);
    }
}

// ---- the sequential half.  Returns true when the problem is found unbounded (NS.cs:321-325: no blocking arc and delta == 0).
MCF_HD inline bool batch_pivot(BatchWork &w, int in_arc)
{
    const Pivot p = find_cycle(w, in_arc, w.state[in_arc]);
    if (!p.change && p.delta == 0) return true;
    // NS.cs:1030-1039, from the flows as they are
    if (p.change) {
        const int out = w.par_arc[p.u_out];
        const int8_t out_state = leaving_state(w, p);
        w.state[in_arc] = MCF_STATE_TREE;
        w.state[out] = out_state;
    } else {
        w.state[in_arc] = (int8_t)-p.in_state;
    }
    // the plain walk (NS.cs:1185-1209): the subtree of u_out as it hangs now
    if (p.change) {
        const int64_t sigma = pivot_sigma(p, w.pi, w.cost);
        int u = p.u_out;
        for (int i = w.sub[p.u_out]; i > 0; --i) { w.pi[u] += sigma; u = w.nxt[u]; }
    }
    push_flow(w, p);
    if (p.change) rehang_subtree(w, p);
    return false;
}

// ---- the potentials of a basis under costs it was not built with (a warm re-solve): pi[root] = 0, then down the thread
// list, which is a preorder, so a node's parent has its potential first; each node's tree arc gets reduced cost 0 in batch_reduced_cost's
// convention (cost + pi[tail] - pi[head]; an arc with par_dir kUp leaves the node, so pi[u] = pi[parent] - par_dir[u] * cost).  Exactly n
// steps by count: a thread list that is not what rehang_subtree leaves cannot make this spin.  Sequential like batch_pivot: lane 0 runs it.
MCF_HD inline void batch_reprice(BatchWork &w, int lane, int lanes)
{
    (void)lanes;
    lanes_sync();
    if (lane == 0) {
        const int root = w.n;
        w.pi[root] = 0;
        int u = w.nxt[root];
        for (int i = 0; i < w.n && (unsigned)u < (unsigned)root; ++i) {        // a node, not the root: the root has no tree arc
            w.pi[u] = w.pi[w.par[u]] - w.par_dir[u] * w.cost[w.par_arc[u]];
            u = w.nxt[u];
        }
    }
    lanes_sync();
}

// ---- the dual phase of a re-solve with new supplies or bounds (uniform_redata of uniform_step.hip.h, DESIGN.md 3.14 "Re-solve with new
// data").  The basis is dual feasible (costs and potentials are the last solve's) and some tree flows lie outside their bounds.  A dual
// pivot: the tree arc with the largest violation leaves, and of the arcs across its cut that move it toward the bound it violates the one
// with the smallest reduced cost enters.  Both searches are over (lane, lanes) like the rules above; the rest is batch_pivot's sequence on
// a Pivot filled here instead of by find_cycle.

// the tree arc above a node v < n with the largest violation max(-flow, flow - upper), the lowest node among equals; false: none is violated
MCF_HD inline bool batch_find_violated(const BatchWork &w, int lane, int lanes, int32_t *u_out, int64_t *violation)
{
    int64_t mine = 0;
    uint32_t at = kNoPos;
    for (int v = lane; v < w.n; v += lanes) {
        const int e = w.par_arc[v];
        const int64_t f = w.flow[e], up = w.upper[e];
        const int64_t below = -f, above = up >= kInf ? 0 : f - up;
        const int64_t worst = below > above ? below : above;
        if (worst > mine) { mine = worst; at = (uint32_t)v; }
    }
    const int64_t best = lanes_max_i64(mine);
    if (best <= 0) return false;
    *u_out = (int32_t)lanes_min_u32(mine == best ? at : kNoPos);
    *violation = best;
    return true;
}

// The ratio test.  mark: what scratch[] holds for the nodes below the leaving arc.  An arc leaves the marked side when its tail is marked;
// raising the flow of an arc that crosses the cut the way the leaving arc does lowers the leaving arc's flow, and the other way round.
// raise: the leaving arc's flow is below 0.  The minimum of batch_reduced_cost (>= 0 by dual feasibility), the lowest arc among equals.
MCF_HD inline bool batch_find_dual_entering(const BatchWork &w, int lane, int lanes, int32_t mark, bool out_leaves, bool raise, int32_t *in_arc)
{
    const int m_s = w.search_arcs;
    int64_t mine = kMax;
    uint32_t at = kNoPos;
    for (int e = lane; e < m_s; e += lanes) {
        const int8_t st = w.state[e];
        if (st == MCF_STATE_TREE) continue;
        const bool tail_in = w.scratch[w.tail[e]] == mark, head_in = w.scratch[w.head[e]] == mark;
        if (tail_in == head_in) continue;
        const bool same_way = tail_in == out_leaves, grows = st == MCF_STATE_LOWER;
        if ((grows != same_way) != raise) continue;
        const int64_t c = batch_reduced_cost(w, e);
        if (c < mine) { mine = c; at = (uint32_t)e; }
    }
    const int64_t best = lanes_min_i64(mine);
    const uint32_t pos = lanes_min_u32(mine == best ? at : kNoPos);
    if (pos == kNoPos) return false;
    *in_arc = (int32_t)pos;
    return true;
}

// the sequential half of a dual pivot: batch_pivot's steps in its order, for the leaving arc above u_out and the entering arc in_arc
MCF_HD inline void batch_dual_pivot(BatchWork &w, int in_arc, int u_out, int64_t violation, int32_t mark)
{
    Pivot p;
    p.in_arc = in_arc;
    p.in_state = w.state[in_arc];
    const int tail = w.tail[in_arc], head = w.head[in_arc];
    const bool tail_in = w.scratch[tail] == mark;
    p.u_in = tail_in ? tail : head;
    p.v_in = tail_in ? head : tail;
    p.dir_in = tail_in ? kUp : kDown;
    p.u_out = u_out;
    p.v_out = w.par[u_out];
    p.delta = violation;
    p.change = true;
    p.out_on_tail_path = tail_in;         // u_out lies between u_in and the join node
    int a = tail, b = head;               // NS.cs:925-941
    while (a != b) {
        if (w.sub[a] < w.sub[b]) a = w.par[a]; else b = w.par[b];
    }
    p.join = a;
    const int out = w.par_arc[u_out];
    const int8_t out_state = leaving_state(w, p);
    w.state[in_arc] = MCF_STATE_TREE;
    w.state[out] = out_state;
    const int64_t sigma = pivot_sigma(p, w.pi, w.cost);
    int u = u_out;
    for (int i = w.sub[u_out]; i > 0; --i) { w.pi[u] += sigma; u = w.nxt[u]; }
    push_flow(w, p);
    rehang_subtree(w, p);
}

// At most `budget` dual pivots; returns what is left of the budget.  Ends with w.run = kBatchRunning when no tree arc is violated (the
// primal batch_run takes over), kBatchDual when the budget ran out, else how the phase ended.  Every lane runs this like batch_run.
// The nodes below the leaving arc are marked in scratch[] with -(dual pivots so far + 1): rehang_subtree leaves node ids (>= 0) there, an
// earlier pivot left a larger value, and uniform_redata clears the array, so no other node carries the mark.
MCF_HD inline int64_t batch_dual_run(BatchWork &w, int lane, int lanes, int64_t budget)
{
    while (budget > 0) {
        int32_t u_out = -1, arc = -1;
        int64_t violation = 0;
        if (!batch_find_violated(w, lane, lanes, &u_out, &violation)) { w.run = kBatchRunning; return budget; }
        const int32_t mark = (int32_t)-(w.dual_pivots + 1);
        lanes_sync();
        if (lane == 0) {
            int u = u_out;
            for (int i = w.sub[u_out]; i > 0; --i) { w.scratch[u] = mark; u = w.nxt[u]; }
        }
        lanes_sync();
        const int out = w.par_arc[u_out];
        if (!batch_find_dual_entering(w, lane, lanes, mark, w.par_dir[u_out] == kUp, w.flow[out] < 0, &arc)) { w.run = kBatchDualStuck; return budget; }
        if (lane == 0 && w.trace && w.pivots < w.trace_cap) w.trace[w.pivots] = arc;
        ++w.pivots;
        if (w.pivots > w.max_iter) { w.run = kBatchMaxIter; return budget; }
        if (w.pivots > w.pivot_limit) { --w.pivots; w.run = kBatchLimit; return budget; }
        ++w.dual_pivots;
        --budget;
        lanes_sync();
        if (lane == 0) batch_dual_pivot(w, arc, u_out, violation, mark);
        lanes_sync();
    }
    return 0;
}

// ---- at most `budget` pivots of the main loop (NS.cs:283-336).  Every lane runs this with its own copy of the scalars in w, and they stay equal.
MCF_HD inline void batch_run(BatchWork &w, int lane, int lanes, int64_t budget)
{
    w.run = kBatchRunning;
    while (budget-- > 0) {
        int32_t arc = -1;
        if (!batch_find_entering(w, lane, lanes, &arc)) { w.run = kBatchNoEntering; return; }
        if (lane == 0 && w.trace && w.pivots < w.trace_cap) w.trace[w.pivots] = arc;
        ++w.pivots;
        if (w.pivots > w.max_iter) { w.run = kBatchMaxIter; return; }                        // NS.cs:311-317
        if (w.pivots > w.pivot_limit) { --w.pivots; w.run = kBatchLimit; return; }
        int32_t unbounded = 0;
        lanes_sync();
        if (lane == 0) unbounded = batch_pivot(w, arc) ? 1 : 0;
        lanes_sync();
        if (lanes_from_first(unbounded)) { w.run = kBatchUnbounded; return; }
    }
}

// ---- a slice of a re-solve with new supplies or bounds: the dual phase where the instance is in it, then the primal pivots within the
// same budget (an instance that started again cold comes with kBatchRunning and runs as ever)
MCF_HD inline void batch_run_after_dual(BatchWork &w, int lane, int lanes, int64_t budget)
{
    if (w.run == kBatchDual) budget = batch_dual_run(w, lane, lanes, budget);
    if (w.run == kBatchRunning) batch_run(w, lane, lanes, budget);
}

}  // namespace mcf
