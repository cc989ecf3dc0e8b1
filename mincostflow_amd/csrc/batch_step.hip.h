// batch_step.hip.h -- ONE network-simplex pivot, stated once for host and device (the batch solver, batch.hip).
//
// The functions work on a BatchWork: plain pointers to the arrays mcf_ns keeps (ns_core.h) plus the pivot rule's state.  They never learn
// where the pointers point: the kernel binds them to LDS or to the instance's workspace in global memory, mcf_batch_run_on_host binds
// them to host vectors.  Two halves per pivot:
//   * the entering-arc search is written over (lane, lanes): 64 lanes of one wave share it on the device, one "lane" runs it on the host.
//     What the lanes found is combined by lanes_min_* (a wave reduction on the device, the identity on the host), so every lane leaves
//     the search with the same answer and the same rule state.  Rules: First Eligible, Best Eligible and the plain Block Search of
//     NS.cs:1292-1668 (find_first / find_best / find_block_plain of oracle/ns_oracle.c), ties broken as there: the first arc in scan
//     order among equals.
//   * join node, leaving arc, State[] writes, potentials of the subtree, flows round the cycle and the tree surgery are sequential:
//     batch_pivot restates find_join_and_leaving, decide_states, the plain walk of shift_potentials, push_flow and rehang_subtree of
//     ns_host.cpp.  Lane 0 runs it while the others wait.
// block_adapt_step is the arithmetic of mcf_block_adapt (NS.cs:1400-1438); util.cpp calls it, so there is one statement of it.
#pragma once

#include <stdint.h>

#include "../../include/mcf_hip.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MCF_HD __host__ __device__
#else
#define MCF_HD
#endif

namespace mcf {

// how a slice of pivots ended (BatchWork::run)
enum BatchRun : int32_t {
    kBatchRunning = 0,     // the slice's budget ran out: relaunch
    kBatchNoEntering = 1,  // no eligible arc: the host finishes (feasibility, lower bounds)
    kBatchUnbounded = 2,   // NS.cs:321-325
    kBatchLimit = 3,       // the instance's pivot limit
    kBatchMaxIter = 4      // the reference's own iteration guard (NS.cs:280, :311-317): Infeasible
};

struct BatchWork {
    // arcs [0, all_arcs); the rules scan [0, search_arcs)
    const int32_t *tail, *head;
    const int64_t *cost, *upper;
    int64_t *flow;
    int8_t *state;
    // nodes [0, n], n = the artificial root
    int64_t *pi;
    const int64_t *supply;             // host only: no pivot reads it, so a workspace does not carry it
    int32_t *par, *par_arc, *nxt, *prv, *sub, *fin;
    int8_t *par_dir;
    int32_t *scratch;                  // n + 2 entries
    int32_t *trace;                    // entering arc of every pivot, up to trace_cap (may be null)
    int32_t n, search_arcs, rule;
    // the rule's state
    int32_t next_arc, block_size, dyn_min;
    int32_t counters[2];               // _consecutiveLowHits, _consecutiveHighHits
    mcf_block_config cfg;
    int64_t pivots, pivot_limit, max_iter, trace_cap;
    int32_t run;                       // BatchRun
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
    constexpr int8_t kUp = 1, kDown = -1;
    constexpr int64_t kMax = INT64_MAX, kInf = INT64_MAX / 2;
    int32_t *const par = w.par, *const parc = w.par_arc, *const nxt = w.nxt, *const prv = w.prv, *const sub = w.sub, *const fin = w.fin;
    int8_t *const pdir = w.par_dir;
    int64_t *const flow = w.flow;
    const int64_t *const upper = w.upper;

    // -- find_join_and_leaving (NS.cs:925-1010 in one climb; the tie rules are explained in ns_host.cpp)
    const int8_t in_state = w.state[in_arc];
    const bool lower = in_state == MCF_STATE_LOWER;
    const int tail = w.tail[in_arc], head = w.head[in_arc];
    int a = tail, b = head;
    int64_t d_first = kMax, d_second = kMax;
    int u_first = -1, u_second = -1;
    const int8_t gain_a = lower ? kDown : kUp, gain_b = lower ? kUp : kDown;
    while (a != b) {
        if (sub[a] < sub[b]) {
            const int e = parc[a];
            int64_t room = flow[e];
            if (pdir[a] == gain_a) room = upper[e] >= kMax ? kInf : upper[e] - room;
            if (lower) { if (room < d_first) { d_first = room; u_first = a; } }
            else { if (room <= d_second) { d_second = room; u_second = a; } }
            a = par[a];
        } else {
            const int e = parc[b];
            int64_t room = flow[e];
            if (pdir[b] == gain_b) room = upper[e] >= kMax ? kInf : upper[e] - room;
            if (lower) { if (room <= d_second) { d_second = room; u_second = b; } }
            else { if (room < d_first) { d_first = room; u_first = b; } }
            b = par[b];
        }
    }
    const int join = a;
    const int first = lower ? tail : head, second = lower ? head : tail;
    int64_t delta = upper[in_arc];
    int side = 0, u_out = -1;
    if (u_first >= 0 && d_first < delta) { delta = d_first; u_out = u_first; side = 1; }
    if (u_second >= 0 && d_second <= delta) { delta = d_second; u_out = u_second; side = 2; }
    const int u_in = side == 1 ? first : second, v_in = side == 1 ? second : first;
    const bool out_on_tail_path = side != 0 && ((side == 1) == (first == tail));
    const bool change = side != 0;
    if (!change && delta == 0) return true;

    // -- decide_states (NS.cs:1030-1039), from the flows as they are
    if (change) {
        const int out = parc[u_out];
        const int64_t val = in_state * delta;
        const int64_t after = out_on_tail_path ? flow[out] - pdir[u_out] * val : flow[out] + pdir[u_out] * val;
        w.state[in_arc] = MCF_STATE_TREE;
        w.state[out] = after == 0 ? MCF_STATE_LOWER : MCF_STATE_UPPER;
    } else {
        w.state[in_arc] = (int8_t)-in_state;
    }
    const int8_t dir_in = u_in == tail ? kUp : kDown;

    // -- shift_potentials, the plain walk (NS.cs:1185-1209): the subtree of u_out as it hangs now
    if (change) {
        const int64_t sigma = w.pi[v_in] - w.pi[u_in] - dir_in * w.cost[in_arc];
        int u = u_out;
        for (int i = sub[u_out]; i > 0; --i) { w.pi[u] += sigma; u = nxt[u]; }
    }

    // -- push_flow (NS.cs:1012-1029)
    if (delta > 0) {
        const int64_t val = in_state * delta;
        flow[in_arc] += val;
        for (int u = tail; u != join; u = par[u]) flow[parc[u]] -= pdir[u] * val;
        for (int u = head; u != join; u = par[u]) flow[parc[u]] += pdir[u] * val;
    }
    if (!change) return false;

    // -- rehang_subtree (NS.cs:1042-1183)
    const int before_out = prv[u_out], size_out = sub[u_out], fin_out_old = fin[u_out];
    const int v_out = par[u_out];
    if (u_in == u_out) {
        par[u_in] = v_in; parc[u_in] = in_arc; pdir[u_in] = dir_in;
        if (nxt[v_in] != u_out) {
            int after = nxt[fin_out_old];
            nxt[before_out] = after; prv[after] = before_out;
            after = nxt[v_in];
            nxt[v_in] = u_out; prv[u_out] = v_in;
            nxt[fin_out_old] = after; prv[after] = fin_out_old;
        }
    } else {
        const int resume = before_out == v_in ? nxt[fin_out_old] : nxt[v_in];
        int stem = u_in, new_par = v_in, last = fin[u_in], after = nxt[last];
        nxt[v_in] = u_in;
        int n_dirty = 0;
        w.scratch[n_dirty++] = v_in;
        while (stem != u_out) {
            const int up = par[stem];
            nxt[last] = up;
            w.scratch[n_dirty++] = last;
            const int before = prv[stem];
            nxt[before] = after; prv[after] = before;
            par[stem] = new_par;
            new_par = stem;
            stem = up;
            last = fin[stem] == fin[new_par] ? prv[new_par] : fin[stem];
            after = nxt[last];
        }
        par[u_out] = new_par;
        nxt[last] = resume; prv[resume] = last;
        fin[u_out] = last;
        if (before_out != v_in) { nxt[before_out] = after; prv[after] = before_out; }
        for (int i = 0; i < n_dirty; ++i) { const int u = w.scratch[i]; prv[nxt[u]] = u; }
        int acc = 0;
        const int fin_new = fin[u_out];
        for (int u = u_out, p = par[u]; u != u_in; u = p, p = par[u]) {
            parc[u] = parc[p];
            pdir[u] = (int8_t)-pdir[p];
            acc += sub[u] - sub[p];
            sub[u] = acc;
            fin[p] = fin_new;
        }
        parc[u_in] = in_arc; pdir[u_in] = dir_in; sub[u_in] = size_out;
    }
    const int stop_out = fin[join] == v_in ? join : -1;
    const int fin_moved = fin[u_out];
    for (int u = v_in; u != -1 && fin[u] == v_in; u = par[u]) fin[u] = fin_moved;
    if (join != before_out && v_in != before_out) {
        for (int u = v_out; u != stop_out && fin[u] == fin_out_old; u = par[u]) fin[u] = before_out;
    } else if (fin_moved != fin_out_old) {
        for (int u = v_out; u != stop_out && fin[u] == fin_out_old; u = par[u]) fin[u] = fin_moved;
    }
    for (int u = v_in; u != join; u = par[u]) sub[u] += size_out;
    for (int u = v_out; u != join; u = par[u]) sub[u] -= size_out;
    return false;
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

}  // namespace mcf
