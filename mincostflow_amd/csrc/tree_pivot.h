// tree_pivot.h -- the sequential steps of ONE network-simplex pivot on the thread-index spanning tree, stated once for the host driver
// (ns_host.cpp) and the batch solver (batch_step.hip.h, on the device and on the host).
//
// The functions work on a TreeView: plain pointers to the arrays a pivot touches.  They never learn where the pointers point (host vectors of
// an NsCore, LDS, a workspace in device memory) nor which caller they serve.  What is NOT here: State[] writes (mcf_ns records them for its
// engines, the batch does not), the walk that moves the subtree's potentials (ns_host.cpp's shift_potentials and batch_pivot's plain walk are
// different code for different machines), and the order of the steps (mcf_ns runs the flows and the tree while the device searches).
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

constexpr int8_t kUp = 1, kDown = -1;   // SpanningTree.cs:67-71 DIR_UP / DIR_DOWN
constexpr int64_t kMax = INT64_MAX;     // NS.cs:126
constexpr int64_t kInf = INT64_MAX / 2; // NS.cs:127

// a view, not an owner: NsCore::tree() fills it from the host vectors, bind() of batch.hip from a workspace
struct TreeView {
    // arcs
    const int32_t *tail, *head;
    const int64_t *upper;
    int64_t *flow;
    // nodes [0, n], n = the artificial root: Parent, Pred, Thread, RevThread, SuccNum, LastSucc, PredDir
    int32_t *par, *par_arc, *nxt, *prv, *sub, *fin;
    int8_t *par_dir;
    int32_t *scratch;                  // n + 2 entries: the re-hanging's list of nodes whose RevThread is repaired last
};

// the pivot being carried out: what find_cycle found, read by every later step
struct Pivot {
    int32_t in_arc = -1, join = -1, u_in = -1, v_in = -1, u_out = -1, v_out = -1;
    int64_t delta = 0;
    int8_t in_state = 0;              // State[in_arc] when the pivot started
    int8_t dir_in = 0;                // u_in's new parent direction: kUp when u_in is the entering arc's tail (v_in is its head), else kDown
    bool out_on_tail_path = false;    // the leaving arc lies on the cycle half that starts at the entering arc's tail
    bool change = false;              // the pivot changes the basis (a blocking arc was found); !change && delta == 0: unbounded (NS.cs:321-325)
};

// find_join + find_leaving in ONE climb.  The reference climbs twice: first to the join node (NS.cs:925-941: whichever side has the smaller
// SuccNum steps up), then from both end points of the entering arc to the join again, taking the minimum residual of each path (NS.cs:943-1010).
// Both climbs visit the same nodes in the same bottom-up order per side, and the second one only needs to know where each side stops -- which
// the first one discovers as it goes.  So the residuals are folded into the first climb: a step on the FIRST path (the side the entering arc's
// state makes "first") compares with '<', a step on the second with '<=', exactly as NS.cs:957-997 -- with one difference in ORDER: the
// reference finishes the first path before it starts the second, here the two interleave.  That matters for ties between the paths: the
// reference lets a second-path arc with residual EQUAL to the first path's minimum win (d <= delta), whenever it comes.  Interleaved, each
// side keeps its own minimum and the two are combined at the end with the same rule (second path wins ties), which is the same arc:
//   first-path winner  = the lowest node u on it with residual < everything below it      (strict: the first among equals, bottom-up)
//   second-path winner = the highest node u on it with residual <= everything below it and <= the first path's minimum (the last among equals)
// and the second path's own '<=' chain must be evaluated against min(first-path minimum, running): since min is associative the result
// is: delta = min(d1, d2); leaving = second-path's LAST node with d == d2 if d2 <= d1, else first-path's FIRST node with d == d1.
MCF_HD inline Pivot find_cycle(const TreeView &t, int in_arc, int8_t in_state)
{
    const int32_t *const par = t.par, *const sub = t.sub, *const parc = t.par_arc;
    const int8_t *const pdir = t.par_dir;
    const int64_t *const flow = t.flow, *const upper = t.upper;
    const bool lower = in_state == MCF_STATE_LOWER;
    const int tail = t.tail[in_arc], head = t.head[in_arc];
    // side A climbs from the tail, side B from the head; the FIRST path starts at the tail when the arc is at its lower bound
    int a = tail, b = head;
    // residual of the tree arc above u when flow is pushed along the cycle: on the first path arcs pointing DOWN gain flow, on the second arcs pointing UP
    int64_t d_first = kMax, d_second = kMax;
    int u_first = -1, u_second = -1;
    const int8_t gain_a = lower ? kDown : kUp;            // the direction whose arcs GAIN flow (residual = upper - flow) on side A ...
    const int8_t gain_b = lower ? kUp : kDown;            // ... and on side B
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
    Pivot p;
    p.in_arc = in_arc;
    p.in_state = in_state;
    p.join = a;
    const int first = lower ? tail : head, second = lower ? head : tail;
    // NS.cs:952: delta starts at the entering arc's capacity; the first path replaces it only with something strictly smaller, the second
    // with anything not larger
    int64_t delta = upper[in_arc];
    int side = 0;
    if (u_first >= 0 && d_first < delta) { delta = d_first; p.u_out = u_first; side = 1; }
    if (u_second >= 0 && d_second <= delta) { delta = d_second; p.u_out = u_second; side = 2; }
    p.delta = delta;
    p.u_in = side == 1 ? first : second;
    p.v_in = side == 1 ? second : first;
    p.dir_in = p.u_in == tail ? kUp : kDown;
    p.change = side != 0;
    p.out_on_tail_path = side != 0 && ((side == 1) == (first == tail));
    if (p.change) p.v_out = par[p.u_out];
    return p;
}

// ---- NS.cs:1030-1039, before the flows are touched: State[] of the leaving arc.  It depends on the arc's flow after ChangeFlow
// (0 -> LOWER, else UPPER), which is its flow now -/+ delta along its half of the cycle (same sums as push_flow).  Only for p.change; the
// entering arc becomes TREE then, and -in_state otherwise.
MCF_HD inline int8_t leaving_state(const TreeView &t, const Pivot &p)
{
    const int out = t.par_arc[p.u_out];
    const int64_t val = p.in_state * p.delta;
    const int64_t after = p.out_on_tail_path ? t.flow[out] - t.par_dir[p.u_out] * val : t.flow[out] + t.par_dir[p.u_out] * val;
    return after == 0 ? MCF_STATE_LOWER : MCF_STATE_UPPER;
}

// ---- NS.cs:1187-1188 (PredDir[u_in] there is u_in's NEW parent direction): what the potentials of the subtree that moves change by
MCF_HD inline int64_t pivot_sigma(const Pivot &p, const int64_t *pi, const int64_t *cost)
{
    return pi[p.v_in] - pi[p.u_in] - p.dir_in * cost[p.in_arc];
}

// ---- NS.cs:1012-1029: the flow change around the cycle (old tree; nothing a search needs)
MCF_HD inline void push_flow(const TreeView &t, const Pivot &p)
{
    if (p.delta <= 0) return;
    const int32_t *const par = t.par, *const parc = t.par_arc;
    const int8_t *const pdir = t.par_dir;
    int64_t *const flow = t.flow;
    const int64_t val = p.in_state * p.delta;
    const int tail = p.dir_in == kUp ? p.u_in : p.v_in, head = p.dir_in == kUp ? p.v_in : p.u_in;     // the entering arc's end points
    flow[p.in_arc] += val;
    for (int u = tail; u != p.join; u = par[u]) flow[parc[u]] -= pdir[u] * val;
    for (int u = head; u != p.join; u = par[u]) flow[parc[u]] += pdir[u] * val;
}

// what rehang_subtree tells about its Thread writes when nobody listens
struct NoThreadNote { MCF_HD void operator()(int) const {} };

// ---- NS.cs:1042-1183.  The subtree of u_out is cut off v_out, re-rooted at u_in and hung below v_in; the preorder
// (thread) list is spliced accordingly and SuccNum / LastSucc are repaired along the two root paths.  Only for p.change.
// note(a) is called after every write of nxt[a] (the host driver keeps its bitmap of thread breaks current with it, thread_breaks.h;
// the batch solver passes nothing and gets the code it had).
template <class Note = NoThreadNote>
MCF_HD inline void rehang_subtree(const TreeView &t, const Pivot &p, const Note &note = Note())
{
    int32_t *const par = t.par, *const parc = t.par_arc, *const nxt = t.nxt, *const prv = t.prv, *const sub = t.sub, *const fin = t.fin;
    int32_t *const dirty = t.scratch;
    int8_t *const pdir = t.par_dir;
    const int u_in = p.u_in, v_in = p.v_in, u_out = p.u_out, v_out = p.v_out, in_arc = p.in_arc, join = p.join;
    const int before_out = prv[u_out], size_out = sub[u_out], fin_out_old = fin[u_out];
    const int8_t dir_in = p.dir_in;

    if (u_in == u_out) {
        // the whole subtree moves as it is
        par[u_in] = v_in; parc[u_in] = in_arc; pdir[u_in] = dir_in;
        if (nxt[v_in] != u_out) {
            int after = nxt[fin_out_old];
            nxt[before_out] = after; note(before_out); prv[after] = before_out;          // unlink [u_out .. fin_out_old]
            after = nxt[v_in];
            nxt[v_in] = u_out; note(v_in); prv[u_out] = v_in;                       // relink right behind v_in
            nxt[fin_out_old] = after; note(fin_out_old); prv[after] = fin_out_old;
        }
    } else {
        // before_out == v_in also means join == v_out
        const int resume = before_out == v_in ? nxt[fin_out_old] : nxt[v_in];
        int stem = u_in, new_par = v_in, last = fin[u_in], after = nxt[last];
        nxt[v_in] = u_in; note(v_in);
        int n_dirty = 0;
        dirty[n_dirty++] = v_in;
        while (stem != u_out) {
            const int up = par[stem];
            nxt[last] = up; note(last);           // the next stem node follows this stem's subtree
            dirty[n_dirty++] = last;
            const int before = prv[stem];         // drop the stem's subtree from its old place
            nxt[before] = after; note(before); prv[after] = before;
            par[stem] = new_par;
            new_par = stem;
            stem = up;
            last = fin[stem] == fin[new_par] ? prv[new_par] : fin[stem];
            after = nxt[last];
        }
        par[u_out] = new_par;
        nxt[last] = resume; note(last); prv[resume] = last;
        fin[u_out] = last;
        if (before_out != v_in) { nxt[before_out] = after; note(before_out); prv[after] = before_out; }
        for (int i = 0; i < n_dirty; ++i) { const int u = dirty[i]; prv[nxt[u]] = u; }
        // reverse the parent arcs along the stem, rebuild sizes
        int acc = 0;
        const int fin_new = fin[u_out];
        for (int u = u_out, q = par[u]; u != u_in; u = q, q = par[u]) {
            parc[u] = parc[q];
            pdir[u] = (int8_t)-pdir[q];
            acc += sub[u] - sub[q];
            sub[u] = acc;
            fin[q] = fin_new;
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
}

}  // namespace mcf
