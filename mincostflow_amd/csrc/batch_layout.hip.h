// batch_layout.hip.h -- where an instance of the batch solver keeps its state: the workspace layout and the per-instance slot.
//
// Shared by batch.hip (the kernels and both ABIs) and uniform_step.hip.h (the device set-up and the device end of a solve), so that
// there is one statement of where every array lies.
#pragma once

#include <stdint.h>

#include "batch_step.hip.h"

namespace mcf {

// ---- workspace of one instance: A = all_arcs arcs, N = n + 1 nodes; every array starts on a 16-byte boundary.
//   constant part:  tail[A] i32 | head[A] i32 | cost[A] i64 | upper[A] i64
//   changing part:  flow[A] i64 | pi[N] i64 | par, par_arc, nxt, prv, sub, fin [N] i32 each | scratch[N + 1] i32 | state[A] i8 | par_dir[N] i8
// bytes = 33 A + 37 N + 4 + padding (at most 15 per array)
struct Layout {
    uint32_t tail, head, cost, upper, flow, pi, par, par_arc, nxt, prv, sub, fin, scratch, state, par_dir;
    uint32_t changing;      // = flow: first byte of the part a launch writes back
    uint32_t bytes;
};
MCF_HD inline uint32_t up16(uint32_t x) { return (x + 15u) & ~15u; }
MCF_HD inline Layout layout_of(uint32_t A, uint32_t N)
{
    Layout l;
    uint32_t o = 0;
    l.tail = o; o = up16(o + 4 * A);
    l.head = o; o = up16(o + 4 * A);
    l.cost = o; o = up16(o + 8 * A);
    l.upper = o; o = up16(o + 8 * A);
    l.flow = l.changing = o; o = up16(o + 8 * A);
    l.pi = o; o = up16(o + 8 * N);
    l.par = o; o = up16(o + 4 * N);
    l.par_arc = o; o = up16(o + 4 * N);
    l.nxt = o; o = up16(o + 4 * N);
    l.prv = o; o = up16(o + 4 * N);
    l.sub = o; o = up16(o + 4 * N);
    l.fin = o; o = up16(o + 4 * N);
    l.scratch = o; o = up16(o + 4 * (N + 1));
    l.state = o; o = up16(o + A);
    l.par_dir = o; o = up16(o + N);
    l.bytes = o;
    return l;
}
MCF_HD inline void bind(BatchWork &w, unsigned char *base, const Layout &l)
{
    w.tail = (const int32_t *)(base + l.tail); w.head = (const int32_t *)(base + l.head);
    w.cost = (const int64_t *)(base + l.cost); w.upper = (const int64_t *)(base + l.upper);
    w.flow = (int64_t *)(base + l.flow); w.pi = (int64_t *)(base + l.pi);
    w.par = (int32_t *)(base + l.par); w.par_arc = (int32_t *)(base + l.par_arc); w.nxt = (int32_t *)(base + l.nxt);
    w.prv = (int32_t *)(base + l.prv); w.sub = (int32_t *)(base + l.sub); w.fin = (int32_t *)(base + l.fin);
    w.scratch = (int32_t *)(base + l.scratch); w.state = (int8_t *)(base + l.state); w.par_dir = (int8_t *)(base + l.par_dir);
}

// what a launch needs to know of an instance and what it leaves behind; one per instance, in device memory
struct BatchSlot {
    uint64_t workspace;         // byte offset of the workspace in the slab
    uint64_t trace;             // index of the first trace entry in the trace buffer
    int64_t pivots, pivot_limit, max_iter;
    int32_t n, all_arcs, search_arcs, rule;
    int32_t next_arc, block_size, dyn_min, counters[2];
    int32_t trace_cap;
    int32_t run;                // mcf::BatchRun
    int32_t reprice;            // a warm re-solve: the potentials are recomputed from the basis before the first pivot; the launch that did it clears this
    uint64_t staged_cost;       // a re-solve's staging buffer: where this instance's new cost[] waits (stage_kernel<true>) ...
    uint64_t staged_out;        // ... and where its changing part goes for the download (stage_kernel<false>)
    mcf_block_config cfg;
};

static_assert(sizeof(BatchSlot) == 104 + sizeof(mcf_block_config), "BatchSlot has no padding: a re-solve counts the bytes it uploads by it");

MCF_HD inline void load_slot(BatchWork &w, const BatchSlot &s, int32_t *trace_base)
{
    w.n = s.n; w.search_arcs = s.search_arcs; w.rule = s.rule;
    w.next_arc = s.next_arc; w.block_size = s.block_size; w.dyn_min = s.dyn_min;
    w.counters[0] = s.counters[0]; w.counters[1] = s.counters[1];
    w.cfg = s.cfg;
    w.pivots = s.pivots; w.pivot_limit = s.pivot_limit; w.max_iter = s.max_iter;
    w.trace_cap = s.trace_cap;
    w.trace = s.trace_cap > 0 ? trace_base + s.trace : nullptr;
    w.run = s.run;
}
MCF_HD inline void store_slot(BatchSlot &s, const BatchWork &w)
{
    s.next_arc = w.next_arc; s.block_size = w.block_size;
    s.counters[0] = w.counters[0]; s.counters[1] = w.counters[1];
    s.pivots = w.pivots;
    s.run = w.run;
    s.reprice = 0;
}

}  // namespace mcf
