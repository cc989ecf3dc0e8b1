// batch.hip -- mcf_batch_*: many small independent instances, one whole solve per workgroup.
//
// The pivot itself is batch_step.hip.h, shared with the host.  This file is what surrounds it:
//   * per instance an NsCore (ns_core.h): set up by the host with the code mcf_ns uses, finished by it afterwards;
//   * a WORKSPACE per instance in one slab of device memory, the home of its state between launches (layout: Layout below);
//   * batch_kernel: one workgroup of ONE wave per instance.  LDS tier: the workspace is copied into dynamic LDS at entry, the pivots run
//     there, the part that changes is copied back at exit.  Global tier: the pivots run in place on the workspace.  Same step functions;
//   * bounded launches: a launch runs every unfinished instance for at most pivots_per_launch pivots and returns; the host relaunches
//     until every instance is done.  The rule's state and the pivot count travel in the instance's BatchSlot.
//   * re-solves: the slab, the slots and the trace buffer live as long as the batch.  mcf_batch_set_costs + mcf_batch_resolve run the changed
//     instances again: from the basis they ended with where that ended Optimal (new cost[] up, batch_reprice on the device, changing part
//     down), from the start basis otherwise.
//   * re-solves with new supplies and bounds (mcf_ubatch_resolve_data, mcf_rbatch_resolve_data): batch_dual_kernel runs the dual pivots of
//     batch_step.hip.h in front of the primal ones, between a re-data launch and a settle launch (step_kernel on uniform_redata and
//     uniform_redata_settle, uniform_step.hip.h).
//   * the placed batches (mcf_ubatch_*, mcf_rbatch_*): problem data in and results out where they are.  Their kernels are stated once
//     over the kind of problem -- step_kernel<Problem, Step>, finish_kernel<Problem>, validate_kernel<Problem>, query_kernel<Problem,
//     Query, kLds> -- as their host side is stated once over a placement; view_of (uniform_step.hip.h) is what tells a UniformProblem
//     from a RaggedProblem.
//   * cost ranges of the kept basis (mcf_ubatch_cost_ranges, mcf_rbatch_cost_ranges): query_kernel<.., CostRanges, ..> runs
//     ranges_step.hip.h on the workspaces as the last solve call left them, and writes nothing there.
//   * supply and bound ranges of the kept basis (mcf_ubatch_data_ranges, mcf_rbatch_data_ranges): query_kernel<.., DataRanges, ..> runs
//     data_ranges_step.hip.h on the same state, the same way; every walk gathers into registers, so it needs no atomics.
//   * why an instance is infeasible (mcf_ubatch_diagnose, mcf_rbatch_diagnose): query_kernel<.., Diagnose, ..> runs diagnose_step.hip.h on
//     the same state, the same way; marks and frontiers lie in LDS or, for the global tier, in a buffer of the handle's.
//   * unbounded or not (mcf_ubatch_rays, mcf_rbatch_rays): query_kernel<.., Rays, ..> runs rays_step.hip.h on the costs and capacities of
//     the same state, the same way; labels, marks and frontiers lie in LDS or, for the global tier, in the same buffer of the handle's.
//   * solves that start from a basis the caller supplies (mcf_ubatch_solve_from, mcf_rbatch_solve_from): step_kernel<.., uniform_begin_from>
//     is the set-up launch; rounds and settle launch are those of a re-solve with new data.
// Device code does no bounds checks: mcf_batch_add validates every end point (core_create), and every index the kernel follows after
// that was written by start_basis or by the pivot itself.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cstring>
#include <vector>

#include "batch_layout.hip.h"
#include "batch_step.hip.h"
#include "common.h"
#include "data_ranges_step.hip.h"
#include "diagnose_step.hip.h"
#include "ns_core.h"
#include "ranges_step.hip.h"
#include "rays_step.hip.h"
#include "uniform_step.hip.h"

namespace {

#define HIP_TRY(expr)                                                                                      \
    do {                                                                                                   \
        hipError_t err__ = (expr);                                                                         \
        if (err__ != hipSuccess) return mcf::fail(MCF_ERR_HIP, "%s: %s", #expr, hipGetErrorString(err__)); \
    } while (0)

constexpr int kBatchThreads = 64;          // one wave: the sequential and the lane-parallel half alternate without a workgroup of waves to hold
constexpr int kDefaultPivotsPerLaunch = 2048;   // 15 us per pivot in LDS, 35 in place -> launches of 30 - 70 ms

// the workspace layout and the per-instance slot: batch_layout.hip.h
using mcf::BatchSlot;
using mcf::Layout;
using mcf::bind;
using mcf::layout_of;
using mcf::load_slot;
using mcf::store_slot;

// One workgroup = one wave = one instance: ids[blockIdx.x].  kLds: dynamic LDS holds the workspace (the host launches with at least
// layout.bytes of it); otherwise the pivots run on the workspace itself.
template <bool kLds>
__global__ __launch_bounds__(kBatchThreads) void batch_kernel(BatchSlot *slots, const int32_t *ids, unsigned char *slab, int32_t *traces, int32_t budget)
{
    extern __shared__ __align__(16) unsigned char lds[];
    const int lane = (int)threadIdx.x;
    BatchSlot &slot = slots[ids[blockIdx.x]];
    const bool reprice = slot.reprice != 0;
    const Layout l = layout_of((uint32_t)slot.all_arcs, (uint32_t)slot.n + 1u);
    unsigned char *const home = slab + slot.workspace;
    mcf::BatchWork w;
    load_slot(w, slot, traces);
    if (kLds) {
        const uint4 *src = (const uint4 *)home;
        uint4 *dst = (uint4 *)lds;
        for (uint32_t i = (uint32_t)lane; i < l.bytes / 16; i += kBatchThreads) dst[i] = src[i];
        bind(w, lds, l);
    } else {
        bind(w, home, l);
    }
    __syncthreads();
    if (reprice) mcf::batch_reprice(w, lane, kBatchThreads);        // on LDS in the LDS tier: the new cost[] came in with the copy above
    mcf::batch_run(w, lane, kBatchThreads, (int64_t)budget);
    __syncthreads();
    if (kLds) {
        const uint4 *src = (const uint4 *)lds;
        uint4 *dst = (uint4 *)home;
        for (uint32_t i = l.changing / 16 + (uint32_t)lane; i < l.bytes / 16; i += kBatchThreads) dst[i] = src[i];
    }
    if (lane == 0) store_slot(slot, w);
}

// batch_kernel for a re-solve with new supplies or bounds (mcf_*batch_resolve_data): the dual phase of an instance that is in it goes
// first, the primal pivots follow within the same budget.  A kernel of its own, so that batch_kernel keeps its code and its registers
// for the solves that never enter a dual phase.  The dual pivot count travels in slot.staged_out, which only mcf_batch_resolve uses
// otherwise, and reprice == 2 (a warm attempt, for uniform_redata_settle) outlives the launch.
template <bool kLds>
__global__ __launch_bounds__(kBatchThreads) void batch_dual_kernel(BatchSlot *slots, const int32_t *ids, unsigned char *slab, int32_t *traces, int32_t budget)
{
    extern __shared__ __align__(16) unsigned char lds[];
    const int lane = (int)threadIdx.x;
    BatchSlot &slot = slots[ids[blockIdx.x]];
    const int32_t attempt = slot.reprice;
    const Layout l = layout_of((uint32_t)slot.all_arcs, (uint32_t)slot.n + 1u);
    unsigned char *const home = slab + slot.workspace;
    mcf::BatchWork w;
    load_slot(w, slot, traces);
    w.dual_pivots = (int64_t)slot.staged_out;
    if (kLds) {
        const uint4 *src = (const uint4 *)home;
        uint4 *dst = (uint4 *)lds;
        for (uint32_t i = (uint32_t)lane; i < l.bytes / 16; i += kBatchThreads) dst[i] = src[i];
        bind(w, lds, l);
    } else {
        bind(w, home, l);
    }
    __syncthreads();
    mcf::batch_run_after_dual(w, lane, kBatchThreads, (int64_t)budget);
    __syncthreads();
    if (kLds) {
        const uint4 *src = (const uint4 *)lds;
        uint4 *dst = (uint4 *)home;
        for (uint32_t i = l.changing / 16 + (uint32_t)lane; i < l.bytes / 16; i += kBatchThreads) dst[i] = src[i];
    }
    if (lane == 0) {
        store_slot(slot, w);
        slot.staged_out = (uint64_t)w.dual_pivots;
        slot.reprice = attempt == 2 ? 2 : 0;
    }
}

// A re-solve moves only what changed.  Block k serves instance ids[k].  kIn: its new cost[0, all_arcs) (rounded up to 16 bytes, as the
// layout is) from the staging buffer into its workspace; else: the changing part of its workspace into the staging buffer, from where
// one copy takes every instance's home.  Both offsets are in the slot; the host sizes the staging buffer for the larger of the two sums.
constexpr int kStageThreads = 256;
template <bool kIn>
__global__ __launch_bounds__(kStageThreads) void stage_kernel(const BatchSlot *slots, const int32_t *ids, unsigned char *slab, unsigned char *stage)
{
    const BatchSlot &slot = slots[ids[blockIdx.x]];
    const Layout l = layout_of((uint32_t)slot.all_arcs, (uint32_t)slot.n + 1u);
    unsigned char *const home = slab + slot.workspace;
    const uint4 *const src = (const uint4 *)(kIn ? stage + slot.staged_cost : home + l.changing);
    uint4 *const dst = (uint4 *)(kIn ? home + l.cost : stage + slot.staged_out);
    const uint32_t count = (kIn ? l.upper - l.cost : l.bytes - l.changing) / 16;
    for (uint32_t i = threadIdx.x; i < count; i += kStageThreads) dst[i] = src[i];
}

// The placed batches (mcf_ubatch_*, mcf_rbatch_*): the steps of uniform_step.hip.h and of the query headers, each kernel stated once over
// the kind of problem.  view_of forms the placed view of an instance from either kind: a UniformProblem places by strides (the caller's
// arrays as base + i * stride, the workspace at i * stride), a RaggedProblem by the handle's tables in device memory (the instance's graph
// record, its rows and its workspace at running sums, its graph's slot template); every table entry a block reads is the same for all its
// lanes.  One workgroup of one wave per instance, like batch_kernel: the start basis numbers the artificial arcs by a wave-wide prefix
// count, and every step combines its lanes by wave reductions.  Consecutive lanes work on consecutive arcs or nodes.
//
// step_kernel: the set-up launch of a solve (uniform_begin, _recost, _redata, _begin_from) and the settle launch (uniform_redata_settle).
// Block i serves instance i, on its workspace in device memory, with its graph's slot template, and leaves at once where `changed` (a
// re-solve's mask) says so.  A fresh solve and a solve from a given basis have no mask: solve_on_device clears it for a call that is no
// re-solve, check_call refuses one beside a basis, so for uniform_begin and uniform_begin_from the test never holds.
using Step = void (*)(const mcf::InstanceView &, const BatchSlot &, BatchSlot &, int, int);
template <class Problem, Step kStep>
__global__ __launch_bounds__(kBatchThreads) void step_kernel(Problem p, const BatchSlot *tmpl, BatchSlot *slots, unsigned char *slab)
{
    const int64_t i = (int64_t)blockIdx.x;
    if (p.changed && !p.changed[i]) return;
    int32_t t;
    const mcf::InstanceView v = mcf::view_of(p, nullptr, i, slab, &t);
    kStep(v, tmpl[t], slots[i], (int)threadIdx.x, kBatchThreads);
}
// the finish launch: the status and the output rows of every instance the call ran
template <class Problem>
__global__ __launch_bounds__(kBatchThreads) void finish_kernel(Problem p, mcf::UniformOutputs o, const BatchSlot *slots, unsigned char *slab, const int32_t *traces)
{
    const int64_t i = (int64_t)blockIdx.x;
    if (p.changed && !p.changed[i]) return;
    mcf::uniform_finish(mcf::view_of(p, &o, i, slab, nullptr), o, slots[i], traces, (int)threadIdx.x, kBatchThreads);
}
// mcf_*batch_validate: block i checks instance i's rows.  One wave for the same reason: every combine is a wave reduction.  It touches
// neither slab nor slots; the only words instances share are the two of the summary, and only invalid instances write them.
template <class Problem>
__global__ __launch_bounds__(kBatchThreads) void validate_kernel(Problem p, mcf::UniformCheck c, const int64_t *flows, const int64_t *potentials)
{
    mcf::uniform_validate(mcf::check_view_of(p, flows, potentials, (int64_t)blockIdx.x), c, (int)threadIdx.x, kBatchThreads);
}

// The queries of the kept state (mcf_*batch_cost_ranges, _data_ranges, _diagnose, _rays): Query is one of the descriptions below (CostRanges,
// DataRanges, Diagnose, Rays), whose step<kLds> runs its header's step.  Block k serves instance ids[k] (the handle's table of the
// instances by tier and footprint class, up once per handle and query).  One wave, like every kernel here: what the lanes of one
// instance share meets in its own rows, its own LDS or its own part of the work buffer, and the barriers between the passes are the
// workgroup's.  kLds: dynamic LDS holds what the step reads and its working arrays (the host launches with at least Query::footprint(n, m)
// bytes of it):
//   cost ranges   what the walks read and the two accumulators; otherwise the walks run on the workspace, the minima in the caller's rows;
//   data ranges   what a hop reads and the room arrays, written before the one barrier and read after it; otherwise the walks follow the
//                 workspace in place.  The walks gather into registers and the answers go straight to the caller's rows;
//   diagnosis     flow and upper of the caller's arcs, unmet, marks and frontiers;
//   rays          cost and upper of the caller's arcs, the two label arrays, preds, frontiers and marks.
// Otherwise diagnosis and rays read the workspace, and block k keeps its working arrays in work + k * work_stride, which the host sized
// for the largest instance of the global tier (prepare_work); the two range queries keep none and get a stride of 0.  pairs: the data
// ranges' pair lists, one for all or one per graph (pairs_of); empty for the other queries.
template <class Problem, class Query, bool kLds>
__global__ __launch_bounds__(kBatchThreads) void query_kernel(Problem p, typename Query::Outputs o, mcf::PairArgs pairs, const BatchSlot *slots, unsigned char *slab,
                                                              const int32_t *ids, unsigned char *work, uint64_t work_stride)
{
    extern __shared__ __align__(16) unsigned char lds[];
    const int64_t i = (int64_t)ids[blockIdx.x];
    Query::template step<kLds>(mcf::view_of(p, nullptr, i, slab, nullptr), o, mcf::pairs_of(p, pairs, i), slots[i], kLds ? lds : work + (uint64_t)blockIdx.x * work_stride,
                               (int)threadIdx.x, kBatchThreads);
}

struct Instance {
    mcf::NsCore core;
    Layout layout{};
    BatchSlot slot{};
    std::vector<int32_t> trace;
    int64_t trace_len = 0;
    bool on_device = false;     // false: infeasible by its bounds, nothing to run
    bool on_slab = false;       // the workspace in device memory holds this instance's state as its last solve left it
    bool changed = false;       // mcf_batch_set_costs since the last solve
    std::vector<int64_t> new_cost;
};

struct DeviceBuffers {
    unsigned char *slab = nullptr, *stage = nullptr;
    BatchSlot *slots = nullptr;
    int32_t *ids = nullptr, *traces = nullptr;
    size_t stage_bytes = 0;
    DeviceBuffers() = default;
    DeviceBuffers(const DeviceBuffers &) = delete;
    DeviceBuffers &operator=(const DeviceBuffers &) = delete;
    ~DeviceBuffers()
    {
        if (slab) (void)hipFree(slab);
        if (stage) (void)hipFree(stage);
        if (slots) (void)hipFree(slots);
        if (ids) (void)hipFree(ids);
        if (traces) (void)hipFree(traces);
    }
};

}  // namespace

struct mcf_batch {
    mcf_batch_desc d{};
    std::vector<Instance *> inst;
    bool solved = false;
    mcf_batch_stats stats{};
    mcf_batch_resolve_stats resolve_stats{};
    // device memory lives until mcf_batch_destroy: a re-solve starts from the state the last solve left in the slab
    DeviceBuffers dev;
    uint64_t slab_bytes = 0, trace_entries = 0;
    int lds_max = 0;
    ~mcf_batch() { for (Instance *i : inst) delete i; }
};

namespace {

// what a handle's descriptor says of every solve it runs (mcf_batch_desc and mcf_ubatch_desc agree on these)
struct RunLimits {
    int32_t rule;
    int64_t pivot_limit;
    int32_t trace_capacity;
};
template <class Desc>
RunLimits limits_of(const Desc &d) { return RunLimits{d.pivot_rule, d.pivot_limit, d.trace_capacity}; }

// the rule's state at a cold start (NS.cs:237-270: the constructor's block size), the counts and the limits, for a slot whose graph
// (n, search_arcs, rule, cfg) is set; m = its arcs without the root links
int reset_run_state(BatchSlot &s, const RunLimits &lim, int32_t m)
{
    s.next_arc = 0; s.block_size = 0; s.dyn_min = 0; s.counters[0] = s.counters[1] = 0;
    if (s.rule == MCF_RULE_BLOCK_SEARCH) {
        int32_t block = 0, dyn_min = 0;
        if (const int rc = mcf_block_initial_size(&s.cfg, s.search_arcs, s.n, &block, &dyn_min)) return rc;
        s.block_size = std::max(1, block);
        s.dyn_min = dyn_min;
    }
    s.pivots = 0;
    s.pivot_limit = lim.pivot_limit > 0 ? lim.pivot_limit : 64 * ((int64_t)m + 2 * (int64_t)s.n) + 1024;
    s.max_iter = std::max<int64_t>(1000000, (int64_t)s.n * (int64_t)m);      // NS.cs:280
    s.trace_cap = lim.trace_capacity;
    s.run = mcf::kBatchRunning;
    s.reprice = 0;
    return MCF_OK;
}

// NS.cs:237-270 for one graph: the configuration `new NetworkSimplex(g).Solve()` chooses, the search range, the rule and its start state.
// Everything in a slot that depends on the topology and the descriptor alone: mcf_batch fills one per instance, mcf_ubatch one per handle
// (the template uniform_begin copies).  all_arcs, workspace and trace are the caller's.
int configure_slot(BatchSlot &s, const RunLimits &lim, int32_t n, int32_t m, const int32_t *tail, const int32_t *head)
{
    if (const int rc = mcf_block_config_auto(&s.cfg, n, m, tail, head)) return rc;
    s.n = n; s.search_arcs = m + n; s.rule = lim.rule;
    return reset_run_state(s, lim, m);
}

// NS.cs:237-270 per instance: the configuration `new NetworkSimplex(g).Solve()` chooses, the constructor's block size, the limits.
// Where the instance's workspace and trace lie does not depend on its costs: a second call (a cold re-solve) keeps them.
int prepare_instance(const mcf_batch *b, Instance *in)
{
    mcf::NsCore &c = in->core;
    BatchSlot &s = in->slot;
    const uint64_t workspace = s.workspace, trace = s.trace;
    s = BatchSlot{};
    s.workspace = workspace; s.trace = trace;
    in->trace_len = 0;
    in->on_device = mcf::core_begin(&c);
    if (!in->on_device) return MCF_OK;
    if (const int rc = configure_slot(s, limits_of(b->d), c.n, c.m, c.tail.data(), c.head.data())) return rc;
    s.all_arcs = c.all_arcs;
    in->layout = layout_of((uint32_t)c.all_arcs, (uint32_t)c.n + 1u);
    in->trace.assign((size_t)std::max(0, b->d.trace_capacity), 0);
    return MCF_OK;
}

// A changed instance before its re-solve.  Warm (its last solve ended Optimal with no flow on an artificial arc): tree, State[] and the standard-form flows stay, the new
// costs go in, the rule's state, the pivot count and the trace start again; the potentials are the kernel's (or the hook's) to recompute.
// Cold (any other ending): everything from the start basis, as in a fresh batch.
int prepare_resolve(const mcf_batch *b, Instance *in, bool *warm)
{
    mcf::NsCore &c = in->core;
    *warm = in->on_device && c.status == MCF_OPTIMAL;
    // Optimal with flow left on an artificial arc is the reference's answer to a surplus it cannot place (core_finish looks at the root
    // links only): the artificial arcs are never searched, so which node keeps the surplus depends on the pivot path.  Cold, like a fresh batch.
    for (int e = c.m + c.n; *warm && e < c.all_arcs; ++e)
        if (c.flow[e] != 0) *warm = false;
    in->changed = false;
    mcf::core_reopen(&c);           // supplies (and flows) in standard form again, whichever way the solve starts
    if (!*warm) {
        mcf::core_recost(&c, in->new_cost.data());
        return prepare_instance(b, in);
    }
    mcf::core_recost(&c, in->new_cost.data());
    if (const int rc = reset_run_state(in->slot, limits_of(b->d), c.m)) return rc;
    in->trace_len = 0;
    in->slot.reprice = 1;
    return MCF_OK;
}

// the end of Solve() for one instance, from how its pivots ended
void finish_instance(Instance *in)
{
    mcf::NsCore &c = in->core;
    if (!in->on_device) return;                                         // Infeasible, set by core_begin
    in->trace_len = std::min<int64_t>(in->slot.pivots, in->slot.trace_cap);
    switch (in->slot.run) {
    case mcf::kBatchNoEntering: mcf::core_finish(&c); break;
    case mcf::kBatchUnbounded: c.status = MCF_UNBOUNDED; break;
    case mcf::kBatchMaxIter: c.status = MCF_INFEASIBLE; break;          // NS.cs:311-317
    default: c.status = MCF_NOT_SOLVED; break;                          // the pivot limit
    }
}

void pack(const Instance *in, unsigned char *base)
{
    const mcf::NsCore &c = in->core;
    const Layout &l = in->layout;
    const size_t A = (size_t)c.all_arcs, N = (size_t)c.n + 1;
    memcpy(base + l.tail, c.tail.data(), 4 * A); memcpy(base + l.head, c.head.data(), 4 * A);
    memcpy(base + l.cost, c.cost.data(), 8 * A); memcpy(base + l.upper, c.upper.data(), 8 * A);
    memcpy(base + l.flow, c.flow.data(), 8 * A); memcpy(base + l.pi, c.pi.data(), 8 * N);
    memcpy(base + l.par, c.par.data(), 4 * N); memcpy(base + l.par_arc, c.par_arc.data(), 4 * N);
    memcpy(base + l.nxt, c.nxt.data(), 4 * N); memcpy(base + l.prv, c.prv.data(), 4 * N);
    memcpy(base + l.sub, c.sub.data(), 4 * N); memcpy(base + l.fin, c.fin.data(), 4 * N);
    memcpy(base + l.state, c.state.data(), A); memcpy(base + l.par_dir, c.par_dir.data(), N);
}
// part: the changing part of the instance's workspace (Layout::changing onwards)
void unpack(Instance *in, const unsigned char *part)
{
    mcf::NsCore &c = in->core;
    const Layout &l = in->layout;
    const size_t A = (size_t)c.all_arcs, N = (size_t)c.n + 1;
    const auto at = [&](uint32_t offset) { return part + (offset - l.changing); };
    memcpy(c.flow.data(), at(l.flow), 8 * A); memcpy(c.pi.data(), at(l.pi), 8 * N);
    memcpy(c.par.data(), at(l.par), 4 * N); memcpy(c.par_arc.data(), at(l.par_arc), 4 * N);
    memcpy(c.nxt.data(), at(l.nxt), 4 * N); memcpy(c.prv.data(), at(l.prv), 4 * N);
    memcpy(c.sub.data(), at(l.sub), 4 * N); memcpy(c.fin.data(), at(l.fin), 4 * N);
    memcpy(c.state.data(), at(l.state), A); memcpy(c.par_dir.data(), at(l.par_dir), N);
}

// the pivots of one instance with one lane on the host (the test hooks)
void run_instance_on_host(Instance *in)
{
    mcf::NsCore &c = in->core;
    mcf::BatchWork w{};
    load_slot(w, in->slot, in->trace.data());
    w.trace = in->slot.trace_cap > 0 ? in->trace.data() : nullptr;      // the host keeps a trace per instance, not one buffer
    static_cast<mcf::TreeView &>(w) = c.tree();
    w.cost = c.cost.data(); w.state = c.state.data(); w.pi = c.pi.data();
    if (in->slot.reprice) mcf::batch_reprice(w, 0, 1);
    mcf::batch_run(w, 0, 1, INT64_MAX);
    store_slot(in->slot, w);
}

int at(mcf_batch *b, int32_t index, Instance **out)
{
    if (!b) return mcf::fail(MCF_ERR_INVALID, "null batch");
    if (index < 0 || (size_t)index >= b->inst.size()) return mcf::fail(MCF_ERR_INVALID, "instance %d is not in the batch (%zu instances)", index, b->inst.size());
    if (!b->solved) return mcf::fail(MCF_ERR_STATE, "the batch has not been solved");
    *out = b->inst[(size_t)index];
    return MCF_OK;
}

int begin_solve(mcf_batch *b)
{
    if (!b) return mcf::fail(MCF_ERR_INVALID, "null batch");
    if (b->solved) return mcf::fail(MCF_ERR_STATE, "a batch is solved once (Solve() is single-shot, NS.cs:649); create a new batch, or give it new costs (mcf_batch_set_costs) and re-solve");
    return MCF_OK;
}

int begin_resolve(mcf_batch *b, const char *what)
{
    if (!b) return mcf::fail(MCF_ERR_INVALID, "null batch");
    if (!b->solved) return mcf::fail(MCF_ERR_STATE, "%s: the batch has not been solved", what);
    return MCF_OK;
}

int have_device(int32_t device, const char *what)
{
    int devices = 0;
    if (hipGetDeviceCount(&devices) != hipSuccess || devices < 1) { (void)hipGetLastError(); return mcf::fail(MCF_ERR_NO_DEVICE, "%s: no HIP device (the host hooks are test hooks, not solvers)", what); }
    if (device >= devices) return mcf::fail(MCF_ERR_NO_DEVICE, "%s: device %d of %d", what, device, devices);
    return MCF_OK;
}

// makes the device current; *lds_max_out = the dynamic LDS one workgroup of batch_kernel<true> may have
int open_device(int32_t device, int *lds_max_out)
{
    HIP_TRY(hipSetDevice(device));
    // the LDS one workgroup may have: the device's figure, never a constant of ours
    int lds_max = 0, lds_optin = 0;
    HIP_TRY(hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, device));
    if (hipDeviceGetAttribute(&lds_optin, hipDeviceAttributeSharedMemPerBlockOptin, device) != hipSuccess) { (void)hipGetLastError(); lds_optin = 0; }
    if (lds_optin > lds_max) lds_max = lds_optin;
    // the opt-in for dynamic LDS above the default limit; where the runtime refuses it, the default limit of 64 KiB holds
    if (hipFuncSetAttribute((const void *)batch_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max) != hipSuccess) {
        (void)hipGetLastError();
        lds_max = std::min(lds_max, 64 << 10);
    }
    if (hipFuncSetAttribute((const void *)batch_dual_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max) != hipSuccess) {
        (void)hipGetLastError();
        lds_max = std::min(lds_max, 64 << 10);
    }
    *lds_max_out = lds_max;
    return MCF_OK;
}

// Groups: the LDS tier in classes of the footprint (lds_max / 16, / 8, / 4, / 3, / 2, / 1: the steps at which one more workgroup fits a CU),
// each launched with the largest footprint it holds, so that no launch sizes every workgroup for the batch's largest; the global tier last.
constexpr int kClasses = 7;
int class_of(int lds_max, uint32_t bytes)
{
    const int divisor[kClasses - 1] = {16, 8, 4, 3, 2, 1};
    for (int k = 0; k < kClasses - 1; ++k)
        if ((int64_t)bytes <= (int64_t)lds_max / divisor[k]) return k;
    return kClasses - 1;
}

// places the workspaces and the traces of the instances that run on the device and allocates the device's buffers
int allocate(mcf_batch *b)
{
    const size_t count = b->inst.size();
    b->slab_bytes = b->trace_entries = 0;
    for (Instance *in : b->inst) {
        if (!in->on_device) continue;
        in->slot.workspace = b->slab_bytes; b->slab_bytes += in->layout.bytes;
        in->slot.trace = b->trace_entries; b->trace_entries += (uint64_t)in->slot.trace_cap;
    }
    if (!b->slab_bytes) return MCF_OK;
    HIP_TRY(hipMalloc((void **)&b->dev.slab, (size_t)b->slab_bytes));
    HIP_TRY(hipMalloc((void **)&b->dev.slots, count * sizeof(BatchSlot)));
    HIP_TRY(hipMalloc((void **)&b->dev.ids, count * sizeof(int32_t)));
    HIP_TRY(hipMalloc((void **)&b->dev.traces, (size_t)std::max<uint64_t>(b->trace_entries, 1) * sizeof(int32_t)));
    return MCF_OK;
}

struct LaunchTotals {
    int64_t launches = 0, lds_bytes_max = 0, bytes_down = 0, bytes_up = 0;
    double kernel_ns = 0;
};

// what the launch loop needs of a handle: the device's buffers, the LDS limit, the budget of a launch and every instance's footprint --
// one figure per instance (mcf_batch: the instances differ) or one for all (mcf_ubatch: one topology, workspaces at a fixed stride, so
// the whole batch is one class)
struct LaunchPlan {
    DeviceBuffers *dev;
    int lds_max;
    int32_t pivots_per_launch;          // the descriptor's: 0 = the default
    const uint32_t *footprint;          // per instance, or null:
    uint32_t footprint_all;
    bool dual = false;                  // a re-solve with new supplies or bounds: batch_dual_kernel, and kBatchDual runs on like kBatchRunning
    uint32_t bytes(int32_t i) const { return footprint ? footprint[(size_t)i] : footprint_all; }
};

// Relaunches the instances `run` (ascending; their slots are on the device) until none is left running; every round ends in a
// synchronising copy of the slots between the first and the last of them.  slots: the host's copy of every slot.
int run_launches(const LaunchPlan &plan, std::vector<BatchSlot> &slots, const std::vector<int32_t> &run, LaunchTotals *t)
{
    if (run.empty()) return MCF_OK;
    std::vector<int32_t> group[kClasses];
    for (int32_t i : run) group[class_of(plan.lds_max, plan.bytes(i))].push_back(i);
    const size_t lo = (size_t)run.front(), span = (size_t)run.back() - lo + 1;
    const int32_t budget = plan.pivots_per_launch > 0 ? plan.pivots_per_launch : kDefaultPivotsPerLaunch;
    DeviceBuffers &dev = *plan.dev;
    std::vector<int32_t> ids;
    for (;;) {
        ids.clear();
        struct Launch { int first, n; uint32_t lds; bool in_lds; };
        std::vector<Launch> launches;
        for (int g = 0; g < kClasses; ++g) {
            Launch L{(int)ids.size(), 0, 0, g != kClasses - 1};
            for (int32_t i : group[g]) {
                if (slots[(size_t)i].run != mcf::kBatchRunning && slots[(size_t)i].run != mcf::kBatchDual) continue;
                ids.push_back(i);
                L.n++;
                L.lds = std::max(L.lds, plan.bytes(i));
            }
            if (L.n) launches.push_back(L);
        }
        if (launches.empty()) break;
        const double tk = mcf::now_ns();
        HIP_TRY(hipMemcpy(dev.ids, ids.data(), ids.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        t->bytes_up += (int64_t)(ids.size() * sizeof(int32_t));
        for (const Launch &L : launches) {
            const auto kernel = L.in_lds ? (plan.dual ? batch_dual_kernel<true> : batch_kernel<true>) : (plan.dual ? batch_dual_kernel<false> : batch_kernel<false>);
            hipLaunchKernelGGL(kernel, dim3((unsigned)L.n), dim3(kBatchThreads), L.in_lds ? L.lds : 0, 0, dev.slots, dev.ids + L.first, dev.slab, dev.traces, budget);
            if (L.in_lds) t->lds_bytes_max = std::max<int64_t>(t->lds_bytes_max, L.lds);
            HIP_TRY(hipGetLastError());
            t->launches++;
        }
        HIP_TRY(hipMemcpy(slots.data() + lo, dev.slots + lo, span * sizeof(BatchSlot), hipMemcpyDeviceToHost));     // waits for the launches
        t->bytes_down += (int64_t)(span * sizeof(BatchSlot));
        t->kernel_ns += mcf::now_ns() - tk;
    }
    return MCF_OK;
}

// the recorded entering arcs of the instances `run`, from one copy of the trace buffer between the first and the last of them
int fetch_traces(mcf_batch *b, const std::vector<int32_t> &run, int64_t *bytes_down)
{
    if (run.empty() || !b->trace_entries) return MCF_OK;
    const Instance *first = b->inst[(size_t)run.front()], *last = b->inst[(size_t)run.back()];
    const uint64_t lo = first->slot.trace, hi = last->slot.trace + (uint64_t)last->slot.trace_cap;
    std::vector<int32_t> traces((size_t)(hi - lo));
    if (hi > lo) HIP_TRY(hipMemcpy(traces.data(), b->dev.traces + lo, (size_t)(hi - lo) * sizeof(int32_t), hipMemcpyDeviceToHost));
    *bytes_down += (int64_t)((hi - lo) * sizeof(int32_t));
    for (int32_t i : run) {
        Instance *in = b->inst[(size_t)i];
        const int64_t len = std::min<int64_t>(in->slot.pivots, in->slot.trace_cap);
        const ptrdiff_t from = (ptrdiff_t)(in->slot.trace - lo);
        if (len > 0) std::copy(traces.begin() + from, traces.begin() + from + (ptrdiff_t)len, in->trace.begin());
    }
    return MCF_OK;
}

// rules, semantics, flags and limits of a batch of either kind (mcf_batch_desc and mcf_ubatch_desc agree on these fields)
template <class Desc>
int check_batch_desc(const Desc &d, const char *who)
{
    if (d.pivot_rule == MCF_RULE_CANDIDATE_LIST || d.pivot_rule == MCF_RULE_ALTERING_LIST)
        return mcf::fail(MCF_ERR_INVALID, "%s: the list rules (Candidate List, Altering List) are not part of the batch solver; use mcf_ns_set_list_pivot_rule", who);
    if (d.pivot_rule != MCF_RULE_FIRST_ELIGIBLE && d.pivot_rule != MCF_RULE_BEST_ELIGIBLE && d.pivot_rule != MCF_RULE_BLOCK_SEARCH)
        return mcf::fail(MCF_ERR_INVALID, "%s: unknown pivot rule %d", who, d.pivot_rule);
    if (d.semantics == MCF_SEM_OPTIMIZED)
        return mcf::fail(MCF_ERR_INVALID, "%s: MCF_SEM_OPTIMIZED (BlockSearchPivotOptimized and its vector-width reading) is not part of the batch solver; use mcf_ns_solve", who);
    if (d.semantics != 0 && d.semantics != MCF_SEM_PLAIN) return mcf::fail(MCF_ERR_INVALID, "%s: unknown semantics %d", who, d.semantics);
    if (d.flags & MCF_BATCH_SHARDED) return mcf::fail(MCF_ERR_INVALID, "%s: sharding is not part of the batch solver (a batch runs on one device)", who);
    if (d.flags & ~MCF_BATCH_SHARDED) return mcf::fail(MCF_ERR_INVALID, "%s: unknown flags %d", who, d.flags);
    if (d.device < 0 || d.pivot_limit < 0 || d.pivots_per_launch < 0 || d.trace_capacity < 0)
        return mcf::fail(MCF_ERR_INVALID, "%s: negative device, pivot limit, pivots per launch or trace capacity", who);
    return MCF_OK;
}

// the incidence lists of one graph, inc_start[n + 1] and inc[2m]: a stable counting sort of the 2m arc ends by node, so arc ids ascend
// within a node; a self-loop is there twice
void build_incidence(size_t n, size_t m, const int32_t *source, const int32_t *target, int32_t *inc_start, int32_t *inc)
{
    std::fill(inc_start, inc_start + n + 1, 0);
    for (size_t e = 0; e < m; ++e) { ++inc_start[(size_t)source[e] + 1]; ++inc_start[(size_t)target[e] + 1]; }
    for (size_t v = 0; v < n; ++v) inc_start[v + 1] += inc_start[v];
    std::vector<int32_t> next(inc_start, inc_start + n);
    for (size_t e = 0; e < m; ++e) {
        inc[(size_t)next[(size_t)source[e]]++] = (int32_t)(e << 1);
        inc[(size_t)next[(size_t)target[e]]++] = (int32_t)(e << 1 | 1);
    }
}

// the launch plan of a mcf_batch: `footprints` gets every instance's workspace size and must outlive the plan
LaunchPlan plan_of(mcf_batch *b, std::vector<uint32_t> &footprints)
{
    footprints.resize(b->inst.size());
    for (size_t i = 0; i < b->inst.size(); ++i) footprints[i] = b->inst[i]->layout.bytes;
    return LaunchPlan{&b->dev, b->lds_max, b->d.pivots_per_launch, footprints.data(), 0};
}

}  // namespace

extern "C" {

int mcf_batch_create(mcf_batch **out, const mcf_batch_desc *desc)
{
    if (!out || !desc) return mcf::fail(MCF_ERR_INVALID, "mcf_batch_create: null argument");
    *out = nullptr;
    if (const int rc = check_batch_desc(*desc, "mcf_batch_create")) return rc;
    mcf_batch *b = new mcf_batch();
    b->d = *desc;
    b->d.semantics = MCF_SEM_PLAIN;
    *out = b;
    return MCF_OK;
}

void mcf_batch_destroy(mcf_batch *b) { delete b; }

int mcf_batch_add(mcf_batch *b, int32_t node_count, int32_t arc_count, const int32_t *source, const int32_t *target, const int64_t *lower,
                  const int64_t *upper, const int64_t *cost, const int64_t *supply, int32_t supply_type, int32_t *index)
{
    if (!b) return mcf::fail(MCF_ERR_INVALID, "null batch");
    if (b->solved) return mcf::fail(MCF_ERR_STATE, "the batch has been solved; create a new batch");
    if (supply_type != MCF_SUPPLY_GEQ && supply_type != MCF_SUPPLY_LEQ) return mcf::fail(MCF_ERR_INVALID, "Invalid supply type");
    if (arc_count > MCF_BATCH_MAX_ARCS || node_count > MCF_BATCH_MAX_NODES)
        return mcf::fail(MCF_ERR_INVALID, "mcf_batch_add: %d nodes / %d arcs is above the batch solver's limit of %d / %d per instance; solve it with mcf_ns_solve",
                         node_count, arc_count, MCF_BATCH_MAX_NODES, MCF_BATCH_MAX_ARCS);
    if (b->inst.size() >= (size_t)MCF_BATCH_MAX_INSTANCES) return mcf::fail(MCF_ERR_INVALID, "mcf_batch_add: a batch holds at most %d instances", MCF_BATCH_MAX_INSTANCES);
    Instance *in = new Instance();
    if (const int rc = mcf::core_create(&in->core, node_count, arc_count, source, target)) { delete in; return rc; }
    mcf::core_set_problem(&in->core, lower, upper, cost, supply);
    in->core.supply_type = supply_type;
    if (index) *index = (int32_t)b->inst.size();
    b->inst.push_back(in);
    b->stats.instances = (int64_t)b->inst.size();
    return MCF_OK;
}

int mcf_batch_run_on_host(mcf_batch *b)
{
    if (const int rc = begin_solve(b)) return rc;
    const double t0 = mcf::now_ns();
    b->solved = true;
    int64_t total = 0;
    for (Instance *in : b->inst) {
        if (const int rc = prepare_instance(b, in)) return rc;
        if (in->on_device) {
            run_instance_on_host(in);
            total += in->slot.pivots;
        }
        finish_instance(in);
    }
    b->stats.total_pivots = total;
    b->stats.host_ns = mcf::now_ns() - t0;
    return MCF_OK;
}

int mcf_batch_solve(mcf_batch *b)
{
    if (const int rc = begin_solve(b)) return rc;
    if (const int rc = have_device(b->d.device, "mcf_batch_solve")) return rc;
    const double t_start = mcf::now_ns();
    b->solved = true;
    if (const int rc = open_device(b->d.device, &b->lds_max)) return rc;

    // set every instance up; place the workspaces
    const size_t count = b->inst.size();
    for (Instance *in : b->inst)
        if (const int rc = prepare_instance(b, in)) return rc;
    if (const int rc = allocate(b)) return rc;
    std::vector<BatchSlot> slots(count);
    std::vector<int32_t> run;
    for (size_t i = 0; i < count; ++i) {
        const Instance *in = b->inst[i];
        slots[i] = in->slot;
        if (!in->on_device) continue;
        run.push_back((int32_t)i);
        if (class_of(b->lds_max, in->layout.bytes) == kClasses - 1) b->stats.global_instances++; else b->stats.lds_instances++;
    }
    b->stats.workspace_bytes = (int64_t)b->slab_bytes;

    DeviceBuffers &dev = b->dev;
    std::vector<unsigned char> host_slab((size_t)b->slab_bytes);
    if (b->slab_bytes) {
        for (Instance *in : b->inst) if (in->on_device) { pack(in, host_slab.data() + in->slot.workspace); in->on_slab = true; }
        HIP_TRY(hipMemcpy(dev.slab, host_slab.data(), (size_t)b->slab_bytes, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(dev.slots, slots.data(), count * sizeof(BatchSlot), hipMemcpyHostToDevice));
    }
    LaunchTotals t;
    std::vector<uint32_t> footprints;
    if (const int rc = run_launches(plan_of(b, footprints), slots, run, &t)) return rc;
    b->stats.launches = t.launches;
    b->stats.lds_bytes_max = t.lds_bytes_max;
    // the state comes home; the host finishes every instance
    if (b->slab_bytes) HIP_TRY(hipMemcpy(host_slab.data(), dev.slab, (size_t)b->slab_bytes, hipMemcpyDeviceToHost));
    for (int32_t i : run) {
        Instance *in = b->inst[(size_t)i];
        in->slot = slots[(size_t)i];
        unpack(in, host_slab.data() + in->slot.workspace + in->layout.changing);
    }
    int64_t unused = 0;
    if (const int rc = fetch_traces(b, run, &unused)) return rc;
    int64_t total = 0;
    for (Instance *in : b->inst) {
        if (in->on_device) total += in->slot.pivots;
        finish_instance(in);
    }
    b->stats.total_pivots = total;
    b->stats.kernel_ns = t.kernel_ns;
    b->stats.host_ns = mcf::now_ns() - t_start - t.kernel_ns;
    return MCF_OK;
}

int mcf_batch_set_costs(mcf_batch *b, int32_t index, const int64_t *cost)
{
    Instance *in = nullptr;
    if (!b || !cost) return mcf::fail(MCF_ERR_INVALID, "mcf_batch_set_costs: null argument");
    if (const int rc = at(b, index, &in)) return rc;        // MCF_ERR_STATE before a solve: until then the costs come with mcf_batch_add
    in->new_cost.assign(cost, cost + in->core.m);
    in->changed = true;
    return MCF_OK;
}

int mcf_batch_rerun_on_host(mcf_batch *b)
{
    if (const int rc = begin_resolve(b, "mcf_batch_rerun_on_host")) return rc;
    const double t0 = mcf::now_ns();
    mcf_batch_resolve_stats st{};
    for (Instance *in : b->inst) {
        if (!in->changed) { st.untouched_instances++; continue; }
        bool warm = false;
        if (const int rc = prepare_resolve(b, in, &warm)) return rc;
        if (warm) st.warm_instances++; else st.cold_instances++;
        if (in->on_device) {
            run_instance_on_host(in);
            st.total_pivots += in->slot.pivots;
            in->on_slab = false;            // the device's copy is stale: the next mcf_batch_resolve packs this instance again
        }
        finish_instance(in);
    }
    st.host_ns = mcf::now_ns() - t0;
    b->resolve_stats = st;
    return MCF_OK;
}

int mcf_batch_resolve(mcf_batch *b)
{
    if (const int rc = begin_resolve(b, "mcf_batch_resolve")) return rc;
    const size_t count = b->inst.size();
    std::vector<int32_t> changed;
    for (size_t i = 0; i < count; ++i)
        if (b->inst[i]->changed) changed.push_back((int32_t)i);
    mcf_batch_resolve_stats st{};
    st.untouched_instances = (int64_t)(count - changed.size());
    if (changed.empty()) { b->resolve_stats = st; return MCF_OK; }          // nothing to launch: no device needed either
    if (const int rc = have_device(b->d.device, "mcf_batch_resolve")) return rc;       // the batch is as it was
    const double t_start = mcf::now_ns();
    if (const int rc = open_device(b->d.device, &b->lds_max)) return rc;
    DeviceBuffers &dev = b->dev;

    // Warm instances whose state is in the slab get their new cost[] (through the staging buffer) and their slot; every other instance
    // that runs -- cold, or never packed since the host hooks last ran it -- gets its whole workspace.
    std::vector<int32_t> run, staged;
    uint64_t stage_in = 0, stage_out = 0;
    for (int32_t i : changed) {
        Instance *in = b->inst[(size_t)i];
        bool warm = false;
        if (const int rc = prepare_resolve(b, in, &warm)) return rc;
        if (warm) st.warm_instances++; else st.cold_instances++;
        if (!in->on_device) continue;                                       // infeasible by its bounds, whatever the costs
        run.push_back(i);
        if (warm && in->on_slab) {
            staged.push_back(i);
            in->slot.staged_cost = stage_in; stage_in += in->layout.upper - in->layout.cost;
        }
        in->slot.staged_out = stage_out; stage_out += in->layout.bytes - in->layout.changing;
    }
    if (!run.empty() && !dev.slab)                                          // the first solve was mcf_batch_run_on_host
        if (const int rc = allocate(b)) return rc;
    std::vector<BatchSlot> slots(count);
    for (size_t i = 0; i < count; ++i) slots[i] = b->inst[i]->slot;
    LaunchTotals t;
    if (!run.empty()) {
        const uint64_t stage_need = std::max(stage_in, stage_out);
        if (dev.stage_bytes < stage_need) {
            if (dev.stage) { HIP_TRY(hipFree(dev.stage)); dev.stage = nullptr; dev.stage_bytes = 0; }
            HIP_TRY(hipMalloc((void **)&dev.stage, (size_t)stage_need));
            dev.stage_bytes = (size_t)stage_need;
        }
        const size_t lo = (size_t)run.front(), span = (size_t)run.back() - lo + 1;
        HIP_TRY(hipMemcpy(dev.slots + lo, slots.data() + lo, span * sizeof(BatchSlot), hipMemcpyHostToDevice));
        st.bytes_uploaded += (int64_t)(span * sizeof(BatchSlot));
        std::vector<unsigned char> buffer;
        if (!staged.empty()) {
            buffer.assign((size_t)stage_in, 0);
            for (int32_t i : staged) {
                const Instance *in = b->inst[(size_t)i];
                memcpy(buffer.data() + in->slot.staged_cost, in->core.cost.data(), 8 * (size_t)in->core.all_arcs);
            }
            HIP_TRY(hipMemcpy(dev.stage, buffer.data(), (size_t)stage_in, hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(dev.ids, staged.data(), staged.size() * sizeof(int32_t), hipMemcpyHostToDevice));
            hipLaunchKernelGGL(stage_kernel<true>, dim3((unsigned)staged.size()), dim3(kStageThreads), 0, 0, dev.slots, dev.ids, dev.slab, dev.stage);
            HIP_TRY(hipGetLastError());
            st.bytes_uploaded += (int64_t)stage_in;
        }
        // whole workspaces: neighbours in the slab go in one copy
        for (size_t k = 0; k < run.size();) {
            Instance *in = b->inst[(size_t)run[k]];
            if (in->on_slab && in->slot.reprice) { ++k; continue; }
            const uint64_t begin = in->slot.workspace;
            uint64_t end = begin;
            size_t j = k;
            for (; j < run.size(); ++j) {
                Instance *next = b->inst[(size_t)run[j]];
                if ((next->on_slab && next->slot.reprice) || next->slot.workspace != end) break;
                end += next->layout.bytes;
            }
            buffer.assign((size_t)(end - begin), 0);
            for (size_t q = k; q < j; ++q) {
                Instance *next = b->inst[(size_t)run[q]];
                pack(next, buffer.data() + (next->slot.workspace - begin));
                next->on_slab = true;
            }
            HIP_TRY(hipMemcpy(dev.slab + begin, buffer.data(), (size_t)(end - begin), hipMemcpyHostToDevice));
            st.bytes_uploaded += (int64_t)(end - begin);
            k = j;
        }
        std::vector<uint32_t> footprints;
        if (const int rc = run_launches(plan_of(b, footprints), slots, run, &t)) return rc;
        // only the changing part of the instances that ran comes home
        HIP_TRY(hipMemcpy(dev.ids, run.data(), run.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        hipLaunchKernelGGL(stage_kernel<false>, dim3((unsigned)run.size()), dim3(kStageThreads), 0, 0, dev.slots, dev.ids, dev.slab, dev.stage);
        HIP_TRY(hipGetLastError());
        buffer.resize((size_t)stage_out);
        HIP_TRY(hipMemcpy(buffer.data(), dev.stage, (size_t)stage_out, hipMemcpyDeviceToHost));
        t.bytes_down += (int64_t)stage_out;
        for (int32_t i : run) {
            Instance *in = b->inst[(size_t)i];
            const uint64_t staged_out = in->slot.staged_out;
            in->slot = slots[(size_t)i];
            unpack(in, buffer.data() + staged_out);
        }
        if (const int rc = fetch_traces(b, run, &t.bytes_down)) return rc;
    }
    for (int32_t i : changed) {
        Instance *in = b->inst[(size_t)i];
        if (in->on_device) st.total_pivots += in->slot.pivots;
        finish_instance(in);
    }
    st.launches = t.launches;
    st.bytes_downloaded = t.bytes_down;
    st.kernel_ns = t.kernel_ns;
    st.host_ns = mcf::now_ns() - t_start - t.kernel_ns;
    b->resolve_stats = st;
    return MCF_OK;
}

int mcf_batch_get_resolve_stats(mcf_batch *b, mcf_batch_resolve_stats *out)
{
    if (!b || !out) return mcf::fail(MCF_ERR_INVALID, "null argument");
    if (!b->solved) return mcf::fail(MCF_ERR_STATE, "the batch has not been solved");
    *out = b->resolve_stats;
    return MCF_OK;
}

int mcf_batch_get_status(mcf_batch *b, int32_t index, int32_t *status)
{
    if (!status) return mcf::fail(MCF_ERR_INVALID, "null argument");
    Instance *in = nullptr;
    if (const int rc = at(b, index, &in)) return rc;
    *status = in->core.status;
    return MCF_OK;
}

static int optimal_instance(mcf_batch *b, int32_t index, const void *out, Instance **in)
{
    if (!out) return mcf::fail(MCF_ERR_INVALID, "null argument");
    if (const int rc = at(b, index, in)) return rc;
    if ((*in)->core.status != MCF_OPTIMAL) return mcf::fail(MCF_ERR_STATE, "Solution not optimal");     // NS.cs:418-421
    return MCF_OK;
}
int mcf_batch_get_total_cost(mcf_batch *b, int32_t index, int64_t *cost)
{
    Instance *in = nullptr;
    if (const int rc = optimal_instance(b, index, cost, &in)) return rc;
    *cost = mcf::core_total_cost(&in->core);
    return MCF_OK;
}
int mcf_batch_get_flows(mcf_batch *b, int32_t index, int64_t *out)
{
    Instance *in = nullptr;
    if (const int rc = optimal_instance(b, index, out, &in)) return rc;
    std::copy(in->core.flow.begin(), in->core.flow.begin() + in->core.m, out);
    return MCF_OK;
}
int mcf_batch_get_potentials(mcf_batch *b, int32_t index, int64_t *out)
{
    Instance *in = nullptr;
    if (const int rc = optimal_instance(b, index, out, &in)) return rc;
    std::copy(in->core.pi.begin(), in->core.pi.begin() + in->core.n, out);
    return MCF_OK;
}
int mcf_batch_get_pivots(mcf_batch *b, int32_t index, int64_t *pivots)
{
    if (!pivots) return mcf::fail(MCF_ERR_INVALID, "null argument");
    Instance *in = nullptr;
    if (const int rc = at(b, index, &in)) return rc;
    *pivots = in->on_device ? in->slot.pivots : 0;
    return MCF_OK;
}
int mcf_batch_get_trace(mcf_batch *b, int32_t index, int32_t *out, int64_t capacity, int64_t *length)
{
    if (!length || capacity < 0 || (capacity > 0 && !out)) return mcf::fail(MCF_ERR_INVALID, "null argument");
    Instance *in = nullptr;
    if (const int rc = at(b, index, &in)) return rc;
    *length = in->trace_len;
    std::copy(in->trace.begin(), in->trace.begin() + (ptrdiff_t)std::min(capacity, in->trace_len), out);
    return MCF_OK;
}
int mcf_batch_get_stats(mcf_batch *b, mcf_batch_stats *out)
{
    if (!b || !out) return mcf::fail(MCF_ERR_INVALID, "null argument");
    *out = b->stats;
    return MCF_OK;
}

}  // extern "C"

// ================================================================================================
// mcf_ubatch_* and mcf_rbatch_*: problem data in and results out where they are ("Uniform batch", "Ragged batch").
// One handle body (PlacedBatch) and one set of drivers for both.  What differs between one topology at a fixed stride and a set of
// graphs at running sums -- sizes, tables, how a problem value is formed, the rules only one has -- is a placement: UniformPlacement
// and RaggedPlacement, static members of the same names, chosen at compile time by the entry points.  The kernels and the host loops
// take the placement's Problem and form their views from it (view_of, check_view_of, pairs_of).
// ================================================================================================
namespace {

struct PlacedBatch {
    enum Where { kNowhere, kOnHost, kOnDevice } where = kNowhere;      // who holds the state the last solve of either kind left
    mcf_ubatch_stats stats{};
    mcf_ubatch_redata_stats redata_stats{};     // of the last re-solve with new supplies or bounds
    mcf_ubatch_start_stats start_stats{};       // of the last solve from a given basis
    int32_t supply_type = -1;           // of the last solve call of any kind: a re-solve with new data must name the same
    int lds_max = 0;
    DeviceBuffers dev;                  // slab, slots, ids, traces
    unsigned char *d_tables = nullptr;  // the topology, its incidence lists and the placement's tables: one allocation, up once per handle
    BatchSlot *d_tmpl = nullptr;        // the placement's slot templates, sent with every solve call
    int64_t *d_summary = nullptr;       // validation: invalid instances, the lowest invalid index.  Allocated last: it says the tables are up
    unsigned char *d_io = nullptr;      // MCF_MEM_HOST: the caller's arrays on their way up and down
    size_t d_io_bytes = 0;
    // The queries of the kept state (cost ranges, data ranges, diagnosis, rays): each has its own plan -- the instances by tier and by the class
    // of ITS footprint, planned for the lds_max it names, the id table up once -- and the statistics of its last call that succeeded.
    struct QueryLaunch { int first, n; uint32_t lds; bool in_lds; };
    struct QueryPlan {
        std::vector<QueryLaunch> launches;
        int32_t *d_ids = nullptr;
        int lds_max = -1;
        ~QueryPlan() { if (d_ids) (void)hipFree(d_ids); }
    };
    template <class Stats>
    struct Query {
        QueryPlan plan;
        Stats stats{};
        operator const Stats &() const { return stats; }
    };
    Query<mcf_ubatch_range_stats> cost_ranges;
    Query<mcf_ubatch_data_range_stats> data_ranges;
    Query<mcf_ubatch_diagnose_stats> diagnose;
    Query<mcf_ubatch_rays_stats> rays;
    int64_t *d_query_summary = nullptr; // kQuerySummaryWords, whichever query runs; allocated with the first device call of any of them
    // diagnosis and rays, global tier: the working arrays of whichever runs, diag_work_stride bytes per instance of that tier in launch
    // order (the last call's stride; allocated with the first call that has such instances, grown where a later one needs more)
    unsigned char *d_diag_work = nullptr;
    size_t diag_work_bytes = 0;
    uint64_t diag_work_stride = 0;
    std::vector<unsigned char> h_slab;  // the host hooks' slab, slots and traces: the device's layout
    std::vector<BatchSlot> h_slots;
    std::vector<int32_t> h_traces;
    ~PlacedBatch()
    {
        for (void *p : {(void *)d_tables, (void *)d_tmpl, (void *)d_summary, (void *)d_io, (void *)d_query_summary, (void *)d_diag_work})
            if (p) (void)hipFree(p);
    }
};
constexpr int kQuerySummaryWords = std::max({mcf::kDiagSummaryWords, mcf::kRaysSummaryWords, 3});    // the most any query has

}  // namespace

struct mcf_ubatch : PlacedBatch {
    mcf_ubatch_desc d{};
    std::vector<int32_t> source, target;
    std::vector<int32_t> inc_start, inc; // per node its arcs, arc << 1 | (the node is the target): what mcf_ubatch_validate walks
    BatchSlot tmpl{};                   // everything of a slot that the topology and the descriptor decide (configure_slot), filled once
    uint32_t stride = 0;                // bytes between workspaces
    mcf::UniformProblem dt{};           // the pointers into d_tables: source, target, inc_start, inc
};

struct mcf_rbatch : PlacedBatch {
    mcf_rbatch_desc d{};
    // the tables of ragged_view, as the host hooks read them; the device gets one copy of all of them (d_tables)
    std::vector<int32_t> source, target, inc_start, inc, graph_of;
    std::vector<mcf::RaggedGraph> graphs;
    std::vector<int64_t> arc_row, node_row;     // [count + 1]
    std::vector<uint64_t> workspace;            // [count + 1]: the last entry is the slab's size
    std::vector<uint32_t> footprint;            // [count]: layout_of(m + 2n, n + 1).bytes of the instance's graph
    std::vector<BatchSlot> tmpl;                // one per graph (configure_slot): search_arcs, block configuration and limits go by n and m
    mcf::RaggedProblem dt{};                    // the pointers into d_tables
};

namespace {

// the calls make the handle's device current while they run and leave the caller's (torch's, in a process that has it) as it was
struct DeviceGuard {
    int previous = -1;
    DeviceGuard() { if (hipGetDevice(&previous) != hipSuccess) { (void)hipGetLastError(); previous = -1; } }
    ~DeviceGuard() { if (previous >= 0) (void)hipSetDevice(previous); }
};

// The arrays of a solve call or of a validation call, whichever of the four public structs they came in (io_of, at the entry points).
struct BatchIo {
    bool given, check;                  // given: the caller's pointer was not null.  check: a validation call
    int32_t memory, supply_type;
    const int64_t *lower, *upper, *cost, *supply;
    int64_t lower_stride, upper_stride, cost_stride, supply_stride;     // the uniform structs'; 0 from a ragged one
    const uint8_t *changed;             // re-solves only
    bool basis_given;                   // a solve from a given basis: the caller's basis io was not null ...
    int32_t basis_memory;               // ... and what it says
    const int8_t *start_state;
    int64_t start_stride;               // the uniform struct's; 0 from a ragged one
    int32_t *status;                    // the solution: a solve call writes it; a validation call only reads it, and has no pivots or trace
    int64_t *pivots, *total_cost, *flows, *potentials;
    int32_t *trace;
    int32_t *valid, *errors, *first;    // a validation's answers
    int64_t *objective, *dual_cost;
};
template <class Io>
BatchIo problem_io(const Io *io, bool check)           // what all four structs have
{
    BatchIo x{};
    if (!io) return x;
    x.given = true; x.check = check; x.memory = io->memory; x.supply_type = io->supply_type;
    x.lower = io->lower; x.upper = io->upper; x.cost = io->cost; x.supply = io->supply;
    return x;
}
template <class Io>
BatchIo solve_io(const Io *io)
{
    BatchIo x = problem_io(io, false);
    if (!io) return x;
    x.changed = io->changed;
    x.status = io->status; x.pivots = io->pivots; x.total_cost = io->total_cost; x.flows = io->flows; x.potentials = io->potentials; x.trace = io->trace;
    return x;
}
template <class Io>
BatchIo check_io(const Io *io)
{
    BatchIo x = problem_io(io, true);
    if (!io) return x;
    x.status = const_cast<int32_t *>(io->status); x.total_cost = const_cast<int64_t *>(io->total_cost);
    x.flows = const_cast<int64_t *>(io->flows); x.potentials = const_cast<int64_t *>(io->potentials);
    x.valid = io->valid; x.errors = io->errors; x.first = io->first; x.objective = io->objective; x.dual_cost = io->dual_cost;
    return x;
}
template <class Io>
BatchIo with_strides(BatchIo x, const Io *io)
{
    if (io) { x.lower_stride = io->lower_stride; x.upper_stride = io->upper_stride; x.cost_stride = io->cost_stride; x.supply_stride = io->supply_stride; }
    return x;
}
BatchIo io_of(const mcf_ubatch_io *io) { return with_strides(solve_io(io), io); }
BatchIo io_of(const mcf_rbatch_io *io) { return solve_io(io); }
BatchIo with_basis(BatchIo x, const mcf_ubatch_basis_io *basis)
{
    if (basis) { x.basis_given = true; x.basis_memory = basis->memory; x.start_state = basis->arc_state; x.start_stride = basis->state_stride; }
    return x;
}
BatchIo with_basis(BatchIo x, const mcf_rbatch_basis_io *basis)
{
    if (basis) { x.basis_given = true; x.basis_memory = basis->memory; x.start_state = basis->arc_state; }
    return x;
}
BatchIo io_of(const mcf_ubatch_check_io *io) { return with_strides(check_io(io), io); }
BatchIo io_of(const mcf_rbatch_check_io *io) { return check_io(io); }

// One array of the caller's on its way through the staging buffer of a MCF_MEM_HOST call (stage_arrays): where the call keeps its
// pointer, its true length, whether the call reads it and whether it writes it.
struct StagedArray { void **slot; size_t bytes; bool up, down; };

// ---- The queries of the kept state: mcf_*batch_cost_ranges, _data_ranges, _diagnose and _rays, each a device call and a host hook.  One driver
// runs all of them on both placements (query_on_device, query_on_host, check_query_call); a description says what differs between the
// queries, the way a placement says what differs between the handles:
//   Io, io_of        the call's arrays, whichever public struct they came in
//   Stats, state     a call's statistics, and where the handle keeps the last ones with the query's plan
//   check            the query's own refusals: after those every call has, before "has not been solved"
//   arrays           MCF_MEM_HOST: one StagedArray per array of the caller's
//   footprint        what one instance keeps in LDS: it classes the instances of the LDS tier
//   kWords, outputs, stats_of      the summary words: how many, the step's outputs with them, what they say
//   room             the working arrays of an instance of N nodes (the root among them) that is not served in LDS, in bytes: the global tier's buffer has
//                    as much per block (prepare_work), the host hook as much for the instance at hand
//   pairs            the call's pair lists, for pairs_of
//   step<kLds>       the step of the query's header for one instance: what query_kernel runs with 64 lanes and query_on_host with one
struct PlainQuery {                     // what a query has unless it says otherwise
    static uint32_t room(uint32_t) { return 0; }
    template <class Io> static mcf::PairArgs pairs(const Io &) { return mcf::PairArgs{}; }
};

struct CostRanges : PlainQuery {        // uniform_ranges (ranges_step.hip.h)
    using Stats = mcf_ubatch_range_stats;
    using Outputs = mcf::RangeOutputs;
    struct Io {
        bool given;
        int32_t memory;
        int32_t *ranged;
        int8_t *arc_state;
        int64_t *cost_down, *cost_up;
    };
    template <class T> static Io io_of(const T *io) { return io ? Io{true, io->memory, io->ranged, io->arc_state, io->cost_down, io->cost_up} : Io{}; }
    static PlacedBatch::Query<Stats> &state(PlacedBatch *b) { return b->cost_ranges; }
    template <class P> static int check(const typename P::Handle *, Io *io, const char *what)
    {
        if (!io->cost_down != !io->cost_up) return mcf::fail(MCF_ERR_INVALID, "%s: cost_down and cost_up come together or not at all", what);
        return MCF_OK;
    }
    template <class P> static std::array<StagedArray, 4> arrays(const typename P::Handle *b, Io *io)
    {
        const size_t count = (size_t)b->d.count, arcs = P::arc_rows(b);
        return {{{(void **)&io->ranged, 4 * count, false, true},
                 {(void **)&io->arc_state, arcs, false, true},
                 {(void **)&io->cost_down, 8 * arcs, false, true},
                 {(void **)&io->cost_up, 8 * arcs, false, true}}};
    }
    static uint32_t footprint(int32_t n, int32_t m) { return mcf::range_layout_of((uint32_t)(m + 2 * n), (uint32_t)n + 1u, (uint32_t)m).bytes; }
    static constexpr int kWords = 3;
    static Outputs outputs(const Io &io, int64_t *summary) { return Outputs{io.ranged, io.arc_state, io.cost_down, io.cost_up, summary}; }
    static void stats_of(const int64_t *words, Stats *st) { st->ranged = words[0]; st->tree_arcs = words[1]; st->cycle_hops = words[2]; }
    template <bool kLds>
    MCF_HD static void step(const mcf::InstanceView &v, const Outputs &o, const mcf::PairList &, const BatchSlot &slot, unsigned char *room, int lane, int lanes)
    {
        mcf::uniform_ranges<kLds>(v, o, slot, room, lane, lanes);
    }
};

// how many pairs and ship entries a call's arrays hold, where the host can know (the tables of a ragged MCF_MEM_DEVICE call lie on the device)
struct PairSizes {
    bool known;
    size_t pairs, ships;
};
struct DataRanges : PlainQuery {        // uniform_data_ranges (data_ranges_step.hip.h)
    using Stats = mcf_ubatch_data_range_stats;
    using Outputs = mcf::DataRangeOutputs;
    struct Io {                         // the uniform struct's one pair list or the ragged struct's tables, never both
        bool given;
        int32_t memory;
        const int32_t *pairs;
        int64_t pair_count;                 // the uniform struct's
        const int64_t *pair_row, *ship_row; // the ragged struct's
        int32_t *ranged;
        int8_t *arc_state;
        int64_t *flow_down, *flow_up, *ship_forth, *ship_back;
        PairSizes sizes;                    // what check learned (P::check_pairs)
    };
    static Io io_of(const mcf_ubatch_data_range_io *io)
    {
        if (!io) return Io{};
        return Io{true, io->memory, io->pairs, io->pair_count, nullptr, nullptr, io->ranged, io->arc_state, io->flow_down, io->flow_up, io->ship_forth, io->ship_back, {}};
    }
    static Io io_of(const mcf_rbatch_data_range_io *io)
    {
        if (!io) return Io{};
        return Io{true, io->memory, io->pairs, 0, io->pair_row, io->ship_row, io->ranged, io->arc_state, io->flow_down, io->flow_up, io->ship_forth, io->ship_back, {}};
    }
    static PlacedBatch::Query<Stats> &state(PlacedBatch *b) { return b->data_ranges; }
    template <class P> static int check(const typename P::Handle *b, Io *io, const char *what)
    {
        if (!io->flow_down != !io->flow_up) return mcf::fail(MCF_ERR_INVALID, "%s: flow_down and flow_up come together or not at all", what);
        if (!io->ship_forth != !io->ship_back) return mcf::fail(MCF_ERR_INVALID, "%s: ship_forth and ship_back come together or not at all", what);
        return P::check_pairs(b, *io, what, &io->sizes);
    }
    // the only query with arrays that go up: the pairs and, from a ragged call, their tables.  No pairs: the kernel gets a null list
    template <class P> static std::array<StagedArray, 9> arrays(const typename P::Handle *b, Io *io)
    {
        const size_t count = (size_t)b->d.count, arcs = P::arc_rows(b), graphs = P::template_count(b);
        if (!io->sizes.pairs) io->pairs = nullptr;
        return {{{(void **)&io->pairs, 8 * io->sizes.pairs, true, false},
                 {(void **)&io->pair_row, 8 * (graphs + 1), true, false},
                 {(void **)&io->ship_row, 8 * (count + 1), true, false},
                 {(void **)&io->ranged, 4 * count, false, true},
                 {(void **)&io->arc_state, arcs, false, true},
                 {(void **)&io->flow_down, 8 * arcs, false, true},
                 {(void **)&io->flow_up, 8 * arcs, false, true},
                 {(void **)&io->ship_forth, 8 * io->sizes.ships, false, true},
                 {(void **)&io->ship_back, 8 * io->sizes.ships, false, true}}};
    }
    static uint32_t footprint(int32_t n, int32_t m) { return mcf::data_range_layout_of((uint32_t)m, (uint32_t)n + 1u).bytes; }
    static constexpr int kWords = 3;
    static Outputs outputs(const Io &io, int64_t *summary)
    {
        return Outputs{io.ranged, io.arc_state, io.flow_down, io.flow_up, io.ship_forth, io.ship_back, summary};
    }
    static void stats_of(const int64_t *words, Stats *st) { st->ranged = words[0]; st->walks = words[1]; st->hops = words[2]; }
    static mcf::PairArgs pairs(const Io &io) { return mcf::PairArgs{io.pairs, io.pair_count, io.pair_row, io.ship_row}; }
    template <bool kLds>
    MCF_HD static void step(const mcf::InstanceView &v, const Outputs &o, const mcf::PairList &q, const BatchSlot &slot, unsigned char *room, int lane, int lanes)
    {
        mcf::uniform_data_ranges<kLds>(v, o, q, slot, room, lane, lanes);
    }
};

struct Diagnose : PlainQuery {          // uniform_diagnose (diagnose_step.hip.h)
    using Stats = mcf_ubatch_diagnose_stats;
    using Outputs = mcf::DiagOutputs;
    struct Io {
        bool given;
        int32_t memory;
        int32_t *verdict;
        int64_t *violation;
        int32_t *set_size;
        int8_t *side;
        int64_t *unmet;
    };
    template <class T> static Io io_of(const T *io) { return io ? Io{true, io->memory, io->verdict, io->violation, io->set_size, io->side, io->unmet} : Io{}; }
    static PlacedBatch::Query<Stats> &state(PlacedBatch *b) { return b->diagnose; }
    template <class P> static int check(const typename P::Handle *, Io *, const char *) { return MCF_OK; }
    template <class P> static std::array<StagedArray, 5> arrays(const typename P::Handle *b, Io *io)
    {
        const size_t count = (size_t)b->d.count, nodes = P::node_rows(b);
        return {{{(void **)&io->verdict, 4 * count, false, true},
                 {(void **)&io->violation, 8 * count, false, true},
                 {(void **)&io->set_size, 4 * count, false, true},
                 {(void **)&io->side, nodes, false, true},
                 {(void **)&io->unmet, 8 * nodes, false, true}}};
    }
    static uint32_t footprint(int32_t n, int32_t m) { return mcf::diag_layout_of((uint32_t)m, (uint32_t)n + 1u).bytes; }
    static constexpr int kWords = mcf::kDiagSummaryWords;
    static Outputs outputs(const Io &io, int64_t *summary) { return Outputs{io.verdict, io.violation, io.set_size, io.side, io.unmet, summary}; }
    static void stats_of(const int64_t *words, Stats *st)
    {
        st->none = words[MCF_DIAG_NONE]; st->feasible = words[MCF_DIAG_FEASIBLE]; st->cut = words[MCF_DIAG_CUT]; st->open = words[MCF_DIAG_OPEN];
        st->bounds = words[MCF_DIAG_BOUNDS];
        st->levels = words[MCF_DIAG_BOUNDS + 1]; st->frontier_nodes = words[MCF_DIAG_BOUNDS + 2]; st->inc_entries = words[MCF_DIAG_BOUNDS + 3];
    }
    static uint32_t room(uint32_t N) { return mcf::diag_layout_of(0, N).bytes; }        // unmet, marks and frontiers
    template <bool kLds>
    MCF_HD static void step(const mcf::InstanceView &v, const Outputs &o, const mcf::PairList &, const BatchSlot &slot, unsigned char *room, int lane, int lanes)
    {
        mcf::uniform_diagnose<kLds>(v, o, slot, room, lane, lanes);
    }
};

struct Rays : PlainQuery {              // uniform_rays (rays_step.hip.h)
    using Stats = mcf_ubatch_rays_stats;
    using Outputs = mcf::RaysOutputs;
    struct Io {
        bool given;
        int32_t memory;
        int32_t *verdict;
        int64_t *cycle_cost;
        int32_t *cycle_length;
        int8_t *on_cycle;
        int64_t *label;
    };
    template <class T> static Io io_of(const T *io) { return io ? Io{true, io->memory, io->verdict, io->cycle_cost, io->cycle_length, io->on_cycle, io->label} : Io{}; }
    static PlacedBatch::Query<Stats> &state(PlacedBatch *b) { return b->rays; }
    template <class P> static int check(const typename P::Handle *, Io *, const char *) { return MCF_OK; }
    template <class P> static std::array<StagedArray, 5> arrays(const typename P::Handle *b, Io *io)
    {
        const size_t count = (size_t)b->d.count, arcs = P::arc_rows(b), nodes = P::node_rows(b);
        return {{{(void **)&io->verdict, 4 * count, false, true},
                 {(void **)&io->cycle_cost, 8 * count, false, true},
                 {(void **)&io->cycle_length, 4 * count, false, true},
                 {(void **)&io->on_cycle, arcs, false, true},
                 {(void **)&io->label, 8 * nodes, false, true}}};
    }
    static uint32_t footprint(int32_t n, int32_t m) { return mcf::rays_layout_of((uint32_t)m, (uint32_t)n + 1u).bytes; }
    static constexpr int kWords = mcf::kRaysSummaryWords;
    static Outputs outputs(const Io &io, int64_t *summary) { return Outputs{io.verdict, io.cycle_cost, io.cycle_length, io.on_cycle, io.label, summary}; }
    static void stats_of(const int64_t *words, Stats *st)
    {
        st->none = words[MCF_RAY_NONE]; st->bounded = words[MCF_RAY_BOUNDED]; st->cycle = words[MCF_RAY_CYCLE]; st->bounds = words[MCF_RAY_BOUNDS];
        st->rounds = words[MCF_RAY_BOUNDS + 1]; st->frontier_nodes = words[MCF_RAY_BOUNDS + 2]; st->inc_entries = words[MCF_RAY_BOUNDS + 3];
        st->cycle_arcs = words[MCF_RAY_BOUNDS + 4];
    }
    static uint32_t room(uint32_t N) { return mcf::rays_layout_of(0, N).bytes; }        // labels, preds, marks and frontiers
    template <bool kLds>
    MCF_HD static void step(const mcf::InstanceView &v, const Outputs &o, const mcf::PairList &, const BatchSlot &slot, unsigned char *room, int lane, int lanes)
    {
        mcf::uniform_rays<kLds>(v, o, slot, room, lane, lanes);
    }
};

mcf::UniformOutputs outputs_of(const BatchIo &io)
{
    return mcf::UniformOutputs{io.status, io.pivots, io.total_cost, io.flows, io.potentials, io.trace};
}
mcf::UniformCheck check_of(const BatchIo &io, int64_t *summary)
{
    return mcf::UniformCheck{io.status, io.total_cost, io.valid, io.errors, io.first, io.objective, io.dual_cost, summary};
}
void summary_of(const int64_t words[2], int64_t count, mcf_ubatch_check_summary *out)
{
    out->instances = count;
    out->invalid = words[0];
    out->first_invalid = words[0] ? words[1] : -1;
}
int solution_missing(const char *what)
{
    return mcf::fail(MCF_ERR_INVALID, "%s: status, total_cost, flows and potentials are the solution to check, all four are required", what);
}

// the byte lengths of the caller's arrays that go by arcs and nodes; everything else is one entry (or trace_capacity, or MCF_VAL_KINDS) per instance
struct RowBytes {
    size_t lower, upper, cost, supply, flows, potentials, state;       // state: the rows of a given basis, one byte per arc
};
size_t input_elements(size_t count, int64_t stride, size_t length) { return count ? (count - 1) * (size_t)stride + length : 0; }

// tables in one image, each part on a 16-byte boundary, in one allocation and one copy; parts[k].at = where part k lies in d_tables
struct TablePart {
    const void *host;
    size_t bytes, at;
};
int upload_image(PlacedBatch *b, TablePart *parts, size_t part_count)
{
    size_t total = 0;
    for (size_t k = 0; k < part_count; ++k) { parts[k].at = total; total += (parts[k].bytes + 15) & ~(size_t)15; }
    std::vector<unsigned char> image(total, 0);
    for (size_t k = 0; k < part_count; ++k)
        if (parts[k].bytes) memcpy(image.data() + parts[k].at, parts[k].host, parts[k].bytes);
    // a call that failed half way left what it had allocated: that is kept and filled again, not allocated twice
    if (!b->d_tables) HIP_TRY(hipMalloc((void **)&b->d_tables, std::max<size_t>(total, 16)));
    if (total) HIP_TRY(hipMemcpy(b->d_tables, image.data(), total, hipMemcpyHostToDevice));
    return MCF_OK;
}

// ---- one topology, instance i at i * stride: rows by the caller's strides, one slot template
struct UniformPlacement {
    using Handle = mcf_ubatch;
    using Problem = mcf::UniformProblem;
    // one list for every instance
    static int check_pairs(const Handle *b, const DataRanges::Io &io, const char *what, PairSizes *sizes)
    {
        if (io.pair_count < 0) return mcf::fail(MCF_ERR_INVALID, "%s: negative pair count", what);
        if (io.pair_count > 0 && !io.pairs) return mcf::fail(MCF_ERR_INVALID, "%s: null pairs", what);
        if (io.ship_forth && io.pair_count == 0) return mcf::fail(MCF_ERR_INVALID, "%s: ship rows without pairs", what);
        *sizes = PairSizes{true, (size_t)io.pair_count, (size_t)b->d.count * (size_t)io.pair_count};
        return MCF_OK;
    }
    static void sizes(const Handle *b, size_t, int32_t *n, int32_t *m) { *n = b->d.node_count; *m = b->d.arc_count; }
    static size_t arc_rows(const Handle *b) { return (size_t)b->d.count * (size_t)b->d.arc_count; }
    static size_t node_rows(const Handle *b) { return (size_t)b->d.count * (size_t)b->d.node_count; }
    static size_t slab_bytes(const Handle *b) { return (size_t)b->d.count * (size_t)b->stride; }
    static LaunchPlan plan(Handle *b) { return LaunchPlan{&b->dev, b->lds_max, b->d.pivots_per_launch, nullptr, b->stride}; }     // one class for all
    static const BatchSlot *templates(const Handle *b) { return &b->tmpl; }
    static size_t template_count(const Handle *) { return 1; }
    static RowBytes row_bytes(const Handle *b, const BatchIo &io)
    {
        const size_t count = (size_t)b->d.count, n = (size_t)b->d.node_count, m = (size_t)b->d.arc_count;
        return RowBytes{8 * input_elements(count, io.lower_stride, m), 8 * input_elements(count, io.upper_stride, m), 8 * input_elements(count, io.cost_stride, m),
                        8 * input_elements(count, io.supply_stride, n), 8 * count * m, 8 * count * n, input_elements(count, io.start_stride, m)};
    }
    static int check_rows(const Handle *b, const BatchIo &io, const char *what)
    {
        if (io.lower_stride < 0 || io.upper_stride < 0 || io.cost_stride < 0 || io.supply_stride < 0 || io.start_stride < 0) return mcf::fail(MCF_ERR_INVALID, "%s: negative stride", what);
        if (io.check && b->d.count > 0 && (!io.status || !io.total_cost || !io.flows || !io.potentials)) return solution_missing(what);     // an empty tensor has no address
        return MCF_OK;
    }
    // the topology and its incidence lists
    static int upload_tables(Handle *b)
    {
        TablePart parts[] = {{b->source.data(), b->source.size() * sizeof(int32_t), 0},
                             {b->target.data(), b->target.size() * sizeof(int32_t), 0},
                             {b->inc_start.data(), b->inc_start.size() * sizeof(int32_t), 0},
                             {b->inc.data(), b->inc.size() * sizeof(int32_t), 0}};
        if (const int rc = upload_image(b, parts, 4)) return rc;
        const unsigned char *const base = b->d_tables;
        Problem &p = b->dt;
        p = Problem{};
        p.source = (const int32_t *)(base + parts[0].at); p.target = (const int32_t *)(base + parts[1].at);
        p.inc_start = (const int32_t *)(base + parts[2].at); p.inc = (const int32_t *)(base + parts[3].at);
        return MCF_OK;
    }
    // the problem where the steps run: the topology and its lists in device memory or the host's, with the rows of io
    static Problem problem(const Handle *b, const BatchIo &io, bool on_device)
    {
        Problem p = b->dt;
        if (!on_device) { p.source = b->source.data(); p.target = b->target.data(); p.inc_start = b->inc_start.data(); p.inc = b->inc.data(); }
        p.n = b->d.node_count; p.m = b->d.arc_count; p.supply_type = io.supply_type; p.trace_cap = b->d.trace_capacity;
        p.lower = io.lower; p.upper = io.upper; p.cost = io.cost; p.supply = io.supply;
        p.lower_stride = io.lower_stride; p.upper_stride = io.upper_stride; p.cost_stride = io.cost_stride; p.supply_stride = io.supply_stride;
        p.stride = b->stride;
        p.changed = io.changed;
        p.start_state = io.start_state; p.start_stride = io.start_stride;
        return p;
    }
};

// ---- a set of graphs, instance i's rows and workspace at running sums: tables say where, one slot template per graph
struct RaggedPlacement {
    using Handle = mcf_rbatch;
    using Problem = mcf::RaggedProblem;
    // one list per graph: pair_row says where each begins, ship_row where each instance's answers do.  Tables in host memory are checked
    // against each other; tables in device memory are the caller's word, as the rows of every call are.
    static int check_pairs(const Handle *b, const DataRanges::Io &io, const char *what, PairSizes *sizes)
    {
        const size_t count = (size_t)b->d.count, G = b->graphs.size();
        if (!io.pair_row != !io.ship_row) return mcf::fail(MCF_ERR_INVALID, "%s: pair_row and ship_row come together or not at all", what);
        if (io.pairs && !io.pair_row) return mcf::fail(MCF_ERR_INVALID, "%s: pairs without pair_row and ship_row", what);
        if (io.ship_forth && !io.pair_row) return mcf::fail(MCF_ERR_INVALID, "%s: ship rows without pairs", what);
        *sizes = PairSizes{!io.pair_row, 0, 0};
        if (!io.pair_row || io.memory != MCF_MEM_HOST) return MCF_OK;
        if (io.pair_row[0] != 0 || io.ship_row[0] != 0) return mcf::fail(MCF_ERR_INVALID, "%s: pair_row and ship_row begin at 0", what);
        for (size_t g = 0; g < G; ++g)
            if (io.pair_row[g + 1] < io.pair_row[g]) return mcf::fail(MCF_ERR_INVALID, "%s: negative pair count of graph %zu", what, g);
        for (size_t i = 0; i < count; ++i) {
            const size_t g = (size_t)b->graph_of[i];
            if (io.ship_row[i + 1] - io.ship_row[i] != io.pair_row[g + 1] - io.pair_row[g])
                return mcf::fail(MCF_ERR_INVALID, "%s: ship_row gives instance %zu %lld answers, its graph has %lld pairs", what, i,
                                 (long long)(io.ship_row[i + 1] - io.ship_row[i]), (long long)(io.pair_row[g + 1] - io.pair_row[g]));
        }
        if (io.pair_row[G] > 0 && !io.pairs) return mcf::fail(MCF_ERR_INVALID, "%s: null pairs", what);
        if (io.ship_forth && io.ship_row[count] == 0 && io.pair_row[G] == 0) return mcf::fail(MCF_ERR_INVALID, "%s: ship rows without pairs", what);
        *sizes = PairSizes{true, (size_t)io.pair_row[G], (size_t)io.ship_row[count]};
        return MCF_OK;
    }
    static void sizes(const Handle *b, size_t i, int32_t *n, int32_t *m) { const mcf::RaggedGraph &g = b->graphs[(size_t)b->graph_of[i]]; *n = g.n; *m = g.m; }
    static size_t arc_rows(const Handle *b) { return (size_t)b->arc_row[(size_t)b->d.count]; }
    static size_t node_rows(const Handle *b) { return (size_t)b->node_row[(size_t)b->d.count]; }
    static size_t slab_bytes(const Handle *b) { return (size_t)b->workspace[(size_t)b->d.count]; }
    static LaunchPlan plan(Handle *b) { return LaunchPlan{&b->dev, b->lds_max, b->d.pivots_per_launch, b->footprint.data(), 0}; }  // a class per instance
    static const BatchSlot *templates(const Handle *b) { return b->tmpl.data(); }
    static size_t template_count(const Handle *b) { return b->tmpl.size(); }
    static RowBytes row_bytes(const Handle *b, const BatchIo &)
    {
        const size_t arcs = 8 * (size_t)b->arc_row[(size_t)b->d.count], nodes = 8 * (size_t)b->node_row[(size_t)b->d.count];
        return RowBytes{arcs, arcs, arcs, nodes, arcs, nodes, arcs / 8};
    }
    static int check_rows(const Handle *b, const BatchIo &io, const char *what)
    {
        const size_t count = (size_t)b->d.count;
        if (io.check && count > 0 && (!io.status || !io.total_cost || (b->arc_row[count] && !io.flows) || (b->node_row[count] && !io.potentials)))    // an empty tensor has no address
            return solution_missing(what);
        return MCF_OK;
    }
    // the tables, the topology and its incidence lists
    static int upload_tables(Handle *b)
    {
        const size_t count = (size_t)b->d.count;
        TablePart parts[] = {{b->graph_of.data(), count * sizeof(int32_t), 0},
                             {b->graphs.data(), b->graphs.size() * sizeof(mcf::RaggedGraph), 0},
                             {b->arc_row.data(), (count + 1) * sizeof(int64_t), 0},
                             {b->node_row.data(), (count + 1) * sizeof(int64_t), 0},
                             {b->workspace.data(), count * sizeof(uint64_t), 0},
                             {b->source.data(), b->source.size() * sizeof(int32_t), 0},
                             {b->target.data(), b->target.size() * sizeof(int32_t), 0},
                             {b->inc_start.data(), b->inc_start.size() * sizeof(int32_t), 0},
                             {b->inc.data(), b->inc.size() * sizeof(int32_t), 0}};
        if (const int rc = upload_image(b, parts, 9)) return rc;
        const unsigned char *const base = b->d_tables;
        Problem &r = b->dt;
        r = Problem{};
        r.graph_of = (const int32_t *)(base + parts[0].at); r.graphs = (const mcf::RaggedGraph *)(base + parts[1].at);
        r.arc_row = (const int64_t *)(base + parts[2].at); r.node_row = (const int64_t *)(base + parts[3].at);
        r.workspace = (const uint64_t *)(base + parts[4].at);
        r.source = (const int32_t *)(base + parts[5].at); r.target = (const int32_t *)(base + parts[6].at);
        r.inc_start = (const int32_t *)(base + parts[7].at); r.inc = (const int32_t *)(base + parts[8].at);
        return MCF_OK;
    }
    // the tables where the steps run, with the rows of io
    static Problem problem(const Handle *b, const BatchIo &io, bool on_device)
    {
        Problem r = b->dt;
        if (!on_device) {
            r.graph_of = b->graph_of.data(); r.graphs = b->graphs.data();
            r.arc_row = b->arc_row.data(); r.node_row = b->node_row.data(); r.workspace = b->workspace.data();
            r.source = b->source.data(); r.target = b->target.data(); r.inc_start = b->inc_start.data(); r.inc = b->inc.data();
        }
        r.supply_type = io.supply_type; r.trace_cap = b->d.trace_capacity;
        r.lower = io.lower; r.upper = io.upper; r.cost = io.cost; r.supply = io.supply;
        r.changed = io.changed;
        r.start_state = io.start_state;
        return r;
    }
};

// what every call refuses before it touches the handle.  Solve calls take MCF_SUPPLY_GEQ / _LEQ, validation calls MCF_SUPPLY_EQ too
// a solve call: fresh, a re-solve with new costs, or a re-solve with new supplies and bounds
// or a solve that starts from a basis the caller supplies
enum Call { kFresh, kRecost, kRedata, kStart };
inline bool is_resolve(Call call) { return call == kRecost || call == kRedata; }        // goes on from the state the last call left
inline bool has_attempts(Call call) { return call == kRedata || call == kStart; }       // dual phase, settle launch, fallback

template <class P>
int check_call(const typename P::Handle *b, const BatchIo &io, const char *what, bool host_only, Call call)
{
    const bool resolve = is_resolve(call);
    if (!b || !io.given || (call == kStart && !io.basis_given)) return mcf::fail(MCF_ERR_INVALID, "%s: null argument", what);
    if (io.memory != MCF_MEM_HOST && io.memory != MCF_MEM_DEVICE) return mcf::fail(MCF_ERR_INVALID, "%s: unknown memory kind %d", what, io.memory);
    if (host_only && io.memory != MCF_MEM_HOST) return mcf::fail(MCF_ERR_INVALID, "%s: the host hooks read and write host memory (MCF_MEM_HOST)", what);
    if (!io.check) {
        if (io.supply_type != MCF_SUPPLY_GEQ && io.supply_type != MCF_SUPPLY_LEQ) return mcf::fail(MCF_ERR_INVALID, "Invalid supply type");
    } else if (io.supply_type < MCF_SUPPLY_GEQ || io.supply_type > MCF_SUPPLY_EQ) {
        return mcf::fail(MCF_ERR_INVALID, "%s: supply type %d", what, io.supply_type);
    }
    if (const int rc = P::check_rows(b, io, what)) return rc;
    if (call == kStart) {
        if (io.basis_memory != io.memory) return mcf::fail(MCF_ERR_INVALID, "%s: the basis lies in memory kind %d, the problem in %d: one call, one kind", what, io.basis_memory, io.memory);
        if (!io.start_state && P::arc_rows(b)) return mcf::fail(MCF_ERR_INVALID, "%s: null arc_state", what);
        if (io.changed) return mcf::fail(MCF_ERR_INVALID, "%s: a solve from a given basis takes no `changed` mask (an unmarked instance of a fresh handle would have no state)", what);
    }
    if (resolve && b->where == PlacedBatch::kNowhere) return mcf::fail(MCF_ERR_STATE, "%s: the batch has not been solved", what);
    if (call == kRedata && io.supply_type != b->supply_type)
        return mcf::fail(MCF_ERR_INVALID, "%s: supply type %d, the last solve's was %d (the kept basis belongs to that one)", what, io.supply_type, b->supply_type);
    return MCF_OK;
}

// the placement's tables go up once per handle, with its first device call of any kind
template <class P>
int ensure_tables(typename P::Handle *b)
{
    if (b->d_summary) return MCF_OK;
    if (const int rc = P::upload_tables(b)) return rc;
    HIP_TRY(hipMalloc((void **)&b->d_summary, 2 * sizeof(int64_t)));          // last: it says the rest is there
    return MCF_OK;
}

template <class P>
int ensure_device_buffers(typename P::Handle *b)
{
    if (const int rc = ensure_tables<P>(b)) return rc;
    DeviceBuffers &dev = b->dev;
    if (dev.slab) return MCF_OK;
    const size_t count = (size_t)b->d.count;
    // a call that failed half way left what it had allocated: those are kept.  The slab comes last and says the rest is there
    if (!dev.slots) HIP_TRY(hipMalloc((void **)&dev.slots, count * sizeof(BatchSlot)));
    if (!dev.ids) HIP_TRY(hipMalloc((void **)&dev.ids, count * sizeof(int32_t)));
    if (!dev.traces) HIP_TRY(hipMalloc((void **)&dev.traces, std::max<size_t>(count * (size_t)b->d.trace_capacity, 1) * sizeof(int32_t)));
    if (!b->d_tmpl) HIP_TRY(hipMalloc((void **)&b->d_tmpl, std::max<size_t>(P::template_count(b), 1) * sizeof(BatchSlot)));
    HIP_TRY(hipMalloc((void **)&dev.slab, std::max<size_t>(P::slab_bytes(b), 16)));
    return MCF_OK;
}

// MCF_MEM_HOST: one copy up per array the call reads and one down per array it writes, through one device buffer
struct Staged {
    struct Piece { const void *host_in; void *host_out; size_t offset, bytes; };
    std::vector<Piece> pieces;
    size_t total = 0;
    // returns the offset; the device pointer is known once the buffer is
    size_t add(const void *in, void *out, size_t bytes)
    {
        const size_t at = total;
        pieces.push_back(Piece{in, out, at, bytes});
        total += (bytes + 15) & ~(size_t)15;
        return at;
    }
};

// the staging buffer of MCF_MEM_HOST calls holds at least `bytes`
int reserve_io(PlacedBatch *b, size_t bytes)
{
    if (b->d_io_bytes >= bytes) return MCF_OK;
    if (b->d_io) { HIP_TRY(hipFree(b->d_io)); b->d_io = nullptr; b->d_io_bytes = 0; }
    HIP_TRY(hipMalloc((void **)&b->d_io, bytes));
    b->d_io_bytes = bytes;
    return MCF_OK;
}

// The state the last solve call left moves whole, slab and slots, to where the next call runs.  Neither changes `where`: the caller
// does, once the state there is the one that counts.
int state_to_device(PlacedBatch *b, size_t count, int64_t *bytes_up)     // the device's buffers are there (ensure_device_buffers)
{
    if (b->where != PlacedBatch::kOnHost) return MCF_OK;
    if (!b->h_slab.empty()) HIP_TRY(hipMemcpy(b->dev.slab, b->h_slab.data(), b->h_slab.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(b->dev.slots, b->h_slots.data(), count * sizeof(BatchSlot), hipMemcpyHostToDevice));
    *bytes_up += (int64_t)(b->h_slab.size() + count * sizeof(BatchSlot));
    return MCF_OK;
}
int state_to_host(PlacedBatch *b, int32_t device, size_t count)          // h_slab and h_slots have their sizes
{
    if (b->where != PlacedBatch::kOnDevice || !count) return MCF_OK;
    const DeviceGuard guard;
    HIP_TRY(hipSetDevice(device));
    if (!b->h_slab.empty()) HIP_TRY(hipMemcpy(b->h_slab.data(), b->dev.slab, b->h_slab.size(), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(b->h_slots.data(), b->dev.slots, count * sizeof(BatchSlot), hipMemcpyDeviceToHost));
    return MCF_OK;
}

// MCF_MEM_HOST: every array of the table that is there gets its piece of the staging buffer (of `at_least` bytes or more), what the call
// reads is uploaded and counted by its true length, and the caller's pointer becomes the staged copy's.  stage_down brings back what
// the call wrote.
int stage_arrays(PlacedBatch *b, const StagedArray *arrays, size_t n, size_t at_least, Staged *st, int64_t *bytes_up)
{
    for (size_t k = 0; k < n; ++k)
        if (void *const host = *arrays[k].slot) st->add(arrays[k].up ? host : nullptr, arrays[k].down ? host : nullptr, arrays[k].bytes);
    if (const int rc = reserve_io(b, std::max(st->total, at_least))) return rc;
    for (const Staged::Piece &pc : st->pieces)
        if (pc.host_in && pc.bytes) {
            HIP_TRY(hipMemcpy(b->d_io + pc.offset, pc.host_in, pc.bytes, hipMemcpyHostToDevice));
            *bytes_up += (int64_t)pc.bytes;
        }
    size_t piece = 0;                                                       // the pieces are the arrays that are there, in the table's order
    for (size_t k = 0; k < n; ++k)
        if (*arrays[k].slot) *arrays[k].slot = b->d_io + st->pieces[piece++].offset;
    return MCF_OK;
}

// The caller's io as the kernels see it: itself for MCF_MEM_DEVICE, staged for MCF_MEM_HOST.  A solve call reads the problem and writes
// the solution; where it will not write every row (a masked re-solve) the solution goes up too.  A validation call reads both and
// writes the answers.
template <class P>
int stage_up(typename P::Handle *b, BatchIo *io, Staged *st, int64_t *bytes_up)
{
    if (io->memory == MCF_MEM_DEVICE) return MCF_OK;
    const size_t count = (size_t)b->d.count, cap = (size_t)b->d.trace_capacity;
    const RowBytes rows = P::row_bytes(b, *io);
    const bool solution_up = io->check || io->changed, solution_down = !io->check;
    const StagedArray arrays[] = {{(void **)&io->lower, rows.lower, true, false},
                            {(void **)&io->upper, rows.upper, true, false},
                            {(void **)&io->cost, rows.cost, true, false},
                            {(void **)&io->supply, rows.supply, true, false},
                            {(void **)&io->changed, count, true, false},
                            {(void **)&io->start_state, rows.state, true, false},
                            {(void **)&io->status, 4 * count, solution_up, solution_down},
                            {(void **)&io->pivots, 8 * count, solution_up, solution_down},
                            {(void **)&io->total_cost, 8 * count, solution_up, solution_down},
                            {(void **)&io->flows, rows.flows, solution_up, solution_down},
                            {(void **)&io->potentials, rows.potentials, solution_up, solution_down},
                            {(void **)&io->trace, 4 * count * cap, solution_up, solution_down},
                            {(void **)&io->valid, 4 * count, false, true},
                            {(void **)&io->errors, 4 * count * MCF_VAL_KINDS, false, true},
                            {(void **)&io->first, 4 * count * MCF_VAL_KINDS, false, true},
                            {(void **)&io->objective, 8 * count, false, true},
                            {(void **)&io->dual_cost, 8 * count, false, true}};
    return stage_arrays(b, arrays, sizeof(arrays) / sizeof(arrays[0]), 0, st, bytes_up);
}
int stage_down(PlacedBatch *b, const Staged &st, int64_t *bytes_down)
{
    for (const Staged::Piece &pc : st.pieces)
        if (pc.host_out && pc.bytes) {
            HIP_TRY(hipMemcpy(pc.host_out, b->d_io + pc.offset, pc.bytes, hipMemcpyDeviceToHost));
            *bytes_down += (int64_t)pc.bytes;
        }
    return MCF_OK;
}

// What a re-solve with new data counts, on the device and in the hook alike.  An instance is warm by the step's rule (uniform_redata left
// it in the dual phase), cold by rule (marked, and started again at once) or untouched; a warm attempt that did not stand and ran again
// cold is a fallback, and the pivots of its attempt stay counted.
struct RedataCount {
    mcf_ubatch_redata_stats st{};
    int64_t primal_starts = 0;             // a solve from a given basis only: accepted with nothing violated (uniform_begin_from)
    void begun(const BatchSlot &s, bool marked)
    {
        if (!marked) st.untouched_instances++;
        else if (s.run == mcf::kBatchDual) st.warm_instances++;
        else if (s.run == mcf::kBatchRunning && s.reprice == 2) primal_starts++;
        else st.cold_instances++;
    }
    void ran(const BatchSlot &s)           // a slot as the launches left it: staged_out = its dual pivots
    {
        st.dual_pivots += (int64_t)s.staged_out;
        st.primal_pivots += s.pivots - (int64_t)s.staged_out;
    }
    void finish(const mcf_ubatch_stats &of_call)
    {
        st.launches = of_call.launches; st.bytes_up = of_call.bytes_up; st.bytes_down = of_call.bytes_down;
        st.kernel_ns = of_call.kernel_ns; st.host_ns = of_call.host_ns; st.begin_ns = of_call.begin_ns; st.finish_ns = of_call.finish_ns;
    }
    mcf_ubatch_start_stats of_start() const        // after finish()
    {
        return mcf_ubatch_start_stats{primal_starts, st.warm_instances, st.cold_instances, st.fallback_instances, st.dual_pivots, st.primal_pivots,
                                      st.launches, st.bytes_up, st.bytes_down, st.kernel_ns, st.host_ns, st.begin_ns, st.finish_ns};
    }
    // the call's statistics into the handle, by its kind
    void record(Call call, PlacedBatch *b)
    {
        if (!has_attempts(call)) return;
        finish(b->stats);
        if (call == kRedata) b->redata_stats = st; else b->start_stats = of_start();
    }
};

// mcf_*batch_solve, _resolve and _resolve_data: set-up (or re-cost, or re-data) launch, the launch loop of mcf_batch_solve, finish launch.
// A re-solve with new data has one more step between the last two: the settle launch, and the launch loop again for the warm attempts
// that did not stand.
template <class P>
int solve_on_device(typename P::Handle *b, BatchIo io, Call call, const char *what)
{
    const bool resolve = is_resolve(call);
    if (const int rc = check_call<P>(b, io, what, false, call)) return rc;
    if (const int rc = have_device(b->d.device, what)) return rc;          // the handle is as it was
    const double t_start = mcf::now_ns();
    const DeviceGuard guard;
    if (const int rc = open_device(b->d.device, &b->lds_max)) return rc;
    const size_t count = (size_t)b->d.count;
    LaunchPlan plan = P::plan(b);
    plan.dual = has_attempts(call);
    b->stats = mcf_ubatch_stats{};
    b->stats.instances = (int64_t)count;
    for (size_t i = 0; i < count; ++i)
        (class_of(b->lds_max, plan.bytes((int32_t)i)) != kClasses - 1 ? b->stats.lds_instances : b->stats.global_instances)++;
    b->stats.workspace_bytes = (int64_t)P::slab_bytes(b);
    if (call == kRedata) b->redata_stats = mcf_ubatch_redata_stats{};
    if (call == kStart) b->start_stats = mcf_ubatch_start_stats{};
    if (!count) { b->where = PlacedBatch::kOnDevice; b->supply_type = io.supply_type; b->stats.host_ns = mcf::now_ns() - t_start; return MCF_OK; }
    if (const int rc = ensure_device_buffers<P>(b)) return rc;
    DeviceBuffers &dev = b->dev;
    if (resolve)                                                            // the last solve was a host hook's: its state goes up whole
        if (const int rc = state_to_device(b, count, &b->stats.bytes_up)) return rc;
    if (!resolve) io.changed = nullptr;
    std::vector<uint8_t> marked;                                            // a re-solve with new data counts its instances by the mask: one byte each
    if (call == kRedata && io.changed) {
        marked.resize(count);
        if (io.memory == MCF_MEM_HOST) memcpy(marked.data(), io.changed, count);
        else {
            HIP_TRY(hipMemcpy(marked.data(), io.changed, count, hipMemcpyDeviceToHost));
            b->stats.bytes_down += (int64_t)count;
        }
    }
    Staged staged;
    if (const int rc = stage_up<P>(b, &io, &staged, &b->stats.bytes_up)) return rc;
    const typename P::Problem p = P::problem(b, io, true);

    const double t_begin = mcf::now_ns();
    HIP_TRY(hipMemcpy(b->d_tmpl, P::templates(b), P::template_count(b) * sizeof(BatchSlot), hipMemcpyHostToDevice));
    b->stats.bytes_up += (int64_t)(P::template_count(b) * sizeof(BatchSlot));
    const auto begin_kernel = call == kFresh    ? step_kernel<typename P::Problem, mcf::uniform_begin>
                              : call == kRecost ? step_kernel<typename P::Problem, mcf::uniform_recost>
                              : call == kRedata ? step_kernel<typename P::Problem, mcf::uniform_redata>
                                                : step_kernel<typename P::Problem, mcf::uniform_begin_from>;
    hipLaunchKernelGGL(begin_kernel, dim3((unsigned)count), dim3(kBatchThreads), 0, 0, p, b->d_tmpl, dev.slots, dev.slab);
    HIP_TRY(hipGetLastError());
    b->where = PlacedBatch::kOnDevice;
    b->supply_type = io.supply_type;
    std::vector<BatchSlot> slots(count);
    HIP_TRY(hipMemcpy(slots.data(), dev.slots, count * sizeof(BatchSlot), hipMemcpyDeviceToHost));      // waits for the launch; says who runs
    b->stats.bytes_down += (int64_t)(count * sizeof(BatchSlot));
    b->stats.begin_ns = mcf::now_ns() - t_begin;

    std::vector<int32_t> run, attempts;
    RedataCount redata;
    for (size_t i = 0; i < count; ++i) {
        if (has_attempts(call)) redata.begun(slots[i], marked.empty() || marked[i]);
        if (slots[i].reprice == 2) attempts.push_back((int32_t)i);            // a warm attempt or an accepted start: kBatchDual, or kBatchRunning from a primal start
        if (slots[i].run == mcf::kBatchRunning || slots[i].run == mcf::kBatchDual) run.push_back((int32_t)i);   // a re-solve's unmarked instances ended their last solve: not running
    }
    LaunchTotals t;
    if (const int rc = run_launches(plan, slots, run, &t)) return rc;
    if (has_attempts(call))
        for (int32_t i : run) redata.ran(slots[(size_t)i]);
    if (!attempts.empty()) {
        // the warm attempts are judged where they lie; the ones that did not stand have been set up again and run like a fresh solve's
        hipLaunchKernelGGL((step_kernel<typename P::Problem, mcf::uniform_redata_settle>), dim3((unsigned)count), dim3(kBatchThreads), 0, 0, p, b->d_tmpl, dev.slots, dev.slab);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpy(slots.data(), dev.slots, count * sizeof(BatchSlot), hipMemcpyDeviceToHost));
        b->stats.bytes_down += (int64_t)(count * sizeof(BatchSlot));
        std::vector<int32_t> again;
        for (int32_t i : attempts)
            if (slots[(size_t)i].run == mcf::kBatchRunning) again.push_back(i);
        redata.st.fallback_instances = (int64_t)again.size();
        if (const int rc = run_launches(plan, slots, again, &t)) return rc;
        for (int32_t i : again) redata.ran(slots[(size_t)i]);
    }
    for (int32_t i : run) b->stats.total_pivots += slots[(size_t)i].pivots;
    b->stats.launches = t.launches;
    b->stats.lds_bytes_max = t.lds_bytes_max;
    b->stats.bytes_up += t.bytes_up;
    b->stats.bytes_down += t.bytes_down;
    b->stats.kernel_ns = t.kernel_ns;

    const double t_finish = mcf::now_ns();
    hipLaunchKernelGGL(finish_kernel<typename P::Problem>, dim3((unsigned)count), dim3(kBatchThreads), 0, 0, p, outputs_of(io), dev.slots, dev.slab, dev.traces);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    b->stats.finish_ns = mcf::now_ns() - t_finish;
    if (const int rc = stage_down(b, staged, &b->stats.bytes_down)) return rc;
    b->stats.host_ns = mcf::now_ns() - t_start - t.kernel_ns;
    redata.record(call, b);
    return MCF_OK;
}

// the pivots of one placed instance with one lane, from its slot and back into it: what a launch loop does for it on the device
void run_slot_on_host(BatchSlot &slot, unsigned char *home, int32_t *traces)
{
    const int32_t attempt = slot.reprice;
    mcf::BatchWork w{};
    load_slot(w, slot, traces);
    w.dual_pivots = (int64_t)slot.staged_out;
    bind(w, home, layout_of((uint32_t)slot.all_arcs, (uint32_t)slot.n + 1u));
    if (attempt == 1) mcf::batch_reprice(w, 0, 1);
    mcf::batch_run_after_dual(w, 0, 1, INT64_MAX);
    store_slot(slot, w);
    slot.staged_out = (uint64_t)w.dual_pivots;
    slot.reprice = attempt == 2 ? 2 : 0;
}

// the host hooks: the steps and the pivots with one lane, on a host slab of the device's layout
template <class P>
int solve_on_host(typename P::Handle *b, BatchIo io, Call call, const char *what)
{
    const bool resolve = is_resolve(call);
    if (const int rc = check_call<P>(b, io, what, true, call)) return rc;
    const double t_start = mcf::now_ns();
    const size_t count = (size_t)b->d.count;
    b->h_slab.resize(P::slab_bytes(b));
    b->h_slots.resize(count);
    b->h_traces.resize(std::max<size_t>(count * (size_t)b->d.trace_capacity, 1));
    if (resolve)                                                            // the last solve was the device's: its state comes down whole
        if (const int rc = state_to_host(b, b->d.device, count)) return rc;
    b->stats = mcf_ubatch_stats{};
    b->stats.instances = (int64_t)count;
    b->stats.workspace_bytes = (int64_t)b->h_slab.size();
    if (!resolve) io.changed = nullptr;
    const typename P::Problem p = P::problem(b, io, false);
    const mcf::UniformOutputs o = outputs_of(io);
    RedataCount redata;
    for (size_t i = 0; i < count; ++i) {
        BatchSlot &slot = b->h_slots[i];
        if (io.changed && !io.changed[i]) { redata.begun(slot, false); continue; }
        int32_t t = 0;
        const mcf::InstanceView v = mcf::view_of(p, &o, (int64_t)i, b->h_slab.data(), &t);
        const BatchSlot &tmpl = P::templates(b)[t];
        if (call == kFresh) mcf::uniform_begin(v, tmpl, slot, 0, 1);
        else if (call == kRecost) mcf::uniform_recost(v, tmpl, slot, 0, 1);
        else if (call == kRedata) mcf::uniform_redata(v, tmpl, slot, 0, 1);
        else mcf::uniform_begin_from(v, tmpl, slot, 0, 1);
        redata.begun(slot, true);
        const bool ran = slot.run == mcf::kBatchRunning || slot.run == mcf::kBatchDual;
        if (ran) {
            run_slot_on_host(slot, v.home, b->h_traces.data());
            redata.ran(slot);
            if (slot.reprice == 2) {                                        // a warm attempt: judged, and run again cold where it did not stand
                mcf::uniform_redata_settle(v, tmpl, slot, 0, 1);
                if (slot.run == mcf::kBatchRunning) {
                    redata.st.fallback_instances++;
                    run_slot_on_host(slot, v.home, b->h_traces.data());
                    redata.ran(slot);
                }
            }
            b->stats.total_pivots += slot.pivots;
        }
        mcf::uniform_finish(v, o, slot, b->h_traces.data(), 0, 1);
    }
    b->where = PlacedBatch::kOnHost;
    b->supply_type = io.supply_type;
    b->stats.host_ns = mcf::now_ns() - t_start;
    redata.record(call, b);
    return MCF_OK;
}

// ---- mcf_*batch_validate / _validate_on_host: uniform_validate for every instance; independent of the solve state
template <class P>
int validate_on_device(typename P::Handle *b, BatchIo io, mcf_ubatch_check_summary *out, const char *what)
{
    if (!out) return mcf::fail(MCF_ERR_INVALID, "%s: null argument", what);
    if (const int rc = check_call<P>(b, io, what, false, kFresh)) return rc;
    if (const int rc = have_device(b->d.device, what)) return rc;
    *out = mcf_ubatch_check_summary{};
    out->first_invalid = -1;
    const size_t count = (size_t)b->d.count;
    if (!count) return MCF_OK;
    const DeviceGuard guard;
    HIP_TRY(hipSetDevice(b->d.device));
    if (const int rc = ensure_tables<P>(b)) return rc;
    Staged staged;                                                          // MCF_MEM_HOST: the arrays go through the staging buffer of the solve calls
    if (const int rc = stage_up<P>(b, &io, &staged, &out->bytes_up)) return rc;
    int64_t words[2] = {0, INT64_MAX};
    HIP_TRY(hipMemcpy(b->d_summary, words, sizeof(words), hipMemcpyHostToDevice));
    out->bytes_up += (int64_t)sizeof(words);
    const double t_launch = mcf::now_ns();
    hipLaunchKernelGGL(validate_kernel<typename P::Problem>, dim3((unsigned)count), dim3(kBatchThreads), 0, 0, P::problem(b, io, true), check_of(io, b->d_summary), io.flows,
                       io.potentials);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    out->kernel_ns = mcf::now_ns() - t_launch;
    HIP_TRY(hipMemcpy(words, b->d_summary, sizeof(words), hipMemcpyDeviceToHost));
    out->bytes_down += (int64_t)sizeof(words);
    if (const int rc = stage_down(b, staged, &out->bytes_down)) return rc;
    summary_of(words, (int64_t)count, out);
    return MCF_OK;
}

template <class P>
int validate_on_host(typename P::Handle *b, const BatchIo &io, mcf_ubatch_check_summary *out, const char *what)
{
    if (!out) return mcf::fail(MCF_ERR_INVALID, "%s: null argument", what);
    if (const int rc = check_call<P>(b, io, what, true, kFresh)) return rc;
    *out = mcf_ubatch_check_summary{};
    int64_t words[2] = {0, INT64_MAX};
    const typename P::Problem p = P::problem(b, io, false);
    const mcf::UniformCheck c = check_of(io, words);
    const double t_start = mcf::now_ns();
    for (int64_t i = 0; i < (int64_t)b->d.count; ++i) mcf::uniform_validate(mcf::check_view_of(p, io.flows, io.potentials, i), c, 0, 1);
    out->kernel_ns = mcf::now_ns() - t_start;
    summary_of(words, (int64_t)b->d.count, out);
    return MCF_OK;
}

// ---- mcf_*batch_cost_ranges, _data_ranges, _diagnose, _rays and their _on_host hooks: query Q's step for every instance, on the state the last
// solve call left; the state is only read.  What every such call refuses before it touches the handle, in this order:
template <class P, class Q>
int check_query_call(const typename P::Handle *b, typename Q::Io *io, const char *what, bool host_only)
{
    if (!b || !io->given) return mcf::fail(MCF_ERR_INVALID, "%s: null argument", what);
    if (io->memory != MCF_MEM_HOST && io->memory != MCF_MEM_DEVICE) return mcf::fail(MCF_ERR_INVALID, "%s: unknown memory kind %d", what, io->memory);
    if (host_only && io->memory != MCF_MEM_HOST) return mcf::fail(MCF_ERR_INVALID, "%s: the host hooks read and write host memory (MCF_MEM_HOST)", what);
    if (const int rc = Q::template check<P>(b, io, what)) return rc;
    if (b->where == PlacedBatch::kNowhere) return mcf::fail(MCF_ERR_STATE, "%s: the batch has not been solved", what);
    return MCF_OK;
}

// the instances by tier and, in the LDS tier, by the class of what query Q keeps there (Q::footprint(n, m), never more than the solve's);
// the table goes up once per handle and query (again only if the device's LDS limit were another).  An instance is queried in LDS
// exactly when it is solved there.
template <class P, class Q>
int ensure_query_plan(typename P::Handle *b, PlacedBatch::QueryPlan &qp)
{
    if (qp.d_ids && qp.lds_max == b->lds_max) return MCF_OK;
    const size_t count = (size_t)b->d.count;
    const LaunchPlan plan = P::plan(b);
    std::vector<int32_t> group[kClasses];
    std::vector<uint32_t> bytes(count);
    for (size_t i = 0; i < count; ++i) {
        int32_t n = 0, m = 0;
        P::sizes(b, i, &n, &m);
        bytes[i] = Q::footprint(n, m);                                      // no more than plan.bytes(i)
        const bool in_lds = class_of(b->lds_max, plan.bytes((int32_t)i)) != kClasses - 1;
        group[in_lds ? class_of(b->lds_max, bytes[i]) : kClasses - 1].push_back((int32_t)i);
    }
    std::vector<int32_t> ids;
    qp.launches.clear();
    for (int g = 0; g < kClasses; ++g) {
        if (group[g].empty()) continue;
        PlacedBatch::QueryLaunch L{(int)ids.size(), (int)group[g].size(), 0, g != kClasses - 1};
        for (int32_t i : group[g]) {
            ids.push_back(i);
            if (L.in_lds) L.lds = std::max(L.lds, bytes[(size_t)i]);
        }
        qp.launches.push_back(L);
    }
    if (!qp.d_ids) HIP_TRY(hipMalloc((void **)&qp.d_ids, count * sizeof(int32_t)));
    HIP_TRY(hipMemcpy(qp.d_ids, ids.data(), count * sizeof(int32_t), hipMemcpyHostToDevice));
    qp.lds_max = b->lds_max;
    return MCF_OK;
}

// The global tier's room for the working arrays of a diagnosis or a rays call: per block what the largest instance of that tier needs
// (Q::room(n + 1)), 0 when the plan has no such launch or the query keeps no such arrays; the buffer is the handle's one and only grows.
template <class P, class Q>
int prepare_work(typename P::Handle *b, const PlacedBatch::QueryPlan &plan)
{
    b->diag_work_stride = 0;
    for (const PlacedBatch::QueryLaunch &L : plan.launches) {
        if (L.in_lds) continue;
        const LaunchPlan solve = P::plan(b);
        uint32_t most = 0;
        for (size_t i = 0; i < (size_t)b->d.count; ++i) {
            if (class_of(b->lds_max, solve.bytes((int32_t)i)) != kClasses - 1) continue;
            int32_t n = 0, m = 0;
            P::sizes(b, i, &n, &m);
            most = std::max(most, Q::room((uint32_t)n + 1u));
        }
        b->diag_work_stride = most;
        const size_t need = (size_t)L.n * (size_t)most;
        if (b->diag_work_bytes < need) {
            if (b->d_diag_work) { HIP_TRY(hipFree(b->d_diag_work)); b->d_diag_work = nullptr; b->diag_work_bytes = 0; }
            HIP_TRY(hipMalloc((void **)&b->d_diag_work, need));
            b->diag_work_bytes = need;
        }
    }
    return MCF_OK;
}

// the problem of a query: the placement's tables where the step runs and the last solve call's supply type (the kept flow belongs to
// that one); no rows of the caller's
template <class P>
typename P::Problem kept_problem(const typename P::Handle *b, bool on_device)
{
    BatchIo kept{};
    kept.supply_type = b->supply_type;
    return P::problem(b, kept, on_device);
}

template <class P, class Q>
int query_on_device(typename P::Handle *b, typename Q::Io io, const char *what)
{
    if (const int rc = check_query_call<P, Q>(b, &io, what, false)) return rc;
    if (const int rc = have_device(b->d.device, what)) return rc;          // the handle is as it was
    const DeviceGuard guard;
    if (const int rc = open_device(b->d.device, &b->lds_max)) return rc;
    const size_t count = (size_t)b->d.count;
    PlacedBatch::Query<typename Q::Stats> &query = Q::state(b);
    typename Q::Stats st{};
    st.instances = (int64_t)count;
    if (!count) { query.stats = st; return MCF_OK; }
    if (const int rc = ensure_device_buffers<P>(b)) return rc;
    const bool first = !query.plan.d_ids;
    if (const int rc = ensure_query_plan<P, Q>(b, query.plan)) return rc;
    if (first) st.bytes_up += (int64_t)(count * sizeof(int32_t));
    if (!b->d_query_summary) HIP_TRY(hipMalloc((void **)&b->d_query_summary, kQuerySummaryWords * sizeof(int64_t)));
    if (const int rc = prepare_work<P, Q>(b, query.plan)) return rc;
    if (const int rc = state_to_device(b, count, &st.bytes_up)) return rc;
    b->where = PlacedBatch::kOnDevice;                                      // the same state, now there too
    Staged staged;                                                          // MCF_MEM_HOST: the arrays go through the staging buffer of the solve calls
    if (io.memory == MCF_MEM_HOST) {
        const auto arrays = Q::template arrays<P>(b, &io);
        if (const int rc = stage_arrays(b, arrays.data(), arrays.size(), 16, &staged, &st.bytes_up)) return rc;
    }
    int64_t words[Q::kWords] = {};
    HIP_TRY(hipMemcpy(b->d_query_summary, words, sizeof(words), hipMemcpyHostToDevice));
    st.bytes_up += (int64_t)sizeof(words);
    const typename P::Problem p = kept_problem<P>(b, true);
    const typename Q::Outputs o = Q::outputs(io, b->d_query_summary);
    const mcf::PairArgs pairs = Q::pairs(io);
    const auto in_lds = query_kernel<typename P::Problem, Q, true>, in_place = query_kernel<typename P::Problem, Q, false>;
    unsigned char *const work = b->diag_work_stride ? b->d_diag_work : nullptr;        // a stride of 0: no block works there in this call
    bool opted_in = false;
    const double t_launch = mcf::now_ns();
    for (const PlacedBatch::QueryLaunch &L : query.plan.launches) {
        if (L.in_lds && !opted_in && b->lds_max > (64 << 10)) {             // the opt-in open_device got for the solve's kernels
            HIP_TRY(hipFuncSetAttribute((const void *)in_lds, hipFuncAttributeMaxDynamicSharedMemorySize, b->lds_max));
            opted_in = true;
        }
        hipLaunchKernelGGL(L.in_lds ? in_lds : in_place, dim3((unsigned)L.n), dim3(kBatchThreads), L.lds, 0, p, o, pairs, b->dev.slots, b->dev.slab,
                           query.plan.d_ids + L.first, work, b->diag_work_stride);
        HIP_TRY(hipGetLastError());
        (L.in_lds ? st.lds_instances : st.global_instances) += L.n;
    }
    HIP_TRY(hipDeviceSynchronize());
    st.kernel_ns = mcf::now_ns() - t_launch;
    HIP_TRY(hipMemcpy(words, b->d_query_summary, sizeof(words), hipMemcpyDeviceToHost));
    st.bytes_down += (int64_t)sizeof(words);
    if (const int rc = stage_down(b, staged, &st.bytes_down)) return rc;
    Q::stats_of(words, &st);
    query.stats = st;                                                       // only a call that succeeded replaces the last one's
    return MCF_OK;
}

template <class P, class Q>
int query_on_host(typename P::Handle *b, typename Q::Io io, const char *what)
{
    if (const int rc = check_query_call<P, Q>(b, &io, what, true)) return rc;
    const size_t count = (size_t)b->d.count;
    b->h_slab.resize(P::slab_bytes(b));
    b->h_slots.resize(count);
    if (const int rc = state_to_host(b, b->d.device, count)) return rc;
    b->where = PlacedBatch::kOnHost;                                        // the same state, now here too
    typename Q::Stats st{};
    st.instances = (int64_t)count;
    int64_t words[Q::kWords] = {};
    const typename Q::Outputs o = Q::outputs(io, words);
    const typename P::Problem p = kept_problem<P>(b, false);
    const mcf::PairArgs pairs = Q::pairs(io);
    struct alignas(16) Word { uint64_t lo, hi; };
    std::vector<Word> room;                                                 // one instance's working arrays at a time (Q::room), as the layouts align them
    const double t_start = mcf::now_ns();
    for (size_t i = 0; i < count; ++i) {
        const mcf::InstanceView v = mcf::view_of(p, nullptr, (int64_t)i, b->h_slab.data(), nullptr);
        const size_t words_needed = Q::room((uint32_t)v.n + 1u) / sizeof(Word);
        if (room.size() < words_needed) room.resize(words_needed);
        Q::template step<false>(v, o, mcf::pairs_of(p, pairs, (int64_t)i), b->h_slots[i], (unsigned char *)room.data(), 0, 1);
    }
    st.kernel_ns = mcf::now_ns() - t_start;
    Q::stats_of(words, &st);
    Q::state(b).stats = st;
    return MCF_OK;
}

// mcf_*batch_get_*stats: the handle's member that holds them -- the statistics themselves, or a query's state with them
template <class Stats, class Held>
int get_stats(const PlacedBatch *b, Stats *out, Held PlacedBatch::*member)
{
    if (!b || !out) return mcf::fail(MCF_ERR_INVALID, "null argument");
    *out = b->*member;
    return MCF_OK;
}

}  // namespace

extern "C" {

int mcf_ubatch_create(mcf_ubatch **out, const mcf_ubatch_desc *desc)
{
    if (!out || !desc) return mcf::fail(MCF_ERR_INVALID, "mcf_ubatch_create: null argument");
    *out = nullptr;
    if (const int rc = check_batch_desc(*desc, "mcf_ubatch_create")) return rc;
    if (desc->count < 0) return mcf::fail(MCF_ERR_INVALID, "mcf_ubatch_create: negative instance count");
    if (desc->arc_count > MCF_BATCH_MAX_ARCS || desc->node_count > MCF_BATCH_MAX_NODES)
        return mcf::fail(MCF_ERR_INVALID, "mcf_ubatch_create: %d nodes / %d arcs is above the batch solver's limit of %d / %d per instance; solve it with mcf_ns_solve",
                         desc->node_count, desc->arc_count, MCF_BATCH_MAX_NODES, MCF_BATCH_MAX_ARCS);
    if (desc->count > MCF_BATCH_MAX_INSTANCES) return mcf::fail(MCF_ERR_INVALID, "mcf_ubatch_create: a batch holds at most %d instances", MCF_BATCH_MAX_INSTANCES);
    mcf::NsCore checked;                                                    // end points, as mcf_batch_add validates them
    if (const int rc = mcf::core_create(&checked, desc->node_count, desc->arc_count, desc->source, desc->target)) return rc;
    mcf_ubatch *b = new mcf_ubatch();
    b->d = *desc;
    b->d.semantics = MCF_SEM_PLAIN;                                         // 0 means the same
    b->source.assign(desc->source, desc->source + desc->arc_count);
    b->target.assign(desc->target, desc->target + desc->arc_count);
    b->d.source = b->d.target = nullptr;                                    // the caller's arrays are not kept
    if (const int rc = configure_slot(b->tmpl, limits_of(b->d), desc->node_count, desc->arc_count, b->source.data(), b->target.data())) { delete b; return rc; }
    b->stride = layout_of((uint32_t)(desc->arc_count + 2 * desc->node_count), (uint32_t)desc->node_count + 1u).bytes;
    b->inc_start.resize((size_t)desc->node_count + 1);
    b->inc.resize(2 * (size_t)desc->arc_count);
    build_incidence((size_t)desc->node_count, (size_t)desc->arc_count, b->source.data(), b->target.data(), b->inc_start.data(), b->inc.data());
    *out = b;
    return MCF_OK;
}

int mcf_rbatch_create(mcf_rbatch **out, const mcf_rbatch_desc *desc)
{
    const char *const who = "mcf_rbatch_create";
    if (!out || !desc) return mcf::fail(MCF_ERR_INVALID, "%s: null argument", who);
    *out = nullptr;
    if (const int rc = check_batch_desc(*desc, who)) return rc;
    if (desc->graph_count < 0 || desc->count < 0) return mcf::fail(MCF_ERR_INVALID, "%s: negative graph or instance count", who);
    if (desc->count > MCF_BATCH_MAX_INSTANCES) return mcf::fail(MCF_ERR_INVALID, "%s: a batch holds at most %d instances", who, MCF_BATCH_MAX_INSTANCES);
    const size_t G = (size_t)desc->graph_count, count = (size_t)desc->count;
    if (G && (!desc->node_count || !desc->arc_start)) return mcf::fail(MCF_ERR_INVALID, "%s: null node_count or arc_start", who);
    if (!desc->graph_of && count != G)
        return mcf::fail(MCF_ERR_INVALID, "%s: without graph_of instance i is graph i, so count (%d) must equal graph_count (%d)", who, desc->count, desc->graph_count);
    for (size_t i = 0; desc->graph_of && i < count; ++i)
        if (desc->graph_of[i] < 0 || (size_t)desc->graph_of[i] >= G)
            return mcf::fail(MCF_ERR_INVALID, "%s: graph_of[%zu] = %d is not one of the %d graphs", who, i, desc->graph_of[i], desc->graph_count);
    const int64_t first_arc = G ? desc->arc_start[0] : 0;
    if (first_arc < 0) return mcf::fail(MCF_ERR_INVALID, "%s: arc_start[0] is negative", who);
    for (size_t g = 0; g < G; ++g) {
        const int64_t m = desc->arc_start[g + 1] - desc->arc_start[g];
        if (m < 0) return mcf::fail(MCF_ERR_INVALID, "%s: arc_start is not monotone at graph %zu", who, g);
        if (m > MCF_BATCH_MAX_ARCS || desc->node_count[g] > MCF_BATCH_MAX_NODES)
            return mcf::fail(MCF_ERR_INVALID, "%s: graph %zu: %d nodes / %lld arcs is above the batch solver's limit of %d / %d per instance; solve it with mcf_ns_solve",
                             who, g, desc->node_count[g], (long long)m, MCF_BATCH_MAX_NODES, MCF_BATCH_MAX_ARCS);
    }
    mcf_rbatch *b = new mcf_rbatch();
    b->d = *desc;
    b->d.semantics = MCF_SEM_PLAIN;                                         // 0 means the same
    const size_t arcs = G ? (size_t)(desc->arc_start[G] - first_arc) : 0;
    if (arcs && (!desc->source || !desc->target)) { delete b; return mcf::fail(MCF_ERR_INVALID, "%s: null source or target", who); }
    if (arcs) {
        b->source.assign(desc->source + first_arc, desc->source + first_arc + arcs);
        b->target.assign(desc->target + first_arc, desc->target + first_arc + arcs);
    }
    b->graphs.resize(G);
    b->tmpl.resize(G);
    size_t nodes = 0;
    for (size_t g = 0; g < G; ++g) {                                        // the records; node_count is checked below, by core_create
        mcf::RaggedGraph &rec = b->graphs[g];
        rec.n = desc->node_count[g]; rec.m = (int32_t)(desc->arc_start[g + 1] - desc->arc_start[g]); rec.tmpl = (int32_t)g; rec.reserved = 0;
        rec.ends = desc->arc_start[g] - first_arc; rec.inc_start = (int64_t)(nodes + g); rec.inc = 2 * rec.ends;
        nodes += (size_t)std::max(rec.n, 0);
    }
    b->inc_start.resize(nodes + G);
    b->inc.resize(2 * arcs);
    for (size_t g = 0; g < G; ++g) {
        const mcf::RaggedGraph &rec = b->graphs[g];
        const int32_t *const src = b->source.data() + rec.ends, *const tgt = b->target.data() + rec.ends;
        mcf::NsCore checked;                                                // end points, as mcf_batch_add validates them
        if (const int rc = mcf::core_create(&checked, rec.n, rec.m, src, tgt)) { delete b; return rc; }
        if (const int rc = configure_slot(b->tmpl[g], limits_of(b->d), rec.n, rec.m, src, tgt)) { delete b; return rc; }
        build_incidence((size_t)rec.n, (size_t)rec.m, src, tgt, b->inc_start.data() + rec.inc_start, b->inc.data() + rec.inc);
    }
    b->graph_of.resize(count);
    for (size_t i = 0; i < count; ++i) b->graph_of[i] = desc->graph_of ? desc->graph_of[i] : (int32_t)i;
    // rows and workspaces: running sums.  Every footprint is a multiple of 16 (layout_of), so every workspace starts on a 16-byte boundary
    b->arc_row.assign(count + 1, 0); b->node_row.assign(count + 1, 0); b->workspace.assign(count + 1, 0);
    b->footprint.resize(count);
    for (size_t i = 0; i < count; ++i) {
        const mcf::RaggedGraph &rec = b->graphs[(size_t)b->graph_of[i]];
        b->footprint[i] = layout_of((uint32_t)(rec.m + 2 * rec.n), (uint32_t)rec.n + 1u).bytes;
        b->arc_row[i + 1] = b->arc_row[i] + rec.m;
        b->node_row[i + 1] = b->node_row[i] + rec.n;
        b->workspace[i + 1] = b->workspace[i] + b->footprint[i];
    }
    b->d.node_count = nullptr; b->d.arc_start = nullptr; b->d.source = b->d.target = nullptr; b->d.graph_of = nullptr;     // the caller's arrays are not kept
    *out = b;
    return MCF_OK;
}

int mcf_rbatch_get_rows(mcf_rbatch *b, int64_t *arc_row, int64_t *node_row)
{
    if (!b) return mcf::fail(MCF_ERR_INVALID, "null argument");
    if (arc_row) std::copy(b->arc_row.begin(), b->arc_row.end(), arc_row);
    if (node_row) std::copy(b->node_row.begin(), b->node_row.end(), node_row);
    return MCF_OK;
}

void mcf_ubatch_destroy(mcf_ubatch *b) { delete b; }
int mcf_ubatch_solve(mcf_ubatch *b, const mcf_ubatch_io *io) { return solve_on_device<UniformPlacement>(b, io_of(io), kFresh, "mcf_ubatch_solve"); }
int mcf_ubatch_resolve(mcf_ubatch *b, const mcf_ubatch_io *io) { return solve_on_device<UniformPlacement>(b, io_of(io), kRecost, "mcf_ubatch_resolve"); }
int mcf_ubatch_resolve_data(mcf_ubatch *b, const mcf_ubatch_io *io) { return solve_on_device<UniformPlacement>(b, io_of(io), kRedata, "mcf_ubatch_resolve_data"); }
int mcf_ubatch_run_on_host(mcf_ubatch *b, const mcf_ubatch_io *io) { return solve_on_host<UniformPlacement>(b, io_of(io), kFresh, "mcf_ubatch_run_on_host"); }
int mcf_ubatch_rerun_on_host(mcf_ubatch *b, const mcf_ubatch_io *io) { return solve_on_host<UniformPlacement>(b, io_of(io), kRecost, "mcf_ubatch_rerun_on_host"); }
int mcf_ubatch_rerun_data_on_host(mcf_ubatch *b, const mcf_ubatch_io *io) { return solve_on_host<UniformPlacement>(b, io_of(io), kRedata, "mcf_ubatch_rerun_data_on_host"); }
int mcf_ubatch_validate(mcf_ubatch *b, const mcf_ubatch_check_io *io, mcf_ubatch_check_summary *out)
{
    return validate_on_device<UniformPlacement>(b, io_of(io), out, "mcf_ubatch_validate");
}
int mcf_ubatch_validate_on_host(mcf_ubatch *b, const mcf_ubatch_check_io *io, mcf_ubatch_check_summary *out)
{
    return validate_on_host<UniformPlacement>(b, io_of(io), out, "mcf_ubatch_validate_on_host");
}
int mcf_ubatch_get_stats(mcf_ubatch *b, mcf_ubatch_stats *out) { return get_stats(b, out, &PlacedBatch::stats); }
int mcf_ubatch_get_redata_stats(mcf_ubatch *b, mcf_ubatch_redata_stats *out) { return get_stats(b, out, &PlacedBatch::redata_stats); }
int mcf_ubatch_solve_from(mcf_ubatch *b, const mcf_ubatch_io *io, const mcf_ubatch_basis_io *basis)
{
    return solve_on_device<UniformPlacement>(b, with_basis(io_of(io), basis), kStart, "mcf_ubatch_solve_from");
}
int mcf_ubatch_run_from_on_host(mcf_ubatch *b, const mcf_ubatch_io *io, const mcf_ubatch_basis_io *basis)
{
    return solve_on_host<UniformPlacement>(b, with_basis(io_of(io), basis), kStart, "mcf_ubatch_run_from_on_host");
}
int mcf_ubatch_get_start_stats(mcf_ubatch *b, mcf_ubatch_start_stats *out) { return get_stats(b, out, &PlacedBatch::start_stats); }
int mcf_ubatch_cost_ranges(mcf_ubatch *b, const mcf_ubatch_range_io *io) { return query_on_device<UniformPlacement, CostRanges>(b, CostRanges::io_of(io), "mcf_ubatch_cost_ranges"); }
int mcf_ubatch_cost_ranges_on_host(mcf_ubatch *b, const mcf_ubatch_range_io *io) { return query_on_host<UniformPlacement, CostRanges>(b, CostRanges::io_of(io), "mcf_ubatch_cost_ranges_on_host"); }
int mcf_ubatch_get_range_stats(mcf_ubatch *b, mcf_ubatch_range_stats *out) { return get_stats(b, out, &PlacedBatch::cost_ranges); }
int mcf_ubatch_data_ranges(mcf_ubatch *b, const mcf_ubatch_data_range_io *io) { return query_on_device<UniformPlacement, DataRanges>(b, DataRanges::io_of(io), "mcf_ubatch_data_ranges"); }
int mcf_ubatch_data_ranges_on_host(mcf_ubatch *b, const mcf_ubatch_data_range_io *io) { return query_on_host<UniformPlacement, DataRanges>(b, DataRanges::io_of(io), "mcf_ubatch_data_ranges_on_host"); }
int mcf_ubatch_get_data_range_stats(mcf_ubatch *b, mcf_ubatch_data_range_stats *out) { return get_stats(b, out, &PlacedBatch::data_ranges); }
int mcf_ubatch_diagnose(mcf_ubatch *b, const mcf_ubatch_diagnose_io *io) { return query_on_device<UniformPlacement, Diagnose>(b, Diagnose::io_of(io), "mcf_ubatch_diagnose"); }
int mcf_ubatch_diagnose_on_host(mcf_ubatch *b, const mcf_ubatch_diagnose_io *io) { return query_on_host<UniformPlacement, Diagnose>(b, Diagnose::io_of(io), "mcf_ubatch_diagnose_on_host"); }
int mcf_ubatch_get_diagnose_stats(mcf_ubatch *b, mcf_ubatch_diagnose_stats *out) { return get_stats(b, out, &PlacedBatch::diagnose); }
int mcf_ubatch_rays(mcf_ubatch *b, const mcf_ubatch_rays_io *io) { return query_on_device<UniformPlacement, Rays>(b, Rays::io_of(io), "mcf_ubatch_rays"); }
int mcf_ubatch_rays_on_host(mcf_ubatch *b, const mcf_ubatch_rays_io *io) { return query_on_host<UniformPlacement, Rays>(b, Rays::io_of(io), "mcf_ubatch_rays_on_host"); }
int mcf_ubatch_get_rays_stats(mcf_ubatch *b, mcf_ubatch_rays_stats *out) { return get_stats(b, out, &PlacedBatch::rays); }

void mcf_rbatch_destroy(mcf_rbatch *b) { delete b; }
int mcf_rbatch_solve(mcf_rbatch *b, const mcf_rbatch_io *io) { return solve_on_device<RaggedPlacement>(b, io_of(io), kFresh, "mcf_rbatch_solve"); }
int mcf_rbatch_resolve(mcf_rbatch *b, const mcf_rbatch_io *io) { return solve_on_device<RaggedPlacement>(b, io_of(io), kRecost, "mcf_rbatch_resolve"); }
int mcf_rbatch_resolve_data(mcf_rbatch *b, const mcf_rbatch_io *io) { return solve_on_device<RaggedPlacement>(b, io_of(io), kRedata, "mcf_rbatch_resolve_data"); }
int mcf_rbatch_run_on_host(mcf_rbatch *b, const mcf_rbatch_io *io) { return solve_on_host<RaggedPlacement>(b, io_of(io), kFresh, "mcf_rbatch_run_on_host"); }
int mcf_rbatch_rerun_on_host(mcf_rbatch *b, const mcf_rbatch_io *io) { return solve_on_host<RaggedPlacement>(b, io_of(io), kRecost, "mcf_rbatch_rerun_on_host"); }
int mcf_rbatch_rerun_data_on_host(mcf_rbatch *b, const mcf_rbatch_io *io) { return solve_on_host<RaggedPlacement>(b, io_of(io), kRedata, "mcf_rbatch_rerun_data_on_host"); }
int mcf_rbatch_validate(mcf_rbatch *b, const mcf_rbatch_check_io *io, mcf_ubatch_check_summary *out)
{
    return validate_on_device<RaggedPlacement>(b, io_of(io), out, "mcf_rbatch_validate");
}
int mcf_rbatch_validate_on_host(mcf_rbatch *b, const mcf_rbatch_check_io *io, mcf_ubatch_check_summary *out)
{
    return validate_on_host<RaggedPlacement>(b, io_of(io), out, "mcf_rbatch_validate_on_host");
}
int mcf_rbatch_get_stats(mcf_rbatch *b, mcf_ubatch_stats *out) { return get_stats(b, out, &PlacedBatch::stats); }
int mcf_rbatch_get_redata_stats(mcf_rbatch *b, mcf_ubatch_redata_stats *out) { return get_stats(b, out, &PlacedBatch::redata_stats); }
int mcf_rbatch_solve_from(mcf_rbatch *b, const mcf_rbatch_io *io, const mcf_rbatch_basis_io *basis)
{
    return solve_on_device<RaggedPlacement>(b, with_basis(io_of(io), basis), kStart, "mcf_rbatch_solve_from");
}
int mcf_rbatch_run_from_on_host(mcf_rbatch *b, const mcf_rbatch_io *io, const mcf_rbatch_basis_io *basis)
{
    return solve_on_host<RaggedPlacement>(b, with_basis(io_of(io), basis), kStart, "mcf_rbatch_run_from_on_host");
}
int mcf_rbatch_get_start_stats(mcf_rbatch *b, mcf_ubatch_start_stats *out) { return get_stats(b, out, &PlacedBatch::start_stats); }
int mcf_rbatch_cost_ranges(mcf_rbatch *b, const mcf_rbatch_range_io *io) { return query_on_device<RaggedPlacement, CostRanges>(b, CostRanges::io_of(io), "mcf_rbatch_cost_ranges"); }
int mcf_rbatch_cost_ranges_on_host(mcf_rbatch *b, const mcf_rbatch_range_io *io) { return query_on_host<RaggedPlacement, CostRanges>(b, CostRanges::io_of(io), "mcf_rbatch_cost_ranges_on_host"); }
int mcf_rbatch_get_range_stats(mcf_rbatch *b, mcf_ubatch_range_stats *out) { return get_stats(b, out, &PlacedBatch::cost_ranges); }
int mcf_rbatch_data_ranges(mcf_rbatch *b, const mcf_rbatch_data_range_io *io) { return query_on_device<RaggedPlacement, DataRanges>(b, DataRanges::io_of(io), "mcf_rbatch_data_ranges"); }
int mcf_rbatch_data_ranges_on_host(mcf_rbatch *b, const mcf_rbatch_data_range_io *io) { return query_on_host<RaggedPlacement, DataRanges>(b, DataRanges::io_of(io), "mcf_rbatch_data_ranges_on_host"); }
int mcf_rbatch_get_data_range_stats(mcf_rbatch *b, mcf_ubatch_data_range_stats *out) { return get_stats(b, out, &PlacedBatch::data_ranges); }
int mcf_rbatch_diagnose(mcf_rbatch *b, const mcf_rbatch_diagnose_io *io) { return query_on_device<RaggedPlacement, Diagnose>(b, Diagnose::io_of(io), "mcf_rbatch_diagnose"); }
int mcf_rbatch_diagnose_on_host(mcf_rbatch *b, const mcf_rbatch_diagnose_io *io) { return query_on_host<RaggedPlacement, Diagnose>(b, Diagnose::io_of(io), "mcf_rbatch_diagnose_on_host"); }
int mcf_rbatch_get_diagnose_stats(mcf_rbatch *b, mcf_ubatch_diagnose_stats *out) { return get_stats(b, out, &PlacedBatch::diagnose); }
int mcf_rbatch_rays(mcf_rbatch *b, const mcf_rbatch_rays_io *io) { return query_on_device<RaggedPlacement, Rays>(b, Rays::io_of(io), "mcf_rbatch_rays"); }
int mcf_rbatch_rays_on_host(mcf_rbatch *b, const mcf_rbatch_rays_io *io) { return query_on_host<RaggedPlacement, Rays>(b, Rays::io_of(io), "mcf_rbatch_rays_on_host"); }
int mcf_rbatch_get_rays_stats(mcf_rbatch *b, mcf_ubatch_rays_stats *out) { return get_stats(b, out, &PlacedBatch::rays); }

}  // extern "C"
