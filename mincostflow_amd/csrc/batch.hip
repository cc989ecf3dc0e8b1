// batch.hip -- mcf_batch_*: many small independent instances, one whole solve per workgroup.
//
// The pivot itself is batch_step.hip.h, shared with the host.  This file is what surrounds it:
//   * per instance an NsCore (ns_core.h): set up by the host with the code mcf_ns uses, finished by it afterwards;
//   * a WORKSPACE per instance in one slab of device memory, the home of its state between launches (layout: Layout below);
//   * batch_kernel: one workgroup of ONE wave per instance.  LDS tier: the workspace is copied into dynamic LDS at entry, the pivots run
//     there, the part that changes is copied back at exit.  Global tier: the pivots run in place on the workspace.  Same step functions;
//   * bounded launches: a launch runs every unfinished instance for at most pivots_per_launch pivots and returns; the host relaunches
//     until every instance is done.  The rule's state and the pivot count travel in the instance's BatchSlot.
// Device code does no bounds checks: mcf_batch_add validates every end point (core_create), and every index the kernel follows after
// that was written by start_basis or by the pivot itself.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "batch_step.hip.h"
#include "common.h"
#include "ns_core.h"

namespace {

#define HIP_TRY(expr)                                                                                      \
    do {                                                                                                   \
        hipError_t err__ = (expr);                                                                         \
        if (err__ != hipSuccess) return mcf::fail(MCF_ERR_HIP, "%s: %s", #expr, hipGetErrorString(err__)); \
    } while (0)

constexpr int kBatchThreads = 64;          // one wave: the sequential and the lane-parallel half alternate without a workgroup of waves to hold
constexpr int kDefaultPivotsPerLaunch = 2048;   // 15 us per pivot in LDS, 35 in place -> launches of 30 - 70 ms

// ---- workspace of one instance: A = all_arcs arcs, N = n + 1 nodes; every array starts on a 16-byte boundary.
//   constant part:  tail[A] i32 | head[A] i32 | cost[A] i64 | upper[A] i64
//   changing part:  flow[A] i64 | pi[N] i64 | par, par_arc, nxt, prv, sub, fin [N] i32 each | scratch[N + 1] i32 | state[A] i8 | par_dir[N] i8
// bytes = 33 A + 37 N + 4 + padding (at most 15 per array)
struct Layout {
    uint32_t tail, head, cost, upper, flow, pi, par, par_arc, nxt, prv, sub, fin, scratch, state, par_dir;
    uint32_t changing;      // = flow: first byte of the part a launch writes back
    uint32_t bytes;
};
__host__ __device__ inline uint32_t up16(uint32_t x) { return (x + 15u) & ~15u; }
__host__ __device__ inline Layout layout_of(uint32_t A, uint32_t N)
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
__host__ __device__ inline void bind(mcf::BatchWork &w, unsigned char *base, const Layout &l)
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
    int32_t pad;
    mcf_block_config cfg;
};

__host__ __device__ inline void load_slot(mcf::BatchWork &w, const BatchSlot &s, int32_t *trace_base)
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
__host__ __device__ inline void store_slot(BatchSlot &s, const mcf::BatchWork &w)
{
    s.next_arc = w.next_arc; s.block_size = w.block_size;
    s.counters[0] = w.counters[0]; s.counters[1] = w.counters[1];
    s.pivots = w.pivots;
    s.run = w.run;
}

// One workgroup = one wave = one instance: ids[blockIdx.x].  kLds: dynamic LDS holds the workspace (the host launches with at least
// layout.bytes of it); otherwise the pivots run on the workspace itself.
template <bool kLds>
__global__ __launch_bounds__(kBatchThreads) void batch_kernel(BatchSlot *slots, const int32_t *ids, unsigned char *slab, int32_t *traces, int32_t budget)
{
    extern __shared__ __align__(16) unsigned char lds[];
    const int lane = (int)threadIdx.x;
    BatchSlot &slot = slots[ids[blockIdx.x]];
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
    mcf::batch_run(w, lane, kBatchThreads, (int64_t)budget);
    __syncthreads();
    if (kLds) {
        const uint4 *src = (const uint4 *)lds;
        uint4 *dst = (uint4 *)home;
        for (uint32_t i = l.changing / 16 + (uint32_t)lane; i < l.bytes / 16; i += kBatchThreads) dst[i] = src[i];
    }
    if (lane == 0) store_slot(slot, w);
}

struct Instance {
    mcf::NsCore core;
    Layout layout{};
    BatchSlot slot{};
    std::vector<int32_t> trace;
    int64_t trace_len = 0;
    bool on_device = false;     // false: infeasible by its bounds, nothing to run
};

}  // namespace

struct mcf_batch {
    mcf_batch_desc d{};
    std::vector<Instance *> inst;
    bool solved = false;
    mcf_batch_stats stats{};
    ~mcf_batch() { for (Instance *i : inst) delete i; }
};

namespace {

// NS.cs:237-270 per instance: the configuration `new NetworkSimplex(g).Solve()` chooses, the constructor's block size, the limits
int prepare_instance(const mcf_batch *b, Instance *in)
{
    mcf::NsCore &c = in->core;
    BatchSlot &s = in->slot;
    s = BatchSlot{};
    in->on_device = mcf::core_begin(&c);
    if (!in->on_device) return MCF_OK;
    int rc = mcf_block_config_auto(&s.cfg, c.n, c.m, c.tail.data(), c.head.data());
    if (rc) return rc;
    s.n = c.n; s.all_arcs = c.all_arcs; s.search_arcs = c.search_arcs; s.rule = b->d.pivot_rule;
    if (s.rule == MCF_RULE_BLOCK_SEARCH) {
        int32_t block = 0, dyn_min = 0;
        rc = mcf_block_initial_size(&s.cfg, c.search_arcs, c.n, &block, &dyn_min);
        if (rc) return rc;
        s.block_size = std::max(1, block);
        s.dyn_min = dyn_min;
    }
    s.pivot_limit = b->d.pivot_limit > 0 ? b->d.pivot_limit : 64 * ((int64_t)c.m + 2 * (int64_t)c.n) + 1024;
    s.max_iter = std::max<int64_t>(1000000, (int64_t)c.n * (int64_t)c.m);      // NS.cs:280
    s.trace_cap = b->d.trace_capacity;
    s.run = mcf::kBatchRunning;
    in->layout = layout_of((uint32_t)c.all_arcs, (uint32_t)c.n + 1u);
    in->trace.assign((size_t)std::max(0, b->d.trace_capacity), 0);
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
void unpack(Instance *in, const unsigned char *base)
{
    mcf::NsCore &c = in->core;
    const Layout &l = in->layout;
    const size_t A = (size_t)c.all_arcs, N = (size_t)c.n + 1;
    memcpy(c.flow.data(), base + l.flow, 8 * A); memcpy(c.pi.data(), base + l.pi, 8 * N);
    memcpy(c.par.data(), base + l.par, 4 * N); memcpy(c.par_arc.data(), base + l.par_arc, 4 * N);
    memcpy(c.nxt.data(), base + l.nxt, 4 * N); memcpy(c.prv.data(), base + l.prv, 4 * N);
    memcpy(c.sub.data(), base + l.sub, 4 * N); memcpy(c.fin.data(), base + l.fin, 4 * N);
    memcpy(c.state.data(), base + l.state, A); memcpy(c.par_dir.data(), base + l.par_dir, N);
}

struct DeviceBuffers {
    unsigned char *slab = nullptr;
    BatchSlot *slots = nullptr;
    int32_t *ids = nullptr, *traces = nullptr;
    ~DeviceBuffers()
    {
        if (slab) (void)hipFree(slab);
        if (slots) (void)hipFree(slots);
        if (ids) (void)hipFree(ids);
        if (traces) (void)hipFree(traces);
    }
};

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
    if (b->solved) return mcf::fail(MCF_ERR_STATE, "a batch is solved once (Solve() is single-shot, NS.cs:649); create a new batch");
    return MCF_OK;
}

}  // namespace

extern "C" {

int mcf_batch_create(mcf_batch **out, const mcf_batch_desc *desc)
{
    if (!out || !desc) return mcf::fail(MCF_ERR_INVALID, "mcf_batch_create: null argument");
    *out = nullptr;
    if (desc->pivot_rule == MCF_RULE_CANDIDATE_LIST || desc->pivot_rule == MCF_RULE_ALTERING_LIST)
        return mcf::fail(MCF_ERR_INVALID, "mcf_batch_create: the list rules (Candidate List, Altering List) are not part of the batch solver; use mcf_ns_set_list_pivot_rule");
    if (desc->pivot_rule != MCF_RULE_FIRST_ELIGIBLE && desc->pivot_rule != MCF_RULE_BEST_ELIGIBLE && desc->pivot_rule != MCF_RULE_BLOCK_SEARCH)
        return mcf::fail(MCF_ERR_INVALID, "mcf_batch_create: unknown pivot rule %d", desc->pivot_rule);
    if (desc->semantics == MCF_SEM_OPTIMIZED)
        return mcf::fail(MCF_ERR_INVALID, "mcf_batch_create: MCF_SEM_OPTIMIZED (BlockSearchPivotOptimized and its vector-width reading) is not part of the batch solver; use mcf_ns_solve");
    if (desc->semantics != 0 && desc->semantics != MCF_SEM_PLAIN) return mcf::fail(MCF_ERR_INVALID, "mcf_batch_create: unknown semantics %d", desc->semantics);
    if (desc->flags & MCF_BATCH_SHARDED) return mcf::fail(MCF_ERR_INVALID, "mcf_batch_create: sharding is not part of the batch solver (a batch runs on one device)");
    if (desc->flags & ~MCF_BATCH_SHARDED) return mcf::fail(MCF_ERR_INVALID, "mcf_batch_create: unknown flags %d", desc->flags);
    if (desc->device < 0 || desc->pivot_limit < 0 || desc->pivots_per_launch < 0 || desc->trace_capacity < 0)
        return mcf::fail(MCF_ERR_INVALID, "mcf_batch_create: negative device, pivot limit, pivots per launch or trace capacity");
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
            mcf::NsCore &c = in->core;
            mcf::BatchWork w{};
            load_slot(w, in->slot, in->trace.data());
            static_cast<mcf::TreeView &>(w) = c.tree();
            w.cost = c.cost.data(); w.state = c.state.data(); w.pi = c.pi.data();
            mcf::batch_run(w, 0, 1, INT64_MAX);
            store_slot(in->slot, w);
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
    int devices = 0;
    if (hipGetDeviceCount(&devices) != hipSuccess || devices < 1) { (void)hipGetLastError(); return mcf::fail(MCF_ERR_NO_DEVICE, "mcf_batch_solve: no HIP device (mcf_batch_run_on_host is a test hook, not a solver)"); }
    if (b->d.device >= devices) return mcf::fail(MCF_ERR_NO_DEVICE, "mcf_batch_solve: device %d of %d", b->d.device, devices);
    const double t_start = mcf::now_ns();
    double kernel_ns = 0;
    b->solved = true;
    HIP_TRY(hipSetDevice(b->d.device));
    // the LDS one workgroup may have: the device's figure, never a constant of ours
    int lds_max = 0, lds_optin = 0;
    HIP_TRY(hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, b->d.device));
    if (hipDeviceGetAttribute(&lds_optin, hipDeviceAttributeSharedMemPerBlockOptin, b->d.device) != hipSuccess) { (void)hipGetLastError(); lds_optin = 0; }
    if (lds_optin > lds_max) lds_max = lds_optin;
    // the opt-in for dynamic LDS above the default limit; where the runtime refuses it, the default limit of 64 KiB holds
    if (hipFuncSetAttribute((const void *)batch_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max) != hipSuccess) {
        (void)hipGetLastError();
        lds_max = std::min(lds_max, 64 << 10);
    }

    // set every instance up; place the workspaces
    const size_t count = b->inst.size();
    std::vector<BatchSlot> slots(count);
    uint64_t slab_bytes = 0, trace_entries = 0;
    for (size_t i = 0; i < count; ++i) {
        Instance *in = b->inst[i];
        if (const int rc = prepare_instance(b, in)) return rc;
        if (in->on_device) {
            in->slot.workspace = slab_bytes; slab_bytes += in->layout.bytes;
            in->slot.trace = trace_entries; trace_entries += (uint64_t)in->slot.trace_cap;
        }
        slots[i] = in->slot;
    }
    // Groups: the LDS tier in classes of the footprint (lds_max / 16, / 8, / 4, / 3, / 2, / 1: the steps at which one more workgroup fits a CU),
    // each launched with the largest footprint it holds, so that no launch sizes every workgroup for the batch's largest; the global tier last.
    const int kClasses = 7;
    const int divisor[kClasses - 1] = {16, 8, 4, 3, 2, 1};
    std::vector<int32_t> group[kClasses];
    for (size_t i = 0; i < count; ++i) {
        const Instance *in = b->inst[i];
        if (!in->on_device) continue;
        int g = kClasses - 1;
        for (int k = 0; k < kClasses - 1; ++k)
            if ((int64_t)in->layout.bytes <= (int64_t)lds_max / divisor[k]) { g = k; break; }
        group[g].push_back((int32_t)i);
        if (g == kClasses - 1) b->stats.global_instances++; else b->stats.lds_instances++;
    }
    b->stats.workspace_bytes = (int64_t)slab_bytes;

    DeviceBuffers dev;
    std::vector<unsigned char> host_slab((size_t)slab_bytes);
    if (slab_bytes) {
        for (const Instance *in : b->inst) if (in->on_device) pack(in, host_slab.data() + in->slot.workspace);
        HIP_TRY(hipMalloc((void **)&dev.slab, (size_t)slab_bytes));
        HIP_TRY(hipMalloc((void **)&dev.slots, count * sizeof(BatchSlot)));
        HIP_TRY(hipMalloc((void **)&dev.ids, count * sizeof(int32_t)));
        HIP_TRY(hipMalloc((void **)&dev.traces, (size_t)std::max<uint64_t>(trace_entries, 1) * sizeof(int32_t)));
        HIP_TRY(hipMemcpy(dev.slab, host_slab.data(), (size_t)slab_bytes, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(dev.slots, slots.data(), count * sizeof(BatchSlot), hipMemcpyHostToDevice));
    }
    const int32_t budget = b->d.pivots_per_launch > 0 ? b->d.pivots_per_launch : kDefaultPivotsPerLaunch;
    // relaunch until nobody is left running; every round ends in a synchronising copy of the slots
    std::vector<int32_t> ids;
    for (;;) {
        ids.clear();
        struct Launch { int first, n; uint32_t lds; bool in_lds; };
        std::vector<Launch> launches;
        for (int g = 0; g < kClasses; ++g) {
            Launch L{(int)ids.size(), 0, 0, g != kClasses - 1};
            for (int32_t i : group[g]) {
                if (slots[(size_t)i].run != mcf::kBatchRunning) continue;
                ids.push_back(i);
                L.n++;
                L.lds = std::max(L.lds, b->inst[(size_t)i]->layout.bytes);
            }
            if (L.n) launches.push_back(L);
        }
        if (launches.empty()) break;
        const double tk = mcf::now_ns();
        HIP_TRY(hipMemcpy(dev.ids, ids.data(), ids.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        for (const Launch &L : launches) {
            if (L.in_lds) {
                hipLaunchKernelGGL(batch_kernel<true>, dim3((unsigned)L.n), dim3(kBatchThreads), L.lds, 0, dev.slots, dev.ids + L.first, dev.slab, dev.traces, budget);
                b->stats.lds_bytes_max = std::max<int64_t>(b->stats.lds_bytes_max, L.lds);
            } else {
                hipLaunchKernelGGL(batch_kernel<false>, dim3((unsigned)L.n), dim3(kBatchThreads), 0, 0, dev.slots, dev.ids + L.first, dev.slab, dev.traces, budget);
            }
            HIP_TRY(hipGetLastError());
            b->stats.launches++;
        }
        HIP_TRY(hipMemcpy(slots.data(), dev.slots, count * sizeof(BatchSlot), hipMemcpyDeviceToHost));     // waits for the launches
        kernel_ns += mcf::now_ns() - tk;
    }
    // the state comes home; the host finishes every instance
    std::vector<int32_t> traces((size_t)trace_entries);
    if (slab_bytes) {
        HIP_TRY(hipMemcpy(host_slab.data(), dev.slab, (size_t)slab_bytes, hipMemcpyDeviceToHost));
        if (trace_entries) HIP_TRY(hipMemcpy(traces.data(), dev.traces, (size_t)trace_entries * sizeof(int32_t), hipMemcpyDeviceToHost));
    }
    int64_t total = 0;
    for (size_t i = 0; i < count; ++i) {
        Instance *in = b->inst[i];
        if (in->on_device) {
            in->slot = slots[i];
            unpack(in, host_slab.data() + in->slot.workspace);
            const int64_t len = std::min<int64_t>(in->slot.pivots, in->slot.trace_cap);
            if (len > 0) std::copy(traces.begin() + (ptrdiff_t)in->slot.trace, traces.begin() + (ptrdiff_t)(in->slot.trace + (uint64_t)len), in->trace.begin());
            total += in->slot.pivots;
        }
        finish_instance(in);
    }
    b->stats.total_pivots = total;
    b->stats.kernel_ns = kernel_ns;
    b->stats.host_ns = mcf::now_ns() - t_start - kernel_ns;
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
