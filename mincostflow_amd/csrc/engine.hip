// engine.hip -- host half of the device engine behind the network-simplex pivot seam (MI355X, gfx950).  Kernels: kernels.hip.h; the resident
// grids' mailbox / posting / collecting: resident_host.hip.h; the exact candidate cache: candidate_cache.hip.h (all three included here).
//
// What the engine does:
//   a1/a2/a3  entering-arc search c = state[e] * (cost[e] + pi[source[e]] - pi[target[e]])   (NS.cs:1351-1352) with an exact,
//             tie-break preserving argmin per rule; every workgroup answers with one 64-byte line in pinned host memory and the
//             host merges the records (no stream synchronisation per pivot)
//   a4        potential update over the moved subtree                                          (NS.cs:1185-1209)
//   a5        the one or two State[] writes of ChangeFlow                                      (NS.cs:1030-1039)
//
// Default mode: ONE resident grid per solve; requests (sequence number, next_arc, block size, the previous pivot's patches as final values)
// are written by the host through the PCIe BAR into a mailbox in fine-grained VRAM, every workgroup applies all patches itself before it
// reads anything, scans the arcs it keeps in registers and answers; for Best Eligible on sparse graphs most searches are answered on the
// host from the last answer's candidate list (candidate_cache.hip.h).  Arcs that fit neither registers nor LDS use the RC layout: reduced
// costs kept per arc, shifted by the moved nodes' arc lists, scanned without gathers by a resident grid of its own or one dispatch per
// search.  Dispatch mode (RCCL-sharded engines, timing flags, no host-writable VRAM, no free resident slot): one scan dispatch per search
// with the patches in its kernel arguments.  See DESIGN.md sections 2 and 3.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <hsa/hsa.h>
#include <hsa/hsa_ext_amd.h>

#include <dlfcn.h>
#include <immintrin.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <vector>

#include "common.h"
#include "candidate_state.h"

#include "kernels.hip.h"
#include "collect.hip.h"

namespace {

#define HIP_TRY(expr)                                                                                      \
    do {                                                                                                   \
        hipError_t err__ = (expr);                                                                         \
        if (err__ != hipSuccess) return mcf::fail(MCF_ERR_HIP, "%s: %s", #expr, hipGetErrorString(err__)); \
    } while (0)

// --- RCCL, bound lazily so that the library loads on machines without it
struct Id128 { char b[128]; };
typedef int (*nccl_get_unique_id_t)(Id128 *);
typedef int (*nccl_comm_init_rank_t)(void **, int, Id128, int);
typedef int (*nccl_all_gather_t)(const void *, void *, size_t, int, void *, hipStream_t);
typedef int (*nccl_comm_destroy_t)(void *);
typedef const char *(*nccl_get_error_string_t)(int);
typedef int (*nccl_comm_count_t)(void *, int *);
struct RcclApi {
    void *lib = nullptr;
    nccl_get_unique_id_t get_unique_id = nullptr;
    nccl_comm_init_rank_t comm_init_rank = nullptr;
    nccl_all_gather_t all_gather = nullptr;
    nccl_comm_destroy_t comm_destroy = nullptr;
    nccl_get_error_string_t error_string = nullptr;
    nccl_comm_count_t comm_count = nullptr;
};
RcclApi *rccl()
{
    static RcclApi api;
    static std::once_flag once;
    std::call_once(once, [] {
        api.lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!api.lib) api.lib = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
        if (api.lib) {
            api.get_unique_id = (nccl_get_unique_id_t)dlsym(api.lib, "ncclGetUniqueId");
            api.comm_init_rank = (nccl_comm_init_rank_t)dlsym(api.lib, "ncclCommInitRank");
            api.all_gather = (nccl_all_gather_t)dlsym(api.lib, "ncclAllGather");
            api.comm_destroy = (nccl_comm_destroy_t)dlsym(api.lib, "ncclCommDestroy");
            api.error_string = (nccl_get_error_string_t)dlsym(api.lib, "ncclGetErrorString");
            api.comm_count = (nccl_comm_count_t)dlsym(api.lib, "ncclCommCount");
        }
    });
    return (api.lib && api.get_unique_id && api.comm_init_rank && api.all_gather) ? &api : nullptr;
}
constexpr int kNcclChar = 0;   // ncclInt8 / ncclChar
constexpr int kStageStates = 4096;   // state patches one staged update carries
constexpr int kScanMaxGrid = 2048;   // workgroups of the dispatched gathering scan at most (desc.scan_workgroups overrides)
constexpr int kRcMaxGrid = 512;      // ... and of the dispatched RC scan

}  // namespace

// ------------------------------------------------------------------------------------------------ engine

struct mcf_engine : CandState {
    mcf_engine_desc d{};
    int begin = 0, end = 0;        // shard [begin, end) of the search arcs
    int count_padded = 0;
    int next_arc = 0, block_size = 0;
    // plain Block Search sizing (NS.cs:1304-1337) and its adaptive rule (NS.cs:1400-1438); inert unless mcf_engine_set_block_config was called
    mcf_block_config cfg{};
    bool cfg_set = false;
    int dyn_min_block = 0, low_hits = 0, high_hits = 0;
    hipStream_t stream = nullptr;
    // The resident grid runs on a stream of its own, of the highest priority, that exists only while the grid does.  HIP multiplexes the
    // streams of one priority over GPU_MAX_HW_QUEUES (4) hardware queues, giving a new stream the least-used one; a queue runs its packets in
    // order and a resident grid never leaves its queue.  With the grid on the engine's ordinary stream, a process that keeps more than a
    // handful of engines (or other streams) alive ends up with a grid and somebody else's work -- another engine's upload, its grid, a
    // collective -- on one queue, and that work waits until the grid leaves.  Streams of another priority have queues of their own, and
    // streams that only exist while their grid runs are never more than the resident slots.
    hipStream_t res_stream = nullptr;
    int32_t *d_src = nullptr, *d_tgt = nullptr;
    void *d_cost = nullptr, *d_pi = nullptr;
    int8_t *d_state = nullptr;
    Slot *h_slots = nullptr, *d_slots = nullptr;    // pinned host memory and its device alias
    Slot *d_dev_slots = nullptr;                    // the same records in device memory (RCCL exchange: they are folded on the device)
    Slot *slots_target = nullptr;                   // where the next dispatch writes its records
    int grid = 0, unroll = 1;
    bool lds_pi = false;           // node_count <= kLdsPiMax: kernels keep the potentials in LDS
    // bucketed layout (Best Eligible, potentials neither in LDS nor next to register-resident arcs, large sparse instances): the arcs are
    // stored stably sorted by target-node range so that one range's potentials (1 MB) stay in every XCD's L2 while the grid sweeps it
    int bucket_nodes = 0;          // nodes per range; 0 = arcs are stored in their own order
    std::vector<int32_t> pos_of;   // local arc -> local position (identity when bucket_nodes == 0: empty)
    int32_t *d_orig = nullptr;     // local position -> global arc id
    // RC layout (kernels.hip.h): reduced costs kept per arc, maintained by scatter from the moved nodes; the scan gathers nothing
    bool rc_mode = false;
    bool rc_lds = false;           // resident RC grid: every workgroup's window of arcs fits LDS
    int rc_window = 0;             // arcs per workgroup in that case
    int64_t *d_rc = nullptr;
    int32_t *d_adj_start = nullptr;
    uint32_t *d_adj = nullptr;     // the shard's arcs at each node: local position, bit 31 = the node is the arc's target
    mcf::hvec<int32_t> h_adj_start;   // host copy of d_adj_start (short lists name their arc lists in the scan's arguments)
    int rc_recompute_above = INT32_MAX;   // RC layout: potential lists longer than this are followed by a full recomputation instead of per-arc shifts
    int rc_list_max = 0;                  // resident RC grid: {node, shift} entries one request may carry (longer lists stop the grid)
    bool pend_shift = false;       // every pending potential is its node's previous value + pend_sigma (mcf_engine_shift_potential)
    int64_t pend_sigma = 0;
    bool no_pireg = false;         // MCF_ENGINE_SHARE_DEVICE: the resident grid gathers the potentials for every request
    int lds_grid = 0;
    uint32_t seq = 0;
    bool uploaded = false;
    // host mirror of pi: patches carry final values
    mcf::hvec<int64_t> pi;
    bool mirror_valid = false;     // mcf_engine_set_potential stops maintaining the mirror; update_potential rebuilds it on demand
    bool ext_pi_pinned = false;        // the bound array is registered with HIP (the device can copy it by itself): mcf_engine_reload_potentials
    const int64_t *d_ext_pi = nullptr; // ... and this is where the device sees it: the resident RC grid copies it itself (cmd 3), no stop
    uint32_t *d_barrier = nullptr;     // counter of that grid's grid-wide barrier
    int32_t *d_node_map = nullptr;     // mcf_engine_renumber_nodes: the permutation on the device (kept between calls)
    bool reload_pi = false;            // the whole bound array is to be copied to the device before the next search (and the RC layout recomputed)
    const int64_t *ext_pi = nullptr;   // mcf_engine_bind_potentials: the caller's own array is read instead of the mirror (no second copy to keep up to date)
    int64_t max_abs_cost = 0;
    // pending patches of the current pivot
    mcf::hvec<int32_t> pend_node, pend_arc, pend_state;
    mcf::hvec<int64_t> pend_val;
    // staging for lists that do not fit the kernel arguments (pinned, read by update_kernel over PCIe)
    struct Staging {
        int32_t *nodes = nullptr, *arcs = nullptr, *states = nullptr;
        int64_t *values = nullptr;
        void *d_nodes = nullptr, *d_arcs = nullptr, *d_states = nullptr, *d_values = nullptr;
        hipEvent_t done = nullptr;
        bool busy = false;
        int cap_nodes = 0;
    } stage[2];
    int stage_next = 0;
    // kernel timing samples
    static constexpr int kEvRing = 64;
    hipEvent_t ev_start[kEvRing]{}, ev_stop[kEvRing]{};
    int ev_head = 0, ev_tail = 0;
    mcf_engine_stats st{};
    // sharding
    void *comm = nullptr;
    int rank = 0, world = 1;
    mcf_candidate *d_cand_local = nullptr, *d_cand_all = nullptr, *h_cand_all = nullptr;
    // the exchange of a RESIDENT engine: 64-byte records {seq, candidate, seq} in pinned host memory that the device sees -- the host writes its
    // own into x_send, ncclAllGather (on a stream of its own: the engine's stream is held by the resident grid) moves them, the host polls
    // x_recv until every rank's record carries this exchange's number.  No copy, no stream synchronisation per pivot.
    struct XRec { uint64_t head; mcf_candidate c; uint64_t pad[2]; uint64_t tail; };
    XRec *x_send = nullptr, *x_recv = nullptr;
    void *d_x_send = nullptr, *d_x_recv = nullptr;
    hipStream_t comm_stream = nullptr;
    uint64_t x_seq = 0;
    bool comm_resident = false;
    // resident mode (flag MCF_ENGINE_RESIDENT): mailbox in BAR-mapped fine-grained VRAM, exit record in pinned host memory
    bool resident_ok = false, resident_running = false, resident_reg = false;
    bool has_slot = false;         // this engine's grid occupies one of the device's resident slots (resident_slot_acquire)
    // the candidate cache's register-resident grid that is patched straight from the request (resident_cand_kernel): the one big subtree of
    // a pivot travels as bare node ids + sigma, the arrays in memory are only read when the grid starts (and written by the host when it stops)
    int shift_reload_min = 0;          // shift grid: nodes from which a walk is announced as a reload of the bound potentials (0 = never)
    bool shift_grid = false;
    uint32_t shift_base = 0;       // dword offset of the shift lines in the mailbox
    int max_shift_lines = 0;
    int cand_tiles = 1;            // register tiles per thread of that grid
    int shift_streamed = 0;        // shift lines of the coming request already in place (cmd 2 posts)
    // host-side phase times are counted in time-stamp-counter ticks (a clock call costs 20+ ns, four of them per search) and scaled to ns
    // in mcf_engine_get_stats against the wall clock since creation
    double wait_ticks = 0, launch_ticks = 0, cal_ns = 0, cal_ticks = 0;
    // a search that has been posted / launched but not collected yet (mcf_engine_search_begin .. _end)
    enum { kNoSearch = 0, kAnswered, kResidentSearch, kCandSearch, kDispatchSearch } in_flight = kNoSearch;
    Key answered{0, kNone, kNone};
    Key range_key{0, kNone, kNone};   // OPTIMIZED Block Search: the range key of the search collected last (kernels.hip.h: kDual)
    int vec = 0;                      // Vector<long>.Count of the reference's host for that rule (0 = not hardware accelerated): desc.vector_width
    bool in_flight_timed = false;
    int stream_lines = 0;          // entry lines of the coming request that an "apply" post has already put in place
    uint32_t stream_sub = 0;       // counter of those posts
    uint32_t *mailbox = nullptr;
    int mailbox_lines = 0, mailbox_max_st = 0;
    uint32_t idle_ticks = 0;       // a resident grid leaves after this long without a request (kResidentIdleTicks; MCF_HIP_IDLE_MS)
    uint32_t prev_seq = 0;
    // candidate cache (Best Eligible, resident, register-resident tiles, sparse graphs): see cand_* below
    bool cand_on = false;                       // (the decision state -- epochs, heap, list, memos -- is the CandState base: candidate_state.h)
    mcf::hvec<int32_t> h_src, h_tgt;            // host mirrors of the resident arrays (search arcs only)
    mcf::hvec<int64_t> h_cost;
    mcf::hvec<int8_t> h_state;
    mcf::hvec<int32_t> adj_start;
    mcf::hvec<AdjEnt> adj;                      // arcs incident to each node, with what a re-evaluation needs next to each other
    mcf::hvec<int32_t> adj_pos;                 // where the two entries of an arc sit in adj (the second is -1 for a self loop): a state write reaches both
    std::vector<int32_t> sync_nodes, sync_arcs;   // changed since the device last heard from us (values are read from the mirrors when the request is built)
    size_t blind_count = 0;                       // the same for big subtrees: node lists taken over wholesale, with their values -- they are the
                                                  // first blind_count entries of pend_node / pend_val already (and may have started travelling)
    // A big list may also come as RUNS of consecutive node ids (mcf_engine_shift_potential_runs: after a relabelling in thread order a subtree
    // is a few hundred runs, not tens of thousands of nodes).  Then blind_runs holds {first, length} pairs, blind_count the nodes they cover, and
    // pend_node has NO entries for them until somebody needs ids (cand_materialise_blind) -- the shift grid takes the pairs as they are.
    std::vector<uint32_t> blind_runs;
    bool blind_lazy = false;
    uint32_t blind_epoch = 0;                     // epoch of the first of those lists
    int blind_sets = 0;                           // lists in there that did not come as the continuation of another one
    bool force_device_search = false;             // mcf_engine_bench_search: every search goes to the device (the cache would answer without one)
    bool cand_appending = false;                  // mcf_engine_append_potential is calling mcf_engine_set_potential
    struct NodeShift { int32_t node; int64_t shift; };
    std::vector<NodeShift> rc_sync;               // RC layout: the small lists' nodes with the shift of their pivot, one entry per occurrence
    bool rc_shift_unknown = false;                // ... unless some change came without its shift (mcf_engine_set_potential): then values travel
    bool call_shift_known = false;                // mcf_engine_shift_potential is calling: every node of the call moves by call_shift
    int64_t call_shift = 0;
    std::vector<CandState::CandKey> cand_records; // a device answer's records as they are read from the slots (cand_collect)
    uint32_t async_at = 0, posted_at = 0;
    int patch_capacity = 0;                       // potential patches one request / one staged update can carry (2 * node_count + 256)
    uint32_t cand_epoch0 = 1;                     // the epoch an upload starts from (MCF_HIP_CAND_EPOCH0: tests start close to the wrap)
    bool cand_debug = false;                      // MCF_HIP_CAND_DEBUG: host-side time breakdown of the candidate cache on stderr
    // where the host's time goes in candidate mode (TSC ticks; printed by mcf_engine_destroy when cand_debug is set)
    double tk_absorb = 0, tk_decide = 0, tk_post = 0, tk_collect = 0, tk_probe = 0;
    int64_t n_sync_posts = 0, n_async_waits = 0, n_gap_pivots = 0, n_list_skip = 0;
    uint32_t *h_exit = nullptr, *d_exit = nullptr;
    int res_grid = 0, res_threads = kResidentThreads;
    hipEvent_t res_start = nullptr, res_stop = nullptr;
    // flush buffer for cold micro-benchmarks
    void *d_flush = nullptr;
    size_t flush_bytes = 0;
    // LEMON's list rules (MCF_RULE_CANDIDATE_LIST / MCF_RULE_ALTERING_LIST): dispatch mode only, searched by mcf_engine_collect_eligible alone.
    // Between two device calls the host answers several searches itself, so several pivots' potential lists queue up: they are merged per
    // node (the later value replaces the earlier one, as applying them in order would), pend_index[u] = where u's entry sits in pend_node
    // (valid when pend_node[pend_index[u]] == u, so no clearing is needed when the list is shipped)
    bool list_rule = false;
    std::vector<int32_t> pend_index;
    CollectTile *d_tiles = nullptr;
    CollectHeader *h_collect_hdr = nullptr, *d_collect_hdr = nullptr;   // pinned host memory and its device alias
    CollectEntry *h_collect = nullptr, *d_collect = nullptr;
    int collect_cap = 0;
};

namespace {
// no big list is pending any more (in either form)
inline void blind_clear(mcf_engine *e)
{
    e->blind_count = 0;
    e->blind_runs.clear();
    e->blind_lazy = false;
}

#include "engine_helpers.hip.h"

bool fits32(int64_t v) { return v >= INT32_MIN && v <= INT32_MAX; }

int drain_events(mcf_engine *e, bool all)
{
    while (e->ev_tail != e->ev_head) {
        const int i = e->ev_tail % mcf_engine::kEvRing;
        if (!all && hipEventQuery(e->ev_stop[i]) != hipSuccess) break;
        HIP_TRY(hipEventSynchronize(e->ev_stop[i]));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, e->ev_start[i], e->ev_stop[i]));
        e->st.timed_scans += 1;
        e->st.timed_scan_ns += (double)ms * 1e6;
        e->ev_tail++;
    }
    return MCF_OK;
}

template <typename T>
void fill_params(mcf_engine *e, ScanParams<T> &p, bool with_patches)
{
    p.src = e->d_src;
    p.tgt = e->d_tgt;
    p.cost = (const T *)e->d_cost;
    p.state = e->d_state;
    p.pi = (T *)e->d_pi;
    p.slots = e->slots_target ? e->slots_target : e->d_slots;
    p.orig = e->bucket_nodes > 0 ? e->d_orig : nullptr;
    p.base = e->begin;
    p.count_padded = e->count_padded;
    p.m_s = e->d.search_arc_num;
    const SearchHeader h = search_header(e);
    p.next_arc = h.next_arc;
    p.block_size = h.block_size;
    p.rstar = h.rstar;
    p.seq = e->seq;
    p.n_pi = 0;
    p.n_st = 0;
    if (with_patches) {
        p.n_pi = (int)e->pend_node.size();
        p.n_st = (int)e->pend_arc.size();
        for (int i = 0; i < p.n_pi; ++i) { p.pi_node[i] = e->pend_node[i]; p.pi_val[i] = (T)e->pend_val[i]; }
        for (int i = 0; i < p.n_st; ++i) { p.st_arc[i] = e->pend_arc[i]; p.st_val[i] = e->pend_state[i]; }
    }
}

void fill_rc_params(mcf_engine *e, RcParams &p, bool with_states)
{
    p.state_ro = e->d_state; p.state = e->d_state; p.rc = e->d_rc; p.slots = e->slots_target ? e->slots_target : e->d_slots;
    p.base = e->begin; p.count_padded = e->count_padded; p.m_s = e->d.search_arc_num;
    const SearchHeader h = search_header(e);
    p.next_arc = h.next_arc;
    p.block_size = h.block_size;
    p.rstar = h.rstar;
    p.seq = e->seq;
    p.n_st = 0;
    p.n_pi = 0;
    p.sigma = 0;
    p.pi = e->d_pi;
    p.adj = e->d_adj;
    p.narrow = e->d.int_width == 32 ? 1 : 0;
    if (with_states) {
        p.n_st = (int)e->pend_arc.size();
        for (int i = 0; i < p.n_st; ++i) { p.st_arc[i] = e->pend_arc[i]; p.st_val[i] = e->pend_state[i]; }
        p.n_pi = (int)e->pend_node.size();           // rc_inline_ok has checked the list
        p.sigma = e->pend_sigma;
        p.prefix[0] = 0;
        for (int i = 0; i < p.n_pi; ++i) {
            const int u = e->pend_node[i];
            p.pi_node[i] = u;
            p.adj_lo[i] = e->h_adj_start[u];
            p.prefix[i + 1] = p.prefix[i] + (e->h_adj_start[u + 1] - e->h_adj_start[u]);
        }
    }
}

// a pending potential list short enough to ride in the scan's arguments (RC layout): one common shift, few nodes, short arc lists
bool rc_inline_ok(const mcf_engine *e)
{
    const size_t n = e->pend_node.size();
    if (n == 0) return true;
    if (!e->pend_shift || n > (size_t)kRcInlineNodes) return false;
    int64_t entries = 0;
    for (size_t i = 0; i < n; ++i) entries += e->h_adj_start[e->pend_node[i] + 1] - e->h_adj_start[e->pend_node[i]];
    return entries <= kRcInlineEntries;
}

// one dispatch of the search kernel that the engine's layout, rule and width select, timed by the two events when they are given
void dispatch_search(mcf_engine *e, bool with_patches, hipEvent_t start, hipEvent_t stop)
{
    with_rule(e, [&](auto rule, auto opt) {
        constexpr int RULE = decltype(rule)::value;
        constexpr bool OPT = decltype(opt)::value;
        const dim3 grid(e->grid), block(kThreads);
        if (e->rc_mode) {
            RcParams p;
            fill_rc_params(e, p, with_patches);
            if (e->unroll == 2) launch(scan_rc_kernel<RULE, OPT, 2>, grid, block, e->stream, start, stop, p);
            else launch(scan_rc_kernel<RULE, OPT, 1>, grid, block, e->stream, start, stop, p);
            return;
        }
        with_width(e, [&](auto width) {
            using T = decltype(width);
            ScanParams<T> p;
            fill_params(e, p, with_patches);
            if (e->lds_pi) {
                if (e->unroll >= 2) launch(scan_kernel_lds<T, RULE, OPT, 2>, grid, dim3(kResidentThreads), e->stream, start, stop, p, e->d.node_count);
                else launch(scan_kernel_lds<T, RULE, OPT, 1>, grid, dim3(kResidentThreads), e->stream, start, stop, p, e->d.node_count);
                return;
            }
            if constexpr (RULE == MCF_RULE_BEST_ELIGIBLE) {
                if (e->bucket_nodes > 0) {
                    if (e->unroll == 2) launch(scan_kernel<T, RULE, OPT, 2, true>, grid, block, e->stream, start, stop, p);
                    else launch(scan_kernel<T, RULE, OPT, 1, true>, grid, block, e->stream, start, stop, p);
                    return;
                }
            }
            if (e->unroll == 2) launch(scan_kernel<T, RULE, OPT, 2>, grid, block, e->stream, start, stop, p);
            else launch(scan_kernel<T, RULE, OPT, 1>, grid, block, e->stream, start, stop, p);
        });
    });
}

// a search's dispatch; timed: its duration is sampled through the event ring (drain_events)
int launch_search(mcf_engine *e, bool with_patches, bool timed)
{
    hipEvent_t start = nullptr, stop = nullptr;
    if (timed) {
        if (e->ev_head - e->ev_tail >= mcf_engine::kEvRing) { int rc = drain_events(e, true); if (rc) return rc; }
        const int i = e->ev_head % mcf_engine::kEvRing;
        start = e->ev_start[i];
        stop = e->ev_stop[i];
        e->ev_head++;
    }
    dispatch_search(e, with_patches, start, stop);
    HIP_TRY(hipGetLastError());
    e->st.scan_launches += 1;
    e->st.arcs_scanned += e->end - e->begin;
    return MCF_OK;
}

// (re)computes the per-arc reduced costs of the RC layout from the arrays on the device
int rc_recompute(mcf_engine *e)
{
    with_width(e, [&](auto width) {
        using T = decltype(width);
        launch(rc_init_kernel<T>, dim3(e->count_padded / kThreads), dim3(kThreads), e->stream, nullptr, nullptr, e->d_src, e->d_tgt, (const T *)e->d_cost, (const T *)e->d_pi, e->d_rc, e->count_padded);
    });
    HIP_TRY(hipGetLastError());
    return MCF_OK;
}

// the shard's arcs at each node (RC layout): counting sort of the local positions by end point
int rc_build_adjacency(mcf_engine *e, const int32_t *src_local, const int32_t *tgt_local)
{
    const int n = e->d.node_count, count = e->end - e->begin;
    std::vector<int32_t> start((size_t)n + 1, 0);
    for (int i = 0; i < count; ++i) { start[src_local[i] + 1]++; start[tgt_local[i] + 1]++; }
    for (int u = 0; u < n; ++u) start[u + 1] += start[u];
    std::vector<uint32_t> adj((size_t)std::max(1, 2 * count), 0u);
    std::vector<int32_t> fill(start.begin(), start.end() - 1);
    for (int i = 0; i < count; ++i) {
        adj[fill[src_local[i]]++] = (uint32_t)i;
        adj[fill[tgt_local[i]]++] = (uint32_t)i | 0x80000000u;
    }
    HIP_TRY(hipMemcpy(e->d_adj_start, start.data(), sizeof(int32_t) * ((size_t)n + 1), hipMemcpyHostToDevice));
    e->h_adj_start.assign(start.begin(), start.end());
    HIP_TRY(hipMemcpy(e->d_adj, adj.data(), sizeof(uint32_t) * adj.size(), hipMemcpyHostToDevice));
    return MCF_OK;
}

// One launch over a potential list and a state list in device-visible memory (timed by the two events when they are given).  per_arc: the RC
// layout's update_rc_kernel, which also shifts the reduced costs of the nodes' arcs; otherwise update_kernel
void launch_list_update(mcf_engine *e, bool per_arc, hipEvent_t start, hipEvent_t stop, const int32_t *nodes, const int64_t *values, int n_pi, const int32_t *arcs,
                        const int32_t *states, int n_st)
{
    const dim3 grid((std::max(n_pi, n_st) + kThreads - 1) / kThreads), block(kThreads);
    with_width(e, [&](auto width) {
        using T = decltype(width);
        if (per_arc) launch(update_rc_kernel<T>, grid, block, e->stream, start, stop, (T *)e->d_pi, nodes, values, n_pi, e->d_state, arcs, states, n_st, e->begin, e->count_padded, e->d_rc, e->d_adj_start, e->d_adj);
        else launch(update_kernel<T>, grid, block, e->stream, start, stop, (T *)e->d_pi, nodes, values, n_pi, e->d_state, arcs, states, n_st, e->begin, e->count_padded);
    });
}

// ship the pending patches with update_kernel (lists too long for the kernel arguments, or explicit flush)
int cand_build_patches(mcf_engine *e);
int flush_pending(mcf_engine *e)
{
    // candidate mode keeps what the device has not heard yet as lists of nodes / arcs: turn them into patches (current values from the mirrors).
    // The list and the heap stay valid: they are bookkeeping about epochs, not about what the device knows.
    if (e->cand_on && (!e->sync_nodes.empty() || !e->sync_arcs.empty() || e->blind_count > 0)) { const int rcb = cand_build_patches(e); if (rcb) return rcb; }
    const bool reload = e->reload_pi;
    if (reload) {
        // mcf_engine_reload_potentials: the caller's whole array instead of lists (whatever was noted since is part of it), then -- below, after
        // the state writes -- every reduced cost of the shard again
        pend_clear_potentials(e);
        HIP_TRY(hipMemcpyAsync(e->d_pi, e->ext_pi, sizeof(int64_t) * (size_t)e->d.node_count, hipMemcpyHostToDevice, e->stream));
        e->reload_pi = false;
    }
    const int n_pi_all = (int)e->pend_node.size(), n_st_all = (int)e->pend_arc.size();
    if (n_pi_all == 0 && n_st_all == 0) {
        if (reload) { if (int rcr = rc_recompute(e)) return rcr; e->st.rc_recomputes += 1; }
        return MCF_OK;
    }
    // the staging buffers hold kStageStates state patches: longer lists go out in rounds (the potentials ride in the first)
    for (int st0 = 0, round = 0; round == 0 || st0 < n_st_all; st0 += kStageStates, ++round) {
        const int n_pi = round == 0 ? n_pi_all : 0, n_st = std::min(kStageStates, n_st_all - st0);
        mcf_engine::Staging &s = e->stage[e->stage_next];
        e->stage_next ^= 1;
        if (s.busy) { HIP_TRY(hipEventSynchronize(s.done)); s.busy = false; }
        if (n_pi) { memcpy(s.nodes, e->pend_node.data(), sizeof(int32_t) * n_pi); memcpy(s.values, e->pend_val.data(), sizeof(int64_t) * n_pi); }
        if (n_st) { memcpy(s.arcs, e->pend_arc.data() + st0, sizeof(int32_t) * n_st); memcpy(s.states, e->pend_state.data() + st0, sizeof(int32_t) * n_st); }
        // RC layout, a list that names more than a sixteenth of the nodes: shifting their arcs one by one (2 ns per node on config 5: 18 atomics in
        // memory each) costs more than writing the potentials and computing every reduced cost of the shard again (12 ps per arc: 107 us for 9 M arcs)
        const bool recompute = e->rc_mode && n_pi > e->rc_recompute_above;
        launch_list_update(e, e->rc_mode && !recompute, nullptr, nullptr, (const int32_t *)s.d_nodes, (const int64_t *)s.d_values, n_pi, (const int32_t *)s.d_arcs,
                           (const int32_t *)s.d_states, n_st);
        HIP_TRY(hipGetLastError());
        if (recompute) {
            if (int rcr = rc_recompute(e)) return rcr;
            e->st.rc_recomputes += 1;
        }
        HIP_TRY(hipEventRecord(s.done, e->stream));
        s.busy = true;
        e->st.update_launches += 1;
    }
    pend_clear(e);
    if (reload) { if (int rcr = rc_recompute(e)) return rcr; e->st.rc_recomputes += 1; }
    return MCF_OK;
}

#include "resident_host.hip.h"
#include "candidate_cache.hip.h"

// posts / launches the search; search_end collects it.  local_search = both.
int search_begin(mcf_engine *e)
{
    if (e->list_rule) return mcf::fail(MCF_ERR_STATE, "engines of the list rules (3, 4) are searched with mcf_engine_collect_eligible only");
    if (!e->uploaded) return mcf::fail(MCF_ERR_STATE, "mcf_engine_upload has not been called");
    if (e->in_flight != mcf_engine::kNoSearch) return mcf::fail(MCF_ERR_STATE, "a search is already in flight");
    Key *const k = &e->answered;
    const double t0 = (double)__rdtsc();
    const bool had = !e->pend_node.empty() || !e->pend_arc.empty();
    // a resident grid needs one of the device's slots; without one this search is served by a dispatch (the arrays are the same)
    const bool resident_now = e->resident_ok && (e->resident_running || resident_slot_acquire(e));
    if (e->cand_on && e->cand_now >= kCandEpochWrap && !e->async_posted) {
        cand_restart_epochs(e);
    }
    if (e->cand_on) {
        const double ta = (double)__rdtsc();
        if (e->pivot_overflow) e->n_gap_pivots += 1;
        cand_absorb_pivot(e, cand_graph(e));
        const double tb = (double)__rdtsc();
        e->tk_absorb += tb - ta;
        if (resident_now) {
            // ---- candidate cache: answer from the host whenever that provably is the scan's answer
            if (e->async_posted && cand_records_ready(e, 0)) { int rc = cand_collect(e, e->async_at); if (rc) return rc; }      // the refresh has arrived
            const double tc = (double)__rdtsc();
            e->tk_probe += tc - tb;
            bool decided = !e->force_device_search && cand_decide(e, k);
            e->tk_decide += (double)__rdtsc() - tc;
            if (e->force_device_search && e->async_posted) { int rc = cand_collect(e, e->async_at); if (rc) return rc; }       // one request at a time
            if (!decided && e->async_posted) {              // the refresh is what we are waiting for
                e->n_async_waits += 1;
                int rc = cand_collect(e, e->async_at);
                if (rc) return rc;
                decided = cand_decide(e, k);
            }
            if (decided) {
                e->st.searches += 1;
                e->st.host_decided += 1;
                e->in_flight = mcf_engine::kAnswered;
                // running low: ask for the next list now and keep answering from this one until it is here
                if (!e->async_posted && e->cand_thr.p != kNone && e->cand_list.size() - e->cand_ptr <= (size_t)kCandRefreshLow) {
                    int rc = cand_post(e);
                    if (rc) return rc;
                    e->async_posted = true;
                    e->async_at = e->posted_at;
                    e->st.async_refreshes += 1;
                }
                e->cand_now += 1;
                e->launch_ticks += (double)__rdtsc() - t0;
                return MCF_OK;
            }
            // the device searches: ship every node / arc touched since it last heard from us, with their current values
            const double tp = (double)__rdtsc();
            int rc = cand_post(e);
            if (rc) return rc;
            e->tk_post += (double)__rdtsc() - tp;
            e->n_sync_posts += 1;
            e->cand_now += 1;
            e->launch_ticks += (double)__rdtsc() - t0;
            e->st.searches += 1;
            e->in_flight = mcf_engine::kCandSearch;
            return MCF_OK;
        }
        e->cand_now += 1;
    }
    if (e->resident_ok && !resident_now) {
        const int rcf = flush_pending(e);       // the resident grid would have received these with its request
        if (rcf) return rcf;
    }
    if (resident_now) {
        // ---- resident mode: post the request into the mailbox, the grid is already running
        bool fits = (int)e->pend_arc.size() <= e->mailbox_max_st;     // any number of potentials fits the mailbox
        bool rc_reload = false;
        if (e->rc_mode) {
            // resident RC grid: a request is one staging chunk of {node, shift} entries; anything else goes through update_rc_kernel with the grid stopped
            // resident RC grid: a request carries {node, shift} entries, any number the mailbox holds (the grid works them off in chunks); a
            // reload of the bound potentials is a request too (cmd 3) when the device can read the array itself.  Anything else -- a change
            // that came without its shift, a reload of an array the device cannot see -- goes through update_rc_kernel with the grid stopped
            rc_reload = e->reload_pi && e->d_ext_pi != nullptr;
            if (rc_reload) { pend_clear_potentials(e); e->reload_pi = false; }          // whatever was announced since is part of the array
            const int64_t n_pi = (int64_t)e->pend_node.size(), n_st = (int64_t)e->pend_arc.size();
            fits = !e->reload_pi && (n_pi == 0 || e->pend_shift) && n_pi <= (int64_t)e->rc_list_max && n_st <= e->mailbox_max_st;
            if (fits && n_pi > 0) std::fill(e->pend_val.begin(), e->pend_val.end(), e->pend_sigma);      // the entries carry the shift, not the value
        }
        if (!fits) {
            // a list that does not fit the mailbox: stop the grid, ship it with update_kernel, start again
            int rc = resident_stop(e);
            if (!rc) rc = flush_pending(e);
            if (rc) return rc;
        }
        next_request_keep_prev(e);
        int rc = resident_start(e, e->prev_seq);
        if (rc) return rc;
        resident_post(e, e->seq, rc_reload ? kCmdReload : kCmdScan, fits);
        if (rc_reload) e->st.rc_reloads_in_grid += 1;
        if (fits) {
            if (had) e->st.inline_updates += 1;
            pend_clear(e);
        }
        e->launch_ticks += (double)__rdtsc() - t0;
        e->st.searches += 1;
        e->st.arcs_scanned += e->end - e->begin;
        e->in_flight = mcf_engine::kResidentSearch;
        return MCF_OK;
    }
    next_request(e);
    // RC layout: a potential change is a shift of the reduced costs of the node's arcs.  A short list with one common shift rides in the
    // scan's arguments (every workgroup shifts the arcs it scans itself); anything else goes through update_rc_kernel first
    const bool inline_ok = !(e->d.flags & MCF_ENGINE_NO_INLINE_UPDATE) && !e->reload_pi && (e->rc_mode ? rc_inline_ok(e) : (int)e->pend_node.size() <= kInlinePi) &&
                           (int)e->pend_arc.size() <= kInlineState;
    if (!inline_ok) { int rc = flush_pending(e); if (rc) return rc; }
    const bool timed = (e->d.flags & MCF_ENGINE_TIME_EVERY_KERNEL) ||
                       ((e->d.flags & MCF_ENGINE_SAMPLE_KERNEL_TIME) && (e->st.scan_launches & 15) == 0);
    int rc = launch_search(e, inline_ok, timed);
    if (rc) return rc;
    if (inline_ok) {
        if (had) e->st.inline_updates += 1;
        pend_clear(e);
    }
    e->launch_ticks += (double)__rdtsc() - t0;
    e->st.searches += 1;
    e->in_flight = mcf_engine::kDispatchSearch;
    e->in_flight_timed = timed;
    return MCF_OK;
}

int search_end(mcf_engine *e, Key *k)
{
    const auto what = e->in_flight;
    e->in_flight = mcf_engine::kNoSearch;
    int rc = MCF_OK;
    switch (what) {
    case mcf_engine::kNoSearch: return mcf::fail(MCF_ERR_STATE, "no search in flight");
    case mcf_engine::kAnswered: *k = e->answered; return MCF_OK;
    case mcf_engine::kCandSearch:
        rc = cand_collect(e, e->posted_at);
        if (rc) return rc;
        // the device saw everything up to this search, so its best key IS the answer (the global minimum is some workgroup's best and lies
        // below every unreported key); changes reported since search_begin belong to the next search and are not looked at
        k->r = 0;
        if (e->cand_list.empty()) { k->c = 0; k->p = kNone; }
        else { k->c = e->cand_list[0].c; k->p = e->cand_list[0].p; }
        return MCF_OK;
    case mcf_engine::kResidentSearch: return collect(e, e->res_grid, k);
    case mcf_engine::kDispatchSearch:
        rc = collect(e, e->grid, k);
        if (rc) return rc;
        if (e->in_flight_timed) drain_events(e, false);
        return MCF_OK;
    }
    return rc;
}

int local_search(mcf_engine *e, Key *k)
{
    const int rc = search_begin(e);
    return rc ? rc : search_end(e, k);
}

// entering arc, reduced cost and the rule's next_arc from the winning key (host part of the rules)
// *checked (optional) = arcs the reference's plain BlockSearchPivot examines in this call (its arcsChecked, NS.cs:1345-1372); 0 for the others
// vec / range: OPTIMIZED Block Search on a host with Vector<long>.Count == vec (0: not hardware accelerated); range = the scan's range key
void resolve_key_raw(int rule, int semantics, int vec, int m_s, int B, int &next_arc, const Key &k, const Key &range, int32_t *found, int32_t *arc, int64_t *rcost,
                     int64_t *checked = nullptr)
{
    const bool counts = rule == MCF_RULE_BLOCK_SEARCH && semantics != MCF_SEM_OPTIMIZED;
    if (checked) *checked = counts ? m_s : 0;         // nothing eligible, or the cycle ran out before a block boundary: every arc once
    if (k.p == kNone) { *found = 0; *arc = -1; if (rcost) *rcost = 0; return; }
    *found = 1;
    if (rcost) *rcost = k.c;
    if (rule == MCF_RULE_BEST_ELIGIBLE) { *arc = (int32_t)k.p; return; }          // stateless: NS.cs:1644-1667
    const int na = next_arc >= m_s ? 0 : next_arc;
    const int a = (int)(((int64_t)k.p + na) % m_s);
    *arc = a;
    if (rule == MCF_RULE_FIRST_ELIGIBLE) { next_arc = a + 1; return; }             // NS.cs:1617, BSPO.cs:199
    const int64_t r = k.p / B, boundary = (r + 1) * (int64_t)B - 1;   // scan position of the block's last arc
    if (semantics != MCF_SEM_OPTIMIZED) {
        // NS.cs:1358-1397: stop at the boundary -> next_arc = that arc; cycle exhausted first -> unchanged
        if (boundary <= m_s - 1) { next_arc = (int)((boundary + na) % m_s); if (checked) *checked = boundary + 1; }
        return;
    }
    // BSPO.cs:49-63: first range [next_arc, m_s), wrapped range [0, next_arc) only if the first one found nothing.  The counter runs on
    // across the two (ref cnt), so the first block boundary behind an eligible arc is the one the block key names.  Where that boundary
    // falls decides what the reference does there (BSPO.cs:69-156):
    //   * inside the "SIMD" part of its range -- the first floor(len / vec) * vec arcs of a range of len >= 2 * vec arcs, vec > 0 --
    //     ProcessArcRangeSIMD returns idx + 1 and ProcessArcRange's scalar loop carries on with cnt == 0, which never counts down to 0
    //     again: it scans to the END of the range, min / bestArc end up as the best arc of the whole range (strict <: first in scan
    //     order among equals; the blocks before the hit held nothing eligible), and the range's end is returned -> _nextArc;
    //   * in the scalar tail, or in a range too short for the SIMD part, or with vec == 0: stop there, _nextArc = boundary arc + 1;
    //   * behind the end of the range (a partial last block): the range ends first and ProcessArcRange returns `end`.
    const int64_t len1 = next_arc >= m_s ? 0 : m_s - next_arc;
    const bool first_range = a >= next_arc && next_arc < m_s;
    const int64_t start = first_range ? 0 : len1;                    // scan position where the winning arc's range begins ...
    const int64_t len = first_range ? len1 : m_s - len1;             // ... and its length
    const int range_end = first_range ? m_s : next_arc;              // what ProcessArcRange returns when it runs to `end`
    if (boundary < start + len) {
        const bool simd_hit = vec > 0 && len >= 2 * (int64_t)vec && boundary - start < len / vec * vec;
        if (simd_hit) {
            *arc = (int)(((int64_t)range.p + na) % m_s);             // the range key: the first range with an eligible arc is this one
            if (rcost) *rcost = range.c;
            next_arc = range_end;
        } else {
            next_arc = (int)(first_range ? next_arc + boundary + 1 : boundary - len1 + 1);
        }
    } else {
        next_arc = range_end;                                        // first range: m_s (BSPO.cs:52 does not wrap, min < 0); wrapped: unchanged
    }
}

void resolve_key(mcf_engine *e, const Key &k, int32_t *found, int32_t *arc, int64_t *rcost)
{
    int64_t checked = 0;
    resolve_key_raw(e->d.rule, e->d.semantics, e->vec, e->d.search_arc_num, e->block_size, e->next_arc, k, e->range_key, found, arc, rcost, &checked);
    e->st.arcs_checked += checked;
    if (!*found || !e->cfg_set || !(e->cfg.flags & MCF_OPT_ADAPTIVE_BLOCK_SIZE) || e->d.rule != MCF_RULE_BLOCK_SEARCH || e->d.semantics == MCF_SEM_OPTIMIZED) return;
    int32_t counters[2] = {e->low_hits, e->high_hits};
    mcf_block_adapt(&e->cfg, e->dyn_min_block, checked, &e->block_size, counters);      // NS.cs:1400-1438
    e->low_hits = counters[0];
    e->high_hits = counters[1];
    if (e->block_size < 1) e->block_size = 1;       // a block of 0 arcs never reaches a boundary in the reference; keep the kernels' divisor sane
}

// MINLOC over the shards' candidates with the rule's ordering; *range_out = the same over their range keys (OPTIMIZED Block Search)
Key merge_candidates(int rule, int semantics, int m_s, int B, int next_arc, int count, const mcf_candidate *all, Key *range_out)
{
    const SearchHeader h = search_header(rule, semantics, m_s, next_arc, B);
    Key best{0, kNone, kNone}, range{0, kNone, kNone};
    for (int i = 0; i < count; ++i) {
        if (all[i].pos == kNone) continue;
        Key k{all[i].reduced_cost, 0, all[i].pos};
        if (rule == MCF_RULE_BLOCK_SEARCH) k.r = h.block_rank(k.p, all[i].arc);
        if (key_better(rule, k, best)) best = k;
        if (h.dual && all[i].range_pos != kNone) {
            const Key q{all[i].range_cost, h.wrapped(all[i].range_arc), all[i].range_pos};
            if (range_better(q, range)) range = q;
        }
    }
    if (range_out) *range_out = range;
    return best;
}

}  // namespace

extern "C" {

int mcf_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return n;
}

int mcf_device_compute_units(int32_t device)
{
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return cus;
}

int mcf_shard_range(int32_t m_s, int32_t rank, int32_t world, int32_t *begin, int32_t *end)
{
    if (world < 1 || rank < 0 || rank >= world || m_s < 0 || !begin || !end) return mcf::fail(MCF_ERR_INVALID, "mcf_shard_range: bad arguments");
    const int64_t groups = ((int64_t)m_s + kArcsPerThread - 1) / kArcsPerThread;
    const int64_t b = groups * rank / world * kArcsPerThread, en = groups * (rank + 1) / world * kArcsPerThread;
    *begin = (int32_t)std::min<int64_t>(b, m_s);
    *end = (int32_t)std::min<int64_t>(en, m_s);
    return MCF_OK;
}

int mcf_engine_create(mcf_engine **out, const mcf_engine_desc *desc)
{
    if (!out || !desc) return mcf::fail(MCF_ERR_INVALID, "mcf_engine_create: null argument");
    *out = nullptr;
    if (desc->node_count < 1 || desc->search_arc_num < 0 || desc->arc_capacity < desc->search_arc_num)
        return mcf::fail(MCF_ERR_INVALID, "mcf_engine_create: bad sizes (nodes %d, arcs %d, search %d)", desc->node_count, desc->arc_capacity, desc->search_arc_num);
    if (desc->int_width != 32 && desc->int_width != 64) return mcf::fail(MCF_ERR_INVALID, "int_width must be 32 or 64");
    if (desc->rule < 0 || desc->rule > 4) return mcf::fail(MCF_ERR_INVALID, "pivot rule %d does not exist (Types/PivotRule.cs:7-41)", desc->rule);
    const bool list_rule = desc->rule == MCF_RULE_CANDIDATE_LIST || desc->rule == MCF_RULE_ALTERING_LIST;
    if (list_rule && !((desc->shard_begin == 0 && desc->shard_end == 0) || (desc->shard_begin == 0 && desc->shard_end == desc->search_arc_num)))
        return mcf::fail(MCF_ERR_INVALID, "the list rules (3, 4) scan the whole search range: no arc shards");
    if (desc->semantics != MCF_SEM_PLAIN && desc->semantics != MCF_SEM_OPTIMIZED) return mcf::fail(MCF_ERR_INVALID, "bad semantics %d", desc->semantics);
    if (desc->vector_width != MCF_VECTOR_DEFAULT && desc->vector_width != MCF_VECTOR_NONE && desc->vector_width != 2 && desc->vector_width != 4 && desc->vector_width != 8)
        return mcf::fail(MCF_ERR_INVALID, "vector_width %d is not Vector<long>.Count of any machine (2, 4, 8, MCF_VECTOR_NONE, or 0 = 4)", desc->vector_width);
    if (mcf_device_count() <= desc->device || desc->device < 0)
        return mcf::fail(MCF_ERR_NO_DEVICE, "HIP device %d not available (%d visible); this library has no CPU search path", desc->device, mcf_device_count());
    HIP_TRY(hipSetDevice(desc->device));
    mcf_engine *e = new mcf_engine();
    e->cal_ns = mcf::now_ns();
    e->cal_ticks = (double)__rdtsc();
    e->d = *desc;
    e->list_rule = list_rule;
    e->vec = desc->vector_width == MCF_VECTOR_NONE ? 0 : (desc->vector_width == MCF_VECTOR_DEFAULT ? 4 : desc->vector_width);
    e->begin = desc->shard_begin;
    e->end = desc->shard_end;
    if (e->begin == 0 && e->end == 0) e->end = desc->search_arc_num;
    if (e->begin < 0 || e->end < e->begin || e->end > desc->search_arc_num || (e->begin % kArcsPerThread) != 0) {
        delete e;
        return mcf::fail(MCF_ERR_INVALID, "bad shard [%d, %d)", desc->shard_begin, desc->shard_end);
    }
    const int count = e->end - e->begin;
    // geometry of the resident grid: as many workgroups as CUs (<= 256), each just wide enough to hold its share of the arcs in
    // registers (4 per thread); above 1M arcs the workgroups are 1024 wide and loop over memory instead
    {
        const int64_t groups4 = ((int64_t)count + kArcsPerThread - 1) / kArcsPerThread;            // threads needed
        // at least four waves per workgroup before a second workgroup is opened: every workgroup is a poller and a record to collect
        // (config 2: 157 x 64 threads -> 40 x 256 took 1.3-1.8 us off each pivot)
        // several engines that share a device (arc shards rehearsed on one GPU) must all be co-resident, or a grid that never gets its
        // CUs would never answer: desc.resident_workgroups caps the grid
        const int max_grid = desc->resident_workgroups > 0 ? std::min(desc->resident_workgroups, kResidentMaxGrid) : kResidentMaxGrid;
        int g = (int)std::min<int64_t>(max_grid, std::max<int64_t>(1, (groups4 + 255) / 256));
        int64_t t = ((groups4 + g - 1) / g + 63) / 64 * 64;
        t = std::max<int64_t>(64, std::min<int64_t>(t, kResidentThreads));
        e->res_grid = g;
        e->res_threads = (int)t;
        e->resident_reg = (int64_t)g * t * kArcsPerThread >= count;
    }
    e->count_padded = std::max(kPad, (count + kPad - 1) / kPad * kPad);
    if (e->resident_reg) {
        const int64_t need = (int64_t)e->res_grid * e->res_threads * kArcsPerThread;
        if (need > e->count_padded) e->count_padded = (int)((need + kPad - 1) / kPad * kPad);
    }
    e->block_size = desc->block_size > 0 ? desc->block_size : mcf::default_block_size(desc->search_arc_num, desc->semantics);
    e->unroll = count > (1 << 20) ? 2 : 1;
    const int groups = e->count_padded / (kTile * e->unroll);
    e->grid = desc->scan_workgroups > 0 ? std::min(desc->scan_workgroups, kMaxWorkgroups) : std::min(groups, kScanMaxGrid);
    e->grid = std::max(1, std::min(e->grid, groups));
    e->lds_pi = desc->node_count <= kLdsPiMax;
    e->no_pireg = (desc->flags & MCF_ENGINE_SHARE_DEVICE) != 0;
    if (e->lds_pi) {
        // one 1024-thread workgroup per CU (the 128 KB potential copy allows no more); each loops over its 4096-arc tiles
        e->unroll = count > (2 << 20) ? 2 : 1;
        const int tiles = e->count_padded / (e->unroll * kResidentTile);
        e->grid = std::max(1, std::min(tiles, desc->scan_workgroups > 0 ? desc->scan_workgroups : 256));
    }
    // RC layout: for arcs that would be streamed from memory for every search anyway (neither register-resident nor beside LDS-resident
    // potentials) -- what also picks one dispatch per search.  MCF_HIP_RC=1 forces it on any size (tests), MCF_HIP_RC=0 keeps the gathering
    // scan (and with it the bucketed layout).
    {
        bool want = !e->resident_reg && !e->lds_pi;
        want = mcf::env_int("MCF_HIP_RC", 0, 1, want) != 0;
        if (list_rule) want = false;          // the list rules read the SoA arrays themselves (collect.hip.h)
        e->rc_mode = want;
        if (e->rc_mode) {
            // pure streaming: more bytes in flight per thread, the grid sized so that every workgroup gets the same number of trips
            // measured on config 5's arrays (profiles/r02_rc_layout_scan.txt, r02_rc_layout_scan_threads.txt): everything between 256 and 1024
            // workgroups of 256 .. 1024 threads lands within 14.3-15.6 us warm / 16.6-17.7 cold for 81 MB; 512 x 256 with two tiles per trip is
            // the best of them, more workgroups only add launch ramp and tail
            e->rc_recompute_above = std::max(1024, desc->node_count / 16);
            e->rc_list_max = kRcResidentNodes;
            const int recompute = (int)mcf::env_int("MCF_HIP_RC_RECOMPUTE", 0, INT32_MAX, e->rc_recompute_above);
            e->rc_recompute_above = recompute == 0 ? INT32_MAX : recompute;      // 0: never
            e->unroll = count > (1 << 20) ? 2 : 1;
            const int groups_rc = std::max(1, e->count_padded / (kThreads * kArcsPerThread * e->unroll));
            e->grid = desc->scan_workgroups > 0 ? std::min(desc->scan_workgroups, kMaxWorkgroups) : std::min(groups_rc, kRcMaxGrid);
            e->grid = std::max(1, std::min(e->grid, groups_rc));
        }
    }
    e->patch_capacity = 2 * desc->node_count + 256;
    const size_t w = desc->int_width / 8;
    hipError_t err = hipSuccess;
    auto chk = [&](hipError_t x) { if (err == hipSuccess && x != hipSuccess) err = x; };
    chk(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
    chk(hipMalloc((void **)&e->d_src, sizeof(int32_t) * e->count_padded));
    chk(hipMalloc((void **)&e->d_tgt, sizeof(int32_t) * e->count_padded));
    chk(hipMalloc(&e->d_cost, w * e->count_padded));
    chk(hipMalloc((void **)&e->d_state, e->count_padded));
    chk(hipMalloc(&e->d_pi, w * (size_t)desc->node_count));
    if (e->rc_mode) {
        chk(hipMalloc((void **)&e->d_rc, sizeof(int64_t) * e->count_padded));
        chk(hipMalloc((void **)&e->d_adj_start, sizeof(int32_t) * ((size_t)desc->node_count + 1)));
        chk(hipMalloc((void **)&e->d_adj, sizeof(uint32_t) * (size_t)std::max(1, 2 * count)));
    }
    chk(hipHostMalloc((void **)&e->h_slots, sizeof(Slot) * kMaxWorkgroups * kSlotStride, hipHostMallocMapped | hipHostMallocCoherent));
    if (err == hipSuccess) {
        memset(e->h_slots, 0, sizeof(Slot) * kMaxWorkgroups * kSlotStride);
        chk(hipHostGetDevicePointer((void **)&e->d_slots, e->h_slots, 0));
    }
    for (int i = 0; i < 2 && err == hipSuccess; ++i) {
        mcf_engine::Staging &s = e->stage[i];
        s.cap_nodes = 2 * desc->node_count + 256;
        chk(hipHostMalloc((void **)&s.nodes, sizeof(int32_t) * s.cap_nodes, hipHostMallocMapped | hipHostMallocCoherent));
        chk(hipHostMalloc((void **)&s.values, sizeof(int64_t) * s.cap_nodes, hipHostMallocMapped | hipHostMallocCoherent));
        chk(hipHostMalloc((void **)&s.arcs, sizeof(int32_t) * kStageStates, hipHostMallocMapped | hipHostMallocCoherent));
        chk(hipHostMalloc((void **)&s.states, sizeof(int32_t) * kStageStates, hipHostMallocMapped | hipHostMallocCoherent));
        if (err == hipSuccess) {
            chk(hipHostGetDevicePointer(&s.d_nodes, s.nodes, 0));
            chk(hipHostGetDevicePointer(&s.d_values, s.values, 0));
            chk(hipHostGetDevicePointer(&s.d_arcs, s.arcs, 0));
            chk(hipHostGetDevicePointer(&s.d_states, s.states, 0));
        }
        chk(hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
    }
    for (int i = 0; i < mcf_engine::kEvRing && err == hipSuccess; ++i) { chk(hipEventCreate(&e->ev_start[i])); chk(hipEventCreate(&e->ev_stop[i])); }
    if (list_rule && err == hipSuccess) {
        e->pend_index.assign((size_t)desc->node_count, -1);
        chk(hipMalloc((void **)&e->d_tiles, sizeof(CollectTile) * kCollectMaxTiles));
        chk(hipHostMalloc((void **)&e->h_collect_hdr, sizeof(CollectHeader), hipHostMallocMapped | hipHostMallocCoherent));
        if (err == hipSuccess) chk(hipHostGetDevicePointer((void **)&e->d_collect_hdr, e->h_collect_hdr, 0));
    }
    if (err != hipSuccess) {
        const int rc = mcf::fail(MCF_ERR_HIP, "mcf_engine_create: %s", hipGetErrorString(err));
        mcf_engine_destroy(e);
        return rc;
    }
    // resident mode: the default (MCF_ENGINE_DISPATCH / MCF_HIP_RESIDENT=0 ask for one dispatch per search)
    {
        const int env = (int)mcf::env_int("MCF_HIP_RESIDENT", 0, 1, -1);
        bool want = (desc->flags & MCF_ENGINE_DISPATCH) == 0;      // resident unless dispatch mode is asked for
        // arcs that fit neither registers nor (with their potentials) LDS are streamed from memory for every search anyway: one dispatch
        // per search with 2048 workgroups is then faster than 256 resident ones (config 5: 71 vs 85 us per pivot)
        if (!e->resident_reg && !e->lds_pi) want = false;
        // the RC layout has its own resident grid (resident_rc_kernel): windows of arcs in LDS when they fit, streamed otherwise
        if (e->rc_mode) want = (desc->flags & MCF_ENGINE_DISPATCH) == 0;
        if (env == 1 && !e->rc_mode) want = true;
        if (env == 0) want = false;
        if (list_rule) want = false;          // dispatch mode only: no resident grid, hence no candidate cache either
        // an arc shard is served by a resident grid like a whole instance (every workgroup applies every potential patch, state patches
        // outside the shard are ignored); only the RCCL exchange needs the stream, and mcf_engine_comm_init switches to dispatch mode
        if (want && !(desc->flags & (MCF_ENGINE_TIME_EVERY_KERNEL | MCF_ENGINE_NO_INLINE_UPDATE))) {
            e->mailbox_max_st = 4096;
            e->mailbox_lines = 2 + (e->patch_capacity + e->mailbox_max_st + kMailboxPatchesPerLine - 1) / kMailboxPatchesPerLine;
            e->max_shift_lines = (desc->node_count + kShiftNodesPerLine - 1) / kShiftNodesPerLine + 1;
            e->shift_base = (uint32_t)kMailboxTail + 16u * (uint32_t)e->mailbox_lines;
            e->idle_ticks = (uint32_t)(mcf::env_int("MCF_HIP_IDLE_MS", 1, 10000, kResidentIdleTicks / 100000) * 100000);
            e->mailbox = alloc_bar_vram(desc->device, (size_t)kMailboxTail * 4 + ((size_t)e->mailbox_lines + e->max_shift_lines) * 64);
            if (e->mailbox && hipHostMalloc((void **)&e->h_exit, 64, hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess &&
                hipHostGetDevicePointer((void **)&e->d_exit, e->h_exit, 0) == hipSuccess &&
                hipEventCreate(&e->res_start) == hipSuccess && hipEventCreate(&e->res_stop) == hipSuccess) {
                alignas(16) uint32_t zero[16] = {0};
                for (size_t l = 0; l < (size_t)kMailboxTail / 16 + e->mailbox_lines + e->max_shift_lines; ++l) mailbox_write_line(e->mailbox + 16 * l, zero);
                _mm_sfence();
                e->resident_ok = true;
                if (e->rc_mode) {
                    // one 1024-thread workgroup per CU; a window of at most kRcWindow arcs per workgroup stays in LDS
                    const int max_grid = desc->resident_workgroups > 0 ? std::min(desc->resident_workgroups, kResidentMaxGrid) : kResidentMaxGrid;
                    e->res_threads = kResidentThreads;
                    e->res_grid = std::max(1, std::min(max_grid, e->count_padded / kResidentTile));
                    const int64_t per = ((int64_t)e->count_padded + e->res_grid - 1) / e->res_grid;
                    e->rc_window = (int)((per + kResidentTile - 1) / kResidentTile * kResidentTile);
                    e->rc_lds = e->rc_window <= kRcWindow && !mcf::env_off("MCF_HIP_RC_LDS");
                    if (!e->rc_lds) e->rc_window = 0;
                    e->resident_reg = false;
                    // the grid-wide barrier of that grid (long lists are dealt out, reloads are carried out in the grid): one counter in device memory
                    if (hipMalloc((void **)&e->d_barrier, 64) != hipSuccess) { e->d_barrier = nullptr; (void)hipGetLastError(); }
                    e->rc_list_max = e->d_barrier ? std::min(2 * desc->node_count, std::max(kRcResidentNodes, e->rc_recompute_above)) : kRcResidentNodes;
                }
                e->cand_on = !(desc->flags & MCF_ENGINE_NO_CANDIDATES) && !mcf::env_off("MCF_HIP_CANDIDATES") &&
                             (e->resident_reg || e->rc_mode) && desc->rule == MCF_RULE_BEST_ELIGIBLE && desc->node_count < (1 << 29) &&
                             2 * (int64_t)desc->search_arc_num <= (int64_t)kCandMaxAvgDegree * desc->node_count;
                e->shift_grid = e->cand_on && e->resident_reg && !e->rc_mode && !e->lds_pi && !e->no_pireg && desc->int_width == 64 &&
                                desc->node_count <= kShiftBits;
                if (e->shift_grid) {
                    // that grid keeps 2 or 4 tiles of four arcs per thread: at most 256 threads, one wave per SIMD
                    const int64_t groups4 = ((int64_t)count + kArcsPerThread - 1) / kArcsPerThread;
                    e->cand_tiles = groups4 <= (int64_t)2 * e->res_grid * kCandThreads ? 2 : 4;
                    const int64_t t = std::max<int64_t>(64, ((groups4 + (int64_t)e->cand_tiles * e->res_grid - 1) / ((int64_t)e->cand_tiles * e->res_grid) + 63) / 64 * 64);
                    if (t > kCandThreads) e->shift_grid = false;       // cannot happen: resident_reg caps the arcs at 1 M
                    else e->res_threads = (int)t;
                }
                if (e->shift_grid) {
                    // walks of this many nodes and more travel as "reload the bound potentials" (cmd 3: copy + grid-wide barrier + gather, inside the
                    // grid) instead of as a node list: the host's walk then writes nothing but its own potentials.  MCF_HIP_SHIFT_RELOAD=N (0 = never)
                    // Measured on config 3 (tools/gpu_walk_variants.py): the reload costs 40 - 44 us in the grid (800 KB over PCIe, the barrier, the
                    // gather) against 13 - 15 for a list that travelled during the walk, and saves the walk its list only before the first
                    // relabelling -- from 32768 nodes on it wins (246 against 240 - 245 k pivots/s), from 8192 on it does not (243 k).
                    e->shift_reload_min = (int)mcf::env_int("MCF_HIP_SHIFT_RELOAD", 0, INT32_MAX, 32768);
                    if (e->shift_reload_min > 0 && hipMalloc((void **)&e->d_barrier, 64) != hipSuccess) { e->d_barrier = nullptr; (void)hipGetLastError(); }
                }
            }
        }
    }
    e->st.scan_workgroups = e->resident_ok ? e->res_grid : e->grid;
    {
        // bucketed layout: automatic for large sparse Best-Eligible instances; MCF_HIP_BUCKET_NODES=N forces N nodes per range (0 = off)
        int want = (count >= kBucketMinArcs && desc->node_count > 2 * kBucketNodes) ? kBucketNodes : 0;
        want = (int)mcf::env_int("MCF_HIP_BUCKET_NODES", 0, INT32_MAX, want);
        const bool tile_loop = !e->lds_pi && !(e->resident_ok && e->resident_reg) && !e->rc_mode;
        if (want > 0 && desc->rule == MCF_RULE_BEST_ELIGIBLE && tile_loop && !e->cand_on) {
            if (hipMalloc((void **)&e->d_orig, sizeof(int32_t) * e->count_padded) == hipSuccess) e->bucket_nodes = want;
        }
    }
    e->st.scan_threads = e->resident_ok ? e->res_threads : (e->lds_pi ? kResidentThreads : kThreads);
    e->st.resident = e->resident_ok ? 1 : 0;
    e->st.candidates = e->cand_on ? 1 : 0;
    e->st.bytes_per_scan = (int64_t)(desc->int_width == 64 ? 17 : 13) * count + (int64_t)w * desc->node_count;
    e->st.scan_bytes_read = e->rc_mode ? (int64_t)9 * count : e->st.bytes_per_scan;
    e->st.rc_layout = e->rc_mode ? 1 : 0;
    e->st.shift_grid = e->shift_grid ? 1 : 0;
    e->st.initial_block_size = e->st.current_block_size = e->block_size;
    e->cand_epoch0 = (uint32_t)mcf::env_int("MCF_HIP_CAND_EPOCH0", 1, 0xFFFFFFFFll, 1);
    e->heap_compact_above = (size_t)mcf::env_int("MCF_HIP_CAND_HEAP_COMPACT", 1, 1ll << 30, (long long)e->heap_compact_above);
    e->cand_debug = getenv("MCF_HIP_CAND_DEBUG") != nullptr;
    *out = e;
    return MCF_OK;
}

namespace {
// Host arrays registered with HIP on behalf of the engines that bind them (several engines of one solver bind the same array): one
// registration per array, given back when the last engine lets go of it.
std::mutex g_pin_mutex;
std::map<const void *, int> g_pins;
bool host_pin(const void *p, size_t bytes)
{
    std::lock_guard<std::mutex> lock(g_pin_mutex);
    auto it = g_pins.find(p);
    if (it != g_pins.end()) { it->second += 1; return true; }
    const hipError_t r = hipHostRegister(const_cast<void *>(p), bytes, hipHostRegisterPortable | hipHostRegisterMapped);
    (void)hipGetLastError();                      // a refusal is not an error of the engine: it then takes node lists only
    if (r != hipSuccess) return false;
    g_pins[p] = 1;
    return true;
}
void host_unpin(const void *p)
{
    std::lock_guard<std::mutex> lock(g_pin_mutex);
    auto it = g_pins.find(p);
    if (it == g_pins.end()) return;
    if (--it->second > 0) return;
    g_pins.erase(it);
    (void)hipHostUnregister(const_cast<void *>(p));
    (void)hipGetLastError();
}
}  // namespace

void mcf_engine_destroy(mcf_engine *e)
{
    if (!e) return;
    if (e->cand_on && e->cand_debug && e->st.searches > 1000) {
        const double ns_per_tick = (mcf::now_ns() - e->cal_ns) / std::max(1.0, (double)__rdtsc() - e->cal_ticks);
        const double n = (double)e->st.searches;
        fprintf(stderr, "[cand] searches %lld host %lld async %lld sync_posts %lld async_waits %lld gap_pivots %lld | per search ns: absorb %.0f probe %.0f decide %.0f post %.0f collect %.0f wait %.0f | heap size %zu pushes %lld admitted %lld pops %lld sweeps %lld\n",
                (long long)e->st.searches, (long long)e->st.host_decided, (long long)e->st.async_refreshes, (long long)e->n_sync_posts, (long long)e->n_async_waits,
                (long long)e->n_gap_pivots, e->tk_absorb * ns_per_tick / n, e->tk_probe * ns_per_tick / n, e->tk_decide * ns_per_tick / n, e->tk_post * ns_per_tick / n,
                e->tk_collect * ns_per_tick / n, e->wait_ticks * ns_per_tick / n, e->heap.size(), (long long)e->n_heap_push, (long long)e->n_heap_admit, (long long)e->n_heap_pop,
                (long long)e->n_heap_sweeps);
    }
    (void)hipSetDevice(e->d.device);
    (void)resident_stop(e);
    if (e->ext_pi && e->ext_pi_pinned) { if (e->stream) (void)hipStreamSynchronize(e->stream); host_unpin(e->ext_pi); }
    if (e->stream) (void)hipStreamSynchronize(e->stream);
    if (e->res_stream) { (void)hipStreamSynchronize(e->res_stream); (void)hipStreamDestroy(e->res_stream); e->res_stream = nullptr; }
    if (e->mailbox) hsa_amd_memory_pool_free(e->mailbox);
    if (e->h_exit) (void)hipHostFree(e->h_exit);
    if (e->res_start) (void)hipEventDestroy(e->res_start);
    if (e->res_stop) (void)hipEventDestroy(e->res_stop);
    if (e->comm && rccl() && rccl()->comm_destroy) rccl()->comm_destroy(e->comm);
    if (e->d_orig) (void)hipFree(e->d_orig);
    (void)hipFree(e->d_rc); (void)hipFree(e->d_adj_start); (void)hipFree(e->d_adj); (void)hipFree(e->d_barrier); (void)hipFree(e->d_node_map);
    (void)hipFree(e->d_src); (void)hipFree(e->d_tgt); (void)hipFree(e->d_cost); (void)hipFree(e->d_state); (void)hipFree(e->d_pi);
    (void)hipFree(e->d_cand_local); (void)hipFree(e->d_cand_all); (void)hipFree(e->d_flush); (void)hipFree(e->d_dev_slots);
    (void)hipFree(e->d_tiles);
    if (e->h_collect_hdr) (void)hipHostFree(e->h_collect_hdr);
    if (e->h_collect) (void)hipHostFree(e->h_collect);
    if (e->h_cand_all) (void)hipHostFree(e->h_cand_all);
    if (e->comm_stream) { (void)hipStreamSynchronize(e->comm_stream); (void)hipStreamDestroy(e->comm_stream); }
    if (e->x_send) (void)hipHostFree(e->x_send);
    if (e->x_recv) (void)hipHostFree(e->x_recv);
    if (e->h_slots) (void)hipHostFree(e->h_slots);
    for (auto &s : e->stage) {
        if (s.nodes) (void)hipHostFree(s.nodes);
        if (s.values) (void)hipHostFree(s.values);
        if (s.arcs) (void)hipHostFree(s.arcs);
        if (s.states) (void)hipHostFree(s.states);
        if (s.done) (void)hipEventDestroy(s.done);
    }
    for (int i = 0; i < mcf_engine::kEvRing; ++i) {
        if (e->ev_start[i]) (void)hipEventDestroy(e->ev_start[i]);
        if (e->ev_stop[i]) (void)hipEventDestroy(e->ev_stop[i]);
    }
    if (e->stream) (void)hipStreamDestroy(e->stream);
    delete e;
}

int mcf_engine_upload(mcf_engine *e, const int32_t *source, const int32_t *target, const int64_t *cost, const int8_t *state, const int64_t *pi)
{
    if (!e || !source || !target || !cost || !state || !pi) return mcf::fail(MCF_ERR_INVALID, "mcf_engine_upload: null argument");
    HIP_TRY(hipSetDevice(e->d.device));
    if (int rcs = resident_stop(e)) return rcs;
    const int n = e->d.node_count, count = e->end - e->begin, cp = e->count_padded;
    for (int i = e->begin; i < e->end; ++i)
        if ((unsigned)source[i] >= (unsigned)n || (unsigned)target[i] >= (unsigned)n)
            return mcf::fail(MCF_ERR_INVALID, "arc %d has an end point outside [0, %d)", i, n);
    int64_t maxc = 0;
    for (int i = e->begin; i < e->end; ++i) maxc = std::max<int64_t>(maxc, cost[i] < 0 ? -cost[i] : cost[i]);
    e->max_abs_cost = maxc;
    std::vector<int32_t> s(cp, 0), t(cp, 0);
    std::vector<int8_t> st(cp, 0);
    const int32_t *pos = nullptr;                      // local arc -> local position
    if (e->bucket_nodes > 0) {
        // stable counting sort by target range: inside a range the arcs keep their order (sources stay grouped, ties resolve by position)
        const int buckets = (n + e->bucket_nodes - 1) / e->bucket_nodes;
        std::vector<int32_t> start(buckets + 1, 0);
        for (int i = 0; i < count; ++i) start[target[e->begin + i] / e->bucket_nodes + 1]++;
        for (int b = 0; b < buckets; ++b) start[b + 1] += start[b];
        e->pos_of.resize(count);
        std::vector<int32_t> orig(cp, 0x7FFFFFFF);
        for (int i = 0; i < count; ++i) {
            const int q = start[target[e->begin + i] / e->bucket_nodes]++;
            e->pos_of[i] = q;
            orig[q] = e->begin + i;
        }
        pos = e->pos_of.data();
        HIP_TRY(hipMemcpy(e->d_orig, orig.data(), sizeof(int32_t) * cp, hipMemcpyHostToDevice));
    }
    auto at = [&](int i) { return pos ? pos[i] : i; };
    for (int i = 0; i < count; ++i) { const int q = at(i); s[q] = source[e->begin + i]; t[q] = target[e->begin + i]; st[q] = state[e->begin + i]; }
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipMemcpy(e->d_src, s.data(), sizeof(int32_t) * cp, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(e->d_tgt, t.data(), sizeof(int32_t) * cp, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(e->d_state, st.data(), cp, hipMemcpyHostToDevice));
    if (e->d.int_width == 32) {
        // d = cost + pi[s] - pi[t] is formed in 64 bits on the device, so each operand only has to fit int32
        std::vector<int32_t> c(cp, 0), p(n);
        for (int i = 0; i < count; ++i) {
            if (!fits32(cost[e->begin + i])) return mcf::fail(MCF_ERR_OVERFLOW, "cost of arc %d does not fit int32", e->begin + i);
            c[at(i)] = (int32_t)cost[e->begin + i];
        }
        for (int i = 0; i < n; ++i) {
            if (!fits32(pi[i])) return mcf::fail(MCF_ERR_OVERFLOW, "potential of node %d does not fit int32", i);
            p[i] = (int32_t)pi[i];
        }
        HIP_TRY(hipMemcpy(e->d_cost, c.data(), sizeof(int32_t) * cp, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(e->d_pi, p.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice));
    } else {
        std::vector<int64_t> c(cp, 0);
        for (int i = 0; i < count; ++i) c[at(i)] = cost[e->begin + i];
        HIP_TRY(hipMemcpy(e->d_cost, c.data(), sizeof(int64_t) * cp, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(e->d_pi, pi, sizeof(int64_t) * n, hipMemcpyHostToDevice));
    }
    if (e->rc_mode) {
        int rcr = rc_build_adjacency(e, source + e->begin, target + e->begin);      // arcs keep their own order in this layout: position = arc - begin
        if (!rcr) rcr = rc_recompute(e);
        if (rcr) return rcr;
        HIP_TRY(hipStreamSynchronize(e->stream));
    }
    e->pi.assign(pi, pi + n);
    e->mirror_valid = true;
    if (e->cand_on) {
        const int m_s = e->d.search_arc_num;
        e->h_src.assign(source, source + m_s);
        e->h_tgt.assign(target, target + m_s);
        e->h_cost.assign(cost, cost + m_s);
        e->h_state.assign(state, state + m_s);
        cand_build_adjacency(e);
        e->node_at.assign(n, 0u);
        e->arc_at.assign(m_s, 0u);
        e->cand_now = 1;
        e->snap_at = 0;
        e->heap_gap = 0;
        e->async_posted = false;
        e->sync_nodes.clear(); e->sync_arcs.clear(); blind_clear(e);
        e->rc_sync.clear(); e->rc_shift_unknown = false;
        cand_reset(e);
        e->heap_gap = 0;
        e->cand_now = e->cand_epoch0;
    }
    // the pending lists grow to a subtree's size: get (and touch) their memory now, not in the middle of a solve
    e->pend_node.assign((size_t)e->patch_capacity, 0); e->pend_val.assign((size_t)e->patch_capacity, 0);
    pend_clear(e);
    e->next_arc = 0;
    e->uploaded = true;
    return MCF_OK;
}

int mcf_engine_patch_state(mcf_engine *e, int32_t count, const int32_t *arcs, const int8_t *states)
{
    if (!e || count < 0 || (count && (!arcs || !states))) return mcf::fail(MCF_ERR_INVALID, "mcf_engine_patch_state: bad arguments");
    for (int i = 0; i < count; ++i) {
        if (arcs[i] < 0 || arcs[i] >= e->d.arc_capacity) return mcf::fail(MCF_ERR_INVALID, "arc %d out of range", arcs[i]);
        if (states[i] < -1 || states[i] > 1) return mcf::fail(MCF_ERR_INVALID, "state %d is not -1/0/1", states[i]);
        if (arcs[i] < e->begin || arcs[i] >= e->end) continue;   // not resident here (outside the search range or another shard)
        if (e->cand_on) {
            const int a = arcs[i];
            e->h_state[a] = states[i];
            for (int side = 0; side < 2; ++side) {             // the copies of the state beside the arc's two adjacency entries
                const int q = e->adj_pos[2 * (size_t)a + side];
                if (q >= 0) e->adj[q].other = (e->adj[q].other & ~(3u << 29)) | ((uint32_t)(states[i] + 1) << 29);
            }
            cand_note_arc(e, a);
            continue;
        }
        // the device addresses state[] by position: begin + position of the arc in the stored order
        if (e->bucket_nodes > 0 && e->pos_of.empty()) return mcf::fail(MCF_ERR_STATE, "mcf_engine_upload has not been called");
        const int32_t where = e->bucket_nodes > 0 ? e->begin + e->pos_of[arcs[i] - e->begin] : arcs[i];
        bool dup = false;
        for (size_t j = 0; j < e->pend_arc.size(); ++j)
            if (e->pend_arc[j] == where) { e->pend_state[j] = states[i]; dup = true; }
        if (dup) continue;
        // Dispatch mode ships long lists with update_kernel, in stream order before the next scan.  A resident grid would only run that
        // kernel after it has left (and would have scanned with stale state meanwhile): there the list simply grows -- the mailbox
        // carries up to mailbox_max_st state patches and search_begin stops the grid first for anything longer.
        if (!e->resident_ok && (int)e->pend_arc.size() >= 64) { int rc = flush_pending(e); if (rc) return rc; }
        e->pend_arc.push_back(where);
        e->pend_state.push_back(states[i]);
    }
    return MCF_OK;
}

}  // extern "C"
namespace { int list_merge_potentials(mcf_engine *e, int32_t count, const int32_t *nodes, const int64_t *values); }
extern "C" {

int mcf_engine_update_potential(mcf_engine *e, int32_t count, const int32_t *nodes, int64_t sigma)
{
    if (!e || count < 0 || (count && !nodes)) return mcf::fail(MCF_ERR_INVALID, "mcf_engine_update_potential: bad arguments");
    if (!e->uploaded) return mcf::fail(MCF_ERR_STATE, "mcf_engine_upload has not been called");
    if (count == 0) return MCF_OK;
    if (e->ext_pi) return mcf::fail(MCF_ERR_STATE, "the potentials are bound to the caller's array (mcf_engine_bind_potentials): pass the new values with set / append / shift_potential");
    if (!e->mirror_valid) {          // the caller switched from set_potential to += sigma: fetch the current values once
        int rc = mcf_engine_download_pi(e, e->pi.data());
        if (rc) return rc;
        e->mirror_valid = true;
    }
    if (e->cand_on) {
        for (int i = 0; i < count; ++i) {
            if ((unsigned)nodes[i] >= (unsigned)e->d.node_count) return mcf::fail(MCF_ERR_INVALID, "node %d out of range", nodes[i]);
            if (e->d.int_width == 32 && !fits32(e->pi[nodes[i]] + sigma)) return mcf::fail(MCF_ERR_OVERFLOW, "potential of node %d leaves int32; create the engine with int_width 64", nodes[i]);
        }
        if (count > kCandMaxNodes || e->pivot_overflow) {
            std::vector<int64_t> vals((size_t)count);
            for (int i = 0; i < count; ++i) vals[i] = (e->pi[nodes[i]] += sigma);
            const bool first = e->blind_count == 0;
            e->pend_shift = first;            // one list with one shift (known before the list starts travelling)
            e->pend_sigma = sigma;
            const int rcn = cand_note_nodes_blind(e, count, nodes, vals.data(), false);
            if (rcn) return rcn;
        } else {
            for (int i = 0; i < count; ++i) { e->pi[nodes[i]] += sigma; cand_note_node(e, nodes[i], true, sigma); }
        }
        e->st.potential_nodes += count;
        return MCF_OK;
    }
    if (e->list_rule) {                 // merged per node with what is queued already
        std::vector<int64_t> vals((size_t)count);
        for (int i = 0; i < count; ++i) {
            if ((unsigned)nodes[i] >= (unsigned)e->d.node_count) return mcf::fail(MCF_ERR_INVALID, "node %d out of range", nodes[i]);
            vals[i] = e->pi[nodes[i]] + sigma;
        }
        const int rc = list_merge_potentials(e, count, nodes, vals.data());
        if (rc) return rc;
        for (int i = 0; i < count; ++i) e->pi[nodes[i]] = vals[i];
        e->mirror_valid = true;
        return MCF_OK;
    }
    // one list per dispatch: a second list may repeat nodes of the first
    if (!e->pend_node.empty()) { int rc = resident_stop(e); if (!rc) rc = flush_pending(e); if (rc) return rc; }
    if (count > e->d.node_count) return mcf::fail(MCF_ERR_INVALID, "%d nodes in a graph of %d", count, e->d.node_count);
    e->pend_node.resize(count);
    e->pend_val.resize(count);
    for (int i = 0; i < count; ++i) {
        const int u = nodes[i];
        if ((unsigned)u >= (unsigned)e->d.node_count) { pend_clear_potentials(e); return mcf::fail(MCF_ERR_INVALID, "node %d out of range", u); }
        const int64_t v = e->pi[u] + sigma;
        if (e->d.int_width == 32 && !fits32(v)) { pend_clear_potentials(e); return mcf::fail(MCF_ERR_OVERFLOW, "potential of node %d leaves int32; create the engine with int_width 64", u); }
        e->pend_node[i] = u;
        e->pend_val[i] = v;
    }
    for (int i = 0; i < count; ++i) e->pi[nodes[i]] = e->pend_val[i];
    e->pend_shift = true;
    e->pend_sigma = sigma;
    e->st.potential_nodes += count;
    return MCF_OK;
}

}  // extern "C"

namespace {

// the nodes of a list are inside the graph (and, for 32-bit engines, their values inside int32); values == nullptr: the bound array holds them
int check_potential_list(mcf_engine *e, int32_t count, const int32_t *nodes, const int64_t *values)
{
    const uint32_t n = (uint32_t)e->d.node_count;
    uint32_t beyond = 0;
    for (int i = 0; i < count; ++i) beyond |= (uint32_t)((uint32_t)nodes[i] >= n);      // no early exit: the loop vectorises
    if (beyond) for (int i = 0; i < count; ++i) if ((uint32_t)nodes[i] >= n) return mcf::fail(MCF_ERR_INVALID, "node %d out of range", nodes[i]);
    if (e->d.int_width == 32)
        for (int i = 0; i < count; ++i)
            if (!fits32(values ? values[i] : e->ext_pi[nodes[i]])) return mcf::fail(MCF_ERR_OVERFLOW, "potential of node %d leaves int32; create the engine with int_width 64", nodes[i]);
    return MCF_OK;
}

// appends `count` values to pend_val: the caller's, or the bound array's
void pend_values_append(mcf_engine *e, int32_t count, const int32_t *nodes, const int64_t *values)
{
    if (values) { e->pend_val.insert(e->pend_val.end(), values, values + count); return; }
    const size_t at = e->pend_val.size();
    e->pend_val.resize(at + (size_t)count);
    for (int i = 0; i < count; ++i) e->pend_val[at + i] = e->ext_pi[nodes[i]];
}

// list rules: the entries join the pending list, one per node -- a node already in it takes the new value (the lists of several pivots, in order)
int list_merge_potentials(mcf_engine *e, int32_t count, const int32_t *nodes, const int64_t *values)
{
    if (const int rcc = check_potential_list(e, count, nodes, values)) return rcc;
    for (int i = 0; i < count; ++i) {
        const int32_t u = nodes[i];
        const int64_t v = values ? values[i] : e->ext_pi[u];
        const uint32_t q = (uint32_t)e->pend_index[u];
        if (q < e->pend_node.size() && e->pend_node[q] == u) { e->pend_val[q] = v; continue; }
        e->pend_index[u] = (int32_t)e->pend_node.size();
        e->pend_node.push_back(u);
        e->pend_val.push_back(v);
    }
    e->pend_shift = false;
    e->mirror_valid = false;
    e->st.potential_nodes += count;
    return MCF_OK;
}

int set_potential_impl(mcf_engine *e, int32_t count, const int32_t *nodes, const int64_t *values)
{
    if (!e->uploaded) return mcf::fail(MCF_ERR_STATE, "mcf_engine_upload has not been called");
    if (count == 0) return MCF_OK;
    if (count > e->d.node_count) return mcf::fail(MCF_ERR_INVALID, "%d nodes in a graph of %d", count, e->d.node_count);
    if (const int rcc = check_potential_list(e, count, nodes, values)) return rcc;
    if (e->cand_on) {                 // the mirror stays authoritative in candidate mode
        if (!e->ext_pi) for (int i = 0; i < count; ++i) e->pi[nodes[i]] = values[i];      // bound potentials: the caller's array already holds them
        if (count > kCandMaxNodes || e->pivot_overflow) {
            const bool first = e->blind_count == 0;
            // the big list has ONE shift when every piece of it came with the same announced shift (decided before the piece starts travelling)
            e->pend_shift = e->call_shift_known && (first || (e->pend_shift && e->pend_sigma == e->call_shift));
            e->pend_sigma = e->call_shift;
            const int rcn = cand_note_nodes_blind(e, count, nodes, values, e->cand_appending);
            if (rcn) return rcn;
        }
        else for (int i = 0; i < count; ++i) cand_note_node(e, nodes[i], e->call_shift_known, e->call_shift);
        e->st.potential_nodes += count;
        return MCF_OK;
    }
    if (e->list_rule) return list_merge_potentials(e, count, nodes, values);
    if (!e->pend_node.empty()) { int rc = resident_stop(e); if (!rc) rc = flush_pending(e); if (rc) return rc; }
    e->pend_node.assign(nodes, nodes + count);
    e->pend_val.clear();
    pend_values_append(e, count, nodes, values);
    e->pend_shift = false;
    e->mirror_valid = false;
    e->st.potential_nodes += count;
    resident_stream(e);       // a long list starts travelling now; the search only has to finish it
    return MCF_OK;
}

int append_potential_impl(mcf_engine *e, int32_t count, const int32_t *nodes, const int64_t *values)
{
    if (!e->uploaded) return mcf::fail(MCF_ERR_STATE, "mcf_engine_upload has not been called");
    if (count == 0) return MCF_OK;
    if (e->cand_on) {              // candidate mode takes any number of calls; a piece that continues this pivot's list repeats none of its nodes
        e->cand_appending = e->pivot_overflow && e->blind_count > 0 && e->blind_epoch == e->cand_now;
        const int rc = set_potential_impl(e, count, nodes, values);
        e->cand_appending = false;
        return rc;
    }
    if (e->list_rule || e->pend_node.empty()) return set_potential_impl(e, count, nodes, values);     // nothing queued yet / merged per node
    if ((int64_t)e->pend_node.size() + count > e->d.node_count) return mcf::fail(MCF_ERR_INVALID, "more nodes appended than the graph has: the lists of one pivot must not repeat nodes");
    if (const int rcc = check_potential_list(e, count, nodes, values)) return rcc;
    e->pend_node.insert(e->pend_node.end(), nodes, nodes + count);
    pend_values_append(e, count, nodes, values);
    e->pend_shift = false;
    e->mirror_valid = false;
    e->st.potential_nodes += count;
    resident_stream(e);
    return MCF_OK;
}

}  // namespace

extern "C" {

int mcf_engine_set_potential(mcf_engine *e, int32_t count, const int32_t *nodes, const int64_t *values)
{
    if (!e || count < 0 || (count && (!nodes || !values))) return mcf::fail(MCF_ERR_INVALID, "mcf_engine_set_potential: bad arguments");
    return set_potential_impl(e, count, nodes, values);
}

int mcf_engine_append_potential(mcf_engine *e, int32_t count, const int32_t *nodes, const int64_t *values)
{
    if (!e || count < 0 || (count && (!nodes || !values))) return mcf::fail(MCF_ERR_INVALID, "mcf_engine_append_potential: bad arguments");
    return append_potential_impl(e, count, nodes, values);
}

int mcf_engine_bind_potentials(mcf_engine *e, const int64_t *pi)
{
    if (!e) return mcf::fail(MCF_ERR_INVALID, "mcf_engine_bind_potentials: null engine");
    if (e->in_flight != mcf_engine::kNoSearch) return mcf::fail(MCF_ERR_STATE, "mcf_engine_bind_potentials: a search is in flight");
    // a running grid was launched with the old array's address among its arguments (it reloads from there): it leaves first
    if (e->resident_running) { (void)hipSetDevice(e->d.device); const int rcs = resident_stop(e); if (rcs) return rcs; }
    if (e->ext_pi && e->ext_pi_pinned) host_unpin(e->ext_pi);
    e->ext_pi_pinned = false;
    e->reload_pi = false;
    e->ext_pi = pi;
    if (!pi) e->mirror_valid = false;
    // RC layout, 64-bit potentials: the array is made known to HIP so that a reload (mcf_engine_reload_potentials) is one asynchronous copy.
    // Several engines of one solver bind the same array: the first registers it, the others find it registered.
    e->d_ext_pi = nullptr;
    if (pi && (e->rc_mode || (e->shift_grid && e->shift_reload_min > 0)) && e->d.int_width == 64) {
        (void)hipSetDevice(e->d.device);
        e->ext_pi_pinned = host_pin(pi, sizeof(int64_t) * (size_t)e->d.node_count);
        if (e->ext_pi_pinned && e->resident_ok) {
            void *dp = nullptr;
            if (e->d_barrier && hipHostGetDevicePointer(&dp, const_cast<int64_t *>(pi), 0) == hipSuccess) e->d_ext_pi = (const int64_t *)dp;
            (void)hipGetLastError();
        }
    }
    return MCF_OK;
}

int mcf_engine_reload_threshold(mcf_engine *e, int32_t *min_nodes)
{
    if (!e || !min_nodes) return mcf::fail(MCF_ERR_INVALID, "mcf_engine_reload_threshold: null argument");
    *min_nodes = (e->rc_mode && e->ext_pi && e->ext_pi_pinned && e->rc_recompute_above < INT32_MAX) ? e->rc_recompute_above + 1 : 0;
    if (e->shift_grid && e->ext_pi && e->ext_pi_pinned && e->d_ext_pi && e->shift_reload_min > 0) *min_nodes = e->shift_reload_min;
    return MCF_OK;
}

int mcf_engine_reload_potentials(mcf_engine *e, int32_t changed_nodes)
{
    if (!e || changed_nodes < 0) return mcf::fail(MCF_ERR_INVALID, "mcf_engine_reload_potentials: bad arguments");
    if (!e->uploaded) return mcf::fail(MCF_ERR_STATE, "mcf_engine_upload has not been called");
    if (!((e->rc_mode || (e->shift_grid && e->d_ext_pi)) && e->ext_pi && e->ext_pi_pinned)) return mcf::fail(MCF_ERR_STATE, "mcf_engine_reload_potentials: this engine takes node lists (see mcf_engine_reload_threshold)");
    if (e->in_flight == mcf_engine::kResidentSearch || e->in_flight == mcf_engine::kCandSearch || e->in_flight == mcf_engine::kDispatchSearch) {
        // the array must not change while a search reads from it: the caller is between two searches by contract; an answered one may still wait to be fetched
        return mcf::fail(MCF_ERR_STATE, "mcf_engine_reload_potentials: a search is in flight");
    }
    // every potential change that is still waiting for the device is part of the array: the lists are dropped, the state writes stay
    if (e->stream_lines > 0) { const int rc = resident_stop(e); if (rc) return rc; }
    pend_clear_potentials(e);
    e->pend_shift = false;
    if (e->cand_on) {
        e->pivot_overflow = true;           // nothing is evaluated on the host: the device searches next (cand_absorb_pivot notes the gap)
        e->sync_nodes.clear();
        e->rc_sync.clear();
        e->rc_shift_unknown = false;
        blind_clear(e);
    }
    e->reload_pi = true;
    e->mirror_valid = false;
    e->st.potential_nodes += changed_nodes;
    return MCF_OK;
}

int mcf_engine_shift_potential(mcf_engine *e, int32_t count, const int32_t *nodes, const int64_t *values, int64_t sigma)
{
    if (!e || count < 0 || (count && !nodes)) return mcf::fail(MCF_ERR_INVALID, "mcf_engine_shift_potential: bad arguments");
    if (count && !values && !e->ext_pi) return mcf::fail(MCF_ERR_INVALID, "mcf_engine_shift_potential: values may only be left out when the potentials are bound (mcf_engine_bind_potentials)");
    const bool first = e->pend_node.empty();
    const bool same = first || (e->pend_shift && e->pend_sigma == sigma);
    e->call_shift_known = true;
    e->call_shift = sigma;
    const int rc = append_potential_impl(e, count, nodes, values);
    e->call_shift_known = false;
    if (rc) return rc;
    if (count > 0 && !e->cand_on) { e->pend_shift = same; e->pend_sigma = sigma; }
    return MCF_OK;
}

int mcf_engine_shift_potential_runs(mcf_engine *e, int32_t n_runs, const int32_t *first, const int32_t *length, int64_t sigma)
{
    if (!e || n_runs < 0 || (n_runs && (!first || !length))) return mcf::fail(MCF_ERR_INVALID, "mcf_engine_shift_potential_runs: bad arguments");
    if (!e->uploaded) return mcf::fail(MCF_ERR_STATE, "mcf_engine_upload has not been called");
    if (n_runs && !e->ext_pi) return mcf::fail(MCF_ERR_INVALID, "mcf_engine_shift_potential_runs: the potentials must be bound (mcf_engine_bind_potentials): the runs carry no values");
    int64_t total = 0;
    for (int r = 0; r < n_runs; ++r) {
        if (first[r] < 0 || length[r] <= 0 || (int64_t)first[r] + length[r] > e->d.node_count) return mcf::fail(MCF_ERR_INVALID, "run %d: nodes [%d, %d + %d) outside the graph", r, first[r], first[r], length[r]);
        total += length[r];
    }
    if (total > e->d.node_count) return mcf::fail(MCF_ERR_INVALID, "%lld nodes in a graph of %d: the runs of one pivot must not overlap", (long long)total, e->d.node_count);
    if (total == 0) return MCF_OK;
    if (e->cand_on && e->shift_grid && e->d.int_width == 64 && (total > kCandMaxNodes || e->pivot_overflow)) {
        // the register-resident candidate grid takes the pairs as they are (seven to a line instead of fifteen node ids)
        const bool first_list = e->blind_count == 0;
        e->pend_shift = first_list || (e->pend_shift && e->pend_sigma == sigma);
        e->pend_sigma = sigma;
        const bool continuation = e->pivot_overflow && e->blind_count > 0 && e->blind_epoch == e->cand_now;
        const int rc = cand_note_runs_blind(e, n_runs, first, length, total, continuation);
        if (rc) return rc;
        e->st.potential_nodes += total;
        return MCF_OK;
    }
    // every other engine: the same list as node ids
    std::vector<int32_t> ids;
    ids.reserve((size_t)total);
    for (int r = 0; r < n_runs; ++r) for (int k = 0; k < length[r]; ++k) ids.push_back(first[r] + k);
    return mcf_engine_shift_potential(e, (int32_t)total, ids.data(), nullptr, sigma);
}

int mcf_engine_patch_arcs(mcf_engine *e, int32_t count, const int32_t *arcs, const int32_t *source, const int32_t *target, const int64_t *cost)
{
    if (!e || count < 0 || (count && (!arcs || !source || !target || !cost))) return mcf::fail(MCF_ERR_INVALID, "mcf_engine_patch_arcs: bad arguments");
    HIP_TRY(hipSetDevice(e->d.device));
    int rc = resident_stop(e);
    if (!rc) rc = flush_pending(e);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));
    bool cand_touched = false;
    for (int i = 0; i < count; ++i) {
        const int a = arcs[i];
        if (a < 0 || a >= e->d.arc_capacity) return mcf::fail(MCF_ERR_INVALID, "arc %d out of range", a);
        if ((unsigned)source[i] >= (unsigned)e->d.node_count || (unsigned)target[i] >= (unsigned)e->d.node_count) return mcf::fail(MCF_ERR_INVALID, "arc %d: end point out of range", a);
        if (a < e->begin || a >= e->end) continue;
        if (e->bucket_nodes > 0 && e->pos_of.empty()) return mcf::fail(MCF_ERR_STATE, "mcf_engine_upload has not been called");
        const int l = e->bucket_nodes > 0 ? e->pos_of[a - e->begin] : a - e->begin;     // the arc keeps its position even if its target leaves the range
        if (e->cand_on) { e->h_src[a] = source[i]; e->h_tgt[a] = target[i]; e->h_cost[a] = cost[i]; cand_touched = true; }
        HIP_TRY(hipMemcpy(e->d_src + l, &source[i], 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(e->d_tgt + l, &target[i], 4, hipMemcpyHostToDevice));
        if (e->d.int_width == 32) {
            if (!fits32(cost[i])) return mcf::fail(MCF_ERR_OVERFLOW, "cost of arc %d does not fit int32", a);
            const int32_t c = (int32_t)cost[i];
            HIP_TRY(hipMemcpy((int32_t *)e->d_cost + l, &c, 4, hipMemcpyHostToDevice));
        } else {
            HIP_TRY(hipMemcpy((int64_t *)e->d_cost + l, &cost[i], 8, hipMemcpyHostToDevice));
        }
    }
    if (cand_touched) {      // the candidate cache's mirrors: new arc lists, and nothing it knew about keys holds any more
        cand_build_adjacency(e);
        cand_reset(e);
        e->async_posted = false;
    }
    if (e->rc_mode) {        // end points and costs changed: the arcs' reduced costs and the nodes' arc lists are rebuilt from the device arrays
        const int cnt = e->end - e->begin;
        std::vector<int32_t> s2((size_t)std::max(1, cnt)), t2((size_t)std::max(1, cnt));
        HIP_TRY(hipMemcpy(s2.data(), e->d_src, sizeof(int32_t) * cnt, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(t2.data(), e->d_tgt, sizeof(int32_t) * cnt, hipMemcpyDeviceToHost));
        int rcr = rc_build_adjacency(e, s2.data(), t2.data());
        if (!rcr) rcr = rc_recompute(e);
        if (rcr) return rcr;
        HIP_TRY(hipStreamSynchronize(e->stream));
    }
    return MCF_OK;
}

int mcf_engine_check_reduced_costs(mcf_engine *e, int64_t *mismatches, int32_t *first_arc)
{
    if (!e || !mismatches) return mcf::fail(MCF_ERR_INVALID, "mcf_engine_check_reduced_costs: null argument");
    *mismatches = 0;
    if (first_arc) *first_arc = -1;
    if (!e->rc_mode) return MCF_OK;
    HIP_TRY(hipSetDevice(e->d.device));
    int rc = resident_stop(e);
    if (!rc) rc = flush_pending(e);
    if (rc) return rc;
    unsigned long long *d_bad = nullptr;
    HIP_TRY(hipMalloc((void **)&d_bad, 16));
    const int big = INT32_MAX;
    HIP_TRY(hipMemsetAsync(d_bad, 0, 8, e->stream));
    HIP_TRY(hipMemcpyAsync((char *)d_bad + 8, &big, 4, hipMemcpyHostToDevice, e->stream));
    const int count = e->end - e->begin, blocks = (count + kThreads - 1) / kThreads;
    if (count > 0)
        with_width(e, [&](auto width) {
            using T = decltype(width);
            launch(rc_check_kernel<T>, dim3(blocks), dim3(kThreads), e->stream, nullptr, nullptr, e->d_src, e->d_tgt, (const T *)e->d_cost, (const T *)e->d_pi, e->d_rc, count, d_bad, (int *)((char *)d_bad + 8));
        });
    unsigned long long bad = 0; int first = 0;
    hipError_t err = hipMemcpyAsync(&bad, d_bad, 8, hipMemcpyDeviceToHost, e->stream);
    if (err == hipSuccess) err = hipMemcpyAsync(&first, (char *)d_bad + 8, 4, hipMemcpyDeviceToHost, e->stream);
    if (err == hipSuccess) err = hipStreamSynchronize(e->stream);
    (void)hipFree(d_bad);
    if (err != hipSuccess) return mcf::fail(MCF_ERR_HIP, "mcf_engine_check_reduced_costs: %s", hipGetErrorString(err));
    *mismatches = (int64_t)bad;
    if (first_arc && bad) *first_arc = e->begin + first;
    return MCF_OK;
}

int mcf_engine_can_renumber(mcf_engine *e, int32_t *yes)
{
    if (!e || !yes) return mcf::fail(MCF_ERR_INVALID, "mcf_engine_can_renumber: null argument");
    // not the bucketed layout (it orders its arcs by target id); and not an engine that shares its device with other solvers' grids: a
    // relabelling stops and restarts the resident grid, and a grid that comes back while the CUs are full of the others' workgroups waits for
    // them -- four solves in flight fell from 350 k to 190 k pivots/s together when their grids kept leaving and re-entering
    *yes = (e->bucket_nodes > 0 || (e->d.flags & MCF_ENGINE_SHARE_DEVICE)) ? 0 : 1;
    return MCF_OK;
}

int mcf_engine_renumber_nodes(mcf_engine *e, const int32_t *new_of)
{
    if (!e || !new_of) return mcf::fail(MCF_ERR_INVALID, "mcf_engine_renumber_nodes: null argument");
    if (!e->uploaded) return mcf::fail(MCF_ERR_STATE, "mcf_engine_upload has not been called");
    if (e->bucket_nodes > 0) return mcf::fail(MCF_ERR_STATE, "mcf_engine_renumber_nodes: the bucketed layout orders its arcs by target id (mcf_engine_can_renumber)");
    if (e->in_flight != mcf_engine::kNoSearch) return mcf::fail(MCF_ERR_STATE, "mcf_engine_renumber_nodes: a search is in flight");
    const int n = e->d.node_count;
    {   // a permutation of [0, n)?
        std::vector<uint8_t> seen((size_t)n, 0);
        for (int u = 0; u < n; ++u) {
            if ((unsigned)new_of[u] >= (unsigned)n || seen[new_of[u]]) return mcf::fail(MCF_ERR_INVALID, "mcf_engine_renumber_nodes: not a permutation (node %d)", u);
            seen[new_of[u]] = 1;
        }
    }
    HIP_TRY(hipSetDevice(e->d.device));
    // everything the device has not heard yet goes out under the old ids; a bound potential array has been permuted by its owner already,
    // so what is pending of it is dropped and the whole array is copied below
    int rc = resident_stop(e);
    if (rc) return rc;
    if (e->ext_pi) {
        pend_clear_potentials(e); e->pend_shift = false;
        e->reload_pi = false;
        if (e->cand_on) { e->sync_nodes.clear(); e->rc_sync.clear(); e->rc_shift_unknown = false; blind_clear(e); }
    }
    rc = flush_pending(e);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));
    // device: end points, potentials.  (The map's buffer is kept: hipMalloc / hipFree synchronise the whole device, and other solvers' resident
    // grids on it only leave when their solves end -- four solves in flight took 2.9 s each instead of 0.8 while this allocated per call.)
    if (!e->d_node_map) HIP_TRY(hipMalloc((void **)&e->d_node_map, sizeof(int32_t) * (size_t)n));
    hipError_t err = hipMemcpyAsync(e->d_node_map, new_of, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, e->stream);
    if (err == hipSuccess) {
        hipLaunchKernelGGL(renumber_kernel, dim3(e->count_padded / kThreads), dim3(kThreads), 0, e->stream, e->d_src, e->d_tgt, e->d_node_map, e->count_padded);
        err = hipGetLastError();
    }
    if (err == hipSuccess) err = hipStreamSynchronize(e->stream);
    if (err != hipSuccess) return mcf::fail(MCF_ERR_HIP, "mcf_engine_renumber_nodes: %s", hipGetErrorString(err));
    if (!e->ext_pi) {
        if (!e->mirror_valid) { rc = mcf_engine_download_pi(e, e->pi.data()); if (rc) return rc; e->mirror_valid = true; }
        mcf::hvec<int64_t> moved((size_t)n);
        for (int u = 0; u < n; ++u) moved[new_of[u]] = e->pi[u];
        std::copy(moved.begin(), moved.end(), e->pi.begin());
    }
    {
        const int64_t *pi = e->ext_pi ? e->ext_pi : e->pi.data();
        if (e->d.int_width == 32) {
            std::vector<int32_t> p32((size_t)n);
            for (int u = 0; u < n; ++u) { if (!fits32(pi[u])) return mcf::fail(MCF_ERR_OVERFLOW, "potential of node %d does not fit int32", u); p32[u] = (int32_t)pi[u]; }
            HIP_TRY(hipMemcpyAsync(e->d_pi, p32.data(), sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, e->stream));
            HIP_TRY(hipStreamSynchronize(e->stream));
        } else {
            HIP_TRY(hipMemcpyAsync(e->d_pi, pi, sizeof(int64_t) * (size_t)n, hipMemcpyHostToDevice, e->stream));
            HIP_TRY(hipStreamSynchronize(e->stream));
        }
    }
    // host mirrors of the candidate cache
    if (e->cand_on) {
        const int m_s = e->d.search_arc_num;
        for (int a = 0; a < m_s; ++a) { e->h_src[a] = new_of[e->h_src[a]]; e->h_tgt[a] = new_of[e->h_tgt[a]]; }
        cand_build_adjacency(e);
        cand_renumber(e, new_of, n);
        for (int32_t &u : e->sync_nodes) u = new_of[u];
        for (auto &x : e->rc_sync) x.node = new_of[x.node];
    }
    // RC layout: the reduced costs stay where they are (same arcs, same values); the nodes' arc lists are keyed by node id
    if (e->rc_mode) {
        const int cnt = e->end - e->begin;
        std::vector<int32_t> s2((size_t)std::max(1, cnt)), t2((size_t)std::max(1, cnt));
        if (e->cand_on) { std::copy(e->h_src.begin() + e->begin, e->h_src.begin() + e->end, s2.begin()); std::copy(e->h_tgt.begin() + e->begin, e->h_tgt.begin() + e->end, t2.begin()); }
        else {
            HIP_TRY(hipMemcpy(s2.data(), e->d_src, sizeof(int32_t) * cnt, hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(t2.data(), e->d_tgt, sizeof(int32_t) * cnt, hipMemcpyDeviceToHost));
        }
        rc = rc_build_adjacency(e, s2.data(), t2.data());
        // potential changes that were dropped above in favour of the whole array never reached the per-arc reduced costs: all of them again
        if (!rc) rc = rc_recompute(e);
        if (rc) return rc;
        HIP_TRY(hipStreamSynchronize(e->stream));
    }
    e->st.renumberings += 1;
    return MCF_OK;
}

int mcf_engine_find_entering(mcf_engine *e, int32_t *found, int32_t *arc, int64_t *reduced_cost)
{
    if (!e || !found || !arc) return mcf::fail(MCF_ERR_INVALID, "mcf_engine_find_entering: null argument");
    if (e->begin != 0 || e->end != e->d.search_arc_num) return mcf::fail(MCF_ERR_STATE, "sharded engine: use mcf_engine_find_entering_local / _sharded");
    Key k;
    int rc = local_search(e, &k);
    if (rc) return rc;
    resolve_key(e, k, found, arc, reduced_cost);
    return MCF_OK;
}

int mcf_engine_search_begin(mcf_engine *e)
{
    if (!e) return mcf::fail(MCF_ERR_INVALID, "mcf_engine_search_begin: null argument");
    return search_begin(e);
}

int mcf_engine_search_end(mcf_engine *e, int32_t *found, int32_t *arc, int64_t *reduced_cost)
{
    if (!e || !found || !arc) return mcf::fail(MCF_ERR_INVALID, "mcf_engine_search_end: null argument");
    if (e->begin != 0 || e->end != e->d.search_arc_num) return mcf::fail(MCF_ERR_STATE, "sharded engine: use mcf_engine_search_end_local + mcf_engine_resolve");
    Key k;
    const int rc = search_end(e, &k);
    if (rc) return rc;
    resolve_key(e, k, found, arc, reduced_cost);
    return MCF_OK;
}

namespace {
void key_to_candidate(const mcf_engine *e, const Key &k, mcf_candidate *out)
{
    out->reduced_cost = k.p == kNone ? 0 : k.c;
    out->pos = k.p;
    const SearchHeader h = search_header(e);
    const int na = h.next_arc;
    if (k.p == kNone) out->arc = -1;
    else if (e->d.rule == MCF_RULE_BEST_ELIGIBLE) out->arc = (int32_t)k.p;
    else out->arc = (int32_t)(((int64_t)k.p + na) % e->d.search_arc_num);
    const bool dual = h.dual && e->range_key.p != kNone;
    out->range_cost = dual ? e->range_key.c : 0;
    out->range_pos = dual ? e->range_key.p : kNone;
    out->range_arc = dual ? (int32_t)(((int64_t)e->range_key.p + na) % e->d.search_arc_num) : -1;
}
}  // namespace

int mcf_engine_search_end_local(mcf_engine *e, mcf_candidate *out)
{
    if (!e || !out) return mcf::fail(MCF_ERR_INVALID, "mcf_engine_search_end_local: null argument");
    Key k;
    const int rc = search_end(e, &k);
    if (rc) return rc;
    key_to_candidate(e, k, out);
    return MCF_OK;
}

int mcf_engine_find_entering_local(mcf_engine *e, mcf_candidate *out)
{
    if (!e || !out) return mcf::fail(MCF_ERR_INVALID, "mcf_engine_find_entering_local: null argument");
    Key k;
    int rc = local_search(e, &k);
    if (rc) return rc;
    key_to_candidate(e, k, out);
    return MCF_OK;
}

int mcf_engine_resolve(mcf_engine *e, int32_t count, const mcf_candidate *all, int32_t *found, int32_t *arc, int64_t *reduced_cost)
{
    if (!e || count < 0 || (count && !all) || !found || !arc) return mcf::fail(MCF_ERR_INVALID, "mcf_engine_resolve: bad arguments");
    const Key best = merge_candidates(e->d.rule, e->d.semantics, e->d.search_arc_num, e->block_size, e->next_arc, count, all, &e->range_key);
    resolve_key(e, best, found, arc, reduced_cost);
    return MCF_OK;
}

int mcf_resolve_candidates(int32_t rule, int32_t semantics, int32_t vector_width, int32_t search_arc_num, int32_t block_size, int32_t *next_arc,
                           int32_t count, const mcf_candidate *all, int32_t *found, int32_t *arc, int64_t *reduced_cost)
{
    if (!next_arc || count < 0 || (count && !all) || !found || !arc || rule < 0 || rule > 2 || search_arc_num < 0 ||
        (semantics != MCF_SEM_PLAIN && semantics != MCF_SEM_OPTIMIZED) || *next_arc < 0 || *next_arc > search_arc_num ||
        (vector_width != MCF_VECTOR_DEFAULT && vector_width != MCF_VECTOR_NONE && vector_width != 2 && vector_width != 4 && vector_width != 8))
        return mcf::fail(MCF_ERR_INVALID, "mcf_resolve_candidates: bad arguments");
    const int B = block_size > 0 ? block_size : mcf::default_block_size(search_arc_num, semantics);
    const int vec = vector_width == MCF_VECTOR_NONE ? 0 : (vector_width == MCF_VECTOR_DEFAULT ? 4 : vector_width);
    Key range{0, kNone, kNone};
    const Key best = merge_candidates(rule, semantics, search_arc_num, B, *next_arc, count, all, &range);
    int na = *next_arc;
    resolve_key_raw(rule, semantics, vec, search_arc_num, B, na, best, range, found, arc, reduced_cost);
    *next_arc = na;
    return MCF_OK;
}

}  // extern "C"

// ---- the device half of LEMON's list rules (collect.hip.h)
namespace {
template <typename T>
int launch_collect(mcf_engine *e, const mcf_collect_request *rq, int capacity, int rounds, int n_tiles)
{
    CollectArgs<T> a;
    a.src = e->d_src; a.tgt = e->d_tgt; a.cost = (const T *)e->d_cost; a.state = e->d_state; a.pi = (const T *)e->d_pi;
    a.m_s = e->d.search_arc_num; a.next_arc = rq->next_arc; a.rounds = rounds; a.mode = rq->mode;
    a.limit = rq->mode == MCF_COLLECT_FIRST_N ? rq->limit : 0;
    a.block_size = rq->mode == MCF_COLLECT_BLOCKS ? rq->block_size : 0;
    a.head_length = rq->head_length; a.survivors = rq->survivors;
    launch(collect_count_kernel<T>, dim3(n_tiles), dim3(kCollectThreads), e->stream, nullptr, nullptr, a, e->d_tiles);
    HIP_TRY(hipGetLastError());
    launch(collect_emit_kernel<T>, dim3(n_tiles), dim3(kCollectThreads), e->stream, nullptr, nullptr, a, (const CollectTile *)e->d_tiles, n_tiles, e->d_collect, capacity,
           e->d_collect_hdr);
    HIP_TRY(hipGetLastError());
    return MCF_OK;
}
}  // namespace

extern "C" {

int mcf_engine_collect_eligible(mcf_engine *e, const mcf_collect_request *rq, int32_t capacity, int32_t *count, int32_t *arcs,
                                int64_t *reduced_costs, int32_t *end_arc, int64_t *arcs_scanned)
{
    if (!e || !rq || capacity < 0 || !count || !end_arc || (capacity > 0 && (!arcs || !reduced_costs)))
        return mcf::fail(MCF_ERR_INVALID, "mcf_engine_collect_eligible: bad arguments");
    if (!e->list_rule) return mcf::fail(MCF_ERR_STATE, "mcf_engine_collect_eligible: the engine was not created with a list rule (3, 4)");
    if (!e->uploaded) return mcf::fail(MCF_ERR_STATE, "mcf_engine_upload has not been called");
    const int m_s = e->d.search_arc_num;
    if (rq->mode == MCF_COLLECT_FIRST_N) {
        if (rq->limit < 1) return mcf::fail(MCF_ERR_INVALID, "mcf_engine_collect_eligible: limit %d < 1", rq->limit);
    } else if (rq->mode == MCF_COLLECT_BLOCKS) {
        if (rq->block_size < 1 || rq->head_length < 0 || rq->survivors < 0)
            return mcf::fail(MCF_ERR_INVALID, "mcf_engine_collect_eligible: block_size %d, head_length %d, survivors %d", rq->block_size, rq->head_length, rq->survivors);
    } else {
        return mcf::fail(MCF_ERR_INVALID, "mcf_engine_collect_eligible: mode %d", rq->mode);
    }
    if (m_s == 0 ? rq->next_arc != 0 : (rq->next_arc < 0 || rq->next_arc >= m_s))
        return mcf::fail(MCF_ERR_INVALID, "mcf_engine_collect_eligible: next_arc %d outside [0, %d)", rq->next_arc, m_s);
    const double t0 = (double)__rdtsc();
    HIP_TRY(hipSetDevice(e->d.device));
    int rc = flush_pending(e);                 // every queued state write and potential, in order, before the scan (same stream)
    if (rc) return rc;
    if (m_s == 0) { *count = 0; *end_arc = rq->next_arc; if (arcs_scanned) *arcs_scanned = 0; return MCF_OK; }
    if (e->collect_cap < std::max(capacity, 1)) {
        HIP_TRY(hipStreamSynchronize(e->stream));
        if (e->h_collect) { (void)hipHostFree(e->h_collect); e->h_collect = nullptr; e->d_collect = nullptr; e->collect_cap = 0; }
        const int cap = std::max({capacity, 1024, 2 * e->collect_cap});
        HIP_TRY(hipHostMalloc((void **)&e->h_collect, sizeof(CollectEntry) * (size_t)cap, hipHostMallocMapped | hipHostMallocCoherent));
        HIP_TRY(hipHostGetDevicePointer((void **)&e->d_collect, e->h_collect, 0));
        e->collect_cap = cap;
    }
    const int64_t per_round = (int64_t)kCollectThreads * kCollectMaxTiles;
    const int rounds = (int)std::max<int64_t>(4, ((int64_t)m_s + per_round - 1) / per_round);
    const int tile_len = rounds * kCollectThreads;
    const int n_tiles = (m_s + tile_len - 1) / tile_len;     // <= kCollectMaxTiles
    volatile CollectHeader *hdr = e->h_collect_hdr;
    hdr->count = -1;
    rc = with_width(e, [&](auto width) { return launch_collect<decltype(width)>(e, rq, capacity, rounds, n_tiles); });
    if (rc) return rc;
    const double t1 = (double)__rdtsc();
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->launch_ticks += t1 - t0;
    e->wait_ticks += (double)__rdtsc() - t1;
    const int32_t got = hdr->count;
    if (got < 0) return mcf::fail(MCF_ERR_HIP, "mcf_engine_collect_eligible: the scan left no answer");
    *count = got;
    *end_arc = hdr->end_arc;
    if (arcs_scanned) *arcs_scanned = hdr->arcs_scanned;
    e->st.scan_launches += 1;
    e->st.arcs_scanned += m_s;
    if (got > capacity) return mcf::fail(MCF_ERR_INVALID, "mcf_engine_collect_eligible: %d eligible arcs, capacity %d", got, capacity);
    for (int i = 0; i < got; ++i) { arcs[i] = e->h_collect[i].arc; reduced_costs[i] = e->h_collect[i].c; }
    return MCF_OK;
}

int mcf_engine_park(mcf_engine *e)
{
    if (!e) return mcf::fail(MCF_ERR_INVALID, "null argument");
    (void)hipSetDevice(e->d.device);
    return resident_stop(e);
}

int mcf_engine_get_next_arc(mcf_engine *e, int32_t *next_arc) { if (!e || !next_arc) return mcf::fail(MCF_ERR_INVALID, "null argument"); *next_arc = e->next_arc; return MCF_OK; }
int mcf_engine_set_next_arc(mcf_engine *e, int32_t next_arc)
{
    if (!e || next_arc < 0 || next_arc > e->d.search_arc_num) return mcf::fail(MCF_ERR_INVALID, "next_arc out of range");
    e->next_arc = next_arc;
    return MCF_OK;
}
int mcf_engine_get_block_size(mcf_engine *e, int32_t *b) { if (!e || !b) return mcf::fail(MCF_ERR_INVALID, "null argument"); *b = e->block_size; return MCF_OK; }

int mcf_engine_set_block_config(mcf_engine *e, const mcf_block_config *c, int32_t graph_node_count)
{
    if (!e || !c || graph_node_count < 0) return mcf::fail(MCF_ERR_INVALID, "mcf_engine_set_block_config: bad arguments");
    if (e->st.searches > 0 || e->in_flight != mcf_engine::kNoSearch) return mcf::fail(MCF_ERR_STATE, "mcf_engine_set_block_config: call before the first search");
    if (c->consecutive_hits_before_adapt < 0 || c->min_block_size < 0) return mcf::fail(MCF_ERR_INVALID, "mcf_engine_set_block_config: negative sizes");
    e->cfg = *c;
    e->cfg_set = true;
    e->low_hits = e->high_hits = 0;
    if (e->d.rule != MCF_RULE_BLOCK_SEARCH || e->d.semantics == MCF_SEM_OPTIMIZED) return MCF_OK;   // BSPO.cs:27-28 ignores the configuration
    int32_t b = 0, dyn_min = 0;
    const int rc = mcf_block_initial_size(c, e->d.search_arc_num, graph_node_count, &b, &dyn_min);      // NS.cs:1304-1336
    if (rc) return rc;
    e->dyn_min_block = dyn_min;
    if (e->d.block_size <= 0) e->block_size = std::max(1, b);
    e->st.initial_block_size = e->st.current_block_size = e->block_size;
    return MCF_OK;
}

int mcf_engine_download_pi(mcf_engine *e, int64_t *out)
{
    if (!e || !out) return mcf::fail(MCF_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(e->d.device));
    int rc = resident_stop(e);
    if (!rc) rc = flush_pending(e);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));
    const int n = e->d.node_count;
    if (e->d.int_width == 32) {
        std::vector<int32_t> t(n);
        HIP_TRY(hipMemcpy(t.data(), e->d_pi, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
        for (int i = 0; i < n; ++i) out[i] = t[i];
    } else {
        HIP_TRY(hipMemcpy(out, e->d_pi, sizeof(int64_t) * n, hipMemcpyDeviceToHost));
    }
    return MCF_OK;
}

int mcf_engine_download_state(mcf_engine *e, int8_t *out)
{
    if (!e || !out) return mcf::fail(MCF_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(e->d.device));
    int rc = resident_stop(e);
    if (!rc) rc = flush_pending(e);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (e->bucket_nodes > 0) {
        std::vector<int8_t> stored(e->end - e->begin);
        HIP_TRY(hipMemcpy(stored.data(), e->d_state, stored.size(), hipMemcpyDeviceToHost));
        for (int i = 0; i < e->end - e->begin; ++i) out[e->begin + i] = stored[e->pos_of[i]];
        return MCF_OK;
    }
    HIP_TRY(hipMemcpy(out + e->begin, e->d_state, e->end - e->begin, hipMemcpyDeviceToHost));
    return MCF_OK;
}

int mcf_engine_get_stats(mcf_engine *e, mcf_engine_stats *out)
{
    if (!e || !out) return mcf::fail(MCF_ERR_INVALID, "null argument");
    (void)hipSetDevice(e->d.device);
    int rc = resident_stop(e);
    if (!rc) rc = drain_events(e, true);
    if (rc) return rc;
    const double ns_per_tick = (mcf::now_ns() - e->cal_ns) / std::max(1.0, (double)__rdtsc() - e->cal_ticks);
    e->st.host_wait_ns = e->wait_ticks * ns_per_tick;
    e->st.host_launch_ns = e->launch_ticks * ns_per_tick;
    e->st.current_block_size = e->block_size;
    e->st.heap_compactions = e->n_heap_sweeps;
    *out = e->st;
    return MCF_OK;
}

int mcf_engine_reset_stats(mcf_engine *e)
{
    if (!e) return mcf::fail(MCF_ERR_INVALID, "null argument");
    (void)hipSetDevice(e->d.device);
    drain_events(e, true);
    const mcf_engine_stats keep = e->st;
    e->st = mcf_engine_stats{};
    e->wait_ticks = e->launch_ticks = 0;
    e->n_heap_sweeps = 0;
    e->st.scan_workgroups = keep.scan_workgroups;
    e->st.scan_threads = keep.scan_threads;
    e->st.bytes_per_scan = keep.bytes_per_scan;
    e->st.resident = keep.resident;
    e->st.candidates = keep.candidates;
    e->st.initial_block_size = keep.initial_block_size;
    e->st.current_block_size = e->block_size;
    e->st.comm_ranks = keep.comm_ranks;
    e->st.scan_bytes_read = keep.scan_bytes_read;
    e->st.rc_layout = keep.rc_layout;
    e->st.shift_grid = keep.shift_grid;
    return MCF_OK;
}

int mcf_engine_bench_scan(mcf_engine *e, int32_t reps, int32_t cold, int64_t flush_bytes, double *avg_ns, double *min_ns)
{
    if (!e || reps < 1 || !avg_ns || !min_ns) return mcf::fail(MCF_ERR_INVALID, "mcf_engine_bench_scan: bad arguments");
    if (e->list_rule) return mcf::fail(MCF_ERR_STATE, "engines of the list rules (3, 4) are searched with mcf_engine_collect_eligible only");
    if (!e->uploaded) return mcf::fail(MCF_ERR_STATE, "mcf_engine_upload has not been called");
    HIP_TRY(hipSetDevice(e->d.device));
    int rc = resident_stop(e);
    if (!rc) rc = flush_pending(e);
    if (rc) return rc;
    if (cold) {
        const size_t want = (size_t)std::max<int64_t>(flush_bytes, 1 << 20);
        if (e->flush_bytes < want) {
            (void)hipFree(e->d_flush);
            e->d_flush = nullptr;
            HIP_TRY(hipMalloc(&e->d_flush, want));
            HIP_TRY(hipMemset(e->d_flush, 0, want));
            e->flush_bytes = want;
        }
    }
    hipEvent_t a, b;
    HIP_TRY(hipEventCreate(&a));
    HIP_TRY(hipEventCreate(&b));
    double sum = 0, mn = 1e30;
    for (int r = 0; r < reps; ++r) {
        if (cold) hipLaunchKernelGGL(flush_kernel, dim3(2048), dim3(256), 0, e->stream, (uint4 *)e->d_flush, e->flush_bytes / 16);
        next_request(e);
        dispatch_search(e, false, a, b);      // same dispatch as a search, timed on the engine's stream; the records are simply not merged
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventSynchronize(b));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, a, b));
        sum += ms * 1e6;
        mn = std::min(mn, (double)ms * 1e6);
    }
    HIP_TRY(hipStreamSynchronize(e->stream));
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
    *avg_ns = sum / reps;
    *min_ns = mn;
    return MCF_OK;
}

// The potential update as a kernel of its own (what dispatch mode runs for lists that do not fit the scan's arguments, and what a stopped
// resident grid's engine falls back to): `count` distinct nodes get new values, `reps` times, each launch timed with HIP events on the
// engine's stream.  update_kernel moves 20 bytes per node (index 4, value 8 read; potential 8 written; 12 with 32-bit potentials);
// update_rc_kernel additionally walks the node's arc list (4 bytes per entry) and shifts each arc's reduced cost (8 read + 8 written).
// The values alternate between +1 and back, so the engine's state is what it was when the call returns (reps is rounded up to even).
int mcf_engine_bench_update(mcf_engine *e, int32_t count, int32_t reps, double *avg_ns, double *min_ns, int64_t *bytes)
{
    if (!e || count < 1 || count > e->d.node_count || reps < 1 || !avg_ns || !min_ns) return mcf::fail(MCF_ERR_INVALID, "mcf_engine_bench_update: bad arguments");
    if (!e->uploaded) return mcf::fail(MCF_ERR_STATE, "mcf_engine_upload has not been called");
    HIP_TRY(hipSetDevice(e->d.device));
    int rc = resident_stop(e);
    if (!rc) rc = flush_pending(e);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));
    const int n = e->d.node_count;
    std::vector<int64_t> cur((size_t)n);
    rc = mcf_engine_download_pi(e, cur.data());
    if (rc) return rc;
    // every (n / count)-th node: distinct, spread over the whole table
    std::vector<int32_t> nodes((size_t)count);
    const int64_t stride = std::max<int64_t>(1, n / count);
    for (int i = 0; i < count; ++i) nodes[i] = (int32_t)((i * stride) % n);
    std::sort(nodes.begin(), nodes.end());
    nodes.erase(std::unique(nodes.begin(), nodes.end()), nodes.end());
    const int k = (int)nodes.size();
    int32_t *d_nodes = nullptr; int64_t *d_vals[2] = {nullptr, nullptr};
    HIP_TRY(hipMalloc((void **)&d_nodes, sizeof(int32_t) * k));
    HIP_TRY(hipMalloc((void **)&d_vals[0], sizeof(int64_t) * k));
    HIP_TRY(hipMalloc((void **)&d_vals[1], sizeof(int64_t) * k));
    std::vector<int64_t> v0((size_t)k), v1((size_t)k);
    int64_t degree = 0;
    for (int i = 0; i < k; ++i) {
        v0[i] = cur[nodes[i]]; v1[i] = cur[nodes[i]] + (e->d.int_width == 32 && cur[nodes[i]] == INT32_MAX ? -1 : 1);
        if (e->rc_mode) degree += e->h_adj_start[nodes[i] + 1] - e->h_adj_start[nodes[i]];
    }
    HIP_TRY(hipMemcpy(d_nodes, nodes.data(), sizeof(int32_t) * k, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_vals[0], v0.data(), sizeof(int64_t) * k, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_vals[1], v1.data(), sizeof(int64_t) * k, hipMemcpyHostToDevice));
    hipEvent_t a, b;
    HIP_TRY(hipEventCreate(&a));
    HIP_TRY(hipEventCreate(&b));
    const int rounds = (reps + 1) / 2 * 2;
    double sum = 0, mn = 1e30;
    for (int r = 0; r < rounds; ++r) {
        const int64_t *vals = d_vals[(r + 1) & 1];          // +1 first, back second
        launch_list_update(e, e->rc_mode, a, b, d_nodes, vals, k, nullptr, nullptr, 0);
        hipError_t err = hipGetLastError();
        if (err == hipSuccess) err = hipEventSynchronize(b);
        float ms = 0.f;
        if (err == hipSuccess) err = hipEventElapsedTime(&ms, a, b);
        if (err != hipSuccess) { (void)hipFree(d_nodes); (void)hipFree(d_vals[0]); (void)hipFree(d_vals[1]); return mcf::fail(MCF_ERR_HIP, "mcf_engine_bench_update: %s", hipGetErrorString(err)); }
        sum += ms * 1e6;
        mn = std::min(mn, (double)ms * 1e6);
    }
    HIP_TRY(hipStreamSynchronize(e->stream));
    (void)hipEventDestroy(a); (void)hipEventDestroy(b);
    (void)hipFree(d_nodes); (void)hipFree(d_vals[0]); (void)hipFree(d_vals[1]);
    *avg_ns = sum / rounds;
    *min_ns = mn;
    if (bytes) *bytes = (int64_t)k * (e->d.int_width == 64 ? 20 : 12) + (e->rc_mode ? (int64_t)k * 8 + degree * 20 : 0);
    return MCF_OK;
}

// host wall time of a whole search (post / launch -> records merged) on the engine's resident arrays, `reps` times back to back without
// patches: the round trip a pivot waits for.  Works on whole and on sharded engines; next_arc is left alone.
int mcf_engine_bench_search(mcf_engine *e, int32_t reps, double *avg_ns, double *min_ns)
{
    if (!e || reps < 1 || !avg_ns || !min_ns) return mcf::fail(MCF_ERR_INVALID, "mcf_engine_bench_search: bad arguments");
    if (!e->uploaded) return mcf::fail(MCF_ERR_STATE, "mcf_engine_upload has not been called");
    HIP_TRY(hipSetDevice(e->d.device));
    Key k;
    struct Forced { mcf_engine *e; ~Forced() { e->force_device_search = false; } } forced{e};
    e->force_device_search = true;
    for (int r = 0; r < 16; ++r) { const int rc = local_search(e, &k); if (rc) return rc; }      // the grid is up, the caches are warm
    double sum = 0, mn = 1e30;
    for (int r = 0; r < reps; ++r) {
        const double t0 = mcf::now_ns();
        const int rc = local_search(e, &k);
        if (rc) return rc;
        const double dt = mcf::now_ns() - t0;
        sum += dt;
        mn = std::min(mn, dt);
    }
    *avg_ns = sum / reps;
    *min_ns = mn;
    return MCF_OK;
}

// ------------------------------------------------------------------------------------------------ RCCL exchange

int mcf_comm_unique_id(uint8_t id_out[128])
{
    RcclApi *r = rccl();
    if (!r) return mcf::fail(MCF_ERR_COMM, "librccl.so could not be loaded");
    Id128 id;
    const int rc = r->get_unique_id(&id);
    if (rc != 0) return mcf::fail(MCF_ERR_COMM, "ncclGetUniqueId: %s", r->error_string ? r->error_string(rc) : "error");
    memcpy(id_out, id.b, 128);
    return MCF_OK;
}

int mcf_engine_comm_init(mcf_engine *e, const uint8_t id[128], int32_t rank, int32_t world)
{
    if (!e || !id || world < 1 || rank < 0 || rank >= world) return mcf::fail(MCF_ERR_INVALID, "mcf_engine_comm_init: bad arguments");
    if (e->list_rule) return mcf::fail(MCF_ERR_STATE, "the list rules (3, 4) are not sharded");
    RcclApi *r = rccl();
    if (!r) return mcf::fail(MCF_ERR_COMM, "librccl.so could not be loaded");
    HIP_TRY(hipSetDevice(e->d.device));
    if (int rcs = resident_stop(e)) return rcs;
    if (e->in_flight != mcf_engine::kNoSearch) return mcf::fail(MCF_ERR_STATE, "mcf_engine_comm_init: a search is in flight");
    // A resident engine keeps its grid and its candidate cache: the collective gets a stream of its own and moves records that lie in pinned
    // host memory.  Its kernel needs room beside the resident grid, which therefore must leave a few CUs alone (desc.resident_workgroups:
    // mcf_ns_set_sharding asks for 8 fewer than there are CUs); a grid that fills the device -- and the RC grid's workgroups take whole CUs --
    // would starve it, so such an engine falls back to one dispatch per search with the exchange on its own stream, as in rounds 1 and 2.
    int cus = 0;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, e->d.device);
    const bool keep = e->resident_ok && e->res_grid + 8 <= std::max(cus, 16);      // room beside the resident grid
    if (!keep) {
        if (e->cand_on) {              // the candidate cache lives on the resident grid's answers: hand what it still holds to the device and switch it off
            if (int rcf = flush_pending(e)) return rcf;
            e->cand_on = false;
            e->shift_grid = false;
            e->st.candidates = 0;
        }
        if (e->resident_ok) {
            e->resident_ok = false;
            e->st.resident = 0;
            e->st.scan_workgroups = e->grid;
            e->st.scan_threads = e->lds_pi ? kResidentThreads : kThreads;
        }
    }
    e->comm_resident = keep;
    Id128 nid;
    memcpy(nid.b, id, 128);
    const int rc = r->comm_init_rank(&e->comm, world, nid, rank);
    if (rc != 0) return mcf::fail(MCF_ERR_COMM, "ncclCommInitRank: %s", r->error_string ? r->error_string(rc) : "error");
    e->rank = rank;
    e->world = world;
    e->st.comm_ranks = world;
    if (r->comm_count) { int seen = 0; if (r->comm_count(e->comm, &seen) == 0) e->st.comm_ranks = seen; }     // as the communicator itself reports it
    {
        // The collective must not share a hardware queue with a resident grid (a queue runs its packets in order: the all-gather would
        // wait until the grid leaves).  HIP multiplexes the streams of one priority over a handful of queues (GPU_MAX_HW_QUEUES, 4), so
        // with a few engines alive two of their streams do share one; streams of another priority have queues of their own.
        int prio_least = 0, prio_greatest = 0;
        HIP_TRY(hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest));
        HIP_TRY(hipStreamCreateWithPriority(&e->comm_stream, hipStreamNonBlocking, prio_greatest));
        HIP_TRY(hipHostMalloc((void **)&e->x_send, sizeof(mcf_engine::XRec), hipHostMallocMapped | hipHostMallocCoherent));
        HIP_TRY(hipHostMalloc((void **)&e->x_recv, sizeof(mcf_engine::XRec) * world, hipHostMallocMapped | hipHostMallocCoherent));
        memset(e->x_send, 0, sizeof(mcf_engine::XRec));
        memset(e->x_recv, 0, sizeof(mcf_engine::XRec) * world);
        HIP_TRY(hipHostGetDevicePointer(&e->d_x_send, e->x_send, 0));
        HIP_TRY(hipHostGetDevicePointer(&e->d_x_recv, e->x_recv, 0));
        e->x_seq = 0;
    }
    if (keep) return MCF_OK;
    HIP_TRY(hipMalloc((void **)&e->d_cand_local, sizeof(mcf_candidate)));
    HIP_TRY(hipMalloc((void **)&e->d_cand_all, sizeof(mcf_candidate) * world));
    HIP_TRY(hipMalloc((void **)&e->d_dev_slots, sizeof(Slot) * kMaxWorkgroups * kSlotStride));
    HIP_TRY(hipHostMalloc((void **)&e->h_cand_all, sizeof(mcf_candidate) * world, hipHostMallocDefault));
    return MCF_OK;
}

int mcf_engine_find_entering_sharded(mcf_engine *e, int32_t *found, int32_t *arc, int64_t *reduced_cost)
{
    if (!e || !found || !arc) return mcf::fail(MCF_ERR_INVALID, "null argument");
    if (!e->comm) return mcf::fail(MCF_ERR_STATE, "mcf_engine_comm_init has not been called");
    HIP_TRY(hipSetDevice(e->d.device));
    if (e->comm_resident || e->in_flight != mcf_engine::kNoSearch) {
        // ---- resident engine (or a search that mcf_engine_search_begin has already posted): its own candidate as usual (from the cache
        // when the shard's range can be decided on the host, from its grid when not), then the exchange
        if (e->in_flight == mcf_engine::kNoSearch) { const int rcb = search_begin(e); if (rcb) return rcb; }
        Key k;
        int rc = search_end(e, &k);
        if (rc) return rc;
        mcf_engine::XRec mine{};
        key_to_candidate(e, k, &mine.c);
        const uint64_t xs = ++e->x_seq;
        mine.head = mine.tail = xs;
        *e->x_send = mine;
        std::atomic_thread_fence(std::memory_order_release);
        const int nrc = rccl()->all_gather(e->d_x_send, e->d_x_recv, sizeof(mcf_engine::XRec), kNcclChar, e->comm, e->comm_stream);
        if (nrc != 0) return mcf::fail(MCF_ERR_COMM, "ncclAllGather: %s", rccl()->error_string ? rccl()->error_string(nrc) : "error");
        std::vector<mcf_candidate> all((size_t)e->world);
        const volatile mcf_engine::XRec *got = e->x_recv;
        double t0 = 0;
        for (int r = 0; r < e->world; ++r) {
            uint64_t spins = 0;
            while (!(got[r].head == xs && got[r].tail == xs)) {
                _mm_pause();
                if ((++spins & 0xFFFFF) == 0) {
                    const hipError_t q = hipStreamQuery(e->comm_stream);
                    if (q != hipSuccess && q != hipErrorNotReady) return mcf::fail(MCF_ERR_HIP, "the exchange failed: %s", hipGetErrorString(q));
                    if (t0 == 0) t0 = mcf::now_ns();
                    else if (mcf::now_ns() - t0 > 30e9) return mcf::fail(MCF_ERR_TIMEOUT, "rank %d's record of exchange %llu did not arrive within 30 s", r, (unsigned long long)xs);
                }
            }
            std::atomic_thread_fence(std::memory_order_acquire);
            memcpy(&all[r], (const void *)&got[r].c, sizeof(mcf_candidate));
            if (!(got[r].head == xs && got[r].tail == xs)) { --r; continue; }       // overwritten while it was being read: cannot happen in lock-step, checked anyway
        }
        return mcf_engine_resolve(e, e->world, all.data(), found, arc, reduced_cost);
    }
    // the scan writes its per-workgroup records into device memory and one more workgroup folds them into the all-gather's send buffer:
    // no host poll and no 16-byte copy to the device between the scan and the collective
    e->slots_target = e->d_dev_slots;
    int rc = search_begin(e);                // one dispatch (comm_init took the engine out of resident mode), patches as usual
    e->slots_target = nullptr;
    if (rc) return rc;
    if (e->in_flight != mcf_engine::kDispatchSearch) return mcf::fail(MCF_ERR_STATE, "sharded search did not dispatch");
    e->in_flight = mcf_engine::kNoSearch;    // nothing will be collected from the host records
    {
        const SearchHeader h = search_header(e);
        with_rule(e, [&](auto rule, auto) {
            launch(reduce_records_kernel<decltype(rule)::value>, dim3(1), dim3(kThreads), e->stream, nullptr, nullptr, e->d_dev_slots, e->grid, e->d.search_arc_num, h.next_arc,
                   e->next_arc, h.block_size, h.rstar, h.dual ? 1 : 0, e->d_cand_local);
        });
        HIP_TRY(hipGetLastError());
    }
    // MINLOC over (key, arc): RCCL has no MINLOC, so all-gather the 32-byte records and reduce locally
    const int nrc = rccl()->all_gather(e->d_cand_local, e->d_cand_all, sizeof(mcf_candidate), kNcclChar, e->comm, e->stream);
    if (nrc != 0) return mcf::fail(MCF_ERR_COMM, "ncclAllGather: %s", rccl()->error_string ? rccl()->error_string(nrc) : "error");
    HIP_TRY(hipMemcpyAsync(e->h_cand_all, e->d_cand_all, sizeof(mcf_candidate) * e->world, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return mcf_engine_resolve(e, e->world, e->h_cand_all, found, arc, reduced_cost);
}

}  // extern "C"
