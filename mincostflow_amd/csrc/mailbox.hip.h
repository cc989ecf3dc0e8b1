// mailbox.hip.h -- the resident grids' request protocol, for both sides: the layout of the mailbox, the device helpers with which
// resident_kernel, resident_cand_kernel and resident_rc_kernel (kernels.hip.h) read it, and the host helpers with which resident_host.hip.h
// and candidate_cache.hip.h write it.  DESIGN.md sections 3.1, 3.3, 3.4.
//
// The mailbox lives in fine-grained VRAM that the host writes through the PCIe BAR (write-combining); the workgroups of a resident grid poll
// it.  It is made of 64-byte lines, and dword 15 of EVERY line repeats the sequence number of the request it belongs to, so a torn read of any
// line (one whose four 16-byte stores have not all landed) is detected and read again.
//   poll unit    line 0 = the header, line 1 = entry line 0.  kMaxReplicas copies, kReplicaStride dwords apart; workgroup g polls copy
//                g % poll_replicas, so that 256 pollers do not hammer one address.  Line 1 rides with the header because the poll reads both
//                (128 bytes per workgroup and poll): a request whose entries fit one line needs no further read.
//   entry lines  entry line 0 in the poll unit, entry line l >= 1 at dword kMailboxTail + 16 (l - 1).  kMailboxPatchesPerLine entries {a, b, c}
//                per line: the value entries {node, lo, hi} first, then the state writes {arc, state, 0}.  The header carries value entry 0 and
//                state writes 0 and 1, so entry line 0 starts with value entry 1 and state write 2.
//   shift lines  (resident_cand_kernel) from dword shift_base: kShiftNodesPerLine node ids each, or kShiftPairsPerLine {first id, length}
//                pairs (runs of consecutive ids: the host relabels the nodes in thread order); [15] = seq of the scan request they belong to.
// Apply posts (kCmdApply, kCmdApplyRuns) carry no search: they say that entry lines (resident_kernel) or shift lines (resident_cand_kernel)
// 0 .. L-1 of the COMING scan request are in place while the host is still producing the rest, under that request's seq and a post counter
// of their own.  The grid applies what it has not applied yet and goes back to polling; no answer.  The posts are cumulative, so one that is
// overwritten before a workgroup saw it loses nothing; the scan request finishes the list.
// A value entry or a state write is a final value: applying it twice is harmless, and a torn line simply makes the grid poll again.  A
// shift (resident_cand_kernel: sigma onto a subtree's nodes; resident_rc_kernel: {node, delta} onto the arcs' reduced costs) is not: those
// grids remember for which request, and how far, they shifted, so that reading a request again does not repeat it.
#pragma once

#include <hip/hip_runtime.h>
#include <immintrin.h>

#include <cstdint>
#include <cstring>

namespace {

constexpr int kMailboxLines = 256;                // lines staged in LDS at a time: 16 KB = line 0 + a chunk of 255 entry lines (1275 entries)
constexpr int kMailboxPatchesPerLine = 5;         // entries {a, b, c} per entry line
constexpr int kMaxReplicas = 16;                  // copies of the poll unit
constexpr int kReplicaStride = 1024;              // dwords between them (4 KB)
constexpr int kMailboxTail = kMaxReplicas * kReplicaStride;   // dword offset of entry line 1
constexpr int kShiftNodesPerLine = 15;            // node ids per shift line ...
constexpr int kShiftPairsPerLine = 7;             // ... or {first id, length} pairs

// commands (header word kHdrCmd)
enum : uint32_t {
    kCmdScan = 0,        // apply the entries, search, answer
    kCmdQuit = 1,        // leave
    kCmdApply = 2,       // apply post: resident_kernel's entry lines / resident_cand_kernel's shift lines as node ids
    kCmdReload = 3,      // read the bound potentials again (host_pi), then as kCmdScan
    kCmdApplyRuns = 4,   // apply post of resident_cand_kernel's shift lines as {first, length} pairs
};
// exit codes (word 0 of the exit record)
enum : uint32_t {
    kExitQuit = 1,       // told to
    kExitIdle = 2,       // no request within idle_ticks
    kExitBarrier = 3,    // the grid-wide barrier of a reload gave up
    kExitPartial = 4,    // a dealt-out list was applied in part: the device arrays are undefined
};
// header words (line 0 of the poll unit)
enum : int {
    // every grid
    kHdrSeq = 0, kHdrCmd = 1,
    kHdrStates = 5,      // n_st: state writes, two of them in the header
    kHdrState0 = 6,      // state writes 0, 1: {arc, state} at 6..7, 8..9
    kHdrValue0 = 10,     // value entry 0: {node, lo, hi} at 10..12
    kHdrTag = 15,
    // resident_kernel, resident_rc_kernel (resident_post, resident_stream)
    kHdrNextArc = 2, kHdrRstar = 3,
    kHdrValues = 4,      // n_pi: value entries (resident_rc_kernel: {node, delta}), one of them in the header
    kHdrBlockSize = 13,  // scan: block size of THIS search (the reference's adaptive rule changes it between searches, NS.cs:1400-1438)
    kHdrApplyLines = 13, // kCmdApply: entry lines in place so far
    kHdrApplySub = 14,   // kCmdApply: post counter
    // resident_cand_kernel (shift_post_request, shift_stream)
    kShHdrValues = 2,    // n_val: value entries, one of them in the header
    kShHdrShift = 3,     // scan: shift entries (node ids or pairs); apply posts: shift lines in place so far
    kShHdrRuns = 4,      // scan: 1 = the shift lines hold pairs
    kShHdrApplySub = 4,  // apply posts: post counter
    kShHdrSigma = 13,    // the shift, lo at 13, hi at 14
};

// the mailbox part of a resident grid's kernel arguments (mailbox_params fills it)
struct MailboxParams {
    const uint32_t *mailbox;    // fine-grained VRAM, written by the host through the BAR
    uint32_t *exit_word;        // pinned host memory: the exit record ([0] exit code, [1] requests served, [2..3] scan ticks of workgroup 0, ...)
    uint32_t start_seq, idle_ticks;
    int32_t max_pi;             // value entries the mailbox can hold
    int32_t max_st;             // state writes it can hold
    int32_t poll_replicas, poll_sleep;
    const int64_t *host_pi;     // the caller's bound potentials in mapped host memory (kCmdReload reads them), or null
    uint32_t *barrier;          // ... and the arrival counter of the grid-wide barrier (zero at launch)
};

// ------------------------------------------------------------------------------------------------ device side
// All of it is inlined into the grids, and none of it declares LDS of its own: the callers pass their staging areas and flag word in.
typedef uint32_t v4u __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int clamp_count(int x, int hi) { return x < 0 ? 0 : (x > hi ? hi : x); }

// entry line l (entry line 0 sits in the poll unit `unit`, the others in the tail)
__device__ __forceinline__ const uint32_t *entry_line(const uint32_t *mailbox, const uint32_t *unit, int l)
{
    return l == 0 ? unit + 16 : mailbox + (kMailboxTail + (size_t)(l - 1) * 16);
}
// entry i of entry lines that lie one after the other from `base`
__device__ __forceinline__ const uint32_t *entry_at(const uint32_t *base, int i)
{
    return base + (i / kMailboxPatchesPerLine) * 16 + 3 * (i % kMailboxPatchesPerLine);
}

// Wave 0 polls lines 0 and 1 of the poll unit (system-scope reads of device memory) in a tight loop until a request newer than `last`
// arrives, or until idle_ticks have passed since idle_since; the other waves wait at the barrier.  An apply post (is_apply(cmd)) is only
// new when its post counter, header word SUB_WORD, differs from last_sub (SUB_WORD < 0: the grid takes no apply posts).  Both lines land in
// lm[0..31]; true when the grid is to leave on its idle timeout.
template <int SUB_WORD, typename IsApply>
__device__ __forceinline__ bool poll_request(const uint32_t *unit, uint32_t last, uint32_t last_sub, IsApply is_apply, uint64_t idle_since,
                                             const MailboxParams &mb, uint32_t *lm, uint32_t &s_flag)
{
    const int tid = threadIdx.x;
    if (tid < 64) {
        v4u x = v4u{0u, 0u, 0u, 0u};
        uint32_t flag;
        for (;;) {
            if (tid < 8) asm volatile("global_load_dwordx4 %0, %1, off sc0 sc1" : "=v"(x) : "v"(unit + tid * 4) : "memory");
            asm volatile("s_waitcnt vmcnt(0)" : "+v"(x)::"memory");
            const uint32_t seq0 = (uint32_t)__builtin_amdgcn_readlane((int)x[0], 0), tag0 = (uint32_t)__builtin_amdgcn_readlane((int)x[3], 3);
            bool fresh = seq0 != last && tag0 == seq0;
            if constexpr (SUB_WORD >= 0) {
                const uint32_t cmd0 = (uint32_t)__builtin_amdgcn_readlane((int)x[1], 0), sub0 = (uint32_t)__builtin_amdgcn_readlane((int)x[SUB_WORD & 3], SUB_WORD >> 2);
                fresh = fresh && (!is_apply(cmd0) || sub0 != last_sub);
            }
            if (fresh) { flag = 1u; break; }
            if (__builtin_amdgcn_s_memrealtime() - idle_since > mb.idle_ticks) { flag = kExitIdle; break; }
            for (int z = 0; z < mb.poll_sleep; ++z) __builtin_amdgcn_s_sleep(1);
        }
        if (tid < 8) *reinterpret_cast<v4u *>(lm + tid * 4) = x;
        if (tid == 0) s_flag = flag;
    }
    __syncthreads();
    return s_flag == kExitIdle;
}

// Stages n_a shift lines (shift line first_a on) followed by n_v entry lines (entry line first_v on) into dst, DEPTH 16-byte reads per
// thread in flight per wait; true when every staged line carries the tag seq.
template <int DEPTH>
__device__ __forceinline__ bool stage_lines(uint32_t *dst, const uint32_t *mailbox, const uint32_t *unit, uint32_t shift_base, int n_a, int first_a,
                                            int n_v, int first_v, uint32_t seq)
{
    static_assert(DEPTH == 1 || DEPTH == 4, "one or four reads per wait");
    const int tid = threadIdx.x, nt = (int)blockDim.x;
    const int count = n_a + n_v;
    for (int base = 0; base < count * 4; base += nt * DEPTH) {
        v4u x[DEPTH];
#pragma unroll
        for (int q = 0; q < DEPTH; ++q) {
            x[q] = v4u{0u, 0u, 0u, 0u};
            const int c = base + q * nt + tid;
            if (c < count * 4) {
                const int l = c >> 2;
                const uint32_t *src = l < n_a ? mailbox + (shift_base + (size_t)(first_a + l) * 16) : entry_line(mailbox, unit, first_v + l - n_a);
                asm volatile("global_load_dwordx4 %0, %1, off sc0 sc1" : "=v"(x[q]) : "v"(src + (c & 3) * 4) : "memory");
            }
        }
        if constexpr (DEPTH == 4) asm volatile("s_waitcnt vmcnt(0)" : "+v"(x[0]), "+v"(x[1]), "+v"(x[2]), "+v"(x[3])::"memory");
        else asm volatile("s_waitcnt vmcnt(0)" : "+v"(x[0])::"memory");
#pragma unroll
        for (int q = 0; q < DEPTH; ++q) {
            const int c = base + q * nt + tid;
            if (c < count * 4) *reinterpret_cast<v4u *>(dst + c * 4) = x[q];
        }
    }
    __syncthreads();
    int bad = 0;
    for (int l = tid; l < count; l += nt) bad |= (dst[l * 16 + 15] != seq);
    return __syncthreads_or(bad) == 0;
}

// One wave reads the line at src (lanes 0..3, 16 bytes each) until it carries the tag seq; false when it has not arrived within idle_ticks.
__device__ __forceinline__ bool wait_line(const uint32_t *src, uint32_t seq, uint32_t idle_ticks, v4u &x)
{
    const int lane = threadIdx.x & 63;
    x = v4u{0u, 0u, 0u, 0u};
    const uint64_t t_line = __builtin_amdgcn_s_memrealtime();
    for (;;) {
        if (lane < 4) asm volatile("global_load_dwordx4 %0, %1, off sc0 sc1" : "=v"(x) : "v"(src + lane * 4) : "memory");
        asm volatile("s_waitcnt vmcnt(0)" : "+v"(x)::"memory");
        if ((uint32_t)__builtin_amdgcn_readlane((int)x[3], 3) == seq) return true;
        if (__builtin_amdgcn_s_memrealtime() - t_line > idle_ticks) return false;
    }
}

// kCmdReload: this workgroup's slice of the bound potentials into the device array.  Agent scope: written through to memory, where the
// workgroups of the other XCDs (each with an L2 of its own) will find it after the grid-wide barrier.
// narrow: pi holds int32 potentials, else int64.
__device__ __forceinline__ void reload_slice(void *pi, bool narrow, const int64_t *host_pi, int n_nodes)
{
    const int per = (n_nodes + (int)gridDim.x - 1) / (int)gridDim.x;
    const int lo = (int)blockIdx.x * per, hi = lo + per < n_nodes ? lo + per : n_nodes;
    for (int i = lo + (int)threadIdx.x; i < hi; i += (int)blockDim.x) {
        const int64_t v = host_pi[i];
        if (narrow) __hip_atomic_store(reinterpret_cast<int32_t *>(pi) + i, (int32_t)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else __hip_atomic_store(reinterpret_cast<int64_t *>(pi) + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// Grid-wide barrier (all workgroups are resident: one per CU); `barriers` counts this launch's barriers so far.  False when it gave up: a
// workgroup that never got a CU (somebody else's grid holds them) must not hang the others -- every spin of a resident grid is bounded.
__device__ __forceinline__ bool grid_barrier(const MailboxParams &mb, uint32_t &barriers, uint32_t &s_flag)
{
    const int tid = threadIdx.x;
    __builtin_amdgcn_s_waitcnt(0);
    __syncthreads();
    barriers += 1;
    if (tid == 0) {
        __hip_atomic_fetch_add(mb.barrier, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t want = barriers * gridDim.x;
        const uint64_t t_bar = __builtin_amdgcn_s_memrealtime();
        uint32_t gave_up = 0u;
        while (__hip_atomic_load(mb.barrier, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) < want) {
            __builtin_amdgcn_s_sleep(2);
            if (__builtin_amdgcn_s_memrealtime() - t_bar > 8ull * mb.idle_ticks) { gave_up = 1u; break; }
        }
        s_flag = gave_up ? kExitBarrier : 0u;
    }
    __syncthreads();
    if (s_flag == kExitBarrier) return false;
    // what other XCDs wrote through to memory may still sit in this CU's L1 / this XCD's L2 in its old form: forget it (once per workgroup)
    if (tid < 64) asm volatile("buffer_inv sc1\n\ts_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    return true;
}

// words 0..3 of the exit record; the exit code goes last (resident_harvest reads the rest, resident_cand_kernel writes words 4..11 before it)
__device__ __forceinline__ void resident_exit(uint32_t *exit_word, uint32_t code, uint32_t served, uint64_t scan_ticks)
{
    __hip_atomic_store(exit_word + 1, served, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(exit_word + 2, (uint32_t)scan_ticks, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(exit_word + 3, (uint32_t)(scan_ticks >> 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(exit_word, code, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// ------------------------------------------------------------------------------------------------ host side
struct MailboxLine {
    alignas(16) uint32_t w[16];
};

// one 64-byte line into the write-combining BAR mapping: four 16-byte stores, the tag goes out with the last one
inline void mailbox_write_line(uint32_t *dst, const uint32_t *line16)
{
    const __m128i *src = (const __m128i *)line16;
    __m128i *d = (__m128i *)dst;
    _mm_store_si128(d + 0, _mm_loadu_si128(src + 0));
    _mm_store_si128(d + 1, _mm_loadu_si128(src + 1));
    _mm_store_si128(d + 2, _mm_loadu_si128(src + 2));
    _mm_store_si128(d + 3, _mm_loadu_si128(src + 3));
}

// entry k of a list: {node[lo + k], value[lo + k]} (value entries), {arc[lo + k], state[lo + k]} (state writes)
struct ValueEntries { const int32_t *node; const int64_t *value; size_t lo; int n; };
struct StateEntries { const int32_t *arc; const int32_t *state; size_t lo; int n; };

// Encodes the value entries and then the state writes as entry lines with the tag seq.  Entry lines 1.. go into the tail, except lines
// 1 .. in_place - 1, which apply posts have put there already; entry line 0 is returned: it goes out with the header (mailbox_publish).
inline MailboxLine mailbox_encode_entries(uint32_t *mailbox, const ValueEntries &v, const StateEntries &s, uint32_t seq, int in_place = 0)
{
    MailboxLine line0{}, line;
    const int entries = v.n + s.n;
    for (int l = 0, i = 0; i < entries; ++l) {
        if (l > 0 && l < in_place) { i += kMailboxPatchesPerLine; continue; }
        memset(line.w, 0, sizeof(line.w));
        for (int k = 0; k < kMailboxPatchesPerLine && i < entries; ++k, ++i) {
            uint32_t *q = line.w + 3 * k;
            if (i < v.n) {
                const uint64_t x = (uint64_t)v.value[v.lo + i];
                q[0] = (uint32_t)v.node[v.lo + i];
                q[1] = (uint32_t)x;
                q[2] = (uint32_t)(x >> 32);
            } else {
                q[0] = (uint32_t)s.arc[s.lo + (i - v.n)];
                q[1] = (uint32_t)s.state[s.lo + (i - v.n)];
            }
        }
        line.w[15] = seq;
        if (l == 0) line0 = line;
        else mailbox_write_line(mailbox + kMailboxTail + 16 * (size_t)(l - 1), line.w);
    }
    return line0;
}

// The header, and entry line 0 when there is one, into every copy of the poll unit.  The first sfence makes whatever went into the tail or
// the shift lines leave the write-combining buffers before any header does (a caller that wrote nothing there may leave it out).
inline void mailbox_publish(uint32_t *mailbox, int replicas, const MailboxLine &header, const MailboxLine *line0, bool fence_first = true)
{
    if (fence_first) _mm_sfence();
    for (int r = 0; r < replicas; ++r) {
        uint32_t *unit = mailbox + (size_t)r * kReplicaStride;
        if (line0) mailbox_write_line(unit + 16, line0->w);
        mailbox_write_line(unit, header.w);
    }
    _mm_sfence();
}

}  // namespace
