// collect.hip.h -- device half of LEMON's list rules (included by engine.hip after kernels.hip.h): the eligible arcs of the cyclic scan
// that starts at next_arc, IN SCAN ORDER, up to where LEMON's loop stops (mcf_engine_collect_eligible in include/mcf_hip.h).
//
// Two dispatches in stream order, no communication between the workgroups of one launch:
//   collect_count_kernel  one workgroup per tile of consecutive ROTATED positions p = (arc - next_arc) mod m_s: how many eligible arcs the tile
//                         holds, how many of them lie in the first block (p < block_size) and the first eligible position p >= block_size
//   collect_emit_kernel   the same tiles again: every workgroup folds the tile records (the exclusive prefix of the counts before it, the
//                         totals) -- which is the whole stop rule -- and the tiles that lie before the stop write their eligible arcs at
//                         prefix + rank: rank within a wave from __ballot + mbcnt, across the four waves from an LDS prefix
// The stop needs the totals of all tiles, which a single pass could only learn through a look-back across workgroups; at the sizes the
// rules run at (40 k - 400 k search arcs: 40 - 400 tiles) the second pass costs one launch and a re-read of the tiles before the stop.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace {

constexpr int kCollectThreads = 256;       // 4 wavefronts of 64
constexpr int kCollectMaxTiles = 1024;     // tiles grow (more rounds of 256 positions) beyond 1024 * 1024 search arcs

struct alignas(16) CollectTile {
    int32_t count;        // eligible arcs in the tile
    int32_t head;         // ... of them at rotated positions < block_size
    int32_t first_beyond; // first eligible rotated position >= block_size in the tile, INT32_MAX when none
    int32_t pad;
};

// 16 bytes per collected arc, one vector store each, into pinned host memory
struct alignas(16) CollectEntry {
    int64_t c;
    int32_t arc;
    int32_t pos;
};

struct alignas(16) CollectHeader {
    int32_t count;        // eligible arcs up to the stop (may exceed the capacity: only the first `capacity` are written)
    int32_t end_arc;
    int64_t arcs_scanned;
};

template <typename T>
struct CollectArgs {
    const int32_t *src;
    const int32_t *tgt;
    const T *cost;
    const int8_t *state;
    const T *pi;
    int32_t m_s;
    int32_t next_arc;
    int32_t rounds;          // rounds of kCollectThreads positions per tile
    int32_t mode;            // MCF_COLLECT_FIRST_N / MCF_COLLECT_BLOCKS
    int32_t limit;
    int32_t block_size;      // BLOCKS; 0 for FIRST_N
    int32_t head_length;
    int32_t survivors;
};

// reduced cost of the arc at rotated position p (< m_s): state * (cost + pi[source] - pi[target]) in 64 bits (ns.h:480); a basic arc is 0
template <typename T>
__device__ inline int64_t collect_rc(const CollectArgs<T> &a, int p, int &e)
{
    e = a.next_arc + p;
    if (e >= a.m_s) e -= a.m_s;
    const int st = a.state[e];
    if (st == 0) return 0;
    return (int64_t)st * ((int64_t)a.cost[e] + (int64_t)a.pi[a.src[e]] - (int64_t)a.pi[a.tgt[e]]);
}

__device__ inline int wave_sum(int v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ inline int wave_min(int v)
{
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
    return v;
}

template <typename T>
__global__ __launch_bounds__(kCollectThreads) void collect_count_kernel(CollectArgs<T> a, CollectTile *tiles)
{
    __shared__ int s_red[3][kCollectThreads / 64];
    const int base = blockIdx.x * a.rounds * kCollectThreads;
    int cnt = 0, head = 0, first = INT32_MAX;
    for (int r = 0; r < a.rounds; ++r) {
        const int p = base + r * kCollectThreads + (int)threadIdx.x;
        if (p >= a.m_s) break;
        int e;
        if (collect_rc(a, p, e) < 0) {
            ++cnt;
            if (p < a.block_size) ++head;
            else first = min(first, p);
        }
    }
    cnt = wave_sum(cnt); head = wave_sum(head); first = wave_min(first);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { s_red[0][wave] = cnt; s_red[1][wave] = head; s_red[2][wave] = first; }
    __syncthreads();
    if (threadIdx.x == 0) {
        CollectTile t{0, 0, INT32_MAX, 0};
        for (int w = 0; w < kCollectThreads / 64; ++w) { t.count += s_red[0][w]; t.head += s_red[1][w]; t.first_beyond = min(t.first_beyond, s_red[2][w]); }
        tiles[blockIdx.x] = t;
    }
}

template <typename T>
__global__ __launch_bounds__(kCollectThreads) void collect_emit_kernel(CollectArgs<T> a, const CollectTile *tiles, int n_tiles,
                                                                      CollectEntry *out, int capacity, CollectHeader *hdr)
{
    __shared__ int s_red[4][kCollectThreads / 64];
    __shared__ int s_wave[kCollectThreads / 64];
    const int tile = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tile_len = a.rounds * kCollectThreads;
    const int base = tile * tile_len;
    // fold the tile records: arcs before this tile, all arcs, arcs of the first block, first eligible position beyond it
    int pre = 0, total = 0, head = 0, first = INT32_MAX;
    for (int i = threadIdx.x; i < n_tiles; i += kCollectThreads) {
        const CollectTile t = tiles[i];
        if (i < tile) pre += t.count;
        total += t.count;
        head += t.head;
        first = min(first, t.first_beyond);
    }
    pre = wave_sum(pre); total = wave_sum(total); head = wave_sum(head); first = wave_min(first);
    if (lane == 0) { s_red[0][wave] = pre; s_red[1][wave] = total; s_red[2][wave] = head; s_red[3][wave] = first; }
    __syncthreads();
    pre = total = head = 0; first = INT32_MAX;
    for (int w = 0; w < kCollectThreads / 64; ++w) { pre += s_red[0][w]; total += s_red[1][w]; head += s_red[2][w]; first = min(first, s_red[3][w]); }

    // the last rotated position LEMON's loop visits (p_end; beyond the cycle when it runs to its end) and the last one this call returns
    int64_t p_end = INT64_MAX;
    if (a.mode == MCF_COLLECT_BLOCKS) {
        const int64_t B = a.block_size;
        if ((int64_t)a.survivors + head > a.head_length) p_end = B - 1;                  // ns.h:596-597 after the first block
        else if ((int64_t)a.survivors + head > 0) p_end = 2 * B - 1;                      // after the second (limit = 0)
        else if (first != INT32_MAX) p_end = ((int64_t)first / B + 1) * B - 1;            // after the first block that has an eligible arc
    }
    const int64_t p_lim = p_end < (int64_t)a.m_s ? p_end : (int64_t)a.m_s - 1;
    if (a.mode == MCF_COLLECT_FIRST_N) {
        if (tile == 0 && threadIdx.x == 0 && total < a.limit) { hdr->count = total; hdr->end_arc = a.next_arc; hdr->arcs_scanned = a.m_s; }
        if (pre >= a.limit) return;                  // the limit-th eligible arc lies before this tile (uniform: every thread returns)
    } else if ((int64_t)base > p_lim) {
        return;
    }

    int run = pre;                                   // index of the next eligible arc in scan order
    for (int r = 0; r < a.rounds; ++r) {
        const int p = base + r * kCollectThreads + (int)threadIdx.x;
        int e = 0;
        int64_t c = 0;
        const bool in = p < a.m_s && (int64_t)p <= p_lim;
        if (in) c = collect_rc(a, p, e);
        const bool hit = in && c < 0;
        const uint64_t mask = __ballot(hit);
        const int rank = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
        if (lane == 0) s_wave[wave] = __popcll(mask);
        __syncthreads();
        int off = 0, all = 0;
        for (int w = 0; w < kCollectThreads / 64; ++w) { off += w < wave ? s_wave[w] : 0; all += s_wave[w]; }
        if (hit) {
            const int g = run + off + rank;
            const bool keep = a.mode != MCF_COLLECT_FIRST_N || g < a.limit;
            if (keep && g < capacity) { CollectEntry x; x.c = c; x.arc = e; x.pos = p; out[g] = x; }
            if (a.mode == MCF_COLLECT_FIRST_N && g == a.limit - 1) { hdr->count = a.limit; hdr->end_arc = e; hdr->arcs_scanned = (int64_t)p + 1; }
        }
        run += all;
        __syncthreads();                             // s_wave is written again by the next round
    }
    if (a.mode == MCF_COLLECT_BLOCKS && threadIdx.x == 0 && p_lim >= (int64_t)base && p_lim < (int64_t)base + tile_len) {
        int end = a.next_arc;
        if (p_end < (int64_t)a.m_s) { end = a.next_arc + (int)p_end; if (end >= a.m_s) end -= a.m_s; }
        hdr->count = run;
        hdr->end_arc = end;
        hdr->arcs_scanned = p_lim + 1;
    }
}

}  // namespace
