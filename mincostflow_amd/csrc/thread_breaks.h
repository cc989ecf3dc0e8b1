// thread_breaks.h -- the two walkers over a moved subtree: run by run after the nodes have been relabelled in thread order (BreakWalk, with
// the bitmap it reads), node by node with prefetch hints before that (HintWalk, at the end of the file).
//
// After a relabelling the successor of node a in the thread list is a + 1 almost everywhere.  Where it is not, the list has a BREAK.  The
// driver keeps one bit per node, set exactly where nxt[a] != a + 1, and the walk takes the end of the run it is in from that bitmap instead
// of comparing every loaded successor: no branch of the walk depends on a load of nxt, so the load of the jump's target is in flight
// while the run's potentials are added.  JUMP HINTS make the misses of several jumps overlap: follow[a] of a run start a names the run start
// that came kJumpAhead jumps later the last time a walk passed here, and its lines are prefetched when the walk reaches a.
//
// Plain C++ on plain pointers, nothing of HIP: ns_host.cpp uses it inside a solve, tools/thread_breaks_check.cpp drives it on its own under
// the sanitizers.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace mcf {

constexpr int kJumpAhead = 6;      // how many jumps ahead a hint points (2 .. 12 swept on config 3's replay)
constexpr int kJumpRing = 16;      // run starts remembered, a power of two > kJumpAhead

// ---- the bitmap: bit a of [0, n] (n = the root) is set exactly when nxt[a] != a + 1.  The bits above n in the last word are set, and two
// words of ones follow, so that a 64-bit window starting at any node may be read and a scan for the next break always ends.
inline size_t breaks_words(int n) { return ((size_t)n + 64) / 64 + 2; }

inline void breaks_note(uint64_t *bits, const int32_t *nxt, int a)
{
    const uint64_t m = 1ull << (a & 63);
    uint64_t &w = bits[a >> 6];
    w = nxt[a] != a + 1 ? (w | m) : (w & ~m);
}

inline void breaks_rebuild(uint64_t *bits, const int32_t *nxt, int n)
{
    const size_t words = breaks_words(n);
    for (size_t w = 0; w < words; ++w) bits[w] = ~0ull;
    for (int a = 0; a <= n; ++a) if (nxt[a] == a + 1) bits[a >> 6] &= ~(1ull << (a & 63));
}

// how many bits are not what nxt says (the padding and the sentinel words count as well)
inline int64_t breaks_mismatches(const uint64_t *bits, const int32_t *nxt, int n)
{
    int64_t bad = 0;
    const size_t words = breaks_words(n);
    for (size_t w = 0; w < words; ++w)
        for (int b = 0; b < 64; ++b) {
            const size_t a = w * 64 + (size_t)b;
            const bool want = a > (size_t)n || nxt[a] != (int32_t)a + 1;
            bad += ((bits[w] >> b) & 1) != (want ? 1u : 0u);
        }
    return bad;
}

// rehang_subtree's note hook (tree_pivot.h)
struct BreakNote {
    uint64_t *bits;
    const int32_t *nxt;
    void operator()(int a) const { breaks_note(bits, nxt, a); }
};

// ---- the walker.  One object per walk; advance() may be called piece by piece, and a piece boundary may cut a run: the rest of the run
// goes on in the next piece (it starts no new hint).
struct BreakWalk {
    int64_t *pi;
    const int32_t *nxt;
    int32_t *follow;
    const uint64_t *bits;
    int64_t sigma;
    int a;                      // the next node to visit
    bool at_start = true;       // a starts a run: the walk's first node or the target of a jump
    int64_t jumps = 0;          // runs that ended in a break
    unsigned starts = 0;
    int32_t ring[kJumpRing];

    // the next `count` nodes move by sigma; emit(first, length) is called once per run (or part of a run) in walk order
    template <class Emit> void advance(int count, Emit emit)
    {
        int a = this->a, left = count;
        bool at_start = this->at_start;
        while (left > 0) {
            if (at_start) {
                const int h = follow[a];
                __builtin_prefetch(&nxt[h]);
                __builtin_prefetch(&pi[h]);
                __builtin_prefetch(&follow[h]);
                __builtin_prefetch(&bits[h >> 6]);
                if (starts >= (unsigned)kJumpAhead) follow[ring[(starts - kJumpAhead) & (kJumpRing - 1)]] = a;
                ring[starts & (kJumpRing - 1)] = a;
                ++starts;
            }
            // the run's end: the first break at or behind a, from a 64-bit window of the bitmap that starts at a
            const size_t w = (size_t)a >> 6;
            const unsigned sh = (unsigned)a & 63;
            const uint64_t window = (bits[w] >> sh) | ((bits[w + 1] << 1) << (63 - sh));
            int len;                                   // nodes from a to the break, both included
            bool whole = true;                         // the break lies inside this piece
            if (window) {
                len = __builtin_ctzll(window) + 1;
            } else {
                len = 64;                              // no break in a .. a + 63: word by word from there, no farther than the walk goes
                whole = false;
                while (len < left) {
                    const size_t pos = (size_t)a + (size_t)len;
                    const uint64_t word = bits[pos >> 6] >> (pos & 63);
                    if (word) { len += __builtin_ctzll(word) + 1; whole = true; break; }
                    len += 64 - (int)(pos & 63);
                }
            }
            if (len > left) { whole = false; len = left; }
            const int32_t *const jump = &nxt[a + len - 1];
            __builtin_prefetch(jump);                  // the jump's load starts before the potentials are touched
            for (int k = 0; k < len; ++k) pi[a + k] += sigma;
            emit(a, len);
            left -= len;
            if (whole) { a = *jump; ++jumps; at_start = true; }
            else { a += len; at_start = false; }
        }
        this->a = a;
        this->at_start = at_start;
    }
};

// ---- the walker used before the first relabelling, when the thread order has nothing to do with the id order: node by node along nxt, one
// dependent load per node.  PREFETCH HINTS shorten that chain: follow[v] remembers which node came kWalkAhead steps after v the last time a
// walk passed v, and its lines are prefetched when the walk reaches v.  The thread order of a subtree changes little between pivots, so most
// hints are still right; a stale one costs a useless prefetch, nothing else.  Same shape as BreakWalk: one object per walk, advance() piece
// by piece, cut anywhere.
constexpr int kWalkAhead = 8;      // a power of two

struct HintWalk {
    int64_t *pi;
    const int32_t *nxt;
    int32_t *follow;
    int64_t sigma;
    int a;                      // the next node to visit
    unsigned seen = 0;          // nodes visited so far
    int32_t ring[kWalkAhead];   // the last kWalkAhead of them

    // the next `count` nodes move by sigma; emit(node, its new potential) is called once per node in walk order
    template <class Emit> void advance(int count, Emit emit)
    {
        int a = this->a;
        unsigned i = seen;
        const unsigned end = i + (unsigned)count;
        auto step = [&](bool hint) {
            const int h = follow[a];
            __builtin_prefetch(&nxt[h]);
            __builtin_prefetch(&pi[h]);
            __builtin_prefetch(&follow[h]);
            emit(a, pi[a] += sigma);
            if (hint) follow[ring[i & (kWalkAhead - 1)]] = a;
            ring[i & (kWalkAhead - 1)] = a;
            a = nxt[a];
        };
        // the walk's first kWalkAhead nodes have no node that far behind them to leave a hint with
        for (; i < end && i < (unsigned)kWalkAhead; ++i) step(false);
        for (; i < end; ++i) step(true);
        this->a = a;
        seen = i;
    }
};

}  // namespace mcf
