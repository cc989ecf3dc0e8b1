// thread_breaks_check.cpp -- the thread-break bitmap and the two walkers of the host driver (mincostflow_amd/csrc/thread_breaks.h) together
// with rehang_subtree's note hook (tree_pivot.h) as a stand-alone program, to be built under -fsanitize=address,undefined and run on a CPU
// (DESIGN.md section 4).  Needs no GPU, no HIP and is not loaded into Python.
//
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -I../include thread_breaks_check.cpp -o thread_breaks_check
//   ./thread_breaks_check [pivots per tree, default 4000]
//
// For every node count from 63 to 130 (the root id n and the sentinel words before, on and behind a word boundary): random pivots re-hang
// random subtrees of the start basis' tree, the nodes are relabelled in thread order every now and then, and after every pivot
//   * the bitmap kept by the hook equals a recomputation from the thread list,
//   * a walk over a random subtree or over its complement (through the root), cut into pieces of odd sizes, visits exactly the nodes of a plain
//     thread walk, in the same order, adds sigma to exactly their potentials, emits only runs of consecutive ids and counts the breaks it
//     crossed,
//   * the hinted walker (the one the driver uses before its first relabelling) over another such segment, cut the same way, visits the same
//     nodes as a plain thread walk in the same order and emits their new potentials, and follow[] holds node ids only.
// All arrays are sized exactly, so a read or write past node n is the sanitizer's to find.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "../mincostflow_amd/csrc/thread_breaks.h"
#include "../mincostflow_amd/csrc/tree_pivot.h"

namespace {

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd(uint32_t below)
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (uint32_t)((rng_state >> 11) % below);
}

struct Tree {
    int n;
    std::vector<int32_t> par, par_arc, nxt, prv, sub, fin, scratch, follow, tail, head;
    std::vector<int8_t> par_dir;
    std::vector<int64_t> pi, upper, flow;
    std::vector<uint64_t> bits;
    explicit Tree(int n_) : n(n_)
    {
        const size_t N = (size_t)n + 1;
        par.assign(N, n); par_arc.resize(N); nxt.resize(N); prv.resize(N); sub.assign(N, 1); fin.resize(N); scratch.assign(N + 1, 0);
        follow.assign(N, 0); par_dir.assign(N, mcf::kUp); pi.resize(N);
        tail.assign(1, 0); head.assign(1, 0); upper.assign(1, 0); flow.assign(1, 0);
        for (int u = 0; u <= n; ++u) { par_arc[(size_t)u] = u; nxt[(size_t)u] = u == n ? 0 : u + 1; prv[(size_t)u] = u == 0 ? n : u - 1; fin[(size_t)u] = u; pi[(size_t)u] = 1000 * u; }
        par[(size_t)n] = -1; sub[(size_t)n] = n + 1; fin[(size_t)n] = n - 1;
        bits.assign(mcf::breaks_words(n), 0);
        mcf::breaks_rebuild(bits.data(), nxt.data(), n);
    }
    mcf::TreeView view()
    {
        mcf::TreeView t{};
        t.tail = tail.data(); t.head = head.data(); t.upper = upper.data(); t.flow = flow.data();
        t.par = par.data(); t.par_arc = par_arc.data(); t.nxt = nxt.data(); t.prv = prv.data(); t.sub = sub.data(); t.fin = fin.data();
        t.par_dir = par_dir.data(); t.scratch = scratch.data();
        return t;
    }
    int depth(int u) const { int d = 0; while (par[(size_t)u] >= 0) { u = par[(size_t)u]; ++d; } return d; }
    int lca(int a, int b) const
    {
        int da = depth(a), db = depth(b);
        while (da > db) { a = par[(size_t)a]; --da; }
        while (db > da) { b = par[(size_t)b]; --db; }
        while (a != b) { a = par[(size_t)a]; b = par[(size_t)b]; }
        return a;
    }
    // ids in thread order, the root keeps n (what the driver's relabelling does to the arrays used here)
    void relabel()
    {
        const size_t N = (size_t)n + 1;
        std::vector<int32_t> to(N);
        int u = nxt[(size_t)n];
        for (int k = 0; k < n; ++k) { to[(size_t)u] = k; u = nxt[(size_t)u]; }
        to[(size_t)n] = n;
        auto permute = [&](auto &v) { auto tmp = v; for (size_t x = 0; x < N; ++x) tmp[(size_t)to[x]] = v[x]; for (size_t x = 0; x < N; ++x) v[x] = tmp[x]; };
        auto translate = [&](auto &v) { for (size_t x = 0; x < N; ++x) if (v[x] >= 0) v[x] = to[(size_t)v[x]]; };
        permute(par); permute(par_arc); permute(nxt); permute(prv); permute(sub); permute(fin); permute(par_dir); permute(pi); permute(follow);
        translate(par); translate(nxt); translate(prv); translate(fin); translate(follow);
        mcf::breaks_rebuild(bits.data(), nxt.data(), n);
    }
};

#define REQUIRE(cond, ...)                                                      \
    do {                                                                        \
        if (!(cond)) { fprintf(stderr, "FAILED %s: ", #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } \
    } while (0)

// the thread list is one cycle over all nodes, prv is its inverse and sub / fin describe the preorder
void check_tree(const Tree &t, int n, long pivot)
{
    int u = n, seen = 0;
    do {
        const int v = t.nxt[(size_t)u];
        REQUIRE(v >= 0 && v <= n && t.prv[(size_t)v] == u, "n %d pivot %ld: prv[%d]", n, pivot, v);
        u = v;
        ++seen;
    } while (u != n && seen <= n + 1);
    REQUIRE(seen == n + 1 && u == n, "n %d pivot %ld: the thread list visits %d nodes", n, pivot, seen);
    for (int x = 0; x <= n; ++x) {
        int last = x;
        for (int k = 1; k < t.sub[(size_t)x]; ++k) last = t.nxt[(size_t)last];
        REQUIRE(last == t.fin[(size_t)x], "n %d pivot %ld: fin[%d]", n, pivot, x);
    }
}

long walks = 0, hint_walks = 0, runs_seen = 0, cut_runs = 0;

// a subtree, or everything but a subtree (from the node behind its last one round through the root to the node before it), walked plainly
struct Segment {
    int first, count, behind;
    int64_t sigma, breaks = 0;
    std::vector<int32_t> plain;
    std::vector<int64_t> want;      // every potential after the walk
    explicit Segment(const Tree &t) : want(t.pi)
    {
        const int n = t.n, top = (int)rnd((uint32_t)n);
        first = top; count = t.sub[(size_t)top];
        if (rnd(3) == 0 && count <= n) { first = t.nxt[(size_t)t.fin[(size_t)top]]; count = n + 1 - count; }
        sigma = (int64_t)rnd(1000) - 500;
        int u = first;
        for (int k = 0; k < count; ++k) { plain.push_back(u); want[(size_t)u] += sigma; breaks += t.nxt[(size_t)u] != u + 1; u = t.nxt[(size_t)u]; }
        behind = u;
    }
    // odd sizes, many of them inside a run
    int piece(int done) const
    {
        int k = 1 + 2 * (int)rnd(12);
        if (rnd(4) == 0) k = count;
        return k > count - done ? count - done : k;
    }
};

void check_hint_walk(Tree &t, long pivot)
{
    const int n = t.n;
    const Segment sg(t);
    mcf::HintWalk w;
    w.pi = t.pi.data(); w.nxt = t.nxt.data(); w.follow = t.follow.data();
    w.sigma = sg.sigma; w.a = sg.first;
    std::vector<int32_t> got;
    for (int done = 0; done < sg.count;) {
        const int piece = sg.piece(done);
        const size_t before = got.size();
        w.advance(piece, [&](int a, int64_t v) {
            REQUIRE(a >= 0 && a <= n && v == sg.want[(size_t)a], "n %d pivot %ld: hinted walk emits node %d with %lld", n, pivot, a, (long long)v);
            got.push_back(a);
        });
        REQUIRE(got.size() - before == (size_t)piece, "n %d pivot %ld: a hinted piece of %d nodes emitted %zu", n, pivot, piece, got.size() - before);
        done += piece;
    }
    REQUIRE(got == sg.plain, "n %d pivot %ld: the hinted walk from %d over %d nodes visits other nodes than the thread list", n, pivot, sg.first, sg.count);
    REQUIRE(t.pi == sg.want, "n %d pivot %ld: potentials after the hinted walk from %d over %d nodes", n, pivot, sg.first, sg.count);
    REQUIRE(w.a == sg.behind && w.seen == (unsigned)sg.count, "n %d pivot %ld: the hinted walk stopped before %d after %u nodes", n, pivot, w.a, w.seen);
    for (int x = 0; x <= n; ++x) REQUIRE(t.follow[(size_t)x] >= 0 && t.follow[(size_t)x] <= n, "n %d pivot %ld: hint of %d", n, pivot, x);
    ++hint_walks;
}

void check_walk(Tree &t, long pivot)
{
    const int n = t.n;
    const Segment sg(t);
    const int first = sg.first, count = sg.count, behind = sg.behind;
    const int64_t sigma = sg.sigma, breaks = sg.breaks;
    const std::vector<int32_t> &plain = sg.plain;
    const std::vector<int64_t> &want = sg.want;

    mcf::BreakWalk w;
    w.pi = t.pi.data(); w.nxt = t.nxt.data(); w.follow = t.follow.data(); w.bits = t.bits.data();
    w.sigma = sigma; w.a = first;
    std::vector<int32_t> got;
    int done = 0;
    while (done < count) {
        const int piece = sg.piece(done);
        int in_piece = 0;
        w.advance(piece, [&](int start, int len) {
            REQUIRE(len >= 1 && start >= 0 && start + len - 1 <= n, "n %d pivot %ld: run %d+%d", n, pivot, start, len);
            for (int k = 0; k < len; ++k) got.push_back(start + k);
            in_piece += len;
            ++runs_seen;
        });
        REQUIRE(in_piece == piece, "n %d pivot %ld: a piece of %d nodes emitted %d", n, pivot, piece, in_piece);
        done += piece;
        if (done < count && !w.at_start) ++cut_runs;
    }
    REQUIRE(got == plain, "n %d pivot %ld: the walk from %d over %d nodes visits other nodes than the thread list", n, pivot, first, count);
    REQUIRE(t.pi == want, "n %d pivot %ld: potentials after the walk from %d over %d nodes", n, pivot, first, count);
    // a walk that ends inside a run has not crossed that run's break
    const bool ends_on_break = t.nxt[(size_t)plain.back()] != plain.back() + 1;
    REQUIRE(w.jumps == breaks && w.a == behind && w.at_start == ends_on_break, "n %d pivot %ld: %lld jumps for %lld breaks, stopped before %d", n, pivot,
            (long long)w.jumps, (long long)breaks, w.a);
    for (int x = 0; x <= n; ++x) REQUIRE(t.follow[(size_t)x] >= 0 && t.follow[(size_t)x] <= n, "n %d pivot %ld: hint of %d", n, pivot, x);
    ++walks;
}

}  // namespace

int main(int argc, char **argv)
{
    const long pivots = argc > 1 ? atol(argv[1]) : 4000;
    long total = 0, whole_moves = 0;
    for (int n = 63; n <= 130; ++n) {
        Tree t(n);
        const mcf::TreeView tv = t.view();
        for (long k = 0; k < pivots; ++k) {
            // an entering arc between two nodes x, y; the leaving arc is above a random node between x and the join, the join excluded
            int x = (int)rnd((uint32_t)n + 1), y = (int)rnd((uint32_t)n + 1);
            if (x == y) continue;
            const int join = t.lca(x, y);
            if (x == join) std::swap(x, y);
            int steps = 0;
            for (int u = x; u != join; u = t.par[(size_t)u]) ++steps;
            int u_out = x;
            for (int s = (int)rnd((uint32_t)steps); s > 0; --s) u_out = t.par[(size_t)u_out];
            mcf::Pivot p;
            p.in_arc = (int)(k % 1000); p.join = join; p.u_in = x; p.v_in = y; p.u_out = u_out; p.v_out = t.par[(size_t)u_out];
            p.dir_in = rnd(2) ? mcf::kUp : mcf::kDown; p.change = true;
            whole_moves += x == u_out;
            mcf::rehang_subtree(tv, p, mcf::BreakNote{t.bits.data(), t.nxt.data()});
            ++total;
            check_tree(t, n, k);
            const int64_t bad = mcf::breaks_mismatches(t.bits.data(), t.nxt.data(), n);
            REQUIRE(bad == 0, "n %d pivot %ld: %lld bits of the bitmap differ from the thread list", n, k, (long long)bad);
            check_walk(t, k);
            check_hint_walk(t, k);
            if (rnd(40) == 0) {
                t.relabel();
                check_tree(t, n, k);
                REQUIRE(mcf::breaks_mismatches(t.bits.data(), t.nxt.data(), n) == 0, "n %d pivot %ld: bitmap after a relabelling", n, k);
                check_walk(t, k);
            }
        }
    }
    printf("ok: %ld pivots on trees of 63 .. 130 nodes (%ld moved a subtree as it was), %ld run walks, %ld runs emitted, %ld pieces ended inside a run, %ld hinted walks\n",
           total, whole_moves, walks, runs_seen, cut_runs, hint_walks);
    return 0;
}
