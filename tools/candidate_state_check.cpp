// candidate_state_check.cpp -- the decision state of the engine's candidate cache (mincostflow_amd/csrc/candidate_state.h) as a stand-alone
// program, to be built under -fsanitize=address,undefined and run on a CPU (DESIGN.md sections 3.4 and 4).  Needs no GPU, no HIP and is not
// loaded into Python.
//
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all candidate_state_check.cpp -o candidate_state_check
//   ./candidate_state_check [pivots per instance, default 3000]
//
// Random sparse graphs of 60-400 nodes with random states and potentials; thousands of pivots that each move 1-40 nodes, take the entering
// arc out (state 0) and let others in or flip their bound; every 20th pivot is a gap (a big subtree: its nodes are not noted, nothing is absorbed).  The
// "device" is a brute-force scan taken when a search is posted, cut to the K best keys of each of G fake workgroups plus each group's next
// key, so that thresholds arise as they do in cand_collect; an asynchronous answer is delivered 0-12 searches late.  The driver below follows
// search_begin's order: wrap, absorb, probe, decide, wait for the refresh if undecided, post.  After every search
//   * a decision that cand_decide returned equals the brute-force argmin (c, arc) of that moment,
//   * a `false` is a case where list and heap cannot tell: no list, a gap after the list's epoch, or no clean entry left on an incomplete
//     list and no arc touched after the list's epoch whose key is below the threshold -- judged from the epochs by brute force,
//   * the heap holds no entry that violates the INVARIANT of candidate_state.h.
// The scenarios that must have occurred by the end (counted, and asserted):
//   RISING   an install whose threshold is higher than the one it replaces, with arcs touched during the flight whose keys lie between the two
//   COMPLETE a complete list (threshold none)
//   PERMUTED a node permutation in the middle of a flight
//   WRAP     a start 300 epochs before the wrap of the epoch counter
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <vector>

#include "../mincostflow_amd/csrc/candidate_state.h"

namespace {

using Key = CandState::CandKey;

#define CHECK(cond, ...) do { if (!(cond)) { fprintf(stderr, "FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

struct Counts { long rising = 0, complete = 0, permuted = 0, wraps = 0, decided = 0, undecided = 0, async_posts = 0, late = 0, waits = 0, rejected = 0; };

struct Instance {
    mcf::SplitMix64 rng;
    int n, m, groups, per_group, refresh_low;
    std::vector<int32_t> src, tgt, adj_start, adj_pos;
    std::vector<int64_t> cost, pi;
    std::vector<int8_t> state;
    std::vector<CandState::AdjEnt> adj;
    CandState s;
    // the answer that is in flight
    std::vector<Key> fl_rec;
    Key fl_thr{0, kCandNone};
    uint32_t async_at = 0;
    long due = 0, searches = 0;
    Counts *cnt;

    Instance(uint64_t seed, int n_, int groups_, int per_group_, int refresh_low_, uint32_t epoch0, Counts *c)
        : rng(seed), n(n_), m(3 * n_), groups(groups_), per_group(per_group_), refresh_low(refresh_low_), cnt(c)
    {
        src.resize(m); tgt.resize(m); cost.resize(m); state.resize(m); pi.resize(n);
        for (int a = 0; a < m; ++a) {
            src[a] = (int32_t)rng.range(0, n - 1);
            tgt[a] = rng.range(0, 19) == 0 ? src[a] : (int32_t)rng.range(0, n - 1);      // a few self loops: one adjacency entry
            cost[a] = rng.range(-50, 50);
            state[a] = (int8_t)rng.range(-1, 1);
        }
        for (int u = 0; u < n; ++u) pi[u] = rng.range(-200, 0);
        build_adjacency();
        s.node_at.assign(n, 0u);
        s.arc_at.assign(m, 0u);
        cand_reset(&s);
        s.heap_gap = 0;
        s.cand_now = epoch0;
        s.heap_compact_above = (size_t)rng.range(1, 40);
    }

    CandGraph graph() const { return CandGraph{adj_start.data(), adj.data(), src.data(), tgt.data(), cost.data(), state.data(), pi.data()}; }

    void build_adjacency()          // as cand_build_adjacency lays it out
    {
        adj_start.assign(n + 1, 0);
        for (int a = 0; a < m; ++a) { adj_start[src[a] + 1]++; if (tgt[a] != src[a]) adj_start[tgt[a] + 1]++; }
        for (int u = 0; u < n; ++u) adj_start[u + 1] += adj_start[u];
        adj.assign(adj_start[n], CandState::AdjEnt{0, 0u, 0});
        adj_pos.assign((size_t)2 * m, -1);
        std::vector<int32_t> fill(adj_start.begin(), adj_start.end() - 1);
        for (int a = 0; a < m; ++a) {
            const uint32_t st_bits = (uint32_t)(state[a] + 1) << 29;
            adj_pos[2 * (size_t)a] = fill[src[a]];
            adj[fill[src[a]]++] = CandState::AdjEnt{a, (uint32_t)tgt[a] | st_bits, cost[a]};
            if (tgt[a] != src[a]) {
                adj_pos[2 * (size_t)a + 1] = fill[tgt[a]];
                adj[fill[tgt[a]]++] = CandState::AdjEnt{a, (uint32_t)src[a] | st_bits | 0x80000000u, cost[a]};
            }
        }
    }

    bool key_of(int a, Key *k) const          // eligible: its key
    {
        if (state[a] == 0) return false;
        const int64_t d = cost[a] + pi[src[a]] - pi[tgt[a]];
        const int64_t rc = state[a] > 0 ? d : -d;
        if (rc >= 0) return false;
        *k = Key{rc, (uint32_t)a};
        return true;
    }
    Key brute_min() const
    {
        Key best{0, kCandNone}, k;
        for (int a = 0; a < m; ++a) if (key_of(a, &k) && (best.p == kCandNone || cand_key_less(k, best))) best = k;
        return best;
    }
    uint32_t touched_at(int a) const { return std::max(s.arc_at[a], std::max(s.node_at[src[a]], s.node_at[tgt[a]])); }

    // the fake device: every group's per_group best keys, and the smallest key that no group reported
    void device_scan(std::vector<Key> *rec, Key *thr) const
    {
        rec->clear();
        *thr = Key{0, kCandNone};
        for (int g = 0; g < groups; ++g) {
            std::vector<Key> mine;
            Key k;
            for (int a = g; a < m; a += groups) if (key_of(a, &k)) mine.push_back(k);
            std::sort(mine.begin(), mine.end(), cand_key_less);
            for (size_t i = 0; i < mine.size() && i < (size_t)per_group; ++i) rec->push_back(mine[i]);
            if (mine.size() > (size_t)per_group && (thr->p == kCandNone || cand_key_less(mine[per_group], *thr))) *thr = mine[per_group];
        }
    }

    void check_heap(const char *when) const
    {
        for (const CandState::HeapEnt &t : s.heap) {
            CHECK(t.c < 0, "%s: a heap entry that was never eligible (arc %u)", when, t.p);
            CHECK(t.at > s.snap_at, "%s: heap entry of arc %u from epoch %u, list of epoch %u", when, t.p, t.at, s.snap_at);
            if (!s.async_posted && s.cand_valid && s.cand_thr.p != kCandNone)
                CHECK(cand_key_less(Key{t.c, t.p}, s.cand_thr), "%s: heap entry (%lld, %u) not below the threshold (%lld, %u)", when, (long long)t.c, t.p,
                      (long long)s.cand_thr.c, s.cand_thr.p);
            // a current entry carries the arc's key of this moment (unless nodes moved unseen: a gap, absorbed or still to be)
            if (s.heap_gap < t.at && !s.pivot_overflow && cand_heap_current(&s, t)) {
                Key k;
                CHECK(key_of((int)t.p, &k) && k.c == t.c, "%s: current heap entry of arc %u holds %lld", when, t.p, (long long)t.c);
                CHECK((t.u == src[t.p] && t.v == tgt[t.p]) || (t.u == tgt[t.p] && t.v == src[t.p]), "%s: end points of arc %u", when, t.p);
            }
        }
    }

    void install_flight()
    {
        if (s.cand_valid && s.cand_thr.p != kCandNone && (fl_thr.p == kCandNone || cand_key_less(s.cand_thr, fl_thr))) {
            // RISING: is there an arc touched during the flight whose key lies between the two thresholds?
            for (const CandState::HeapEnt &t : s.heap)
                if (t.at > async_at && cand_heap_current(&s, t) && !cand_key_less(Key{t.c, t.p}, s.cand_thr) && (fl_thr.p == kCandNone || cand_key_less(Key{t.c, t.p}, fl_thr))) {
                    cnt->rising += 1;
                    break;
                }
        }
        cand_install(&s, graph(), fl_rec.data(), fl_rec.size(), fl_thr, async_at);
        if (s.cand_thr.p == kCandNone) cnt->complete += 1;
        check_heap("after an asynchronous install");
    }

    // a `false` of cand_decide: list and heap cannot tell
    void check_undecided() const
    {
        if (!s.cand_valid || s.snap_at < s.heap_gap) return;
        CHECK(s.cand_thr.p != kCandNone, "undecided with a complete list and no gap");
        for (size_t i = 0; i < s.cand_list.size(); ++i)
            CHECK(touched_at((int)s.cand_list[i].p) > s.snap_at, "undecided although list entry %zu (arc %u) is clean", i, s.cand_list[i].p);
        Key k;
        for (int a = 0; a < m; ++a)
            if (touched_at(a) > s.snap_at && key_of(a, &k))
                CHECK(!cand_key_less(k, s.cand_thr), "undecided although touched arc %d has key (%lld) below the threshold (%lld, %u)", a, (long long)k.c,
                      (long long)s.cand_thr.c, s.cand_thr.p);
    }

    // one search, in search_begin's order; returns the entering arc's key
    Key search()
    {
        searches += 1;
        if (s.cand_now >= kCandEpochWrap && !s.async_posted) { cand_restart_epochs(&s); cnt->wraps += 1; }
        const int64_t offered = s.n_heap_push, admitted = s.n_heap_admit;
        cand_absorb_pivot(&s, graph());
        cnt->rejected += (s.n_heap_push - offered) - (s.n_heap_admit - admitted);
        check_heap("after the absorb");
        if (s.async_posted && searches >= due) install_flight();                      // the probe: the refresh has arrived
        Key win{0, kCandNone};
        bool decided = cand_decide(&s, &win);
        if (!decided && s.async_posted) {                                             // the refresh is what we are waiting for
            check_undecided();
            cnt->waits += 1;
            install_flight();
            decided = cand_decide(&s, &win);
        }
        const Key want = brute_min();
        if (decided) {
            cnt->decided += 1;
            CHECK(win.p == want.p && (win.p == kCandNone || win.c == want.c), "search %ld: decided (%lld, %u), the scan finds (%lld, %u)", searches, (long long)win.c, win.p,
                  (long long)want.c, want.p);
            if (!s.async_posted && s.cand_thr.p != kCandNone && s.cand_list.size() - s.cand_ptr <= (size_t)refresh_low) {
                device_scan(&fl_rec, &fl_thr);
                async_at = s.cand_now;
                s.async_posted = true;
                const long delay = (long)rng.range(0, 12);
                due = searches + 1 + delay;
                cnt->async_posts += 1;
                cnt->late += delay > 0;
            }
        } else {
            cnt->undecided += 1;
            check_undecided();
            // the device searches and is waited for: its best key is the answer, its list is of this epoch
            device_scan(&fl_rec, &fl_thr);
            cand_install(&s, graph(), fl_rec.data(), fl_rec.size(), fl_thr, s.cand_now);
            if (s.cand_thr.p == kCandNone) cnt->complete += 1;
            CHECK(s.heap.empty(), "after a waited-for request the heap holds %zu entries", s.heap.size());
            win = s.cand_list.empty() ? Key{0, kCandNone} : s.cand_list[0];
            CHECK(win.p == want.p, "search %ld: the installed list starts with arc %u, the scan finds %u", searches, win.p, want.p);
        }
        s.cand_now += 1;
        return win;
    }

    void set_state(int a, int8_t st)
    {
        state[a] = st;
        for (int side = 0; side < 2; ++side) {
            const int q = adj_pos[2 * (size_t)a + side];
            if (q >= 0) adj[q].other = (adj[q].other & ~(3u << 29)) | ((uint32_t)(st + 1) << 29);
        }
        (void)cand_state_note_arc(&s, a);
    }

    void pivot(Key entering, bool gap)
    {
        if (entering.p != kCandNone) set_state((int)entering.p, 0);
        for (int i = 0; i < 3; ++i) {        // others come in or change their bound, so that the eligible arcs do not run out
            const int leaving = (int)rng.range(0, m - 1);
            const int8_t st = rng.range(0, 1) ? 1 : -1;
            if (state[leaving] != st) set_state(leaving, st);
        }
        const int64_t sigma = rng.range(-30, 30);
        if (gap) {
            // a big subtree: taken over as it is, without a look at its nodes (cand_note_nodes_blind) -- and a refresh that has arrived
            // meanwhile is taken in there
            s.pivot_overflow = true;
            for (int u = 0; u < n; ++u) if (rng.range(0, 2) == 0) pi[u] += sigma;
            if (s.async_posted && rng.range(0, 1)) install_flight();
        } else {
            const int moved = (int)rng.range(1, 40);
            for (int i = 0; i < moved; ++i) {
                const int u = (int)rng.range(0, n - 1);
                if (s.node_at[u] == s.cand_now) continue;           // one shift per node and pivot
                pi[u] += sigma;
                (void)cand_state_note_node(&s, u, adj_start.data());
            }
        }
    }

    void permute()
    {
        std::vector<int32_t> new_of(n);
        std::iota(new_of.begin(), new_of.end(), 0);
        for (int i = n - 1; i > 0; --i) std::swap(new_of[i], new_of[rng.range(0, i)]);
        for (int a = 0; a < m; ++a) { src[a] = new_of[src[a]]; tgt[a] = new_of[tgt[a]]; }
        std::vector<int64_t> moved(n);
        for (int u = 0; u < n; ++u) moved[new_of[u]] = pi[u];
        pi = moved;
        build_adjacency();
        if (s.async_posted) cnt->permuted += 1;               // PERMUTED: the answer in flight names arcs, which keep their ids
        cand_renumber(&s, new_of.data(), n);
        check_heap("after a permutation");
    }

    void run(int pivots)
    {
        for (int it = 1; it <= pivots; ++it) {
            const Key entering = search();
            pivot(entering, it % 20 == 0);
            if (it % 37 == 0) permute();
        }
    }
};

}  // namespace

int main(int argc, char **argv)
{
    const int pivots = argc > 1 ? atoi(argv[1]) : 3000;
    Counts total;
    // {nodes, fake workgroups, records per group, list entries left when the next list is asked for, first epoch}
    const struct { int n, groups, per_group, refresh_low; uint32_t epoch0; } cases[] = {
        {60, 4, 8, 12, 1},   {61, 2, 200, 3, 1},       // COMPLETE: 2 x 200 records hold every eligible arc of 183
        {127, 4, 8, 12, kCandEpochWrap - 300},         // WRAP
        {200, 8, 6, 12, 1},  {256, 4, 6, 3, 1},  {333, 3, 11, 0, kCandEpochWrap - 300},  {400, 16, 2, 12, 1},
    };
    uint64_t seed = 13502460;
    for (const auto &c : cases) {
        Counts cnt;
        Instance inst(seed++, c.n, c.groups, c.per_group, c.refresh_low, c.epoch0, &cnt);
        inst.run(pivots);
        printf("n %3d groups %2d x %3d: decided %ld undecided %ld async %ld (late %ld, waited for %ld) | rising %ld complete %ld permuted-in-flight %ld wraps %ld | pushes %lld admitted %lld pops %lld sweeps %lld\n",
               c.n, c.groups, c.per_group, cnt.decided, cnt.undecided, cnt.async_posts, cnt.late, cnt.waits, cnt.rising, cnt.complete, cnt.permuted, cnt.wraps,
               (long long)inst.s.n_heap_push, (long long)inst.s.n_heap_admit, (long long)inst.s.n_heap_pop, (long long)inst.s.n_heap_sweeps);
        if (c.epoch0 != 1) CHECK(cnt.wraps >= 1, "the epoch counter did not wrap");
        if (c.per_group >= 200) CHECK(cnt.complete >= 1, "no complete list");
        CHECK(cnt.decided > pivots / 4, "the cache hardly decided anything");
        if (c.per_group < 200) CHECK(cnt.async_posts > 0 && cnt.late > 0,"hardly any asynchronous refresh (a complete list asks for none)");
        total.rising += cnt.rising; total.complete += cnt.complete; total.permuted += cnt.permuted; total.wraps += cnt.wraps; total.rejected += cnt.rejected;
    }
    CHECK(total.rising >= 1, "RISING did not occur");
    CHECK(total.complete >= 1, "COMPLETE did not occur");
    CHECK(total.permuted >= 1, "PERMUTED did not occur");
    CHECK(total.wraps >= 2, "WRAP did not occur");
    CHECK(total.rejected >= 1, "the admission rule never rejected a key");
    printf("candidate_state_check: ok\n");
    return 0;
}
