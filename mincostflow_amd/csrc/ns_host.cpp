// ns_host.cpp -- the sequential half of the primal network simplex, kept on the CPU.
//
// Drives the host side of the reference solver (NS.cs = src/MinCostFlow.Core/Lemon/Algorithms/
// NetworkSimplex.cs): problem set-up, standard form and the artificial-root start basis are
// ns_core.cpp; per pivot the cycle search, flow augmentation and spanning-tree surgery on the
// thread-index representation are tree_pivot.h, and what is here is their order, the walk over
// the subtree's potentials and what the engines are told.  The two data-parallel pieces --
// FindEnteringArc and the potential update -- are NOT here: they are calls into the device engine
// (engine.hip).  There is no CPU entering-arc search in this file or anywhere else in the library.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <x86intrin.h>

#include "common.h"
#include "ns_core.h"
#include "thread_breaks.h"

struct mcf_ns : mcf::NsCore {                                         // the problem, the flows and the tree: ns_core.h
    int rule = MCF_RULE_BLOCK_SEARCH;                                  // NS.cs:77
    bool optimized_pivot = false;                                      // NS.cs:34
    int vector_width = MCF_VECTOR_DEFAULT;                             // Vector<long>.Count of the reference's host (BSPO.cs:74): mcf_ns_set_vector_width
    int device = 0, int_width = 0, block_size = 0, engine_flags = 0;
    bool auto_config = true;                                           // NS.cs:90
    mcf_block_config config{};                                         // _optimizationConfig, NS.cs:89
    // Node ids in use inside a solve may differ from the caller's: renumber_nodes() relabels the nodes in thread (preorder) order so that the
    // subtree walks, the cycle searches and the engines' per-node tables run through memory front to back instead of chasing pointers.
    // new_of[caller's id] = id in use, orig_of = the inverse; empty = identity.  Arc ids never change, so no pivot rule can tell.
    std::vector<int32_t> new_of, orig_of;
    int64_t walked_since_renumber = 0, jumps_since_renumber = 0, renumbers = 0;
    bool allow_renumber = false;
    bool use_runs = true;             // after a relabelling, big walks go to the shift grid as runs of consecutive ids (it takes them as they are)
    double renumber_every = 128.0;    // relabel when the walks since the last relabelling covered this many times the node count
    double renumber_ticks = 0, renumber_last_ticks = 0, renumber_last_at = 0, renumber_jump_budget = 0;
    int64_t renumber_at_pivot = 0;
    bool renumber_forced = false;     // MCF_NS_RENUMBER set: relabel at that interval whatever it costs (tests)
    bool begun = false, prepared = false, solved = false;
    mcf::TreeView tv{};               // the arrays the steps of tree_pivot.h work on: bound by begin()
    mcf::Pivot pv;                    // the pivot being carried out
    // what the last pivot changed (the engine calls of a host)
    int n_state = 0;
    int32_t st_arc[2] = {0, 0};
    int8_t st_val[2] = {0, 0};
    mcf::hvec<int32_t> follow;      // prefetch hints of shift_potentials
    // one bit per node, set where nxt[a] != a + 1 (thread_breaks.h): empty before the first relabelling, rebuilt by every relabelling and kept
    // current by the re-hanging from then on
    std::vector<uint64_t> breaks;
    // What the last walk produced, for whoever has to tell the engines (or a caller) which potentials moved.  pivot_front resets it, the walk of
    // shift_potentials fills it (normalise_potentials: all nodes at once), hand_over_moved sends what the engines do not have yet.
    struct MovedList {
        enum Form { kNothing = 0,   // no potential moved
                    kValues,        // nodes[] and vals[], their new potentials
                    kIds,           // nodes[] alone: the engines read the bound _pi where they need a value
                    kRuns,          // run_first[] / run_len[]: runs of consecutive ids (mcf_engine_shift_potential_runs), nodes[] is not written
                    kReload };      // nothing written down: the engines reload _pi
        Form form = kNothing;
        int n = 0;                  // nodes the walk moves
        int walked = 0;             // of them, moved so far (= n once the walk is over)
        int sent = 0;               // of those, what the engines already have (handed over during the walk)
        int runs_n = 0, runs_sent = 0;
        mcf::hvec<int32_t> nodes;   // capacity n + 1 each
        mcf::hvec<int64_t> vals;
        mcf::hvec<int32_t> run_first, run_len;
        void begin(Form f, int count) { form = f; n = count; walked = sent = runs_n = runs_sent = 0; }
    } moved;
    bool shift_smaller_side = false;  // inside mcf_ns_solve with 64-bit engines: see shift_potentials
    int reload_min = 0;               // inside mcf_ns_solve: walks of at least this many nodes are announced as a reload of _pi (0: never)
    int reload_min_engines = 0;       // what the engines asked for (mcf_engine_reload_threshold), 0 when one of them only takes lists
    bool allow_smaller_side = false;
    // MCF_NS_DEBUG only (reset by every mcf_ns_solve): moved subtrees by log2 of their size -- how many, how many nodes, and where their pivots'
    // time went (ticks): the walk incl. hand-over, the wait for the search that follows, everything else of the pivot
    struct Debug {
        bool on = false;
        int64_t reload_walks = 0, over_half = 0, over_half_nodes = 0;
        int64_t n[32] = {0}, nodes[32] = {0};
        double walk[32] = {0}, wait[32] = {0}, rest[32] = {0};
        int size_class = -1;          // of the pivot whose search is being waited for
        double t_prev = 0;
        struct Buckets { double search, tree, pot, hand, begin, pieces; };      // ticks of the whole solve
        void waited(double t0, double t_got);
        void pivoted(const mcf_ns *s, double walk_ticks, double t_got);
        void report(const mcf_ns *s, int64_t it, const Buckets &t, double ns_per_tick, double tick_start) const;
    } dbg;
    int resident_workgroups = 0;      // mcf_ns_set_device_share: workgroups of this solver's resident grid (0 = the whole device)
    int engine_rc = 0;                // first error of an engine call made from inside a pivot
    double piece_ticks = 0;           // time inside the hand-over calls made during the walks (part of the potential-update bucket)
    bool hand_over = false;           // a device engine is attached: state writes and potential pieces go to it as they arise
    int64_t sigma = 0;
    // engine(s) + sharding.  kRccl / kHost: one process per GPU, this rank's engine holds one arc shard and the candidates are exchanged
    // by ncclAllGather / through shared memory; kGroup: this process drives every shard itself (peers[] next to engine)
    enum ShardMode { kWhole = 0, kRccl, kHost, kGroup };
    mcf_engine *engine = nullptr;
    std::vector<mcf_engine *> peers;          // kGroup: shards 1 .. R-1 (shard 0 is `engine`)
    std::vector<int32_t> group_devices;
    std::vector<mcf_candidate> cands;
    int shard_mode = kWhole;
    bool sharded = false;                     // kRccl
    uint8_t nccl_id[128];
    std::string exchange_name;
    mcf_exchange *exchange = nullptr;
    int rank = 0, world = 1;
    // trace / metrics
    int32_t *trace = nullptr;
    int64_t trace_cap = 0, trace_len = 0;
    int64_t pivot_limit = 0;          // 0 = none; otherwise Solve() stops after that many pivots with status NotSolved
    mcf_ns_metrics metrics{};
    // LEMON's list rules (mcf_ns_set_list_pivot_rule): 0 = none, else MCF_RULE_CANDIDATE_LIST / MCF_RULE_ALTERING_LIST.  The rule's state is
    // kept here (lemon/network_simplex.h:415-635, member for member); the engine only carries out the major scans (mcf_engine_collect_eligible)
    int list_rule = 0;
    struct ListRule {
        int list_length = 0, minor_limit = 0, curr_length = 0, minor_count = 0;   // Candidate List (_curr_length also Altering List's)
        int block_size = 0, head_length = 0;                                    // Altering List
        int next_arc = 0;
        std::vector<int32_t> candidates;
        std::vector<int64_t> cand_cost;     // Altering List: _cand_cost, indexed by arc
        std::vector<int64_t> got;           // reduced costs the device returned with the collected arcs
        double collect_ticks = 0;
    } lr;
    mcf_list_rule_stats list_stats{};
};

namespace {

inline double ticks() { return (double)__rdtsc(); }     // invariant TSC; scaled to ns once per solve

using mcf::kInf;     // tree_pivot.h

// ---- the engine calls of a pivot, fanned out to every shard this process drives (the first error ends the round)
template <class Call> int engines_each(mcf_ns *s, Call call)
{
    int rc = s->engine ? call(s->engine) : MCF_OK;
    for (size_t i = 0; i < s->peers.size() && !rc; ++i) rc = call(s->peers[i]);
    return rc;
}
int engines_search_begin(mcf_ns *s)
{
    // (RCCL-sharded engines too: their exchange has a stream of its own; a dispatching one launches its scan here)
    return engines_each(s, [](mcf_engine *e) { return mcf_engine_search_begin(e); });
}
int engines_search_end(mcf_ns *s, int32_t *found, int32_t *arc)
{
    switch (s->shard_mode) {
    case mcf_ns::kWhole: return mcf_engine_search_end(s->engine, found, arc, nullptr);
    case mcf_ns::kRccl: return mcf_engine_find_entering_sharded(s->engine, found, arc, nullptr);
    case mcf_ns::kHost: {
        mcf_candidate mine;
        int rc = mcf_engine_search_end_local(s->engine, &mine);
        if (!rc) rc = mcf_exchange_all_gather(s->exchange, &mine, s->cands.data());
        if (!rc) rc = mcf_engine_resolve(s->engine, s->world, s->cands.data(), found, arc, nullptr);
        return rc;
    }
    default: {
        int rc = mcf_engine_search_end_local(s->engine, &s->cands[0]);
        for (size_t i = 0; i < s->peers.size() && !rc; ++i) rc = mcf_engine_search_end_local(s->peers[i], &s->cands[i + 1]);
        // every shard's rule state (next_arc, adaptive block size) advances with the same global answer
        if (!rc) rc = mcf_engine_resolve(s->engine, (int32_t)s->cands.size(), s->cands.data(), found, arc, nullptr);
        for (size_t i = 0; i < s->peers.size() && !rc; ++i) {
            int32_t f2 = 0, a2 = -1;
            rc = mcf_engine_resolve(s->peers[i], (int32_t)s->cands.size(), s->cands.data(), &f2, &a2, nullptr);
        }
        return rc;
    }
    }
}
void engines_destroy(mcf_ns *s)
{
    engines_each(s, [](mcf_engine *e) { mcf_engine_destroy(e); return MCF_OK; });
    s->engine = nullptr;
    s->peers.clear();
    if (s->exchange) { mcf_exchange_close(s->exchange); s->exchange = nullptr; }
}

// ---- NS.cs:1030-1039, before the flows are touched: the State[] writes of the pivot, kept for the engines
void decide_states(mcf_ns *s)
{
    s->n_state = 0;
    auto set_state = [&](int arc, int8_t v) {
        s->state[arc] = v;
        s->st_arc[s->n_state] = arc;
        s->st_val[s->n_state] = v;
        s->n_state++;
    };
    const mcf::Pivot &p = s->pv;
    if (p.change) {
        set_state(p.in_arc, MCF_STATE_TREE);
        set_state(s->par_arc[p.u_out], mcf::leaving_state(s->tv, p));
    } else {
        set_state(p.in_arc, (int8_t)-p.in_state);
    }
}

// ---- NS.cs:1185-1209: host copy of pi is kept current (sigma needs pi[v_in], pi[u_in]); what the walk writes down (mcf_ns::MovedList) is what
// the engines are told.
// The subtree of u_in is the thread segment u_in .. LastSucc[u_in], SuccNum[u_in] nodes long; NS.cs:1196-1208 walks it front to back,
// one dependent load per node, and that latency chain is what a big subtree costs (2 % of config 3's pivots move 24 000 nodes on
// average and carry 92 % of all moved nodes).  The same walk here, in four steps that change neither the set of nodes nor their values:
//  1. the SIDE: the subtree, or (inside a solve) everything else when that is smaller;
//  2. the FORM in which the engines hear of it: nodes with values, nodes alone, runs of consecutive ids, or "reload _pi";
//  3. the WALKER: from both ends at once below kWalkHintMin nodes (Thread forwards, RevThread backwards: two independent chains); above,
//     mcf::HintWalk before the first relabelling and mcf::BreakWalk after it (thread_breaks.h);
//  4. the PIECES: a long list is handed to the engines while the walk goes on (walk_in_pieces, hand_over_moved).
// The order of the resulting list is irrelevant to the engine (final values).
using mcf::kWalkAhead;
constexpr int kWalkHintMin = 48;
static_assert(kWalkHintMin > kWalkAhead, "a hinted walk is longer than its hints reach");
// What a step of a walk that leaves the id order is charged when the next relabelling is scheduled.  It was the scalar run loop's cost of a
// jump (a mispredicted branch and then a miss, 23 - 25 ns); the walker of thread_breaks.h overlaps its jumps' misses and pays less than half of
// that, but a jump is also one more run for the engines to take, and the budget did not follow the walk down: charged 9 ns (2.7 times the
// budget) config 3 was 1 - 7 % slower in 6 of 6 alternations, with or without an earlier first relabelling.
constexpr double kJumpNs = 24.0;
constexpr int kRunsMin = 512;      // walks of this many nodes and more hand over runs of consecutive ids (after a relabelling)
constexpr int kWalkPiece = 2048;   // a big walk hands its nodes to the engine in pieces of this size (mcf_engine_append_potential);
                                   // 1024 .. 8192 measure alike on config 3, no hand-over at all costs 0.9 us per pivot

// ---- the hand-over: what the engines do not have yet of the moved list, in the list's form.  During a walk (between pieces), once after
// pivot_front, and for normalise_potentials.  An engine's error is kept in engine_rc, and nothing more is sent after one.
void hand_over_moved(mcf_ns *s)
{
    using M = mcf_ns::MovedList;
    M &m = s->moved;
    if (m.sent == m.walked) return;
    if (!s->engine_rc) s->engine_rc = engines_each(s, [&](mcf_engine *e) {       // the potentials are replicated on every shard
        switch (m.form) {
        case M::kRuns: return mcf_engine_shift_potential_runs(e, m.runs_n - m.runs_sent, m.run_first.data() + m.runs_sent, m.run_len.data() + m.runs_sent, s->sigma);
        case M::kReload: return mcf_engine_reload_potentials(e, m.n);
        default: return mcf_engine_shift_potential(e, m.walked - m.sent, m.nodes.data() + m.sent, m.form == M::kValues ? m.vals.data() + m.sent : nullptr, s->sigma);
        }
    });
    m.sent = m.walked;
    m.runs_sent = m.runs_n;
}

// ---- the piece loop: advance(k) moves the walker over the next k nodes of the list begun in s->moved.  With engines attached, a list is handed
// over every kWalkPiece nodes as long as at least half a piece is still to come: the grid applies the piece while the walk goes on (resident
// mode), and the hand-over after the pivot finishes the list.  (A reload has no pieces: there is no list.)
template <class Advance> void walk_in_pieces(mcf_ns *s, Advance advance)
{
    mcf_ns::MovedList &m = s->moved;
    const bool pieces = s->hand_over && m.form != mcf_ns::MovedList::kReload;
    while (m.walked < m.n) {
        const int stop = pieces && m.n - (m.walked + kWalkPiece) >= kWalkPiece / 2 ? m.walked + kWalkPiece : m.n;
        advance(stop - m.walked);
        m.walked = stop;
        if (stop < m.n) {
            const double tp = ticks();
            hand_over_moved(s);
            s->piece_ticks += ticks() - tp;
        }
    }
}

// fewer than kWalkHintMin nodes: from both ends at once, nodes with values
void walk_from_both_ends(mcf_ns *s, int first, int last, int64_t sigma)
{
    mcf_ns::MovedList &m = s->moved;
    int32_t *const nodes = m.nodes.data();
    int64_t *const vals = m.vals.data();
    int64_t *const pi = s->pi.data();
    const int32_t *const nxt = s->nxt.data(), *const prv = s->prv.data();
    int lo = 0, hi = m.n - 1;
    int a = first, b = last;
    while (lo < hi) {
        nodes[lo] = a; vals[lo] = (pi[a] += sigma); a = nxt[a]; ++lo;
        nodes[hi] = b; vals[hi] = (pi[b] += sigma); b = prv[b]; --hi;
    }
    if (lo == hi) { nodes[lo] = a; vals[lo] = (pi[a] += sigma); }
    m.walked = m.n;
}

void shift_potentials(mcf_ns *s)
{
    using M = mcf_ns::MovedList;
    // runs BEFORE the re-hanging: the nodes that move are the subtree of u_out as it hangs now, and u_in's new parent direction is known
    const int u_out = s->pv.u_out;
    s->sigma = mcf::pivot_sigma(s->pv, s->pi.data(), s->cost.data());
    // 1. the side
    int count = s->sub[u_out];
    int first = u_out, last = s->fin[u_out];
    // (the common offset pi[root] that this builds up is bounded: past 2^60 the complement is never walked again, so it stops growing and every
    // potential stays representable -- the reference's values differ from ours by exactly that offset until normalise_potentials takes it out)
    if (s->shift_smaller_side && (s->pi[s->root] > (1ll << 60) || s->pi[s->root] < -(1ll << 60))) s->shift_smaller_side = false;
    if (s->shift_smaller_side && 2 * (int64_t)count > (int64_t)s->n + 1) {
        // Reduced costs only see differences of potentials: moving the subtree by sigma and moving EVERYTHING ELSE by -sigma give the same
        // search results.  Inside mcf_ns_solve the smaller side is walked -- the rest of the preorder list, from the node after the
        // subtree's last one round to the node before u_out, the root included -- and the common offset (it is pi[root], which the
        // reference keeps at 0) is taken out again before the solve returns (normalise_potentials).
        s->sigma = -s->sigma;
        first = s->nxt[last];
        last = s->prv[u_out];
        count = s->n + 1 - count;
    }
    const int64_t sigma = s->sigma;
    // 2. the form.  A walk of reload_min nodes (never below kWalkHintMin) is cheaper for the engines as "reload _pi" than as a list: nothing is
    // written down, the walk only moves the potentials.  After a relabelling the engines have _pi bound (mcf_engine_bind_potentials) and a list
    // goes without values; from kRunsMin nodes on it goes as one {first id, length} pair per run -- the walk stores nothing per node but the
    // potential itself, and the engines get a list an order of magnitude shorter (the register-resident candidate grid takes the pairs as
    // they are).
    const bool relabelled = s->renumbers > 0;
    M &m = s->moved;
    m.begin(s->reload_min > 0 && count >= s->reload_min ? M::kReload
            : count < kWalkHintMin || !relabelled       ? M::kValues
            : s->use_runs && count >= kRunsMin          ? M::kRuns
                                                        : M::kIds,
            count);
    if (m.form == M::kReload && s->dbg.on) s->dbg.reload_walks += 1;
    // 3. the walker, 4. in pieces
    if (count < kWalkHintMin) { walk_from_both_ends(s, first, last, sigma); return; }
    if (relabelled) {
        // In thread order the successor of node a is a + 1 almost everywhere: RUNS of consecutive ids, their ends from the bitmap of thread
        // breaks, not from comparing each loaded successor, so no branch depends on a load of nxt; the load of the jump's target is issued
        // before the run's potentials are added, and the hints in follow[] (run start -> the run start kJumpAhead jumps later) have the misses
        // of several jumps in flight at once.  (Measured and dropped: eight successors compared per AVX2 step -- slower on the runs of 16 that
        // the solves have; the bitmap without hints, and hints on the scalar loop without the bitmap -- neither gains on a cold cache,
        // DESIGN.md section 4.)
        mcf::BreakWalk w;
        w.pi = s->pi.data(); w.nxt = s->nxt.data(); w.follow = s->follow.data(); w.bits = s->breaks.data();
        w.sigma = sigma; w.a = first;
        if (m.form == M::kRuns) {
            int32_t *const rf = m.run_first.data(), *const rl = m.run_len.data();
            int nr = 0;
            walk_in_pieces(s, [&](int k) { w.advance(k, [&](int start, int len) { rf[nr] = start; rl[nr] = len; ++nr; }); m.runs_n = nr; });
        } else if (m.form == M::kIds) {
            int32_t *out = m.nodes.data();
            walk_in_pieces(s, [&](int k) { w.advance(k, [&](int start, int len) { for (int j = 0; j < len; ++j) out[j] = start + j; out += len; }); });
        } else {
            walk_in_pieces(s, [&](int k) { w.advance(k, [](int, int) {}); });
        }
        s->jumps_since_renumber += w.jumps;
    } else {
        mcf::HintWalk w;
        w.pi = s->pi.data(); w.nxt = s->nxt.data(); w.follow = s->follow.data();
        w.sigma = sigma; w.a = first;
        if (m.form == M::kValues) {
            int32_t *const nodes = m.nodes.data();
            int64_t *const vals = m.vals.data();
            int i = 0;
            walk_in_pieces(s, [&](int k) { w.advance(k, [&](int a, int64_t v) { nodes[i] = a; vals[i] = v; ++i; }); });
        } else {
            walk_in_pieces(s, [&](int k) { w.advance(k, [](int, int64_t) {}); });
        }
    }
}

// pi[root] back to 0 (where the reference keeps it; the smaller-side walks let it drift) without telling an engine: every potential moves
// by -pi[root].  Returns what pi[root] was.
int64_t zero_root_potential(mcf::NsCore *s)
{
    const int64_t off = s->pi[s->root];
    if (off != 0) for (int u = 0; u <= s->n; ++u) s->pi[u] -= off;
    return off;
}

// the same at the end of a solve, where the engines hear of it: as one list of all nodes, or as a reload of _pi
int normalise_potentials(mcf_ns *s)
{
    using M = mcf_ns::MovedList;
    const int64_t off = zero_root_potential(s);
    if (off == 0) return MCF_OK;
    const int total = s->n + 1;
    M &m = s->moved;
    s->sigma = -off;
    m.begin(s->reload_min > 0 ? M::kReload : M::kValues, total);
    if (m.form == M::kValues) for (int u = 0; u < total; ++u) { m.nodes[u] = u; m.vals[u] = s->pi[u]; }
    m.walked = total;
    hand_over_moved(s);
    return s->engine_rc;
}

// Everything indexed by node moves to to[its id], every node id kept in those arrays and every arc's end points are translated; arc ids,
// states, flows, costs stay where they are.
void apply_node_permutation(mcf_ns *s, const std::vector<int32_t> &to)
{
    const int N = s->n + 1;
    auto permute = [&](auto &vec) {                 // in place: the engines have the potentials' storage bound (and registered with HIP)
        using E = typename std::remove_reference<decltype(vec)>::type::value_type;
        std::vector<E> tmp((size_t)N);
        for (int u = 0; u < N; ++u) tmp[to[u]] = vec[u];
        std::copy(tmp.begin(), tmp.end(), vec.begin());
    };
    auto translate = [&](auto &vec) { for (int u = 0; u < N; ++u) if (vec[u] >= 0) vec[u] = to[vec[u]]; };
    permute(s->supply); permute(s->pi); permute(s->par); permute(s->par_arc); permute(s->nxt); permute(s->prv); permute(s->sub); permute(s->fin);
    permute(s->par_dir); permute(s->follow);
    translate(s->par); translate(s->nxt); translate(s->prv); translate(s->fin); translate(s->follow);
    const size_t A = s->tail.size();
    for (size_t e = 0; e < A; ++e) { s->tail[e] = to[s->tail[e]]; s->head[e] = to[s->head[e]]; }
}

// Relabels the nodes so that id order = current thread order (root keeps id n).  perm_out (optional) receives new id per CURRENT id.
void renumber_nodes(mcf_ns *s, std::vector<int32_t> *perm_out)
{
    const int n = s->n, N = n + 1;
    std::vector<int32_t> to(N);                      // current id -> new id
    {
        int u = s->nxt[s->root];
        for (int k = 0; k < n; ++k) { to[u] = k; u = s->nxt[u]; }
        to[s->root] = n;
    }
    apply_node_permutation(s, to);
    if (s->new_of.empty()) {
        s->new_of = to;
    } else {
        for (int v = 0; v < N; ++v) s->new_of[v] = to[s->new_of[v]];
    }
    s->orig_of.assign(N, 0);
    for (int v = 0; v < N; ++v) s->orig_of[s->new_of[v]] = v;
    // the pivot in progress (none between pivots, but keep the fields meaningful)
    auto tr1 = [&](int32_t &x) { if (x >= 0) x = to[x]; };
    tr1(s->pv.join); tr1(s->pv.u_in); tr1(s->pv.v_in); tr1(s->pv.u_out); tr1(s->pv.v_out);
    s->walked_since_renumber = 0; s->jumps_since_renumber = 0; s->renumbers += 1;
    s->breaks.resize(mcf::breaks_words(n));
    mcf::breaks_rebuild(s->breaks.data(), s->nxt.data(), n);
    if (perm_out) perm_out->swap(to);
}

// back to the caller's ids (end of a solve)
void restore_node_ids(mcf_ns *s)
{
    if (s->new_of.empty()) return;
    apply_node_permutation(s, s->orig_of);      // id in use -> caller's id
    s->new_of.clear(); s->orig_of.clear();
    // walks after this (the stepwise API) still go run by run, over the caller's ids: the bitmap follows
    if (!s->breaks.empty()) mcf::breaks_rebuild(s->breaks.data(), s->nxt.data(), s->n);
}

// ---- When to relabel.  The first time: when the walks have covered renumber_every times the node count, or a quarter of n pivots have passed
// (the cycle searches and the candidate cache's re-evaluation of the moved nodes' arcs chase the same ids).  After that the walks count
// their JUMPS -- the steps that leave the id order, charged kJumpNs each, which is what a relabelling buys back -- and the next relabelling
// comes when the jumps since the last one have cost five times what that one took (2.9 ms with 400 k arcs, 0.3 s with 9 M: the engines
// rebuild their per-node tables).  Config 5, whole solve: 28.9 s with the 4 relabellings of the first policy (a fixed interval, and never
// before 25 times the last one's duration), 26.7 with 6, 27.9 with 12; config 3: flat between 6 and 13.  MCF_NS_RENUMBER=x forces an interval.
bool relabelling_due(const mcf_ns *s, int64_t it)
{
    if (!s->allow_renumber) return false;
    const bool walked_enough = (double)s->walked_since_renumber > s->renumber_every * (s->n + 1);
    if (s->renumber_forced) return walked_enough;
    if (s->renumbers == 0) return walked_enough || 4 * (it - s->renumber_at_pivot) > (int64_t)s->n;
    return (double)s->jumps_since_renumber > s->renumber_jump_budget;
}

// relabels the nodes in thread order, here and in the engines, before pivot `it`; sets the jump budget up to the next time
int relabel(mcf_ns *s, int64_t it, double t_start, double tick_start)
{
    const double tr0 = ticks();
    std::vector<int32_t> perm;
    renumber_nodes(s, &perm);
    const int rc = engines_each(s, [&](mcf_engine *e) { return mcf_engine_renumber_nodes(e, perm.data()); });
    s->renumber_last_ticks = ticks() - tr0;
    s->renumber_last_at = ticks();
    s->renumber_at_pivot = it;
    const double ns_per_tick_now = (mcf::now_ns() - t_start) / std::max(1.0, ticks() - tick_start);
    s->renumber_jump_budget = 5.0 * s->renumber_last_ticks * ns_per_tick_now / kJumpNs;     // jumps that cost five times this relabelling
    s->renumber_ticks += s->renumber_last_ticks;
    return rc;
}

// One pivot with a given entering arc, in two halves.  pivot_front does what the next search depends on -- the cycle, the State[] writes and
// the potentials of the subtree that is about to move (handed to the engine as they arise) -- and returns true when the problem is
// found unbounded (NS.cs:321-325).  pivot_back does the rest (flows around the cycle, re-hanging the subtree): the solve loop runs it
// while the device is already searching.
bool pivot_front(mcf_ns *s, int arc, double *t_pot)
{
    s->moved.begin(mcf_ns::MovedList::kNothing, 0);
    s->sigma = 0;
    s->pv = mcf::find_cycle(s->tv, arc, s->state[arc]);
    const mcf::Pivot &p = s->pv;
    if (!p.change && p.delta == 0) return true;
    decide_states(s);
    // the engine hears about the state writes before any piece of the potential list (the pieces may start travelling at once)
    if (s->hand_over && !s->engine_rc)       // (every engine keeps the writes that fall into its shard)
        s->engine_rc = engines_each(s, [&](mcf_engine *e) { return mcf_engine_patch_state(e, s->n_state, s->st_arc, s->st_val); });
    if (p.delta == 0) s->metrics.degenerate_pivots++;
    if (p.change) {
        const double t1 = ticks();
        shift_potentials(s);
        if (t_pot) *t_pot += ticks() - t1;
    }
    return false;
}

void pivot_back(mcf_ns *s, double *t_tree)
{
    mcf::push_flow(s->tv, s->pv);
    if (s->pv.change) {
        const double t0 = ticks();
        if (s->breaks.empty()) mcf::rehang_subtree(s->tv, s->pv);
        else mcf::rehang_subtree(s->tv, s->pv, mcf::BreakNote{s->breaks.data(), s->nxt.data()});
        if (t_tree) *t_tree += ticks() - t0;
    }
}

bool pivot(mcf_ns *s, int arc, double *t_tree, double *t_pot)
{
    if (pivot_front(s, arc, t_pot)) return true;
    pivot_back(s, t_tree);
    return false;
}

// ---- LEMON's Candidate List and Altering List rules (lemon/network_simplex.h:415-635) on this driver's _state, _pi, _cost: minor iterations,
// the re-check of the list and the partial sort here, the major scans on the device.  m_s = _searchArcNum of the C# driver (m + n).
void list_rule_init(mcf_ns *s)
{
    auto &L = s->lr;
    L = mcf_ns::ListRule{};
    const int m_s = s->search_arcs;
    s->list_stats = mcf_list_rule_stats{};
    s->list_stats.rule = s->list_rule;
    if (s->list_rule == MCF_RULE_CANDIDATE_LIST) {
        // ns.h:444-455
        const double LIST_LENGTH_FACTOR = 0.25;
        const int MIN_LIST_LENGTH = 10;
        const double MINOR_LIMIT_FACTOR = 0.1;
        const int MIN_MINOR_LIMIT = 3;
        L.list_length = std::max(int(LIST_LENGTH_FACTOR * std::sqrt(double(m_s))), MIN_LIST_LENGTH);
        L.minor_limit = std::max(int(MINOR_LIMIT_FACTOR * L.list_length), MIN_MINOR_LIMIT);
        L.curr_length = L.minor_count = 0;
        L.candidates.resize(L.list_length);
        L.got.resize(L.list_length);
        s->list_stats.list_length = L.list_length;
        s->list_stats.minor_limit = L.minor_limit;
    } else {
        // ns.h:552-569
        const double BLOCK_SIZE_FACTOR = 1.0;
        const int MIN_BLOCK_SIZE = 10;
        const double HEAD_LENGTH_FACTOR = 0.01;
        const int MIN_HEAD_LENGTH = 3;
        L.block_size = std::max(int(BLOCK_SIZE_FACTOR * std::sqrt(double(m_s))), MIN_BLOCK_SIZE);
        L.head_length = std::max(int(HEAD_LENGTH_FACTOR * L.block_size), MIN_HEAD_LENGTH);
        L.candidates.resize(L.head_length + L.block_size);
        L.got.resize(L.head_length + L.block_size);
        L.cand_cost.assign((size_t)m_s, 0);
        L.curr_length = 0;
        s->list_stats.list_length = L.head_length + L.block_size;
        s->list_stats.block_size = L.block_size;
        s->list_stats.head_length = L.head_length;
    }
}

inline int64_t host_reduced_cost(const mcf_ns *s, int e)     // ns.h:469 / :577
{
    return s->state[e] * (s->cost[e] + s->pi[s->tail[e]] - s->pi[s->head[e]]);
}

// the device scan of a major iteration: `capacity` entries at out / L.got
int list_collect(mcf_ns *s, const mcf_collect_request &rq, int32_t capacity, int32_t *out, int32_t *count, int32_t *end)
{
    const double t0 = ticks();
    int64_t scanned = 0;
    const int rc = mcf_engine_collect_eligible(s->engine, &rq, capacity, count, out, s->lr.got.data(), end, &scanned);
    s->lr.collect_ticks += ticks() - t0;
    s->list_stats.major_scans += 1;
    s->list_stats.device_arcs_read += s->search_arcs;
    s->list_stats.lemon_arcs_scanned += scanned;
    s->list_stats.collected += *count;
    return rc;
}

int list_find_entering(mcf_ns *s, int32_t *found, int32_t *in_arc)
{
    auto &L = s->lr;
    s->list_stats.searches += 1;
    *found = 0;
    if (s->list_rule == MCF_RULE_CANDIDATE_LIST) {
        // ns.h:458-508
        int64_t min, c;
        int e;
        if (L.curr_length > 0 && L.minor_count < L.minor_limit) {
            // Minor iteration: select the best eligible arc from the current candidate list
            ++L.minor_count;
            min = 0;
            for (int i = 0; i < L.curr_length; ++i) {
                e = L.candidates[i];
                c = host_reduced_cost(s, e);
                if (c < min) {
                    min = c;
                    *in_arc = e;
                } else if (c >= 0) {
                    L.candidates[i--] = L.candidates[--L.curr_length];
                }
            }
            if (min < 0) { s->list_stats.host_answered += 1; *found = 1; return MCF_OK; }
        }
        // Major iteration: build a new candidate list (the device collects the first _list_length eligible arcs from _next_arc on)
        const mcf_collect_request rq{L.next_arc, MCF_COLLECT_FIRST_N, L.list_length, 0, 0, 0};
        int32_t k = 0, end = L.next_arc;
        const int rc = list_collect(s, rq, L.list_length, L.candidates.data(), &k, &end);
        if (rc) return rc;
        min = 0;
        L.curr_length = k;
        for (int i = 0; i < k; ++i) {
            if (L.got[i] < min) {
                min = L.got[i];
                *in_arc = L.candidates[i];
            }
        }
        if (L.curr_length == 0) return MCF_OK;
        L.minor_count = 1;
        L.next_arc = end;
        *found = 1;
        return MCF_OK;
    }
    // ns.h:573-631.  Check the current candidate list
    for (int i = 0; i != L.curr_length; ++i) {
        const int e = L.candidates[i];
        const int64_t c = host_reduced_cost(s, e);
        if (c < 0) {
            L.cand_cost[e] = c;
        } else {
            L.candidates[i--] = L.candidates[--L.curr_length];
        }
    }
    // Extend the list (the device scans the blocks from _next_arc on and returns the eligible arcs up to LEMON's stop)
    const mcf_collect_request rq{L.next_arc, MCF_COLLECT_BLOCKS, 0, L.block_size, L.head_length, L.curr_length};
    int32_t k = 0, end = L.next_arc;
    const int rc = list_collect(s, rq, (int32_t)L.candidates.size() - L.curr_length, L.candidates.data() + L.curr_length, &k, &end);
    if (rc) return rc;
    for (int i = 0; i < k; ++i) L.cand_cost[L.candidates[L.curr_length + i]] = L.got[i];
    L.curr_length += k;
    if (L.curr_length == 0) return MCF_OK;
    // Perform partial sort operation on the candidate list (libstdc++'s, as LEMON built with g++ runs it: ties resolve alike)
    const int new_length = std::min(L.head_length + 1, L.curr_length);
    const int64_t *const cc = L.cand_cost.data();
    std::partial_sort(L.candidates.begin(), L.candidates.begin() + new_length, L.candidates.begin() + L.curr_length,
                      [cc](int left, int right) { return cc[left] < cc[right]; });
    // Select the entering arc and remove it from the list
    *in_arc = L.candidates[0];
    L.next_arc = end;
    L.candidates[0] = L.candidates[new_length - 1];
    L.curr_length = new_length - 1;
    *found = 1;
    return MCF_OK;
}

int begin(mcf_ns *s, int32_t *status)
{
    s->status = MCF_NOT_SOLVED;
    s->metrics = mcf_ns_metrics{};
    s->trace_len = 0;
    if (s->begun) return mcf::fail(MCF_ERR_STATE, "Solve() is single-shot: the reference mutates bounds and supplies in place (NS.cs:649, D11); create a new solver");
    s->begun = true;
    // the vectors were sized by core_create and are never resized; renumber_nodes and restore_node_ids permute them in place, so the view
    // stays valid across a relabelling
    s->tv = s->tree();
    mcf::core_begin(s);                                  // Infeasible on an inverted bound pair (NS.cs:227-231), else the start basis
    if (status) *status = s->status;
    return MCF_OK;
}

int pick_int_width(const mcf_ns *s)
{
    if (s->int_width == 32 || s->int_width == 64) return s->int_width;
    // |pi| <= ART_COST + n * max|cost| <= 2 * ART_COST; the device forms cost + pi - pi in 64 bits, so each
    // operand just has to fit int32.  ART_COST = (max|cost| + 1) * n (NS.cs:668).
    const __int128 bound = (__int128)4 * s->art_cost;
    return bound < (__int128)INT32_MAX ? 32 : 64;
}

}  // namespace

// ---- MCF_NS_DEBUG: the per-pivot bookkeeping and the report on stderr
void mcf_ns::Debug::waited(double t0, double t_got)
{
    if (size_class >= 0) { wait[size_class] += t_got - t0; rest[size_class] += t0 - t_prev; }
}

void mcf_ns::Debug::pivoted(const mcf_ns *s, double walk_ticks, double t_got)
{
    const int moved_n = s->moved.n;
    const int b = moved_n > 0 ? 31 - __builtin_clz((unsigned)moved_n) + 1 : 0;      // class 0: nothing moved; class b: 2^(b-1) .. 2^b - 1 nodes
    size_class = b;
    n[b] += 1; nodes[b] += moved_n;
    walk[b] += walk_ticks;              // walk + hand-over + posting the search
    t_prev = t_got + walk_ticks;        // what remains until the next wait begins is "rest" (cycle search, flows, tree)
    if (2 * (int64_t)moved_n > s->n) { over_half += 1; over_half_nodes += moved_n; }
}

void mcf_ns::Debug::report(const mcf_ns *s, int64_t it, const Buckets &t, double ns_per_tick, double tick_start) const
{
    fprintf(stderr, "[ns] per pivot ns: search wait %.0f | walk %.0f | pieces handed over during walks %.0f | last hand-over %.0f | search begin %.0f | tree %.0f | everything else %.0f\n",
            t.search * ns_per_tick / it, (t.pot - t.hand - t.begin - t.pieces) * ns_per_tick / it, t.pieces * ns_per_tick / it, t.hand * ns_per_tick / it, t.begin * ns_per_tick / it, t.tree * ns_per_tick / it,
            ((ticks() - tick_start) - t.search - t.pot - t.tree) * ns_per_tick / it);
    fprintf(stderr, "[ns] pivots by size of the moved subtree: nodes | pivots | share of pivots | nodes moved | us per pivot: walk+hand-over, search wait, rest | share of the solve\n");
    const double all_ticks = std::max(1.0, ticks() - tick_start);
    for (int b = 0; b < 32; ++b) {
        if (!n[b]) continue;
        const double k = (double)n[b], us = ns_per_tick / 1e3;
        char label[48];
        if (b == 0) snprintf(label, sizeof(label), "0");
        else if (b == 1) snprintf(label, sizeof(label), "1");
        else snprintf(label, sizeof(label), "%d-%d", 1 << (b - 1), (1 << b) - 1);
        fprintf(stderr, "[ns]   %14s | %8lld | %5.1f %% | %11lld | %7.2f %7.2f %7.2f | %5.1f %%\n", label, (long long)n[b], 100.0 * k / (double)it, (long long)nodes[b],
                walk[b] * us / k, wait[b] * us / k, rest[b] * us / k, 100.0 * (walk[b] + wait[b] + rest[b]) / all_ticks);
    }
    fprintf(stderr, "[ns] more than half of the %d nodes: %lld pivots / %lld nodes | walks announced as a reload of _pi (%d nodes and more): %lld | nodes relabelled in thread order %lld times, %.1f ms (%.1f %% of the steps since the last time left the id order)\n", s->n, (long long)over_half,
            (long long)over_half_nodes, s->reload_min_engines, (long long)reload_walks, (long long)s->renumbers, s->renumber_ticks * ns_per_tick / 1e6, 100.0 * (double)s->jumps_since_renumber / std::max<double>(1.0, (double)s->walked_since_renumber));
}

extern "C" {

int mcf_ns_create(mcf_ns **out, int32_t node_count, int32_t arc_count, const int32_t *source, const int32_t *target)
{
    if (!out) return mcf::fail(MCF_ERR_INVALID, "mcf_ns_create: null argument");
    *out = nullptr;
    mcf_ns *s = new mcf_ns();
    if (const int rc = mcf::core_create(s, node_count, arc_count, source, target)) { delete s; return rc; }
    mcf_block_config_default(&s->config);
    const size_t N = (size_t)node_count + 1;
    s->moved.nodes.assign(N, 0); s->moved.vals.assign(N, 0); s->follow.assign(N, 0);
    s->moved.run_first.assign(N, 0); s->moved.run_len.assign(N, 0);
    *out = s;
    return MCF_OK;
}

void mcf_ns_destroy(mcf_ns *s)
{
    if (!s) return;
    engines_destroy(s);
    delete s;
}

int mcf_ns_set_arc_bounds(mcf_ns *s, int32_t arc, int64_t lower, int64_t upper)
{
    if (!s || arc < 0 || arc >= s->m) return mcf::fail(MCF_ERR_INVALID, "Invalid arc");
    s->lower[arc] = lower;
    s->upper[arc] = upper == MCF_INF_CAP ? kInf : upper;
    s->orig_lower[arc] = lower;
    return MCF_OK;
}
int mcf_ns_set_arc_cost(mcf_ns *s, int32_t arc, int64_t cost)
{
    if (!s || arc < 0 || arc >= s->m) return mcf::fail(MCF_ERR_INVALID, "Invalid arc");
    s->cost[arc] = cost;
    return MCF_OK;
}
int mcf_ns_set_node_supply(mcf_ns *s, int32_t node, int64_t supply)
{
    if (!s || node < 0 || node >= s->n) return mcf::fail(MCF_ERR_INVALID, "Invalid node");
    s->supply[node] = supply;
    return MCF_OK;
}
int mcf_ns_set_problem(mcf_ns *s, const int64_t *lower, const int64_t *upper, const int64_t *cost, const int64_t *supply)
{
    if (!s) return mcf::fail(MCF_ERR_INVALID, "null solver");
    mcf::core_set_problem(s, lower, upper, cost, supply);
    return MCF_OK;
}
int mcf_ns_set_supply_type(mcf_ns *s, int32_t type)
{
    if (!s || (type != MCF_SUPPLY_GEQ && type != MCF_SUPPLY_LEQ)) return mcf::fail(MCF_ERR_INVALID, "bad supply type");
    s->supply_type = type;
    return MCF_OK;
}
int mcf_ns_set_pivot_rule(mcf_ns *s, int32_t rule)
{
    if (!s) return mcf::fail(MCF_ERR_INVALID, "null solver");
    if (rule < 0 || rule > 2) return mcf::fail(MCF_ERR_INVALID, "Pivot rule %d not implemented yet (NS.cs:884)", rule);
    s->rule = rule;
    s->list_rule = 0;
    return MCF_OK;
}
int mcf_ns_set_list_pivot_rule(mcf_ns *s, int32_t rule)
{
    if (!s) return mcf::fail(MCF_ERR_INVALID, "null solver");
    if (rule != MCF_RULE_CANDIDATE_LIST && rule != MCF_RULE_ALTERING_LIST)
        return mcf::fail(MCF_ERR_INVALID, "mcf_ns_set_list_pivot_rule: %d is not a list rule (3 = Candidate List, 4 = Altering List)", rule);
    s->list_rule = rule;
    return MCF_OK;
}
int mcf_ns_enable_optimized_pivot(mcf_ns *s, int32_t enable)
{
    if (!s) return mcf::fail(MCF_ERR_INVALID, "null solver");
    s->optimized_pivot = enable != 0;
    return MCF_OK;
}
int mcf_ns_set_vector_width(mcf_ns *s, int32_t vector_width)
{
    if (!s) return mcf::fail(MCF_ERR_INVALID, "null solver");
    if (vector_width != MCF_VECTOR_DEFAULT && vector_width != MCF_VECTOR_NONE && vector_width != 2 && vector_width != 4 && vector_width != 8)
        return mcf::fail(MCF_ERR_INVALID, "vector_width %d is not Vector<long>.Count of any machine (2, 4, 8, MCF_VECTOR_NONE, or 0 = 4)", vector_width);
    s->vector_width = vector_width;
    return MCF_OK;
}
int mcf_ns_set_optimization_config(mcf_ns *s, const mcf_block_config *config)       // NS.cs:557-561
{
    if (!s) return mcf::fail(MCF_ERR_INVALID, "null solver");
    if (!config) return mcf::fail(MCF_ERR_INVALID, "config must not be null (ArgumentNullException, NS.cs:559)");
    s->config = *config;
    s->auto_config = false;
    return MCF_OK;
}
int mcf_ns_enable_optimizations(mcf_ns *s, int32_t flags)                            // NS.cs:549-552
{
    if (!s) return mcf::fail(MCF_ERR_INVALID, "null solver");
    s->config.flags = flags;
    return MCF_OK;
}
int mcf_ns_set_auto_configuration(mcf_ns *s, int32_t enable)                         // NS.cs:567-570
{
    if (!s) return mcf::fail(MCF_ERR_INVALID, "null solver");
    s->auto_config = enable != 0;
    return MCF_OK;
}
int mcf_ns_set_device(mcf_ns *s, int32_t device, int32_t int_width, int32_t block_size, int32_t engine_flags)
{
    if (!s || (int_width != 0 && int_width != 32 && int_width != 64) || block_size < 0 || device < 0) return mcf::fail(MCF_ERR_INVALID, "mcf_ns_set_device: bad arguments");
    s->device = device; s->int_width = int_width; s->block_size = block_size; s->engine_flags = engine_flags;
    return MCF_OK;
}
int mcf_ns_set_device_share(mcf_ns *s, int32_t resident_workgroups)
{
    if (!s || resident_workgroups < 0 || resident_workgroups > 256 || (resident_workgroups > 0 && resident_workgroups < 8))
        return mcf::fail(MCF_ERR_INVALID, "mcf_ns_set_device_share: 0 (the whole device) or 8 .. 256 workgroups");
    s->resident_workgroups = resident_workgroups;
    return MCF_OK;
}
int mcf_ns_set_sharding(mcf_ns *s, const uint8_t id[128], int32_t rank, int32_t world)
{
    if (!s || !id || world < 1 || rank < 0 || rank >= world) return mcf::fail(MCF_ERR_INVALID, "mcf_ns_set_sharding: bad arguments");
    memcpy(s->nccl_id, id, 128);
    s->rank = rank; s->world = world; s->sharded = true; s->shard_mode = mcf_ns::kRccl;   // world 1 still goes through the RCCL exchange (tests)
    return MCF_OK;
}
int mcf_ns_set_sharding_host(mcf_ns *s, const char *exchange_name, int32_t rank, int32_t world)
{
    if (!s || !exchange_name || exchange_name[0] != '/' || world < 1 || rank < 0 || rank >= world) return mcf::fail(MCF_ERR_INVALID, "mcf_ns_set_sharding_host: bad arguments");
    s->exchange_name = exchange_name;
    s->rank = rank; s->world = world; s->shard_mode = mcf_ns::kHost; s->sharded = false;
    return MCF_OK;
}
int mcf_ns_set_shard_group(mcf_ns *s, int32_t shards, const int32_t *devices)
{
    if (!s || shards < 1 || shards > 64 || !devices) return mcf::fail(MCF_ERR_INVALID, "mcf_ns_set_shard_group: bad arguments");
    for (int i = 0; i < shards; ++i) if (devices[i] < 0) return mcf::fail(MCF_ERR_INVALID, "mcf_ns_set_shard_group: negative device");
    s->group_devices.assign(devices, devices + shards);
    s->world = shards; s->rank = 0; s->shard_mode = mcf_ns::kGroup; s->sharded = false;
    return MCF_OK;
}
int mcf_ns_set_pivot_limit(mcf_ns *s, int64_t max_pivots)
{
    if (!s || max_pivots < 0) return mcf::fail(MCF_ERR_INVALID, "bad pivot limit");
    s->pivot_limit = max_pivots;
    return MCF_OK;
}
int mcf_ns_set_trace(mcf_ns *s, int32_t *trace, int64_t capacity)
{
    if (!s || capacity < 0) return mcf::fail(MCF_ERR_INVALID, "bad trace buffer");
    s->trace = trace; s->trace_cap = trace ? capacity : 0; s->trace_len = 0;
    return MCF_OK;
}
int mcf_ns_get_trace_length(mcf_ns *s, int64_t *length) { if (!s || !length) return mcf::fail(MCF_ERR_INVALID, "null argument"); *length = s->trace_len; return MCF_OK; }

int mcf_ns_begin(mcf_ns *s, int32_t *status)
{
    if (!s) return mcf::fail(MCF_ERR_INVALID, "null solver");
    return begin(s, status);
}

int mcf_ns_apply_pivot(mcf_ns *s, int32_t arc, int32_t *unbounded)
{
    if (!s) return mcf::fail(MCF_ERR_INVALID, "null solver");
    if (!s->transformed) return mcf::fail(MCF_ERR_STATE, "mcf_ns_begin has not been called (or found the bounds infeasible)");
    if (arc < 0 || arc >= s->search_arcs) return mcf::fail(MCF_ERR_INVALID, "entering arc %d outside the search range [0, %d)", arc, s->search_arcs);
    if (s->state[arc] == MCF_STATE_TREE) return mcf::fail(MCF_ERR_INVALID, "arc %d is in the basis and cannot enter", arc);
    const bool unb = pivot(s, arc, nullptr, nullptr);
    if (unb) s->status = MCF_UNBOUNDED; else s->metrics.iterations++;
    if (unbounded) *unbounded = unb ? 1 : 0;
    return MCF_OK;
}

// Measurement / test aid: `count` pivots with the given entering arcs applied back to back without an engine -- the sequential half alone
// (cycle search, flows, subtree walk, tree surgery), with the walk aids of mcf_ns_solve (smaller side, node renumbering every `renumber_every`
// walked nodes per node of the graph; 0 = never).  Phase times land in the metrics; ids are the caller's again when it returns.
int mcf_ns_replay(mcf_ns *s, const int32_t *arcs, int64_t count, int32_t smaller_side, double renumber_every)
{
    if (!s || count < 0 || (count && !arcs)) return mcf::fail(MCF_ERR_INVALID, "mcf_ns_replay: bad arguments");
    if (!s->transformed) return mcf::fail(MCF_ERR_STATE, "mcf_ns_begin has not been called");
    const double t_start = mcf::now_ns(), tick_start = ticks();
    double t_tree = 0, t_pot = 0, t_renum = 0;
    s->shift_smaller_side = smaller_side != 0;
    s->walked_since_renumber = 0;
    int64_t it = 0, moved = 0;
    for (; it < count; ++it) {
        const int arc = arcs[it];
        if (arc < 0 || arc >= s->search_arcs || s->state[arc] == MCF_STATE_TREE) { s->shift_smaller_side = false; return mcf::fail(MCF_ERR_INVALID, "pivot %lld: arc %d cannot enter", (long long)it, arc); }
        if (pivot(s, arc, &t_tree, &t_pot)) { s->status = MCF_UNBOUNDED; break; }
        moved += s->moved.n;
        s->walked_since_renumber += s->moved.n;
        if (renumber_every > 0 && (double)s->walked_since_renumber > renumber_every * (s->n + 1)) {
            const double t0 = ticks();
            renumber_nodes(s, nullptr);
            t_renum += ticks() - t0;
        }
    }
    s->shift_smaller_side = false;
    const double t0 = ticks();
    restore_node_ids(s);
    zero_root_potential(s);
    t_renum += ticks() - t0;
    const double ns_per_tick = (mcf::now_ns() - t_start) / std::max(1.0, ticks() - tick_start);
    s->metrics.iterations += it;
    s->metrics.potential_nodes += moved;
    s->metrics.tree_update_us = t_tree * ns_per_tick / 1e3;
    s->metrics.potential_update_us = t_pot * ns_per_tick / 1e3;
    s->metrics.setup_us = t_renum * ns_per_tick / 1e3;           // here: time spent renumbering
    s->metrics.loop_us = (mcf::now_ns() - t_start) / 1e3;
    s->metrics.reserved = (int32_t)s->renumbers;
    return MCF_OK;
}

int mcf_ns_check_thread_breaks(mcf_ns *s, int64_t *mismatches)
{
    if (!s || !mismatches) return mcf::fail(MCF_ERR_INVALID, "null argument");
    *mismatches = s->breaks.empty() ? 0 : mcf::breaks_mismatches(s->breaks.data(), s->nxt.data(), s->n);
    return MCF_OK;
}

int mcf_ns_finish(mcf_ns *s, int32_t *status)
{
    if (!s) return mcf::fail(MCF_ERR_INVALID, "null solver");
    if (!s->transformed) return mcf::fail(MCF_ERR_STATE, "mcf_ns_begin has not been called");
    if (s->status != MCF_UNBOUNDED) mcf::core_finish(s);
    if (status) *status = s->status;
    return MCF_OK;
}

int mcf_ns_internal(mcf_ns *s, int32_t *search_arc_num, int32_t *arc_capacity, const int32_t **source, const int32_t **target,
                    const int64_t **cost, const int8_t **state, const int64_t **pi)
{
    if (!s) return mcf::fail(MCF_ERR_INVALID, "null solver");
    if (search_arc_num) *search_arc_num = s->search_arcs;
    if (arc_capacity) *arc_capacity = (int32_t)s->tail.size();
    if (source) *source = s->tail.data();
    if (target) *target = s->head.data();
    if (cost) *cost = s->cost.data();
    if (state) *state = s->state.data();
    if (pi) *pi = s->pi.data();
    return MCF_OK;
}

int mcf_ns_tree(mcf_ns *s, const int32_t **parent, const int32_t **pred_arc, const int32_t **succ_num, const int8_t **pred_dir,
                const int64_t **flow, const int64_t **upper)
{
    if (!s) return mcf::fail(MCF_ERR_INVALID, "null solver");
    if (!s->transformed) return mcf::fail(MCF_ERR_STATE, "mcf_ns_begin has not been called");
    if (parent) *parent = s->par.data();
    if (pred_arc) *pred_arc = s->par_arc.data();
    if (succ_num) *succ_num = s->sub.data();
    if (pred_dir) *pred_dir = s->par_dir.data();
    if (flow) *flow = s->flow.data();
    if (upper) *upper = s->upper.data();
    return MCF_OK;
}

int mcf_ns_last_pivot(mcf_ns *s, int32_t *n_state, int32_t arcs[2], int8_t states[2], int32_t *n_nodes, const int32_t **nodes, int64_t *sigma)
{
    if (!s) return mcf::fail(MCF_ERR_INVALID, "null solver");
    if (n_state) *n_state = s->n_state;
    for (int i = 0; i < s->n_state; ++i) { if (arcs) arcs[i] = s->st_arc[i]; if (states) states[i] = s->st_val[i]; }
    mcf_ns::MovedList &m = s->moved;
    if (n_nodes) *n_nodes = (int32_t)m.n;
    if (nodes) {
        if (m.form == mcf_ns::MovedList::kRuns) {       // never inside a solve: the runs may be written out
            int32_t *out = m.nodes.data();
            for (int r = 0; r < m.runs_n; ++r) for (int j = 0; j < m.run_len[r]; ++j) *out++ = m.run_first[r] + j;
        }
        *nodes = m.form == mcf_ns::MovedList::kReload ? nullptr : m.nodes.data();
    }
    if (sigma) *sigma = s->sigma;
    return MCF_OK;
}

// ---- everything of Solve() (NS.cs:215-411) that precedes the pivot loop
int mcf_ns_prepare(mcf_ns *s)
{
    if (!s) return mcf::fail(MCF_ERR_INVALID, "null solver");
    if (s->list_rule && s->shard_mode != mcf_ns::kWhole)
        return mcf::fail(MCF_ERR_INVALID, "the list rules (3, 4) scan the whole search range on one engine: no sharding");
    if (s->prepared) return MCF_OK;
    if (mcf_device_count() <= s->device)
        return mcf::fail(MCF_ERR_NO_DEVICE, "HIP device %d not available (%d visible); the entering-arc search only exists on the device", s->device, mcf_device_count());
    const double t_start = mcf::now_ns();
    int rc = begin(s, nullptr);
    if (rc) return rc;
    s->prepared = true;
    if (s->status == MCF_INFEASIBLE) return MCF_OK;

    // CreatePivotRuleFinder (NS.cs:847-886): the finder is the device engine
    mcf_engine_desc d{};
    d.node_count = s->n + 1;
    d.arc_capacity = (int32_t)s->tail.size();
    d.search_arc_num = s->search_arcs;
    d.int_width = pick_int_width(s);
    // 32-bit engines check that every potential fits: the common offset of shift_potentials' smaller-side walk could break that, so they walk the subtree
    s->allow_smaller_side = d.int_width == 64;
    d.rule = s->rule;
    d.semantics = s->optimized_pivot ? MCF_SEM_OPTIMIZED : MCF_SEM_PLAIN;
    d.vector_width = s->vector_width;
    d.block_size = s->block_size;
    d.device = s->device;
    d.flags = s->engine_flags;
    if (s->list_rule) { d.rule = s->list_rule; d.semantics = MCF_SEM_PLAIN; d.vector_width = MCF_VECTOR_DEFAULT; d.flags |= MCF_ENGINE_DISPATCH; }
    // NS.cs:237-250: the solver configures itself from the problem's shape unless told otherwise.  (The reference analyses after
    // TransformToStandardForm; the analysis only reads the graph, which that step does not touch.)
    if (s->auto_config) { rc = mcf_block_config_auto(&s->config, s->n, s->m, s->tail.data(), s->head.data()); if (rc) return rc; }
    engines_destroy(s);
    const int shards = s->shard_mode == mcf_ns::kGroup ? (int)s->group_devices.size() : 1;
    for (int r = 0; r < shards; ++r) {
        mcf_engine_desc dr = d;
        if (s->shard_mode != mcf_ns::kWhole) {
            rc = mcf_shard_range(s->search_arcs, s->shard_mode == mcf_ns::kGroup ? r : s->rank, s->world, &dr.shard_begin, &dr.shard_end);
            if (rc) return rc;
        }
        // mcf_ns_set_device_share: several independent solvers of one process on one device, each with a grid of that many workgroups
        // (256 / K: every grid gets CUs of its own; an instance whose arcs no longer fit the registers of so few workgroups keeps reduced
        // costs per arc instead, section 3.8 of DESIGN.md)
        if (s->shard_mode == mcf_ns::kWhole && dr.resident_workgroups == 0) dr.resident_workgroups = s->resident_workgroups;
        if (s->shard_mode == mcf_ns::kRccl && dr.resident_workgroups == 0) {
            // the collective's kernel needs room beside the resident grid: leave one CU per XCD alone (mcf_engine_comm_init checks)
            const int cus = mcf_device_compute_units(dr.device);
            if (cus >= 64) dr.resident_workgroups = cus - 8;
        }
        if (s->shard_mode == mcf_ns::kGroup) {
            dr.device = s->group_devices[r];
            const int sharing = (int)std::count(s->group_devices.begin(), s->group_devices.end(), dr.device);
            if (sharing > 1) {                       // shards rehearsed on one GPU: every grid must fit beside the others
                dr.flags |= MCF_ENGINE_SHARE_DEVICE;
                // workgroups go to the 8 XCDs (32 CUs each) round-robin: an even share per XCD, or one XCD ends up with more 1024-thread
                // workgroups than CUs and a grid never becomes fully resident
                dr.resident_workgroups = std::max(8, 32 / sharing * 8);
                if (sharing > 3) dr.flags |= MCF_ENGINE_DISPATCH;      // more grids than the device has hardware queues for this process (engine.hip: resident slots)
            }
        }
        mcf_engine *e = nullptr;
        rc = mcf_engine_create(&e, &dr);
        if (rc) return rc;
        if (r == 0) s->engine = e; else s->peers.push_back(e);
        rc = mcf_engine_upload(e, s->tail.data(), s->head.data(), s->cost.data(), s->state.data(), s->pi.data());
        if (rc) return rc;
        if (s->shard_mode == mcf_ns::kRccl) { rc = mcf_engine_comm_init(e, s->nccl_id, s->rank, s->world); if (rc) return rc; }
        rc = mcf_engine_set_block_config(e, &s->config, s->n);
        if (rc) return rc;
        rc = mcf_engine_bind_potentials(e, s->pi.data());       // this solver's _pi is current whenever a search begins and still while it is in flight
        if (rc) return rc;
    }
    {
        // every engine of the solver has to agree to reloads (they all follow the same potentials): the largest of their thresholds, or none
        int32_t lo = 0;
        bool all = true;
        for (int r = 0; r < shards && all; ++r) {
            int32_t v = 0;
            rc = mcf_engine_reload_threshold(r == 0 ? s->engine : s->peers[r - 1], &v);
            if (rc) return rc;
            if (v <= 0) all = false;
            lo = std::max(lo, v);
        }
        s->reload_min_engines = all ? std::max<int32_t>(lo, kWalkHintMin) : 0;
    }
    {
        // node relabelling in thread order (renumber_nodes) needs every engine's consent; MCF_NS_RENUMBER=0 switches it off, =x sets the
        // interval in walked nodes per node of the graph
        const char *env = getenv("MCF_NS_RENUMBER");
        bool all = !(env && strcmp(env, "0") == 0);
        for (int r = 0; r < shards && all; ++r) {
            int32_t yes = 0;
            rc = mcf_engine_can_renumber(r == 0 ? s->engine : s->peers[r - 1], &yes);
            if (rc) return rc;
            all = yes != 0;
        }
        s->allow_renumber = all;
        s->renumber_every = 128.0;
        if (env && atof(env) > 0) { s->renumber_every = atof(env); s->renumber_forced = true; }
        // runs of consecutive ids instead of node lists: for the grid that takes them as they are (every other engine would expand them again)
        {
            mcf_engine_stats es;
            s->use_runs = mcf_engine_get_stats(s->engine, &es) == MCF_OK && es.shift_grid != 0 && s->peers.empty();
        }
    }
    s->cands.assign((size_t)std::max(1, s->world), mcf_candidate{0, 0xFFFFFFFFu, -1, 0, 0xFFFFFFFFu, -1});
    if (s->shard_mode == mcf_ns::kHost) { rc = mcf_exchange_open(&s->exchange, s->exchange_name.c_str(), s->rank, s->world); if (rc) return rc; }
    s->metrics.config_flags = s->config.flags;
    if (!s->list_rule && !s->optimized_pivot && (s->config.flags & MCF_OPT_REDUCED_COST_CACHING) && s->rule == MCF_RULE_BLOCK_SEARCH) {
        // NS.cs:855-883: `_nodeCount * _nodeCount` is an int product (it wraps) before the conversion to double
        const int32_t nn = (int32_t)((uint32_t)s->n * (uint32_t)s->n);
        const double density = (double)s->search_arcs / (double)nn;
        s->metrics.reference_selects_cached_pivot = (density < 0.01 && s->search_arcs < 10000) ? 1 : 0;
    }
    s->metrics.search_arc_num = s->search_arcs;
    s->metrics.int_width = d.int_width;
    mcf_engine_get_block_size(s->engine, &s->metrics.block_size);
    if (s->list_rule) s->metrics.block_size = 0;
    s->metrics.setup_us = (mcf::now_ns() - t_start) / 1e3;
    return MCF_OK;
}

// ---- Solve(): NS.cs:215-411
int mcf_ns_solve(mcf_ns *s, int32_t *status)
{
    if (!s) return mcf::fail(MCF_ERR_INVALID, "null solver");
    if (s->solved) return mcf::fail(MCF_ERR_STATE, "Solve() is single-shot (NS.cs:649, D11); create a new solver");
    int rc = mcf_ns_prepare(s);
    if (rc) return rc;
    s->solved = true;
    if (s->status == MCF_INFEASIBLE) { if (status) *status = s->status; return MCF_OK; }
    const double t_start = mcf::now_ns();
    const double tick_start = ticks();

    const int64_t max_iter = std::max<int64_t>(1000000, (int64_t)s->n * (int64_t)s->m);   // NS.cs:280
    int64_t it = 0;
    bool limited = false;
    double t_search = 0, t_tree = 0, t_pot = 0, t_hand = 0, t_begin = 0;      // t_hand, t_begin: the last hand-over and the posting of the search, parts of t_pot
    s->hand_over = true;
    s->engine_rc = 0;
    s->piece_ticks = 0;
    s->shift_smaller_side = s->allow_smaller_side;
    s->reload_min = s->reload_min_engines;
    s->walked_since_renumber = 0;
    s->renumber_ticks = 0;
    s->renumber_at_pivot = 0;
    s->dbg = mcf_ns::Debug{};
    s->dbg.on = getenv("MCF_NS_DEBUG") != nullptr;
    // a list rule searches synchronously at the top of the loop (the host answers from its list or the device collects); nothing is posted
    s->list_stats = mcf_list_rule_stats{};
    if (s->list_rule) list_rule_init(s);
    // The search for pivot k+1 is posted as soon as the device has what it depends on (State[] writes, potentials); the rest of pivot k
    // (flows around the cycle, re-hanging the subtree) runs while the device is searching.  Engines sharded over RCCL search in one
    // blocking call (the all-gather runs on their stream), so for them the two halves simply follow each other.
    rc = s->list_rule ? MCF_OK : engines_search_begin(s);
    while (!rc) {
        const double t0 = ticks();
        int32_t found = 0, arc = -1;
        rc = s->list_rule ? list_find_entering(s, &found, &arc) : engines_search_end(s, &found, &arc);
        const double t_got = ticks();
        t_search += t_got - t0;
        if (s->dbg.on) s->dbg.waited(t0, t_got);
        if (rc || !found) break;
        if (s->trace && it < s->trace_cap) s->trace[it] = arc;
        ++it;
        if (it > max_iter) { s->status = MCF_INFEASIBLE; break; }                          // NS.cs:311-317
        if (s->pivot_limit && it > s->pivot_limit) { --it; limited = true; break; }
        if (s->dbg.on && (it % 100000) == 0) fprintf(stderr, "[ns] %lld pivots, %.2f s\n", (long long)it, (mcf::now_ns() - t_start) / 1e9);
        // no search in flight, nothing of a pivot half done: the place to relabel
        if (relabelling_due(s, it)) { rc = relabel(s, it, t_start, tick_start); if (rc) break; }
        const double t_pot_before = t_pot;
        if (pivot_front(s, arc, &t_pot)) { s->status = MCF_UNBOUNDED; break; }
        const double t1 = ticks();
        hand_over_moved(s);                // the rest of the list, or all of it
        rc = s->engine_rc;
        const double t2 = ticks();
        if (!rc && !s->list_rule) rc = engines_search_begin(s);
        const double t3 = ticks();
        t_pot += t3 - t1;
        t_hand += t2 - t1;
        t_begin += t3 - t2;
        if (rc) break;                     // the pivot stays half done: the solver is unusable after an engine error, but nothing is left running
        pivot_back(s, &t_tree);
        s->metrics.potential_nodes += (int64_t)s->moved.n;
        s->walked_since_renumber += s->moved.n;
        if (s->dbg.on) s->dbg.pivoted(s, t_pot - t_pot_before, t_got);
    }
    // ONE way out, error or not: no hand-over pending, no resident grid left spinning, trace length and iteration count filled in
    s->hand_over = false;
    s->shift_smaller_side = false;
    if (!rc) rc = normalise_potentials(s);
    else zero_root_potential(s);     // after an engine error the engines are not told any more, but the caller's view of _pi is the reference's
    s->reload_min = 0;
    restore_node_ids(s);             // the caller's node ids again (the parked engines keep the relabelled ones: Solve() is single-shot)
    const char *first_error = rc ? mcf_last_error() : nullptr;
    std::string keep_error = first_error ? first_error : "";
    engines_each(s, [](mcf_engine *e) { mcf_engine_park(e); return MCF_OK; });     // a resident scan grid must not outlive Solve()
    s->trace_len = std::min(it, s->trace_cap);
    s->metrics.iterations = it;
    if (!rc && s->status == MCF_NOT_SOLVED && !limited) mcf::core_finish(s);
    // the phase buckets were counted in time-stamp-counter ticks (a clock call per phase costs 20+ ns, seven of them per pivot): scale them
    const double ns_per_tick = (mcf::now_ns() - t_start) / std::max(1.0, ticks() - tick_start);
    s->metrics.pivot_search_us = t_search * ns_per_tick / 1e3;
    s->metrics.tree_update_us = t_tree * ns_per_tick / 1e3;
    s->metrics.potential_update_us = t_pot * ns_per_tick / 1e3;
    if (s->dbg.on && it > 1000) s->dbg.report(s, it, {t_search, t_tree, t_pot, t_hand, t_begin, s->piece_ticks}, ns_per_tick, tick_start);
    mcf_engine_get_stats(s->engine, &s->metrics.engine);
    // the rest of SolverMetrics: NS.cs:262-270 (initial block size), :276 (expected iterations), :344-357
    const bool plain_block = !s->list_rule && s->rule == MCF_RULE_BLOCK_SEARCH && !s->optimized_pivot;
    s->list_stats.collect_us = s->lr.collect_ticks * ns_per_tick / 1e3;
    s->metrics.initial_block_size = plain_block ? s->metrics.engine.initial_block_size : 0;
    s->metrics.final_block_size = plain_block ? s->metrics.engine.current_block_size : 0;
    s->metrics.total_arcs_checked = s->metrics.engine.arcs_checked;
    s->metrics.average_arcs_checked_per_pivot = it > 0 ? (double)s->metrics.total_arcs_checked / (double)it : 0;
    {
        const double expected = std::sqrt((double)s->search_arcs) * s->n * 0.5;
        s->metrics.baseline_iterations = expected < 2147483648.0 ? (int32_t)expected : INT32_MIN;     // what (int) of an oversized double gives on x64
    }
    s->metrics.iteration_ratio = s->metrics.baseline_iterations > 0 ? (double)it / s->metrics.baseline_iterations : 1.0;
    s->metrics.loop_us = (mcf::now_ns() - t_start) / 1e3;
    s->metrics.total_solve_us = s->metrics.loop_us + s->metrics.setup_us;
    if (status) *status = s->status;
    if (rc) { mcf::set_error("%s", keep_error.c_str()); return rc; }
    return MCF_OK;
}

int mcf_ns_status(mcf_ns *s, int32_t *status) { if (!s || !status) return mcf::fail(MCF_ERR_INVALID, "null argument"); *status = s->status; return MCF_OK; }

static int need_optimal(const mcf_ns *s)
{
    if (s->status != MCF_OPTIMAL) return mcf::fail(MCF_ERR_STATE, "Solution not optimal");   // NS.cs:418-421
    return MCF_OK;
}
int mcf_ns_get_flow(mcf_ns *s, int32_t arc, int64_t *flow)
{
    if (!s || !flow) return mcf::fail(MCF_ERR_INVALID, "null argument");
    if (int rc = need_optimal(s)) return rc;
    if (arc < 0 || arc >= s->m) return mcf::fail(MCF_ERR_INVALID, "Invalid arc");
    *flow = s->flow[arc];
    return MCF_OK;
}
int mcf_ns_get_potential(mcf_ns *s, int32_t node, int64_t *potential)
{
    if (!s || !potential) return mcf::fail(MCF_ERR_INVALID, "null argument");
    if (int rc = need_optimal(s)) return rc;
    if (node < 0 || node >= s->n) return mcf::fail(MCF_ERR_INVALID, "Invalid node");
    *potential = s->pi[node];
    return MCF_OK;
}
int mcf_ns_get_total_cost(mcf_ns *s, int64_t *cost)
{
    if (!s || !cost) return mcf::fail(MCF_ERR_INVALID, "null argument");
    if (int rc = need_optimal(s)) return rc;
    *cost = mcf::core_total_cost(s);
    return MCF_OK;
}
int mcf_ns_get_flows(mcf_ns *s, int64_t *out)
{
    if (!s || !out) return mcf::fail(MCF_ERR_INVALID, "null argument");
    if (int rc = need_optimal(s)) return rc;
    std::copy(s->flow.begin(), s->flow.begin() + s->m, out);
    return MCF_OK;
}
int mcf_ns_get_potentials(mcf_ns *s, int64_t *out)
{
    if (!s || !out) return mcf::fail(MCF_ERR_INVALID, "null argument");
    if (int rc = need_optimal(s)) return rc;
    std::copy(s->pi.begin(), s->pi.begin() + s->n, out);
    return MCF_OK;
}
int mcf_ns_get_arc_upper_bound(mcf_ns *s, int32_t arc, int64_t *upper)
{
    if (!s || !upper) return mcf::fail(MCF_ERR_INVALID, "null argument");
    if (arc < 0 || arc >= s->m) return mcf::fail(MCF_ERR_INVALID, "Invalid arc");
    *upper = s->upper[arc];
    return MCF_OK;
}
// SolutionValidator(graph, solver).Validate() (SolutionValidator.cs:20-52) with the checks run on the device
int mcf_ns_validate(mcf_ns *s, mcf_validation *out)
{
    if (!s || !out) return mcf::fail(MCF_ERR_INVALID, "null argument");
    memset(out, 0, sizeof(*out));
    for (int k = 0; k < MCF_VAL_KINDS; ++k) out->first[k] = -1;
    out->supply_type = s->supply_type;
    if (s->status != MCF_OPTIMAL) {                      // :28-33: nothing else is looked at
        out->errors[MCF_VAL_STATUS] = 1;
        out->first[MCF_VAL_STATUS] = 0;
        return MCF_OK;
    }
    mcf_validator *v = nullptr;
    int rc = mcf_validator_create(&v, s->device, s->n, s->m);
    if (rc) return rc;
    int64_t total = 0;                                   // GetTotalCost(), NS.cs:452-465
    for (int e = 0; e < s->m; ++e) total = (int64_t)((uint64_t)total + (uint64_t)s->flow[e] * (uint64_t)s->cost[e]);
    rc = mcf_validator_upload(v, s->tail.data(), s->head.data(), s->orig_lower.data(), s->upper.data(), s->cost.data(), s->supply.data(),
                              s->flow.data(), s->pi.data());
    if (!rc) rc = mcf_validator_run(v, s->supply_type, total, out);
    mcf_validator_destroy(v);
    return rc;
}
int mcf_ns_check_reduced_costs(mcf_ns *s, int64_t *mismatches)
{
    if (!s || !mismatches) return mcf::fail(MCF_ERR_INVALID, "null argument");
    *mismatches = 0;
    return engines_each(s, [&](mcf_engine *e) {
        int64_t m = 0;
        const int rc = mcf_engine_check_reduced_costs(e, &m, nullptr);
        *mismatches += m;
        return rc;
    });
}
int mcf_ns_get_metrics(mcf_ns *s, mcf_ns_metrics *out)
{
    if (!s || !out) return mcf::fail(MCF_ERR_INVALID, "null argument");
    *out = s->metrics;
    return MCF_OK;
}
int mcf_ns_get_list_rule_stats(mcf_ns *s, mcf_list_rule_stats *out)
{
    if (!s || !out) return mcf::fail(MCF_ERR_INVALID, "null argument");
    *out = s->list_stats;
    return MCF_OK;
}

}  // extern "C"
