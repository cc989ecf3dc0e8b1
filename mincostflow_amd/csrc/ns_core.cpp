// ns_core.cpp -- set-up and end of a solve on an NsCore (ns_core.h): nothing here drives a device.
#include <algorithm>

#include "ns_core.h"

namespace mcf {

namespace {

// ---- NS.cs:624-669
bool bounds_ok(const NsCore *s)
{
    for (int e = 0; e < s->m; ++e)
        if (s->upper[e] < s->lower[e]) return false;
    return true;
}

int64_t art_cost_of(const NsCore *s)
{
    int64_t biggest = 0;
    for (int e = 0; e < s->m; ++e) biggest = std::max<int64_t>(biggest, s->cost[e] < 0 ? -s->cost[e] : s->cost[e]);
    return (biggest + 1) * (int64_t)s->n;
}

void to_standard_form(NsCore *s)
{
    for (int e = 0; e < s->m; ++e) {
        const int64_t lo = s->lower[e];
        if (lo == 0) continue;
        s->supply[s->tail[e]] -= lo;
        s->supply[s->head[e]] += lo;
        s->upper[e] -= lo;
        s->lower[e] = 0;
    }
    s->sum_supply = 0;
    for (int v = 0; v < s->n; ++v) s->sum_supply += s->supply[v];
    s->art_cost = art_cost_of(s);
    s->transformed = true;
}

// ---- NS.cs:671-845: star basis on the artificial root.  GEQ: nodes with supply <= 0 hang on a zero-cost
// root->v arc, the others on an ART_COST v->root arc and get a zero-cost root->v arc at its lower bound; LEQ mirrored.
void start_basis(NsCore *s)
{
    const int n = s->n, m = s->m, root = s->root = n;
    s->par[root] = -1; s->par_arc[root] = -1; s->nxt[root] = 0; s->prv[0] = root;
    s->sub[root] = n + 1; s->fin[root] = n - 1; s->par_dir[root] = 0; s->pi[root] = 0;
    for (int e = 0; e < m; ++e) { s->state[e] = MCF_STATE_LOWER; s->flow[e] = 0; }
    s->search_arcs = m + n;
    int extra = m + n;
    for (int v = 0; v < n; ++v) { s->nxt[v] = v + 1 < n ? v + 1 : root; }
    for (int v = 0; v < n; ++v) s->prv[s->nxt[v]] = v;
    const bool geq = s->supply_type == MCF_SUPPLY_GEQ;
    for (int v = 0; v < n; ++v) {
        const int link = m + v;
        s->par[v] = root; s->sub[v] = 1; s->fin[v] = v;
        const bool plain = geq ? s->supply[v] <= 0 : s->supply[v] >= 0;
        // direction of the zero-cost link: GEQ root->v, LEQ v->root
        const int lt = geq ? root : v, lh = geq ? v : root;
        s->tail[link] = lt; s->head[link] = lh; s->upper[link] = kInf; s->cost[link] = 0;
        if (plain) {
            s->par_dir[v] = geq ? kDown : kUp;
            s->pi[v] = 0;
            s->par_arc[v] = link;
            s->flow[link] = geq ? -s->supply[v] : s->supply[v];
            s->state[link] = MCF_STATE_TREE;
        } else {
            s->par_dir[v] = geq ? kUp : kDown;
            s->pi[v] = geq ? -s->art_cost : s->art_cost;
            s->par_arc[v] = extra;
            s->tail[extra] = lh; s->head[extra] = lt;   // the opposite direction
            s->upper[extra] = kInf;
            s->flow[extra] = geq ? s->supply[v] : -s->supply[v];
            s->cost[extra] = s->art_cost;
            s->state[extra] = MCF_STATE_TREE;
            s->flow[link] = 0;
            s->state[link] = MCF_STATE_LOWER;
            ++extra;
        }
    }
    if (n > 0) s->prv[root] = n - 1;
    s->all_arcs = extra;
}

}  // namespace

bool core_begin(NsCore *s)
{
    s->status = MCF_NOT_SOLVED;
    s->bounds_restored = false;
    if (!bounds_ok(s)) { s->status = MCF_INFEASIBLE; return false; }   // NS.cs:227-231
    to_standard_form(s);
    start_basis(s);
    return true;
}

void core_finish(NsCore *s)
{
    // NS.cs:1272-1283 with _allArcNum overwritten by _searchArcNum at NS.cs:689 (difference D9): only the n root links
    for (int e = s->m; e < s->search_arcs; ++e)
        if (s->flow[e] != 0) { s->status = MCF_INFEASIBLE; return; }
    s->status = MCF_OPTIMAL;
    for (int e = 0; e < s->m; ++e) {                      // NS.cs:364-388
        const int64_t lo = s->orig_lower[e];
        if (lo == 0) continue;
        s->flow[e] += lo;
        s->supply[s->tail[e]] += lo;
        s->supply[s->head[e]] -= lo;
    }
    s->bounds_restored = true;
}

void core_reopen(NsCore *s)
{
    s->status = MCF_NOT_SOLVED;
    if (!s->bounds_restored) return;
    for (int e = 0; e < s->m; ++e) {
        const int64_t lo = s->orig_lower[e];
        if (lo == 0) continue;
        s->flow[e] -= lo;
        s->supply[s->tail[e]] -= lo;
        s->supply[s->head[e]] += lo;
    }
    s->bounds_restored = false;
}

void core_recost(NsCore *s, const int64_t *cost)
{
    std::copy(cost, cost + s->m, s->cost.begin());
    s->art_cost = art_cost_of(s);
    for (int e = s->m + s->n; e < s->all_arcs; ++e) s->cost[e] = s->art_cost;
}

int64_t core_total_cost(const NsCore *s)
{
    int64_t total = 0;
    // NS.cs:459-464; C#'s unchecked long wraps, and a flow at an infinite bound makes it (unsigned here: the same bits, defined)
    for (int e = 0; e < s->m; ++e) total = (int64_t)((uint64_t)total + (uint64_t)s->flow[e] * (uint64_t)s->cost[e]);
    return total;
}

int core_create(NsCore *s, int32_t node_count, int32_t arc_count, const int32_t *source, const int32_t *target)
{
    if (node_count < 0 || arc_count < 0 || (arc_count && (!source || !target))) return fail(MCF_ERR_INVALID, "graph must not be null (NS.cs:121)");
    if ((int64_t)arc_count + 2 * (int64_t)node_count > INT32_MAX - 4096) return fail(MCF_ERR_INVALID, "graph too large for 32-bit arc ids");
    for (int e = 0; e < arc_count; ++e)
        if ((unsigned)source[e] >= (unsigned)node_count || (unsigned)target[e] >= (unsigned)node_count)
            return fail(MCF_ERR_INVALID, "arc %d: end point out of range", e);
    s->n = node_count; s->m = arc_count;
    const size_t A = (size_t)arc_count + 2 * (size_t)node_count, N = (size_t)node_count + 1;
    s->tail.assign(A, 0); s->head.assign(A, 0);
    std::copy(source, source + arc_count, s->tail.begin());
    std::copy(target, target + arc_count, s->head.begin());
    s->lower.assign(A, 0); s->upper.assign(A, kInf); s->cost.assign(A, 0); s->flow.assign(A, 0);   // NS.cs:614-617
    s->orig_lower.assign(arc_count, 0);
    s->state.assign(A, 0);
    s->supply.assign(N, 0); s->pi.assign(N, 0);
    s->par.assign(N, -1); s->par_arc.assign(N, -1); s->nxt.assign(N, 0); s->prv.assign(N, 0);
    s->sub.assign(N, 0); s->fin.assign(N, 0); s->par_dir.assign(N, 0); s->scratch.assign(N + 1, 0);
    return MCF_OK;
}

void core_set_problem(NsCore *s, const int64_t *lower, const int64_t *upper, const int64_t *cost, const int64_t *supply)
{
    for (int e = 0; e < s->m; ++e) {
        if (lower) { s->lower[e] = lower[e]; s->orig_lower[e] = lower[e]; }
        if (upper) s->upper[e] = upper[e] == MCF_INF_CAP ? kInf : upper[e];
        if (cost) s->cost[e] = cost[e];
    }
    if (supply) std::copy(supply, supply + s->n, s->supply.begin());
}

}  // namespace mcf
