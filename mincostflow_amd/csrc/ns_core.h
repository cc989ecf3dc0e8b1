// ns_core.h -- the arrays of one network-simplex solve and the host steps around the pivot loop.
//
// NsCore is what mcf_ns keeps of a problem and its spanning tree (NS.cs:126-151), without anything that drives a device.  mcf_ns derives
// from it; the batch solver (batch.hip) keeps one per instance.  The functions are the set-up and the end of Solve() (NS.cs:215-393),
// defined once in ns_core.cpp and used by both.  The pivot between them is tree_pivot.h, on the view that tree() gives.
#pragma once

#include "common.h"
#include "tree_pivot.h"

namespace mcf {

struct NsCore {
    int n = 0, m = 0, root = 0;
    int search_arcs = 0, all_arcs = 0;
    int supply_type = MCF_SUPPLY_GEQ;                                  // NS.cs:38
    // arcs: m + 2n entries (NS.cs:130)
    hvec<int32_t> tail, head;
    hvec<int64_t> lower, upper, cost, flow, orig_lower;
    hvec<int8_t> state;
    // nodes: n + 1 entries, the last one is the artificial root (NS.cs:137,144)
    hvec<int64_t> supply, pi;
    hvec<int32_t> par, par_arc, nxt, prv, sub, fin;   // Parent, Pred, Thread, RevThread, SuccNum, LastSucc
    hvec<int8_t> par_dir;
    std::vector<int32_t> scratch;                     // n + 2 entries: the re-hanging's list of nodes whose RevThread is repaired last
    int64_t sum_supply = 0, art_cost = 0;
    int status = MCF_NOT_SOLVED;
    bool transformed = false;
    bool bounds_restored = false;                     // core_finish has added the lower bounds to flow[] and supply[]; core_reopen takes them out again

    // the arrays a pivot touches; valid as long as the vectors are not resized (core_create sizes them, nothing does after it)
    TreeView tree()
    {
        return TreeView{tail.data(), head.data(), upper.data(), flow.data(), par.data(), par_arc.data(), nxt.data(), prv.data(),
                        sub.data(), fin.data(), par_dir.data(), scratch.data()};
    }
};

// the checks and allocations of mcf_ns_create (NS.cs:113-151, :605-617); source / target are validated here, before anything can reach a device
int core_create(NsCore *s, int32_t node_count, int32_t arc_count, const int32_t *source, const int32_t *target);
// mcf_ns_set_problem: any of the four may be null (left as it is)
void core_set_problem(NsCore *s, const int64_t *lower, const int64_t *upper, const int64_t *cost, const int64_t *supply);
// NS.cs:227-250: false (status Infeasible) when a bound pair is inverted, else standard form and the artificial-root start basis
bool core_begin(NsCore *s);
// NS.cs:359-393 after the loop found no entering arc: feasibility over the root links, lower bounds restored
void core_finish(NsCore *s);
// The inverse of core_finish's last step, for a solve that goes on from the basis an earlier one left (the batch solver's warm re-solve):
// flow[e] -= orig_lower[e] and the supplies moved back, so that flows and supplies are in standard form again; status Not Solved.
// Does nothing unless core_finish restored the bounds since the last core_begin / core_reopen, so a chain of re-solves cannot drift.
void core_reopen(NsCore *s);
// New arc costs for a core that has been through core_begin: cost[0, m), art_cost as to_standard_form derives it and, with it, the
// artificial arcs [m + n, all_arcs); the root links [m, m + n) keep cost 0.  Tree, flows and State[] are not touched.
void core_recost(NsCore *s, const int64_t *cost);
// NS.cs:459-464
int64_t core_total_cost(const NsCore *s);

}  // namespace mcf
