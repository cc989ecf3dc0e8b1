// rbatch_host_check.cpp -- the host side of the ragged batch (mcf_rbatch_create, _run_on_host, _rerun_on_host, _validate_on_host) as a
// stand-alone program, so that it can be built together with the library's host sources under -fsanitize=address,undefined and run on a
// CPU ("Ragged batch").  Needs no GPU and is not loaded into Python.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -I../include \
//         rbatch_host_check.cpp ../mincostflow_amd/csrc/{batch.hip,ns_core.cpp,ns_host.cpp,engine.hip,validate.hip,problems.cpp,util.cpp,exchange.cpp} \
//         -fsanitize=address,undefined -ldl -lrt -lhsa-runtime64 -o rbatch_host_check
//   ./rbatch_host_check instances.txt
//
// Input, whitespace-separated integers: G count; per graph: n m, m sources, m targets; count entries of graph_of; then per instance, in
// order: m lower, m upper, m cost, n supply, m second cost (for the re-solve).  Upper bounds may be MCF_INF_CAP.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mcf_hip.h"

static long long next(FILE *f)
{
    long long v = 0;
    if (fscanf(f, "%lld", &v) != 1) { fprintf(stderr, "short input\n"); exit(2); }
    return v;
}
#define CHECK(call)                                                                    \
    do {                                                                               \
        const int rc__ = (call);                                                       \
        if (rc__ != MCF_OK) { fprintf(stderr, "%s: %d %s\n", #call, rc__, mcf_last_error()); return 1; } \
    } while (0)

int main(int argc, char **argv)
{
    FILE *f = argc > 1 ? fopen(argv[1], "r") : nullptr;
    if (!f) { fprintf(stderr, "usage: %s instances.txt\n", argv[0]); return 2; }
    const int32_t G = (int32_t)next(f), count = (int32_t)next(f);
    std::vector<int32_t> node_count, source, target, graph_of;
    std::vector<int64_t> arc_start{0};
    for (int g = 0; g < G; ++g) {
        node_count.push_back((int32_t)next(f));
        const int64_t m = next(f);
        arc_start.push_back(arc_start.back() + m);
        for (int64_t e = 0; e < m; ++e) source.push_back((int32_t)next(f));
        for (int64_t e = 0; e < m; ++e) target.push_back((int32_t)next(f));
    }
    for (int i = 0; i < count; ++i) graph_of.push_back((int32_t)next(f));
    std::vector<int64_t> lower, upper, cost, supply, cost2;
    for (int i = 0; i < count; ++i) {
        const int g = graph_of[(size_t)i];
        const int64_t m = arc_start[(size_t)g + 1] - arc_start[(size_t)g], n = node_count[(size_t)g];
        for (int64_t e = 0; e < m; ++e) lower.push_back(next(f));
        for (int64_t e = 0; e < m; ++e) upper.push_back(next(f));
        for (int64_t e = 0; e < m; ++e) cost.push_back(next(f));
        for (int64_t v = 0; v < n; ++v) supply.push_back(next(f));
        for (int64_t e = 0; e < m; ++e) cost2.push_back(next(f));
    }
    fclose(f);

    int64_t pivots_total = 0, invalid_total = 0;
    for (int32_t rule : {MCF_RULE_BLOCK_SEARCH, MCF_RULE_BEST_ELIGIBLE, MCF_RULE_FIRST_ELIGIBLE})
        for (int32_t stype : {MCF_SUPPLY_GEQ, MCF_SUPPLY_LEQ}) {
            mcf_rbatch_desc d{};
            d.pivot_rule = rule; d.semantics = MCF_SEM_PLAIN; d.trace_capacity = 64;
            d.graph_count = G; d.count = count;
            d.node_count = node_count.data(); d.arc_start = arc_start.data(); d.source = source.data(); d.target = target.data(); d.graph_of = graph_of.data();
            mcf_rbatch *b = nullptr;
            CHECK(mcf_rbatch_create(&b, &d));
            std::vector<int64_t> arc_row((size_t)count + 1), node_row((size_t)count + 1);
            CHECK(mcf_rbatch_get_rows(b, arc_row.data(), node_row.data()));
            if (arc_row.back() != (int64_t)lower.size() || node_row.back() != (int64_t)supply.size()) { fprintf(stderr, "rows do not match the input\n"); return 1; }
            // exactly sized outputs: a write past a row's end is a write past the allocation for the last instance, and the sanitizer's to find
            std::vector<int32_t> status((size_t)count), trace((size_t)count * 64);
            std::vector<int64_t> pivots((size_t)count), total((size_t)count), flows(lower.size()), potentials(supply.size());
            mcf_rbatch_io io{};
            io.memory = MCF_MEM_HOST; io.supply_type = stype;
            io.lower = lower.data(); io.upper = upper.data(); io.cost = cost.data(); io.supply = supply.data();
            io.status = status.data(); io.pivots = pivots.data(); io.total_cost = total.data(); io.flows = flows.data(); io.potentials = potentials.data(); io.trace = trace.data();
            CHECK(mcf_rbatch_run_on_host(b, &io));
            std::vector<int32_t> valid((size_t)count), errors((size_t)count * MCF_VAL_KINDS), first((size_t)count * MCF_VAL_KINDS);
            std::vector<int64_t> objective((size_t)count), dual((size_t)count);
            mcf_rbatch_check_io c{};
            c.memory = MCF_MEM_HOST; c.supply_type = stype;
            c.lower = lower.data(); c.upper = upper.data(); c.cost = cost.data(); c.supply = supply.data();
            c.status = status.data(); c.total_cost = total.data(); c.flows = flows.data(); c.potentials = potentials.data();
            c.valid = valid.data(); c.errors = errors.data(); c.first = first.data(); c.objective = objective.data(); c.dual_cost = dual.data();
            mcf_ubatch_check_summary summary{};
            CHECK(mcf_rbatch_validate_on_host(b, &c, &summary));
            invalid_total += summary.invalid;
            std::vector<uint8_t> changed((size_t)count);
            for (int i = 0; i < count; ++i) changed[(size_t)i] = i % 3 != 1;
            io.cost = cost2.data(); io.changed = changed.data();
            CHECK(mcf_rbatch_rerun_on_host(b, &io));
            io.changed = nullptr;
            CHECK(mcf_rbatch_rerun_on_host(b, &io));
            c.cost = cost2.data();
            CHECK(mcf_rbatch_validate_on_host(b, &c, &summary));
            mcf_ubatch_stats st{};
            CHECK(mcf_rbatch_get_stats(b, &st));
            pivots_total += st.total_pivots;
            mcf_rbatch_destroy(b);
        }
    printf("ok: %d instances of %d graphs, 3 rules x 2 supply types; %lld pivots in the last re-solves, %lld rows flagged by the first validations\n", count, G,
           (long long)pivots_total, (long long)invalid_total);
    return 0;
}
