// rbatch_host_check.cpp -- the host side of the placed batches as a stand-alone program, so that it can be built together with the
// library's host sources under -fsanitize=address,undefined and run on a CPU ("Ragged batch").  It runs the ragged entry
// points (mcf_rbatch_create, _run_on_host, _rerun_on_host, _validate_on_host) on its input, exports the first solve's basis with its
// cost ranges (_cost_ranges_on_host), asks the same basis' supply and bound ranges (_data_ranges_on_host, pairs included), diagnoses the
// same state (_diagnose_on_host, verdict counts printed), asks whether it is unbounded (_rays_on_host with and without the rows, every
// cycle summed and every row of labels checked, verdict counts printed) and starts a second handle from it (_run_from_on_host: the same data must give
// the first solve's status and total cost; the second costs run for the sanitizer's sake), then the instances of the input's first graph
// through the uniform entry points (mcf_ubatch_*), which share the drivers -- the solves, the validations and all three queries of the
// kept state (cost ranges, data ranges with graph 0's pair list, diagnosis, rays) -- and compares every row of the two.  Needs no GPU and is
// not loaded into Python.
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

constexpr int kTrace = 64;

// the rows of the instances `sel`, each `length` long and beginning at row[i] * scale in `flat`, one after the other
template <class T>
static std::vector<T> dense(const std::vector<T> &flat, const std::vector<int64_t> &row, int64_t scale, int64_t length, const std::vector<int> &sel)
{
    std::vector<T> out;
    for (int i : sel) out.insert(out.end(), flat.begin() + row[(size_t)i] * scale, flat.begin() + row[(size_t)i] * scale + length);
    return out;
}

// what a diagnose call wrote, exactly sized
struct Diagnosis {
    std::vector<int32_t> verdict, set_size;
    std::vector<int64_t> violation, unmet;
    std::vector<int8_t> side;
    Diagnosis(size_t count, size_t nodes) : verdict(count), set_size(count), violation(count), unmet(nodes), side(nodes) {}
};

// what a rays call wrote, exactly sized
struct Rays {
    std::vector<int32_t> verdict, cycle_length;
    std::vector<int64_t> cycle_cost, label;
    std::vector<int8_t> on_cycle;
    Rays(size_t count, size_t arcs, size_t nodes) : verdict(count), cycle_length(count), cycle_cost(count), label(nodes), on_cycle(arcs) {}
};

// what a solve call and a validation call wrote
struct Answers {
    std::vector<int32_t> status, trace, valid, errors, first;
    std::vector<int64_t> pivots, total, flows, potentials, objective, dual;
    Answers(size_t count, size_t arcs, size_t nodes)
        : status(count), trace(count * kTrace), valid(count), errors(count * MCF_VAL_KINDS), first(count * MCF_VAL_KINDS), pivots(count), total(count), flows(arcs),
          potentials(nodes), objective(count), dual(count) {}
};
// u: the uniform batch's answers for the instances `sel`; r: the ragged batch's for all
static bool same(const char *when, const Answers &u, const Answers &r, const std::vector<int64_t> &one, const std::vector<int64_t> &arc_row,
                 const std::vector<int64_t> &node_row, int64_t n, int64_t m, const std::vector<int> &sel)
{
    const bool ok = u.status == dense(r.status, one, 1, 1, sel) && u.pivots == dense(r.pivots, one, 1, 1, sel) && u.total == dense(r.total, one, 1, 1, sel) &&
                    u.flows == dense(r.flows, arc_row, 1, m, sel) && u.potentials == dense(r.potentials, node_row, 1, n, sel) &&
                    u.trace == dense(r.trace, one, kTrace, kTrace, sel) && u.valid == dense(r.valid, one, 1, 1, sel) &&
                    u.errors == dense(r.errors, one, MCF_VAL_KINDS, MCF_VAL_KINDS, sel) && u.first == dense(r.first, one, MCF_VAL_KINDS, MCF_VAL_KINDS, sel) &&
                    u.objective == dense(r.objective, one, 1, 1, sel) && u.dual == dense(r.dual, one, 1, 1, sel);
    if (!ok) fprintf(stderr, "%s: the uniform batch's answers differ from the ragged batch's\n", when);
    return ok;
}

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
    // the uniform pass: the instances of graph 0
    std::vector<int> sel;
    std::vector<int64_t> one;
    for (int i = 0; i < count; ++i) {
        one.push_back(i);
        if (graph_of[(size_t)i] == 0) sel.push_back(i);
    }
    const int64_t n0 = G ? node_count[0] : 0, m0 = G ? arc_start[1] : 0;
    std::vector<uint8_t> changed((size_t)count);
    for (int i = 0; i < count; ++i) changed[(size_t)i] = i % 3 != 1;

    int64_t pivots_total = 0, invalid_total = 0, started = 0, data_ranged_total = 0, data_walks = 0;
    int64_t verdicts[MCF_DIAG_BOUNDS + 1] = {}, uniform_verdicts[MCF_DIAG_BOUNDS + 1] = {}, diag_levels = 0;
    int64_t ray_verdicts[MCF_RAY_BOUNDS + 1] = {}, uniform_ray_verdicts[MCF_RAY_BOUNDS + 1] = {}, ray_rounds = 0;
    for (int32_t rule : {MCF_RULE_BLOCK_SEARCH, MCF_RULE_BEST_ELIGIBLE, MCF_RULE_FIRST_ELIGIBLE})
        for (int32_t stype : {MCF_SUPPLY_GEQ, MCF_SUPPLY_LEQ}) {
            mcf_rbatch_desc d{};
            d.pivot_rule = rule; d.semantics = MCF_SEM_PLAIN; d.trace_capacity = kTrace;
            d.graph_count = G; d.count = count;
            d.node_count = node_count.data(); d.arc_start = arc_start.data(); d.source = source.data(); d.target = target.data(); d.graph_of = graph_of.data();
            mcf_rbatch *b = nullptr;
            CHECK(mcf_rbatch_create(&b, &d));
            std::vector<int64_t> arc_row((size_t)count + 1), node_row((size_t)count + 1);
            CHECK(mcf_rbatch_get_rows(b, arc_row.data(), node_row.data()));
            if (arc_row.back() != (int64_t)lower.size() || node_row.back() != (int64_t)supply.size()) { fprintf(stderr, "rows do not match the input\n"); return 1; }
            // exactly sized outputs: a write past a row's end is a write past the allocation for the last instance, and the sanitizer's to find
            Answers r((size_t)count, lower.size(), supply.size());
            mcf_rbatch_io io{};
            io.memory = MCF_MEM_HOST; io.supply_type = stype;
            io.lower = lower.data(); io.upper = upper.data(); io.cost = cost.data(); io.supply = supply.data();
            io.status = r.status.data(); io.pivots = r.pivots.data(); io.total_cost = r.total.data(); io.flows = r.flows.data(); io.potentials = r.potentials.data(); io.trace = r.trace.data();
            CHECK(mcf_rbatch_run_on_host(b, &io));
            mcf_rbatch_check_io c{};
            c.memory = MCF_MEM_HOST; c.supply_type = stype;
            c.lower = lower.data(); c.upper = upper.data(); c.cost = cost.data(); c.supply = supply.data();
            c.status = r.status.data(); c.total_cost = r.total.data(); c.flows = r.flows.data(); c.potentials = r.potentials.data();
            c.valid = r.valid.data(); c.errors = r.errors.data(); c.first = r.first.data(); c.objective = r.objective.data(); c.dual_cost = r.dual.data();
            mcf_ubatch_check_summary summary{};
            CHECK(mcf_rbatch_validate_on_host(b, &c, &summary));
            invalid_total += summary.invalid;
            const Answers r_first = r;
            // the basis as far as the caller's arcs go and its cost ranges, exactly sized like the outputs
            std::vector<int8_t> arc_state(lower.size());
            std::vector<int32_t> ranged((size_t)count);
            std::vector<int64_t> cost_down(lower.size()), cost_up(lower.size());
            mcf_rbatch_range_io rio{};
            rio.memory = MCF_MEM_HOST; rio.ranged = ranged.data(); rio.arc_state = arc_state.data(); rio.cost_down = cost_down.data(); rio.cost_up = cost_up.data();
            CHECK(mcf_rbatch_cost_ranges_on_host(b, &rio));
            // the supply and bound ranges of the same basis: per graph the two ends of every third arc, its first and last node both
            // ways round, a pair (0, 0) and one with an id out of range; pairs, tables and every output exactly sized
            std::vector<int32_t> pairs;
            std::vector<int64_t> pair_row{0}, ship_row{0}, flow_down(lower.size()), flow_up(lower.size()), ship_forth, ship_back;
            {
                for (int g = 0; g < G; ++g) {
                    const int32_t n = node_count[(size_t)g];
                    for (int64_t e = arc_start[(size_t)g]; e < arc_start[(size_t)g + 1]; e += 3) { pairs.push_back(source[(size_t)e]); pairs.push_back(target[(size_t)e]); }
                    for (int32_t v : {0, n - 1, n - 1, 0, 0, 0, n, 0}) pairs.push_back(v);
                    pair_row.push_back((int64_t)pairs.size() / 2);
                }
                for (int i = 0; i < count; ++i) {
                    const size_t g = (size_t)graph_of[(size_t)i];
                    ship_row.push_back(ship_row.back() + pair_row[g + 1] - pair_row[g]);
                }
                std::vector<int8_t> data_state(lower.size());
                std::vector<int32_t> data_ranged((size_t)count);
                ship_forth.resize((size_t)ship_row.back()); ship_back.resize((size_t)ship_row.back());
                mcf_rbatch_data_range_io dio{};
                dio.memory = MCF_MEM_HOST; dio.pairs = pairs.data(); dio.pair_row = pair_row.data(); dio.ship_row = ship_row.data();
                dio.ranged = data_ranged.data(); dio.arc_state = data_state.data(); dio.flow_down = flow_down.data(); dio.flow_up = flow_up.data();
                dio.ship_forth = ship_forth.data(); dio.ship_back = ship_back.data();
                CHECK(mcf_rbatch_data_ranges_on_host(b, &dio));
                if (data_state != arc_state || data_ranged != ranged) { fprintf(stderr, "the data ranges name another basis than the cost ranges\n"); return 1; }
                for (int i = 0; i < count; ++i) {
                    if (!ranged[(size_t)i]) continue;
                    const size_t g = (size_t)graph_of[(size_t)i];
                    int64_t k = ship_row[(size_t)i];
                    for (int64_t e = 0; e < arc_start[g + 1] - arc_start[g]; e += 3, ++k) {
                        const size_t at = (size_t)(arc_row[(size_t)i] + e);
                        if (arc_state[at] != MCF_STATE_TREE && (ship_forth[(size_t)k] != flow_down[at] || ship_back[(size_t)k] != flow_up[at])) {
                            fprintf(stderr, "instance %d, arc %lld: the pair of its ends ships another amount than the arc's flow may move\n", i, (long long)e);
                            return 1;
                        }
                    }
                    if (ship_forth[(size_t)k + 2] != MCF_RANGE_INF || ship_back[(size_t)k + 2] != MCF_RANGE_INF || ship_forth[(size_t)k + 3] != -1 || ship_back[(size_t)k + 3] != -1 ||
                        ship_forth[(size_t)k] != ship_back[(size_t)k + 1] || ship_back[(size_t)k] != ship_forth[(size_t)k + 1]) {
                        fprintf(stderr, "instance %d: the special pairs' answers\n", i);
                        return 1;
                    }
                    ++data_ranged_total;
                }
                mcf_ubatch_data_range_stats ds{};
                CHECK(mcf_rbatch_get_data_range_stats(b, &ds));
                data_walks += ds.walks;
            }
            // why infeasible, from the same kept state: every output exactly sized; a cut's violation is the |unmet| of its side
            Diagnosis dg((size_t)count, supply.size());
            {
                mcf_rbatch_diagnose_io gio{};
                gio.memory = MCF_MEM_HOST; gio.verdict = dg.verdict.data(); gio.violation = dg.violation.data(); gio.set_size = dg.set_size.data();
                gio.side = dg.side.data(); gio.unmet = dg.unmet.data();
                CHECK(mcf_rbatch_diagnose_on_host(b, &gio));
                mcf_ubatch_diagnose_stats gs{};
                CHECK(mcf_rbatch_get_diagnose_stats(b, &gs));
                if (gs.open != 0) { fprintf(stderr, "%lld instances without a certificate\n", (long long)gs.open); return 1; }
                diag_levels += gs.levels;
                for (int i = 0; i < count; ++i) {
                    const int32_t v = dg.verdict[(size_t)i];
                    if (v < MCF_DIAG_NONE || v > MCF_DIAG_BOUNDS) { fprintf(stderr, "instance %d: verdict %d\n", i, v); return 1; }
                    ++verdicts[v];
                    int64_t sum = 0, size = 0;
                    for (int64_t k = node_row[(size_t)i]; k < node_row[(size_t)i + 1]; ++k)
                        if (dg.side[(size_t)k]) { sum += dg.unmet[(size_t)k] < 0 ? -dg.unmet[(size_t)k] : dg.unmet[(size_t)k]; ++size; }
                    if (size != dg.set_size[(size_t)i] || (v == MCF_DIAG_CUT) != (dg.violation[(size_t)i] > 0) || (v == MCF_DIAG_CUT && sum != dg.violation[(size_t)i])) {
                        fprintf(stderr, "instance %d: verdict %d, violation %lld, |unmet| over the side %lld\n", i, v, (long long)dg.violation[(size_t)i], (long long)sum);
                        return 1;
                    }
                }
                gio.side = nullptr; gio.unmet = nullptr;                  // without the rows the walk still runs
                const std::vector<int32_t> with_rows = dg.verdict;
                CHECK(mcf_rbatch_diagnose_on_host(b, &gio));
                if (dg.verdict != with_rows) { fprintf(stderr, "another verdict without the node rows\n"); return 1; }
            }
            // unbounded or not, from the same kept state: every output exactly sized; a cycle's marks sum to its cost and count to its
            // length, a bounded instance's labels hold on every uncapacitated arc
            Rays ry((size_t)count, lower.size(), supply.size());
            {
                mcf_rbatch_rays_io yio{};
                yio.memory = MCF_MEM_HOST; yio.verdict = ry.verdict.data(); yio.cycle_cost = ry.cycle_cost.data(); yio.cycle_length = ry.cycle_length.data();
                yio.on_cycle = ry.on_cycle.data(); yio.label = ry.label.data();
                CHECK(mcf_rbatch_rays_on_host(b, &yio));
                mcf_ubatch_rays_stats ys{};
                CHECK(mcf_rbatch_get_rays_stats(b, &ys));
                ray_rounds += ys.rounds;
                for (int i = 0; i < count; ++i) {
                    const int32_t v = ry.verdict[(size_t)i];
                    if (v < MCF_RAY_NONE || v > MCF_RAY_BOUNDS) { fprintf(stderr, "instance %d: ray verdict %d\n", i, v); return 1; }
                    ++ray_verdicts[v];
                    const size_t g = (size_t)graph_of[(size_t)i];
                    int64_t sum = 0, length = 0;
                    bool holds = true;
                    for (int64_t e = 0; e < arc_start[g + 1] - arc_start[g]; ++e) {
                        const size_t at = (size_t)(arc_row[(size_t)i] + e);
                        if (ry.on_cycle[at]) { sum += cost[at]; ++length; }
                        const int64_t *const label = ry.label.data() + node_row[(size_t)i];
                        if (upper[at] == MCF_INF_CAP) holds = holds && label[target[(size_t)(arc_start[g] + e)]] <= label[source[(size_t)(arc_start[g] + e)]] + cost[at];
                    }
                    if (sum != ry.cycle_cost[(size_t)i] || length != ry.cycle_length[(size_t)i] || (v == MCF_RAY_CYCLE) != (sum < 0) || (v == MCF_RAY_BOUNDED && !holds)) {
                        fprintf(stderr, "instance %d: ray verdict %d, cycle cost %lld over %lld arcs, labels %s\n", i, v, (long long)sum, (long long)length, holds ? "hold" : "broken");
                        return 1;
                    }
                }
                yio.on_cycle = nullptr; yio.label = nullptr;              // without the rows the rounds still run
                const Rays with_rows = ry;
                CHECK(mcf_rbatch_rays_on_host(b, &yio));
                if (ry.verdict != with_rows.verdict || ry.cycle_cost != with_rows.cycle_cost || ry.cycle_length != with_rows.cycle_length) {
                    fprintf(stderr, "another ray verdict without the rows\n");
                    return 1;
                }
            }
            {
                mcf_rbatch *from = nullptr;
                CHECK(mcf_rbatch_create(&from, &d));
                Answers s((size_t)count, lower.size(), supply.size());
                mcf_rbatch_io sio = io;
                sio.status = s.status.data(); sio.pivots = s.pivots.data(); sio.total_cost = s.total.data(); sio.flows = s.flows.data(); sio.potentials = s.potentials.data(); sio.trace = s.trace.data();
                mcf_rbatch_basis_io basis{};
                basis.memory = MCF_MEM_HOST; basis.arc_state = arc_state.data();
                CHECK(mcf_rbatch_run_from_on_host(from, &sio, &basis));
                if (s.status != r_first.status || s.total != r_first.total) { fprintf(stderr, "the start from the exported basis answers differently from the solve that left it\n"); return 1; }
                mcf_ubatch_start_stats ss{};
                CHECK(mcf_rbatch_get_start_stats(from, &ss));
                started += ss.primal_starts + ss.dual_starts;
                sio.cost = cost2.data();                                      // other costs on the kept basis: primal pivots from there, or cold
                CHECK(mcf_rbatch_run_from_on_host(from, &sio, &basis));
                mcf_rbatch_destroy(from);
            }
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
            if (sel.empty()) continue;

            // the same calls on the uniform handle: dense rows [instances of graph 0][m0 or n0]
            const std::vector<int64_t> u_lower = dense(lower, arc_row, 1, m0, sel), u_upper = dense(upper, arc_row, 1, m0, sel), u_cost = dense(cost, arc_row, 1, m0, sel),
                                       u_cost2 = dense(cost2, arc_row, 1, m0, sel), u_supply = dense(supply, node_row, 1, n0, sel);
            const std::vector<uint8_t> u_changed = dense(changed, one, 1, 1, sel);
            mcf_ubatch_desc ud{};
            ud.pivot_rule = rule; ud.semantics = MCF_SEM_PLAIN; ud.trace_capacity = kTrace;
            ud.node_count = (int32_t)n0; ud.arc_count = (int32_t)m0; ud.count = (int32_t)sel.size(); ud.source = source.data(); ud.target = target.data();
            mcf_ubatch *ub = nullptr;
            CHECK(mcf_ubatch_create(&ub, &ud));
            Answers u(sel.size(), u_lower.size(), u_supply.size());
            mcf_ubatch_io uio{};
            uio.memory = MCF_MEM_HOST; uio.supply_type = stype;
            uio.lower = u_lower.data(); uio.upper = u_upper.data(); uio.cost = u_cost.data(); uio.supply = u_supply.data();
            uio.lower_stride = uio.upper_stride = uio.cost_stride = m0; uio.supply_stride = n0;
            uio.status = u.status.data(); uio.pivots = u.pivots.data(); uio.total_cost = u.total.data(); uio.flows = u.flows.data(); uio.potentials = u.potentials.data(); uio.trace = u.trace.data();
            CHECK(mcf_ubatch_run_on_host(ub, &uio));
            mcf_ubatch_check_io uc{};
            uc.memory = MCF_MEM_HOST; uc.supply_type = stype;
            uc.lower = u_lower.data(); uc.upper = u_upper.data(); uc.cost = u_cost.data(); uc.supply = u_supply.data();
            uc.lower_stride = uc.upper_stride = uc.cost_stride = m0; uc.supply_stride = n0;
            uc.status = u.status.data(); uc.total_cost = u.total.data(); uc.flows = u.flows.data(); uc.potentials = u.potentials.data();
            uc.valid = u.valid.data(); uc.errors = u.errors.data(); uc.first = u.first.data(); uc.objective = u.objective.data(); uc.dual_cost = u.dual.data();
            CHECK(mcf_ubatch_validate_on_host(ub, &uc, &summary));
            if (!same("first solve", u, r_first, one, arc_row, node_row, n0, m0, sel)) return 1;
            {
                Diagnosis ug(sel.size(), u_supply.size());
                mcf_ubatch_diagnose_io gio{};
                gio.memory = MCF_MEM_HOST; gio.verdict = ug.verdict.data(); gio.violation = ug.violation.data(); gio.set_size = ug.set_size.data();
                gio.side = ug.side.data(); gio.unmet = ug.unmet.data();
                CHECK(mcf_ubatch_diagnose_on_host(ub, &gio));
                if (ug.verdict != dense(dg.verdict, one, 1, 1, sel) || ug.violation != dense(dg.violation, one, 1, 1, sel) || ug.set_size != dense(dg.set_size, one, 1, 1, sel) ||
                    ug.side != dense(dg.side, node_row, 1, n0, sel) || ug.unmet != dense(dg.unmet, node_row, 1, n0, sel)) {
                    fprintf(stderr, "the uniform batch's diagnosis differs from the ragged batch's\n");
                    return 1;
                }
                for (int32_t v : ug.verdict) ++uniform_verdicts[v];
            }
            {
                Rays uy(sel.size(), u_lower.size(), u_supply.size());
                mcf_ubatch_rays_io yio{};
                yio.memory = MCF_MEM_HOST; yio.verdict = uy.verdict.data(); yio.cycle_cost = uy.cycle_cost.data(); yio.cycle_length = uy.cycle_length.data();
                yio.on_cycle = uy.on_cycle.data(); yio.label = uy.label.data();
                CHECK(mcf_ubatch_rays_on_host(ub, &yio));
                if (uy.verdict != dense(ry.verdict, one, 1, 1, sel) || uy.cycle_cost != dense(ry.cycle_cost, one, 1, 1, sel) || uy.cycle_length != dense(ry.cycle_length, one, 1, 1, sel) ||
                    uy.on_cycle != dense(ry.on_cycle, arc_row, 1, m0, sel) || uy.label != dense(ry.label, node_row, 1, n0, sel)) {
                    fprintf(stderr, "the uniform batch's rays differ from the ragged batch's\n");
                    return 1;
                }
                for (int32_t v : uy.verdict) ++uniform_ray_verdicts[v];
            }
            {
                // the cost ranges, and the data ranges with graph 0's pair list, of the same basis: exactly sized, every row the ragged handle's
                const size_t pairs0 = (size_t)pair_row[1];
                std::vector<int32_t> u_ranged(sel.size()), u_data_ranged(sel.size());
                std::vector<int8_t> u_state(u_lower.size()), u_data_state(u_lower.size());
                std::vector<int64_t> u_down(u_lower.size()), u_up(u_lower.size()), u_flow_down(u_lower.size()), u_flow_up(u_lower.size()),
                    u_forth(sel.size() * pairs0), u_back(sel.size() * pairs0);
                mcf_ubatch_range_io urio{};
                urio.memory = MCF_MEM_HOST; urio.ranged = u_ranged.data(); urio.arc_state = u_state.data(); urio.cost_down = u_down.data(); urio.cost_up = u_up.data();
                CHECK(mcf_ubatch_cost_ranges_on_host(ub, &urio));
                mcf_ubatch_data_range_io udio{};
                udio.memory = MCF_MEM_HOST; udio.pairs = pairs.data(); udio.pair_count = (int64_t)pairs0;
                udio.ranged = u_data_ranged.data(); udio.arc_state = u_data_state.data(); udio.flow_down = u_flow_down.data(); udio.flow_up = u_flow_up.data();
                udio.ship_forth = u_forth.data(); udio.ship_back = u_back.data();
                CHECK(mcf_ubatch_data_ranges_on_host(ub, &udio));
                if (u_ranged != dense(ranged, one, 1, 1, sel) || u_state != dense(arc_state, arc_row, 1, m0, sel) || u_down != dense(cost_down, arc_row, 1, m0, sel) ||
                    u_up != dense(cost_up, arc_row, 1, m0, sel)) {
                    fprintf(stderr, "the uniform batch's cost ranges differ from the ragged batch's\n");
                    return 1;
                }
                if (u_data_ranged != u_ranged || u_data_state != u_state || u_flow_down != dense(flow_down, arc_row, 1, m0, sel) ||
                    u_flow_up != dense(flow_up, arc_row, 1, m0, sel) || u_forth != dense(ship_forth, ship_row, 1, (int64_t)pairs0, sel) ||
                    u_back != dense(ship_back, ship_row, 1, (int64_t)pairs0, sel)) {
                    fprintf(stderr, "the uniform batch's data ranges differ from the ragged batch's\n");
                    return 1;
                }
            }
            uio.cost = u_cost2.data(); uio.changed = u_changed.data();
            CHECK(mcf_ubatch_rerun_on_host(ub, &uio));
            uio.changed = nullptr;
            CHECK(mcf_ubatch_rerun_on_host(ub, &uio));
            uc.cost = u_cost2.data();
            CHECK(mcf_ubatch_validate_on_host(ub, &uc, &summary));
            if (!same("re-solve", u, r, one, arc_row, node_row, n0, m0, sel)) return 1;
            mcf_ubatch_destroy(ub);
        }
    printf("ok: %d instances of %d graphs, 3 rules x 2 supply types; %lld pivots in the last re-solves, %lld rows flagged by the first validations; "
           "%lld starts from an exported basis accepted; %lld instances' supply and bound ranges over %lld walks; "
           "the %zu instances of graph 0 as a uniform batch: every row equal\n",
           count, G, (long long)pivots_total, (long long)invalid_total, (long long)started, (long long)data_ranged_total, (long long)data_walks, sel.size());
    printf("diagnosed over all handles: ragged none %lld, feasible %lld, cut %lld, open %lld, by bounds %lld (%lld levels); "
           "uniform none %lld, feasible %lld, cut %lld, open %lld, by bounds %lld\n",
           (long long)verdicts[MCF_DIAG_NONE], (long long)verdicts[MCF_DIAG_FEASIBLE], (long long)verdicts[MCF_DIAG_CUT], (long long)verdicts[MCF_DIAG_OPEN],
           (long long)verdicts[MCF_DIAG_BOUNDS], (long long)diag_levels, (long long)uniform_verdicts[MCF_DIAG_NONE], (long long)uniform_verdicts[MCF_DIAG_FEASIBLE],
           (long long)uniform_verdicts[MCF_DIAG_CUT], (long long)uniform_verdicts[MCF_DIAG_OPEN], (long long)uniform_verdicts[MCF_DIAG_BOUNDS]);
    printf("rays over all handles: ragged none %lld, bounded %lld, cycle %lld, by bounds %lld (%lld rounds); uniform none %lld, bounded %lld, cycle %lld, by bounds %lld\n",
           (long long)ray_verdicts[MCF_RAY_NONE], (long long)ray_verdicts[MCF_RAY_BOUNDED], (long long)ray_verdicts[MCF_RAY_CYCLE], (long long)ray_verdicts[MCF_RAY_BOUNDS],
           (long long)ray_rounds, (long long)uniform_ray_verdicts[MCF_RAY_NONE], (long long)uniform_ray_verdicts[MCF_RAY_BOUNDED], (long long)uniform_ray_verdicts[MCF_RAY_CYCLE],
           (long long)uniform_ray_verdicts[MCF_RAY_BOUNDS]);
    return 0;
}
