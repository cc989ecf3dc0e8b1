"""LEMON's list rules on the device path against Block Search and Best Eligible: whole-solve time, us per pivot, device calls per pivot,
on config 2 (NETGEN-like 10k nodes / 30k arcs, int32) and config 3 (100k / 300k, int64), the bench's instances (seed 13502460).

    python tools/gpu_list_rules.py [--configs config2,config3] [--json out.json]

Block Search and Best Eligible run as bench.py runs them (EnableOptimizedPivot(true), x64 vector width, resident grid); a device call there is a
search the host's candidate cache did not answer.  For the list rules a device call is a major scan (mcf_engine_collect_eligible: the
queued patches, a count pass and an emit pass, one stream synchronisation).  Every solve is checked Optimal with the same cost.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import mincostflow_amd as M  # noqa: E402

SEED = 13502460
CONFIGS = {
    "config2": (lambda: M.netgen_like(SEED, 10_000, 30_000, 100, 100), 32),
    "config3": (lambda: M.netgen_like(SEED, 100_000, 300_000, 316, 316), 64),
}
RULES = [("BlockSearch", M.PivotRule.BlockSearch), ("BestEligible", M.PivotRule.BestEligible),
         ("CandidateList", M.PivotRule.CandidateList), ("AlteringList", M.PivotRule.AlteringList)]


def run(g, width, name, rule):
    ns = M.NetworkSimplex.from_problem(g)
    if rule in (M.PivotRule.CandidateList, M.PivotRule.AlteringList):
        ns.set_list_pivot_rule(rule)
    else:
        ns.set_pivot_rule(rule).enable_optimized_pivot(True).set_vector_width(4)
    ns.set_device(0, width, 0, 0)
    t0 = time.perf_counter()
    st = ns.solve()
    wall = time.perf_counter() - t0
    assert st == M.SolverStatus.Optimal, (name, st)
    m = ns.get_metrics()
    it = max(m["iterations"], 1)
    out = {"rule": name, "status": st, "cost": ns.get_total_cost(), "pivots": m["iterations"], "solve_s": round(wall, 3),
           "total_solve_us": round(m["total_solve_us"], 1), "loop_us_per_pivot": round(m["loop_us"] / it, 3),
           "search_us_per_pivot": round(m["pivot_search_us"] / it, 3)}
    if rule in (M.PivotRule.CandidateList, M.PivotRule.AlteringList):
        ls = ns.list_rule_stats()
        out.update(device_calls=ls["major_scans"], device_calls_per_pivot=round(ls["major_scans"] / it, 4),
                   host_answered_fraction=round(ls["host_answered"] / max(ls["searches"], 1), 4),
                   collect_us_per_call=round(ls["collect_us"] / max(ls["major_scans"], 1), 2),
                   lemon_arcs_scanned_per_call=round(ls["lemon_arcs_scanned"] / max(ls["major_scans"], 1), 1),
                   collected_per_call=round(ls["collected"] / max(ls["major_scans"], 1), 1), list_stats=ls)
    else:
        e = m["engine"]
        calls = e["searches"] - e["host_decided"]
        out.update(device_calls=calls, device_calls_per_pivot=round(calls / it, 4),
                   host_answered_fraction=round(e["host_decided"] / max(e["searches"], 1), 4), resident=e["resident"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="config2,config3")
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    if M.device_count() < 1:
        raise SystemExit("needs an MI355X")
    res = {}
    for cfg in args.configs.split(","):
        make, width = CONFIGS[cfg]
        g = make()
        rows = []
        for name, rule in RULES:
            r = run(g, width, name, rule)
            rows.append(r)
            print(f"{cfg} {name:14s} pivots {r['pivots']:8d}  solve {r['solve_s']:8.3f} s  {r['loop_us_per_pivot']:8.2f} us/pivot  "
                  f"device calls/pivot {r['device_calls_per_pivot']:.3f}  host-answered {100 * r['host_answered_fraction']:5.1f} %", flush=True)
        costs = {r["cost"] for r in rows}
        assert len(costs) == 1, costs
        res[cfg] = rows
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
