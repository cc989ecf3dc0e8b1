"""A/B of the host half of a pivot between two builds of the library, on the CPU alone (no device is opened): config 3's Best Eligible pivot
sequence through mcf_ns_replay with the walk aids mcf_ns_solve starts with (smaller side, relabelling every 128 n walked nodes).

    python tools/cpu_replay_ab.py trace c3_trace.npy                    # once: the oracle's trace (a minute or two)
    python tools/cpu_replay_ab.py ab c3_trace.npy /path/to/base.so [5]  # base and new alternating, each in a process of its own
    python tools/cpu_replay_ab.py ab c3_trace.npy /path/to/base/checkout [5]   # the same, the base (built) with its own Python side

The trace is the oracle's, which the GPU parity test asserts is also the product's; both builds get the same array.  Per pivot: tree_update_us
(the re-hanging), potential_update_us (the walk) and the rest of loop_us (cycle search, State[], flows, relabellings).  A CPU timing of CPU
code on one pinned core.  (Imports oracle/ for the trace only.)"""
import os
import statistics
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def problem():
    import mincostflow_amd as M
    return M.netgen_like(13502460, 100_000, 300_000, 316, 316)


def main():
    mode, path = sys.argv[1], sys.argv[2]
    if mode == "trace":
        from oracle import ns_oracle as O
        g = problem()
        o = O.Oracle(O.Problem(g.node_count, g.arc_count, g.source, g.target, g.lower, g.upper, g.cost, g.supply), O.SEM_CSHARP_OPT, O.RULE_BEST)
        st, trace = o.solve(trace_cap=1 << 20)
        assert st == O.OPTIMAL
        np.save(path, np.asarray(trace, np.int32))
        print(f"{len(trace)} pivots")
    elif mode == "one":
        os.sched_setaffinity(0, {sorted(os.sched_getaffinity(0))[0]})
        import mincostflow_amd._lib as L
        if os.environ.get("MCF_AB_LIB"):
            L.LIB_PATH = os.environ["MCF_AB_LIB"]
        import mincostflow_amd as M
        g, arcs = problem(), np.load(path)
        ns = M.NetworkSimplex.from_problem(g)
        assert ns.begin() != M.SolverStatus.Infeasible
        ns.replay(arcs, smaller_side=True, renumber_every=128.0)
        m = ns.get_metrics()
        assert m["iterations"] == len(arcs) and ns.finish() == M.SolverStatus.Optimal
        it = m["iterations"]
        print(m["tree_update_us"] / it, m["potential_update_us"] / it, (m["loop_us"] - m["tree_update_us"] - m["potential_update_us"]) / it, m["loop_us"] / it,
              ns.get_total_cost())
    else:
        base, reps = sys.argv[3], int(sys.argv[4]) if len(sys.argv) > 4 else 5
        rows = {"base": [], "new": []}
        for _ in range(reps):
            # base: another build of the library under this tree's Python, or (a directory) another checkout, run with its own Python side --
            # needed when this tree's bindings name a symbol that the base build does not export
            base_script = os.path.join(base, "tools", os.path.basename(__file__)) if os.path.isdir(base) else __file__
            for name, script, env in (("base", base_script, {} if os.path.isdir(base) else {"MCF_AB_LIB": os.path.abspath(base)}), ("new", __file__, {})):
                out = subprocess.run([sys.executable, script, "one", os.path.abspath(path)], env=dict(os.environ, **env), check=True, capture_output=True, text=True).stdout.split()
                rows[name].append([float(x) for x in out[:4]] + [int(out[4])])
                print(name, *out, flush=True)
        assert len({r[4] for rs in rows.values() for r in rs}) == 1, "total costs differ"
        for k, what in enumerate(("tree_update", "potential_update", "rest of loop", "loop")):
            b, n = [r[k] for r in rows["base"]], [r[k] for r in rows["new"]]
            print(f"{what:17s} us/pivot: base median {statistics.median(b):.4f} (min {min(b):.4f}, max {max(b):.4f})   new median {statistics.median(n):.4f} "
                  f"(min {min(n):.4f}, max {max(n):.4f})")


if __name__ == "__main__":
    main()
