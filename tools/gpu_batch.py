"""Throughput of the batch solver (mcf_batch_solve) against what existed before it, on two families of generated instances:

  small  200 nodes / 600 arcs      (the scale of the bundled scheduling instances; every workspace fits LDS)
  large  10 000 nodes / 30 000 arcs (config 2; the pivots run in place on the workspace in global memory)

    timeout 900 python tools/gpu_batch.py [--json profiles/batch_solve.json]

Legs, all with the plain auto-configured Block Search (`new NetworkSimplex(g).Solve()`), every instance with a seed of its own:
  1. the batch: one mcf_batch_solve per batch size (1, 64, 256, 1024, 4096; the large family up to 256);
  2. the same instances one after another through mcf_ns_solve on the same GPU (what there was before), a sample of them;
  3. the CPU oracle (oracle/ns_oracle.c, SEM_CSHARP) on one pinned core, a sample of them.
Legs 2 and 3 solve one instance at a time, so their rate does not depend on the batch size: they are timed over a sample (64 small /
8 large instances) and reported per solve.  Each shape is warmed up first; every time is a host clock round work that ends in a device
synchronise (mcf_batch_solve and mcf_ns_solve both return after their last copy back).  Leg 1's pivot counts are checked against leg 3's.
The script stops at the first failure.  (The one script here that imports oracle/: leg 3 IS the oracle.)
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import mincostflow_amd as M  # noqa: E402
from oracle import ns_oracle as O  # noqa: E402

FAMILIES = {
    "small": dict(nodes=200, arcs=600, ends=4, sizes=[1, 64, 256, 1024, 4096], sample=64, seed0=1),
    "large": dict(nodes=10_000, arcs=30_000, ends=100, sizes=[1, 64, 256], sample=8, seed0=100_001),
}
CORES_PER_JOB = 16


def instances(f, count):
    return [M.netgen_like(f["seed0"] + k, f["nodes"], f["arcs"], f["ends"], f["ends"]) for k in range(count)]


def leg_batch(problems):
    b = M.BatchSolver(rule=M.PivotRule.BlockSearch)
    for g in problems:
        b.add(g)
    t0 = time.perf_counter()
    b.solve()
    wall = time.perf_counter() - t0
    assert all(b.status(i) == M.SolverStatus.Optimal for i in range(len(problems)))
    st = b.stats()
    per_instance = [b.pivots(i) for i in range(len(problems))]
    cus = M._lib.lib().mcf_device_compute_units(0)
    return dict(instances=len(problems), wall_s=wall, kernel_s=st["kernel_ns"] / 1e9, host_s=st["host_ns"] / 1e9, launches=st["launches"],
                pivots=st["total_pivots"], solves_per_s=len(problems) / wall, pivots_per_s=st["total_pivots"] / wall,
                # a workgroup carries one instance from its first pivot to its last: its pivots took the launches' time, or less
                us_per_pivot_per_workgroup=st["kernel_ns"] / 1e3 / max(per_instance), lds_instances=st["lds_instances"],
                global_instances=st["global_instances"], lds_bytes_max=st["lds_bytes_max"], workspace_bytes=st["workspace_bytes"],
                compute_units=cus), per_instance


def leg_single(problems):
    pivots, wall = 0, 0.0
    for g in problems:
        ns = M.NetworkSimplex.from_problem(g).set_pivot_rule(M.PivotRule.BlockSearch).enable_optimized_pivot(False)
        t0 = time.perf_counter()
        st = ns.solve()
        wall += time.perf_counter() - t0
        assert st == M.SolverStatus.Optimal
        pivots += ns.get_metrics()["iterations"]
    return dict(instances=len(problems), wall_s=wall, pivots=pivots, solves_per_s=len(problems) / wall, pivots_per_s=pivots / wall,
                us_per_pivot=wall * 1e6 / pivots)


def leg_oracle(problems):
    pivots, wall, per_instance = 0, 0.0, []
    for g in problems:
        p = O.Problem(g.node_count, g.arc_count, g.source, g.target, g.lower, g.upper, g.cost, g.supply)
        o = O.Oracle(p, O.SEM_CSHARP, O.RULE_BLOCK, auto_config=True)
        t0 = time.perf_counter()
        st, _ = o.solve()
        wall += time.perf_counter() - t0
        assert st == O.OPTIMAL
        pivots += o.n_pivots
        per_instance.append(o.n_pivots)
    return dict(instances=len(problems), wall_s=wall, pivots=pivots, solves_per_s=len(problems) / wall, pivots_per_s=pivots / wall,
                us_per_pivot=wall * 1e6 / pivots), per_instance


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--families", default="small,large")
    args = ap.parse_args()
    if M.device_count() < 1:
        raise SystemExit("needs an MI355X")
    os.sched_setaffinity(0, {sorted(os.sched_getaffinity(0))[0]})          # one pinned core for the whole process (leg 3 is the one it matters for)
    out = {"rule": "BlockSearch (plain, auto-configured)", "families": {}}
    for name in args.families.split(","):
        f = FAMILIES[name]
        problems = instances(f, max(f["sizes"]))
        sample = problems[: f["sample"]]
        leg_batch(sample)                                                  # warm-up of the shape: kernels loaded, allocator primed
        leg_single(sample[:2])
        legs1 = []
        oracle, oracle_pivots = leg_oracle(sample)
        single = leg_single(sample)
        for size in f["sizes"]:
            r, per_instance = leg_batch(problems[:size])
            assert per_instance[: len(oracle_pivots)] == oracle_pivots[:size], "pivot counts differ from the oracle's"
            r["vs_single_solves"] = r["solves_per_s"] / single["solves_per_s"]
            r["vs_one_core"] = r["solves_per_s"] / oracle["solves_per_s"]
            r["vs_16_cores"] = r["vs_one_core"] / CORES_PER_JOB
            legs1.append(r)
            print(f"{name} batch {size:5d}: {r['wall_s'] * 1e3:9.2f} ms  {r['solves_per_s']:10.1f} solves/s  {r['pivots_per_s'] / 1e6:7.3f} M pivots/s  "
                  f"{r['us_per_pivot_per_workgroup']:6.2f} us/pivot/workgroup  launches {r['launches']}  x{r['vs_single_solves']:.2f} of mcf_ns_solve  "
                  f"x{r['vs_one_core']:.2f} of one core  x{r['vs_16_cores']:.2f} of {CORES_PER_JOB} cores", flush=True)
        for label, r in (("mcf_ns_solve, one after another", single), ("oracle, one core", oracle)):
            print(f"{name} {label}: {r['instances']} instances  {r['solves_per_s']:10.1f} solves/s  {r['pivots_per_s'] / 1e6:7.3f} M pivots/s  {r['us_per_pivot']:6.2f} us/pivot", flush=True)
        over = [r["instances"] for r in legs1 if r["vs_16_cores"] > 1.0]
        out["families"][name] = dict(nodes=f["nodes"], arcs=f["arcs"], batch=legs1, single=single, oracle_one_core=oracle,
                                     overtakes_16_cores_from_batch=min(over) if over else None)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)
    print(json.dumps({k: v["overtakes_16_cores_from_batch"] for k, v in out["families"].items()}))


if __name__ == "__main__":
    main()
