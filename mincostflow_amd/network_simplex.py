"""Python mirror of the reference's solver surface over the C ABI.

`NetworkSimplex` keeps the method names and argument meaning of the reference class
(src/MinCostFlow.Core/Lemon/Algorithms/NetworkSimplex.cs:153-587): set_arc_bounds / set_arc_cost /
set_node_supply / set_supply_type / set_pivot_rule / enable_optimized_pivot / solve / get_flow /
get_potential / get_total_cost / status / get_metrics.  Everything is forwarded to libmcf_hip.so; the
entering-arc search and the potential update run on the MI355X, nothing is computed in Python.

`PivotEngine` is the bare device seam (`IFindEnteringArc`, NetworkSimplex.cs:1286-1289) for hosts that
own their spanning tree.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib as L
from ._lib import McfError  # noqa: F401  (re-export)


class PivotRule:                      # Types/PivotRule.cs
    FirstEligible, BestEligible, BlockSearch, CandidateList, AlteringList = 0, 1, 2, 3, 4


class SupplyType:                     # Types/SupplyType.cs
    Geq, Leq = 0, 1


class SolverStatus:                   # Types/SolverStatus.cs
    NotSolved, Optimal, Infeasible, Unbounded, Unbalanced = 0, 1, 2, 3, 4


class Verdict:                        # MCF_DIAG_* of include/mcf_hip.h: what diagnose() says of an instance
    NoVerdict, Feasible, Cut, Open, Bounds = L.DIAG_NONE, L.DIAG_FEASIBLE, L.DIAG_CUT, L.DIAG_OPEN, L.DIAG_BOUNDS


class Ray:                            # MCF_RAY_* of include/mcf_hip.h: what rays() says of an instance
    NoVerdict, Bounded, Cycle, Bounds = L.RAY_NONE, L.RAY_BOUNDED, L.RAY_CYCLE, L.RAY_BOUNDS


def _vector_width_abi(v: int) -> int:
    """Python side: 0 = not hardware accelerated, 2 / 4 / 8 = Vector<long>.Count (the oracle's convention).  C ABI: MCF_VECTOR_NONE = -1, 0 = default (4)."""
    if v not in (0, 2, 4, 8):
        raise ValueError(f"vector_width {v} is not one of 0, 2, 4, 8")
    return L.VECTOR_NONE if v == 0 else v


def _i32(a): return np.ascontiguousarray(a, np.int32)
def _i64(a): return np.ascontiguousarray(a, np.int64)
def _i8(a): return np.ascontiguousarray(a, np.int8)


@dataclass
class Problem:
    """Flat min-cost-flow instance, 0-based; upper == INF_CAP means unbounded."""
    node_count: int
    arc_count: int
    source: np.ndarray
    target: np.ndarray
    lower: np.ndarray
    upper: np.ndarray
    cost: np.ndarray
    supply: np.ndarray

    @staticmethod
    def _take(ps: L.ProblemStruct) -> "Problem":
        n, m = ps.node_count, ps.arc_count
        def arr(ptr, k, dt):
            return np.ctypeslib.as_array(ptr, shape=(max(k, 1),))[:k].astype(dt, copy=True)
        p = Problem(n, m, arr(ps.source, m, np.int32), arr(ps.target, m, np.int32), arr(ps.lower, m, np.int64),
                    arr(ps.upper, m, np.int64), arr(ps.cost, m, np.int64), arr(ps.supply, n, np.int64))
        L.lib().mcf_problem_free(C.byref(ps))
        return p


def netgen_like(seed: int, nodes: int, arcs: int, n_src: int, n_snk: int, min_cost=1, max_cost=10000,
                min_cap=1, max_cap=1000) -> Problem:
    """Build-owned NETGEN-like generator; mirrors the headers of the bundled netgen_8_*.min files."""
    ps = L.ProblemStruct()
    L.check(L.lib().mcf_gen_netgen_like(C.byref(ps), seed, nodes, arcs, n_src, n_snk, min_cost, max_cost, min_cap, max_cap))
    return Problem._take(ps)


def assignment(seed: int, n: int, min_cost=1, max_cost=100) -> Problem:
    ps = L.ProblemStruct()
    L.check(L.lib().mcf_gen_assignment(C.byref(ps), seed, n, min_cost, max_cost))
    return Problem._take(ps)


def read_dimacs(path: str) -> Problem:
    ps = L.ProblemStruct()
    L.check(L.lib().mcf_dimacs_read(C.byref(ps), path.encode()))
    return Problem._take(ps)


def _borrow(p: Problem):
    """A mcf_problem view of p's arrays (they must stay alive while the struct is in use)."""
    keep = (_i32(p.source), _i32(p.target), _i64(p.lower), _i64(p.upper), _i64(p.cost), _i64(p.supply))
    src, tgt, lo, up, co, su = keep
    ps = L.ProblemStruct(p.node_count, p.arc_count, src.ctypes.data_as(C.POINTER(C.c_int32)),
                         tgt.ctypes.data_as(C.POINTER(C.c_int32)), lo.ctypes.data_as(C.POINTER(C.c_int64)),
                         up.ctypes.data_as(C.POINTER(C.c_int64)), co.ctypes.data_as(C.POINTER(C.c_int64)),
                         su.ctypes.data_as(C.POINTER(C.c_int64)))
    return ps, keep


def write_dimacs(p: Problem, path: str) -> None:
    ps, _keep = _borrow(p)
    L.check(L.lib().mcf_dimacs_write(C.byref(ps), path.encode()))


def write_solution(path: str, cost: int, flow, pi=None) -> None:
    """SolutionLoader.SaveToFile (Loaders/SolutionLoader.cs:186-210)."""
    flow = _i64(flow)
    pi = None if pi is None else _i64(pi)
    L.check(L.lib().mcf_solution_write(path.encode(), int(cost), flow.shape[0], flow.ctypes.data_as(C.c_void_p),
                                       0 if pi is None else pi.shape[0], None if pi is None else pi.ctypes.data_as(C.c_void_p)))


def read_solution(path: str, p: Problem) -> dict:
    """SolutionLoader.LoadFromFile (:59-176) mapped onto p's arcs: {'cost' (None when the file has no s line), 'flow', 'pi' (None without p lines)}."""
    ps, _keep = _borrow(p)
    flow, pi = np.zeros(max(p.arc_count, 1), np.int64), np.zeros(max(p.node_count, 1), np.int64)
    cost, has_cost, has_pi = C.c_int64(), C.c_int32(), C.c_int32()
    L.check(L.lib().mcf_solution_read(path.encode(), C.byref(ps), C.byref(cost), C.byref(has_cost), flow.ctypes.data_as(C.c_void_p),
                                      pi.ctypes.data_as(C.c_void_p), C.byref(has_pi)))
    return {"cost": cost.value if has_cost.value else None, "flow": flow[: p.arc_count], "pi": pi[: p.node_count] if has_pi.value else None}


class NetworkSimplex:
    """Primal network simplex; same call sequence as the reference class."""

    def __init__(self, node_count: int, source, target):
        self._src, self._tgt = _i32(source), _i32(target)
        self.node_count, self.arc_count = int(node_count), int(self._src.shape[0])
        self._h = C.c_void_p()
        L.check(L.lib().mcf_ns_create(C.byref(self._h), self.node_count, self.arc_count, self._src, self._tgt))
        self._trace = None

    @classmethod
    def from_problem(cls, p: Problem) -> "NetworkSimplex":
        ns = cls(p.node_count, p.source, p.target)
        ns.set_problem(p.lower, p.upper, p.cost, p.supply)
        return ns

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            L.lib().mcf_ns_destroy(h)
            self._h = None

    # --- NetworkSimplex.cs:153-210
    def set_arc_bounds(self, arc: int, lower: int, upper: int):
        L.check(L.lib().mcf_ns_set_arc_bounds(self._h, arc, lower, upper)); return self

    def set_arc_cost(self, arc: int, cost: int):
        L.check(L.lib().mcf_ns_set_arc_cost(self._h, arc, cost)); return self

    def set_node_supply(self, node: int, supply: int):
        L.check(L.lib().mcf_ns_set_node_supply(self._h, node, supply)); return self

    def set_problem(self, lower=None, upper=None, cost=None, supply=None):
        keep = [None if a is None else _i64(a) for a in (lower, upper, cost, supply)]
        ptr = [None if a is None else a.ctypes.data for a in keep]
        L.check(L.lib().mcf_ns_set_problem(self._h, *ptr)); return self

    def set_supply_type(self, t: int):
        L.check(L.lib().mcf_ns_set_supply_type(self._h, t)); return self

    def set_pivot_rule(self, rule: int):
        L.check(L.lib().mcf_ns_set_pivot_rule(self._h, rule)); return self

    def set_list_pivot_rule(self, rule: int):
        """LEMON's Candidate List (PivotRule.CandidateList) or Altering List (PivotRule.AlteringList) rule: the reference declares both and throws
        (NetworkSimplex.cs:879-885); here minor iterations run on the host driver and the major scans on the device.  set_pivot_rule replaces it.
        The list rules ignore enable_optimized_pivot, the vector width, the optimization config and auto-configuration; sharding is refused."""
        L.check(L.lib().mcf_ns_set_list_pivot_rule(self._h, rule)); return self

    def list_rule_stats(self) -> dict:
        """mcf_ns_get_list_rule_stats: major scans (device calls), searches answered on the host, arcs the device read, of the last solve."""
        st = L.ListRuleStats(); L.check(L.lib().mcf_ns_get_list_rule_stats(self._h, C.byref(st))); return st.as_dict()

    def enable_optimized_pivot(self, enable: bool = True):     # NetworkSimplex.cs:532-535
        L.check(L.lib().mcf_ns_enable_optimized_pivot(self._h, int(enable))); return self

    def set_vector_width(self, vector_width: int):
        """Vector<long>.Count of the machine whose EnableOptimizedPivot(true) Block Search is reproduced: 4 (x64, the default), 2, 8, or
        0 = Vector.IsHardwareAccelerated is false (BlockSearchPivotOptimized.cs:74, :115; the reference reads the property, it has no setter)."""
        L.check(L.lib().mcf_ns_set_vector_width(self._h, _vector_width_abi(vector_width))); return self

    # --- NetworkSimplex.cs:549-570
    def set_optimization_config(self, config):                 # SetOptimizationConfig: switches auto-configuration off
        L.check(L.lib().mcf_ns_set_optimization_config(self._h, C.byref(config))); return self

    def enable_optimizations(self, flags: int):
        L.check(L.lib().mcf_ns_enable_optimizations(self._h, flags)); return self

    def set_auto_configuration(self, enable: bool = True):     # the reference's default is on
        L.check(L.lib().mcf_ns_set_auto_configuration(self._h, int(enable))); return self

    # --- device options (no counterpart in the reference)
    def set_device(self, device=0, int_width=0, block_size=0, engine_flags=0):
        L.check(L.lib().mcf_ns_set_device(self._h, device, int_width, block_size, engine_flags)); return self

    def set_device_share(self, resident_workgroups: int):
        """mcf_ns_set_device_share: this solver's resident grid gets that many workgroups (256 / K for K solvers in flight on one device)."""
        L.check(L.lib().mcf_ns_set_device_share(self._h, resident_workgroups)); return self

    def set_sharding(self, nccl_id: np.ndarray, rank: int, world: int):
        L.check(L.lib().mcf_ns_set_sharding(self._h, np.ascontiguousarray(nccl_id, np.uint8), rank, world)); return self

    def set_sharding_host(self, exchange_name: str, rank: int, world: int):
        """Arc shards over `world` ranks of one node, candidates exchanged through shared memory (mcf_exchange_*)."""
        L.check(L.lib().mcf_ns_set_sharding_host(self._h, exchange_name.encode(), rank, world)); return self

    def set_shard_group(self, devices):
        """Arc shards inside this process: one engine per entry of `devices` (entries may repeat), reduced by the host thread."""
        d = _i32(devices)
        L.check(L.lib().mcf_ns_set_shard_group(self._h, d.shape[0], d)); return self

    def set_pivot_limit(self, max_pivots: int):
        L.check(L.lib().mcf_ns_set_pivot_limit(self._h, max_pivots)); return self

    def record_trace(self, capacity: int):
        self._trace = np.zeros(max(capacity, 1), np.int32)
        L.check(L.lib().mcf_ns_set_trace(self._h, self._trace.ctypes.data, capacity)); return self

    def trace(self) -> np.ndarray:
        n = C.c_int64()
        L.check(L.lib().mcf_ns_get_trace_length(self._h, C.byref(n)))
        return self._trace[: n.value].copy()

    def prepare(self):
        """Standard form, start basis, engine creation and upload of the SoA arrays into HBM (solve() does it if needed)."""
        L.check(L.lib().mcf_ns_prepare(self._h)); return self

    # --- NetworkSimplex.cs:215-470
    def solve(self) -> int:
        st = C.c_int32()
        L.check(L.lib().mcf_ns_solve(self._h, C.byref(st)))
        return st.value

    @property
    def status(self) -> int:
        st = C.c_int32()
        L.check(L.lib().mcf_ns_status(self._h, C.byref(st)))
        return st.value

    def get_flow(self, arc: int) -> int:
        v = C.c_int64(); L.check(L.lib().mcf_ns_get_flow(self._h, arc, C.byref(v))); return v.value

    def get_potential(self, node: int) -> int:
        v = C.c_int64(); L.check(L.lib().mcf_ns_get_potential(self._h, node, C.byref(v))); return v.value

    def get_total_cost(self) -> int:
        v = C.c_int64(); L.check(L.lib().mcf_ns_get_total_cost(self._h, C.byref(v))); return v.value

    def get_arc_upper_bound(self, arc: int) -> int:
        v = C.c_int64(); L.check(L.lib().mcf_ns_get_arc_upper_bound(self._h, arc, C.byref(v))); return v.value

    def flows(self) -> np.ndarray:
        out = np.empty(max(self.arc_count, 1), np.int64); L.check(L.lib().mcf_ns_get_flows(self._h, out)); return out[: self.arc_count]

    def potentials(self) -> np.ndarray:
        out = np.empty(max(self.node_count, 1), np.int64); L.check(L.lib().mcf_ns_get_potentials(self._h, out)); return out[: self.node_count]

    def get_metrics(self) -> dict:
        m = L.NsMetrics(); L.check(L.lib().mcf_ns_get_metrics(self._h, C.byref(m))); return m.as_dict()

    def check_reduced_costs(self) -> int:
        m = C.c_int64(); L.check(L.lib().mcf_ns_check_reduced_costs(self._h, C.byref(m))); return m.value

    def validate(self) -> dict:                                  # SolutionValidator(graph, solver).Validate()
        v = L.Validation(); L.check(L.lib().mcf_ns_validate(self._h, C.byref(v))); return v.as_dict()

    # --- the sequential half on its own (what a C# host keeps); never searches for an entering arc
    def begin(self) -> int:
        st = C.c_int32(); L.check(L.lib().mcf_ns_begin(self._h, C.byref(st))); return st.value

    def apply_pivot(self, entering_arc: int) -> bool:
        unb = C.c_int32(); L.check(L.lib().mcf_ns_apply_pivot(self._h, entering_arc, C.byref(unb))); return bool(unb.value)

    def finish(self) -> int:
        st = C.c_int32(); L.check(L.lib().mcf_ns_finish(self._h, C.byref(st))); return st.value

    def replay(self, arcs, smaller_side=True, renumber_every=0.0):
        """mcf_ns_replay: the given entering arcs applied back to back (no engine): the sequential half alone, timed in get_metrics()."""
        arcs = _i32(arcs)
        L.check(L.lib().mcf_ns_replay(self._h, arcs, arcs.shape[0], int(smaller_side), float(renumber_every)))
        m = L.NsMetrics(); L.check(L.lib().mcf_ns_get_metrics(self._h, C.byref(m)))
        self.replay_relabellings = int(m.reserved)          # how often the nodes were relabelled (mcf_ns_metrics.reserved after a replay)
        return self

    def check_thread_breaks(self) -> int:
        """mcf_ns_check_thread_breaks: bits of the driver's thread-break bitmap that differ from a recomputation (0 without a bitmap)."""
        m = C.c_int64(); L.check(L.lib().mcf_ns_check_thread_breaks(self._h, C.byref(m))); return m.value

    def internal(self) -> dict:
        ms, cap = C.c_int32(), C.c_int32()
        ps, pt = C.POINTER(C.c_int32)(), C.POINTER(C.c_int32)()
        pc, ppi, pst = C.POINTER(C.c_int64)(), C.POINTER(C.c_int64)(), C.POINTER(C.c_int8)()
        L.check(L.lib().mcf_ns_internal(self._h, C.byref(ms), C.byref(cap), C.byref(ps), C.byref(pt), C.byref(pc), C.byref(pst), C.byref(ppi)))
        a, n1 = cap.value, self.node_count + 1
        cp = lambda p, k: np.ctypeslib.as_array(p, shape=(k,)).copy()
        return dict(search_arc_num=ms.value, arc_capacity=a, source=cp(ps, a), target=cp(pt, a), cost=cp(pc, a),
                    state=cp(pst, a), pi=cp(ppi, n1))

    def tree(self) -> dict:
        """Copies of Parent, Pred, SuccNum, PredDir (node_count + 1 entries) and the internal flow / upper arrays (arc_capacity entries)."""
        par, pred, succ = C.POINTER(C.c_int32)(), C.POINTER(C.c_int32)(), C.POINTER(C.c_int32)()
        pdir, flow, upper = C.POINTER(C.c_int8)(), C.POINTER(C.c_int64)(), C.POINTER(C.c_int64)()
        L.check(L.lib().mcf_ns_tree(self._h, C.byref(par), C.byref(pred), C.byref(succ), C.byref(pdir), C.byref(flow), C.byref(upper)))
        n1, a = self.node_count + 1, self.arc_count + 2 * self.node_count
        cp = lambda p, k: np.ctypeslib.as_array(p, shape=(k,)).copy()
        return dict(parent=cp(par, n1), pred_arc=cp(pred, n1), succ_num=cp(succ, n1), pred_dir=cp(pdir, n1), flow=cp(flow, a), upper=cp(upper, a))

    def last_pivot(self) -> dict:
        """mcf_ns_last_pivot: the State[] writes, sigma and the nodes whose potential moved (`count` of them; `nodes` is empty where the
        walk wrote no list down, a reload inside Solve())."""
        ns, nn, sigma = C.c_int32(), C.c_int32(), C.c_int64()
        arcs, states = (C.c_int32 * 2)(), (C.c_int8 * 2)()
        nodes = C.POINTER(C.c_int32)()
        L.check(L.lib().mcf_ns_last_pivot(self._h, C.byref(ns), arcs, states, C.byref(nn), C.byref(nodes), C.byref(sigma)))
        nd = np.ctypeslib.as_array(nodes, shape=(nn.value,)).copy() if nn.value and nodes else np.zeros(0, np.int32)
        return dict(state_arcs=np.array(arcs[: ns.value], np.int32), state_values=np.array(states[: ns.value], np.int8),
                    nodes=nd, count=nn.value, sigma=sigma.value)


class BatchSolver:
    """Many small independent instances, each solved entirely on the device by one workgroup (mcf_batch_*).

    add() copies an instance and returns its index; solve() runs the whole batch on the MI355X; the getters answer per index what
    NetworkSimplex answers for a single solve with the same rule and enable_optimized_pivot(False).  run_on_host() is a test hook
    (the same pivot code with one lane on the CPU), not a supported solver.  A solved batch stays on the device: set_costs() gives
    instances new arc costs and resolve() re-solves those from the basis they ended with (rerun_on_host() is its test hook)."""

    def __init__(self, rule=PivotRule.BlockSearch, pivot_limit=0, record_trace=0, device=0, pivots_per_launch=0, semantics=L.SEM_PLAIN, flags=0):
        self._h = C.c_void_p()
        self._problems = []           # (node_count, arc_count) per index
        d = L.BatchDesc(int(device), int(rule), int(semantics), 0, int(pivot_limit), int(pivots_per_launch), int(record_trace), int(flags))
        L.check(L.lib().mcf_batch_create(C.byref(self._h), C.byref(d)))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            L.lib().mcf_batch_destroy(h)
            self._h = None

    def __len__(self):
        return len(self._problems)

    def add(self, problem, supply_type=SupplyType.Geq) -> int:
        """problem: anything with the fields of Problem (node_count / arc_count / source / ...) or of the oracle's (n / m / src / tgt / ...)."""
        g = lambda a, b: getattr(problem, a) if hasattr(problem, a) else getattr(problem, b)
        n, m = int(g("node_count", "n")), int(g("arc_count", "m"))
        src, tgt = _i32(g("source", "src")), _i32(g("target", "tgt"))
        lo, up, co, su = _i64(problem.lower), _i64(problem.upper), _i64(problem.cost), _i64(problem.supply)
        if src.shape != (m,) or tgt.shape != (m,) or lo.shape != (m,) or up.shape != (m,) or co.shape != (m,) or su.shape != (n,):
            raise ValueError("array lengths do not match node_count / arc_count")
        idx = C.c_int32(-1)
        L.check(L.lib().mcf_batch_add(self._h, n, m, src.ctypes.data, tgt.ctypes.data, lo.ctypes.data, up.ctypes.data, co.ctypes.data,
                                      su.ctypes.data, int(supply_type), C.byref(idx)))
        self._problems.append((n, m))
        return idx.value

    def solve(self):
        L.check(L.lib().mcf_batch_solve(self._h)); return self

    def run_on_host(self):
        L.check(L.lib().mcf_batch_run_on_host(self._h)); return self

    def set_costs(self, i: int, cost):
        """New arc costs for instance i of a solved batch (copied); resolve() then re-solves it from the basis its last solve left."""
        co = _i64(cost)
        if co.shape != (self._dims(i)[1],):
            raise ValueError("cost must have arc_count entries")
        L.check(L.lib().mcf_batch_set_costs(self._h, i, co.ctypes.data)); return self

    def resolve(self):
        L.check(L.lib().mcf_batch_resolve(self._h)); return self

    def rerun_on_host(self):
        """Test hook like run_on_host(): resolve() with one lane on the CPU."""
        L.check(L.lib().mcf_batch_rerun_on_host(self._h)); return self

    def resolve_stats(self) -> dict:
        st = L.BatchResolveStats(); L.check(L.lib().mcf_batch_get_resolve_stats(self._h, C.byref(st))); return st.as_dict()

    def status(self, i: int) -> int:
        v = C.c_int32(); L.check(L.lib().mcf_batch_get_status(self._h, i, C.byref(v))); return v.value

    def total_cost(self, i: int) -> int:
        v = C.c_int64(); L.check(L.lib().mcf_batch_get_total_cost(self._h, i, C.byref(v))); return v.value

    def _dims(self, i: int):
        if not 0 <= i < len(self._problems):
            L.check(L.lib().mcf_batch_get_status(self._h, i, C.byref(C.c_int32())))      # raises the library's own error
        return self._problems[i]

    def flows(self, i: int) -> np.ndarray:
        m = self._dims(i)[1]
        out = np.empty(max(m, 1), np.int64); L.check(L.lib().mcf_batch_get_flows(self._h, i, out.ctypes.data)); return out[:m]

    def potentials(self, i: int) -> np.ndarray:
        n = self._dims(i)[0]
        out = np.empty(max(n, 1), np.int64); L.check(L.lib().mcf_batch_get_potentials(self._h, i, out.ctypes.data)); return out[:n]

    def pivots(self, i: int) -> int:
        v = C.c_int64(); L.check(L.lib().mcf_batch_get_pivots(self._h, i, C.byref(v))); return v.value

    def trace(self, i: int) -> np.ndarray:
        n = C.c_int64()
        L.check(L.lib().mcf_batch_get_trace(self._h, i, None, 0, C.byref(n)))
        out = np.empty(max(n.value, 1), np.int32)
        L.check(L.lib().mcf_batch_get_trace(self._h, i, out.ctypes.data, n.value, C.byref(n)))
        return out[: n.value]

    def stats(self) -> dict:
        st = L.BatchStats(); L.check(L.lib().mcf_batch_get_stats(self._h, C.byref(st))); return st.as_dict()


class UniformResult:
    """What UniformBatch.solve / .resolve return: one row per instance, numpy arrays or tensors like the inputs.  Rows of instances that
    are not Optimal are zero; trace rows are zero behind min(pivots, record_trace)."""
    __slots__ = ("status", "pivots", "total_cost", "flows", "potentials", "trace")
    FIELDS = (("status", "int32", ""), ("pivots", "int64", ""), ("total_cost", "int64", ""), ("flows", "int64", "m"), ("potentials", "int64", "n"),
              ("trace", "int32", "t"))

    def __init__(self, **arrays):
        for name, _, _ in self.FIELDS:
            setattr(self, name, arrays[name])


class UniformValidation:
    """What UniformBatch.validate returns: one row per instance, numpy arrays or tensors like the inputs.  errors[i, k] is the number of
    messages of kind k (VALIDATION_KINDS) the reference's SolutionValidator would add for instance i, first[i, k] the lowest arc / node id
    among them or -1; valid[i] = no message at all.  summary: the mcf_ubatch_check_summary of the call as a dict."""
    __slots__ = ("valid", "errors", "first", "objective", "dual_cost", "summary")
    FIELDS = (("valid", "int32", False), ("errors", "int32", True), ("first", "int32", True), ("objective", "int64", False), ("dual_cost", "int64", False))

    def __init__(self, summary, **arrays):
        self.summary = summary
        for name, _, _ in self.FIELDS:
            setattr(self, name, arrays[name])


def _is_tensor(a) -> bool:
    return type(a).__module__.split(".")[0] == "torch"


class RaggedResult(UniformResult):
    """What RaggedBatch.solve / .resolve return: UniformResult's fields with flows and potentials FLAT -- instance i's arcs are
    flows[arc_rows[i]:arc_rows[i + 1]], its nodes potentials[node_rows[i]:node_rows[i + 1]]; arcs(i) and nodes(i) return those slices
    (views, numpy or tensor like the arrays).  status, pivots and total_cost are [count], trace is [count, record_trace]."""
    __slots__ = ("arc_rows", "node_rows")

    def __init__(self, arc_rows, node_rows, **arrays):
        super().__init__(**arrays)
        self.arc_rows, self.node_rows = arc_rows, node_rows

    def arcs(self, i: int):
        return self.flows[int(self.arc_rows[i]):int(self.arc_rows[i + 1])]

    def nodes(self, i: int):
        return self.potentials[int(self.node_rows[i]):int(self.node_rows[i + 1])]


class UniformRanges:
    """What UniformBatch.cost_ranges returns: one row per instance, numpy arrays or tensors.  ranged[i] = instance i's last solve call left
    an optimal basis with every supply met exactly; for such an instance the kept basis stays optimal exactly while arc e's cost lies in
    [cost - cost_down[i, e], cost + cost_up[i, e]], every other cost fixed (RANGE_INF = no limit on that side), and arc_state[i, e] is the
    arc's place in the basis: 1 at its lower bound, 0 in the tree, -1 at its upper bound.  Rows of every other instance are zero.
    cost_down and cost_up are None where they were not asked for."""
    __slots__ = ("ranged", "arc_state", "cost_down", "cost_up")
    FIELDS = (("ranged", "int32", ""), ("arc_state", "int8", "m"), ("cost_down", "int64", "m"), ("cost_up", "int64", "m"))
    RANGE_INF = L.RANGE_INF

    def __init__(self, **arrays):
        for name, _, _ in self.FIELDS:
            setattr(self, name, arrays.get(name))


class RaggedRanges(UniformRanges):
    """What RaggedBatch.cost_ranges returns: UniformRanges' fields with the per-arc rows FLAT -- instance i's arcs are
    [arc_rows[i], arc_rows[i + 1]); arcs(i) returns (arc_state, cost_down, cost_up) of instance i as views."""
    __slots__ = ("arc_rows",)

    def __init__(self, arc_rows, **arrays):
        super().__init__(**arrays)
        self.arc_rows = arc_rows

    def arcs(self, i: int):
        lo, hi = int(self.arc_rows[i]), int(self.arc_rows[i + 1])
        return tuple(None if a is None else a[lo:hi] for a in (self.arc_state, self.cost_down, self.cost_up))


class UniformDataRanges:
    """What UniformBatch.data_ranges returns: one row per instance, numpy arrays or tensors.  ranged and arc_state as in UniformRanges.  For
    a ranged instance the kept basis stays primal feasible -- a resolve_data() that changes this one thing makes no pivot and does not
    fall back -- while arc e's flow, moved alone, falls by at most flow_down[i, e] or rises by at most flow_up[i, e] (a non-tree arc's are
    not clipped by its own capacity), and while d units of supply move from node b to node a of pair k (supply[a] + d, supply[b] - d)
    with d <= ship_forth[i, k], or the other way with d <= ship_back[i, k].  RANGE_INF = no limit; a pair (a, a) gives RANGE_INF twice, a
    pair with an id out of range -1 twice.  Rows of every other instance are zero.  Rows that were not asked for are None.
    bounds(lower, upper) turns the flow rows into the ranges of the bounds."""
    __slots__ = ("ranged", "arc_state", "flow_down", "flow_up", "ship_forth", "ship_back")
    FIELDS = (("ranged", "int32", ""), ("arc_state", "int8", "m"), ("flow_down", "int64", "m"), ("flow_up", "int64", "m"),
              ("ship_forth", "int64", "p"), ("ship_back", "int64", "p"))
    RANGE_INF = L.RANGE_INF

    def __init__(self, **arrays):
        for name, _, _ in self.FIELDS:
            setattr(self, name, arrays.get(name))

    def _ranged_per_arc(self, xp):
        return self.ranged[:, None] != 0

    def bounds(self, lower, upper):
        """(lower may fall by, lower may rise by, upper may fall by, upper may rise by): four rows shaped like flow_down, from the bounds
        the last solve call was given (lower None = 0, upper None or INF_CAP = uncapacitated; [m] rows are shared by all instances).

            arc_state | lower falls | lower rises            | upper falls              | upper rises
            LOWER  1  | flow_down   | min(flow_up, capacity) | capacity                 | RANGE_INF
            UPPER -1  | RANGE_INF   | capacity               | min(flow_down, capacity) | flow_up
            TREE   0  | RANGE_INF   | flow_down              | flow_up                  | RANGE_INF

        capacity = upper - lower.  RANGE_INF = no limit; for an uncapacitated arc it says in the upper columns that there is no finite
        upper bound to move.  Rows of instances that are not ranged are zero."""
        if self.flow_down is None or self.arc_state is None:
            raise ValueError("bounds() needs arc_state, flow_down and flow_up: data_ranges(flows=True)")
        down, up, state = self.flow_down, self.flow_up, self.arc_state
        tensors = _is_tensor(down)
        if tensors:
            import torch as xp
            as_rows = lambda a: a if _is_tensor(a) else xp.as_tensor(np.asarray(a, np.int64), device=down.device)
        else:
            xp = np
            as_rows = lambda a: np.asarray(a.cpu().numpy() if _is_tensor(a) else a, np.int64)
        inf = xp.full_like(down, L.RANGE_INF)
        zero = xp.zeros_like(down)
        lo = zero if lower is None else as_rows(lower) + zero
        hi = inf if upper is None else as_rows(upper) + zero
        cap = xp.where(hi == L.INF_CAP, inf, hi - xp.where(hi == L.INF_CAP, zero, lo))
        at_lower, at_upper = state == 1, state == -1
        rows = (xp.where(at_lower, down, inf),
                xp.where(at_lower, xp.minimum(up, cap), xp.where(at_upper, cap, down)),
                xp.where(at_lower, cap, xp.where(at_upper, xp.minimum(down, cap), up)),
                xp.where(at_upper, up, inf))
        ranged = self._ranged_per_arc(xp)
        return tuple(xp.where(ranged, r, zero) for r in rows)


class RaggedDataRanges(UniformDataRanges):
    """What RaggedBatch.data_ranges returns: UniformDataRanges' fields FLAT -- instance i's arcs are [arc_rows[i], arc_rows[i + 1]), its
    answers to its graph's pairs [ship_rows[i], ship_rows[i + 1]); arcs(i) returns (arc_state, flow_down, flow_up) and ships(i)
    (ship_forth, ship_back) of instance i as views."""
    __slots__ = ("arc_rows", "ship_rows")

    def __init__(self, arc_rows, ship_rows, **arrays):
        super().__init__(**arrays)
        self.arc_rows, self.ship_rows = arc_rows, ship_rows

    def arcs(self, i: int):
        lo, hi = int(self.arc_rows[i]), int(self.arc_rows[i + 1])
        return tuple(None if a is None else a[lo:hi] for a in (self.arc_state, self.flow_down, self.flow_up))

    def ships(self, i: int):
        lo, hi = int(self.ship_rows[i]), int(self.ship_rows[i + 1])
        return tuple(None if a is None else a[lo:hi] for a in (self.ship_forth, self.ship_back))

    def _ranged_per_arc(self, xp):
        counts = np.diff(self.arc_rows)
        if xp is np:
            return np.repeat(self.ranged != 0, counts)
        return xp.repeat_interleave(self.ranged != 0, xp.as_tensor(counts, device=self.ranged.device))


class UniformDiagnosis:
    """What UniformBatch.diagnose returns: one row per instance, numpy arrays or tensors.  verdict[i] is a Verdict.  Feasible: the flow the
    last solve call left satisfies every constraint, whatever status says.  Cut: the instance is infeasible and side[i] marks a node set S
    that proves it in the caller's numbers -- Geq: violation[i] = supply(S) - (upper(arcs leaving S) - lower(arcs entering S)) > 0;
    Leq: violation[i] = (lower(arcs leaving S) - upper(arcs entering S)) - supply(S) > 0 -- with set_size[i] nodes.  unmet[i, v] is what
    node v could not ship (Geq: > 0 violated, < 0 slack; Leq mirrored); violation is the sum of |unmet| over S.  Bounds: an upper bound
    below its lower bound.  NoVerdict: Unbounded, a limit, never solved.  Open: no certificate (never seen; counted in diagnose_stats()).
    Rows of Bounds and NoVerdict instances are zero.  side and unmet are None where they were not asked for."""
    __slots__ = ("verdict", "violation", "set_size", "side", "unmet")
    FIELDS = (("verdict", "int32", ""), ("violation", "int64", ""), ("set_size", "int32", ""), ("side", "int8", "n"), ("unmet", "int64", "n"))

    def __init__(self, **arrays):
        for name, _, _ in self.FIELDS:
            setattr(self, name, arrays.get(name))


class RaggedDiagnosis(UniformDiagnosis):
    """What RaggedBatch.diagnose returns: UniformDiagnosis' fields with the per-node rows FLAT -- instance i's nodes are
    [node_rows[i], node_rows[i + 1]); nodes(i) returns (side, unmet) of instance i as views."""
    __slots__ = ("node_rows",)

    def __init__(self, node_rows, **arrays):
        super().__init__(**arrays)
        self.node_rows = node_rows

    def nodes(self, i: int):
        lo, hi = int(self.node_rows[i]), int(self.node_rows[i + 1])
        return tuple(None if a is None else a[lo:hi] for a in (self.side, self.unmet))


class UniformRays:
    """What UniformBatch.rays returns: one row per instance, numpy arrays or tensors.  verdict[i] is a Ray.  Cycle: the instance holds a
    directed cycle of uncapacitated arcs (upper = INF_CAP) of total cost < 0 -- on_cycle[i] marks the arcs of one simple such cycle,
    cycle_cost[i] < 0 is their cost, cycle_length[i] their number -- so if it is feasible at all its objective is unbounded below, and
    whatever status says its cost and flows are no optimum.  Bounded: there is none, and label[i] proves it: label[target] <=
    label[source] + cost on every uncapacitated arc.  Bounds: an upper bound below its lower bound.  NoVerdict: never solved.  Rows that
    a verdict does not fill are zero.  on_cycle and label are None where they were not asked for."""
    __slots__ = ("verdict", "cycle_cost", "cycle_length", "on_cycle", "label")
    FIELDS = (("verdict", "int32", ""), ("cycle_cost", "int64", ""), ("cycle_length", "int32", ""), ("on_cycle", "int8", "m"), ("label", "int64", "n"))

    def __init__(self, **arrays):
        for name, _, _ in self.FIELDS:
            setattr(self, name, arrays.get(name))


class RaggedRays(UniformRays):
    """What RaggedBatch.rays returns: UniformRays' fields with the per-arc and per-node rows FLAT -- instance i's arcs are
    [arc_rows[i], arc_rows[i + 1]), its nodes [node_rows[i], node_rows[i + 1]); arcs(i) returns on_cycle and nodes(i) label of
    instance i as views."""
    __slots__ = ("arc_rows", "node_rows")

    def __init__(self, arc_rows, node_rows, **arrays):
        super().__init__(**arrays)
        self.arc_rows, self.node_rows = arc_rows, node_rows

    def arcs(self, i: int):
        return None if self.on_cycle is None else self.on_cycle[int(self.arc_rows[i]):int(self.arc_rows[i + 1])]

    def nodes(self, i: int):
        return None if self.label is None else self.label[int(self.node_rows[i]):int(self.node_rows[i + 1])]


class _PlacedBatch:
    """What UniformBatch and RaggedBatch share: the checks of every array of a call, the calls and their results.  A subclass has the
    constructor (which sets _h, _last = None, count, device, record_trace) and says what differs:
      _PREFIX            the library's functions are <_PREFIX>_solve, _resolve, ...
      _IO, _CHECK_IO     the ctypes structs of a solve call and of a validation call
      _RANGE_IO          the ctypes struct of a cost-ranges call; _ranges(out) makes its result
      _BASIS_IO          the ctypes struct that carries a given basis into solve_from()
      _DIAGNOSE_IO       the ctypes struct of a diagnose call; _diagnosis(out) makes its result
      _RAYS_IO           the ctypes struct of a rays call; _rays_result(out) makes its result
      _RESULT            the result class; _result(out) makes one
      _sizes()           the shapes of the outputs by UniformResult.FIELDS' dimension key
      _stride(...)       the expected shape of the array of a given name, its contiguity, and the stride it is passed with"""

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self._fn("destroy")(h)
            self._h = None

    def __len__(self):
        return self.count

    def _fn(self, name):
        return getattr(L.lib(), f"{self._PREFIX}_{name}")

    def _result(self, out):
        return self._RESULT(**out)

    # ---- one input: (pointer, stride in elements, the object that keeps the memory alive)
    def _input(self, a, name, tensors, dtype="int64"):
        if a is None:
            return None, 0, None
        if tensors:
            import torch
            if not _is_tensor(a):
                raise ValueError(f"{name}: numpy arrays and tensors cannot be mixed in one call")
            if a.device.type != "cuda" or (a.device.index or 0) != self.device:
                raise ValueError(f"{name}: tensor on {a.device}, the batch runs on cuda:{self.device}")
            if a.dtype != getattr(torch, dtype):
                raise ValueError(f"{name}: dtype {a.dtype}, expected {dtype}")
            shape, strides = tuple(a.shape), tuple(a.stride())
        else:
            if _is_tensor(a):
                raise ValueError(f"{name}: numpy arrays and tensors cannot be mixed in one call")
            if not isinstance(a, np.ndarray):
                a = np.asarray(a, dtype)
            if a.dtype != np.dtype(dtype):
                raise ValueError(f"{name}: dtype {a.dtype}, expected {dtype}")
            shape, strides = tuple(a.shape), tuple(s // a.itemsize for s in a.strides)
        stride = self._stride(name, shape, strides)
        return (a.data_ptr() if tensors else a.ctypes.data), int(stride), a

    def _problem(self, io, arrays, tensors, keep):
        """cost, supply, lower, upper into io"""
        io.memory = L.MEM_DEVICE if tensors else L.MEM_HOST
        for name, a in zip(("cost", "supply", "lower", "upper"), arrays):
            ptr, stride, obj = self._input(a, name, tensors)
            keep.append(obj)
            setattr(io, name, ptr)
            if hasattr(io, name + "_stride"):
                setattr(io, name + "_stride", stride)

    def _empty(self, shape, dtype, tensors):
        if tensors:
            import torch
            return torch.empty(shape, dtype=getattr(torch, dtype), device=f"cuda:{self.device}")
        return np.empty(shape, dtype)

    def _outputs(self, tensors, like):
        """Fresh rows, or copies of `like` (the last result) for a call that does not write every row."""
        sizes = self._sizes()
        out = {}
        for name, dtype, dim in UniformResult.FIELDS:
            if like is not None:
                prev = getattr(like, name)
                if _is_tensor(prev) != tensors:
                    raise ValueError("a masked resolve() continues the last result: numpy arrays and tensors cannot be mixed")
                out[name] = prev.clone() if tensors else prev.copy()
            else:
                out[name] = self._empty(sizes[dim], dtype, tensors)
        return out

    def _call(self, fn, cost, supply, lower, upper, supply_type, changed=None, masked=False, numpy_only=False, arc_state=None):
        given = [a for a in (cost, supply, lower, upper, changed, arc_state) if a is not None]
        tensors = any(_is_tensor(a) for a in given)
        if tensors and numpy_only:
            raise ValueError("the host hooks take numpy arrays")
        keep = []
        io = self._IO()
        io.supply_type = int(supply_type)
        self._problem(io, (cost, supply, lower, upper), tensors, keep)
        if changed is not None:
            if not tensors and not isinstance(changed, np.ndarray):
                changed = np.asarray(changed)
            if not tensors and changed.dtype == np.bool_:
                changed = changed.view(np.uint8)
            if tensors:
                import torch
                if changed.dtype == torch.bool:
                    changed = changed.view(torch.uint8)
            ptr, _, obj = self._input(changed, "changed", tensors, dtype="uint8")
            keep.append(obj)
            io.changed = ptr
        if masked and changed is not None and self._last is None:
            raise McfError(L.ERR_STATE, "resolve: the batch has not been solved")
        out = self._outputs(tensors, self._last if masked and changed is not None else None)
        for name, arr in out.items():
            setattr(io, name, arr.data_ptr() if tensors else arr.ctypes.data)
        extra = []
        if arc_state is not None:           # a solve from a given basis: the row(s) of arc states, checked like every other array
            basis = self._BASIS_IO()
            basis.memory = io.memory
            ptr, stride, obj = self._input(arc_state, "arc_state", tensors, dtype="int8")
            keep.append(obj)
            basis.arc_state = ptr
            if hasattr(basis, "state_stride"):
                basis.state_stride = stride
            extra.append(C.byref(basis))
        L.check(self._fn(fn)(self._h, C.byref(io), *extra))
        self._last = self._result(out)
        return self._last

    def solve(self, cost, supply, lower=None, upper=None, supply_type=SupplyType.Geq) -> UniformResult:
        """A fresh solve of every instance; may be repeated with other supplies, bounds or costs."""
        return self._call("solve", cost, supply, lower, upper, supply_type)

    def resolve(self, cost, supply, lower=None, upper=None, supply_type=SupplyType.Geq, changed=None) -> UniformResult:
        """New costs for the instances `changed` marks ([count] bool / uint8, None = all): each goes on from the basis its last solve left
        where that ended Optimal.  supply, lower, upper and supply_type must be what the last solve() was given.  Rows of unmarked
        instances are the last result's."""
        return self._call("resolve", cost, supply, lower, upper, supply_type, changed, masked=True)

    def run_on_host(self, cost, supply, lower=None, upper=None, supply_type=SupplyType.Geq) -> UniformResult:
        """Test hook: solve() with one lane on the CPU.  numpy only."""
        return self._call("run_on_host", cost, supply, lower, upper, supply_type, numpy_only=True)

    def rerun_on_host(self, cost, supply, lower=None, upper=None, supply_type=SupplyType.Geq, changed=None) -> UniformResult:
        """Test hook: resolve() with one lane on the CPU.  numpy only."""
        return self._call("rerun_on_host", cost, supply, lower, upper, supply_type, changed, masked=True, numpy_only=True)

    def resolve_data(self, cost, supply, lower=None, upper=None, supply_type=SupplyType.Geq, changed=None) -> UniformResult:
        """New supplies and bounds for the instances `changed` marks ([count] bool / uint8, None = all): each goes on from the basis its
        last solve left, by dual pivots, where that ended Optimal and the new supplies sum to zero; every other one, and every warm attempt
        that does not hold, is solved again from the start in the same call.  cost and supply_type must be what the last solve call was
        given.  Rows of unmarked instances are the last result's."""
        return self._call("resolve_data", cost, supply, lower, upper, supply_type, changed, masked=True)

    def rerun_data_on_host(self, cost, supply, lower=None, upper=None, supply_type=SupplyType.Geq, changed=None) -> UniformResult:
        """Test hook: resolve_data() with one lane on the CPU.  numpy only."""
        return self._call("rerun_data_on_host", cost, supply, lower, upper, supply_type, changed, masked=True, numpy_only=True)

    def solve_from(self, arc_state, cost, supply, lower=None, upper=None, supply_type=SupplyType.Geq) -> UniformResult:
        """A solve of every instance that starts from the basis in arc_state instead of from the start basis: int8, one state per arc
        (1 lower bound, 0 tree, -1 upper bound) as cost_ranges() returns it -- from this handle or another, of either kind, on the same
        graph.  UniformBatch: [arc_count] (one row for the whole batch) or [count, arc_count]; RaggedBatch: flat, arc_rows[-1] long.
        numpy or tensors like the other arrays.  A row that is no basis the pivots can go on from (a cycle among its tree arcs, supplies
        its components do not balance, ...) is solved from the start basis, bit for bit a solve(); every answer is a fresh solve's.
        Allowed on a handle that has never solved; afterwards resolve(), resolve_data(), cost_ranges() and validate() go on from it."""
        if arc_state is None:
            raise ValueError("arc_state: a basis is required (int8, one state per arc)")
        return self._call("solve_from", cost, supply, lower, upper, supply_type, arc_state=arc_state)

    def run_from_on_host(self, arc_state, cost, supply, lower=None, upper=None, supply_type=SupplyType.Geq) -> UniformResult:
        """Test hook: solve_from() with one lane on the CPU.  numpy only."""
        if arc_state is None:
            raise ValueError("arc_state: a basis is required (int8, one state per arc)")
        return self._call("run_from_on_host", cost, supply, lower, upper, supply_type, numpy_only=True, arc_state=arc_state)

    def _stats(self, fn, struct) -> dict:
        st = struct(); L.check(self._fn(fn)(self._h, C.byref(st))); return st.as_dict()

    def start_stats(self) -> dict:
        """What the last solve_from() / run_from_on_host() did: primal starts, dual starts, instances cold by rule, fallbacks, dual and
        primal pivots."""
        return self._stats("get_start_stats", L.UBatchStartStats)

    def stats(self) -> dict:
        return self._stats("get_stats", L.UBatchStats)

    def resolve_data_stats(self) -> dict:
        """What the last resolve_data() / rerun_data_on_host() did: warm, cold, fallback and untouched instances, dual and primal pivots."""
        return self._stats("get_redata_stats", L.UBatchRedataStats)

    # ---- the queries of the kept state
    def _like_last(self, tensors):
        return self._last is not None and _is_tensor(self._last.status) if tensors is None else tensors

    def _query(self, fn, io, fields, skip, sizes, result, tensors):
        """Fresh rows for every field of `fields` that skip(name, dim) does not leave out, the call, result(rows)"""
        tensors = self._like_last(tensors)
        io.memory = L.MEM_DEVICE if tensors else L.MEM_HOST
        out = {}
        for name, dtype, dim in fields:
            if skip(name, dim):
                continue
            out[name] = self._empty(sizes[dim], dtype, tensors)
            setattr(io, name, out[name].data_ptr() if tensors else out[name].ctypes.data)
        L.check(self._fn(fn)(self._h, C.byref(io)))
        return result(out)

    # ---- cost ranges of the kept basis
    def _ranges(self, out):
        return UniformRanges(**out)

    def _cost_ranges(self, fn, tensors, costs):
        return self._query(fn, self._RANGE_IO(), UniformRanges.FIELDS, lambda name, dim: not costs and name in ("cost_down", "cost_up"),
                           self._sizes(), self._ranges, tensors)

    def cost_ranges(self, tensors=None, costs=True):
        """Post-optimality cost ranging of the basis every instance's last solve call left, on the device: a UniformRanges /
        RaggedRanges.  tensors: True = tensors on the handle's device (nothing that scales with the batch crosses the bus), False = numpy
        arrays, None = like the last result.  costs=False leaves cost_down and cost_up out (ranged and arc_state only: no cycle is
        walked).  The kept state is read, never changed: solve calls and this one mix in any order."""
        return self._cost_ranges("cost_ranges", tensors, costs)

    def cost_ranges_on_host(self, costs=True):
        """Test hook: cost_ranges() with one lane on the CPU.  numpy only."""
        return self._cost_ranges("cost_ranges_on_host", False, costs)

    def range_stats(self) -> dict:
        """What the last cost_ranges() / cost_ranges_on_host() did: instances, ranged ones, tiers, tree arcs ranged, cycle hops, kernel time."""
        return self._stats("get_range_stats", L.UBatchRangeStats)

    # ---- supply and bound ranges of the kept basis
    def _pair_array(self, pairs, tensors, name="pairs"):
        """[k, 2] int32 node ids where the call's arrays lie"""
        if tensors:
            import torch
            if not _is_tensor(pairs):
                pairs = torch.as_tensor(np.ascontiguousarray(np.asarray(pairs, np.int32).reshape(-1, 2)), device=f"cuda:{self.device}")
            if pairs.device.type != "cuda" or (pairs.device.index or 0) != self.device:
                raise ValueError(f"{name}: tensor on {pairs.device}, the batch runs on cuda:{self.device}")
            if pairs.dtype != torch.int32:
                raise ValueError(f"{name}: dtype {pairs.dtype}, expected int32")
            if pairs.dim() != 2 or pairs.shape[1] != 2:
                raise ValueError(f"{name}: shape {tuple(pairs.shape)}, expected (pairs, 2)")
            return pairs.contiguous()
        if _is_tensor(pairs):
            raise ValueError(f"{name}: numpy arrays and tensors cannot be mixed in one call")
        a = np.asarray(pairs)
        if a.size == 0:
            a = np.zeros((0, 2), np.int32)
        if a.dtype.kind not in "iu" or a.ndim != 2 or a.shape[1] != 2:
            raise ValueError(f"{name}: expected integer node ids of shape (pairs, 2), got {a.dtype} {a.shape}")
        if a.size and (a.min() < np.iinfo(np.int32).min or a.max() > np.iinfo(np.int32).max):
            raise ValueError(f"{name}: node ids outside int32")
        return np.ascontiguousarray(a, np.int32)

    def _data_ranges(self, fn, pairs, tensors, flows):
        tensors = self._like_last(tensors)
        io = self._DATA_RANGE_IO()
        keep = []
        ships, ship_rows = self._pairs_into(io, pairs, tensors, keep)           # the shape of the ship rows (None: no pairs)
        return self._query(fn, io, UniformDataRanges.FIELDS,
                           lambda name, dim: (not flows and name in ("flow_down", "flow_up")) or (ships is None and dim == "p"),
                           dict(self._sizes(), p=ships), lambda out: self._data_range_result(out, ship_rows), tensors)

    def data_ranges(self, pairs=None, tensors=None, flows=True):
        """Right-hand-side ranging of the basis every instance's last solve call left, on the device: a UniformDataRanges /
        RaggedDataRanges.  pairs: node pairs (a, b) to ask the supply ranges of -- UniformBatch: one [k, 2] list for every instance;
        RaggedBatch: one such list per graph.  tensors: True = tensors on the handle's device (nothing that scales with the batch crosses
        the bus; pairs given as a tensor are read where they lie), False = numpy arrays, None = like the last result.  flows=False leaves
        flow_down and flow_up out.  Ask before a resolve_data(): a change inside the range is answered from the kept basis with no
        pivot.  The kept state is read, never changed: solve calls and this one mix in any order."""
        return self._data_ranges("data_ranges", pairs, tensors, flows)

    def data_ranges_on_host(self, pairs=None, flows=True):
        """Test hook: data_ranges() with one lane on the CPU.  numpy only."""
        return self._data_ranges("data_ranges_on_host", pairs, False, flows)

    def data_range_stats(self) -> dict:
        """What the last data_ranges() / data_ranges_on_host() did: instances, ranged ones, tiers, walks, hops, kernel time."""
        return self._stats("get_data_range_stats", L.UBatchDataRangeStats)

    # ---- why infeasible: a cut from the kept flow
    def _diagnosis(self, out):
        return UniformDiagnosis(**out)

    def _diagnose(self, fn, tensors, nodes):
        return self._query(fn, self._DIAGNOSE_IO(), UniformDiagnosis.FIELDS, lambda name, dim: not nodes and dim == "n", self._sizes(), self._diagnosis, tensors)

    def diagnose(self, tensors=None, nodes=True):
        """Whether the flow every instance's last solve call left satisfies its constraints and, where it does not, a cut that proves the
        instance infeasible, on the device: a UniformDiagnosis / RaggedDiagnosis.  tensors: True = tensors on the handle's device (nothing
        that scales with the batch crosses the bus), False = numpy arrays, None = like the last result.  nodes=False leaves side and unmet
        out (the walk still runs: the verdict needs it).  The kept state is read, never changed: solve calls, range calls and this one mix
        in any order."""
        return self._diagnose("diagnose", tensors, nodes)

    def diagnose_on_host(self, nodes=True):
        """Test hook: diagnose() with one lane on the CPU.  numpy only."""
        return self._diagnose("diagnose_on_host", False, nodes)

    def diagnose_stats(self) -> dict:
        """What the last diagnose() / diagnose_on_host() did: instances per verdict, tiers, levels, frontier nodes, incidence entries, kernel time."""
        return self._stats("get_diagnose_stats", L.UBatchDiagnoseStats)

    # ---- unbounded or not: a negative cycle or labels from the kept data
    def _rays_result(self, out):
        return UniformRays(**out)

    def _rays(self, fn, tensors, arcs, labels):
        return self._query(fn, self._RAYS_IO(), UniformRays.FIELDS, lambda name, dim: (not arcs and dim == "m") or (not labels and dim == "n"), self._sizes(),
                           self._rays_result, tensors)

    def rays(self, tensors=None, arcs=True, labels=True):
        """Whether every instance's objective is bounded below, from the costs and capacities its last solve call left, on the device: a
        UniformRays / RaggedRays with a negative cycle of uncapacitated arcs where it is not and node labels that prove there is none
        where it is.  The solver mirrors the reference, which answers such a cycle Optimal with a cost that wraps: this is the guard.
        tensors: True = tensors on the handle's device (nothing that scales with the batch crosses the bus), False = numpy arrays, None =
        like the last result.  arcs=False leaves on_cycle out, labels=False label (the verdict, cycle_cost and cycle_length come all the
        same).  The kept state is read, never changed: solve calls, range calls, diagnose() and this one mix in any order."""
        return self._rays("rays", tensors, arcs, labels)

    def rays_on_host(self, arcs=True, labels=True):
        """Test hook: rays() with one lane on the CPU.  numpy only."""
        return self._rays("rays_on_host", False, arcs, labels)

    def ray_stats(self) -> dict:
        """What the last rays() / rays_on_host() did: instances per verdict, tiers, rounds, frontier nodes, incidence entries, cycle arcs, kernel time."""
        return self._stats("get_rays_stats", L.UBatchRaysStats)

    # ---- validation: the solution's rows where they lie
    SOLUTION_ROWS = (("status", "int32", None), ("total_cost", "int64", None), ("flows", "int64", "arc_count"), ("potentials", "int64", "node_count"))

    def _validate(self, fn, rows, cost, supply, lower, upper, supply_type, numpy_only=False):
        if isinstance(rows, dict):
            rows = tuple(rows[name] for name, _, _ in self.SOLUTION_ROWS)
        elif hasattr(rows, "status"):
            rows = tuple(getattr(rows, name) for name, _, _ in self.SOLUTION_ROWS)
        rows = tuple(rows)
        if len(rows) != 4 or any(r is None for r in rows):
            raise ValueError(f"the solution to check is status, total_cost, flows and potentials: a {self._RESULT.__name__}, a dict or the four rows")
        tensors = any(_is_tensor(a) for a in (*rows, cost, supply, lower, upper) if a is not None)
        if tensors and numpy_only:
            raise ValueError("the host hooks take numpy arrays")
        keep = []
        io = self._CHECK_IO()
        io.supply_type = int(supply_type)
        self._problem(io, (cost, supply, lower, upper), tensors, keep)
        for (name, dtype, _), a in zip(self.SOLUTION_ROWS, rows):
            ptr, _, obj = self._input(a, name, tensors, dtype=dtype)
            keep.append(obj)
            setattr(io, name, ptr)
        out = {}
        for name, dtype, per_kind in UniformValidation.FIELDS:
            out[name] = self._empty((self.count, len(L.VALIDATION_KINDS)) if per_kind else (self.count,), dtype, tensors)
            setattr(io, name, out[name].data_ptr() if tensors else out[name].ctypes.data)
        summary = L.UBatchCheckSummary()
        L.check(self._fn(fn)(self._h, C.byref(io), C.byref(summary)))
        return UniformValidation(summary.as_dict(), **out)

    def validate(self, result_or_rows, cost, supply, lower=None, upper=None, supply_type=SupplyType.Geq) -> UniformValidation:
        """The reference's SolutionValidator for every instance in one launch, each against its own graph.  result_or_rows: a result of
        solve(), or status, total_cost, flows and potentials as a dict or in that order -- any solution of these graphs, not only this
        handle's.  Arrays as solve() takes them; with tensors nothing that scales with the graphs or the batch crosses the bus.
        supply_type may also be 2 (equality)."""
        return self._validate("validate", result_or_rows, cost, supply, lower, upper, supply_type)

    def validate_on_host(self, result_or_rows, cost, supply, lower=None, upper=None, supply_type=SupplyType.Geq) -> UniformValidation:
        """Test hook: validate() with one lane on the CPU.  numpy only."""
        return self._validate("validate_on_host", result_or_rows, cost, supply, lower, upper, supply_type, numpy_only=True)


class UniformBatch(_PlacedBatch):
    """`count` instances of ONE graph, solved on the device from arrays that already are there (mcf_ubatch_*, DESIGN.md 3.14 "Uniform
    batch").  solve() and resolve() take either numpy arrays (copied up and down, one copy per array) or torch tensors on the handle's
    device (read and written in place: nothing that scales with the graph crosses the bus) -- never a mix; each array is [count, m]
    ([count, n] for supply) or [m] ([n]) for one row shared by all, int64, contiguous in its last dimension.  Results equal
    BatchSolver's for the same instances bit for bit.  run_on_host() / rerun_on_host() are test hooks (numpy only)."""
    _PREFIX, _IO, _CHECK_IO, _RESULT, _RANGE_IO, _BASIS_IO = "mcf_ubatch", L.UBatchIo, L.UBatchCheckIo, UniformResult, L.UBatchRangeIo, L.UBatchBasisIo
    _ROW = {"cost": "arc_count", "lower": "arc_count", "upper": "arc_count", "flows": "arc_count", "supply": "node_count", "potentials": "node_count",
            "arc_state": "arc_count"}

    def __init__(self, node_count, source, target, count, rule=PivotRule.BlockSearch, pivot_limit=0, record_trace=0, device=0, pivots_per_launch=0,
                 semantics=L.SEM_PLAIN, flags=0):
        src, tgt = _i32(source), _i32(target)
        if src.ndim != 1 or src.shape != tgt.shape:
            raise ValueError("source and target must be one-dimensional and of equal length")
        self.node_count, self.arc_count, self.count, self.device, self.record_trace = int(node_count), int(src.shape[0]), int(count), int(device), int(record_trace)
        self._h = C.c_void_p()
        self._last = None               # the last UniformResult: a masked resolve() starts from its rows
        d = L.UBatchDesc(self.device, int(rule), int(semantics), 0, int(pivot_limit), int(pivots_per_launch), self.record_trace, int(flags),
                         self.node_count, self.arc_count, self.count, src.ctypes.data, tgt.ctypes.data)
        L.check(L.lib().mcf_ubatch_create(C.byref(self._h), C.byref(d)))

    _DATA_RANGE_IO = L.UBatchDataRangeIo
    _DIAGNOSE_IO = L.UBatchDiagnoseIo
    _RAYS_IO = L.UBatchRaysIo

    def _pairs_into(self, io, pairs, tensors, keep):
        """one list for every instance: ship rows [count, k]"""
        if pairs is None:
            return None, None
        a = self._pair_array(pairs, tensors)
        if a.shape[0] == 0:
            return None, None
        keep.append(a)
        io.pair_count = int(a.shape[0])
        io.pairs = a.data_ptr() if tensors else a.ctypes.data
        return (self.count, int(a.shape[0])), None

    def _data_range_result(self, out, ship_rows):
        return UniformDataRanges(**out)

    def _sizes(self):
        return {"": (self.count,), "m": (self.count, self.arc_count), "n": (self.count, self.node_count), "t": (self.count, self.record_trace)}

    def _stride(self, name, shape, strides):
        """cost, lower, upper, supply: one row per instance or one row shared by all; the solution's flows and potentials: dense rows;
        everything else: one entry per instance"""
        row = self._ROW.get(name)
        length = self.count if row is None else getattr(self, row)
        if row is None:
            if shape != (length,):
                raise ValueError(f"{name}: shape {shape}, expected ({length},)")
        elif shape not in ((length,), (self.count, length)):
            raise ValueError(f"{name}: shape {shape}, expected ({length},) or ({self.count}, {length})")
        if self.count > 0 and shape[-1] > 1 and strides[-1] != 1:
            raise ValueError(f"{name}: not contiguous in its last dimension")
        stride = strides[0] if len(shape) == 2 and self.count > 1 else 0
        if stride < 0 or (len(shape) == 2 and self.count > 1 and 0 < stride < length):
            raise ValueError(f"{name}: rows overlap")
        if name in ("flows", "potentials") and (len(shape) != 2 or (self.count > 1 and stride != length)):
            raise ValueError(f"{name}: expected dense rows of shape ({self.count}, {length})")
        return stride


class RaggedBatch(_PlacedBatch):
    """Instances of a SET of graphs in one handle, solved on the device from arrays that already are there (mcf_rbatch_*, DESIGN.md 3.14
    "Ragged batch").  graphs: a sequence of (node_count, source, target); graph_of[i] names the graph of instance i (None: instance i is
    graph i).  Problem data and results are flat: cost, lower, upper and flows have arc_rows[-1] elements, instance i's at
    [arc_rows[i], arc_rows[i + 1]); supply and potentials have node_rows[-1], likewise.  Calls take either flat numpy arrays (copied up
    and down) or flat torch tensors on the handle's device (read and written in place) -- never a mix; int64, contiguous.  Results equal
    BatchSolver's for the same instances bit for bit, and UniformBatch's where there is one graph.  run_on_host() / rerun_on_host() /
    validate_on_host() are test hooks (numpy only)."""
    _PREFIX, _IO, _CHECK_IO, _RESULT, _RANGE_IO, _BASIS_IO = "mcf_rbatch", L.RBatchIo, L.RBatchCheckIo, RaggedResult, L.RBatchRangeIo, L.RBatchBasisIo
    _ROW = {"cost": "arc_total", "lower": "arc_total", "upper": "arc_total", "flows": "arc_total", "supply": "node_total", "potentials": "node_total",
            "arc_state": "arc_total"}

    def __init__(self, graphs, graph_of=None, rule=PivotRule.BlockSearch, pivot_limit=0, record_trace=0, device=0, pivots_per_launch=0,
                 semantics=L.SEM_PLAIN, flags=0):
        graphs = [(int(n), _i32(src), _i32(tgt)) for n, src, tgt in graphs]
        for _, src, tgt in graphs:
            if src.ndim != 1 or src.shape != tgt.shape:
                raise ValueError("source and target must be one-dimensional and of equal length")
        self.graph_count, self.device, self.record_trace = len(graphs), int(device), int(record_trace)
        node_count = np.array([n for n, _, _ in graphs], np.int32)
        arc_start = np.zeros(self.graph_count + 1, np.int64)
        np.cumsum([len(src) for _, src, _ in graphs], out=arc_start[1:])
        source = np.concatenate([src for _, src, _ in graphs]) if graphs else np.zeros(0, np.int32)
        target = np.concatenate([tgt for _, _, tgt in graphs]) if graphs else np.zeros(0, np.int32)
        of = None if graph_of is None else _i32(graph_of)
        if of is not None and of.ndim != 1:
            raise ValueError("graph_of must be one-dimensional")
        self.count = self.graph_count if of is None else int(of.shape[0])
        self._graph_of = np.arange(self.graph_count) if of is None else of.astype(np.int64)
        self._h = C.c_void_p()
        self._last = None               # the last RaggedResult: a masked resolve() starts from its rows
        d = L.RBatchDesc(self.device, int(rule), int(semantics), 0, int(pivot_limit), int(pivots_per_launch), self.record_trace, int(flags),
                         self.graph_count, self.count, node_count.ctypes.data, arc_start.ctypes.data, source.ctypes.data, target.ctypes.data,
                         None if of is None else of.ctypes.data)
        L.check(L.lib().mcf_rbatch_create(C.byref(self._h), C.byref(d)))
        self.arc_rows, self.node_rows = np.zeros(self.count + 1, np.int64), np.zeros(self.count + 1, np.int64)
        L.check(L.lib().mcf_rbatch_get_rows(self._h, self.arc_rows.ctypes.data, self.node_rows.ctypes.data))
        self.arc_total, self.node_total = int(self.arc_rows[-1]), int(self.node_rows[-1])

    def _result(self, out):
        return RaggedResult(self.arc_rows, self.node_rows, **out)

    def _ranges(self, out):
        return RaggedRanges(self.arc_rows, **out)

    _DATA_RANGE_IO = L.RBatchDataRangeIo
    _DIAGNOSE_IO = L.RBatchDiagnoseIo
    _RAYS_IO = L.RBatchRaysIo

    def _rays_result(self, out):
        return RaggedRays(self.arc_rows, self.node_rows, **out)

    def _diagnosis(self, out):
        return RaggedDiagnosis(self.node_rows, **out)

    def _pairs_into(self, io, pairs, tensors, keep):
        """one list per graph, flat, with pair_row (where each graph's begins) and ship_row (where each instance's answers do); the two
        tables are built here and, for a call on tensors, kept on the device while the lists' lengths stay the same"""
        if pairs is None:
            return None, None
        pairs = list(pairs)
        if len(pairs) != self.graph_count:
            raise ValueError(f"pairs: {len(pairs)} lists, the batch has {self.graph_count} graphs (one list per graph)")
        lists = [self._pair_array(p, tensors, f"pairs[{g}]") for g, p in enumerate(pairs)]
        lengths = tuple(int(a.shape[0]) for a in lists)
        if sum(lengths) == 0:
            return None, None
        key = (lengths, bool(tensors))
        if getattr(self, "_pair_tables", (None,))[0] != key:
            pair_row = np.zeros(self.graph_count + 1, np.int64)
            np.cumsum(lengths, out=pair_row[1:])
            ship_rows = np.zeros(self.count + 1, np.int64)
            np.cumsum(np.asarray(lengths, np.int64)[self._graph_of], out=ship_rows[1:])
            tables = (pair_row, ship_rows)
            if tensors:
                import torch
                tables = tuple(torch.as_tensor(t, device=f"cuda:{self.device}") for t in tables)
            self._pair_tables = (key, tables, ship_rows)
        _, tables, ship_rows = self._pair_tables
        if tensors:
            import torch
            flat = torch.cat(lists).contiguous()
        else:
            flat = np.ascontiguousarray(np.concatenate(lists))
        keep.extend((flat,) + tuple(tables))
        ptr = (lambda a: a.data_ptr()) if tensors else (lambda a: a.ctypes.data)
        io.pairs, io.pair_row, io.ship_row = ptr(flat), ptr(tables[0]), ptr(tables[1])
        return (int(ship_rows[-1]),), ship_rows

    def _data_range_result(self, out, ship_rows):
        return RaggedDataRanges(self.arc_rows, ship_rows if ship_rows is not None else np.zeros(self.count + 1, np.int64), **out)

    def _sizes(self):
        return {"": (self.count,), "m": (self.arc_total,), "n": (self.node_total,), "t": (self.count, self.record_trace)}

    def _stride(self, name, shape, strides):
        """every array is flat: all instances' arcs, all instances' nodes, or one entry per instance; there are no strides"""
        row = self._ROW.get(name)
        length = self.count if row is None else getattr(self, row)
        if shape != (length,):
            raise ValueError(f"{name}: shape {shape}, expected ({length},)")
        if length > 1 and strides[-1] != 1:
            raise ValueError(f"{name}: not contiguous")
        return 0



def block_config(**kw) -> "L.BlockConfig":
    """new OptimizationConfig { ... } (OptimizationTypes.cs:24-38): the defaults, with the given fields replaced."""
    c = L.BlockConfig()
    L.lib().mcf_block_config_default(C.byref(c))
    for k, v in kw.items():
        if not hasattr(c, k):
            raise AttributeError(k)
        setattr(c, k, v)
    return c


def auto_block_config(node_count: int, source, target) -> "L.BlockConfig":
    """What the reference's auto-configuration picks for this graph (ProblemAnalyzer + OptimizationSelector)."""
    c = L.BlockConfig()
    src, tgt = _i32(source), _i32(target)
    L.check(L.lib().mcf_block_config_auto(C.byref(c), node_count, src.shape[0], src, tgt))
    return c


class SolutionValidator:
    """The reference's SolutionValidator checks as device reductions (mcf_validator_* of include/mcf_hip.h)."""

    def __init__(self, node_count: int, arc_count: int, device: int = 0):
        self.node_count, self.arc_count = int(node_count), int(arc_count)
        self._h = C.c_void_p()
        L.check(L.lib().mcf_validator_create(C.byref(self._h), device, self.node_count, self.arc_count))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            L.lib().mcf_validator_destroy(h)
            self._h = None

    def _ptrs(self, arrays, kinds, lengths):
        keep, out = [], []
        for a, dt, k in zip(arrays, kinds, lengths):
            if a is None:
                out.append(None)
                continue
            a = np.ascontiguousarray(a, dt)
            if a.shape != (k,):
                raise ValueError(f"expected an array of {k} entries, got {a.shape}")
            keep.append(a)
            out.append(a.ctypes.data_as(C.c_void_p))
        return keep, out

    def upload_network(self, source, target, lower, upper, cost, supply):
        m, n = self.arc_count, self.node_count
        keep, p = self._ptrs((source, target, lower, upper, cost, supply), (np.int32, np.int32, np.int64, np.int64, np.int64, np.int64), (m, m, m, m, m, n))
        L.check(L.lib().mcf_validator_upload(self._h, *p, None, None))
        return self

    def upload_solution(self, flow, pi):
        keep, p = self._ptrs((flow, pi), (np.int64, np.int64), (self.arc_count, self.node_count))
        L.check(L.lib().mcf_validator_upload(self._h, None, None, None, None, None, None, *p))
        return self

    def run(self, supply_type: int, reported_cost: int) -> dict:
        v = L.Validation(); L.check(L.lib().mcf_validator_run(self._h, int(supply_type), int(reported_cost), C.byref(v))); return v.as_dict()


class PivotEngine:
    """Device-resident SoA + pivot rules (mcf_engine_* of include/mcf_hip.h)."""

    def __init__(self, node_count: int, arc_capacity: int, search_arc_num: int, rule=PivotRule.BlockSearch,
                 optimized=True, int_width=64, block_size=0, device=0, shard=(0, 0), scan_workgroups=0, flags=0, resident_workgroups=0, vector_width=4):
        d = L.EngineDesc(node_count, arc_capacity, search_arc_num, int_width, rule, L.SEM_OPTIMIZED if optimized else L.SEM_PLAIN,
                         block_size, device, shard[0], shard[1], scan_workgroups, flags, resident_workgroups, _vector_width_abi(vector_width))
        self._h = C.c_void_p()
        L.check(L.lib().mcf_engine_create(C.byref(self._h), C.byref(d)))
        self.node_count, self.arc_capacity, self.search_arc_num = node_count, arc_capacity, search_arc_num

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            L.lib().mcf_engine_destroy(h)
            self._h = None

    def upload(self, source, target, cost, state, pi):
        L.check(L.lib().mcf_engine_upload(self._h, _i32(source), _i32(target), _i64(cost), _i8(state), _i64(pi)))

    def patch_state(self, arcs, states):
        arcs, states = _i32(arcs), _i8(states)
        L.check(L.lib().mcf_engine_patch_state(self._h, len(arcs), arcs, states))

    def update_potential(self, nodes, sigma: int):
        nodes = _i32(nodes)
        L.check(L.lib().mcf_engine_update_potential(self._h, len(nodes), nodes, sigma))

    def set_potential(self, nodes, values):
        nodes, values = _i32(nodes), _i64(values)
        L.check(L.lib().mcf_engine_set_potential(self._h, len(nodes), nodes, values))

    def append_potential(self, nodes, values):
        nodes, values = _i32(nodes), _i64(values)
        L.check(L.lib().mcf_engine_append_potential(self._h, nodes.shape[0], nodes, values))

    def shift_potential(self, nodes, values, sigma: int):
        """mcf_engine_shift_potential; `values` may be None when the potentials are bound (bind_potentials): the bound array holds them."""
        nodes = _i32(nodes)
        L.check(L.lib().mcf_engine_shift_potential(self._h, nodes.shape[0], nodes, None if values is None else _i64(values), sigma))

    def shift_potential_runs(self, first, length, sigma: int):
        """mcf_engine_shift_potential_runs: nodes first[r] .. first[r] + length[r] - 1 for every r moved by sigma (bound potentials only)."""
        first, length = _i32(first), _i32(length)
        L.check(L.lib().mcf_engine_shift_potential_runs(self._h, first.shape[0], first, length, sigma))

    def bind_potentials(self, pi):
        """mcf_engine_bind_potentials: `pi` (int64[node_count], C-contiguous) is read in place from now on; the caller keeps it alive and current."""
        if pi is None:
            self._bound_pi = None
            L.check(L.lib().mcf_engine_bind_potentials(self._h, None))
            return
        assert pi.dtype == np.int64 and pi.flags["C_CONTIGUOUS"]
        self._bound_pi = pi
        L.check(L.lib().mcf_engine_bind_potentials(self._h, pi.ctypes.data))

    def reload_threshold(self) -> int:
        v = C.c_int32(0)
        L.check(L.lib().mcf_engine_reload_threshold(self._h, C.byref(v)))
        return v.value

    def reload_potentials(self, changed_nodes: int):
        L.check(L.lib().mcf_engine_reload_potentials(self._h, changed_nodes))

    def renumber_nodes(self, new_of):
        """mcf_engine_renumber_nodes: new_of[old id] = new id (a permutation); a bound potential array must already be in the new order."""
        new_of = _i32(new_of)
        assert new_of.shape == (self.node_count,)
        L.check(L.lib().mcf_engine_renumber_nodes(self._h, new_of))

    def check_reduced_costs(self):
        """(mismatching arcs, lowest such arc or -1): the per-arc reduced costs of the RC layout against cost + pi[source] - pi[target] on the device."""
        m, f = C.c_int64(), C.c_int32()
        L.check(L.lib().mcf_engine_check_reduced_costs(self._h, C.byref(m), C.byref(f)))
        return m.value, f.value

    def patch_arcs(self, arcs, source, target, cost):
        arcs = _i32(arcs)
        L.check(L.lib().mcf_engine_patch_arcs(self._h, len(arcs), arcs, _i32(source), _i32(target), _i64(cost)))

    def find_entering(self):
        f, a, c = C.c_int32(), C.c_int32(), C.c_int64()
        L.check(L.lib().mcf_engine_find_entering(self._h, C.byref(f), C.byref(a), C.byref(c)))
        return bool(f.value), a.value, c.value

    def search_begin(self):
        L.check(L.lib().mcf_engine_search_begin(self._h))

    def search_end(self):
        f, a, c = C.c_int32(), C.c_int32(), C.c_int64()
        L.check(L.lib().mcf_engine_search_end(self._h, C.byref(f), C.byref(a), C.byref(c)))
        return bool(f.value), a.value, c.value

    def search_end_local(self) -> L.Candidate:
        c = L.Candidate()
        L.check(L.lib().mcf_engine_search_end_local(self._h, C.byref(c)))
        return c

    def find_entering_local(self) -> L.Candidate:
        c = L.Candidate()
        L.check(L.lib().mcf_engine_find_entering_local(self._h, C.byref(c)))
        return c

    def resolve(self, cands):
        arr = (L.Candidate * len(cands))(*cands)
        f, a, c = C.c_int32(), C.c_int32(), C.c_int64()
        L.check(L.lib().mcf_engine_resolve(self._h, len(cands), arr, C.byref(f), C.byref(a), C.byref(c)))
        return bool(f.value), a.value, c.value

    def collect_eligible(self, next_arc: int, *, limit: int = 0, block_size: int = 0, head_length: int = 0, survivors: int = 0, capacity: int = None):
        """mcf_engine_collect_eligible (list-rule engines only): the eligible arcs of the cyclic scan from next_arc, in scan order, up to LEMON's
        stop -- FIRST_N with limit > 0 (Candidate List), else BLOCKS (Altering List).  Returns (arcs, reduced_costs, end_arc, arcs_scanned)."""
        mode = L.COLLECT_FIRST_N if limit > 0 else L.COLLECT_BLOCKS
        if capacity is None:
            capacity = limit if mode == L.COLLECT_FIRST_N else head_length + block_size
        rq = L.CollectRequest(next_arc, mode, limit, block_size, head_length, survivors)
        arcs, rcs = np.zeros(max(capacity, 1), np.int32), np.zeros(max(capacity, 1), np.int64)
        k, end, scanned = C.c_int32(), C.c_int32(), C.c_int64()
        L.check(L.lib().mcf_engine_collect_eligible(self._h, C.byref(rq), capacity, C.byref(k), arcs.ctypes.data, rcs.ctypes.data,
                                                    C.byref(end), C.byref(scanned)))
        return arcs[: k.value].copy(), rcs[: k.value].copy(), end.value, scanned.value

    @property
    def next_arc(self) -> int:
        v = C.c_int32(); L.check(L.lib().mcf_engine_get_next_arc(self._h, C.byref(v))); return v.value

    @next_arc.setter
    def next_arc(self, v: int):
        L.check(L.lib().mcf_engine_set_next_arc(self._h, v))

    @property
    def block_size(self) -> int:
        v = C.c_int32(); L.check(L.lib().mcf_engine_get_block_size(self._h, C.byref(v))); return v.value

    def set_block_config(self, config, graph_node_count: int):
        L.check(L.lib().mcf_engine_set_block_config(self._h, C.byref(config), graph_node_count))

    def download_pi(self) -> np.ndarray:
        out = np.empty(self.node_count, np.int64); L.check(L.lib().mcf_engine_download_pi(self._h, out)); return out

    def download_state(self) -> np.ndarray:
        out = np.zeros(self.arc_capacity, np.int8); L.check(L.lib().mcf_engine_download_state(self._h, out)); return out

    def stats(self) -> dict:
        s = L.EngineStats(); L.check(L.lib().mcf_engine_get_stats(self._h, C.byref(s))); return s.as_dict()

    def park(self):
        L.check(L.lib().mcf_engine_park(self._h))

    def reset_stats(self):
        L.check(L.lib().mcf_engine_reset_stats(self._h))

    def bench_scan(self, reps=20, cold=False, flush_bytes=512 << 20):
        avg, mn = C.c_double(), C.c_double()
        L.check(L.lib().mcf_engine_bench_scan(self._h, reps, int(cold), flush_bytes, C.byref(avg), C.byref(mn)))
        return avg.value, mn.value


class HostExchange:
    """mcf_exchange_*: all-gather of the 16-byte candidates between the ranks of one node through POSIX shared memory."""

    def __init__(self, name: str, rank: int, world: int):
        self.world = world
        self._h = C.c_void_p()
        L.check(L.lib().mcf_exchange_open(C.byref(self._h), name.encode(), rank, world))

    def all_gather(self, mine: "L.Candidate"):
        out = (L.Candidate * self.world)()
        L.check(L.lib().mcf_exchange_all_gather(self._h, C.byref(mine), out))
        return list(out)

    def close(self):
        if self._h:
            L.lib().mcf_exchange_close(self._h)
            self._h = None

    def __del__(self):
        self.close()


def _bench_update(self, count, reps=20):
    """mcf_engine_bench_update: (avg ns, min ns, algorithmic bytes) of the potential-update kernel over `count` distinct nodes."""
    avg, mn, nb = C.c_double(), C.c_double(), C.c_int64()
    L.check(L.lib().mcf_engine_bench_update(self._h, count, reps, C.byref(avg), C.byref(mn), C.byref(nb)))
    return avg.value, mn.value, nb.value


PivotEngine.bench_update = _bench_update


def _bench_search(self, reps=1000):
    avg, mn = C.c_double(), C.c_double()
    L.check(L.lib().mcf_engine_bench_search(self._h, reps, C.byref(avg), C.byref(mn)))
    return avg.value, mn.value


PivotEngine.bench_search = _bench_search


def shard_range(search_arc_num: int, rank: int, world: int):
    b, e = C.c_int32(), C.c_int32()
    L.check(L.lib().mcf_shard_range(search_arc_num, rank, world, C.byref(b), C.byref(e)))
    return b.value, e.value


def resolve_candidates(rule: int, optimized: bool, search_arc_num: int, block_size: int, next_arc: int, cands, vector_width=4):
    """Engine-free MINLOC over per-shard candidates; returns (found, arc, reduced_cost, new_next_arc)."""
    arr = (L.Candidate * len(cands))(*cands)
    na, f, a, c = C.c_int32(next_arc), C.c_int32(), C.c_int32(), C.c_int64()
    L.check(L.lib().mcf_resolve_candidates(rule, L.SEM_OPTIMIZED if optimized else L.SEM_PLAIN, _vector_width_abi(vector_width), search_arc_num, block_size,
                                           C.byref(na), len(cands), arr, C.byref(f), C.byref(a), C.byref(c)))
    return bool(f.value), a.value, c.value, na.value
