"""ctypes binding of libmcf_hip.so (the C ABI declared in include/mcf_hip.h).

There is no Python or CPU fallback: if the shared library is missing this module raises, and every
device operation fails with McfError when no MI355X is usable.
"""
from __future__ import annotations

import ctypes as C
import importlib.util
import os
import re
import sys
import warnings

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmcf_hip.so")

# enums of include/mcf_hip.h
RULE_FIRST_ELIGIBLE, RULE_BEST_ELIGIBLE, RULE_BLOCK_SEARCH, RULE_CANDIDATE_LIST, RULE_ALTERING_LIST = 0, 1, 2, 3, 4
COLLECT_FIRST_N, COLLECT_BLOCKS = 0, 1        # mcf_collect_request.mode
SEM_PLAIN, SEM_OPTIMIZED = 1, 2
VECTOR_DEFAULT, VECTOR_NONE = 0, -1          # mcf_engine_desc.vector_width: 0 = 4 (x64), -1 = Vector.IsHardwareAccelerated is false
SUPPLY_GEQ, SUPPLY_LEQ = 0, 1
NOT_SOLVED, OPTIMAL, INFEASIBLE, UNBOUNDED, UNBALANCED = 0, 1, 2, 3, 4
STATE_UPPER, STATE_TREE, STATE_LOWER = -1, 0, 1
INF_CAP = np.iinfo(np.int64).max
ENGINE_SAMPLE_KERNEL_TIME, ENGINE_TIME_EVERY_KERNEL, ENGINE_NO_INLINE_UPDATE, ENGINE_RESIDENT, ENGINE_DISPATCH, ENGINE_CANDIDATES = 1, 2, 4, 8, 16, 32
ENGINE_SHARE_DEVICE = 64
ENGINE_NO_CANDIDATES = 128
ERR_INVALID, ERR_NO_DEVICE, ERR_HIP, ERR_OVERFLOW, ERR_TIMEOUT, ERR_STATE, ERR_IO, ERR_COMM = -1, -2, -3, -4, -5, -6, -7, -8


class McfError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"mcf_hip error {code}: {message}")
        self.code = code


class EngineDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("node_count", "arc_capacity", "search_arc_num", "int_width", "rule", "semantics",
                                         "block_size", "device", "shard_begin", "shard_end", "scan_workgroups", "flags", "resident_workgroups", "vector_width")]


class Candidate(C.Structure):
    _fields_ = [("reduced_cost", C.c_int64), ("pos", C.c_uint32), ("arc", C.c_int32),
                ("range_cost", C.c_int64), ("range_pos", C.c_uint32), ("range_arc", C.c_int32)]

    def __init__(self, reduced_cost=0, pos=0xFFFFFFFF, arc=-1, range_cost=0, range_pos=0xFFFFFFFF, range_arc=-1):
        super().__init__(reduced_cost, pos, arc, range_cost, range_pos, range_arc)


class EngineStats(C.Structure):
    _fields_ = [("searches", C.c_int64), ("scan_launches", C.c_int64), ("update_launches", C.c_int64),
                ("inline_updates", C.c_int64), ("potential_nodes", C.c_int64), ("arcs_scanned", C.c_int64),
                ("timed_scans", C.c_int64), ("timed_scan_ns", C.c_double), ("host_wait_ns", C.c_double),
                ("host_launch_ns", C.c_double), ("scan_workgroups", C.c_int32), ("scan_threads", C.c_int32),
                ("bytes_per_scan", C.c_int64), ("resident", C.c_int64), ("resident_launches", C.c_int64),
                ("resident_requests", C.c_int64), ("resident_scan_ns", C.c_double), ("resident_kernel_ns", C.c_double), ("candidates", C.c_int64),
                ("host_decided", C.c_int64), ("arcs_checked", C.c_int64), ("initial_block_size", C.c_int32), ("current_block_size", C.c_int32),
                ("comm_ranks", C.c_int32), ("reserved", C.c_int32), ("async_refreshes", C.c_int64), ("scan_bytes_read", C.c_int64), ("rc_layout", C.c_int64), ("rc_recomputes", C.c_int64), ("renumberings", C.c_int64), ("heap_compactions", C.c_int64), ("rc_reloads_in_grid", C.c_int64), ("shift_grid", C.c_int64), ("shift_lists", C.c_int64), ("mirror_uploads", C.c_int64),
                ("phase_shift_ns", C.c_double), ("phase_values_ns", C.c_double), ("phase_scan_ns", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_ if n != "reserved"}


OPT_NONE, OPT_ADAPTIVE_BLOCK_SIZE, OPT_SMALL_BLOCKS_FOR_DENSE, OPT_REDUCED_COST_CACHING = 0, 1, 2, 4


class BlockConfig(C.Structure):
    """mcf_block_config: the OptimizationConfig fields the plain BlockSearchPivot reads (OptimizationTypes.cs:24-38)."""
    _fields_ = [("flags", C.c_int32), ("min_block_size", C.c_int32), ("max_block_size", C.c_int32), ("consecutive_hits_before_adapt", C.c_int32),
                ("min_block_size_ratio", C.c_double), ("block_size_growth_factor", C.c_double), ("block_size_shrink_factor", C.c_double),
                ("low_hit_rate_threshold", C.c_double), ("high_hit_rate_threshold", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class NsMetrics(C.Structure):
    _fields_ = [("iterations", C.c_int64), ("total_solve_us", C.c_double), ("pivot_search_us", C.c_double),
                ("tree_update_us", C.c_double), ("potential_update_us", C.c_double), ("setup_us", C.c_double),
                ("loop_us", C.c_double), ("search_arc_num", C.c_int32),
                ("block_size", C.c_int32), ("int_width", C.c_int32), ("reserved", C.c_int32),
                ("degenerate_pivots", C.c_int64), ("potential_nodes", C.c_int64), ("engine", EngineStats),
                ("initial_block_size", C.c_int32), ("final_block_size", C.c_int32), ("total_arcs_checked", C.c_int64),
                ("average_arcs_checked_per_pivot", C.c_double), ("baseline_iterations", C.c_int32), ("config_flags", C.c_int32),
                ("iteration_ratio", C.c_double), ("reference_selects_cached_pivot", C.c_int32), ("reserved2", C.c_int32)]

    def as_dict(self):
        d = {n: getattr(self, n) for n, _ in self._fields_ if n not in ("engine", "reserved", "reserved2")}
        d["engine"] = self.engine.as_dict()
        return d


VALIDATION_KINDS = ("conservation", "lower", "upper", "slack_pos", "slack_neg", "node_dual", "node_slack", "objective", "dual_cost", "status")


class CollectRequest(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("next_arc", "mode", "limit", "block_size", "head_length", "survivors")]


class ListRuleStats(C.Structure):
    _fields_ = [("rule", C.c_int32), ("list_length", C.c_int32), ("minor_limit", C.c_int32), ("block_size", C.c_int32), ("head_length", C.c_int32),
                ("reserved", C.c_int32), ("searches", C.c_int64), ("major_scans", C.c_int64), ("host_answered", C.c_int64),
                ("device_arcs_read", C.c_int64), ("lemon_arcs_scanned", C.c_int64), ("collected", C.c_int64), ("collect_us", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_ if n != "reserved"}


class Validation(C.Structure):
    _fields_ = [("valid", C.c_int32), ("supply_type", C.c_int32), ("objective", C.c_int64), ("dual_cost", C.c_int64),
                ("errors", C.c_int64 * len(VALIDATION_KINDS)), ("first", C.c_int64 * len(VALIDATION_KINDS)),
                ("kernel_us", C.c_double), ("algorithmic_bytes", C.c_int64)]

    def as_dict(self):
        return {"valid": int(self.valid), "supply_type": int(self.supply_type), "objective": int(self.objective), "dual_cost": int(self.dual_cost),
                "errors": dict(zip(VALIDATION_KINDS, map(int, self.errors))), "first": dict(zip(VALIDATION_KINDS, map(int, self.first))),
                "kernel_us": float(self.kernel_us), "algorithmic_bytes": int(self.algorithmic_bytes)}


class BatchDesc(C.Structure):
    """mcf_batch_desc"""
    _fields_ = [("device", C.c_int32), ("pivot_rule", C.c_int32), ("semantics", C.c_int32), ("reserved", C.c_int32), ("pivot_limit", C.c_int64),
                ("pivots_per_launch", C.c_int32), ("trace_capacity", C.c_int32), ("flags", C.c_int32)]


class BatchStats(C.Structure):
    """mcf_batch_stats"""
    _fields_ = [("instances", C.c_int64), ("lds_instances", C.c_int64), ("global_instances", C.c_int64), ("launches", C.c_int64),
                ("total_pivots", C.c_int64), ("workspace_bytes", C.c_int64), ("lds_bytes_max", C.c_int64), ("kernel_ns", C.c_double), ("host_ns", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class BatchResolveStats(C.Structure):
    """mcf_batch_resolve_stats"""
    _fields_ = [("warm_instances", C.c_int64), ("cold_instances", C.c_int64), ("untouched_instances", C.c_int64), ("launches", C.c_int64),
                ("total_pivots", C.c_int64), ("bytes_uploaded", C.c_int64), ("bytes_downloaded", C.c_int64), ("kernel_ns", C.c_double), ("host_ns", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


BATCH_MAX_ARCS, BATCH_MAX_NODES, BATCH_MAX_INSTANCES, BATCH_SHARDED = 65536, 32768, 65536, 1
MEM_HOST, MEM_DEVICE = 0, 1


class UBatchDesc(C.Structure):
    """mcf_ubatch_desc"""
    _fields_ = BatchDesc._fields_ + [("node_count", C.c_int32), ("arc_count", C.c_int32), ("count", C.c_int32), ("source", C.c_void_p), ("target", C.c_void_p)]


class UBatchIo(C.Structure):
    """mcf_ubatch_io"""
    _fields_ = [("memory", C.c_int32), ("supply_type", C.c_int32), ("lower", C.c_void_p), ("upper", C.c_void_p), ("cost", C.c_void_p), ("supply", C.c_void_p),
                ("lower_stride", C.c_int64), ("upper_stride", C.c_int64), ("cost_stride", C.c_int64), ("supply_stride", C.c_int64), ("changed", C.c_void_p),
                ("status", C.c_void_p), ("pivots", C.c_void_p), ("total_cost", C.c_void_p), ("flows", C.c_void_p), ("potentials", C.c_void_p), ("trace", C.c_void_p)]


class UBatchStats(C.Structure):
    """mcf_ubatch_stats"""
    _fields_ = BatchStats._fields_ + [("bytes_up", C.c_int64), ("bytes_down", C.c_int64), ("begin_ns", C.c_double), ("finish_ns", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class UBatchRedataStats(C.Structure):
    """mcf_ubatch_redata_stats"""
    _fields_ = [(name, C.c_int64) for name in ("warm_instances", "cold_instances", "fallback_instances", "untouched_instances", "dual_pivots", "primal_pivots",
                                               "launches", "bytes_up", "bytes_down")] + \
               [(name, C.c_double) for name in ("kernel_ns", "host_ns", "begin_ns", "finish_ns")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class UBatchCheckIo(C.Structure):
    """mcf_ubatch_check_io"""
    _fields_ = [("memory", C.c_int32), ("supply_type", C.c_int32), ("lower", C.c_void_p), ("upper", C.c_void_p), ("cost", C.c_void_p), ("supply", C.c_void_p),
                ("lower_stride", C.c_int64), ("upper_stride", C.c_int64), ("cost_stride", C.c_int64), ("supply_stride", C.c_int64),
                ("status", C.c_void_p), ("total_cost", C.c_void_p), ("flows", C.c_void_p), ("potentials", C.c_void_p),
                ("valid", C.c_void_p), ("errors", C.c_void_p), ("first", C.c_void_p), ("objective", C.c_void_p), ("dual_cost", C.c_void_p)]


class UBatchCheckSummary(C.Structure):
    """mcf_ubatch_check_summary"""
    _fields_ = [("instances", C.c_int64), ("invalid", C.c_int64), ("first_invalid", C.c_int64), ("kernel_ns", C.c_double), ("bytes_up", C.c_int64),
                ("bytes_down", C.c_int64)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class RBatchDesc(C.Structure):
    """mcf_rbatch_desc"""
    _fields_ = BatchDesc._fields_ + [("graph_count", C.c_int32), ("count", C.c_int32), ("node_count", C.c_void_p), ("arc_start", C.c_void_p),
                                     ("source", C.c_void_p), ("target", C.c_void_p), ("graph_of", C.c_void_p)]


class RBatchIo(C.Structure):
    """mcf_rbatch_io"""
    _fields_ = [("memory", C.c_int32), ("supply_type", C.c_int32), ("lower", C.c_void_p), ("upper", C.c_void_p), ("cost", C.c_void_p), ("supply", C.c_void_p),
                ("changed", C.c_void_p),
                ("status", C.c_void_p), ("pivots", C.c_void_p), ("total_cost", C.c_void_p), ("flows", C.c_void_p), ("potentials", C.c_void_p), ("trace", C.c_void_p)]


class RBatchCheckIo(C.Structure):
    """mcf_rbatch_check_io"""
    _fields_ = [("memory", C.c_int32), ("supply_type", C.c_int32), ("lower", C.c_void_p), ("upper", C.c_void_p), ("cost", C.c_void_p), ("supply", C.c_void_p),
                ("status", C.c_void_p), ("total_cost", C.c_void_p), ("flows", C.c_void_p), ("potentials", C.c_void_p),
                ("valid", C.c_void_p), ("errors", C.c_void_p), ("first", C.c_void_p), ("objective", C.c_void_p), ("dual_cost", C.c_void_p)]


RANGE_INF = (1 << 63) - 1      # MCF_RANGE_INF


class UBatchRangeIo(C.Structure):
    """mcf_ubatch_range_io"""
    _fields_ = [("memory", C.c_int32), ("reserved", C.c_int32), ("ranged", C.c_void_p), ("arc_state", C.c_void_p), ("cost_down", C.c_void_p), ("cost_up", C.c_void_p)]


class RBatchRangeIo(C.Structure):
    """mcf_rbatch_range_io"""
    _fields_ = UBatchRangeIo._fields_


class UBatchRangeStats(C.Structure):
    """mcf_ubatch_range_stats"""
    _fields_ = [(name, C.c_int64) for name in ("instances", "ranged", "lds_instances", "global_instances", "tree_arcs", "cycle_hops")] + \
               [("kernel_ns", C.c_double), ("bytes_up", C.c_int64), ("bytes_down", C.c_int64)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class UBatchDataRangeIo(C.Structure):
    """mcf_ubatch_data_range_io"""
    _fields_ = [("memory", C.c_int32), ("reserved", C.c_int32), ("pair_count", C.c_int64), ("pairs", C.c_void_p)] + \
               [(name, C.c_void_p) for name in ("ranged", "arc_state", "flow_down", "flow_up", "ship_forth", "ship_back")]


class RBatchDataRangeIo(C.Structure):
    """mcf_rbatch_data_range_io"""
    _fields_ = [("memory", C.c_int32), ("reserved", C.c_int32), ("pairs", C.c_void_p), ("pair_row", C.c_void_p), ("ship_row", C.c_void_p)] + \
               [(name, C.c_void_p) for name in ("ranged", "arc_state", "flow_down", "flow_up", "ship_forth", "ship_back")]


class UBatchDataRangeStats(C.Structure):
    """mcf_ubatch_data_range_stats"""
    _fields_ = [(name, C.c_int64) for name in ("instances", "ranged", "lds_instances", "global_instances", "walks", "hops")] + \
               [("kernel_ns", C.c_double), ("bytes_up", C.c_int64), ("bytes_down", C.c_int64)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class UBatchBasisIo(C.Structure):
    """mcf_ubatch_basis_io"""
    _fields_ = [("memory", C.c_int32), ("reserved", C.c_int32), ("arc_state", C.c_void_p), ("state_stride", C.c_int64)]


class RBatchBasisIo(C.Structure):
    """mcf_rbatch_basis_io"""
    _fields_ = [("memory", C.c_int32), ("reserved", C.c_int32), ("arc_state", C.c_void_p)]


class UBatchStartStats(C.Structure):
    """mcf_ubatch_start_stats"""
    _fields_ = [(name, C.c_int64) for name in ("primal_starts", "dual_starts", "cold_instances", "fallback_instances", "dual_pivots", "primal_pivots",
                                               "launches", "bytes_up", "bytes_down")] + \
               [(name, C.c_double) for name in ("kernel_ns", "host_ns", "begin_ns", "finish_ns")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


DIAG_NONE, DIAG_FEASIBLE, DIAG_CUT, DIAG_OPEN, DIAG_BOUNDS = range(5)      # MCF_DIAG_*


class UBatchDiagnoseIo(C.Structure):
    """mcf_ubatch_diagnose_io"""
    _fields_ = [("memory", C.c_int32), ("reserved", C.c_int32)] + [(name, C.c_void_p) for name in ("verdict", "violation", "set_size", "side", "unmet")]


class RBatchDiagnoseIo(C.Structure):
    """mcf_rbatch_diagnose_io"""
    _fields_ = UBatchDiagnoseIo._fields_


class UBatchDiagnoseStats(C.Structure):
    """mcf_ubatch_diagnose_stats"""
    _fields_ = [(name, C.c_int64) for name in ("instances", "none", "feasible", "cut", "open", "bounds", "lds_instances", "global_instances", "levels",
                                               "frontier_nodes", "inc_entries")] + \
               [("kernel_ns", C.c_double), ("bytes_up", C.c_int64), ("bytes_down", C.c_int64)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


RAY_NONE, RAY_BOUNDED, RAY_CYCLE, RAY_BOUNDS = range(4)                    # MCF_RAY_*


class UBatchRaysIo(C.Structure):
    """mcf_ubatch_rays_io"""
    _fields_ = [("memory", C.c_int32), ("reserved", C.c_int32)] + [(name, C.c_void_p) for name in ("verdict", "cycle_cost", "cycle_length", "on_cycle", "label")]


class RBatchRaysIo(C.Structure):
    """mcf_rbatch_rays_io"""
    _fields_ = UBatchRaysIo._fields_


class UBatchRaysStats(C.Structure):
    """mcf_ubatch_rays_stats"""
    _fields_ = [(name, C.c_int64) for name in ("instances", "none", "bounded", "cycle", "bounds", "lds_instances", "global_instances", "rounds",
                                               "frontier_nodes", "inc_entries", "cycle_arcs")] + \
               [("kernel_ns", C.c_double), ("bytes_up", C.c_int64), ("bytes_down", C.c_int64)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class ProblemStruct(C.Structure):
    _fields_ = [("node_count", C.c_int32), ("arc_count", C.c_int32), ("source", C.POINTER(C.c_int32)),
                ("target", C.POINTER(C.c_int32)), ("lower", C.POINTER(C.c_int64)), ("upper", C.POINTER(C.c_int64)),
                ("cost", C.POINTER(C.c_int64)), ("supply", C.POINTER(C.c_int64))]


_i32p = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")
_i64p = np.ctypeslib.ndpointer(np.int64, flags="C_CONTIGUOUS")


class _i64p_or_null(_i64p):
    """int64 array or None (NULL) -- for the arguments the header marks as optional."""
    @classmethod
    def from_param(cls, obj):
        return None if obj is None else _i64p.from_param(obj)


_i8p = np.ctypeslib.ndpointer(np.int8, flags="C_CONTIGUOUS")
_u8p = np.ctypeslib.ndpointer(np.uint8, flags="C_CONTIGUOUS")
_P = C.POINTER

# every symbol include/mcf_hip.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "mcf_last_error": (C.c_char_p, []),
    "mcf_version": (C.c_char_p, []),
    "mcf_device_count": (C.c_int, []),
    "mcf_device_compute_units": (C.c_int, [C.c_int32]),
    "mcf_engine_create": (C.c_int, [_P(C.c_void_p), _P(EngineDesc)]),
    "mcf_engine_destroy": (None, [C.c_void_p]),
    "mcf_engine_upload": (C.c_int, [C.c_void_p, _i32p, _i32p, _i64p, _i8p, _i64p]),
    "mcf_engine_patch_state": (C.c_int, [C.c_void_p, C.c_int32, _i32p, _i8p]),
    "mcf_engine_update_potential": (C.c_int, [C.c_void_p, C.c_int32, _i32p, C.c_int64]),
    "mcf_engine_set_potential": (C.c_int, [C.c_void_p, C.c_int32, _i32p, _i64p]),
    "mcf_engine_append_potential": (C.c_int, [C.c_void_p, C.c_int32, _i32p, _i64p]),
    "mcf_engine_bind_potentials": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mcf_engine_shift_potential": (C.c_int, [C.c_void_p, C.c_int32, _i32p, _i64p_or_null, C.c_int64]),
    "mcf_engine_shift_potential_runs": (C.c_int, [C.c_void_p, C.c_int32, _i32p, _i32p, C.c_int64]),
    "mcf_engine_reload_threshold": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "mcf_engine_reload_potentials": (C.c_int, [C.c_void_p, C.c_int32]),
    "mcf_engine_patch_arcs": (C.c_int, [C.c_void_p, C.c_int32, _i32p, _i32p, _i32p, _i64p]),
    "mcf_engine_can_renumber": (C.c_int, [C.c_void_p, _P(C.c_int32)]),
    "mcf_engine_check_reduced_costs": (C.c_int, [C.c_void_p, _P(C.c_int64), _P(C.c_int32)]),
    "mcf_ns_check_reduced_costs": (C.c_int, [C.c_void_p, _P(C.c_int64)]),
    "mcf_engine_renumber_nodes": (C.c_int, [C.c_void_p, _i32p]),
    "mcf_engine_find_entering": (C.c_int, [C.c_void_p, _P(C.c_int32), _P(C.c_int32), _P(C.c_int64)]),
    "mcf_engine_search_begin": (C.c_int, [C.c_void_p]),
    "mcf_engine_search_end": (C.c_int, [C.c_void_p, _P(C.c_int32), _P(C.c_int32), _P(C.c_int64)]),
    "mcf_engine_find_entering_local": (C.c_int, [C.c_void_p, _P(Candidate)]),
    "mcf_engine_collect_eligible": (C.c_int, [C.c_void_p, _P(CollectRequest), C.c_int32, _P(C.c_int32), C.c_void_p, C.c_void_p,
                                              _P(C.c_int32), _P(C.c_int64)]),
    "mcf_engine_search_end_local": (C.c_int, [C.c_void_p, _P(Candidate)]),
    "mcf_exchange_open": (C.c_int, [_P(C.c_void_p), C.c_char_p, C.c_int32, C.c_int32]),
    "mcf_exchange_close": (None, [C.c_void_p]),
    "mcf_exchange_all_gather": (C.c_int, [C.c_void_p, _P(Candidate), _P(Candidate)]),
    "mcf_engine_resolve": (C.c_int, [C.c_void_p, C.c_int32, _P(Candidate), _P(C.c_int32), _P(C.c_int32), _P(C.c_int64)]),
    "mcf_resolve_candidates": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P(C.c_int32), C.c_int32, _P(Candidate),
                                        _P(C.c_int32), _P(C.c_int32), _P(C.c_int64)]),
    "mcf_shard_range": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _P(C.c_int32), _P(C.c_int32)]),
    "mcf_engine_park": (C.c_int, [C.c_void_p]),
    "mcf_engine_get_next_arc": (C.c_int, [C.c_void_p, _P(C.c_int32)]),
    "mcf_engine_set_next_arc": (C.c_int, [C.c_void_p, C.c_int32]),
    "mcf_engine_get_block_size": (C.c_int, [C.c_void_p, _P(C.c_int32)]),
    "mcf_block_config_default": (None, [_P(BlockConfig)]),
    "mcf_block_config_auto": (C.c_int, [_P(BlockConfig), C.c_int32, C.c_int32, _i32p, _i32p]),
    "mcf_block_initial_size": (C.c_int, [_P(BlockConfig), C.c_int32, C.c_int32, _P(C.c_int32), _P(C.c_int32)]),
    "mcf_block_adapt": (C.c_int, [_P(BlockConfig), C.c_int32, C.c_int64, _P(C.c_int32), _P(C.c_int32)]),
    "mcf_engine_set_block_config": (C.c_int, [C.c_void_p, _P(BlockConfig), C.c_int32]),
    "mcf_engine_download_pi": (C.c_int, [C.c_void_p, _i64p]),
    "mcf_engine_download_state": (C.c_int, [C.c_void_p, _i8p]),
    "mcf_engine_get_stats": (C.c_int, [C.c_void_p, _P(EngineStats)]),
    "mcf_engine_reset_stats": (C.c_int, [C.c_void_p]),
    "mcf_engine_bench_scan": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int64, _P(C.c_double), _P(C.c_double)]),
    "mcf_engine_bench_search": (C.c_int, [C.c_void_p, C.c_int32, _P(C.c_double), _P(C.c_double)]),
    "mcf_engine_bench_update": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, _P(C.c_double), _P(C.c_double), _P(C.c_int64)]),
    "mcf_comm_unique_id": (C.c_int, [_u8p]),
    "mcf_engine_comm_init": (C.c_int, [C.c_void_p, _u8p, C.c_int32, C.c_int32]),
    "mcf_engine_find_entering_sharded": (C.c_int, [C.c_void_p, _P(C.c_int32), _P(C.c_int32), _P(C.c_int64)]),
    "mcf_ns_create": (C.c_int, [_P(C.c_void_p), C.c_int32, C.c_int32, _i32p, _i32p]),
    "mcf_ns_destroy": (None, [C.c_void_p]),
    "mcf_ns_set_arc_bounds": (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.c_int64]),
    "mcf_ns_set_arc_cost": (C.c_int, [C.c_void_p, C.c_int32, C.c_int64]),
    "mcf_ns_set_node_supply": (C.c_int, [C.c_void_p, C.c_int32, C.c_int64]),
    "mcf_ns_set_problem": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mcf_ns_set_supply_type": (C.c_int, [C.c_void_p, C.c_int32]),
    "mcf_ns_set_pivot_rule": (C.c_int, [C.c_void_p, C.c_int32]),
    "mcf_ns_set_list_pivot_rule": (C.c_int, [C.c_void_p, C.c_int32]),
    "mcf_ns_enable_optimized_pivot": (C.c_int, [C.c_void_p, C.c_int32]),
    "mcf_ns_set_vector_width": (C.c_int, [C.c_void_p, C.c_int32]),
    "mcf_ns_set_optimization_config": (C.c_int, [C.c_void_p, _P(BlockConfig)]),
    "mcf_ns_enable_optimizations": (C.c_int, [C.c_void_p, C.c_int32]),
    "mcf_ns_set_auto_configuration": (C.c_int, [C.c_void_p, C.c_int32]),
    "mcf_ns_set_device": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "mcf_ns_set_device_share": (C.c_int, [C.c_void_p, C.c_int32]),
    "mcf_ns_set_sharding": (C.c_int, [C.c_void_p, _u8p, C.c_int32, C.c_int32]),
    "mcf_ns_set_sharding_host": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int32, C.c_int32]),
    "mcf_ns_set_shard_group": (C.c_int, [C.c_void_p, C.c_int32, _i32p]),
    "mcf_ns_prepare": (C.c_int, [C.c_void_p]),
    "mcf_ns_solve": (C.c_int, [C.c_void_p, _P(C.c_int32)]),
    "mcf_ns_status": (C.c_int, [C.c_void_p, _P(C.c_int32)]),
    "mcf_ns_get_flow": (C.c_int, [C.c_void_p, C.c_int32, _P(C.c_int64)]),
    "mcf_ns_get_potential": (C.c_int, [C.c_void_p, C.c_int32, _P(C.c_int64)]),
    "mcf_ns_get_total_cost": (C.c_int, [C.c_void_p, _P(C.c_int64)]),
    "mcf_ns_get_flows": (C.c_int, [C.c_void_p, _i64p]),
    "mcf_ns_get_potentials": (C.c_int, [C.c_void_p, _i64p]),
    "mcf_ns_get_arc_upper_bound": (C.c_int, [C.c_void_p, C.c_int32, _P(C.c_int64)]),
    "mcf_ns_get_metrics": (C.c_int, [C.c_void_p, _P(NsMetrics)]),
    "mcf_ns_get_list_rule_stats": (C.c_int, [C.c_void_p, _P(ListRuleStats)]),
    "mcf_ns_set_pivot_limit": (C.c_int, [C.c_void_p, C.c_int64]),
    "mcf_ns_set_trace": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    "mcf_ns_get_trace_length": (C.c_int, [C.c_void_p, _P(C.c_int64)]),
    "mcf_ns_begin": (C.c_int, [C.c_void_p, _P(C.c_int32)]),
    "mcf_ns_apply_pivot": (C.c_int, [C.c_void_p, C.c_int32, _P(C.c_int32)]),
    "mcf_ns_finish": (C.c_int, [C.c_void_p, _P(C.c_int32)]),
    "mcf_ns_replay": (C.c_int, [C.c_void_p, _i32p, C.c_int64, C.c_int32, C.c_double]),
    "mcf_ns_check_thread_breaks": (C.c_int, [C.c_void_p, _P(C.c_int64)]),
    "mcf_ns_internal": (C.c_int, [C.c_void_p, _P(C.c_int32), _P(C.c_int32), _P(_P(C.c_int32)), _P(_P(C.c_int32)),
                                  _P(_P(C.c_int64)), _P(_P(C.c_int8)), _P(_P(C.c_int64))]),
    "mcf_ns_tree": (C.c_int, [C.c_void_p, _P(_P(C.c_int32)), _P(_P(C.c_int32)), _P(_P(C.c_int32)), _P(_P(C.c_int8)), _P(_P(C.c_int64)), _P(_P(C.c_int64))]),
    "mcf_ns_last_pivot": (C.c_int, [C.c_void_p, _P(C.c_int32), _P(C.c_int32), _P(C.c_int8), _P(C.c_int32),
                                    _P(_P(C.c_int32)), _P(C.c_int64)]),
    "mcf_validator_create": (C.c_int, [_P(C.c_void_p), C.c_int32, C.c_int32, C.c_int32]),
    "mcf_validator_destroy": (None, [C.c_void_p]),
    "mcf_validator_upload": (C.c_int, [C.c_void_p] + [C.c_void_p] * 8),
    "mcf_validator_run": (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, _P(Validation)]),
    "mcf_ns_validate": (C.c_int, [C.c_void_p, _P(Validation)]),
    "mcf_batch_create": (C.c_int, [_P(C.c_void_p), _P(BatchDesc)]),
    "mcf_batch_destroy": (None, [C.c_void_p]),
    "mcf_batch_add": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, _P(C.c_int32)]),
    "mcf_batch_solve": (C.c_int, [C.c_void_p]),
    "mcf_batch_run_on_host": (C.c_int, [C.c_void_p]),
    "mcf_batch_get_status": (C.c_int, [C.c_void_p, C.c_int32, _P(C.c_int32)]),
    "mcf_batch_get_total_cost": (C.c_int, [C.c_void_p, C.c_int32, _P(C.c_int64)]),
    "mcf_batch_get_flows": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p]),
    "mcf_batch_get_potentials": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p]),
    "mcf_batch_get_pivots": (C.c_int, [C.c_void_p, C.c_int32, _P(C.c_int64)]),
    "mcf_batch_get_trace": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, _P(C.c_int64)]),
    "mcf_batch_get_stats": (C.c_int, [C.c_void_p, _P(BatchStats)]),
    "mcf_batch_set_costs": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p]),
    "mcf_batch_resolve": (C.c_int, [C.c_void_p]),
    "mcf_batch_rerun_on_host": (C.c_int, [C.c_void_p]),
    "mcf_batch_get_resolve_stats": (C.c_int, [C.c_void_p, _P(BatchResolveStats)]),
    "mcf_ubatch_create": (C.c_int, [_P(C.c_void_p), _P(UBatchDesc)]),
    "mcf_ubatch_destroy": (None, [C.c_void_p]),
    "mcf_ubatch_solve": (C.c_int, [C.c_void_p, _P(UBatchIo)]),
    "mcf_ubatch_resolve": (C.c_int, [C.c_void_p, _P(UBatchIo)]),
    "mcf_ubatch_run_on_host": (C.c_int, [C.c_void_p, _P(UBatchIo)]),
    "mcf_ubatch_rerun_on_host": (C.c_int, [C.c_void_p, _P(UBatchIo)]),
    "mcf_ubatch_get_stats": (C.c_int, [C.c_void_p, _P(UBatchStats)]),
    "mcf_ubatch_resolve_data": (C.c_int, [C.c_void_p, _P(UBatchIo)]),
    "mcf_ubatch_rerun_data_on_host": (C.c_int, [C.c_void_p, _P(UBatchIo)]),
    "mcf_ubatch_get_redata_stats": (C.c_int, [C.c_void_p, _P(UBatchRedataStats)]),
    "mcf_ubatch_validate": (C.c_int, [C.c_void_p, _P(UBatchCheckIo), _P(UBatchCheckSummary)]),
    "mcf_ubatch_validate_on_host": (C.c_int, [C.c_void_p, _P(UBatchCheckIo), _P(UBatchCheckSummary)]),
    "mcf_ubatch_cost_ranges": (C.c_int, [C.c_void_p, _P(UBatchRangeIo)]),
    "mcf_ubatch_cost_ranges_on_host": (C.c_int, [C.c_void_p, _P(UBatchRangeIo)]),
    "mcf_ubatch_get_range_stats": (C.c_int, [C.c_void_p, _P(UBatchRangeStats)]),
    "mcf_ubatch_solve_from": (C.c_int, [C.c_void_p, _P(UBatchIo), _P(UBatchBasisIo)]),
    "mcf_ubatch_run_from_on_host": (C.c_int, [C.c_void_p, _P(UBatchIo), _P(UBatchBasisIo)]),
    "mcf_ubatch_get_start_stats": (C.c_int, [C.c_void_p, _P(UBatchStartStats)]),
    "mcf_rbatch_create": (C.c_int, [_P(C.c_void_p), _P(RBatchDesc)]),
    "mcf_rbatch_destroy": (None, [C.c_void_p]),
    "mcf_rbatch_get_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "mcf_rbatch_solve": (C.c_int, [C.c_void_p, _P(RBatchIo)]),
    "mcf_rbatch_resolve": (C.c_int, [C.c_void_p, _P(RBatchIo)]),
    "mcf_rbatch_run_on_host": (C.c_int, [C.c_void_p, _P(RBatchIo)]),
    "mcf_rbatch_rerun_on_host": (C.c_int, [C.c_void_p, _P(RBatchIo)]),
    "mcf_rbatch_get_stats": (C.c_int, [C.c_void_p, _P(UBatchStats)]),
    "mcf_rbatch_resolve_data": (C.c_int, [C.c_void_p, _P(RBatchIo)]),
    "mcf_rbatch_rerun_data_on_host": (C.c_int, [C.c_void_p, _P(RBatchIo)]),
    "mcf_rbatch_get_redata_stats": (C.c_int, [C.c_void_p, _P(UBatchRedataStats)]),
    "mcf_rbatch_validate": (C.c_int, [C.c_void_p, _P(RBatchCheckIo), _P(UBatchCheckSummary)]),
    "mcf_rbatch_validate_on_host": (C.c_int, [C.c_void_p, _P(RBatchCheckIo), _P(UBatchCheckSummary)]),
    "mcf_rbatch_cost_ranges": (C.c_int, [C.c_void_p, _P(RBatchRangeIo)]),
    "mcf_rbatch_cost_ranges_on_host": (C.c_int, [C.c_void_p, _P(RBatchRangeIo)]),
    "mcf_rbatch_get_range_stats": (C.c_int, [C.c_void_p, _P(UBatchRangeStats)]),
    "mcf_ubatch_data_ranges": (C.c_int, [C.c_void_p, _P(UBatchDataRangeIo)]),
    "mcf_ubatch_data_ranges_on_host": (C.c_int, [C.c_void_p, _P(UBatchDataRangeIo)]),
    "mcf_ubatch_get_data_range_stats": (C.c_int, [C.c_void_p, _P(UBatchDataRangeStats)]),
    "mcf_rbatch_data_ranges": (C.c_int, [C.c_void_p, _P(RBatchDataRangeIo)]),
    "mcf_rbatch_data_ranges_on_host": (C.c_int, [C.c_void_p, _P(RBatchDataRangeIo)]),
    "mcf_rbatch_get_data_range_stats": (C.c_int, [C.c_void_p, _P(UBatchDataRangeStats)]),
    "mcf_rbatch_solve_from": (C.c_int, [C.c_void_p, _P(RBatchIo), _P(RBatchBasisIo)]),
    "mcf_rbatch_run_from_on_host": (C.c_int, [C.c_void_p, _P(RBatchIo), _P(RBatchBasisIo)]),
    "mcf_rbatch_get_start_stats": (C.c_int, [C.c_void_p, _P(UBatchStartStats)]),
    "mcf_ubatch_diagnose": (C.c_int, [C.c_void_p, _P(UBatchDiagnoseIo)]),
    "mcf_ubatch_diagnose_on_host": (C.c_int, [C.c_void_p, _P(UBatchDiagnoseIo)]),
    "mcf_ubatch_get_diagnose_stats": (C.c_int, [C.c_void_p, _P(UBatchDiagnoseStats)]),
    "mcf_rbatch_diagnose": (C.c_int, [C.c_void_p, _P(RBatchDiagnoseIo)]),
    "mcf_rbatch_diagnose_on_host": (C.c_int, [C.c_void_p, _P(RBatchDiagnoseIo)]),
    "mcf_rbatch_get_diagnose_stats": (C.c_int, [C.c_void_p, _P(UBatchDiagnoseStats)]),
    "mcf_ubatch_rays": (C.c_int, [C.c_void_p, _P(UBatchRaysIo)]),
    "mcf_ubatch_rays_on_host": (C.c_int, [C.c_void_p, _P(UBatchRaysIo)]),
    "mcf_ubatch_get_rays_stats": (C.c_int, [C.c_void_p, _P(UBatchRaysStats)]),
    "mcf_rbatch_rays": (C.c_int, [C.c_void_p, _P(RBatchRaysIo)]),
    "mcf_rbatch_rays_on_host": (C.c_int, [C.c_void_p, _P(RBatchRaysIo)]),
    "mcf_rbatch_get_rays_stats": (C.c_int, [C.c_void_p, _P(UBatchRaysStats)]),
    "mcf_problem_free": (None, [_P(ProblemStruct)]),
    "mcf_gen_netgen_like": (C.c_int, [_P(ProblemStruct), C.c_uint64, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                      C.c_int64, C.c_int64, C.c_int64, C.c_int64]),
    "mcf_gen_assignment": (C.c_int, [_P(ProblemStruct), C.c_uint64, C.c_int32, C.c_int64, C.c_int64]),
    "mcf_dimacs_read": (C.c_int, [_P(ProblemStruct), C.c_char_p]),
    "mcf_dimacs_write": (C.c_int, [_P(ProblemStruct), C.c_char_p]),
    "mcf_solution_write": (C.c_int, [C.c_char_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]),
    "mcf_solution_read": (C.c_int, [C.c_char_p, _P(ProblemStruct), _P(C.c_int64), _P(C.c_int32), C.c_void_p, C.c_void_p, _P(C.c_int32)]),
}

_lib = None


def _hip_sonames(path):
    """Every libamdhip64.so.N named in a shared library: the runtime it needs, or -- in the runtime itself -- its own soname."""
    with open(path, "rb") as fh:
        return set(re.findall(rb"libamdhip64\.so\.\d+", fh.read()))


def _share_torchs_hip_runtime():
    """torch's ROCm wheels bring a HIP runtime of their own (torch/lib/libamdhip64.so), and a process can open the GPU through one runtime
    only: with two loaded, the second finds no device.  torch asks for its copy by file name, so it never reuses a runtime that is
    already there; this library asks by soname and takes the one that is loaded.  So where torch is installed but not imported yet, and
    its runtime has the soname libmcf_hip.so was linked against, that runtime is loaded first, and a later `import torch` (UniformBatch
    takes tensors) still finds the GPU.  torch itself is not imported.  With another soname (a torch wheel of another ROCm major) nothing
    is preloaded: the library runs on the system's runtime as long as torch.cuda stays unused, as it always did.
    MCF_HIP_RUNTIME=system switches the preload off."""
    if os.environ.get("MCF_HIP_RUNTIME", "").lower() == "system" or "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        return
    if spec is None or not spec.origin:
        return
    path = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if not os.path.exists(path):
        return
    try:
        if not _hip_sonames(LIB_PATH) & _hip_sonames(path):
            return
        C.CDLL(path, mode=C.RTLD_GLOBAL)
    except OSError as e:
        warnings.warn(f"mincostflow_amd: torch's HIP runtime {path} could not be loaded first ({e}); torch.cuda may find no device in this process")


def lib():
    """The loaded library.  Raises if libmcf_hip.so has not been built (python -c 'import __graft_entry__ as g; g.build()')."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: build it with `make -C mincostflow_amd/csrc` "
                              "(there is no Python/CPU implementation to fall back to)")
        _share_torchs_hip_runtime()
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(rc: int):
    if rc != 0:
        raise McfError(rc, lib().mcf_last_error().decode(errors="replace"))


def device_count() -> int:
    return lib().mcf_device_count()


def comm_unique_id() -> np.ndarray:
    """128-byte ncclUniqueId (rank 0 creates it, the caller broadcasts it)."""
    out = np.zeros(128, np.uint8)
    check(lib().mcf_comm_unique_id(out))
    return out
