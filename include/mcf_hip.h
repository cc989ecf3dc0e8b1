/*
 * mcf_hip.h -- C ABI of libmcf_hip.so, the MI355X (gfx950) network-simplex pivot engine.
 *
 * Drop-in boundary.  All file:line citations are relative to the reference
 * repository pdegenhardt/MinCostFlow; "NS.cs" = src/MinCostFlow.Core/Lemon/Algorithms/NetworkSimplex.cs,
 * "BSPO.cs" = src/MinCostFlow.Core/Lemon/Algorithms/Internal/BlockSearchPivotOptimized.cs.
 *
 * Two layers are exported:
 *
 *  (1) mcf_engine_*  -- the device side of the seam `private interface IFindEnteringArc
 *      { bool FindEnteringArc(); }` (NS.cs:1286-1289) plus UpdatePotentials (NS.cs:1185-1209).  The
 *      SoA arc arrays (Source, Target, _cost, State) and the node potentials _pi live in HBM; the
 *      host keeps the sequential pivot loop and the spanning tree.  This is what a C# host binds
 *      with [DllImport("mcf_hip")] in place of OptimizedPivotWrapper (NS.cs:1671-1724); the stub is
 *      in INTEGRATION.md.
 *
 *  (2) mcf_ns_*      -- a C++ restatement of the host side of NetworkSimplex (the public setters /
 *      Solve() / getters of NS.cs:153-527 and the tree maintenance NS.cs:925-1183) that drives
 *      the engine, so the path can be exercised end to end without a .NET toolchain.  Names and
 *      argument meaning mirror the reference class.  There is NO CPU entering-arc search in this
 *      library: mcf_ns_solve() fails with MCF_ERR_NO_DEVICE when no HIP device is usable.  (The one
 *      exception is a test hook, mcf_batch_run_on_host, not a solver.)
 *
 *  (3) mcf_validator_* / mcf_ns_validate -- the reference's SolutionValidator (Validation/SolutionValidator.cs)
 *      as two device reductions; like the search it has no CPU path in this library.
 *
 *  (4) mcf_batch_*   -- many small independent instances, each solved entirely on the device by one
 *      workgroup (no counterpart in the reference, whose callers loop over Solve()).
 *
 * Conventions: every function returns 0 (MCF_OK) or a negative mcf_status; the message is available
 * from mcf_last_error() (thread-local).  Nothing throws across the ABI.  Host arrays are borrowed
 * for the duration of the call only.  One engine / one solver = one host thread at a time (the
 * reference solver is single-threaded: docs/platform-architecture.md:126-130).
 */
#ifndef MCF_HIP_H
#define MCF_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MCF_API __attribute__((visibility("default")))

typedef enum mcf_status {
    MCF_OK = 0,
    MCF_ERR_INVALID = -1,     /* bad argument (ArgumentException in the reference) */
    MCF_ERR_NO_DEVICE = -2,   /* no usable HIP device / HIP runtime failure at start-up */
    MCF_ERR_HIP = -3,         /* a HIP call failed later on */
    MCF_ERR_OVERFLOW = -4,    /* a value does not fit the engine's int_width (use 64) */
    MCF_ERR_TIMEOUT = -5,     /* the device did not answer */
    MCF_ERR_STATE = -6,       /* call out of order (InvalidOperationException in the reference) */
    MCF_ERR_IO = -7,          /* file / parse error */
    MCF_ERR_COMM = -8         /* RCCL failure */
} mcf_status;

/* Types/PivotRule.cs:7-41 (values kept).  CANDIDATE_LIST and ALTERING_LIST are declared by the reference but not implemented there
 * (NS.cs:879-885 throws); this library runs them as LEMON's rules (lemon/network_simplex.h:415-635) on the host driver, with the
 * device doing the major scans only: mcf_ns_set_list_pivot_rule, mcf_engine_collect_eligible. */
typedef enum mcf_pivot_rule { MCF_RULE_FIRST_ELIGIBLE = 0, MCF_RULE_BEST_ELIGIBLE = 1, MCF_RULE_BLOCK_SEARCH = 2,
                              MCF_RULE_CANDIDATE_LIST = 3, MCF_RULE_ALTERING_LIST = 4 } mcf_pivot_rule;
/* Which of the reference's two implementations of a rule is reproduced:
 * PLAIN = the nested classes of NS.cs:1292-1668; OPTIMIZED = BSPO.cs (EnableOptimizedPivot(true)). */
typedef enum mcf_semantics { MCF_SEM_PLAIN = 1, MCF_SEM_OPTIMIZED = 2 } mcf_semantics;
/* OPTIMIZED Block Search depends on a property of the MACHINE the reference runs on (difference D14):
 * BSPO.cs:74 sends ranges of at least 2 * Vector<long>.Count arcs through ProcessArcRangeSIMD when Vector.IsHardwareAccelerated, and a
 * block-boundary hit in there returns into a scalar loop whose counter is 0 and never reaches 0 again (BSPO.cs:84-99, :143-148): the scan
 * runs on to the end of the range, the entering arc is the best of the whole range and _nextArc becomes the range's end.  Only a hit in
 * the tail behind the last full group of Vector<long>.Count arcs stops at the block boundary.  vector_width = Vector<long>.Count:
 * 4 on x64 (AVX2; also .NET 8 on AVX-512 hardware), 2 on Arm NEON, 8 with 512-bit Vector<T> enabled; MCF_VECTOR_NONE = not hardware
 * accelerated (the scalar loop alone: stop at the first block boundary behind an eligible arc).  0 = MCF_VECTOR_DEFAULT = 4. */
#define MCF_VECTOR_DEFAULT 0
#define MCF_VECTOR_NONE (-1)
/* Types/SupplyType.cs */
typedef enum mcf_supply_type { MCF_SUPPLY_GEQ = 0, MCF_SUPPLY_LEQ = 1 } mcf_supply_type;
/* Types/SolverStatus.cs:7-34 (values kept) */
typedef enum mcf_solver_status { MCF_NOT_SOLVED = 0, MCF_OPTIMAL = 1, MCF_INFEASIBLE = 2, MCF_UNBOUNDED = 3, MCF_UNBALANCED = 4 } mcf_solver_status;

/* SpanningTree.cs:53-71 */
#define MCF_STATE_UPPER (-1)
#define MCF_STATE_TREE 0
#define MCF_STATE_LOWER 1

/* "no upper bound" for mcf_ns_set_arc_bounds (the reference's default capacity, NS.cs:127,616) */
#define MCF_INF_CAP INT64_MAX

MCF_API const char *mcf_last_error(void);
MCF_API const char *mcf_version(void);
/* number of visible HIP devices (0 when there is none or the runtime cannot start); never fails */
MCF_API int mcf_device_count(void);
/* compute units of a device (0 when it cannot be asked): a resident grid is one workgroup per CU */
MCF_API int mcf_device_compute_units(int32_t device);

/* ------------------------------------------------------------------------------------------------
 * (1) Engine: entering-arc search + potential update on the device
 * ---------------------------------------------------------------------------------------------- */

typedef struct mcf_engine mcf_engine;

typedef struct mcf_engine_desc {
    int32_t node_count;       /* nodes INCLUDING the artificial root: NS.cs:137 (_nodeCount + 1) */
    int32_t arc_capacity;     /* arcs the host arrays hold: NS.cs:130 (_arcCount + 2 * _nodeCount) */
    int32_t search_arc_num;   /* arcs the pivot rules scan, [0, search_arc_num): NS.cs:722 */
    int32_t int_width;        /* 32 or 64: width of cost / potential ON THE DEVICE (the ABI is always int64) */
    int32_t rule;             /* mcf_pivot_rule */
    int32_t semantics;        /* mcf_semantics */
    int32_t block_size;       /* Block Search: 0 = the reference's default for the semantics
                                 (BSPO.cs:27-28 / NS.cs:1304-1336 with the default OptimizationConfig) */
    int32_t device;           /* HIP device ordinal */
    /* arc shard owned by this engine, [shard_begin, shard_end) within [0, search_arc_num); 0,0 = all.
     * A sharded engine answers for its shard only (mcf_engine_find_entering_local); its candidate cache (MCF_ENGINE_CANDIDATES) covers the
     * shard's arcs, so a holder asks its device only when ITS range cannot be decided on the host. */
    int32_t shard_begin, shard_end;
    int32_t scan_workgroups;  /* 0 = auto; otherwise the grid of the scan kernel */
    int32_t flags;            /* MCF_ENGINE_* */
    int32_t resident_workgroups;  /* 0 = auto (one workgroup per CU, at most 256); otherwise a cap on the resident grid: engines that share
                                     a device (arc shards rehearsed on one GPU) must all be co-resident to answer.  Workgroups are dealt
                                     to the 8 XCDs round-robin, so give k engines 8 * (32 / k) each, not 256 / k */
    int32_t vector_width;         /* MCF_SEM_OPTIMIZED + Block Search: Vector<long>.Count of the reference's host -- 2, 4, 8,
                                     MCF_VECTOR_NONE, or 0 = 4 (x64).  Ignored by every other rule / flavour */
} mcf_engine_desc;

#define MCF_ENGINE_SAMPLE_KERNEL_TIME 1   /* time every 16th scan dispatch with HIP events */
#define MCF_ENGINE_TIME_EVERY_KERNEL 2    /* time every scan dispatch (micro-benchmarks) */
#define MCF_ENGINE_NO_INLINE_UPDATE 4     /* always apply patches with the separate update kernel */
#define MCF_ENGINE_RESIDENT 8             /* (default behaviour, kept for explicitness) serve searches from ONE resident scan grid fed
                                             through a mailbox in BAR-mapped VRAM instead of one dispatch per search */
#define MCF_ENGINE_CANDIDATES 32          /* (default behaviour, kept for explicitness) Best Eligible, resident mode (register-resident arcs, or the grid of the
                                             per-arc reduced-cost layout that large instances get), sparse graph (2 m_s <= 24 n): every device search also returns a candidate list that is complete below a threshold;
                                             the following searches are answered on the host from that list plus a heap of the arcs the pivots
                                             touched, whenever that provably is the scan's answer, and the list is refreshed ahead of need
                                             (identical pivot sequence, a device round trip for about one search in seven).  DESIGN.md 3.4 */
#define MCF_ENGINE_NO_CANDIDATES 128      /* every search is a device search */
#define MCF_ENGINE_SHARE_DEVICE 64        /* several engines use this device at once (independent solves): keep the resident grid's register
                                             and LDS footprint small so that their grids are co-resident on every CU -- the grid then gathers
                                             the potentials for every request instead of keeping them in registers (~0.5 us per search) */
#define MCF_ENGINE_DISPATCH 16            /* one scan dispatch per search.  Also what an engine falls back to when it exchanges over RCCL
                                             (mcf_engine_comm_init), when kernel timing flags are set, when the platform has no host-writable
                                             VRAM, or while the device's resident slots (GPU_MAX_HW_QUEUES per process, 4) are all taken.
                                             The environment variable MCF_HIP_RESIDENT=0/1 overrides the choice. */

/* The part of OptimizationConfig (Algorithms/OptimizationTypes.cs:9-38) that the plain BlockSearchPivot consumes
 * (NS.cs:1304-1337 initial size, :1400-1438 adaptive size).  The OPTIMIZED flavour ignores it (BSPO.cs:27-28), and so
 * do the other rules.  Flag values are the reference's OptimizationFlags. */
#define MCF_OPT_NONE 0
#define MCF_OPT_ADAPTIVE_BLOCK_SIZE 1       /* OptimizationFlags.AdaptiveBlockSize */
#define MCF_OPT_SMALL_BLOCKS_FOR_DENSE 2    /* OptimizationFlags.SmallBlocksForDense */
#define MCF_OPT_REDUCED_COST_CACHING 4      /* OptimizationFlags.ReducedCostCaching: recorded, never acted on */
typedef struct mcf_block_config {
    int32_t flags;                          /* MCF_OPT_* */
    int32_t min_block_size;                 /* MinBlockSize                (default 25)    */
    int32_t max_block_size;                 /* MaxBlockSize                (default 100)   */
    int32_t consecutive_hits_before_adapt;  /* ConsecutiveHitsBeforeAdapt  (default 3)     */
    double min_block_size_ratio;            /* MinBlockSizeRatio           (default 0.125) */
    double block_size_growth_factor;        /* BlockSizeGrowthFactor       (default 1.2)   */
    double block_size_shrink_factor;        /* BlockSizeShrinkFactor       (default 0.8)   */
    double low_hit_rate_threshold;          /* LowHitRateThreshold         (default 0.05)  */
    double high_hit_rate_threshold;         /* HighHitRateThreshold        (default 0.3)   */
} mcf_block_config;
/* new OptimizationConfig() (OptimizationTypes.cs:24-38) */
MCF_API void mcf_block_config_default(mcf_block_config *c);
/* OptimizationSelector.SelectConfiguration(ProblemAnalyzer.Analyze(graph)) (Analysis/OptimizationSelector.cs:14-95,
 * Lemon/ProblemAnalyzer.cs:21-106) restricted to the fields above: what `new NetworkSimplex(g).Solve()` configures
 * itself with by default (NS.cs:90, :237-250).  Needs the original graph only (node count, arc end points). */
MCF_API int mcf_block_config_auto(mcf_block_config *c, int32_t node_count, int32_t arc_count, const int32_t *source, const int32_t *target);
/* The two pieces of BlockSearchPivot that act on the configuration, as pure functions (the engine calls them; a host that keeps
 * its own rule state may too).  mcf_block_initial_size: the constructor, NS.cs:1304-1336 -- *block_size = _blockSize,
 * *dynamic_min = _dynamicMinBlockSize; graph_node_count = the reference's _nodeCount (no artificial root).
 * mcf_block_adapt: NS.cs:1400-1438 after a successful search that examined arcs_checked arcs; counters[0] = _consecutiveLowHits,
 * counters[1] = _consecutiveHighHits. */
MCF_API int mcf_block_initial_size(const mcf_block_config *c, int32_t search_arc_num, int32_t graph_node_count, int32_t *block_size, int32_t *dynamic_min);
MCF_API int mcf_block_adapt(const mcf_block_config *c, int32_t dynamic_min, int64_t arcs_checked, int32_t *block_size, int32_t counters[2]);

/* replaces the constructor of OptimizedPivotWrapper (NS.cs:1677-1697) */
MCF_API int mcf_engine_create(mcf_engine **out, const mcf_engine_desc *desc);
MCF_API void mcf_engine_destroy(mcf_engine *e);

/* Copies the five arrays the reference pins per call (NS.cs:1701-1705): Source, Target (int32[arc_capacity]),
 * _cost (int64[arc_capacity]), State (int8[arc_capacity]), _pi (int64[node_count]). */
MCF_API int mcf_engine_upload(mcf_engine *e, const int32_t *source, const int32_t *target,
                              const int64_t *cost, const int8_t *state, const int64_t *pi);

/* State changes of ChangeFlow (NS.cs:1030-1039): at most two per pivot.  Queued; ordered before the next search. */
MCF_API int mcf_engine_patch_state(mcf_engine *e, int32_t count, const int32_t *arcs, const int8_t *states);

/* UpdatePotentials (NS.cs:1185-1209): pi[nodes[i]] += sigma.  The caller walks the thread list (it owns the tree);
 * nodes must be distinct.  Queued; ordered before the next search. */
MCF_API int mcf_engine_update_potential(mcf_engine *e, int32_t count, const int32_t *nodes, int64_t sigma);

/* Same as update_potential for callers that already hold the new values (the C++ host driver does: it keeps _pi itself):
 * pi[nodes[i]] = values[i]. */
MCF_API int mcf_engine_set_potential(mcf_engine *e, int32_t count, const int32_t *nodes, const int64_t *values);
/* Same, for a list that arrives in pieces (the subtree walk hands over what it has every few thousand nodes): may be called several
 * times between two searches; the pieces of one pivot must not repeat a node (UpdatePotentials visits every node once, NS.cs:1196-1208).
 * In resident mode the complete lines start travelling to the device at once and the grid applies them while the host is still
 * walking; the next search finishes the list. */
MCF_API int mcf_engine_append_potential(mcf_engine *e, int32_t count, const int32_t *nodes, const int64_t *values);
/* append_potential with the caller's promise that every values[i] is its node's previous potential + sigma -- which is what
 * UpdatePotentials produces: one sigma per pivot (NS.cs:1187-1190).  Layouts that keep reduced costs per arc (large sparse instances)
 * then shift those by sigma directly, for short lists inside the next search's dispatch.
 * `values` may be NULL when the potentials are bound (mcf_engine_bind_potentials): the bound array already holds them, and the host
 * driver's walk over a big subtree then writes node ids only. */
MCF_API int mcf_engine_shift_potential(mcf_engine *e, int32_t count, const int32_t *nodes, const int64_t *values, int64_t sigma);
/* The same list as RUNS of consecutive node ids: nodes first[r] .. first[r] + length[r] - 1 for every r, all moved by sigma; bound
 * potentials only (the runs carry no values).  For hosts whose node ids follow the thread order (mcf_engine_renumber_nodes): the subtree
 * of UpdatePotentials is then a few hundred runs instead of tens of thousands of nodes, the walk writes one pair per run, and the
 * register-resident candidate grid takes the pairs as they are.  May be called several times per pivot like append_potential (the runs of
 * one pivot must not overlap); engines without a use for runs expand them into the node list. */
MCF_API int mcf_engine_shift_potential_runs(mcf_engine *e, int32_t n_runs, const int32_t *first, const int32_t *length, int64_t sigma);

/* Optional: the caller keeps _pi anyway (the host solver does: sigma needs _pi[_vIn] and _pi[_uIn], NS.cs:1187-1190) -- bind that array
 * (int64[node_count], must outlive the binding; NULL unbinds) and the engine reads potentials from it instead of keeping a copy of its
 * own up to date.  Contract: when a search begins the array holds the values announced by set / append / shift_potential since the last
 * search, and it does not change while a search is in flight.  mcf_engine_update_potential (+= sigma) is not available while bound. */
MCF_API int mcf_engine_bind_potentials(mcf_engine *e, const int64_t *pi);
/* Bound potentials, layouts that keep reduced costs per arc: when a pivot moves a large part of the tree, naming the nodes costs more than
 * handing the whole array over.  mcf_engine_reload_threshold: *min_nodes = the list length from which a reload is the cheaper call for this
 * engine (0: the engine only takes lists -- no binding, potentials kept in registers / LDS, 32-bit potentials).  mcf_engine_reload_potentials:
 * "the bound array is current, `changed_nodes` of its entries differ from what you last heard" (the count only feeds the statistics); it
 * replaces every set / append / shift_potential call since the last search, is ordered before the next search like them, and the array must
 * stay unchanged until that search has been answered.  The engine copies the array to the device by itself (the binding registered it with HIP)
 * and computes every reduced cost of its shard again (NS.cs:1185-1209 moves the same values; what reaches the device is the result). */
MCF_API int mcf_engine_reload_threshold(mcf_engine *e, int32_t *min_nodes);
MCF_API int mcf_engine_reload_potentials(mcf_engine *e, int32_t changed_nodes);

/* Rewrites (source, target, cost) of arcs, e.g. artificial arcs re-pointed by a warm start. Synchronous. */
MCF_API int mcf_engine_patch_arcs(mcf_engine *e, int32_t count, const int32_t *arcs, const int32_t *source,
                                  const int32_t *target, const int64_t *cost);

/* Node ids are the host's business: the engine only ever sees them as end points of arcs and as indices into the potentials.  A host
 * that relabels its nodes (the C++ driver does, in thread order, so that its subtree walks run through memory front to back) tells the
 * engine with new_of[old id] = new id, a permutation of [0, node_count).  Between two searches; a bound potential array
 * (mcf_engine_bind_potentials) must already be in the new order, and replaces every potential change announced since the last search.
 * Arc ids, states and reduced costs are untouched, so no search result changes.  mcf_engine_can_renumber: 0 for the one layout that
 * orders its arcs by node id (MCF_HIP_BUCKET_NODES). */
/* Test aid, layouts that keep reduced costs per arc: how many of this engine's stored arcs carry a reduced cost that differs from
 * cost + pi[source] - pi[target] as the device holds them (0 for the other layouts); *first_arc (optional) = the lowest such arc. */
MCF_API int mcf_engine_check_reduced_costs(mcf_engine *e, int64_t *mismatches, int32_t *first_arc);
MCF_API int mcf_engine_can_renumber(mcf_engine *e, int32_t *yes);
MCF_API int mcf_engine_renumber_nodes(mcf_engine *e, const int32_t *new_of);

/* IFindEnteringArc.FindEnteringArc (NS.cs:1286-1289, :1699-1723): blocking.  *found = 0/1; *arc = entering arc;
 * *reduced_cost = state*(cost + pi[source] - pi[target]) of that arc.  Advances the rule's internal next_arc exactly
 * as the selected reference implementation does. */
MCF_API int mcf_engine_find_entering(mcf_engine *e, int32_t *found, int32_t *arc, int64_t *reduced_cost);
/* The same search in two halves: _begin posts it and returns, _end waits for the answer.  Between the two the host may do whatever
 * the search does not depend on (the reference's ChangeFlow arithmetic and UpdateTreeStructure of the pivot just made: the device
 * only needs the State[] writes and the potentials); patches queued in between belong to the NEXT search.  find_entering = both. */
MCF_API int mcf_engine_search_begin(mcf_engine *e);
MCF_API int mcf_engine_search_end(mcf_engine *e, int32_t *found, int32_t *arc, int64_t *reduced_cost);

/* The device half of LEMON's list rules (engines created with MCF_RULE_CANDIDATE_LIST / MCF_RULE_ALTERING_LIST only; such engines run in
 * dispatch mode -- no resident grid, no RC layout, no candidate cache, no arc shards -- and refuse find_entering / search_begin with
 * MCF_ERR_STATE).  Scans the search range [0, search_arc_num) cyclically from rq->next_arc and returns the eligible arcs
 * (state * (cost + pi[source] - pi[target]) < 0) IN SCAN ORDER with their reduced costs, up to where LEMON's loop stops:
 *   MCF_COLLECT_FIRST_N (Candidate List, major iteration, ns.h:478-507): at the limit-th eligible arc (*end_arc = that arc); a cycle with
 *     fewer returns all of them and *end_arc = next_arc.
 *   MCF_COLLECT_BLOCKS (Altering List, extension of the list, ns.h:583-610): blocks of block_size arcs, the block counter running on across
 *     the wrap; with c_j eligible arcs in block j (1-based) and `survivors` = the list length after the host re-checked its list, the scan stops
 *     after block 1 if survivors + c_1 > head_length, else after block 2 if survivors + c_1 + c_2 > 0, else after the first block that holds an
 *     eligible arc; *end_arc = the last arc of that block.  A stop that would fall behind the end of the cycle (a partial last block, no
 *     eligible arc) does not happen: every eligible arc of the cycle is returned and *end_arc = next_arc.
 * *arcs_scanned = the arcs LEMON's loop visits.  Patches queued since the last device call (any number of pivots' state writes and potential
 * lists, a node repeated across pivots included) are applied first, in the order they were given.  At most `capacity` entries are written;
 * *count is the full number, and a count above capacity fails with MCF_ERR_INVALID.  Blocking. */
#define MCF_COLLECT_FIRST_N 0
#define MCF_COLLECT_BLOCKS 1
typedef struct mcf_collect_request {
    int32_t next_arc;         /* start of the cyclic scan, [0, search_arc_num) */
    int32_t mode;             /* MCF_COLLECT_FIRST_N | MCF_COLLECT_BLOCKS */
    int32_t limit;            /* FIRST_N: eligible arcs to collect (>= 1) */
    int32_t block_size;       /* BLOCKS: arcs per block (>= 1) */
    int32_t head_length;      /* BLOCKS: LEMON's _head_length */
    int32_t survivors;        /* BLOCKS: the list length before the extension */
} mcf_collect_request;
MCF_API int mcf_engine_collect_eligible(mcf_engine *e, const mcf_collect_request *rq, int32_t capacity, int32_t *count, int32_t *arcs,
                                        int64_t *reduced_costs, int32_t *end_arc, int64_t *arcs_scanned);

/* Sharded search: the local candidate of this engine's shard, as an exchangeable 32-byte record. */
typedef struct mcf_candidate {
    int64_t reduced_cost;   /* 0 when none */
    uint32_t pos;           /* scan position (rule dependent ordering key); 0xFFFFFFFF when none */
    int32_t arc;            /* -1 when none */
    /* OPTIMIZED Block Search only (0 / 0xFFFFFFFF / -1 otherwise): the shard's best arc of the first of the reference's two ranges
     * ([next_arc, m_s), then [0, next_arc)) in which the shard has an eligible arc at all -- what enters when the reference's scan
     * runs to the end of the range (vector_width above) */
    int64_t range_cost;
    uint32_t range_pos;
    int32_t range_arc;
} mcf_candidate;
MCF_API int mcf_engine_find_entering_local(mcf_engine *e, mcf_candidate *out);
/* second half of a search posted with mcf_engine_search_begin on a sharded engine (the first half is the same call for every engine) */
MCF_API int mcf_engine_search_end_local(mcf_engine *e, mcf_candidate *out);
/* Picks the global winner among `count` candidates (one per shard) with the rule's exact tie-breaking and advances
 * next_arc on THIS engine (every rank calls it with the same gathered array).  *found / *arc as above. */
MCF_API int mcf_engine_resolve(mcf_engine *e, int32_t count, const mcf_candidate *all, int32_t *found,
                               int32_t *arc, int64_t *reduced_cost);
/* The same MINLOC + next_arc bookkeeping without an engine (stateless; *next_arc is read and advanced): what every rank
 * does with the all-gathered records.  block_size 0 = the reference default for the semantics. */
MCF_API int mcf_resolve_candidates(int32_t rule, int32_t semantics, int32_t vector_width, int32_t search_arc_num, int32_t block_size, int32_t *next_arc,
                                   int32_t count, const mcf_candidate *all, int32_t *found, int32_t *arc, int64_t *reduced_cost);
/* contiguous shard of [0, search_arc_num) for rank r of R, aligned to 4 arcs */
MCF_API int mcf_shard_range(int32_t search_arc_num, int32_t rank, int32_t world, int32_t *begin, int32_t *end);

/* Stops a running resident grid (it restarts with the next search).  Call before device-wide synchronisation. */
MCF_API int mcf_engine_park(mcf_engine *e);
MCF_API int mcf_engine_get_next_arc(mcf_engine *e, int32_t *next_arc);
MCF_API int mcf_engine_set_next_arc(mcf_engine *e, int32_t next_arc);
MCF_API int mcf_engine_get_block_size(mcf_engine *e, int32_t *block_size);
/* Block Search, PLAIN semantics: size the blocks like `new BlockSearchPivot(ns)` with this configuration (NS.cs:1304-1337;
 * graph_node_count = the reference's _nodeCount, i.e. WITHOUT the artificial root) and, with MCF_OPT_ADAPTIVE_BLOCK_SIZE, adapt
 * the size after every successful search like NS.cs:1400-1438.  The size travels with every search request.  Call before the
 * first search; a block_size given at creation (desc.block_size > 0) stays the initial size. */
MCF_API int mcf_engine_set_block_config(mcf_engine *e, const mcf_block_config *c, int32_t graph_node_count);

/* parity checks */
MCF_API int mcf_engine_download_pi(mcf_engine *e, int64_t *pi_out /* [node_count] */);
MCF_API int mcf_engine_download_state(mcf_engine *e, int8_t *state_out /* [arc_capacity] */);

typedef struct mcf_engine_stats {
    int64_t searches;             /* find_entering calls */
    int64_t scan_launches;        /* scan kernel dispatches */
    int64_t update_launches;      /* separate update kernel dispatches */
    int64_t inline_updates;       /* searches that carried their patches inside the scan dispatch */
    int64_t potential_nodes;      /* sum of update_potential counts */
    int64_t arcs_scanned;         /* sum over scan dispatches of arcs read */
    int64_t timed_scans;          /* scan dispatches timed with HIP events */
    double timed_scan_ns;         /* sum of their device durations, ns */
    double host_wait_ns;          /* host time spent waiting for device answers */
    double host_launch_ns;        /* host time spent inside launch calls */
    int32_t scan_workgroups, scan_threads;
    int64_t bytes_per_scan;       /* algorithmic bytes of one scan: SURVEY.md 8d */
    int64_t resident;             /* 1 when the engine runs in resident mode */
    int64_t resident_launches;    /* dispatches of the resident grid */
    int64_t resident_requests;    /* searches it served */
    double resident_scan_ns;      /* device clock: request seen -> record published, workgroup 0, summed over requests */
    double resident_kernel_ns;    /* HIP-event residency time of those dispatches */
    int64_t candidates;           /* 1 when the candidate cache is active */
    int64_t host_decided;         /* searches answered from the candidate list without a device request */
    int64_t arcs_checked;         /* arcs the REFERENCE's loop would have examined for the same searches: what it adds to
                                     SolverMetrics.TotalArcsChecked (NS.cs:286-290).  Only the plain BlockSearchPivot counts
                                     (NS.cs:1349-1350, :1371-1372); every other finder leaves it at 0, and so does this */
    int32_t initial_block_size, current_block_size;
    int32_t comm_ranks;           /* ranks of the RCCL communicator as ncclCommCount reports them (0: no communicator) */
    int32_t reserved;
    int64_t async_refreshes;      /* candidate lists requested ahead of need (the host kept answering while the device searched) */
    int64_t scan_bytes_read;      /* bytes one scan of THIS engine's layout has to read: bytes_per_scan for the gathering layouts, 9 per arc
                                     (state + the arc's reduced cost) in the RC layout, where the gathers moved into the potential update */
    int64_t rc_layout;            /* 1: reduced costs are kept per arc (large sparse instances) */
    int64_t rc_recomputes;        /* RC layout: potential lists naming more than a sixteenth of the nodes, after which every reduced cost of the
                                     shard was computed again instead of shifting the listed nodes' arcs one by one */
    int64_t renumberings;         /* mcf_engine_renumber_nodes calls */
    int64_t heap_compactions;     /* candidate cache: times the heap of touched arcs was swept of its outdated entries (when a list is installed, or by size) */
    int64_t rc_reloads_in_grid;   /* mcf_engine_reload_potentials carried out by the resident RC grid itself (the workgroups copy the bound array,
                                     meet at a grid-wide barrier and compute their arcs' reduced costs again) instead of stopping the grid */
    int64_t shift_grid;           /* 1: the candidate cache's grid is the one that is patched straight from the request (register-resident arcs
                                     and potentials, 64-bit, at most 131072 nodes): a pivot's one big subtree travels as node ids + sigma */
    int64_t shift_lists;          /* requests that carried such a list */
    int64_t mirror_uploads;       /* times the potentials / states in device memory were written again from the host's mirrors (that grid only
                                     reads them when it starts; the host writes them when it has left) */
    double phase_shift_ns, phase_values_ns, phase_scan_ns;   /* that grid's requests on workgroup 0's clock: fetching shift lines + setting bits /
                                     fetching and applying value entries and state writes / evaluating, reducing, publishing */
} mcf_engine_stats;
MCF_API int mcf_engine_get_stats(mcf_engine *e, mcf_engine_stats *out);
MCF_API int mcf_engine_reset_stats(mcf_engine *e);

/* Scan-only micro-benchmark on the engine's resident arrays: `reps` back-to-back scan dispatches, each timed with HIP
 * events on the engine's stream; cold != 0 streams `flush_bytes` through the caches before every repetition.
 * Results are not consumed (next_arc untouched).  avg/min in ns. */
MCF_API int mcf_engine_bench_scan(mcf_engine *e, int32_t reps, int32_t cold, int64_t flush_bytes,
                                  double *avg_ns, double *min_ns);

/* Potential-update micro-benchmark (20 bytes per node of a list; 12 with 32-bit potentials): the update kernel that dispatch
 * mode runs for long lists -- update_kernel, or update_rc_kernel where reduced costs are kept per arc (then the list's nodes' arc lists are
 * walked and shifted too: + 8 bytes per node for its list bounds and 20 per arc-list entry) -- over `count` distinct nodes, `reps` launches
 * each timed with HIP events.  *bytes = algorithmic bytes of one launch.  The engine's arrays are unchanged when the call returns. */
MCF_API int mcf_engine_bench_update(mcf_engine *e, int32_t count, int32_t reps, double *avg_ns, double *min_ns, int64_t *bytes);

/* Whole-search micro-benchmark: host wall time from posting / launching a search to its merged answer, `reps` times back to back without
 * patches (the candidate cache is bypassed by nothing here: an engine with the cache answers from it).  avg/min in ns. */
MCF_API int mcf_engine_bench_search(mcf_engine *e, int32_t reps, double *avg_ns, double *min_ns);

/* RCCL exchange for sharded engines: one ncclAllGather per pivot.  A resident engine whose grid leaves at least 8 CUs alone
 * (desc.resident_workgroups) KEEPS its grid and its candidate cache: the collective runs on a stream of its own and moves 64-byte records
 * {number, candidate, number} that lie in pinned host memory -- the host writes its own, polls for the others', nothing is copied or
 * synchronised per pivot.  Any other engine serves its searches with one dispatch each from then on; called without a posted search it
 * folds the scan's records on the device into the collective's send buffer (rounds 1-2), after mcf_engine_search_begin it exchanges like a
 * resident one.  id_out/id: the 128-byte ncclUniqueId, created on rank 0 and broadcast by the caller (torch.distributed). */
MCF_API int mcf_comm_unique_id(uint8_t id_out[128]);
MCF_API int mcf_engine_comm_init(mcf_engine *e, const uint8_t id[128], int32_t rank, int32_t world);
/* find_entering_local + all-gather + resolve in one call */
MCF_API int mcf_engine_find_entering_sharded(mcf_engine *e, int32_t *found, int32_t *arc, int64_t *reduced_cost);

/* Host exchange for sharded engines ("per-GPU result slots reduced by the host"): the ranks of ONE node put their
 * 32-byte candidates into POSIX shared memory and read each other's -- an all-gather without a collective library, a fraction of a
 * microsecond per pivot where one ncclAllGather of 32 bytes costs tens.  name: the same on every rank, "/something" (shm_open);
 * all ranks must have returned from mcf_exchange_open (any barrier of the caller's) before the first mcf_exchange_all_gather. */
typedef struct mcf_exchange mcf_exchange;
MCF_API int mcf_exchange_open(mcf_exchange **out, const char *name, int32_t rank, int32_t world);
MCF_API void mcf_exchange_close(mcf_exchange *x);
MCF_API int mcf_exchange_all_gather(mcf_exchange *x, const mcf_candidate *mine, mcf_candidate *all /* [world] */);

/* ------------------------------------------------------------------------------------------------
 * (2) Host driver: NetworkSimplex restated (mirror of the public surface of NS.cs)
 * ---------------------------------------------------------------------------------------------- */

typedef struct mcf_ns mcf_ns;

/* NetworkSimplex(IGraph graph) (NS.cs:119-148): the graph is given as flat arc lists, ids = positions */
MCF_API int mcf_ns_create(mcf_ns **out, int32_t node_count, int32_t arc_count, const int32_t *source, const int32_t *target);
MCF_API void mcf_ns_destroy(mcf_ns *s);
MCF_API int mcf_ns_set_arc_bounds(mcf_ns *s, int32_t arc, int64_t lower, int64_t upper);   /* NS.cs:153-164 */
MCF_API int mcf_ns_set_arc_cost(mcf_ns *s, int32_t arc, int64_t cost);                     /* NS.cs:169-178 */
MCF_API int mcf_ns_set_node_supply(mcf_ns *s, int32_t node, int64_t supply);               /* NS.cs:183-192 */
/* bulk forms of the three setters (NULL = keep defaults: lower 0, upper INF, cost 0, supply 0: NS.cs:614-621) */
MCF_API int mcf_ns_set_problem(mcf_ns *s, const int64_t *lower, const int64_t *upper, const int64_t *cost, const int64_t *supply);
MCF_API int mcf_ns_set_supply_type(mcf_ns *s, int32_t type);                               /* NS.cs:197-201 */
MCF_API int mcf_ns_set_pivot_rule(mcf_ns *s, int32_t rule);                                /* NS.cs:206-210; refuses 3 and 4 like NS.cs:884 */
/* LEMON's Candidate List (3) or Altering List (4) pivot rule (lemon/network_simplex.h:415-635 with LEMON's fixed parameters), run on this
 * host driver: minor iterations, the re-check of the list and the partial sort happen here, the major scans on the device
 * (mcf_engine_collect_eligible, one blocking device call each).  Any other value fails with MCF_ERR_INVALID; a later mcf_ns_set_pivot_rule replaces it.
 * The list rules ignore mcf_ns_enable_optimized_pivot, the vector width, the OptimizationConfig and auto-configuration; sharding of any kind
 * together with a list rule fails at mcf_ns_prepare with MCF_ERR_INVALID. */
MCF_API int mcf_ns_set_list_pivot_rule(mcf_ns *s, int32_t rule);
MCF_API int mcf_ns_enable_optimized_pivot(mcf_ns *s, int32_t enable);                      /* NS.cs:532-535 */
/* Vector<long>.Count of the machine whose EnableOptimizedPivot(true) Block Search is reproduced (mcf_engine_desc.vector_width; the
 * reference has no setter, it reads the property: BSPO.cs:74, :115).  Default 4 = x64. */
MCF_API int mcf_ns_set_vector_width(mcf_ns *s, int32_t vector_width);
/* SetOptimizationConfig (NS.cs:557-561; switches auto-configuration off), EnableOptimizations (NS.cs:549-552),
 * SetAutoConfiguration (NS.cs:567-570; the reference's default is ON, and so is this library's) */
MCF_API int mcf_ns_set_optimization_config(mcf_ns *s, const mcf_block_config *config);
MCF_API int mcf_ns_enable_optimizations(mcf_ns *s, int32_t flags);
MCF_API int mcf_ns_set_auto_configuration(mcf_ns *s, int32_t enable);
/* device-side options that have no counterpart in the reference */
MCF_API int mcf_ns_set_device(mcf_ns *s, int32_t device, int32_t int_width /* 32, 64, 0 = narrowest that is safe */,
                              int32_t block_size /* 0 = reference default */, int32_t engine_flags);
/* Several independent solvers of one process on one device (one host thread each): every solver's resident grid gets
 * `resident_workgroups` workgroups -- 256 / K for K solvers -- so that the grids sit on compute units of their own (a workgroup of
 * these grids fills a CU) instead of competing for the same ones; 0 = the whole device (default).  An instance whose arcs no longer
 * fit the registers of so few workgroups keeps reduced costs per arc (the layout of the large instances); the pivots are the same
 * either way.  A process runs at most GPU_MAX_HW_QUEUES (HIP's variable, default 4; read when HIP starts) resident grids per device:
 * set it to K or more before the first HIP call, further solvers serve their searches with one dispatch each. */
MCF_API int mcf_ns_set_device_share(mcf_ns *s, int32_t resident_workgroups);
/* shard the arc scan over `world` ranks exchanging over RCCL (every rank runs the same host loop) */
MCF_API int mcf_ns_set_sharding(mcf_ns *s, const uint8_t nccl_id[128], int32_t rank, int32_t world);

/* the same sharding with the candidates exchanged through shared memory (mcf_exchange_*) instead of RCCL: every rank runs the same
 * host loop, its engine keeps its arc shard in a resident grid; exchange_name as for mcf_exchange_open */
MCF_API int mcf_ns_set_sharding_host(mcf_ns *s, const char *exchange_name, int32_t rank, int32_t world);
/* the same sharding inside ONE process: `shards` engines, one per entry of devices[] (entries may repeat: arc shards rehearsed on fewer
 * GPUs), driven by this solver's single host thread, which posts every search to all of them and reduces their answers itself */
MCF_API int mcf_ns_set_shard_group(mcf_ns *s, int32_t shards, const int32_t *devices);

/* Optional: everything Solve() does before its pivot loop (CheckBounds, TransformToStandardForm, Initialize, creating the
 * engine and copying the SoA arrays into HBM).  mcf_ns_solve() calls it when the caller has not. */
MCF_API int mcf_ns_prepare(mcf_ns *s);
/* Solve() (NS.cs:215-411).  *status receives a mcf_solver_status. */
MCF_API int mcf_ns_solve(mcf_ns *s, int32_t *status);
MCF_API int mcf_ns_status(mcf_ns *s, int32_t *status);                                     /* NS.cs:470 */
MCF_API int mcf_ns_get_flow(mcf_ns *s, int32_t arc, int64_t *flow);                        /* NS.cs:416-429 */
MCF_API int mcf_ns_get_potential(mcf_ns *s, int32_t node, int64_t *potential);             /* NS.cs:434-447 */
MCF_API int mcf_ns_get_total_cost(mcf_ns *s, int64_t *cost);                               /* NS.cs:452-465 */
MCF_API int mcf_ns_get_flows(mcf_ns *s, int64_t *flow_out /* [arc_count] */);
MCF_API int mcf_ns_get_potentials(mcf_ns *s, int64_t *pi_out /* [node_count] */);
MCF_API int mcf_ns_get_arc_upper_bound(mcf_ns *s, int32_t arc, int64_t *upper);            /* NS.cs:519-527 (reduced after Solve, D11) */

/* SolverMetrics (OptimizationTypes.cs:43-70), same three phase buckets */
typedef struct mcf_ns_metrics {
    int64_t iterations;
    double total_solve_us, pivot_search_us, tree_update_us, potential_update_us;
    double setup_us;              /* mcf_ns_prepare: standard form, start basis, engine creation, upload */
    double loop_us;               /* the pivot loop alone (inputs already resident in HBM) */
    int32_t search_arc_num, block_size, int_width, reserved;
    int64_t degenerate_pivots;
    int64_t potential_nodes;      /* nodes whose potential the host walked over: the moved subtree's, or -- inside mcf_ns_solve with 64-bit engines --
                                     the REST of the tree's when that is the smaller side (reduced costs only see differences, so moving
                                     everything else by -sigma is the same search; the common offset is taken out before Solve() returns) */
    mcf_engine_stats engine;
    /* the remaining SolverMetrics fields (OptimizationTypes.cs:53-59), filled like NS.cs:262-270, :344-357 */
    int32_t initial_block_size, final_block_size;      /* Block Search, plain flavour; 0 otherwise (NS.cs:263-270, :348-355) */
    int64_t total_arcs_checked;                        /* see mcf_engine_stats.arcs_checked */
    double average_arcs_checked_per_pivot;
    int32_t baseline_iterations;                       /* (int)(sqrt(m_s) * n * 0.5), NS.cs:276 */
    int32_t config_flags;                              /* MCF_OPT_* in force during the solve (auto-configured or set) */
    double iteration_ratio;
    int32_t reference_selects_cached_pivot;            /* 1: with this configuration the reference would run CachedBlockSearchPivot
                                                          (NS.cs:855-883), which this library does not reproduce (SURVEY.md 8a row a8:
                                                          documented failure, stale cache entries); the plain Block Search ran instead */
    int32_t reserved2;
} mcf_ns_metrics;
MCF_API int mcf_ns_get_metrics(mcf_ns *s, mcf_ns_metrics *out);                            /* NS.cs:584-587 */
/* Counters of the last Solve() with a list rule (all zero after a solve with rules 0-2).  searches = major_scans + host_answered. */
typedef struct mcf_list_rule_stats {
    int32_t rule;                 /* MCF_RULE_CANDIDATE_LIST / MCF_RULE_ALTERING_LIST, 0 when the last solve ran another rule */
    int32_t list_length;          /* Candidate List: _list_length; Altering List: _head_length + _block_size (the list's capacity) */
    int32_t minor_limit;          /* Candidate List: _minor_limit */
    int32_t block_size;           /* Altering List: _block_size */
    int32_t head_length;          /* Altering List: _head_length */
    int32_t reserved;
    int64_t searches;             /* findEnteringArc calls */
    int64_t major_scans;          /* searches that called the device (mcf_engine_collect_eligible) */
    int64_t host_answered;        /* searches answered from the host's list without a device call */
    int64_t device_arcs_read;     /* arcs the device's count passes read (the whole search range per major scan) */
    int64_t lemon_arcs_scanned;   /* arcs LEMON's loops visit in those major scans */
    int64_t collected;            /* eligible arcs the major scans returned */
    double collect_us;            /* host wall time inside mcf_engine_collect_eligible */
} mcf_list_rule_stats;
MCF_API int mcf_ns_get_list_rule_stats(mcf_ns *s, mcf_list_rule_stats *out);
/* measurement aid: Solve() stops after max_pivots pivots and reports MCF_NOT_SOLVED (0 = no limit) */
MCF_API int mcf_ns_set_pivot_limit(mcf_ns *s, int64_t max_pivots);
/* optional pivot trace: entering arc of every pivot of the next Solve() (for parity tests) */
MCF_API int mcf_ns_set_trace(mcf_ns *s, int32_t *trace, int64_t capacity);
MCF_API int mcf_ns_get_trace_length(mcf_ns *s, int64_t *length);

/* Stepwise host side, the part a C# host keeps (NS.cs:253, :319-340, :360-388).  None of these searches for an
 * entering arc; they let the sequential part be driven (and tested) with entering arcs supplied by the caller. */
MCF_API int mcf_ns_begin(mcf_ns *s, int32_t *status);            /* CheckBounds + TransformToStandardForm + Initialize */
MCF_API int mcf_ns_apply_pivot(mcf_ns *s, int32_t entering_arc, int32_t *unbounded);   /* FindJoinNode .. UpdatePotentials */
MCF_API int mcf_ns_finish(mcf_ns *s, int32_t *status);           /* CheckFeasibility + lower-bound restore */
/* Measurement / test aid: `count` pivots with the given entering arcs applied back to back, no engine involved -- the sequential half
 * alone, with the walk aids mcf_ns_solve uses (smaller_side != 0: shift whichever side of the tree is smaller; renumber_every > 0: relabel
 * the nodes in thread order whenever the walks since the last relabelling covered that many times the node count).  Fills the metrics'
 * tree_update_us / potential_update_us / loop_us (setup_us = time spent relabelling).  Node ids are the caller's again when it returns. */
MCF_API int mcf_ns_replay(mcf_ns *s, const int32_t *arcs, int64_t count, int32_t smaller_side, double renumber_every);
/* debug aid: after the first relabelling the driver keeps one bit per node, set where the thread list leaves the id order (Thread[a] != a + 1),
 * and its walks take their run ends from it.  Recomputes every bit from the thread list and counts the differences (0 = the bitmap is
 * current; also 0 while there is no bitmap yet). */
MCF_API int mcf_ns_check_thread_breaks(mcf_ns *s, int64_t *mismatches);
/* views of the internal SoA after mcf_ns_begin (valid until destroy); sizes: arc_capacity / node_count + 1 */
MCF_API int mcf_ns_internal(mcf_ns *s, int32_t *search_arc_num, int32_t *arc_capacity, const int32_t **source,
                            const int32_t **target, const int64_t **cost, const int8_t **state, const int64_t **pi);
/* views of the spanning tree after mcf_ns_begin / mcf_ns_apply_pivot (valid until the next pivot; node arrays: node_count + 1 entries, the last
 * one is the artificial root; arc arrays: arc_capacity entries): Parent, Pred, SuccNum, PredDir of SpanningTree.cs:10-35 and _flow / _upper.
 * For tools that study the cycle search (NS.cs:925-1010) on real trees; any pointer may be NULL. */
MCF_API int mcf_ns_tree(mcf_ns *s, const int32_t **parent, const int32_t **pred_arc, const int32_t **succ_num, const int8_t **pred_dir,
                        const int64_t **flow, const int64_t **upper);
/* test aid: mcf_engine_check_reduced_costs summed over this solver's engines (after Solve()) */
MCF_API int mcf_ns_check_reduced_costs(mcf_ns *s, int64_t *mismatches);
/* what the last mcf_ns_apply_pivot changed: the engine calls a host would make.  *nodes lists the *n_nodes nodes whose potential moved by
 * *sigma, whatever form the walk wrote them down in (runs of consecutive ids are expanded here; valid until the next pivot).  After a
 * walk that wrote no list (a reload of _pi, inside mcf_ns_solve only) *nodes is NULL and *n_nodes still counts the nodes. */
MCF_API int mcf_ns_last_pivot(mcf_ns *s, int32_t *n_state, int32_t arcs[2], int8_t states[2], int32_t *n_nodes,
                              const int32_t **nodes, int64_t *sigma);

/* ------------------------------------------------------------------------------------------------
 * (3) Solution validator on the device: the checks of
 *     src/MinCostFlow.Core/Lemon/Validation/SolutionValidator.cs as reductions over the arcs and the nodes.
 *     Same arithmetic as the reference (C# long, unchecked: it wraps).  Instead of message strings the result
 *     carries, per check, the number of messages the reference would add and the lowest arc / node id among them.
 * ---------------------------------------------------------------------------------------------- */
typedef enum mcf_validation_kind {
    MCF_VAL_CONSERVATION = 0,   /* node: net flow vs supply under the supply type        SolutionValidator.cs:75-99   */
    MCF_VAL_LOWER = 1,          /* arc : flow < lower                                    :111-115 */
    MCF_VAL_UPPER = 2,          /* arc : flow > upper                                    :117-121 */
    MCF_VAL_SLACK_POS = 3,      /* arc : reduced cost > 0 but flow != lower              :164-168 */
    MCF_VAL_SLACK_NEG = 4,      /* arc : reduced cost < 0 but flow != upper              :170-174 */
    MCF_VAL_NODE_DUAL = 5,      /* node: sign of pi against the supply type              :203-207, :218-222 */
    MCF_VAL_NODE_SLACK = 6,     /* node: pi != 0 but net flow != supply                  :208-213, :223-228 */
    MCF_VAL_OBJECTIVE = 7,      /* sum flow*cost != reported cost                        :257-262 */
    MCF_VAL_DUAL_COST = 8,      /* dual cost != reported cost                            :333-339 */
    MCF_VAL_STATUS = 9,         /* solver status is not Optimal (nothing else is checked) :28-33 */
    MCF_VAL_KINDS = 10
} mcf_validation_kind;
/* a third supply type for the validator only: the reference's `_ =>` equality branch (SolutionValidator.cs:83) */
#define MCF_SUPPLY_EQ 2

typedef struct mcf_validation {
    int32_t valid;                      /* ValidationResult.IsValid: no message at all */
    int32_t supply_type;
    int64_t objective;                  /* calculatedCost (:232-255) */
    int64_t dual_cost;                  /* ValidationResult.DualCost (:270-331) */
    int64_t errors[MCF_VAL_KINDS];
    int64_t first[MCF_VAL_KINDS];       /* lowest failing arc / node id, -1 when the check passes */
    double kernel_us;                   /* HIP events around one run: memset + validate_arcs + validate_nodes + validate_fold */
    int64_t algorithmic_bytes;          /* 40 B per arc + 40 B per node, see DESIGN.md */
} mcf_validation;

typedef struct mcf_validator mcf_validator;
MCF_API int mcf_validator_create(mcf_validator **out, int32_t device, int32_t node_count, int32_t arc_count);
MCF_API void mcf_validator_destroy(mcf_validator *v);
/* Host arrays, copied.  The network (first six arrays) and the solution (flow, pi) may be uploaded separately:
 * pass NULL for everything that stays as it is on the device. */
MCF_API int mcf_validator_upload(mcf_validator *v, const int32_t *source, const int32_t *target, const int64_t *lower,
                                 const int64_t *upper, const int64_t *cost, const int64_t *supply, const int64_t *flow,
                                 const int64_t *pi);
MCF_API int mcf_validator_run(mcf_validator *v, int32_t supply_type, int64_t reported_cost, mcf_validation *out);
/* SolutionValidator(graph, solver).Validate() for a solver of this library: reads what the reference's validator
 * reads through the solver's getters (GetFlow, GetPotential, GetArcLowerBound = the original lower bound,
 * GetArcUpperBound = the bound as mutated by Solve(), NS.cs:519-527, difference D11) */
MCF_API int mcf_ns_validate(mcf_ns *s, mcf_validation *out);

/* ------------------------------------------------------------------------------------------------
 * (4) Problem sources (build-owned; the reference ships NETGEN outputs but no generator: SURVEY.md F6, 8d)
 * ---------------------------------------------------------------------------------------------- */

typedef struct mcf_problem {
    int32_t node_count, arc_count;
    int32_t *source, *target;          /* [arc_count], 0-based */
    int64_t *lower, *upper, *cost;     /* [arc_count] */
    int64_t *supply;                   /* [node_count] */
} mcf_problem;
MCF_API void mcf_problem_free(mcf_problem *p);
/* NETGEN-like transshipment network: SplitMix64(seed); n_src sources / n_snk sinks, total supply 1000*n_src,
 * skeleton chains source -> ... -> sink (cost = max_cost, capacity >= the chain's supply) make it feasible;
 * remaining arcs uniform; arcs are emitted grouped by tail node like NETGEN's output files. */
MCF_API int mcf_gen_netgen_like(mcf_problem *out, uint64_t seed, int32_t nodes, int32_t arcs, int32_t n_src,
                                int32_t n_snk, int64_t min_cost, int64_t max_cost, int64_t min_cap, int64_t max_cap);
/* complete bipartite assignment n x n, cost U[min_cost,max_cost], supply +1/-1, bounds [0,1]
 * (shape of src/MinCostFlow.Problems/Generators/ProblemGenerator.cs:194-232) */
MCF_API int mcf_gen_assignment(mcf_problem *out, uint64_t seed, int32_t n, int64_t min_cost, int64_t max_cost);
/* DIMACS min-cost-flow reader / writer (Loaders/DimacsReader.cs:36-147; lemon/dimacs.h:129-186) */
MCF_API int mcf_dimacs_read(mcf_problem *out, const char *path);
MCF_API int mcf_dimacs_write(const mcf_problem *p, const char *path);
/* .sol files (Loaders/SolutionLoader.cs:59-176 reader, :186-210 writer): "s COST", "f ARC FLOW" (0-based arc id, what the
 * reference writes) or "f SRC DST FLOW" (1-based end points, what its bundled Gurobi solutions hold), "p NODE POTENTIAL".
 * The reader fills flow[arc_count] (and pi[node_count] when given); end-point flows are split over parallel arcs by
 * increasing cost.  pi may be NULL in both. */
MCF_API int mcf_solution_write(const char *path, int64_t cost, int32_t arc_count, const int64_t *flow, int32_t node_count, const int64_t *pi);
MCF_API int mcf_solution_read(const char *path, const mcf_problem *p, int64_t *cost, int32_t *has_cost, int64_t *flow, int64_t *pi, int32_t *has_pi);

/* ------------------------------------------------------------------------------------------------
 * (4) Batch: many small independent instances, each one solved ENTIRELY on the device
 * ----------------------------------------------------------------------------------------------
 * One workgroup (one wave) per instance carries out whole pivots -- search, cycle, flows, tree surgery, potentials -- with no host
 * involvement between them.  An instance's state lives in a workspace in global memory; instances whose workspace fits
 * the LDS a workgroup may have run their pivots there.  The host sets every instance up (bounds check, standard form, start basis) and
 * finishes it (feasibility, lower bounds) with the code mcf_ns uses.  Results are bit-identical to mcf_ns_solve with the same rule and
 * EnableOptimizedPivot(false): same entering arc at every pivot.
 * Limits: at most MCF_BATCH_MAX_ARCS arcs and MCF_BATCH_MAX_NODES nodes per instance (bigger problems are what mcf_ns_solve is for),
 * at most MCF_BATCH_MAX_INSTANCES instances; rules First Eligible, Best Eligible, Block Search in MCF_SEM_PLAIN (Block Search as
 * `new NetworkSimplex(g).Solve()` runs it: auto-configured, adaptive block size).  mcf_batch_create refuses MCF_SEM_OPTIMIZED, the list
 * rules and sharding with MCF_ERR_INVALID. */
#define MCF_BATCH_MAX_ARCS 65536
#define MCF_BATCH_MAX_NODES 32768
#define MCF_BATCH_MAX_INSTANCES 65536
#define MCF_BATCH_SHARDED 1              /* mcf_batch_desc.flags: refused (a batch runs on one device) */

typedef struct mcf_batch mcf_batch;
typedef struct mcf_batch_desc {
    int32_t device;               /* HIP device ordinal */
    int32_t pivot_rule;           /* MCF_RULE_FIRST_ELIGIBLE / _BEST_ELIGIBLE / _BLOCK_SEARCH */
    int32_t semantics;            /* MCF_SEM_PLAIN (0 = the same) */
    int32_t reserved;
    int64_t pivot_limit;          /* per instance, always on: 0 = 64 * (arc_count + 2 * node_count) + 1024.  An instance that reaches it
                                     reports MCF_NOT_SOLVED; the batch call itself returns MCF_OK */
    int32_t pivots_per_launch;    /* a launch runs every unfinished instance for at most this many pivots, writes the state back and
                                     returns; the host relaunches.  0 = default */
    int32_t trace_capacity;       /* entering arcs recorded per instance, 0 = none */
    int32_t flags;                /* MCF_BATCH_* */
} mcf_batch_desc;
typedef struct mcf_batch_stats {
    int64_t instances;            /* added */
    int64_t lds_instances;        /* ran their pivots in LDS */
    int64_t global_instances;     /* ran them in place on the workspace */
    int64_t launches;             /* kernel launches of the last mcf_batch_solve */
    int64_t total_pivots;
    int64_t workspace_bytes;      /* the slab in device memory */
    int64_t lds_bytes_max;        /* the largest dynamic LDS a launch asked for */
    double kernel_ns;             /* host clock round the launches, each ended by a device synchronise */
    double host_ns;               /* the rest of the call: packing, copies, finishing */
} mcf_batch_stats;

MCF_API int mcf_batch_create(mcf_batch **out, const mcf_batch_desc *desc);
MCF_API void mcf_batch_destroy(mcf_batch *b);
/* Adds one instance (everything is copied); *index = its number in the batch (may be NULL).  Validates like mcf_ns_create +
 * mcf_ns_set_problem (lower / upper / cost / supply may be NULL: 0 / unbounded / 0 / 0); supply_type per instance. */
MCF_API int mcf_batch_add(mcf_batch *b, int32_t node_count, int32_t arc_count, const int32_t *source, const int32_t *target,
                          const int64_t *lower, const int64_t *upper, const int64_t *cost, const int64_t *supply, int32_t supply_type,
                          int32_t *index);
/* Solves every instance on the device.  Single-shot like Solve() (new costs: mcf_batch_resolve below).  MCF_ERR_NO_DEVICE without a GPU. */
MCF_API int mcf_batch_solve(mcf_batch *b);
/* TEST HOOK, not a supported solver: the same step functions (csrc/batch_step.hip.h) run on the host with one lane, so that the tree
 * surgery can be put under a host sanitizer or debugger.  Takes the place of mcf_batch_solve for this batch. */
MCF_API int mcf_batch_run_on_host(mcf_batch *b);
/* Per instance, in the caller's numbering and the C# sign convention -- what mcf_ns_status / mcf_ns_get_* return.  MCF_ERR_STATE before
 * a solve; total cost, flows and potentials also unless the instance is optimal (NS.cs:418-421). */
MCF_API int mcf_batch_get_status(mcf_batch *b, int32_t index, int32_t *status);
MCF_API int mcf_batch_get_total_cost(mcf_batch *b, int32_t index, int64_t *cost);
MCF_API int mcf_batch_get_flows(mcf_batch *b, int32_t index, int64_t *out);          /* [arc_count] */
MCF_API int mcf_batch_get_potentials(mcf_batch *b, int32_t index, int64_t *out);     /* [node_count] */
MCF_API int mcf_batch_get_pivots(mcf_batch *b, int32_t index, int64_t *pivots);
/* copies min(capacity, recorded) entering arcs, *length = recorded (out may be NULL with capacity 0) */
MCF_API int mcf_batch_get_trace(mcf_batch *b, int32_t index, int32_t *out, int64_t capacity, int64_t *length);
MCF_API int mcf_batch_get_stats(mcf_batch *b, mcf_batch_stats *out);

/* ---- Re-solving a solved batch with new arc costs ("Re-solve").
 * After a cost change the basis a solve ended with is still primal feasible: only the potentials and the optimality test change.  The
 * batch keeps every instance's state in device memory until mcf_batch_destroy, so a re-solve moves the new costs, not the instances.
 * mcf_batch_* takes new costs only: it sets every instance up on the host, and new supplies, bounds or topology need a new batch there
 * (deliberately: the handles whose data live on the device, mcf_ubatch_* and mcf_rbatch_*, re-solve with new supplies and bounds from the
 * kept basis too, see mcf_ubatch_resolve_data; the topology is fixed per handle everywhere).  mcf_batch_solve, mcf_batch_run_on_host and
 * mcf_batch_add on a solved batch stay MCF_ERR_STATE.
 *
 * Per instance whose costs were set since the last solve:
 *   - infeasible by its bounds (it never reached the device): stays MCF_INFEASIBLE with 0 pivots;
 *   - last status MCF_OPTIMAL and no flow left on an artificial arc: WARM.  Tree, State[] and flows stay; the artificial arcs get the cost `(max |cost| + 1) * node_count` of
 *     the new costs; the potentials are recomputed from the basis; the rule starts as at a cold start (_nextArc 0, the initial block size,
 *     adaptation counters 0); pivot count and trace restart and describe this re-solve; the pivot limit applies to it;
 *   - any other last status (Infeasible after pivots, Unbounded, Not Solved at the pivot limit): COLD, from the start basis: pivot for
 *     pivot what a fresh batch gives with these costs.  Also cold: Optimal WITH flow on an artificial arc.  That is the reference's answer
 *     to supplies that do not sum to zero the wrong way (a surplus under GEQ, a deficit under LEQ): it checks the root links only, the
 *     answer does not conserve flow, and since artificial arcs never enter the basis again, which node keeps the surplus -- and with it
 *     the total cost -- depends on the pivot path.
 * Every other instance keeps status, cost, flows, potentials, pivot count and trace exactly.
 * LIMIT.  The reference answers an uncapacitated negative cycle Optimal with a wrapped cost, and an eligible arc of capacity zero
 * Unbounded; both depend on the path the pivots take, so a warm re-solve of such an instance may answer differently from a cold solve.
 * For instances whose arcs all have finite, positive capacity after the lower-bound shift (upper - lower in [1, MCF_INF_CAP)), status and
 * total cost are those of a cold solve with the new costs; flows and potentials are an optimal pair, not necessarily the cold solve's. */
typedef struct mcf_batch_resolve_stats {
    int64_t warm_instances;       /* changed, last status Optimal (no artificial flow): re-solved from the kept basis */
    int64_t cold_instances;       /* changed, anything else: from the start basis (incl. the ones infeasible by their bounds) */
    int64_t untouched_instances;  /* no new costs: left exactly as they were */
    int64_t launches;             /* batch_kernel launches of this re-solve */
    int64_t total_pivots;         /* of the instances that ran */
    int64_t bytes_uploaded;       /* slots, cost arrays (warm) and whole workspaces (cold, or stale on the device); the 4-byte instance
                                     ids that go with every round of launches are not counted */
    int64_t bytes_downloaded;     /* slots after every round, the changing part of the instances that ran, their traces */
    double kernel_ns;             /* host clock round the launches, each round ended by a synchronising copy */
    double host_ns;               /* the rest of the call */
} mcf_batch_resolve_stats;
/* New costs for instance `index` (copied; [arc_count]).  Only after a solve of any kind: before one, costs come with mcf_batch_add
 * (MCF_ERR_STATE).  May be called several times before a re-solve: the last call wins.  The instance's results are the old ones until
 * the re-solve. */
MCF_API int mcf_batch_set_costs(mcf_batch *b, int32_t index, const int64_t *cost);
/* Re-solves every instance with new costs on the device.  MCF_ERR_STATE before the first solve (of either kind).  With no changed
 * instance: MCF_OK, nothing is launched.  MCF_ERR_NO_DEVICE without a GPU; the batch is left as it was.  May be repeated, and mixed with
 * mcf_batch_rerun_on_host in any order: the results are the same. */
MCF_API int mcf_batch_resolve(mcf_batch *b);
/* TEST HOOK like mcf_batch_run_on_host, not a supported solver: the same re-solve with one lane on the CPU. */
MCF_API int mcf_batch_rerun_on_host(mcf_batch *b);
/* what the last mcf_batch_resolve / mcf_batch_rerun_on_host did (all zero before one) */
MCF_API int mcf_batch_get_resolve_stats(mcf_batch *b, mcf_batch_resolve_stats *out);

/* ---- Uniform batch: `count` instances of ONE topology, problem data in and results out where they are ("Uniform batch").
 * mcf_batch_* above sets every instance up and finishes it on one host thread, and every number passes through the host.  Where the
 * instances share their graph and differ in costs, supplies and bounds, all of that runs on the device: one launch sets every
 * instance up from the caller's arrays (bounds check, standard form, start basis), the launches of mcf_batch_solve carry the pivots
 * (the same kernel), one launch writes status, pivot count, total cost, flows, potentials and trace into the caller's rows.  With
 * MCF_MEM_DEVICE nothing that scales with the arcs or the nodes crosses the bus in a call (the topology goes up once per handle, with
 * its first device call, and is not counted in the statistics of a call).
 * Results are those of mcf_batch_*: bit for bit what mcf_batch_add + mcf_batch_solve give for the same instances.  Workspaces sit at a
 * fixed stride (the footprint of an instance whose every node needs an artificial arc), so the whole batch runs in ONE tier, LDS or
 * global memory, by that stride; both tiers give the same results.
 * Limits and refusals are mcf_batch_create's and mcf_batch_add's: the three rules in MCF_SEM_PLAIN, MCF_BATCH_MAX_ARCS / _NODES /
 * _INSTANCES, end points validated at create. */
#define MCF_MEM_HOST 0
#define MCF_MEM_DEVICE 1

typedef struct mcf_ubatch mcf_ubatch;
typedef struct mcf_ubatch_desc {
    int32_t device;               /* as mcf_batch_desc, field for field ... */
    int32_t pivot_rule;
    int32_t semantics;
    int32_t reserved;
    int64_t pivot_limit;          /* The output rows of an instance stopped by it (MCF_NOT_SOLVED) are zero.  Its trace row holds `limit`
                                     entries (min(limit, trace_capacity)), zeros behind them.  A re-solve of a stopped instance starts cold. */
    int32_t pivots_per_launch;
    int32_t trace_capacity;
    int32_t flags;
    int32_t node_count;           /* ... then the topology every instance shares */
    int32_t arc_count;
    int32_t count;                /* instances, >= 0 */
    const int32_t *source;        /* [arc_count], HOST memory, copied and validated by mcf_ubatch_create */
    const int32_t *target;
} mcf_ubatch_desc;
typedef struct mcf_ubatch_io {
    int32_t memory;               /* MCF_MEM_HOST / MCF_MEM_DEVICE: where EVERY pointer below points (device = mcf_ubatch_desc.device) */
    int32_t supply_type;          /* MCF_SUPPLY_GEQ / _LEQ, for every instance of this call */
    const int64_t *lower;         /* [arc_count] per instance; NULL = 0 */
    const int64_t *upper;         /* NULL = uncapacitated; MCF_INF_CAP as in mcf_ns_set_problem */
    const int64_t *cost;          /* NULL = 0 */
    const int64_t *supply;        /* [node_count] per instance; NULL = 0 */
    int64_t lower_stride, upper_stride, cost_stride, supply_stride;     /* ELEMENTS between instance i and i + 1; 0 = one array shared by all */
    const uint8_t *changed;       /* mcf_ubatch_resolve / _rerun_on_host only: [count], nonzero = re-solve this instance; NULL = all */
    /* results, any may be NULL.  Rows of instances that are not MCF_OPTIMAL are zero-filled (total cost 0); status, pivots and trace are
     * always written, a trace row is zero behind min(pivots, trace_capacity) */
    int32_t *status;              /* [count] */
    int64_t *pivots;              /* [count] */
    int64_t *total_cost;          /* [count] */
    int64_t *flows;               /* [count * arc_count] */
    int64_t *potentials;          /* [count * node_count] */
    int32_t *trace;               /* [count * trace_capacity] */
} mcf_ubatch_io;
typedef struct mcf_ubatch_stats { /* of the last solve call of any kind; the first nine as mcf_batch_stats */
    int64_t instances;
    int64_t lds_instances;        /* the whole batch or none: the tier goes by the stride */
    int64_t global_instances;
    int64_t launches;             /* batch_kernel launches (the set-up, re-cost and finish launches are one each and not counted) */
    int64_t total_pivots;
    int64_t workspace_bytes;      /* count * stride */
    int64_t lds_bytes_max;        /* the stride, when a launch ran in LDS */
    double kernel_ns;             /* host clock round the batch_kernel rounds */
    double host_ns;               /* the rest of the call */
    int64_t bytes_up;             /* MCF_MEM_DEVICE: the slot template and the instance ids of every round of launches */
    int64_t bytes_down;           /* MCF_MEM_DEVICE: the slots, once after the set-up and once per round.  MCF_MEM_HOST adds the arrays */
    double begin_ns, finish_ns;   /* host clock round the set-up (or re-cost) launch with the slots' download, and round the finish launch */
} mcf_ubatch_stats;

MCF_API int mcf_ubatch_create(mcf_ubatch **out, const mcf_ubatch_desc *desc);
MCF_API void mcf_ubatch_destroy(mcf_ubatch *b);
/* Solves all `count` instances on the device, on the null stream; returns synchronised.  May be called again: every call is a fresh solve
 * on the same buffers (new supplies or bounds alone are cheaper through mcf_ubatch_resolve_data).  MCF_ERR_NO_DEVICE without a GPU; the handle is left as it was. */
MCF_API int mcf_ubatch_solve(mcf_ubatch *b, const mcf_ubatch_io *io);
/* Re-solves the instances `changed` marks with the costs in io, as mcf_batch_resolve does: from the kept basis where the instance's last
 * solve ended MCF_OPTIMAL with no flow on an artificial arc, from the start basis otherwise (the limit stated there holds here too).
 * io->cost is read for every marked instance; io->lower / upper / supply are read for the ones that start again and for the output
 * flows, and MUST be what the last mcf_ubatch_solve was given (supply_type too).  Rows of unmarked instances are not written.
 * MCF_ERR_STATE before a solve of either kind. */
MCF_API int mcf_ubatch_resolve(mcf_ubatch *b, const mcf_ubatch_io *io);
/* TEST HOOKS, not supported solvers: the same step functions (csrc/uniform_step.hip.h, csrc/batch_step.hip.h) with one lane on the CPU.
 * io->memory must be MCF_MEM_HOST.  May be mixed with the device calls in any order: the results are the same. */
MCF_API int mcf_ubatch_run_on_host(mcf_ubatch *b, const mcf_ubatch_io *io);
MCF_API int mcf_ubatch_rerun_on_host(mcf_ubatch *b, const mcf_ubatch_io *io);
MCF_API int mcf_ubatch_get_stats(mcf_ubatch *b, mcf_ubatch_stats *out);

/* ---- Re-solving with new supplies and bounds from the kept basis ("Re-solve with new data").
 * The other half of mcf_ubatch_resolve: there the costs change and lower / upper / supply must stay, here lower, upper and supply change
 * and io->cost and io->supply_type MUST be what the last solve call of any kind was given (a supply type other than the last call's is
 * refused with MCF_ERR_INVALID; the costs cannot be checked and are the caller's word).  After such a change the kept basis is still
 * dual feasible -- costs and potentials are untouched -- while its tree flows may leave their bounds.  Per marked instance:
 *   - an upper bound below its lower bound: MCF_INFEASIBLE with 0 pivots, as in a solve;
 *   - WARM where the last solve ended MCF_OPTIMAL with no flow on an artificial arc, no non-tree arc at its upper bound has become
 *     uncapacitated, and the new supplies sum to zero.  The new capacities go in, the non-tree flows follow their state, the tree flows
 *     are recomputed, and DUAL pivots run first: the tree arc with the largest bound violation leaves (lowest node among equals), the
 *     arc across its cut with the smallest reduced cost enters (lowest arc among equals).  When nothing is violated the primal pivots
 *     take over and find nothing to do.  pivots counts both kinds, the trace records every entering arc, the pivot limit applies to the
 *     sum (MCF_NOT_SOLVED, rows zero, cold next time);
 *   - COLD by rule otherwise, and COLD by fallback where a warm attempt did not end with no violation, no entering arc and no flow on a
 *     root link or an artificial arc (the new data are infeasible over the searched arcs, or Unbounded): the instance is set up again
 *     and solved in the same call.  A cold instance's rows are a fresh mcf_ubatch_solve's bit for bit, trace included.
 * A warm instance's status and total cost are those of a fresh solve under the limit stated at mcf_batch_resolve (finite, positive
 * capacities); its flows and potentials are an optimal pair, not necessarily the fresh solve's.  Rows of unmarked instances are not
 * written.  May be mixed with every other solve call and hook in any order: the results are the same.  MCF_ERR_STATE before a solve of
 * either kind; MCF_ERR_NO_DEVICE without a GPU leaves the handle as it was.  With MCF_MEM_DEVICE nothing that scales with the arcs or the
 * nodes crosses the bus: the slot templates and the ids of every round go up; the slots come down after the re-data launch, after every
 * round and once more after the warm attempts are judged, and a `changed` mask comes down as one byte per instance. */
typedef struct mcf_ubatch_redata_stats { /* of the last mcf_*batch_resolve_data / _rerun_data_on_host (all zero before one) */
    int64_t warm_instances;       /* marked and warm by the rule above: re-solved from the kept basis (fallback_instances are among them) */
    int64_t cold_instances;       /* marked and cold by rule (incl. the ones infeasible by their bounds) */
    int64_t fallback_instances;   /* warm attempts that did not stand and were solved again cold in the same call */
    int64_t untouched_instances;  /* not marked */
    int64_t dual_pivots;          /* of all warm attempts, the given-up ones included */
    int64_t primal_pivots;        /* of the cold solves, the fallbacks' and whatever a warm attempt needed after its dual phase */
    int64_t launches;             /* batch kernel launches */
    int64_t bytes_up, bytes_down; /* as mcf_ubatch_stats */
    double kernel_ns, host_ns, begin_ns, finish_ns;    /* as mcf_ubatch_stats; begin_ns is round the re-data launch */
} mcf_ubatch_redata_stats;
MCF_API int mcf_ubatch_resolve_data(mcf_ubatch *b, const mcf_ubatch_io *io);
/* TEST HOOK like mcf_ubatch_rerun_on_host: the same steps (uniform_redata, batch_dual_run) with one lane on the CPU, MCF_MEM_HOST only. */
MCF_API int mcf_ubatch_rerun_data_on_host(mcf_ubatch *b, const mcf_ubatch_io *io);
MCF_API int mcf_ubatch_get_redata_stats(mcf_ubatch *b, mcf_ubatch_redata_stats *out);

/* ---- Validating a uniform batch where it lies ("Uniform batch: validation").  The checks of section (3) above -- the
 * reference's SolutionValidator -- for every instance in ONE launch: block i checks instance i, reading problem and solution as
 * base + i * stride like the solve and writing one row of answers.  Per-node conservation walks incidence lists that mcf_ubatch_create
 * builds from the topology and that go up with it, once per handle: no atomics and no scratch per instance.
 * Per instance: errors[k] = the number of messages of kind k (mcf_validation_kind) the reference would add, first[k] = the lowest arc /
 * node id among them or -1, objective = sum flow * cost, dual_cost as mcf_validation's, valid = no message at all.  An instance whose
 * status is not MCF_OPTIMAL gets errors[MCF_VAL_STATUS] = 1, first[MCF_VAL_STATUS] = 0, everything else 0 / -1, and none of its other
 * rows is read.  upper: NULL or MCF_INF_CAP stand for INT64_MAX / 2, the bound as Solve() leaves it (what mcf_ns_validate passes).
 * All arithmetic wraps (C# long, unchecked).
 * The call belongs to no solve: it works before one, reads whatever solution it is given (not necessarily this handle's) and leaves
 * the handle's solve state -- workspaces, slots, kept basis, statistics -- as it was.  Runs on the null stream, returns synchronised.
 * Refusals: MCF_ERR_INVALID for a null argument, a null status / total_cost / flows / potentials, a supply type outside MCF_SUPPLY_GEQ /
 * _LEQ / MCF_SUPPLY_EQ, an unknown memory kind or a negative stride; MCF_ERR_NO_DEVICE without a GPU. */
typedef struct mcf_ubatch_check_io {
    int32_t memory, supply_type;                       /* MCF_MEM_*, MCF_SUPPLY_GEQ / _LEQ / _EQ */
    const int64_t *lower, *upper, *cost, *supply;      /* as mcf_ubatch_io, NULL as there */
    int64_t lower_stride, upper_stride, cost_stride, supply_stride;
    const int32_t *status;                             /* the solution to check: all four required, rows as mcf_ubatch_io writes them */
    const int64_t *total_cost, *flows, *potentials;
    int32_t *valid;                                    /* results, any may be NULL: [count] */
    int32_t *errors, *first;                           /* [count * MCF_VAL_KINDS]; first = lowest failing arc / node id, -1 */
    int64_t *objective, *dual_cost;                    /* [count] */
} mcf_ubatch_check_io;
typedef struct mcf_ubatch_check_summary {
    int64_t instances, invalid, first_invalid;         /* first_invalid: -1 when none */
    double kernel_ns;                                  /* host clock round the launch */
    int64_t bytes_up, bytes_down;                      /* MCF_MEM_DEVICE: nothing that scales with m, n or count */
} mcf_ubatch_check_summary;
MCF_API int mcf_ubatch_validate(mcf_ubatch *b, const mcf_ubatch_check_io *io, mcf_ubatch_check_summary *out);
/* TEST HOOK: the same step (uniform_validate, csrc/uniform_step.hip.h) with one lane on the CPU.  io->memory must be MCF_MEM_HOST. */
MCF_API int mcf_ubatch_validate_on_host(mcf_ubatch *b, const mcf_ubatch_check_io *io, mcf_ubatch_check_summary *out);

/* ---- Ragged batch: a SET of graphs in one handle, every instance names its own ("Ragged batch").
 * mcf_ubatch_* above demands that every instance share one graph.  Here a handle holds `graph_count` graphs and `count` instances;
 * instance i is an instance of graph graph_of[i].  Problem data and results are RAGGED ROWS of flat arrays: instance i's arcs are the
 * elements [arc_row[i], arc_row[i + 1]) with arc_row[i] = the sum of the arc counts of the instances before it, its nodes the elements
 * [node_row[i], node_row[i + 1]) likewise; mcf_rbatch_get_rows returns both.  All offsets are 64-bit.  There are no strides: a shared
 * row has no meaning across graphs.
 * Set-up, pivots, finish and validation run on the device as for the uniform batch (the same steps and the same kernel for the pivots);
 * the only difference is that a block finds its instance's graph, rows and workspace in per-handle tables in device memory instead of
 * multiplying by strides.  Every instance has the workspace of ITS graph, so one handle mixes the LDS classes and the global tier by
 * instance, as mcf_batch_* does.  With MCF_MEM_DEVICE nothing that scales with the arcs or the nodes crosses the bus in a call: the
 * topology, its incidence lists and the tables go up once per handle, with its first device call, and are not counted in a call's
 * statistics; per call go the slot templates (one per graph, 160 bytes each, counted in bytes_up), the ids of every round of launches
 * and the slots.
 * Results: instance i gets bit for bit what mcf_batch_add + mcf_batch_solve give for the same instance; with one graph every row equals
 * mcf_ubatch_*'s.  Limits per graph are mcf_batch_add's (MCF_BATCH_MAX_ARCS / _NODES), at most MCF_BATCH_MAX_INSTANCES instances; rules
 * and refusals of the first nine descriptor fields are mcf_batch_create's.  mcf_rbatch_create also refuses, with MCF_ERR_INVALID and a
 * message: a graph_of entry outside [0, graph_count), a NULL graph_of with count != graph_count, an arc_start that is not monotone, an
 * end point outside its graph's nodes. */
typedef struct mcf_rbatch mcf_rbatch;
typedef struct mcf_rbatch_desc {
    int32_t device;               /* as mcf_batch_desc, field for field ... */
    int32_t pivot_rule;
    int32_t semantics;
    int32_t reserved;
    int64_t pivot_limit;          /* 0 = the default of each instance's own graph.  The output rows of an instance stopped by it
                                     (MCF_NOT_SOLVED) are zero.  Its trace row holds `limit` entries (min(limit, trace_capacity)), zeros
                                     behind them.  A re-solve of a stopped instance starts cold. */
    int32_t pivots_per_launch;
    int32_t trace_capacity;
    int32_t flags;
    int32_t graph_count;          /* ... then the graphs: distinct topologies, >= 0 */
    int32_t count;                /* instances, >= 0, <= MCF_BATCH_MAX_INSTANCES */
    const int32_t *node_count;    /* [graph_count], HOST memory like every pointer here; all are copied by mcf_rbatch_create */
    const int64_t *arc_start;     /* [graph_count + 1] into source / target: graph g has arc_start[g + 1] - arc_start[g] arcs */
    const int32_t *source;        /* the graphs' end points, concatenated; node ids are the graph's own, from 0 */
    const int32_t *target;
    const int32_t *graph_of;      /* [count] instance -> graph; NULL = instance i is graph i (count must equal graph_count) */
} mcf_rbatch_desc;
typedef struct mcf_rbatch_io {
    int32_t memory;               /* MCF_MEM_HOST / MCF_MEM_DEVICE: where EVERY pointer below points */
    int32_t supply_type;          /* MCF_SUPPLY_GEQ / _LEQ, for every instance of this call */
    const int64_t *lower;         /* [arc_row[count]]; NULL = 0 */
    const int64_t *upper;         /* [arc_row[count]]; NULL = uncapacitated; MCF_INF_CAP as in mcf_ns_set_problem */
    const int64_t *cost;          /* [arc_row[count]]; NULL = 0 */
    const int64_t *supply;        /* [node_row[count]]; NULL = 0 */
    const uint8_t *changed;       /* mcf_rbatch_resolve / _rerun_on_host only: [count], nonzero = re-solve this instance; NULL = all */
    /* results, any may be NULL; zero-filled as mcf_ubatch_io's */
    int32_t *status;              /* [count] */
    int64_t *pivots;              /* [count] */
    int64_t *total_cost;          /* [count] */
    int64_t *flows;               /* [arc_row[count]] */
    int64_t *potentials;          /* [node_row[count]] */
    int32_t *trace;               /* [count * trace_capacity] */
} mcf_rbatch_io;
typedef struct mcf_rbatch_check_io {                   /* mcf_ubatch_check_io without strides */
    int32_t memory, supply_type;                       /* MCF_MEM_*, MCF_SUPPLY_GEQ / _LEQ / _EQ */
    const int64_t *lower, *upper, *cost, *supply;      /* as mcf_rbatch_io, NULL as there */
    const int32_t *status;                             /* the solution to check, rows as mcf_rbatch_io writes them: all four required */
    const int64_t *total_cost, *flows, *potentials;    /* (flows / potentials may be NULL where the handle has no arc / no node at all) */
    int32_t *valid;                                    /* results, any may be NULL: [count] */
    int32_t *errors, *first;                           /* [count * MCF_VAL_KINDS] */
    int64_t *objective, *dual_cost;                    /* [count] */
} mcf_rbatch_check_io;

MCF_API int mcf_rbatch_create(mcf_rbatch **out, const mcf_rbatch_desc *desc);
MCF_API void mcf_rbatch_destroy(mcf_rbatch *b);
/* arc_row and node_row, each [count + 1] (either may be NULL): where instance i's rows begin; the last entry is the total */
MCF_API int mcf_rbatch_get_rows(mcf_rbatch *b, int64_t *arc_row, int64_t *node_row);
/* The contracts of their mcf_ubatch_* namesakes, refusal codes included: null stream, return synchronised, the handle's device is made
 * current and the caller's restored; MCF_ERR_NO_DEVICE without a GPU leaves the handle as it was; a re-solve before any solve is
 * MCF_ERR_STATE; the limit stated at mcf_batch_resolve on warm re-solves holds here word for word.  The four solve calls may follow each
 * other in any order: the state moves whole between host and device, the results are the same. */
MCF_API int mcf_rbatch_solve(mcf_rbatch *b, const mcf_rbatch_io *io);
MCF_API int mcf_rbatch_resolve(mcf_rbatch *b, const mcf_rbatch_io *io);
MCF_API int mcf_rbatch_run_on_host(mcf_rbatch *b, const mcf_rbatch_io *io);        /* TEST HOOKS: one lane on the CPU, MCF_MEM_HOST only */
MCF_API int mcf_rbatch_rerun_on_host(mcf_rbatch *b, const mcf_rbatch_io *io);
/* mcf_ubatch_stats of the last solve call of any kind.  Here lds_instances and global_instances may both be non-zero: the tier goes by
 * each instance's own footprint; workspace_bytes is the sum of the footprints. */
MCF_API int mcf_rbatch_get_stats(mcf_rbatch *b, mcf_ubatch_stats *out);
/* mcf_ubatch_resolve_data, its hook and its statistics for ragged rows, contract for contract. */
MCF_API int mcf_rbatch_resolve_data(mcf_rbatch *b, const mcf_rbatch_io *io);
MCF_API int mcf_rbatch_rerun_data_on_host(mcf_rbatch *b, const mcf_rbatch_io *io);
MCF_API int mcf_rbatch_get_redata_stats(mcf_rbatch *b, mcf_ubatch_redata_stats *out);
/* mcf_ubatch_validate for ragged rows: block i checks instance i against its own graph's incidence lists. */
MCF_API int mcf_rbatch_validate(mcf_rbatch *b, const mcf_rbatch_check_io *io, mcf_ubatch_check_summary *out);
MCF_API int mcf_rbatch_validate_on_host(mcf_rbatch *b, const mcf_rbatch_check_io *io, mcf_ubatch_check_summary *out);

/* ---- Cost ranges of the kept basis (DESIGN.md 3.14 "Cost ranges of the kept basis"): classic post-optimality cost ranging, computed on
 * the device from the state every instance's last solve call left there.  An instance is RANGED when that call, of whichever kind,
 * left it as a warm start with new costs demands: no entering arc, and no flow on a root link or an artificial arc -- Optimal, with
 * every supply met exactly.  For a ranged instance and each of its arcs e the kept basis stays optimal exactly while the arc's cost lies
 * in [cost[e] - cost_down[e], cost[e] + cost_up[e]] with every other cost as the last solve call was given it: a mcf_*batch_resolve with
 * a cost inside the interval makes no pivot and returns the same flows.  Both are >= 0 and deltas, not costs; MCF_RANGE_INF = no limit
 * on that side.  An arc at its lower bound has cost_up = MCF_RANGE_INF, one at its upper bound cost_down = MCF_RANGE_INF; a tree arc's
 * two sides are minima over the non-tree arcs across its cut (csrc/ranges_step.hip.h).  arc_state is the basis itself as far as the
 * caller's arcs go: MCF_STATE_LOWER / _TREE / _UPPER.  Every other instance gets ranged = 0 and zero rows.
 * "Every other cost" includes the cost of the artificial arcs the solver adds, which a re-solve derives anew from the largest |cost| it
 * is given, (max |cost| + 1) * node_count: a limit of about that size comes from a root link seen through an artificial arc that stayed
 * in the tree at flow 0, and a cost moved that far moves the artificial cost along -- read it as "practically unlimited".
 * One wave per instance; an instance is ranged in LDS exactly when it is solved there.  Contract as mcf_ubatch_validate's: null stream,
 * returns synchronised, the handle's device is made current and the caller's restored.  The call reads the kept state and changes none
 * of it: workspaces, slots, basis, results and the other statistics stay, and it mixes with every solve call and hook in any order (the
 * state moves whole between host and device as it does for them).  MCF_ERR_STATE before a solve of either kind; MCF_ERR_NO_DEVICE
 * without a GPU leaves the handle as it was; MCF_ERR_INVALID for a null argument, an unknown memory kind, or one of cost_down / cost_up
 * without the other.  With MCF_MEM_DEVICE nothing that scales with the arcs, the nodes or the instances crosses the bus in a call (a
 * table of one int32 per instance goes up once per handle, with the first call). */
#define MCF_RANGE_INF INT64_MAX
typedef struct mcf_ubatch_range_io {
    int32_t memory;               /* MCF_MEM_HOST / MCF_MEM_DEVICE: where every pointer below points */
    int32_t reserved;
    /* results, any may be NULL -- but cost_down and cost_up both or neither (without them no cycle is walked) */
    int32_t *ranged;              /* [count] 1 / 0 */
    int8_t *arc_state;            /* [count * arc_count] */
    int64_t *cost_down;           /* [count * arc_count] */
    int64_t *cost_up;             /* [count * arc_count] */
} mcf_ubatch_range_io;
typedef struct mcf_rbatch_range_io {                   /* the same with flat rows: instance i's arcs at [arc_row[i], arc_row[i + 1]) */
    int32_t memory;
    int32_t reserved;
    int32_t *ranged;              /* [count] */
    int8_t *arc_state;            /* [arc_row[count]] */
    int64_t *cost_down;           /* [arc_row[count]] */
    int64_t *cost_up;             /* [arc_row[count]] */
} mcf_rbatch_range_io;
typedef struct mcf_ubatch_range_stats { /* of the last mcf_*batch_cost_ranges / _on_host (all zero before one) */
    int64_t instances;
    int64_t ranged;               /* instances with ranged = 1 */
    int64_t lds_instances;        /* of `instances`, by the tier they are solved in; 0 and 0 from the host hook */
    int64_t global_instances;
    int64_t tree_arcs;            /* the ranged instances' tree arcs among the caller's arcs: the rows that took a walk to fill */
    int64_t cycle_hops;           /* steps of all cycle walks: one dependent load chain link each.  Both 0 without cost_down / cost_up */
    double kernel_ns;             /* round the launches, synchronised */
    int64_t bytes_up, bytes_down; /* MCF_MEM_DEVICE: the three summary words; MCF_MEM_HOST adds the arrays */
} mcf_ubatch_range_stats;
MCF_API int mcf_ubatch_cost_ranges(mcf_ubatch *b, const mcf_ubatch_range_io *io);
/* TEST HOOK: the same step (uniform_ranges, csrc/ranges_step.hip.h) with one lane on the CPU.  io->memory must be MCF_MEM_HOST. */
MCF_API int mcf_ubatch_cost_ranges_on_host(mcf_ubatch *b, const mcf_ubatch_range_io *io);
MCF_API int mcf_ubatch_get_range_stats(mcf_ubatch *b, mcf_ubatch_range_stats *out);
MCF_API int mcf_rbatch_cost_ranges(mcf_rbatch *b, const mcf_rbatch_range_io *io);
MCF_API int mcf_rbatch_cost_ranges_on_host(mcf_rbatch *b, const mcf_rbatch_range_io *io);
MCF_API int mcf_rbatch_get_range_stats(mcf_rbatch *b, mcf_ubatch_range_stats *out);

/* ---- Supply and bound ranges of the kept basis (DESIGN.md 3.14 "Supply and bound ranges of the kept basis"): classic right-hand-side
 * ranging, the data side of the cost ranges above, computed on the device from the same kept state.  RANGED as there; every other
 * instance gets ranged = 0 and zero rows.  For a ranged instance the kept basis stays primal feasible -- a mcf_*batch_resolve_data that
 * changes this one thing counts the instance as warm, makes no dual and no primal pivot, does not fall back, and leaves it ranged with
 * the same arc_state -- exactly while
 *   - the flow of arc e, were it moved with every other non-tree flow fixed, falls by at most flow_down[e] or rises by at most flow_up[e].
 *     A tree arc's two sides are its own room within its bounds; a non-tree arc's are the least room along its cycle in the tree
 *     (csrc/data_ranges_step.hip.h) and are NOT clipped by the arc's own capacity.  An arc without an upper bound (MCF_INF_CAP) has no
 *     limit to rise, whatever its lower bound (lower bounds below 2^61 in size);
 *   - d units of supply move from node b to node a of a pair the caller names (supply[a] + d, supply[b] - d) with d <= ship_forth, or
 *     from a to b with d <= ship_back.  a == b gives MCF_RANGE_INF twice; an id outside [0, node_count) gives -1 twice and reads nothing.
 * All are >= 0 and deltas; MCF_RANGE_INF = no limit.  The ranges of the bounds follow per arc without another walk (for an uncapacitated
 * arc MCF_RANGE_INF in the upper columns means there is no finite upper bound to move):
 *
 *   arc_state | lower may fall by | lower may rise by             | upper may fall by             | upper may rise by
 *   LOWER     | flow_down         | min(flow_up, upper - lower)   | upper - lower                 | MCF_RANGE_INF
 *   UPPER     | MCF_RANGE_INF     | upper - lower                 | min(flow_down, upper - lower) | flow_up
 *   TREE      | MCF_RANGE_INF     | flow_down                     | flow_up                       | MCF_RANGE_INF
 *
 * A tree path that passes a root link or an artificial arc has no room: the re-solve lets no warm attempt stand that leaves flow there.
 * One wave per instance; an instance is ranged in LDS exactly when it is solved there.  Contract as mcf_*batch_cost_ranges': null
 * stream, returns synchronised, the handle's device made current and the caller's restored; the call reads the kept state and changes
 * none of it, and mixes with every solve call and hook in any order.  The pairs lie in the memory kind of the call.  MCF_ERR_STATE
 * before a solve of either kind; MCF_ERR_NO_DEVICE without a GPU leaves the handle as it was; MCF_ERR_INVALID for a null argument, an
 * unknown memory kind, one of flow_down / flow_up or of ship_forth / ship_back without the other, ship rows without pairs, a negative
 * pair count, and -- where the tables lie in host memory -- pair_row or ship_row that do not fit each other.  With MCF_MEM_DEVICE nothing
 * that scales with the arcs, the nodes, the pairs or the instances crosses the bus in a call (a table of one int32 per instance goes up
 * once per handle, with the first call). */
typedef struct mcf_ubatch_data_range_io {
    int32_t memory;               /* MCF_MEM_HOST / MCF_MEM_DEVICE: where every pointer below points */
    int32_t reserved;
    /* the pairs: ONE list for every instance; NULL with pair_count 0 */
    int64_t pair_count;
    const int32_t *pairs;         /* [pair_count][2] node ids (a, b) */
    /* results, any may be NULL -- but flow_down and flow_up both or neither, ship_forth and ship_back both or neither */
    int32_t *ranged;              /* [count] 1 / 0 */
    int8_t *arc_state;            /* [count * arc_count] */
    int64_t *flow_down;           /* [count * arc_count] */
    int64_t *flow_up;             /* [count * arc_count] */
    int64_t *ship_forth;          /* [count * pair_count] */
    int64_t *ship_back;           /* [count * pair_count] */
} mcf_ubatch_data_range_io;
typedef struct mcf_rbatch_data_range_io {              /* flat rows: instance i's arcs at [arc_row[i], arc_row[i + 1]) */
    int32_t memory;
    int32_t reserved;
    /* the pairs: one list per GRAPH, flat; graph g's are pairs[pair_row[g] .. pair_row[g + 1]), pair_row[0] = 0.  All three NULL: none */
    const int32_t *pairs;         /* [pair_row[graph_count]][2] */
    const int64_t *pair_row;      /* [graph_count + 1] */
    const int64_t *ship_row;      /* [count + 1]: where instance i's answers begin in the ship rows, running sums of its graph's pair count */
    int32_t *ranged;              /* [count] */
    int8_t *arc_state;            /* [arc_row[count]] */
    int64_t *flow_down;           /* [arc_row[count]] */
    int64_t *flow_up;             /* [arc_row[count]] */
    int64_t *ship_forth;          /* [ship_row[count]] */
    int64_t *ship_back;           /* [ship_row[count]] */
} mcf_rbatch_data_range_io;
typedef struct mcf_ubatch_data_range_stats { /* of the last mcf_*batch_data_ranges / _on_host (all zero before one) */
    int64_t instances;
    int64_t ranged;               /* instances with ranged = 1 */
    int64_t lds_instances;        /* of `instances`, by the tier they are solved in; 0 and 0 from the host hook */
    int64_t global_instances;
    int64_t walks;                /* tree paths walked: one per non-tree arc (with flow rows), one per pair with both ids in range */
    int64_t hops;                 /* steps of all walks: one dependent load chain link each */
    double kernel_ns;             /* round the launches, synchronised */
    int64_t bytes_up, bytes_down; /* MCF_MEM_DEVICE: the three summary words; MCF_MEM_HOST adds the arrays */
} mcf_ubatch_data_range_stats;
MCF_API int mcf_ubatch_data_ranges(mcf_ubatch *b, const mcf_ubatch_data_range_io *io);
/* TEST HOOK: the same step (uniform_data_ranges, csrc/data_ranges_step.hip.h) with one lane on the CPU.  io->memory must be MCF_MEM_HOST. */
MCF_API int mcf_ubatch_data_ranges_on_host(mcf_ubatch *b, const mcf_ubatch_data_range_io *io);
MCF_API int mcf_ubatch_get_data_range_stats(mcf_ubatch *b, mcf_ubatch_data_range_stats *out);
MCF_API int mcf_rbatch_data_ranges(mcf_rbatch *b, const mcf_rbatch_data_range_io *io);
MCF_API int mcf_rbatch_data_ranges_on_host(mcf_rbatch *b, const mcf_rbatch_data_range_io *io);
MCF_API int mcf_rbatch_get_data_range_stats(mcf_rbatch *b, mcf_ubatch_data_range_stats *out);

/* ---- Starting a solve from a basis the caller supplies (DESIGN.md 3.14 "Start from a given basis").  The way back in for what
 * mcf_*batch_cost_ranges writes out as arc_state: one state per arc of the caller's, MCF_STATE_LOWER / _TREE / _UPPER, from a solve of
 * this handle or of another, of a mcf_ubatch or of a mcf_rbatch on the same graph, from today or from a file.  A uniform handle takes one
 * row per instance or, with state_stride 0, ONE row for the whole batch: solve a representative instance once, start the others from
 * its basis.  The call is a solve call like mcf_ubatch_solve: allowed on a handle that has never solved and at any later time, it reads
 * all of io and replaces the kept state of every instance; afterwards mcf_*batch_resolve, _resolve_data, _cost_ranges and _validate go on
 * from it as from any solve.  pivots and the trace describe this call, dual and primal pivots together; mcf_*batch_get_stats too.
 * Per instance (csrc/uniform_step.hip.h, uniform_begin_from):
 *   - the TREE arcs of its row must form a forest on the nodes.  It is walked depth first over the handle's incidence lists (arc ids
 *     ascending per node), components by ascending lowest node, each rooted there and hung on the artificial root by an ARTIFICIAL arc
 *     of cost (max |cost| + 1) * node_count -- not by the node's zero-cost root link, so that all potentials lie beyond that cost as they
 *     do after a real solve and no root link becomes eligible.  The walk is bounded by count: no row can make it spin;
 *   - non-tree arcs carry 0 or, at UPPER, their capacity; tree flows follow from conservation, potentials from the tree's costs;
 *   - COLD BY RULE, which means a fresh mcf_*batch_solve of the instance bit for bit, trace included: a value outside {-1, 0, 1}; a TREE
 *     arc that closes a cycle (a self loop and the second of two parallel TREE arcs are such); UPPER on an uncapacitated arc; supplies that
 *     do not sum to zero; a component whose supplies do not balance by themselves; a basis that is neither of the two below; an upper
 *     bound below its lower bound (MCF_INFEASIBLE with 0 pivots, as in a solve);
 *   - a PRIMAL START where every tree arc's flow lies within its bounds: primal pivots from there -- none at all where the basis is
 *     optimal for the data given, as a basis exported after an Optimal solve without artificial flow is for that solve's data;
 *   - else a DUAL START where every non-tree arc's reduced cost has the sign of its state: dual pivots first, as in
 *     mcf_ubatch_resolve_data, then the primal ones;
 *   - an accepted start that does not end with no entering arc and no flow on a root link or an artificial arc is set up again and solved
 *     cold in the same call (a fallback); the pivot limit is the exception and stays MCF_NOT_SOLVED with zero rows.
 * So every answer is a fresh solve's: status and total cost under the limit stated at mcf_batch_resolve, flows and potentials an optimal
 * pair, not necessarily the fresh solve's.  Refusals, MCF_ERR_INVALID with a message: a null argument or a null arc_state, a basis
 * whose `memory` differs from io->memory, a negative stride, a non-null io->changed (an unmarked instance of a fresh handle would have no
 * state), a hook called with MCF_MEM_DEVICE.  MCF_ERR_NO_DEVICE without a GPU leaves the handle as it was.  With MCF_MEM_DEVICE nothing
 * that scales with the arcs, the nodes or the instances' rows crosses the bus in a call: the slot templates and the ids of every round
 * go up, the slots come down (after the start launch, after every round, after the settle launch); the incidence lists go up once per
 * handle with the topology.  mcf_batch_* has no such call, for the reason given at mcf_ubatch_resolve_data: it sets its instances up
 * on the host. */
typedef struct mcf_ubatch_basis_io {
    int32_t memory;               /* MCF_MEM_HOST / MCF_MEM_DEVICE: must equal io->memory */
    int32_t reserved;
    const int8_t *arc_state;      /* [arc_count] per instance */
    int64_t state_stride;         /* elements between instances' rows; 0 = one row for all */
} mcf_ubatch_basis_io;
typedef struct mcf_rbatch_basis_io {
    int32_t memory;
    int32_t reserved;
    const int8_t *arc_state;      /* [arc_row[count]]: instance i's arcs at [arc_row[i], arc_row[i + 1]) */
} mcf_rbatch_basis_io;
typedef struct mcf_ubatch_start_stats { /* of the last mcf_*batch_solve_from / _run_from_on_host (all zero before one) */
    int64_t primal_starts;        /* accepted with every tree flow within its bounds (fallback_instances may be among them) */
    int64_t dual_starts;          /* accepted with violated tree flows and dual-feasible reduced costs (likewise) */
    int64_t cold_instances;       /* cold by rule */
    int64_t fallback_instances;   /* accepted starts that did not stand and were solved again cold in the same call */
    int64_t dual_pivots;          /* of all dual starts, the given-up ones included */
    int64_t primal_pivots;        /* everything else: primal starts, cold solves, fallbacks, what a dual start needed afterwards */
    int64_t launches;             /* batch kernel launches */
    int64_t bytes_up, bytes_down; /* as mcf_ubatch_stats */
    double kernel_ns, host_ns, begin_ns, finish_ns;    /* as mcf_ubatch_stats; begin_ns is round the start launch */
} mcf_ubatch_start_stats;
MCF_API int mcf_ubatch_solve_from(mcf_ubatch *b, const mcf_ubatch_io *io, const mcf_ubatch_basis_io *basis);
/* TEST HOOK: the same steps (uniform_begin_from, batch_dual_run, batch_run) with one lane on the CPU, MCF_MEM_HOST only. */
MCF_API int mcf_ubatch_run_from_on_host(mcf_ubatch *b, const mcf_ubatch_io *io, const mcf_ubatch_basis_io *basis);
MCF_API int mcf_ubatch_get_start_stats(mcf_ubatch *b, mcf_ubatch_start_stats *out);
MCF_API int mcf_rbatch_solve_from(mcf_rbatch *b, const mcf_rbatch_io *io, const mcf_rbatch_basis_io *basis);
MCF_API int mcf_rbatch_run_from_on_host(mcf_rbatch *b, const mcf_rbatch_io *io, const mcf_rbatch_basis_io *basis);
MCF_API int mcf_rbatch_get_start_stats(mcf_rbatch *b, mcf_ubatch_start_stats *out);

/* ---- Why an instance is infeasible (DESIGN.md 3.14 "Why infeasible: a cut from the kept flow"): a certificate read on the device from
 * the flow every instance's last solve call left there.  The status word mirrors the reference's test (difference D9: the n root links
 * only) and is not mathematical feasibility: an instance can be MCF_OPTIMAL with a supply surplus left on an artificial arc, and
 * MCF_INFEASIBLE with a flow that satisfies every constraint.  This call answers the question itself, for every instance whose last
 * solve call ended with no entering arc (csrc/diagnose_step.hip.h):
 *   unmet[v]   what node v could not ship: with nf(v) the net outflow of v on the caller's arcs, nf(v) = supply'(v) - unmet[v], where
 *              supply' is the supply shifted by the lower bounds.  MCF_SUPPLY_GEQ asks nf >= supply: v is violated where unmet > 0
 *              and has slack where unmet < 0; MCF_SUPPLY_LEQ mirrors both signs.
 *   MCF_DIAG_FEASIBLE  no node is violated: the kept flow satisfies every constraint.  violation 0, set_size 0, side all 0.
 *   MCF_DIAG_CUT       the instance is infeasible, and side[] names a node set S that proves it in the caller's own numbers:
 *                        GEQ  violation = supply(S) - (upper(arcs leaving S) - lower(arcs entering S)) > 0
 *                        LEQ  violation = (lower(arcs leaving S) - upper(arcs entering S)) - supply(S) > 0
 *                      S is what the violated nodes reach (GEQ; LEQ: the nodes that reach them) in the residual graph of the kept flow,
 *                      no uncapacitated arc crosses it in the bounding direction, and violation is the sum of |unmet| over S.
 *   MCF_DIAG_OPEN      S holds a node with slack: the kept flow is not extremal and no certificate comes from it.  side[] is S,
 *                      violation 0.  The artificial cost (max |cost| + 1) * node_count rules this out after a solve that found no
 *                      entering arc; it is counted so that it can be seen to stay zero.
 *   MCF_DIAG_BOUNDS    some arc has upper < lower; no cut.  Zero rows.
 *   MCF_DIAG_NONE      the last solve call ended Unbounded or at a limit, or there was none for this instance.  Zero rows.
 * One wave per instance; an instance is diagnosed in LDS exactly when it is solved there (16 bytes per arc of the caller's and 18 per
 * node, below the solve's footprint); the others walk their workspace in place with marks and frontiers in a buffer of the handle's,
 * allocated with the first call.  Contract as mcf_*batch_cost_ranges': null stream, returns synchronised, the handle's device made
 * current and the caller's restored; the call reads the kept state and changes none of it -- workspaces, slots, basis, results and the
 * other statistics stay -- and mixes with every solve call, range call and hook in any order.  MCF_ERR_STATE before a solve of either
 * kind; MCF_ERR_NO_DEVICE without a GPU leaves the handle as it was; MCF_ERR_INVALID for a null argument or an unknown memory kind.
 * With MCF_MEM_DEVICE nothing that scales with the arcs, the nodes or the instances crosses the bus in a call (a table of one int32 per
 * instance goes up once per handle, with the first call).  Without `side` the walk still runs: the verdict needs it. */
#define MCF_DIAG_NONE 0
#define MCF_DIAG_FEASIBLE 1
#define MCF_DIAG_CUT 2
#define MCF_DIAG_OPEN 3
#define MCF_DIAG_BOUNDS 4
typedef struct mcf_ubatch_diagnose_io {
    int32_t memory;               /* MCF_MEM_HOST / MCF_MEM_DEVICE: where every pointer below points */
    int32_t reserved;
    /* results, any may be NULL */
    int32_t *verdict;             /* [count] MCF_DIAG_* */
    int64_t *violation;           /* [count] */
    int32_t *set_size;            /* [count] nodes in S */
    int8_t *side;                 /* [count * node_count] 1 = in S */
    int64_t *unmet;               /* [count * node_count] */
} mcf_ubatch_diagnose_io;
typedef struct mcf_rbatch_diagnose_io {                /* the same with flat rows: instance i's nodes at [node_row[i], node_row[i + 1]) */
    int32_t memory;
    int32_t reserved;
    int32_t *verdict;             /* [count] */
    int64_t *violation;           /* [count] */
    int32_t *set_size;            /* [count] */
    int8_t *side;                 /* [node_row[count]] */
    int64_t *unmet;               /* [node_row[count]] */
} mcf_rbatch_diagnose_io;
typedef struct mcf_ubatch_diagnose_stats { /* of the last mcf_*batch_diagnose / _on_host (all zero before one) */
    int64_t instances;
    int64_t none, feasible, cut, open, bounds;          /* of `instances`, by verdict */
    int64_t lds_instances;        /* of `instances`, by the tier they are solved in; 0 and 0 from the host hook */
    int64_t global_instances;
    int64_t levels;               /* levels of all walks: two barriers and one sweep over the nodes each */
    int64_t frontier_nodes;       /* nodes of all frontiers = the sizes of all S */
    int64_t inc_entries;          /* incidence entries read: one flow (and capacity) lookup each */
    double kernel_ns;             /* round the launches, synchronised */
    int64_t bytes_up, bytes_down; /* MCF_MEM_DEVICE: the summary words; MCF_MEM_HOST adds the arrays */
} mcf_ubatch_diagnose_stats;
MCF_API int mcf_ubatch_diagnose(mcf_ubatch *b, const mcf_ubatch_diagnose_io *io);
/* TEST HOOK: the same step (uniform_diagnose, csrc/diagnose_step.hip.h) with one lane on the CPU.  io->memory must be MCF_MEM_HOST. */
MCF_API int mcf_ubatch_diagnose_on_host(mcf_ubatch *b, const mcf_ubatch_diagnose_io *io);
MCF_API int mcf_ubatch_get_diagnose_stats(mcf_ubatch *b, mcf_ubatch_diagnose_stats *out);
MCF_API int mcf_rbatch_diagnose(mcf_rbatch *b, const mcf_rbatch_diagnose_io *io);
MCF_API int mcf_rbatch_diagnose_on_host(mcf_rbatch *b, const mcf_rbatch_diagnose_io *io);
MCF_API int mcf_rbatch_get_diagnose_stats(mcf_rbatch *b, mcf_ubatch_diagnose_stats *out);

/* ---- Unbounded or not (DESIGN.md 3.14 "Unbounded or not: a negative cycle or labels from the kept data"): a certificate either way,
 * read on the device from the costs and capacities every instance's last solve call left in its workspace.  The status word mirrors the
 * reference (a negative cycle of uncapacitated arcs is answered MCF_OPTIMAL with flows of 2^62 - 1 and a total cost that wraps), so this
 * call answers the question itself, on the caller's arcs, an arc being uncapacitated where upper = MCF_INF_CAP (csrc/rays_step.hip.h):
 *   MCF_RAY_CYCLE    there is a directed cycle of uncapacitated arcs of total cost < 0: on_cycle[] marks the arcs of ONE simple such
 *                    cycle (a self loop is one of length 1; of parallel arcs one is marked), cycle_cost < 0 is their cost and
 *                    cycle_length >= 1 their number.  If the instance is feasible at all its objective is unbounded below, and
 *                    whatever the status says its cost and flows are no optimum.  label[] is 0.
 *   MCF_RAY_BOUNDED  there is none, and label[] proves it: label[target] <= label[source] + cost on every uncapacitated arc, which
 *                    summed round any cycle of them gives a cost >= 0.  on_cycle all 0, cycle_cost 0, cycle_length 0.
 *   MCF_RAY_BOUNDS   some arc has upper < lower: the workspace was never set up.  Zero rows.
 *   MCF_RAY_NONE     no solve call has set this instance's workspace up.  Zero rows.
 * Every other ending of the last solve call (no entering arc, Unbounded, a limit) gets the real answer: the call reads costs and
 * capacities only, never the flow or the basis, so it also answers after a re-solve of either kind from the data that left.
 * A level-synchronous Bellman-Ford from all-zero labels, one wave per instance: with k nodes that have an uncapacitated arc coming in,
 * at most k + 1 rounds of two barriers and one sweep over the nodes each -- a bounded instance with costs >= 0 takes one, a long
 * negative cycle takes all of them.  An instance is queried in LDS exactly when it is solved there (16 bytes per arc of the caller's
 * and 29 per node, below the solve's footprint); the others read their workspace in place with labels, marks and frontiers in the
 * handle's buffer that mcf_*batch_diagnose uses.  Contract as mcf_*batch_diagnose's: null stream, returns synchronised; the call reads
 * the kept state and changes none of it; MCF_ERR_STATE before a solve of either kind; MCF_ERR_NO_DEVICE without a GPU leaves the handle
 * as it was; MCF_ERR_INVALID for a null argument or an unknown memory kind.  With MCF_MEM_DEVICE only the summary words cross the bus
 * in a call (a table of one int32 per instance goes up once per handle, with the first call).  Without the rows the verdict, cycle_cost
 * and cycle_length are computed all the same. */
#define MCF_RAY_NONE 0
#define MCF_RAY_BOUNDED 1
#define MCF_RAY_CYCLE 2
#define MCF_RAY_BOUNDS 3
typedef struct mcf_ubatch_rays_io {
    int32_t memory;               /* MCF_MEM_HOST / MCF_MEM_DEVICE: where every pointer below points */
    int32_t reserved;
    /* results, any may be NULL */
    int32_t *verdict;             /* [count] MCF_RAY_* */
    int64_t *cycle_cost;          /* [count] */
    int32_t *cycle_length;        /* [count] arcs on the cycle */
    int8_t *on_cycle;             /* [count * arc_count] 1 = on the cycle */
    int64_t *label;               /* [count * node_count] */
} mcf_ubatch_rays_io;
typedef struct mcf_rbatch_rays_io {                    /* the same with flat rows: instance i's arcs at [arc_row[i], arc_row[i + 1]), nodes alike */
    int32_t memory;
    int32_t reserved;
    int32_t *verdict;             /* [count] */
    int64_t *cycle_cost;          /* [count] */
    int32_t *cycle_length;        /* [count] */
    int8_t *on_cycle;             /* [arc_row[count]] */
    int64_t *label;               /* [node_row[count]] */
} mcf_rbatch_rays_io;
typedef struct mcf_ubatch_rays_stats {     /* of the last mcf_*batch_rays / _on_host (all zero before one) */
    int64_t instances;
    int64_t none, bounded, cycle, bounds;               /* of `instances`, by verdict */
    int64_t lds_instances;        /* of `instances`, by the tier they are solved in; 0 and 0 from the host hook */
    int64_t global_instances;
    int64_t rounds;               /* rounds of all instances: two barriers and one sweep over the nodes each */
    int64_t frontier_nodes;       /* nodes of all frontiers; the first of an instance holds every node */
    int64_t inc_entries;          /* incidence entries read, pushing from the frontiers and pulling at the marked nodes */
    int64_t cycle_arcs;           /* the sum of cycle_length */
    double kernel_ns;             /* round the launches, synchronised */
    int64_t bytes_up, bytes_down; /* MCF_MEM_DEVICE: the summary words; MCF_MEM_HOST adds the arrays */
} mcf_ubatch_rays_stats;
MCF_API int mcf_ubatch_rays(mcf_ubatch *b, const mcf_ubatch_rays_io *io);
/* TEST HOOK: the same step (uniform_rays, csrc/rays_step.hip.h) with one lane on the CPU.  io->memory must be MCF_MEM_HOST. */
MCF_API int mcf_ubatch_rays_on_host(mcf_ubatch *b, const mcf_ubatch_rays_io *io);
MCF_API int mcf_ubatch_get_rays_stats(mcf_ubatch *b, mcf_ubatch_rays_stats *out);
MCF_API int mcf_rbatch_rays(mcf_rbatch *b, const mcf_rbatch_rays_io *io);
MCF_API int mcf_rbatch_rays_on_host(mcf_rbatch *b, const mcf_rbatch_rays_io *io);
MCF_API int mcf_rbatch_get_rays_stats(mcf_rbatch *b, mcf_ubatch_rays_stats *out);

#ifdef __cplusplus
}
#endif
#endif /* MCF_HIP_H */
