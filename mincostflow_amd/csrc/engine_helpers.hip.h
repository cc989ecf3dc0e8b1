// engine_helpers.hip.h -- the few decisions the engine's host side takes in many places, each stated once (included by engine.hip only,
// inside its anonymous namespace, after struct mcf_engine): a search's header, the rule's key ordering, the way from an engine to a
// kernel's template arguments, the launch call, the request number and the pending lists.
#pragma once

#include <type_traits>

// ---- a search's header: what every launch, post and merge of one search must agree on
struct SearchHeader {
    int next_arc;      // where the cyclic scan starts: the engine's next_arc, m_s wrapped to 0
    int rstar;         // OPTIMIZED Block Search: the block that holds the end of the first range [next_arc, m_s) when that range ends inside a
                       // block (BSPO.cs:49) -- its wrapped half ranks behind its first half (D14); -1: no such block
    int block_size;
    bool dual;         // OPTIMIZED Block Search: every record line carries a block key and a range key (kernels.hip.h: kDual)
    // arc (>= 0) lies in the wrapped range [0, next_arc)
    uint32_t wrapped(int arc) const { return arc < next_arc ? 1u : 0u; }
    // Key::r of scan position p, which is `arc`: twice the block, + 1 in the wrapped half of the boundary block
    uint32_t block_rank(uint32_t p, int arc) const
    {
        const uint32_t r = p / (uint32_t)block_size;
        return 2 * r + (rstar >= 0 && (int)r == rstar ? wrapped(arc) : 0u);
    }
};
inline SearchHeader search_header(int rule, int semantics, int m_s, int next_arc, int block_size)
{
    SearchHeader h{next_arc >= m_s ? 0 : next_arc, -1, block_size, rule == MCF_RULE_BLOCK_SEARCH && semantics == MCF_SEM_OPTIMIZED};
    if (h.dual && next_arc < m_s) {
        const int len1 = m_s - next_arc;   // BSPO.cs:49 first range
        if (len1 % block_size != 0) h.rstar = len1 / block_size;
    }
    return h;
}
inline SearchHeader search_header(const mcf_engine *e) { return search_header(e->d.rule, e->d.semantics, e->d.search_arc_num, e->next_arc, e->block_size); }

// ---- the rule's ordering of the keys, as the kernels have it: does k come before best?  (Best Eligible keys carry r == 0.)
inline bool key_better(int rule, const Key &k, const Key &best)
{
    if (rule != MCF_RULE_BEST_ELIGIBLE && rule != MCF_RULE_BLOCK_SEARCH) return k.p < best.p;       // First Eligible: scan order alone
    if (best.p == kNone) return true;
    if (k.r != best.r) return k.r < best.r;
    return k.c < best.c || (k.c == best.c && k.p < best.p);
}
// range keys (OPTIMIZED Block Search): r = SearchHeader::wrapped
inline bool range_better(const Key &q, const Key &range) { return key_better(MCF_RULE_BLOCK_SEARCH, q, range); }

// ---- from the engine to template arguments: f(RULE, OPT) as integral constants, f(T{}) with the width's integer type
template <typename F>
auto with_rule(const mcf_engine *e, F &&f)
{
    switch (e->d.rule) {
    case MCF_RULE_BEST_ELIGIBLE: return f(std::integral_constant<int, MCF_RULE_BEST_ELIGIBLE>{}, std::false_type{});
    case MCF_RULE_FIRST_ELIGIBLE: return f(std::integral_constant<int, MCF_RULE_FIRST_ELIGIBLE>{}, std::false_type{});
    default:
        if (e->d.semantics == MCF_SEM_OPTIMIZED) return f(std::integral_constant<int, MCF_RULE_BLOCK_SEARCH>{}, std::true_type{});
        return f(std::integral_constant<int, MCF_RULE_BLOCK_SEARCH>{}, std::false_type{});
    }
}
template <typename F>
auto with_width(const mcf_engine *e, F &&f)
{
    return e->d.int_width == 32 ? f(int32_t{}) : f(int64_t{});
}

// ---- one launch call: timed by the two events when they are given
template <typename... Params, typename... Args>
void launch(void (*kernel)(Params...), dim3 grid, dim3 block, hipStream_t stream, hipEvent_t start, hipEvent_t stop, const Args &...args)
{
    if (start) hipExtLaunchKernelGGL(kernel, grid, block, 0, stream, start, stop, 0, args...);
    else hipLaunchKernelGGL(kernel, grid, block, 0, stream, args...);
}

// ---- the request number: never 0 (what a fresh mailbox and fresh records hold)
inline uint32_t peek_request(const mcf_engine *e) { const uint32_t next = e->seq + 1; return next ? next : 1; }
inline uint32_t next_request(mcf_engine *e) { return e->seq = peek_request(e); }
// ... for a request that a grid may have to be started for: it starts behind the previous request (resident_start, resident_restart)
inline uint32_t next_request_keep_prev(mcf_engine *e) { e->prev_seq = e->seq; return next_request(e); }

// ---- the pending lists
inline void pend_clear_potentials(mcf_engine *e) { e->pend_node.clear(); e->pend_val.clear(); }
inline void pend_clear(mcf_engine *e) { pend_clear_potentials(e); e->pend_arc.clear(); e->pend_state.clear(); }
