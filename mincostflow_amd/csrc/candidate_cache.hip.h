// candidate_cache.hip.h -- the device-facing side of the exact candidate cache of the resident engine (included by engine.hip only, inside its
// anonymous namespace, after the resident-grid helpers it posts and collects with).  The cache's decision state and its rules -- epochs, heap,
// list, admission, decide, install -- are candidate_state.h (plain C++, checked on a CPU by tools/candidate_state_check.cpp); here is what
// needs the engine: what the device has not heard yet, posting a search, polling for its records.  DESIGN.md section 3.4.
#pragma once

// ------------------------------------------------------------------------------------------------ candidate cache
// The list is refreshed ASYNCHRONOUSLY: when it runs low the next device search is posted while the host keeps answering from the current
// list; its answer is installed when it has arrived.  The host only waits for the device when it cannot decide: after a big subtree
// moved, or when the list ran out above the threshold.
static_assert(kCandNone == kNone, "the state's 'no arc' is the kernels'");
constexpr int kCandRefreshLow = 12;            // entries left on the list when the next one is asked for
constexpr int kCandMaxAvgDegree = 24;           // denser graphs: a single moved node already touches too many arcs

inline const int64_t *cand_pi(const mcf_engine *e) { return e->ext_pi ? e->ext_pi : e->pi.data(); }
// what the cache's evaluations read: the host mirrors as they are now
inline CandGraph cand_graph(const mcf_engine *e)
{
    return CandGraph{e->adj_start.data(), e->adj.data(), e->h_src.data(), e->h_tgt.data(), e->h_cost.data(), e->h_state.data(), cand_pi(e)};
}

// a potential / state change reported by the caller (the mirrors e->pi / e->h_state already hold the new value)
inline void cand_note_node(mcf_engine *e, int u, bool sigma_known = false, int64_t sigma = 0)
{
    if (e->rc_mode) {            // the RC layout's resident grid takes {node, shift} entries: one per occurrence (shifts add up)
        if (sigma_known) e->rc_sync.push_back(mcf_engine::NodeShift{u, sigma});
        else e->rc_shift_unknown = true;
    }
    if (e->blind_count > 0 && e->blind_epoch == e->cand_now) e->blind_sets = 2;      // may repeat a node of the big list with a newer value: that list's values are read again
    if (cand_state_note_node(e, u, e->adj_start.data())) e->sync_nodes.push_back(u);
}
inline void cand_note_arc(mcf_engine *e, int a)
{
    if (cand_state_note_arc(e, a)) e->sync_arcs.push_back(a);
}
// Long lists (a big subtree): nothing will be evaluated here -- the device searches next, and a list of its epoch or later makes the
// touched nodes' stamps irrelevant (cand_decide) -- so the list is taken over as it is, without a look at its nodes.
constexpr int kShiftRunMax = 256;           // nodes per pair: a longer run comes as several (a thread of the grid sets one pair's bits)

// a big list that came as runs, as node ids after all (for the paths that read ids): the first blind_count entries of pend_node
inline void cand_materialise_blind(mcf_engine *e)
{
    if (!e->blind_lazy) return;
    e->blind_lazy = false;
    std::vector<int32_t> ids;
    ids.reserve(e->blind_count);
    for (size_t r = 0; r + 1 < e->blind_runs.size(); r += 2)
        for (uint32_t k = 0; k < e->blind_runs[r + 1]; ++k) ids.push_back((int32_t)(e->blind_runs[r] + k));
    e->blind_runs.clear();
    e->pend_node.insert(e->pend_node.begin(), ids.begin(), ids.end());
    e->pend_val.insert(e->pend_val.begin(), ids.size(), 0);
    if (!e->shift_grid) { const int64_t *pi = cand_pi(e); for (size_t i = 0; i < ids.size(); ++i) e->pend_val[i] = pi[ids[i]]; }
}

int resident_stop(mcf_engine *e);
// mcf_engine_shift_potential_runs on the shift grid: the runs are the list (one shift for all of it, bound potentials)
inline int cand_note_runs_blind(mcf_engine *e, int32_t n_runs, const int32_t *first, const int32_t *length, int64_t total, bool continuation)
{
    e->pivot_overflow = true;
    if (e->blind_count == 0) { e->blind_epoch = e->cand_now; e->blind_sets = 0; }
    if (!continuation) {
        e->blind_sets += 1;
        if (e->blind_sets > 1 && e->stream_lines > 0) { const int rc = resident_stop(e); if (rc) return rc; }
    }
    if (e->blind_count > 0 && !e->blind_lazy) {
        // ids are there already (another call brought them): one form per list -- these runs become ids too
        for (int r = 0; r < n_runs; ++r) for (int k = 0; k < length[r]; ++k) e->pend_node.push_back(first[r] + k);
        e->pend_val.resize(e->pend_node.size(), 0);
        e->blind_count = e->pend_node.size();
    } else {
        e->blind_lazy = true;
        for (int r = 0; r < n_runs; ++r)
            for (int32_t at = 0; at < length[r]; at += kShiftRunMax) {
                e->blind_runs.push_back((uint32_t)(first[r] + at));
                e->blind_runs.push_back((uint32_t)std::min<int32_t>(kShiftRunMax, length[r] - at));
            }
        e->blind_count += (size_t)total;
    }
    if (e->async_posted && cand_records_ready(e, 0)) { const int rc = cand_collect(e, e->async_at); if (rc) return rc; }
    shift_stream(e);
    return MCF_OK;
}

inline int cand_note_nodes_blind(mcf_engine *e, int32_t count, const int32_t *nodes, const int64_t *values, bool continuation)
{
    if (e->blind_lazy) {
        // runs are there already: lines of them may have travelled in their own format, which the ids that follow cannot continue
        if (e->shift_streamed > 0) { const int rc = resident_stop(e); if (rc) return rc; }
        cand_materialise_blind(e);
    }
    e->pivot_overflow = true;
    if (e->blind_count == 0) { e->blind_epoch = e->cand_now; e->blind_sets = 0; }
    if (!continuation) {
        e->blind_sets += 1;
        // a second list may repeat nodes of the first with other values: whatever of the first has travelled is applied again, in order
        if (e->blind_sets > 1 && e->stream_lines > 0) { const int rc = resident_stop(e); if (rc) return rc; }
    }
    e->pend_node.insert(e->pend_node.end(), nodes, nodes + count);
    if (values) e->pend_val.insert(e->pend_val.end(), values, values + count);
    else {
        // the bound array holds them; the shift grid never reads a big list's values (cand_post_shift sends the shift, or takes the values
        // of that moment from the array itself)
        const size_t at = e->pend_val.size();
        e->pend_val.resize(at + (size_t)count);
        if (!e->shift_grid) for (int i = 0; i < count; ++i) e->pend_val[at + i] = e->ext_pi[nodes[i]];
    }
    e->blind_count = e->pend_node.size();
    // a list refresh that has arrived meanwhile is taken in now, so that this list can start travelling
    if (e->async_posted && cand_records_ready(e, 0)) { const int rc = cand_collect(e, e->async_at); if (rc) return rc; }
    if (e->shift_grid) shift_stream(e);
    else resident_stream(e);
    return MCF_OK;
}

// true: *k holds the entering arc (or "none": the scan would find nothing either) without asking the device
bool cand_decide(mcf_engine *e, Key *k)
{
    mcf_engine::CandKey win;
    if (!cand_decide(static_cast<CandState *>(e), &win)) return false;
    k->c = win.p == kNone ? 0 : win.c;
    k->r = 0;
    k->p = win.p;
    return true;
}

// the request for a device search: every node / arc changed since the last request, with their CURRENT values
int cand_build_patches(mcf_engine *e)
{
    // Every entry of a node must carry the same value (the device applies a list in no particular order).  Entries gathered here do (they
    // are read from the mirror now); the big lists do when they are ONE pivot's list of this very epoch (its pieces repeat no node
    // and nothing can have changed since) -- otherwise their values are read again too, and nothing of them may have travelled yet.
    const int64_t *pi = cand_pi(e);
    const size_t n_b = e->blind_count, n_s = e->sync_nodes.size();
    const bool blind_current = n_b == 0 || (e->blind_epoch == e->cand_now && e->blind_sets <= 1);
    // lists may repeat nodes (the update kernels take that: same value every time): squeeze the repeats out when they do not fit
    const bool squeeze = (int64_t)n_b + (int64_t)n_s > e->patch_capacity;
    if ((!blind_current || squeeze) && e->stream_lines > 0) { const int rc = resident_stop(e); if (rc) return rc; }
    if (squeeze) {
        e->pend_node.insert(e->pend_node.end(), e->sync_nodes.begin(), e->sync_nodes.end());
        std::sort(e->pend_node.begin(), e->pend_node.end());
        e->pend_node.erase(std::unique(e->pend_node.begin(), e->pend_node.end()), e->pend_node.end());
        e->pend_val.resize(e->pend_node.size());
        for (size_t i = 0; i < e->pend_node.size(); ++i) e->pend_val[i] = pi[e->pend_node[i]];
    } else {
        if (!blind_current) for (size_t i = 0; i < n_b; ++i) e->pend_val[i] = pi[e->pend_node[i]];
        e->pend_node.resize(n_b + n_s);
        e->pend_val.resize(n_b + n_s);
        for (size_t i = 0; i < n_s; ++i) { e->pend_node[n_b + i] = e->sync_nodes[i]; e->pend_val[n_b + i] = pi[e->sync_nodes[i]]; }
    }
    e->pend_arc.assign(e->sync_arcs.begin(), e->sync_arcs.end());
    e->pend_state.resize(e->pend_arc.size());
    for (size_t i = 0; i < e->pend_arc.size(); ++i) e->pend_state[i] = e->h_state[e->pend_arc[i]];
    e->sync_nodes.clear();
    e->sync_arcs.clear();
    blind_clear(e);
    e->rc_sync.clear();
    e->rc_shift_unknown = false;
    return MCF_OK;
}

bool cand_records_ready(const mcf_engine *e, int g)
{
    const volatile Slot *rec = e->h_slots + (size_t)g * kCandRecords;
    for (int r = 0; r < kCandRecords; ++r) { const int64_t c = rec[r].c; const uint32_t q = rec[r].p; if (rec[r].tag != record_tag(e->seq, c, q)) return false; }
    return true;
}

// wait for the candidate records of request e->seq and install them as the list of epoch `at`
int cand_collect(mcf_engine *e, uint32_t at)
{
    const double t0 = (double)__rdtsc();
    double t0_wall = 0;
    const volatile Slot *slots = e->h_slots;
    e->cand_records.clear();
    mcf_engine::CandKey thr{0, kNone};          // the smallest key that was NOT reported
    for (int g = 0; g < e->res_grid; ++g) {
        const volatile Slot *rec = slots + (size_t)g * kCandRecords;
        uint64_t spins = 0;
        while (!cand_records_ready(e, g)) {
            _mm_pause();
            if (e->resident_running && (spins & 0xFFF) == 0xFFF && ((const volatile uint32_t *)e->h_exit)[0] != 0) {
                if (((const volatile uint32_t *)e->h_exit)[0] == kExitPartial) {
                    (void)resident_join(e, false);
                    e->resident_running = false;
                    resident_slot_release(e);
                    return mcf::fail(MCF_ERR_TIMEOUT, "the resident grid could not meet at its grid-wide barrier while a list was being applied (are its workgroups all resident?): the device arrays are undefined");
                }
                int rc = resident_restart(e);
                if (rc) return rc;
            }
            if ((++spins & 0xFFFFF) == 0) {
                const hipError_t q = hipStreamQuery(e->res_stream ? e->res_stream : e->stream);
                if (q != hipSuccess && q != hipErrorNotReady) return mcf::fail(MCF_ERR_HIP, "resident grid failed: %s", hipGetErrorString(q));
                if (t0_wall == 0) t0_wall = mcf::now_ns();
                else if (mcf::now_ns() - t0_wall > 20e9) return mcf::fail(MCF_ERR_TIMEOUT, "no answer from the device after 20 s (workgroup %d of %d)", g, e->res_grid);
            }
        }
        std::atomic_thread_fence(std::memory_order_acquire);
        for (int r = 0; r < kCandPerGroup; ++r)
            if (rec[r].p != kNone) e->cand_records.push_back(mcf_engine::CandKey{rec[r].c, rec[r].p});
        if (rec[kCandPerGroup].p != kNone) {
            const mcf_engine::CandKey t{rec[kCandPerGroup].c, rec[kCandPerGroup].p};
            if (thr.p == kNone || cand_key_less(t, thr)) thr = t;
        }
    }
    e->wait_ticks += (double)__rdtsc() - t0;
    cand_install(e, cand_graph(e), e->cand_records.data(), e->cand_records.size(), thr, at);
    e->tk_collect += (double)__rdtsc() - t0;
    return MCF_OK;
}

// posts a device search that carries everything the device has not heard yet; its list will be of epoch cand_now
// RC layout: the request carries {node, shift} entries -- every occurrence of a node since the last request with the shift of that pivot (the
// pivots' own small lists), plus this pivot's one big list with its common shift when it is short enough -- or, when that is not possible
// (a shift that was not announced, too many entries), the grid is stopped and the values go through update_rc_kernel.
int cand_post_rc(mcf_engine *e)
{
    // a reload of the bound potentials that the grid can carry out itself (kCmdReload): the array is read when the request is served, so every
    // potential change noted up to now is part of it -- the lists are dropped, the state writes travel with the request
    const bool reload = e->reload_pi && e->d_ext_pi != nullptr && (int64_t)e->sync_arcs.size() <= e->mailbox_max_st;
    if (reload) {
        pend_clear_potentials(e);
        e->sync_nodes.clear(); e->rc_sync.clear(); e->rc_shift_unknown = false;
        blind_clear(e);
        e->reload_pi = false;
    }
    const size_t n_b = e->blind_count, n_s = e->rc_sync.size();
    const bool blind_ok = n_b == 0 || (e->pend_shift && e->blind_epoch == e->cand_now);      // shifts add up: a node may sit in both lists
    const int64_t n_st = (int64_t)e->sync_arcs.size();
    const bool fast = !e->reload_pi && !e->rc_shift_unknown && blind_ok && (int64_t)(n_b + n_s) <= (int64_t)e->rc_list_max && n_st <= e->mailbox_max_st;
    if (fast) {
        e->pend_node.resize(n_b + n_s);
        e->pend_val.resize(n_b + n_s);
        for (size_t i = 0; i < n_b; ++i) e->pend_val[i] = e->pend_sigma;
        for (size_t i = 0; i < n_s; ++i) { e->pend_node[n_b + i] = e->rc_sync[i].node; e->pend_val[n_b + i] = e->rc_sync[i].shift; }
        e->pend_arc.assign(e->sync_arcs.begin(), e->sync_arcs.end());
        e->pend_state.resize(e->pend_arc.size());
        for (size_t i = 0; i < e->pend_arc.size(); ++i) e->pend_state[i] = e->h_state[e->pend_arc[i]];
        e->sync_nodes.clear(); e->sync_arcs.clear(); e->rc_sync.clear();
        blind_clear(e);
    } else {
        if (int rcb = cand_build_patches(e)) return rcb;        // {node, current value} lists
        int rc = resident_stop(e);
        if (!rc) rc = flush_pending(e);                          // update_rc_kernel: the device works the differences out itself
        if (rc) return rc;
    }
    next_request_keep_prev(e);
    int rc = resident_start(e, e->prev_seq);
    if (rc) return rc;
    resident_post(e, e->seq, reload ? kCmdReload : kCmdScan, fast);
    if (reload) e->st.rc_reloads_in_grid += 1;
    if (fast && (!e->pend_node.empty() || !e->pend_arc.empty())) e->st.inline_updates += 1;
    pend_clear(e);
    e->posted_at = e->cand_now;
    e->st.arcs_scanned += e->end - e->begin;
    return MCF_OK;
}

// ---- the grid that is patched straight from the request (resident_cand_kernel; mailbox.hip.h has the layout of its requests)

// After that grid has left: the arrays in device memory are as the LAST LAUNCH found them.  The host's mirrors are authoritative in candidate
// mode (potentials: the bound array or e->pi; states: h_state), so they are simply written again -- and with that the device has heard
// everything: whatever was waiting to be told is dropped.
int device_sync_from_mirrors(mcf_engine *e)
{
    const int64_t *pi = cand_pi(e);
    HIP_TRY(hipMemcpyAsync(e->d_pi, pi, sizeof(int64_t) * (size_t)e->d.node_count, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(e->d_state, e->h_state.data() + e->begin, (size_t)(e->end - e->begin), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    pend_clear(e);
    e->pend_shift = false;
    e->sync_nodes.clear(); e->sync_arcs.clear(); e->rc_sync.clear(); e->rc_shift_unknown = false;
    blind_clear(e); e->blind_sets = 0;
    e->shift_streamed = 0;
    e->reload_pi = false;              // the whole array has just been copied
    e->st.mirror_uploads += 1;
    return MCF_OK;
}

// shift lines [from, to) of a list of n entries, with the tag seq: node ids out of pend_node, or (runs) {first, length} pairs out of blind_runs
void shift_write_lines(mcf_engine *e, int from, int to, size_t n, bool runs, uint32_t seq)
{
    const int per_line = runs ? kShiftPairsPerLine : kShiftNodesPerLine;
    MailboxLine line;
    for (int l = from; l < to; ++l) {
        memset(line.w, 0, sizeof(line.w));
        for (int k = 0; k < per_line && (size_t)l * per_line + k < n; ++k) {
            const size_t i = (size_t)l * per_line + k;
            if (runs) { line.w[2 * k] = e->blind_runs[2 * i]; line.w[2 * k + 1] = e->blind_runs[2 * i + 1]; }
            else line.w[k] = (uint32_t)e->pend_node[i];
        }
        line.w[15] = seq;
        mailbox_write_line(e->mailbox + e->shift_base + 16 * (size_t)l, line.w);
    }
}

// header (+ entry and shift lines when with_patches) of request `seq`; the value entries are pend_node / pend_val [val_lo, end), the shift
// list pend_node [0, n_shift)
void shift_post_request(mcf_engine *e, uint32_t seq, uint32_t cmd, size_t val_lo, size_t n_shift, int64_t sigma, bool with_patches, bool runs = false)
{
    const int n_val = with_patches ? (int)(e->pend_node.size() - val_lo) : 0, n_st = with_patches ? (int)e->pend_arc.size() : 0;
    const ValueEntries vals{e->pend_node.data(), e->pend_val.data(), val_lo + 1, n_val > 1 ? n_val - 1 : 0};
    const StateEntries sts{e->pend_arc.data(), e->pend_state.data(), 2, n_st > 2 ? n_st - 2 : 0};
    const MailboxLine line1 = mailbox_encode_entries(e->mailbox, vals, sts, seq);
    if (with_patches) {
        // the shift list: n_shift node ids, or (runs) n_shift {first, length} pairs out of blind_runs
        const int per_line = runs ? kShiftPairsPerLine : kShiftNodesPerLine;
        shift_write_lines(e, e->shift_streamed, (int)((n_shift + per_line - 1) / per_line), n_shift, runs, seq);
        e->shift_streamed = 0;
    }
    MailboxLine h = request_header(e, seq, cmd, n_st, n_val, val_lo);
    h.w[kShHdrValues] = (uint32_t)n_val;
    h.w[kShHdrShift] = with_patches ? (uint32_t)n_shift : 0u;
    h.w[kShHdrRuns] = with_patches && runs ? 1u : 0u;
    h.w[kShHdrSigma] = (uint32_t)(uint64_t)sigma;
    h.w[kShHdrSigma + 1] = (uint32_t)((uint64_t)sigma >> 32);
    mailbox_publish(e->mailbox, kPollReplicas, h, vals.n + sts.n > 0 ? &line1 : nullptr);
}
// a request without patches: quit, or a scan request put there again for a grid that has just been started with current arrays
void shift_post(mcf_engine *e, uint32_t seq, uint32_t cmd, bool) { shift_post_request(e, seq, cmd, 0, 0, 0, false); }

// the complete shift lines of this pivot's big list start travelling while the host is still walking the subtree (kCmdApply / kCmdApplyRuns:
// "shift lines 0 .. L-1 of the coming scan request are in place": the grid sets their bits and goes back to polling)
constexpr int kShiftStreamMinLines = 96;
void shift_stream(mcf_engine *e)
{
    if (e->async_posted || e->blind_epoch != e->cand_now || e->blind_sets > 1 || !e->pend_shift) return;
    if (!e->resident_running || e->in_flight != mcf_engine::kNoSearch) return;
    const bool runs = e->blind_lazy;
    const int complete = runs ? (int)(e->blind_runs.size() / 2 / kShiftPairsPerLine) : (int)(e->blind_count / kShiftNodesPerLine);
    if (complete - e->shift_streamed < kShiftStreamMinLines || complete > e->max_shift_lines) return;
    const uint32_t next_seq = peek_request(e);
    shift_write_lines(e, e->shift_streamed, complete, runs ? e->blind_runs.size() / 2 : e->blind_count, runs, next_seq);
    e->stream_sub += 1;
    if (e->stream_sub == 0) e->stream_sub = 1;
    MailboxLine h = request_header(e, next_seq, runs ? kCmdApplyRuns : kCmdApply);
    h.w[kShHdrShift] = (uint32_t)complete;
    h.w[kShHdrApplySub] = e->stream_sub;
    mailbox_publish(e->mailbox, kPollReplicas, h, nullptr);
    e->shift_streamed = complete;
    e->stream_lines = complete;                    // "a list is travelling": what the other paths test before they change their mind about it
}

// posts a device search on that grid: this pivot's one big list as a shift list when it qualifies, everything else the device has not heard
// as {node, current value} entries; anything that does not fit the scheme stops the grid, which brings the device up to date wholesale
int cand_post_shift(mcf_engine *e)
{
    if (!e->resident_running) {                     // (re)start first: a start after a stop finds the arrays current and nothing left to tell
        const int rc = resident_start(e, e->seq);
        if (rc) return rc;
    }
    if (e->reload_pi) {
        // mcf_engine_reload_potentials: the grid reads the bound array when it serves the request (kCmdReload), so every potential change noted up to
        // now is part of it -- the lists are dropped, the state writes travel with the request.  (A grid that has just been started read the
        // arrays the host wrote from its mirrors: nothing to reload, resident_start cleared the flag.)
        if (!e->d_ext_pi || e->shift_streamed > 0 || (int64_t)e->sync_arcs.size() > (int64_t)e->mailbox_max_st) {
            int rc = resident_stop(e);              // device_sync_from_mirrors: nothing is left to tell
            if (!rc) rc = resident_start(e, e->seq);
            if (rc) return rc;
        }
    }
    if (e->reload_pi) {
        pend_clear_potentials(e);
        e->sync_nodes.clear();
        blind_clear(e);
        e->pend_arc.assign(e->sync_arcs.begin(), e->sync_arcs.end());
        e->pend_state.resize(e->pend_arc.size());
        for (size_t i = 0; i < e->pend_arc.size(); ++i) e->pend_state[i] = e->h_state[e->pend_arc[i]];
        next_request_keep_prev(e);
        shift_post_request(e, e->seq, kCmdReload, 0, 0, 0, true);
        e->st.rc_reloads_in_grid += 1;
        e->pend_arc.clear(); e->pend_state.clear();
        e->sync_arcs.clear();
        e->stream_lines = 0;
        e->reload_pi = false;
        e->posted_at = e->cand_now;
        e->st.arcs_scanned += e->end - e->begin;
        return MCF_OK;
    }
    for (int attempt = 0; attempt < 2; ++attempt) {
        const size_t n_b = e->blind_count, n_s = e->sync_nodes.size();
        const bool blind_current = n_b == 0 || (e->blind_epoch == e->cand_now && e->blind_sets <= 1);
        const size_t n_pairs = e->blind_lazy ? e->blind_runs.size() / 2 : 0;
        const bool as_shift = n_b > 0 && blind_current && e->pend_shift &&
                              (e->blind_lazy ? n_pairs <= (size_t)e->max_shift_lines * kShiftPairsPerLine : n_b <= (size_t)e->max_shift_lines * kShiftNodesPerLine);
        const bool fits = (int64_t)(as_shift ? n_s : n_b + n_s) <= (int64_t)e->patch_capacity && (int64_t)e->sync_arcs.size() <= (int64_t)e->mailbox_max_st;
        if ((!as_shift && e->shift_streamed > 0) || !fits) {
            // lines of a list that is no shift list any more have travelled, or the request would not fit: bring the device up to date wholesale
            int rc = resident_stop(e);              // device_sync_from_mirrors: nothing is left to tell
            if (!rc) rc = resident_start(e, e->seq);
            if (rc) return rc;
            continue;
        }
        const int64_t *pi = cand_pi(e);
        const bool runs = as_shift && e->blind_lazy;          // the pairs travel as they are; pend_node then holds the value entries only
        if (!as_shift) cand_materialise_blind(e);              // ... as ids otherwise
        const size_t base = runs ? 0 : n_b, val_lo = as_shift ? base : 0;
        if (!as_shift) for (size_t i = 0; i < n_b; ++i) e->pend_val[i] = pi[e->pend_node[i]];      // current values (a node named twice carries the same one)
        e->pend_node.resize(base + n_s);
        e->pend_val.resize(base + n_s);
        for (size_t i = 0; i < n_s; ++i) { e->pend_node[base + i] = e->sync_nodes[i]; e->pend_val[base + i] = pi[e->sync_nodes[i]]; }
        e->pend_arc.assign(e->sync_arcs.begin(), e->sync_arcs.end());
        e->pend_state.resize(e->pend_arc.size());
        for (size_t i = 0; i < e->pend_arc.size(); ++i) e->pend_state[i] = e->h_state[e->pend_arc[i]];
        next_request_keep_prev(e);
        shift_post_request(e, e->seq, kCmdScan, val_lo, as_shift ? (runs ? n_pairs : n_b) : 0, e->pend_sigma, true, runs);
        if (!e->pend_node.empty() || !e->pend_arc.empty()) e->st.inline_updates += 1;
        if (as_shift) e->st.shift_lists += 1;
        pend_clear(e);
        e->sync_nodes.clear(); e->sync_arcs.clear();
        blind_clear(e);
        e->stream_lines = 0;
        e->posted_at = e->cand_now;
        e->st.arcs_scanned += e->end - e->begin;
        return MCF_OK;
    }
    return mcf::fail(MCF_ERR_STATE, "cand_post_shift: the request does not fit an empty mailbox");
}

int cand_post(mcf_engine *e)
{
    if (e->shift_grid) return cand_post_shift(e);
    if (e->rc_mode) return cand_post_rc(e);
    if (int rcb = cand_build_patches(e)) return rcb;
    if ((int)e->pend_arc.size() > e->mailbox_max_st) {      // hundreds of pivots' worth of state writes: cannot happen between two requests, kept for safety
        int rc = resident_stop(e);
        if (!rc) rc = flush_pending(e);
        if (rc) return rc;
    }
    next_request_keep_prev(e);
    int rc = resident_start(e, e->prev_seq);
    if (rc) return rc;
    resident_post(e, e->seq, kCmdScan, true);
    if (!e->pend_node.empty() || !e->pend_arc.empty()) e->st.inline_updates += 1;
    pend_clear(e);
    e->posted_at = e->cand_now;
    e->st.arcs_scanned += e->end - e->begin;
    return MCF_OK;
}

// the host mirrors' arc lists per node, with what a re-evaluation needs next to each other (upload, mcf_engine_patch_arcs)
void cand_build_adjacency(mcf_engine *e)
{
    const int n = e->d.node_count, m_s = e->d.search_arc_num;
    const int32_t *source = e->h_src.data(), *target = e->h_tgt.data();
    // an arc shard keeps its own cache: the list, the heap and this adjacency cover the arcs [begin, end) it holds, the answer is the shard's
    // candidate (mcf_engine_search_end_local) and the holders' MINLOC does the rest
    const int lo = e->begin, hi = std::min(e->end, m_s);
    e->adj_start.assign(n + 1, 0);
    for (int a = lo; a < hi; ++a) { e->adj_start[source[a] + 1]++; if (target[a] != source[a]) e->adj_start[target[a] + 1]++; }
    for (int u = 0; u < n; ++u) e->adj_start[u + 1] += e->adj_start[u];
    e->adj.assign(e->adj_start[n], mcf_engine::AdjEnt{0, 0u, 0});
    e->adj_pos.assign((size_t)2 * m_s, -1);
    std::vector<int32_t> fill(e->adj_start.begin(), e->adj_start.end() - 1);
    for (int a = lo; a < hi; ++a) {
        const uint32_t st_bits = (uint32_t)(e->h_state[a] + 1) << 29;
        e->adj_pos[2 * (size_t)a] = fill[source[a]];
        e->adj[fill[source[a]]++] = mcf_engine::AdjEnt{a, (uint32_t)target[a] | st_bits, e->h_cost[a]};
        if (target[a] != source[a]) {
            e->adj_pos[2 * (size_t)a + 1] = fill[target[a]];
            e->adj[fill[target[a]]++] = mcf_engine::AdjEnt{a, (uint32_t)source[a] | st_bits | 0x80000000u, e->h_cost[a]};
        }
    }
}


