// esim_host_flows.h -- how the epidemic travels between Output Areas: esim_area_flows, esim_area_imports, esim_area_invasion (on
// top of tree_enqueue / tree_finish) and esim_lineage_areas (on top of chains_enqueue / chains_finish); the kernels:
// esim_kernels_flows.h, the pair engine under the two sparse outputs: esim_pairs.h; DESIGN 20.  All four work in temporary
// device memory that lives as long as the call, and leave the context as it is.
namespace {

// The pair engine of one call: the table, the dense array behind it and two counters (distinct pairs, keys dropped).
struct PairWork {
    DevTmp<unsigned long long> key, out_key;
    DevTmp<uint32_t> cnt, out_cnt, counters;
    PairTable t;
    uint32_t dense = 0;                 // pairs the dense array holds, a power of two
    uint32_t n = 0, dropped = 0;        // after pairs_sorted
    hipEvent_t ev[4] = { nullptr, nullptr, nullptr, nullptr };   // around insert, compact and sort
    ~PairWork() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
};

// The table for at most n_keys inserts, emptied on the stream: the smallest power of two >= 2 * n_keys, at least 64, so that it
// is never more than half full -- or 1 << ESIM_PAIR_LOG2.  The kernels that insert go between pairs_begin and pairs_sorted.
int pairs_begin(esim_ctx_impl *c, const std::string &who, PairWork *w, uint32_t n_keys)
{
    const uint32_t knob = c->tune.pair_log2;
    if (!knob && n_keys > 0x40000000u) return fail(c, ESIM_ENOMEM, who + ": more than 2^30 entries of the exposure log can fall into the window: the pair table is not built for them");
    const uint32_t cap = knob ? 1u << knob : std::max(64u, pair_pow2(2ull * n_keys));
    w->dense = std::min(cap, std::max(64u, pair_pow2(n_keys)));
    if (w->key.alloc(cap) != hipSuccess || w->cnt.alloc(cap) != hipSuccess || w->out_key.alloc(w->dense) != hipSuccess || w->out_cnt.alloc(w->dense) != hipSuccess ||
        w->counters.alloc(2) != hipSuccess) {
        (void)hipGetLastError();
        return fail(c, ESIM_ENOMEM, who + ": no device memory for the pair table (12 B per slot, " + std::to_string(cap) + " slots, and 12 B per pair of the dense array)");
    }
    w->t.key = w->key.p; w->t.cnt = w->cnt.p; w->t.cap = cap; w->t.overflow = w->counters.p + 1;
    hipError_t e = hipSuccess;
    for (hipEvent_t &ev : w->ev) if (e == hipSuccess) e = hipEventCreate(&ev);
    if (e == hipSuccess) e = hipEventRecord(w->ev[0], c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(w->key.p, 0xFF, sizeof(unsigned long long) * cap, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(w->cnt.p, 0, sizeof(uint32_t) * cap, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(w->out_key.p, 0xFF, sizeof(unsigned long long) * w->dense, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(w->counters.p, 0, 2 * sizeof(uint32_t), c->stream);
    if (e != hipSuccess) return fail(c, ESIM_ENODEVICE, who + ": " + hipGetErrorString(e));
    return ESIM_OK;
}

// Compact -- every pair, or with min_count > 1 those counted at least that often --, and the one read of the number of pairs kept
// (the stream is waited for: the calls wait for it anyway).  Leaves w->n and w->dropped.
int pairs_compacted(esim_ctx_impl *c, PairWork *w, uint32_t min_count)
{
    HIP_TRY(c, hipEventRecord(w->ev[1], c->stream));
    const dim3 grid(grid_capped(c, w->t.cap, PAIR_TPB, 4096)), block(PAIR_TPB);
    if (min_count > 1u) hipLaunchKernelGGL(k_pairs_compact_min, grid, block, 0, c->stream, w->t, min_count, w->out_key.p, w->out_cnt.p, w->dense, w->counters.p);
    else hipLaunchKernelGGL(k_pairs_compact, grid, block, 0, c->stream, w->t, w->out_key.p, w->out_cnt.p, w->dense, w->counters.p);
    HIP_TRY(c, hipEventRecord(w->ev[2], c->stream));
    uint32_t h[2] = { 0u, 0u };
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpy(h, w->counters.p, sizeof h, hipMemcpyDeviceToHost));
    w->n = std::min(h[0], w->dense); w->dropped = h[1];
    return ESIM_OK;
}

// Compact, read, sort.  The sorted pairs lie in w->out_key / w->out_cnt once the stream has been waited for again.
int pairs_sorted(esim_ctx_impl *c, PairWork *w)
{
    if (int rc = pairs_compacted(c, w, 1u)) return rc;
    pairs_sort_enqueue(w->out_key.p, w->out_cnt.p, pair_pow2(w->n), c->stream);
    HIP_TRY(c, hipEventRecord(w->ev[3], c->stream));
    return ESIM_OK;
}

// Behind the wait of the call: the times of the engine's three parts for esim_pair_stats, and ESIM_ENOMEM where keys were dropped.
int pairs_end(esim_ctx_impl *c, const std::string &who, PairWork *w)
{
    PairStats &s = c->pair_stats;
    s.distinct = w->n; s.capacity = w->t.cap; s.dropped = w->dropped;
    for (int k = 0; k < 3; ++k) {
        float ms = 0.0f;
        s.ms[k] = hipEventElapsedTime(&ms, w->ev[k], w->ev[k + 1]) == hipSuccess ? (double)ms : -1.0;
    }
    (void)hipGetLastError();
    if (w->dropped)
        return fail(c, ESIM_ENOMEM, who + ": the pair table of " + std::to_string(w->t.cap) + " slots (ESIM_PAIR_LOG2) is full: " + std::to_string(w->dropped) + " keys were dropped");
    return ESIM_OK;
}

// The sorted pairs to the host, split into the high and the low word of the key; 12 B per pair.
int pairs_deliver(esim_ctx_impl *c, PairWork *w, uint32_t *hi, uint32_t *lo, uint32_t *count)
{
    const size_t n = w->n;
    if (!n) return ESIM_OK;
    if (hi || lo) {
        std::vector<unsigned long long> keys(n);
        HIP_TRY(c, hipMemcpy(keys.data(), w->out_key.p, sizeof(unsigned long long) * n, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n; ++i) {
            if (hi) hi[i] = (uint32_t)(keys[i] >> 32);
            if (lo) lo[i] = (uint32_t)keys[i];
        }
    }
    if (count) HIP_TRY(c, hipMemcpy(count, w->out_cnt.p, sizeof(uint32_t) * n, hipMemcpyDeviceToHost));
    return ESIM_OK;
}

// What esim_area_flows and esim_area_imports check alike, in front of tree_check's refusals and behind them.
int flows_check(esim_ctx_impl *c, const std::string &who, uint32_t setting_mask, uint32_t first_step, uint32_t last_step)
{
    if (setting_mask == 0u || (setting_mask >> ESIM_N_SETTINGS) != 0u)
        return fail(c, ESIM_EINVAL, who + ": a setting mask that is empty or names a setting beyond ESIM_SETTING_TRANSPORT");
    if (int rc = tree_check(c, who)) return rc;
    if (first_step == 0 || last_step < first_step || last_step > c->host_t - 1u)
        return fail(c, ESIM_ERANGE, who + ": steps outside 1 .. the steps run so far, or last_step before first_step");
    return ESIM_OK;
}

// An enqueue that failed behind tree_enqueue / chains_enqueue: their kernels still read host vectors of the work struct.
int flows_unwind(esim_ctx_impl *c, int rc) { (void)hipStreamSynchronize(c->stream); return rc; }

}  // namespace

extern "C" int esim_area_flows(esim_ctx *ctx, uint32_t setting_mask, uint32_t first_step, uint32_t last_step, uint32_t *src, uint32_t *dst, uint32_t *count,
                               uint32_t cap, uint32_t *n_out)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    const std::string who = "esim_area_flows";
    if (!n_out) return fail(c, ESIM_EINVAL, who + ": null n_out");
    if (int rc = flows_check(c, who, setting_mask, first_step, last_step)) return rc;
    HIP_TRY(c, hipSetDevice(c->P.device));
    TreeWork w;
    PairWork p;
    if (int rc = tree_enqueue(c, who, &w, false)) return rc;
    const uint32_t log_len = w.s.log_len;
    if (int rc = pairs_begin(c, who, &p, log_len)) return flows_unwind(c, rc);
    hipLaunchKernelGGL(k_flow_pairs, dim3(grid_capped(c, log_len, TPB, 4096)), dim3(TPB), 0, c->stream, c->d, w.s.q, w.t, setting_mask, first_step, last_step, log_len, p.t);
    if (int rc = pairs_sorted(c, &p)) return flows_unwind(c, rc);
    const int rc = tree_finish(c, who, &w);
    if (rc && rc != ESIM_ESIM) return rc;
    if (int full = pairs_end(c, who, &p)) return full;
    *n_out = p.n;
    if (p.n > cap) return fail(c, ESIM_ERANGE, who + ": buffers too small (n_out holds the size needed)");
    if (int bad = pairs_deliver(c, &p, src, dst, count)) return bad;
    return rc;
}

extern "C" int esim_area_imports(esim_ctx *ctx, uint32_t setting_mask, uint32_t first_step, uint32_t last_step, uint32_t *local, uint32_t *imported, uint32_t *exported)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    const std::string who = "esim_area_imports";
    if (int rc = flows_check(c, who, setting_mask, first_step, last_step)) return rc;
    HIP_TRY(c, hipSetDevice(c->P.device));
    const size_t na = c->d.n_areas;
    DevTmp<uint32_t> tab;
    if (tab.alloc(3 * na) != hipSuccess) { (void)hipGetLastError(); return fail(c, ESIM_ENOMEM, who + ": no device memory for the three tables (12 B per area)"); }
    TreeWork w;
    if (int rc = tree_enqueue(c, who, &w, false)) return rc;
    HIP_TRY(c, hipMemsetAsync(tab.p, 0, sizeof(uint32_t) * std::max<size_t>(1, 3 * na), c->stream));
    if (local || imported || exported)
        hipLaunchKernelGGL(k_flow_imports, dim3(grid_capped(c, w.s.log_len, TPB, 4096)), dim3(TPB), 0, c->stream, c->d, w.s.q, w.t, setting_mask, first_step, last_step, w.s.log_len,
                           local ? tab.p : nullptr, imported ? tab.p + na : nullptr, exported ? tab.p + 2 * na : nullptr);
    const int rc = tree_finish(c, who, &w);
    if (rc && rc != ESIM_ESIM) return rc;
    const size_t bytes = sizeof(uint32_t) * na;
    if (local && bytes) HIP_TRY(c, hipMemcpy(local, tab.p, bytes, hipMemcpyDeviceToHost));
    if (imported && bytes) HIP_TRY(c, hipMemcpy(imported, tab.p + na, bytes, hipMemcpyDeviceToHost));
    if (exported && bytes) HIP_TRY(c, hipMemcpy(exported, tab.p + 2 * na, bytes, hipMemcpyDeviceToHost));
    return rc;
}

extern "C" int esim_area_invasion(esim_ctx *ctx, uint32_t *first_case, uint32_t *step, uint32_t *source_area, uint8_t *setting)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    const std::string who = "esim_area_invasion";
    if (int rc = tree_check(c, who)) return rc;
    HIP_TRY(c, hipSetDevice(c->P.device));
    const size_t na = c->d.n_areas;
    DevTmp<unsigned long long> best;
    DevTmp<uint32_t> tab;
    DevTmp<uint8_t> set;
    if (best.alloc(na) != hipSuccess || tab.alloc(3 * na) != hipSuccess || set.alloc(na) != hipSuccess) {
        (void)hipGetLastError();
        return fail(c, ESIM_ENOMEM, who + ": no device memory for the invasion tree (21 B per area)");
    }
    TreeWork w;
    if (int rc = tree_enqueue(c, who, &w, false)) return rc;
    HIP_TRY(c, hipMemsetAsync(best.p, 0xFF, sizeof(unsigned long long) * std::max<size_t>(1, na), c->stream));
    hipLaunchKernelGGL(k_flow_first, dim3(grid_capped(c, w.s.log_len, TPB, 4096)), dim3(TPB), 0, c->stream, c->d, w.s.q, w.s.log_len, best.p);
    hipLaunchKernelGGL(k_flow_resolve, dim3(grid_capped(c, na, TPB, 4096)), dim3(TPB), 0, c->stream, c->d, w.s.q, w.t, best.p, tab.p, tab.p + na, tab.p + 2 * na, set.p);
    const int rc = tree_finish(c, who, &w);
    if (rc && rc != ESIM_ESIM) return rc;
    const size_t bytes = sizeof(uint32_t) * na;
    if (first_case && bytes) HIP_TRY(c, hipMemcpy(first_case, tab.p, bytes, hipMemcpyDeviceToHost));
    if (step && bytes) HIP_TRY(c, hipMemcpy(step, tab.p + na, bytes, hipMemcpyDeviceToHost));
    if (source_area && bytes) HIP_TRY(c, hipMemcpy(source_area, tab.p + 2 * na, bytes, hipMemcpyDeviceToHost));
    if (setting && na) HIP_TRY(c, hipMemcpy(setting, set.p, na, hipMemcpyDeviceToHost));
    return rc;
}

extern "C" int esim_lineage_areas(esim_ctx *ctx, uint32_t *lineage, uint32_t *area, uint32_t *count, uint32_t cap, uint32_t *n_out)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    const std::string who = "esim_lineage_areas";
    if (!n_out) return fail(c, ESIM_EINVAL, who + ": null n_out");
    if (int rc = tree_check(c, who)) return rc;
    HIP_TRY(c, hipSetDevice(c->P.device));
    ChainWork w;
    PairWork p;
    if (int rc = chains_enqueue(c, who, &w, CHAIN_UP, 0u, 0u)) return rc;
    const uint32_t log_len = w.t.s.log_len;
    if (int rc = pairs_begin(c, who, &p, log_len)) return flows_unwind(c, rc);
    hipLaunchKernelGGL(k_flow_lineages, dim3(grid_capped(c, log_len, TPB, 4096)), dim3(TPB), 0, c->stream, c->d, w.ch, log_len, p.t);
    if (int rc = pairs_sorted(c, &p)) return flows_unwind(c, rc);
    const int rc = chains_finish(c, who, &w);
    if (rc && rc != ESIM_ESIM) return rc;
    if (int full = pairs_end(c, who, &p)) return full;
    *n_out = p.n;
    if (p.n > cap) return fail(c, ESIM_ERANGE, who + ": buffers too small (n_out holds the size needed)");
    if (int bad = pairs_deliver(c, &p, lineage, area, count)) return bad;
    return rc;
}

extern "C" int esim_pair_stats(esim_ctx *ctx, double *ms, uint32_t *counts)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    const PairStats &s = c->pair_stats;
    if (ms) for (int k = 0; k < 3; ++k) ms[k] = s.ms[k];
    if (counts) { counts[0] = s.distinct; counts[1] = s.capacity; counts[2] = s.dropped; }
    return ESIM_OK;
}
