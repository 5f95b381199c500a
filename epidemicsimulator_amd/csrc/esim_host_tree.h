// esim_host_tree.h -- who infected whom: esim_transmission_tree, esim_offspring, esim_reproduction_series, esim_mixing_matrix (the
// kernels: esim_kernels_tree.h), and the chains on top of the tree: esim_transmission_chains, esim_outbreaks,
// esim_transmission_ages (esim_kernels_chains.h).  All of them run on top of settings_enqueue / settings_finish: the setting of every
// logged exposure first, then its candidates and its infector, in temporary device memory that lives as long as the call.
namespace {

// What the four calls refuse alike, behind their own argument checks.
int tree_check(esim_ctx_impl *c, const std::string &who)
{
    if (int rc = settings_check(c, who)) return rc;
    if (c->draw_seam.two_capacities)
        return fail(c, ESIM_ESTATE, who + ": the run was branched from a snapshot under another bus_capacity; a bus replay under two capacities is not built");
    return ESIM_OK;
}

struct TreeWork {
    SettingWork s;
    DevTmp<uint32_t> infector, n_cand, gen, queue, counters, bus;
    Tree t;
};

// The settings, then the tree: infector and candidates per citizen (households in place, the rest through the queue and the wide
// kernel) and, where asked for, the generations, a launch per window of exposed_time + 1 steps; with `buses` the bus number of
// every transport exposure too (esim_transmission_events), 4 B per citizen more.
int tree_enqueue(esim_ctx_impl *c, const std::string &who, TreeWork *w, bool generations, bool buses = false)
{
    if (int rc = settings_enqueue(c, who, &w->s)) return rc;
    const Dev &d = c->d;
    const uint32_t log_len = w->s.log_len, t_done = w->s.q.t_done;
    if (w->infector.alloc(d.n) != hipSuccess || w->n_cand.alloc(d.n) != hipSuccess || w->gen.alloc(d.n) != hipSuccess || w->queue.alloc(log_len) != hipSuccess ||
        w->counters.alloc(3) != hipSuccess || (buses && w->bus.alloc(d.n) != hipSuccess)) {
        (void)hipGetLastError();
        (void)hipStreamSynchronize(c->stream);                         // (the settings' kernels still read the host vectors of w->s)
        return fail(c, ESIM_ENOMEM, who + ": no device memory for the tree (12 B per citizen and 4 B per entry of the exposure log)");
    }
    Tree &t = w->t;
    t.infector = w->infector.p; t.n_cand = w->n_cand.p; t.gen = w->gen.p; t.queue = w->queue.p; t.q_cap = log_len;
    t.n_queue = w->counters.p; t.n_long = w->counters.p + 1; t.orphans = w->counters.p + 2;
    t.bus = buses ? w->bus.p : nullptr;
    hipError_t e = hipMemsetAsync(w->counters.p, 0, 3 * sizeof(uint32_t), c->stream);
    if (e == hipSuccess && buses) e = hipMemsetAsync(w->bus.p, 0, sizeof(uint32_t) * std::max<size_t>(1, d.n), c->stream);
    if (e != hipSuccess) { (void)hipStreamSynchronize(c->stream); return fail(c, ESIM_ENODEVICE, who + ": " + hipGetErrorString(e)); }
    hipLaunchKernelGGL(k_tree_home, dim3(grid_capped(c, d.n, TPB, 4096)), dim3(TPB), 0, c->stream, d, w->s.q, t);
    hipLaunchKernelGGL(k_tree_wide, dim3(grid_capped(c, log_len, TPB / 64u, 4096)), dim3(TPB), 0, c->stream, d, w->s.q, t);
    if (d.max_route > d.bus_capacity) hipLaunchKernelGGL(k_tree_route, dim3(grid_capped(c, log_len, 1, 8192)), dim3(64), 0, c->stream, d, w->s.q, t);
    if (generations && t_done) {
        const uint32_t span = d.exposed_time + 1u, n_win = (t_done + span - 1u) / span;
        const uint32_t grid = grid_capped(c, (size_t)log_len / n_win * 2u + 1u, TPB, 1024);
        for (uint32_t lo = 1u; lo <= t_done; lo += span)
            hipLaunchKernelGGL(k_tree_gen, dim3(grid), dim3(TPB), 0, c->stream, d, w->s.q, t, lo, std::min(t_done, lo + span - 1u), log_len);
    }
    return ESIM_OK;
}

// The tail of the four calls: the wait and both audits -- ESIM_ESIM where an exposure has no draw that explains it, or nobody
// who can have caused it.
int tree_finish(esim_ctx_impl *c, const std::string &who, TreeWork *w)
{
    const int rc = settings_finish(c, who, &w->s);
    if (rc && rc != ESIM_ESIM) return rc;
    uint32_t orphans = 0;
    HIP_TRY(c, hipMemcpy(&orphans, w->t.orphans, sizeof orphans, hipMemcpyDeviceToHost));
    if (rc) return rc;
    if (orphans) return fail(c, ESIM_ESIM, who + ": " + std::to_string(orphans) + " exposures of the log have no candidate: nobody Infected stood where the exposure is credited in that step (they carry ESIM_NO_INFECTOR)");
    return ESIM_OK;
}

}  // namespace

extern "C" int esim_transmission_tree(esim_ctx *ctx, uint32_t *infector, uint32_t *n_candidates, uint32_t *generation)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    const std::string who = "esim_transmission_tree";
    if (int rc = tree_check(c, who)) return rc;
    HIP_TRY(c, hipSetDevice(c->P.device));
    TreeWork w;
    if (int rc = tree_enqueue(c, who, &w, generation != nullptr)) return rc;
    const int rc = tree_finish(c, who, &w);
    if (rc && rc != ESIM_ESIM) return rc;
    const size_t bytes = sizeof(uint32_t) * (size_t)c->d.n;
    if (infector && bytes) HIP_TRY(c, hipMemcpy(infector, w.t.infector, bytes, hipMemcpyDeviceToHost));
    if (n_candidates && bytes) HIP_TRY(c, hipMemcpy(n_candidates, w.t.n_cand, bytes, hipMemcpyDeviceToHost));
    if (generation && bytes) HIP_TRY(c, hipMemcpy(generation, w.t.gen, bytes, hipMemcpyDeviceToHost));
    return rc;
}

extern "C" int esim_offspring(esim_ctx *ctx, uint32_t first_step, uint32_t last_step, uint32_t *counts)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    const std::string who = "esim_offspring";
    if (!counts) return fail(c, ESIM_EINVAL, who + ": null output");
    if (int rc = tree_check(c, who)) return rc;
    if (first_step == 0 || last_step < first_step || last_step > c->host_t - 1u)
        return fail(c, ESIM_ERANGE, who + ": steps outside 1 .. the steps run so far, or last_step before first_step");
    HIP_TRY(c, hipSetDevice(c->P.device));
    const size_t n = c->d.n;
    DevTmp<uint32_t> tab;
    if (tab.alloc(n) != hipSuccess) { (void)hipGetLastError(); return fail(c, ESIM_ENOMEM, who + ": no device memory for the table"); }
    TreeWork w;
    if (int rc = tree_enqueue(c, who, &w, false)) return rc;
    HIP_TRY(c, hipMemsetAsync(tab.p, 0, sizeof(uint32_t) * std::max<size_t>(1, n), c->stream));
    hipLaunchKernelGGL(k_tree_offspring, dim3(grid_capped(c, w.s.log_len, TPB, 4096)), dim3(TPB), 0, c->stream, c->d, w.s.q, w.t, first_step, last_step, w.s.log_len, tab.p);
    const int rc = tree_finish(c, who, &w);
    if (rc && rc != ESIM_ESIM) return rc;
    if (n) HIP_TRY(c, hipMemcpy(counts, tab.p, sizeof(uint32_t) * n, hipMemcpyDeviceToHost));
    return rc;
}

extern "C" int esim_reproduction_series(esim_ctx *ctx, int where, uint32_t first_step, uint32_t n_rows, uint32_t stride, uint32_t *cases, uint32_t *offspring)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    const std::string who = "esim_reproduction_series";
    if ((!cases && !offspring) || (where != ESIM_BY_ALL && where != ESIM_AREA_HOME && where != ESIM_BY_GROUP) || stride == 0 || n_rows == 0)
        return fail(c, ESIM_EINVAL, who + ": no output, unknown `where` (a bus has no area: not ESIM_AREA_CURRENT), stride 0 or no rows");
    if (int rc = tree_check(c, who)) return rc;
    if (where == ESIM_BY_GROUP && !c->grp.lab) return fail(c, ESIM_ESTATE, who + ": by group without labels (esim_set_groups)");
    if ((uint64_t)first_step + (uint64_t)(n_rows - 1u) * stride > c->host_t - 1u)
        return fail(c, ESIM_ERANGE, who + ": rows outside the steps run so far");
    HIP_TRY(c, hipSetDevice(c->P.device));
    TreeRows r;
    r.where = (uint32_t)where; r.first = first_step; r.n_rows = n_rows; r.stride = stride;
    r.n_cols = where == ESIM_BY_ALL ? 1u : where == ESIM_BY_GROUP ? c->grp.n : c->d.n_areas;
    r.grp = where == ESIM_BY_GROUP ? c->grp.lab : nullptr;
    const size_t words = (size_t)n_rows * r.n_cols;
    DevTmp<uint32_t> rows;
    if (rows.alloc(2 * words) != hipSuccess) { (void)hipGetLastError(); return fail(c, ESIM_ENOMEM, who + ": no device memory for the rows (ask for fewer)"); }
    r.cases = cases ? rows.p : nullptr; r.offspring = offspring ? rows.p + words : nullptr;
    TreeWork w;
    if (int rc = tree_enqueue(c, who, &w, false)) return rc;
    HIP_TRY(c, hipMemsetAsync(rows.p, 0, sizeof(uint32_t) * std::max<size_t>(1, 2 * words), c->stream));
    hipLaunchKernelGGL(k_tree_rows, dim3(grid_capped(c, w.s.log_len, TPB, 4096)), dim3(TPB), 0, c->stream, c->d, w.s.q, w.t, r, w.s.log_len);
    const int rc = tree_finish(c, who, &w);
    if (rc && rc != ESIM_ESIM) return rc;
    if (cases && words) HIP_TRY(c, hipMemcpy(cases, rows.p, sizeof(uint32_t) * words, hipMemcpyDeviceToHost));
    if (offspring && words) HIP_TRY(c, hipMemcpy(offspring, rows.p + words, sizeof(uint32_t) * words, hipMemcpyDeviceToHost));
    return rc;
}

extern "C" int esim_mixing_matrix(esim_ctx *ctx, uint32_t setting_mask, uint32_t first_step, uint32_t last_step, uint32_t *counts)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    const std::string who = "esim_mixing_matrix";
    if (!counts || setting_mask == 0u || (setting_mask >> ESIM_N_SETTINGS) != 0u)
        return fail(c, ESIM_EINVAL, who + ": null output, or a setting mask that is empty or names a setting beyond ESIM_SETTING_TRANSPORT");
    if (int rc = tree_check(c, who)) return rc;
    if (!c->grp.lab) return fail(c, ESIM_ESTATE, who + ": no labels (esim_set_groups)");
    if (first_step == 0 || last_step < first_step || last_step > c->host_t - 1u)
        return fail(c, ESIM_ERANGE, who + ": steps outside 1 .. the steps run so far, or last_step before first_step");
    HIP_TRY(c, hipSetDevice(c->P.device));
    const size_t words = (size_t)c->grp.n * c->grp.n;
    DevTmp<uint32_t> tab;
    if (tab.alloc(words) != hipSuccess) { (void)hipGetLastError(); return fail(c, ESIM_ENOMEM, who + ": no device memory for the matrix"); }
    TreeWork w;
    if (int rc = tree_enqueue(c, who, &w, false)) return rc;
    HIP_TRY(c, hipMemsetAsync(tab.p, 0, sizeof(uint32_t) * std::max<size_t>(1, words), c->stream));
    hipLaunchKernelGGL(k_tree_matrix, dim3(grid_capped(c, w.s.log_len, TPB, 4096)), dim3(TPB), 0, c->stream, c->d, w.s.q, w.t, setting_mask, first_step, last_step,
                       (const uint16_t *)c->grp.lab, c->grp.n, w.s.log_len, tab.p);
    const int rc = tree_finish(c, who, &w);
    if (rc && rc != ESIM_ESIM) return rc;
    if (words) HIP_TRY(c, hipMemcpy(counts, tab.p, sizeof(uint32_t) * words, hipMemcpyDeviceToHost));
    return rc;
}

namespace {

enum : unsigned { CHAIN_UP = 1u, CHAIN_DOWN = 2u, CHAIN_TABLE = 4u, CHAIN_AGE = 8u };   // the passes a call needs

struct ChainWork {
    TreeWork t;
    DevTmp<uint32_t> lineage, desc, tab;   // tab: size, depth, last_step [n_seeds] each, the age table, the two audit counters
    Chain ch;
};

// The tree (with the generations where the per-seed table is asked for), then the passes in `what`: the index cases numbered
// and the lineage handed forward, the descendants summed backward -- a launch per window of exposed_time + 1 steps each, as the
// generations take --, the per-seed table, the ages of steps [first, last].  The allocations live as long as *w.
int chains_enqueue(esim_ctx_impl *c, const std::string &who, ChainWork *w, unsigned what, uint32_t first, uint32_t last)
{
    const Dev &d = c->d;
    const size_t n = d.n, n_seeds = c->init_log.size(), words = 3 * n_seeds + CHAIN_AGES + 2u;
    const bool up = (what & CHAIN_UP) != 0u, down = (what & CHAIN_DOWN) != 0u;
    if ((up && w->lineage.alloc(n) != hipSuccess) || (down && w->desc.alloc(n) != hipSuccess) || w->tab.alloc(words) != hipSuccess) {
        (void)hipGetLastError();
        return fail(c, ESIM_ENOMEM, who + ": no device memory for the chains (4 B per citizen each for the lineage and the descendants, 12 B per seed, 8 KB for the ages)");
    }
    if (int rc = tree_enqueue(c, who, &w->t, (what & CHAIN_TABLE) != 0u)) return rc;
    const uint32_t log_len = w->t.s.log_len, t_done = w->t.s.q.t_done;
    Chain &ch = w->ch;
    ch.lineage = w->lineage.p; ch.desc = w->desc.p;
    ch.size = w->tab.p; ch.depth = ch.size + n_seeds; ch.last = ch.depth + n_seeds; ch.ages = ch.last + n_seeds;
    ch.bad_age = ch.ages + CHAIN_AGES; ch.unrooted = ch.bad_age + 1;
    ch.n_seeds = (uint32_t)std::min<size_t>(n_seeds, log_len);
    hipError_t e = hipMemsetAsync(w->tab.p, 0, sizeof(uint32_t) * words, c->stream);
    if (e == hipSuccess && up) e = hipMemsetAsync(ch.lineage, 0xFF, sizeof(uint32_t) * std::max<size_t>(1, n), c->stream);
    if (e == hipSuccess && down) e = hipMemsetAsync(ch.desc, 0, sizeof(uint32_t) * std::max<size_t>(1, n), c->stream);
    if (e != hipSuccess) { (void)hipStreamSynchronize(c->stream); return fail(c, ESIM_ENODEVICE, who + ": " + hipGetErrorString(e)); }
    if (up) hipLaunchKernelGGL(k_chain_roots, dim3(grid_for(ch.n_seeds, TPB, 0xFFFFFFFFu)), dim3(TPB), 0, c->stream, d, ch);
    if ((up || down) && t_done) {
        const uint32_t span = d.exposed_time + 1u, n_win = (t_done + span - 1u) / span;
        const uint32_t grid = grid_capped(c, (size_t)log_len / n_win * 2u + 1u, TPB, 1024);
        if (up)
            for (uint32_t lo = 1u; lo <= t_done; lo += span)
                hipLaunchKernelGGL(k_chain_up, dim3(grid), dim3(TPB), 0, c->stream, d, w->t.s.q, w->t.t, ch, lo, std::min(t_done, lo + span - 1u), log_len);
        if (down)
            for (uint32_t k = n_win; k-- > 0u;) {
                const uint32_t lo = 1u + k * span;
                hipLaunchKernelGGL(k_chain_down, dim3(grid), dim3(TPB), 0, c->stream, d, w->t.s.q, w->t.t, ch, lo, std::min(t_done, lo + span - 1u), log_len);
            }
    }
    if (what & CHAIN_TABLE) hipLaunchKernelGGL(k_chain_outbreaks, dim3(grid_capped(c, log_len, TPB, 4096)), dim3(TPB), 0, c->stream, d, w->t.s.q, w->t.t, ch, log_len);
    // (a workgroup of k_chain_ages walks 32 entries per lane at least before it hands over its table of 2048 counters at most)
    if (what & CHAIN_AGE) hipLaunchKernelGGL(k_chain_ages, dim3(grid_capped(c, log_len, TPB * 32u, 1024, TPB)), dim3(TPB), 0, c->stream, d, w->t.s.q, w->t.t, ch, first, last, log_len);
    return ESIM_OK;
}

// The tail of the three calls: the tree's wait and audits, then the two of the chains -- ESIM_ESIM where a chain does not end at
// an index case, or a transmission has an infectious age that no Infected citizen has.
int chains_finish(esim_ctx_impl *c, const std::string &who, ChainWork *w)
{
    const int rc = tree_finish(c, who, &w->t);
    if (rc) return rc;
    uint32_t bad[2] = { 0u, 0u };
    HIP_TRY(c, hipMemcpy(bad, w->ch.bad_age, sizeof bad, hipMemcpyDeviceToHost));
    if (bad[1]) return fail(c, ESIM_ESIM, who + ": " + std::to_string(bad[1]) + " exposures of the log lie on a chain that does not end at an index case (they carry ESIM_NO_LINEAGE)");
    if (bad[0]) return fail(c, ESIM_ESIM, who + ": " + std::to_string(bad[0]) + " transmissions have an infectious age outside 0 .. infected_time: the infector was not Infected in that step (they are not counted)");
    return ESIM_OK;
}

}  // namespace

extern "C" int esim_transmission_chains(esim_ctx *ctx, uint32_t *lineage, uint32_t *descendants)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    const std::string who = "esim_transmission_chains";
    if (int rc = tree_check(c, who)) return rc;
    HIP_TRY(c, hipSetDevice(c->P.device));
    ChainWork w;
    if (int rc = chains_enqueue(c, who, &w, CHAIN_UP | (descendants ? CHAIN_DOWN : 0u), 0u, 0u)) return rc;   // (the lineage pass carries an audit)
    const int rc = chains_finish(c, who, &w);
    if (rc && rc != ESIM_ESIM) return rc;
    const size_t bytes = sizeof(uint32_t) * (size_t)c->d.n;
    if (lineage && bytes) HIP_TRY(c, hipMemcpy(lineage, w.ch.lineage, bytes, hipMemcpyDeviceToHost));
    if (descendants && bytes) HIP_TRY(c, hipMemcpy(descendants, w.ch.desc, bytes, hipMemcpyDeviceToHost));
    return rc;
}

extern "C" int esim_outbreaks(esim_ctx *ctx, uint32_t *size, uint32_t *depth, uint32_t *last_step, uint32_t cap, uint32_t *n_out)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    const std::string who = "esim_outbreaks";
    if (!n_out) return fail(c, ESIM_EINVAL, who + ": null n_out");
    if (int rc = tree_check(c, who)) return rc;
    const uint32_t n_seeds = (uint32_t)c->init_log.size();
    *n_out = n_seeds;
    if (n_seeds > cap) return fail(c, ESIM_ERANGE, who + ": buffers too small (n_out holds the size needed)");
    HIP_TRY(c, hipSetDevice(c->P.device));
    ChainWork w;
    if (int rc = chains_enqueue(c, who, &w, CHAIN_UP | CHAIN_DOWN | CHAIN_TABLE, 0u, 0u)) return rc;
    const int rc = chains_finish(c, who, &w);
    if (rc && rc != ESIM_ESIM) return rc;
    const size_t bytes = sizeof(uint32_t) * (size_t)n_seeds;
    if (size && bytes) HIP_TRY(c, hipMemcpy(size, w.ch.size, bytes, hipMemcpyDeviceToHost));
    if (depth && bytes) HIP_TRY(c, hipMemcpy(depth, w.ch.depth, bytes, hipMemcpyDeviceToHost));
    if (last_step && bytes) HIP_TRY(c, hipMemcpy(last_step, w.ch.last, bytes, hipMemcpyDeviceToHost));
    return rc;
}

extern "C" int esim_transmission_ages(esim_ctx *ctx, uint32_t first_step, uint32_t last_step, uint32_t *counts)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    const std::string who = "esim_transmission_ages";
    if (!counts) return fail(c, ESIM_EINVAL, who + ": null output");
    if (int rc = tree_check(c, who)) return rc;
    if (first_step == 0 || last_step < first_step || last_step > c->host_t - 1u)
        return fail(c, ESIM_ERANGE, who + ": steps outside 1 .. the steps run so far, or last_step before first_step");
    HIP_TRY(c, hipSetDevice(c->P.device));
    ChainWork w;
    if (int rc = chains_enqueue(c, who, &w, CHAIN_AGE, first_step, last_step)) return rc;
    const int rc = chains_finish(c, who, &w);
    if (rc && rc != ESIM_ESIM) return rc;
    HIP_TRY(c, hipMemcpy(counts, w.ch.ages, sizeof(uint32_t) * CHAIN_AGES, hipMemcpyDeviceToHost));
    return rc;
}
