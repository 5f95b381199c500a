// esim_host_household.h -- household outbreaks: esim_household_outbreaks, esim_household_final_sizes (on top of settings_enqueue /
// settings_finish) and esim_household_sar (on top of tree_enqueue / tree_finish); the kernels: esim_kernels_household.h; DESIGN 19.
// All three work in temporary device memory that lives as long as the call, and leave the context as it is.
namespace {

struct HouseholdWork {
    SettingWork s;
    DevTmp<uint32_t> tab;             // cases, introductions, first_step [n_bld] each, then the two tables of HH_CELLS
    Household h;
};

// The settings, then the per-household pass and, where asked for, the two tables.
int household_enqueue(esim_ctx_impl *c, const std::string &who, HouseholdWork *w, bool tables)
{
    const Dev &d = c->d;
    const size_t nb = d.n_bld, words = 3 * nb + 2 * (size_t)HH_CELLS;
    if (w->tab.alloc(words) != hipSuccess) {
        (void)hipGetLastError();
        return fail(c, ESIM_ENOMEM, who + ": no device memory for the households (12 B per building and 32 KB for the two tables)");
    }
    if (int rc = settings_enqueue(c, who, &w->s)) return rc;
    Household &h = w->h;
    h.cases = w->tab.p; h.intro = h.cases + nb; h.first = h.intro + nb; h.final_size = h.first + nb; h.intro_size = h.final_size + HH_CELLS;
    hipError_t e = hipMemsetAsync(h.cases, 0, sizeof(uint32_t) * std::max<size_t>(1, 2 * nb), c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(h.first, 0xFF, sizeof(uint32_t) * std::max<size_t>(1, nb), c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(h.final_size, 0, sizeof(uint32_t) * 2 * HH_CELLS, c->stream);
    if (e != hipSuccess) { (void)hipStreamSynchronize(c->stream); return fail(c, ESIM_ENODEVICE, who + ": " + hipGetErrorString(e)); }   // (the settings' kernels still read the host vectors of w->s)
    hipLaunchKernelGGL(k_hh_residents, dim3(grid_capped(c, d.n, TPB, 4096)), dim3(TPB), 0, c->stream, d, w->s.q, h);
    // (a workgroup of k_hh_tables bins 32 buildings per lane at least before it hands over its table of 8192 counters at most)
    if (tables) hipLaunchKernelGGL(k_hh_tables, dim3(grid_capped(c, nb, TPB * 32u, 1024, TPB)), dim3(TPB), 0, c->stream, d, h);
    return ESIM_OK;
}

}  // namespace

extern "C" int esim_household_outbreaks(esim_ctx *ctx, uint32_t *cases, uint32_t *introductions, uint32_t *first_step)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    const std::string who = "esim_household_outbreaks";
    if (int rc = settings_check(c, who)) return rc;
    HIP_TRY(c, hipSetDevice(c->P.device));
    HouseholdWork w;
    if (int rc = household_enqueue(c, who, &w, false)) return rc;
    const int rc = settings_finish(c, who, &w.s);
    if (rc && rc != ESIM_ESIM) return rc;
    const size_t bytes = sizeof(uint32_t) * (size_t)c->d.n_bld;
    if (cases && bytes) HIP_TRY(c, hipMemcpy(cases, w.h.cases, bytes, hipMemcpyDeviceToHost));
    if (introductions && bytes) HIP_TRY(c, hipMemcpy(introductions, w.h.intro, bytes, hipMemcpyDeviceToHost));
    if (first_step && bytes) HIP_TRY(c, hipMemcpy(first_step, w.h.first, bytes, hipMemcpyDeviceToHost));
    return rc;
}

extern "C" int esim_household_final_sizes(esim_ctx *ctx, uint32_t *final_size, uint32_t *introductions)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    const std::string who = "esim_household_final_sizes";
    if (int rc = settings_check(c, who)) return rc;
    HIP_TRY(c, hipSetDevice(c->P.device));
    HouseholdWork w;
    if (int rc = household_enqueue(c, who, &w, true)) return rc;
    const int rc = settings_finish(c, who, &w.s);
    if (rc && rc != ESIM_ESIM) return rc;
    if (final_size) HIP_TRY(c, hipMemcpy(final_size, w.h.final_size, sizeof(uint32_t) * HH_CELLS, hipMemcpyDeviceToHost));
    if (introductions) HIP_TRY(c, hipMemcpy(introductions, w.h.intro_size, sizeof(uint32_t) * HH_CELLS, hipMemcpyDeviceToHost));
    return rc;
}

extern "C" int esim_household_sar(esim_ctx *ctx, int where, uint32_t first_step, uint32_t last_step, uint64_t *at_risk, uint64_t *secondary)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    const std::string who = "esim_household_sar";
    if ((!at_risk && !secondary) || (where != ESIM_BY_ALL && where != ESIM_BY_GROUP))
        return fail(c, ESIM_EINVAL, who + ": no output, or a `where` that is neither ESIM_BY_ALL nor ESIM_BY_GROUP");
    if (int rc = tree_check(c, who)) return rc;
    if (where == ESIM_BY_GROUP && !c->grp.lab) return fail(c, ESIM_ESTATE, who + ": by group without labels (esim_set_groups)");
    if (last_step < first_step || last_step > c->host_t - 1u)
        return fail(c, ESIM_ERANGE, who + ": last_step before first_step, or beyond the steps run so far");
    HIP_TRY(c, hipSetDevice(c->P.device));
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the pair counters are 64 bits wide");
    HouseholdSar s;
    s.first = first_step; s.last = last_step;
    s.n_cols = where == ESIM_BY_ALL ? 1u : c->grp.n;
    s.grp = where == ESIM_BY_GROUP ? (const uint16_t *)c->grp.lab : nullptr;
    const size_t cells = (size_t)s.n_cols * s.n_cols, lds = 2 * cells * sizeof(unsigned long long);
    DevTmp<unsigned long long> tab;
    if (tab.alloc(2 * cells) != hipSuccess) { (void)hipGetLastError(); return fail(c, ESIM_ENOMEM, who + ": no device memory for the pair tables (16 B per cell)"); }
    s.at_risk = tab.p; s.secondary = tab.p + cells;
    TreeWork w;
    if (int rc = tree_enqueue(c, who, &w, false)) return rc;
    HIP_TRY(c, hipMemsetAsync(tab.p, 0, sizeof(unsigned long long) * std::max<size_t>(1, 2 * cells), c->stream));
    const uint32_t log_len = w.s.log_len;
    if (where == ESIM_BY_ALL)
        hipLaunchKernelGGL(k_hh_sar<HH_ONE_CELL>, dim3(grid_capped(c, log_len, TPB, 4096)), dim3(TPB), 0, c->stream, c->d, w.s.q, w.t, s, log_len);
    else if (lds <= HH_LDS_BYTES)
        hipLaunchKernelGGL(k_hh_sar<HH_LDS>, dim3(grid_capped(c, log_len, TPB * HH_SAR_PER_LANE, 4096, TPB)), dim3(TPB), lds, c->stream, c->d, w.s.q, w.t, s, log_len);
    else
        hipLaunchKernelGGL(k_hh_sar<HH_GLOBAL>, dim3(grid_capped(c, log_len, TPB, 4096)), dim3(TPB), 0, c->stream, c->d, w.s.q, w.t, s, log_len);
    const int rc = tree_finish(c, who, &w);
    if (rc && rc != ESIM_ESIM) return rc;
    if (at_risk) HIP_TRY(c, hipMemcpy(at_risk, s.at_risk, sizeof(uint64_t) * cells, hipMemcpyDeviceToHost));
    if (secondary) HIP_TRY(c, hipMemcpy(secondary, s.secondary, sizeof(uint64_t) * cells, hipMemcpyDeviceToHost));
    return rc;
}
