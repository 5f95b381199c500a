// esim_host_household.h -- household outbreaks: esim_household_outbreaks, esim_household_final_sizes (on top of settings_enqueue /
// settings_finish) and esim_household_sar (on top of tree_enqueue / tree_finish, through sar_begin / sar_finish, which
// esim_place_sar shares); the kernels: esim_kernels_household.h; DESIGN 19.
// All three work in temporary device memory that lives as long as the call, and leave the context as it is.
namespace {

struct HouseholdWork {
    SettingWork s;
    DevTmp<uint32_t> tab;             // cases, introductions, first_step [n_bld] each, then the two tables of HH_CELLS
    Place h;                          // (the households: no `members`, their sizes are res_off's)
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
    Place &h = w->h;
    h.n_places = d.n_bld; h.members = nullptr;
    h.cases = w->tab.p; h.intro = h.cases + nb; h.first = h.intro + nb; h.final_size = h.first + nb; h.intro_size = h.final_size + HH_CELLS;
    hipError_t e = hipMemsetAsync(h.cases, 0, sizeof(uint32_t) * std::max<size_t>(1, 2 * nb), c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(h.first, 0xFF, sizeof(uint32_t) * std::max<size_t>(1, nb), c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(h.final_size, 0, sizeof(uint32_t) * 2 * HH_CELLS, c->stream);
    if (e != hipSuccess) { (void)hipStreamSynchronize(c->stream); return fail(c, ESIM_ENODEVICE, who + ": " + hipGetErrorString(e)); }   // (the settings' kernels still read the host vectors of w->s)
    hipLaunchKernelGGL(k_list_members<LIST_HOME>, dim3(grid_capped(c, d.n, TPB, 4096)), dim3(TPB), 0, c->stream, d, w->s.q, h);
    // (a workgroup of k_list_tables bins 32 buildings per lane at least before it hands over its table of 8192 counters at most)
    if (tables) hipLaunchKernelGGL(k_list_tables<true>, dim3(grid_capped(c, nb, TPB * 32u, 1024, TPB)), dim3(TPB), 0, c->stream, d, h);
    return ESIM_OK;
}

// What esim_household_sar and esim_place_sar share (esim_host_places.h), around their own launches.
struct SarWork {
    SarWindow s;
    DevTmp<unsigned long long> tab;   // at_risk, then secondary: one block, as SarWindow asks for
    size_t cells, lds;                // counters of one table; bytes of both
    int mode;                         // PAIRTAB_*
    TreeWork w;
};

// The checks behind the call's own of its arguments, then the window, its two tables, the replay of the tree enqueued and the
// tables cleared behind it.
int sar_begin(esim_ctx_impl *c, const std::string &who, int where, uint32_t first_step, uint32_t last_step, SarWork *k)
{
    if (int rc = tree_check(c, who)) return rc;
    if (where == ESIM_BY_GROUP && !c->grp.lab) return fail(c, ESIM_ESTATE, who + ": by group without labels (esim_set_groups)");
    if (last_step < first_step || last_step > c->host_t - 1u)
        return fail(c, ESIM_ERANGE, who + ": last_step before first_step, or beyond the steps run so far");
    HIP_TRY(c, hipSetDevice(c->P.device));
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the pair counters are 64 bits wide");
    SarWindow &s = k->s;
    s.first = first_step; s.last = last_step;
    s.n_cols = where == ESIM_BY_ALL ? 1u : c->grp.n;
    s.grp = where == ESIM_BY_GROUP ? (const uint16_t *)c->grp.lab : nullptr;
    k->cells = (size_t)s.n_cols * s.n_cols;
    k->lds = 2 * k->cells * sizeof(unsigned long long);
    k->mode = pairtab_mode(where, k->lds);
    if (k->tab.alloc(2 * k->cells) != hipSuccess) { (void)hipGetLastError(); return fail(c, ESIM_ENOMEM, who + ": no device memory for the pair tables (16 B per cell)"); }
    s.at_risk = k->tab.p; s.secondary = k->tab.p + k->cells;
    if (int rc = tree_enqueue(c, who, &k->w, false)) return rc;
    HIP_TRY(c, hipMemsetAsync(k->tab.p, 0, sizeof(unsigned long long) * std::max<size_t>(1, 2 * k->cells), c->stream));
    return ESIM_OK;
}

// The replay finished and the tables copied back.
int sar_finish(esim_ctx_impl *c, const std::string &who, SarWork *k, uint64_t *at_risk, uint64_t *secondary)
{
    const int rc = tree_finish(c, who, &k->w);
    if (rc && rc != ESIM_ESIM) return rc;
    if (at_risk) HIP_TRY(c, hipMemcpy(at_risk, k->s.at_risk, sizeof(uint64_t) * k->cells, hipMemcpyDeviceToHost));
    if (secondary) HIP_TRY(c, hipMemcpy(secondary, k->s.secondary, sizeof(uint64_t) * k->cells, hipMemcpyDeviceToHost));
    return rc;
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
    SarWork k;
    if (int rc = sar_begin(c, who, where, first_step, last_step, &k)) return rc;
    const Setting &q = k.w.s.q;
    const uint32_t log_len = k.w.s.log_len;
    if (k.mode == PAIRTAB_ONE_CELL)
        hipLaunchKernelGGL(k_hh_sar<PAIRTAB_ONE_CELL>, dim3(grid_capped(c, log_len, TPB, 4096)), dim3(TPB), 0, c->stream, c->d, q, k.w.t, k.s, log_len);
    else if (k.mode == PAIRTAB_LDS)
        hipLaunchKernelGGL(k_hh_sar<PAIRTAB_LDS>, dim3(grid_capped(c, log_len, TPB * HH_SAR_PER_LANE, 4096, TPB)), dim3(TPB), k.lds, c->stream, c->d, q, k.w.t, k.s, log_len);
    else
        hipLaunchKernelGGL(k_hh_sar<PAIRTAB_GLOBAL>, dim3(grid_capped(c, log_len, TPB, 4096)), dim3(TPB), 0, c->stream, c->d, q, k.w.t, k.s, log_len);
    return sar_finish(c, who, &k, at_risk, secondary);
}
