// esim_host_ensrows.h -- ensemble accumulators over the transmission rows: esim_ensemble_begin_settings (the rows of
// esim_setting_series, folded by k_ensemble_fold_rows and read by esim_ensemble_read_series), esim_ensemble_begin_reproduction
// and esim_ensemble_read_reproduction (the cohort rows of esim_reproduction_series, folded by k_ensemble_fold_ratio), and what
// esim_ensemble_fold does with one of them in force.  The begin and the read-out are those of every kind
// (esim_host_ensemble.h); the replays are those of esim_host_settings.h and esim_host_tree.h, unchanged.
namespace {

// What both begins refuse alike behind their own argument checks: the state errors of esim_ensemble_begin_series.
int ensrows_begin_check(esim_ctx_impl *c, const std::string &who, int where)
{
    if (!c->uploaded) return fail(c, ESIM_ESTATE, who + ": no population uploaded");
    if (c->comm.world > 1) return fail(c, ESIM_ESTATE, who + ": the context has a communicator of several ranks (the rule of esim_restart)");
    if (where == ESIM_BY_GROUP && !c->grp.lab) return fail(c, ESIM_ESTATE, who + ": by group without labels (esim_set_groups)");
    return ESIM_OK;
}

// One member folded into the accumulators of the settings or the reproduction kind: the checks of the series call the kind
// stands for, the kept plane(s) zeroed, the replay, the rows kernel into the planes, the fold kernel, and the replay's wait and
// audits.  An audit's ESIM_ESIM comes back with the member folded, as every call on top of the replay delivers its output.
int fold_transmission(esim_ctx_impl *c)
{
    Rows &r = c->ens.rows;
    const Ensemble::Par &par = c->ens.par;
    const std::string who = "esim_ensemble_fold";
    const bool ratio = c->ens.kind == Ensemble::ENS_REPRODUCTION, by_group = c->ens.where == ESIM_BY_GROUP;
    if (int rc = ratio ? tree_check(c, who) : settings_check(c, who)) return rc;
    if (by_group && (!c->grp.lab || c->grp.n != r.n_cols)) return fail(c, ESIM_ESTATE, who + ": the accumulators were begun for other columns");
    if ((uint64_t)par.first + (uint64_t)(r.n_rows - 1u) * par.stride > c->host_t - 1u)
        return fail(c, ESIM_ERANGE, who + ": rows outside the steps run so far");
    HIP_TRY(c, hipSetDevice(c->P.device));
    const uint64_t cells = (uint64_t)r.n_rows * r.n_cols;
    const uint32_t fold_grid = grid_capped(c, (size_t)(cells >> 2), TPB, 2048);
    HIP_TRY(c, hipMemsetAsync(r.p0, 0, sizeof(uint32_t) * std::max<size_t>(1, (size_t)cells), c->stream));
    if (!ratio) {
        SettingRows q;
        q.where = (uint32_t)c->ens.where; q.mask = par.setting_mask; q.first = par.first; q.n_rows = r.n_rows; q.stride = par.stride; q.n_cols = r.n_cols;
        q.grp = by_group ? c->grp.lab : nullptr; q.rows = r.p0;
        SettingWork w;
        if (int rc = settings_enqueue(c, who, &w)) return rc;
        hipLaunchKernelGGL(k_setting_rows, dim3(grid_capped(c, w.log_len, TPB, 4096)), dim3(TPB), 0, c->stream, c->d, w.q, q, w.log_len);
        hipLaunchKernelGGL(k_ensemble_fold_rows, dim3(fold_grid), dim3(TPB), 0, c->stream, r.p0, cells, par.min_hit, r.hit, r.sum, r.sumsq, r.members);
        const hipError_t kept = members_keep(c);
        const int rc = settings_finish(c, who, &w);
        return kept != hipSuccess ? fail(c, ESIM_ENODEVICE, who + ": " + hipGetErrorString(kept)) : rc;
    }
    HIP_TRY(c, hipMemsetAsync(r.p1, 0, sizeof(uint32_t) * std::max<size_t>(1, (size_t)cells), c->stream));
    TreeRows q;
    q.where = (uint32_t)c->ens.where; q.first = par.first; q.n_rows = r.n_rows; q.stride = par.stride; q.n_cols = r.n_cols;
    q.grp = by_group ? c->grp.lab : nullptr; q.cases = r.p0; q.offspring = r.p1;
    TreeWork w;
    if (int rc = tree_enqueue(c, who, &w, false)) return rc;
    hipLaunchKernelGGL(k_tree_rows, dim3(grid_capped(c, w.s.log_len, TPB, 4096)), dim3(TPB), 0, c->stream, c->d, w.s.q, w.t, q, w.s.log_len);
    hipLaunchKernelGGL(k_ensemble_fold_ratio, dim3(fold_grid), dim3(TPB), 0, c->stream, r.p0, r.p1, cells, par.min_defined, par.r_num, par.r_den, ratio_acc(r));
    return tree_finish(c, who, &w);
}

}  // namespace

extern "C" int esim_ensemble_begin_settings(esim_ctx *ctx, int where, uint32_t setting_mask, uint32_t first_step, uint32_t n_rows, uint32_t stride, uint32_t min_cases)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    const std::string who = "esim_ensemble_begin_settings";
    if ((where != ESIM_BY_SETTING && where != ESIM_AREA_HOME && where != ESIM_BY_GROUP) || setting_mask == 0u || (setting_mask >> ESIM_N_SETTINGS) != 0u || stride == 0 || n_rows == 0)
        return fail(c, ESIM_EINVAL, who + ": unknown `where` (a bus has no area: not ESIM_AREA_CURRENT), a setting mask that is empty or names a setting beyond ESIM_SETTING_TRANSPORT, stride 0 or no rows");
    if (int rc = ensrows_begin_check(c, who, where)) return rc;
    if (first_step == 0) return fail(c, ESIM_ERANGE, who + ": first_step is 1-based");
    HIP_TRY(c, hipSetDevice(c->P.device));
    const uint32_t cols = where == ESIM_BY_SETTING ? (uint32_t)ESIM_N_SETTINGS : where == ESIM_BY_GROUP ? c->grp.n : c->d.n_areas;
    Ensemble::Par par;
    par.setting_mask = setting_mask; par.first = first_step; par.stride = stride; par.min_hit = min_cases;
    return ens_begin(c, who, Ensemble::ENS_SETTINGS, where, n_rows, cols, par);
}

extern "C" int esim_ensemble_begin_reproduction(esim_ctx *ctx, int where, uint32_t first_step, uint32_t n_rows, uint32_t stride, uint32_t min_cohort, uint32_t r_num, uint32_t r_den)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    const std::string who = "esim_ensemble_begin_reproduction";
    if ((where != ESIM_BY_ALL && where != ESIM_AREA_HOME && where != ESIM_BY_GROUP) || stride == 0 || n_rows == 0 || min_cohort == 0 || r_den == 0)
        return fail(c, ESIM_EINVAL, who + ": unknown `where` (a bus has no area: not ESIM_AREA_CURRENT), stride 0, no rows, min_cohort 0 or r_den 0");
    if (int rc = ensrows_begin_check(c, who, where)) return rc;
    HIP_TRY(c, hipSetDevice(c->P.device));
    const uint32_t cols = where == ESIM_BY_ALL ? 1u : where == ESIM_BY_GROUP ? c->grp.n : c->d.n_areas;
    Ensemble::Par par;
    par.first = first_step; par.stride = stride; par.min_defined = min_cohort; par.r_num = r_num; par.r_den = r_den;
    return ens_begin(c, who, Ensemble::ENS_REPRODUCTION, where, n_rows, cols, par);
}

extern "C" int esim_ensemble_read_reproduction(esim_ctx *ctx, uint32_t first_row, uint32_t n, uint32_t *members, uint32_t *defined, uint32_t *hit,
                                               uint64_t *sum_cases, uint64_t *sum_offspring, uint64_t *sumsq_cases, uint64_t *sumsq_offspring, uint64_t *sum_cross)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    return ens_read(c, READ_REPRODUCTION, first_row, n, members, { { defined, &Rows::defined }, { hit, &Rows::hit } },
                    { { sum_cases, &Rows::sum }, { sum_offspring, &Rows::sum_o }, { sumsq_cases, &Rows::sumsq }, { sumsq_offspring, &Rows::sumsq_o }, { sum_cross, &Rows::cross } });
}
