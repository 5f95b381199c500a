// esim_host_ensrows.h -- ensemble accumulators over the transmission rows: esim_ensemble_begin_settings (the rows of
// esim_setting_series, folded by k_ensemble_fold_rows and read by esim_ensemble_read_series), esim_ensemble_begin_reproduction
// and esim_ensemble_read_reproduction (the cohort rows of esim_reproduction_series, folded by k_ensemble_fold_ratio), and what
// esim_ensemble_fold does with one of them in force.  Two more kinds of Ensemble::Rows, beside the series kind of
// esim_host_outputs.h; the replays are those of esim_host_settings.h and esim_host_tree.h, unchanged.  The paired kind of
// esim_host_compare.h shares the allocation (ensrows_begin) and the read-out (read_two_planes) of the reproduction kind.
namespace {

// What both begins refuse alike behind their own argument checks: the state errors of esim_ensemble_begin_series.
int ensrows_begin_check(esim_ctx_impl *c, const std::string &who, int where)
{
    if (!c->uploaded) return fail(c, ESIM_ESTATE, who + ": no population uploaded");
    if (c->comm.world > 1) return fail(c, ESIM_ESTATE, who + ": the context has a communicator of several ranks (the rule of esim_restart)");
    if (where == ESIM_BY_GROUP && !c->grp.lab) return fail(c, ESIM_ESTATE, who + ": by group without labels (esim_set_groups)");
    return ESIM_OK;
}

// The accumulators and the kept plane(s) of one of the two kinds in the shape asked for, zeroed on the stream.  The kind and
// shape in force are kept; any other is allocated before the earlier one goes, so that a refusal leaves everything as it was.
int ensrows_begin(esim_ctx_impl *c, const std::string &who, int kind, uint32_t n_rows, uint32_t cols)
{
    const bool ratio = kind == Ensemble::ROWS_REPRODUCTION || kind == Ensemble::ROWS_PAIRED;   // (two planes, two counters, five sums)
    const size_t cells = (size_t)n_rows * cols;
    Ensemble::Rows &old = c->ens.rows;
    if (!old.hit || old.kind != kind || old.n_rows != n_rows || old.n_cols != cols) {
        Ensemble::Rows r;
        int rc;
        if ((rc = dev_alloc(c, &r.hit, cells)) || (rc = dev_alloc(c, &r.sum, cells)) || (rc = dev_alloc(c, &r.sumsq, cells)) || (rc = dev_alloc(c, &r.members, 1)) ||
            (rc = dev_alloc(c, &r.p0, cells)) ||
            (ratio && ((rc = dev_alloc(c, &r.p1, cells)) || (rc = dev_alloc(c, &r.defined, cells)) || (rc = dev_alloc(c, &r.sum_o, cells)) ||
                       (rc = dev_alloc(c, &r.sumsq_o, cells)) || (rc = dev_alloc(c, &r.cross, cells))))) {
            (void)hipGetLastError();
            rows_free(c, &r);
            return fail(c, ESIM_ENOMEM, who + ": no device memory for the accumulators and the row planes (ask for fewer rows)");
        }
        if (old.hit) HIP_TRY(c, hipStreamSynchronize(c->stream));    // (a fold on the stream may still be using the old ones)
        r.vax = old.vax; old.vax = nullptr;                          // (the series kind's 4 B per citizen, whatever the shape)
        rows_free(c, &old);
        old = r;
    }
    Ensemble::Rows &r = c->ens.rows;
    r.kind = kind; r.n_rows = n_rows; r.n_cols = cols; r.two = ratio;
    r.burden = false;                                              // (a Rows reused: the burden kinds of esim_host_beds.h set it behind this call)
    HIP_TRY(c, hipMemsetAsync(r.hit, 0, sizeof(uint32_t) * cells, c->stream));
    HIP_TRY(c, hipMemsetAsync(r.sum, 0, sizeof(unsigned long long) * cells, c->stream));
    HIP_TRY(c, hipMemsetAsync(r.sumsq, 0, sizeof(unsigned long long) * cells, c->stream));
    HIP_TRY(c, hipMemsetAsync(r.members, 0, sizeof(uint32_t), c->stream));
    if (ratio) {
        HIP_TRY(c, hipMemsetAsync(r.defined, 0, sizeof(uint32_t) * cells, c->stream));
        HIP_TRY(c, hipMemsetAsync(r.sum_o, 0, sizeof(unsigned long long) * cells, c->stream));
        HIP_TRY(c, hipMemsetAsync(r.sumsq_o, 0, sizeof(unsigned long long) * cells, c->stream));
        HIP_TRY(c, hipMemsetAsync(r.cross, 0, sizeof(unsigned long long) * cells, c->stream));
    }
    return ESIM_OK;
}

// One member folded into the accumulators of the settings or the reproduction kind: the checks of the series call the kind
// stands for, the kept plane(s) zeroed, the replay, the rows kernel into the planes, the fold kernel, and the replay's wait and
// audits.  An audit's ESIM_ESIM comes back with the member folded, as every call on top of the replay delivers its output.
int fold_transmission(esim_ctx_impl *c)
{
    Ensemble::Rows &r = c->ens.rows;
    const std::string who = "esim_ensemble_fold";
    const bool ratio = r.kind == Ensemble::ROWS_REPRODUCTION, by_group = c->ens.where == ESIM_BY_GROUP;
    if (int rc = ratio ? tree_check(c, who) : settings_check(c, who)) return rc;
    if (by_group && (!c->grp.lab || c->grp.n != r.n_cols)) return fail(c, ESIM_ESTATE, who + ": the accumulators were begun for other columns");
    if ((uint64_t)r.first + (uint64_t)(r.n_rows - 1u) * r.stride > c->host_t - 1u)
        return fail(c, ESIM_ERANGE, who + ": rows outside the steps run so far");
    HIP_TRY(c, hipSetDevice(c->P.device));
    const uint64_t cells = (uint64_t)r.n_rows * r.n_cols;
    const uint32_t fold_grid = grid_capped(c, (size_t)(cells >> 2), TPB, 2048);
    HIP_TRY(c, hipMemsetAsync(r.p0, 0, sizeof(uint32_t) * std::max<size_t>(1, (size_t)cells), c->stream));
    if (!ratio) {
        SettingRows q;
        q.where = (uint32_t)c->ens.where; q.mask = r.mask; q.first = r.first; q.n_rows = r.n_rows; q.stride = r.stride; q.n_cols = r.n_cols;
        q.grp = by_group ? c->grp.lab : nullptr; q.rows = r.p0;
        SettingWork w;
        if (int rc = settings_enqueue(c, who, &w)) return rc;
        hipLaunchKernelGGL(k_setting_rows, dim3(grid_capped(c, w.log_len, TPB, 4096)), dim3(TPB), 0, c->stream, c->d, w.q, q, w.log_len);
        hipLaunchKernelGGL(k_ensemble_fold_rows, dim3(fold_grid), dim3(TPB), 0, c->stream, r.p0, cells, r.min, r.hit, r.sum, r.sumsq, r.members);
        const hipError_t kept = members_keep(c);
        const int rc = settings_finish(c, who, &w);
        return kept != hipSuccess ? fail(c, ESIM_ENODEVICE, who + ": " + hipGetErrorString(kept)) : rc;
    }
    HIP_TRY(c, hipMemsetAsync(r.p1, 0, sizeof(uint32_t) * std::max<size_t>(1, (size_t)cells), c->stream));
    TreeRows q;
    q.where = (uint32_t)c->ens.where; q.first = r.first; q.n_rows = r.n_rows; q.stride = r.stride; q.n_cols = r.n_cols;
    q.grp = by_group ? c->grp.lab : nullptr; q.cases = r.p0; q.offspring = r.p1;
    RatioAcc a;
    a.defined = r.defined; a.hit = r.hit; a.members = r.members; a.sum_c = r.sum; a.sum_o = r.sum_o; a.sq_c = r.sumsq; a.sq_o = r.sumsq_o; a.cross = r.cross;
    TreeWork w;
    if (int rc = tree_enqueue(c, who, &w, false)) return rc;
    hipLaunchKernelGGL(k_tree_rows, dim3(grid_capped(c, w.s.log_len, TPB, 4096)), dim3(TPB), 0, c->stream, c->d, w.s.q, w.t, q, w.s.log_len);
    hipLaunchKernelGGL(k_ensemble_fold_ratio, dim3(fold_grid), dim3(TPB), 0, c->stream, r.p0, r.p1, cells, r.min, r.r_num, r.r_den, a);
    return tree_finish(c, who, &w);
}

// The read-out of the two kinds with two planes (reproduction, paired): rows [first_row, first_row + n) of the two counters and
// the five sums, any pointer NULL.
int read_two_planes(esim_ctx_impl *c, const std::string &who, int kind, uint32_t first_row, uint32_t n, uint32_t *members, uint32_t *defined, uint32_t *hit,
                    uint64_t *sum_0, uint64_t *sum_1, uint64_t *sumsq_0, uint64_t *sumsq_1, uint64_t *sum_cross)
{
    if (!c->uploaded || !c->ens.valid || !c->ens.series || !c->ens.rows.hit || c->ens.rows.kind != kind)
        return fail(c, ESIM_ESTATE, who + ": no population uploaded, or no begin of this kind in force since the upload (or, by group, since esim_set_groups)");
    const Ensemble::Rows &r = c->ens.rows;
    if ((uint64_t)first_row + n > r.n_rows) return fail(c, ESIM_ERANGE, who + ": rows outside the accumulators");
    HIP_TRY(c, hipSetDevice(c->P.device));
    Ctrl h; int rc;
    if ((rc = read_ctrl(c, &h))) return rc;                        // (the wait for whatever is on the stream)
    const size_t at = (size_t)first_row * r.n_cols, cells = (size_t)n * r.n_cols;
    if (members) HIP_TRY(c, hipMemcpy(members, r.members, sizeof(uint32_t), hipMemcpyDeviceToHost));
    const std::pair<uint32_t *, const uint32_t *> words[] = { { defined, r.defined }, { hit, r.hit } };
    for (const auto &w : words)
        if (w.first && cells) HIP_TRY(c, hipMemcpy(w.first, w.second + at, sizeof(uint32_t) * cells, hipMemcpyDeviceToHost));
    const std::pair<uint64_t *, const unsigned long long *> sums[] = { { sum_0, r.sum }, { sum_1, r.sum_o }, { sumsq_0, r.sumsq }, { sumsq_1, r.sumsq_o }, { sum_cross, r.cross } };
    for (const auto &s : sums)
        if (s.first && cells) HIP_TRY(c, hipMemcpy(s.first, s.second + at, sizeof(uint64_t) * cells, hipMemcpyDeviceToHost));
    return ctrl_error(c, h);
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
    if (int rc = ensrows_begin(c, who, Ensemble::ROWS_SETTINGS, n_rows, cols)) return rc;
    Ensemble::Rows &r = c->ens.rows;
    r.mask = setting_mask; r.first = first_step; r.stride = stride; r.min = min_cases;
    c->ens.where = where; c->ens.series = true; c->ens.arrival = false; c->ens.n = cols; c->ens.valid = true;
    members_end(c);
    return ESIM_OK;
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
    if (int rc = ensrows_begin(c, who, Ensemble::ROWS_REPRODUCTION, n_rows, cols)) return rc;
    Ensemble::Rows &r = c->ens.rows;
    r.first = first_step; r.stride = stride; r.min = min_cohort; r.r_num = r_num; r.r_den = r_den;
    c->ens.where = where; c->ens.series = true; c->ens.arrival = false; c->ens.n = cols; c->ens.valid = true;
    members_end(c);
    return ESIM_OK;
}

extern "C" int esim_ensemble_read_reproduction(esim_ctx *ctx, uint32_t first_row, uint32_t n, uint32_t *members, uint32_t *defined, uint32_t *hit,
                                               uint64_t *sum_cases, uint64_t *sum_offspring, uint64_t *sumsq_cases, uint64_t *sumsq_offspring, uint64_t *sum_cross)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    return read_two_planes(c, "esim_ensemble_read_reproduction", Ensemble::ROWS_REPRODUCTION, first_row, n, members, defined, hit,
                           sum_cases, sum_offspring, sumsq_cases, sumsq_offspring, sum_cross);
}
