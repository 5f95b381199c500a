// esim_host_beds.h -- a run's admitted cases as a list on the device and what hangs on it: the kept burden baseline
// (esim_burden_baseline_keep / _info / _read / _drop), the comparison of the run as it stands with it (esim_burden_compare,
// esim_burden_compare_series), and two kinds of the ensemble accumulators over rows made from lists -- the burden-series kind
// (esim_ensemble_begin_burden_series: the buffers and the reader of the settings kind) and the burden-paired kind
// (esim_ensemble_begin_burden_paired: those of the paired kind), which esim_ensemble_fold folds with fold_beds.  The kernels:
// esim_kernels_beds.h; every launch of the family is in this file.  The checks, the run's front half and the column key are
// those of esim_host_burden.h.  A run that never asks allocates nothing here.
namespace {

// Workgroups of k_beds_collect at most: as the kernels of esim_host_burden.h, whose tables it stages.
const uint32_t BEDS_COLLECT_GRID = 1024u;
// ... of the two consumers: a workgroup a compute unit.  A workgroup of k_beds_rows ends with up to BEDS_LDS_CELLS (4096) adds
// to the global rows, one of k_beds_totals with up to 3 * BURDEN_LDS_COLS (192) to the global tables, which fewer, longer
// workgroups share among more entries.
const uint32_t BEDS_GRID = 256u;

// The list of the run as it stands, for the length of one call: the context's scratch list (BedsBaseline::tmp), allocated at
// the first call that needs one and grown when a run's log is longer -- a fold of every member of an ensemble would otherwise
// allocate and free 12 B per log entry.  Every call that uses it ends with a wait for the stream, so the next one finds it free.
struct BedsTmp {
    uint32_t *list = nullptr, *count = nullptr;
    uint32_t cap = 0;
    hipError_t alloc(esim_ctx_impl *c, uint32_t entries)
    {
        BedsBaseline &b = c->beds;
        if (!b.tmp_count && dev_alloc(c, &b.tmp_count, 2)) return hipErrorOutOfMemory;
        if (!b.tmp || b.tmp_cap < entries) {
            uint32_t *p = nullptr;
            if (dev_alloc(c, &p, 3 * (size_t)entries)) return hipErrorOutOfMemory;
            dev_free(c, b.tmp);
            b.tmp = p; b.tmp_cap = entries;
        }
        list = b.tmp; count = b.tmp_count; cap = entries;
        return hipSuccess;
    }
    BedsList dev() const { return BedsList{ list, list + cap, list + 2 * (size_t)cap, count, cap }; }
};

BedsList beds_kept(const esim_ctx_impl *c)
{
    const BedsBaseline &b = c->beds;
    return BedsList{ b.list, b.list + b.cap, b.list + 2 * b.cap, b.count, (uint32_t)b.cap };
}

// The admitted cases of the run as it stands into l (its counts zeroed first), on the stream behind burden_run's replay.
hipError_t enqueue_beds_collect(esim_ctx_impl *c, const BurdenRun &r, const uint32_t *vax, const BedsList &l)
{
    const hipError_t e = hipMemsetAsync(l.n, 0, 2 * sizeof(uint32_t), c->stream);
    if (e != hipSuccess) return e;
    const Series q = burden_query(c, ESIM_BY_ALL, 1u, r.t_done, r.t_all, r.replay ? vax : nullptr);
    hipLaunchKernelGGL(k_beds_collect, dim3(grid_capped(c, r.log_len, TPB, BEDS_COLLECT_GRID)), dim3(TPB), 0, c->stream, c->d, q, burden_dev(c), r.log_len, l);
    return hipGetLastError();
}

// The rows of esim_burden_series(where, what, ...) of the run a list was taken from (`steps`: the steps it ran; items: its
// entries at most) into the zeroed plane `rows`, summed over the rows for the occupancy and where `cumulative` asks.
hipError_t enqueue_beds_rows(esim_ctx_impl *c, const BedsList &l, uint32_t items, uint32_t steps, int where, int what, uint32_t first_step, uint32_t n_rows,
                             uint32_t stride, bool cumulative, uint32_t *rows)
{
    Series q = burden_query(c, where, first_step, steps, 0xFFFFFFFFu, nullptr);
    q.n_rows = n_rows; q.stride = stride; q.p0 = rows;
    const hipError_t e = hipMemsetAsync(rows, 0, sizeof(uint32_t) * std::max<size_t>(1, (size_t)n_rows * q.n_cols), c->stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_beds_rows, dim3(grid_capped(c, items, TPB, BEDS_GRID)), dim3(TPB), 0, c->stream, c->d, q, l, (uint32_t)what);
    if (what == ESIM_BURDEN_OCCUPANCY || cumulative)
        hipLaunchKernelGGL(k_series_prefix, dim3(grid_for(q.n_cols, TPB, 0xFFFFFFFFu)), dim3(TPB), 0, c->stream, q, nullptr, nullptr);
    return hipGetLastError();
}

// Do the rows first_step + i * stride, i < n_rows, start inside the run as it stands and, with `kept`, inside the baseline's?
bool beds_rows_inside(const esim_ctx_impl *c, uint32_t first_step, uint32_t n_rows, uint32_t stride, bool kept)
{
    const uint32_t steps = kept ? std::min(c->host_t - 1u, c->beds.steps) : c->host_t - 1u;
    return first_step != 0u && (uint64_t)first_step + (uint64_t)(n_rows - 1u) * stride <= steps;
}

// One member folded into the accumulators of the burden-series or the burden-paired kind: the checks, the member's list in
// the context's scratch list, its rows (and, paired, the kept baseline's) into the kept plane(s), the fold kernel of the kind
// the accumulators were allocated under, and the wait -- the replay's plane goes when the call returns.
int fold_beds(esim_ctx_impl *c)
{
    Rows &r = c->ens.rows;
    const Ensemble::Par &par = c->ens.par;
    const std::string who = "esim_ensemble_fold";
    const int where = c->ens.where;
    const bool paired = c->ens.kind == Ensemble::ENS_BURDEN_PAIRED;
    if (int rc = burden_ready(c, who)) return rc;
    if (curve_cols(c, where) != r.n_cols || (where == ESIM_BY_GROUP && !c->grp.lab)) return fail(c, ESIM_ESTATE, who + ": the accumulators were begun for other columns");
    if (paired && !c->beds.held) return fail(c, ESIM_ESTATE, who + ": no burden baseline is kept (esim_burden_baseline_keep)");
    if (!beds_rows_inside(c, par.first, r.n_rows, par.stride, paired))
        return fail(c, ESIM_ERANGE, paired ? who + ": rows outside the steps of the burden baseline or of the run as it stands" : who + ": rows outside the steps run so far");
    DevTmp<uint32_t> vax;
    BurdenRun run;
    if (int rc = burden_run(c, who, &vax, &run)) return rc;
    BedsTmp cur;
    if (cur.alloc(c, run.log_len) != hipSuccess) { (void)hipGetLastError(); return flows_unwind(c, fail(c, ESIM_ENOMEM, who + ": no device memory for the list (12 B per log entry)")); }
    const uint64_t cells = (uint64_t)r.n_rows * r.n_cols;
    const uint32_t fold_grid = grid_capped(c, (size_t)(cells >> 2), TPB, 2048);
    hipError_t e = enqueue_beds_collect(c, run, vax.p, cur.dev());
    if (e == hipSuccess && paired) e = enqueue_beds_rows(c, beds_kept(c), c->beds.n, c->beds.steps, where, par.burden_what, par.first, r.n_rows, par.stride, par.cumulative, r.p0);
    if (e == hipSuccess) e = enqueue_beds_rows(c, cur.dev(), run.log_len, run.t_done, where, par.burden_what, par.first, r.n_rows, par.stride, par.cumulative, paired ? r.p1 : r.p0);
    if (e == hipSuccess) {
        if (paired) hipLaunchKernelGGL(k_ensemble_fold_paired, dim3(fold_grid), dim3(TPB), 0, c->stream, r.p0, r.p1, cells, par.min_defined, par.min_averted, ratio_acc(r));
        else hipLaunchKernelGGL(k_ensemble_fold_rows, dim3(fold_grid), dim3(TPB), 0, c->stream, r.p0, cells, par.min_hit, r.hit, r.sum, r.sumsq, r.members);
        e = members_keep(c);
        if (e == hipSuccess) e = hipGetLastError();
    }
    const hipError_t es = hipStreamSynchronize(c->stream);           // (the replay's plane goes when the call returns; the scratch list is free for the next call)
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return fail(c, ESIM_ENODEVICE, who + ": " + hipGetErrorString(e));
    return ESIM_OK;
}

// What the series calls and begins of this file refuse alike, in front of the state checks.
bool beds_rows_args(int where, int what, uint32_t n_rows, uint32_t stride, int cumulative)
{
    return (where == ESIM_BY_ALL || where == ESIM_AREA_HOME || where == ESIM_BY_GROUP) && what >= ESIM_BURDEN_ADMISSIONS && what <= ESIM_BURDEN_DEATHS &&
           stride != 0u && n_rows != 0u && !(cumulative && what == ESIM_BURDEN_OCCUPANCY);
}

const char *BEDS_ROWS_ARGS = ": `where` must be ESIM_BY_ALL, ESIM_AREA_HOME or ESIM_BY_GROUP; unknown `what`, stride 0, no rows, or cumulative rows of the occupancy";

}  // namespace

extern "C" int esim_burden_baseline_keep(esim_ctx *ctx)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    const std::string who = "esim_burden_baseline_keep";
    if (int rc = burden_ready(c, who)) return rc;
    DevTmp<uint32_t> vax;
    BurdenRun r;
    if (int rc = burden_run(c, who, &vax, &r)) return rc;
    BedsBaseline &b = c->beds;
    if (!b.count && dev_alloc(c, &b.count, 2)) { (void)hipGetLastError(); return flows_unwind(c, fail(c, ESIM_ENOMEM, who + ": no device memory for the list's counts")); }
    if (!b.list || b.cap < r.log_len) {
        uint32_t *list = nullptr;
        if (dev_alloc(c, &list, 3 * (size_t)r.log_len)) { (void)hipGetLastError(); return flows_unwind(c, fail(c, ESIM_ENOMEM, who + ": no device memory for the list (12 B per log entry)")); }
        dev_free(c, b.list);                                         // (the stream was idle behind burden_run's wait: nothing reads the old list)
        b.list = list; b.cap = r.log_len;
    }
    b.held = false;
    hipError_t e = enqueue_beds_collect(c, r, vax.p, beds_kept(c));
    uint32_t counts[2] = { 0u, 0u };
    const hipError_t es = hipStreamSynchronize(c->stream);           // (the replay's plane goes when the call returns)
    if (e == hipSuccess) e = es;
    if (e == hipSuccess) e = hipMemcpy(counts, b.count, sizeof counts, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(c, ESIM_ENODEVICE, who + ": " + hipGetErrorString(e));
    b.held = true; b.steps = r.t_done; b.n = std::min<uint32_t>(counts[0], (uint32_t)b.cap); b.n_died = counts[1]; b.P = c->P;
    return ESIM_OK;
}

extern "C" int esim_burden_baseline_info(esim_ctx *ctx, uint32_t *steps, uint32_t *n_admitted, uint32_t *n_died, esim_params *p)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    if (!c->uploaded || !c->beds.held) return fail(c, ESIM_ESTATE, "esim_burden_baseline_info: no burden baseline is kept (esim_burden_baseline_keep)");
    if (steps) *steps = c->beds.steps;
    if (n_admitted) *n_admitted = c->beds.n;
    if (n_died) *n_died = c->beds.n_died;
    if (p) *p = c->beds.P;
    return ESIM_OK;
}

extern "C" int esim_burden_baseline_drop(esim_ctx *ctx)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    if (!c->uploaded || !c->beds.held) return fail(c, ESIM_ESTATE, "esim_burden_baseline_drop: no burden baseline is kept (esim_burden_baseline_keep)");
    c->beds.held = false;                                            // (the list stays for the next keep)
    return ESIM_OK;
}

extern "C" int esim_burden_baseline_read(esim_ctx *ctx, uint32_t *citizen, uint32_t *admit_step, uint32_t *end_step, uint8_t *died, uint32_t cap, uint32_t *n_out)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    const std::string who = "esim_burden_baseline_read";
    if (!n_out) return fail(c, ESIM_EINVAL, who + ": null n_out");
    const BedsBaseline &b = c->beds;
    if (!c->uploaded || !b.held) return fail(c, ESIM_ESTATE, who + ": no burden baseline is kept (esim_burden_baseline_keep)");
    *n_out = b.n;
    if (b.n > cap) return fail(c, ESIM_ERANGE, who + ": buffers too small (n_out holds the size needed)");
    HIP_TRY(c, hipSetDevice(c->P.device));
    const size_t bytes = sizeof(uint32_t) * (size_t)b.n;
    if (citizen && bytes) HIP_TRY(c, hipMemcpy(citizen, b.list, bytes, hipMemcpyDeviceToHost));
    if (admit_step && bytes) HIP_TRY(c, hipMemcpy(admit_step, b.list + b.cap, bytes, hipMemcpyDeviceToHost));
    if ((end_step || died) && bytes) {
        std::vector<uint32_t> word(b.n);
        HIP_TRY(c, hipMemcpy(word.data(), b.list + 2 * b.cap, bytes, hipMemcpyDeviceToHost));
        for (uint32_t i = 0; i < b.n; ++i) {
            if (end_step) end_step[i] = word[i] & ~BEDS_DIED;
            if (died) died[i] = (word[i] & BEDS_DIED) ? 1u : 0u;
        }
    }
    return ESIM_OK;
}

extern "C" int esim_burden_compare(esim_ctx *ctx, int where, uint32_t first_step, uint32_t last_step, uint64_t *bed_steps_b, uint64_t *bed_steps_c, uint32_t *admissions_b,
                                   uint32_t *admissions_c, uint32_t *deaths_b, uint32_t *deaths_c)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    const std::string who = "esim_burden_compare";
    if (where != ESIM_BY_ALL && where != ESIM_AREA_HOME && where != ESIM_BY_GROUP) return fail(c, ESIM_EINVAL, who + BURDEN_WHERE);
    if (int rc = burden_ready(c, who)) return rc;
    if (where == ESIM_BY_GROUP && !c->grp.lab) return fail(c, ESIM_ESTATE, who + ": by group without labels (esim_set_groups)");
    if (!c->beds.held) return fail(c, ESIM_ESTATE, who + ": no burden baseline is kept (esim_burden_baseline_keep)");
    if (first_step == 0u || last_step < first_step || last_step > std::min(c->host_t - 1u, c->beds.steps))
        return fail(c, ESIM_ERANGE, who + ": first_step 0, last_step before first_step, or beyond the steps of the burden baseline or of the run as it stands");
    DevTmp<uint32_t> vax, cnt; DevTmp<unsigned long long> wide;
    BurdenRun r;
    if (int rc = burden_run(c, who, &vax, &r)) return rc;
    const size_t cols = curve_cols(c, where);
    BedsTmp cur;
    if (cur.alloc(c, r.log_len) != hipSuccess || wide.alloc(2 * cols) != hipSuccess || cnt.alloc(4 * cols) != hipSuccess) {
        (void)hipGetLastError();
        return flows_unwind(c, fail(c, ESIM_ENOMEM, who + ": no device memory for the list (12 B per log entry) and the tables (32 B per column)"));
    }
    // the tables: bed_steps of the baseline and of the run [2][cols]; admissions and deaths of the baseline, then of the run [4][cols]
    hipError_t e = hipMemsetAsync(wide.p, 0, sizeof(unsigned long long) * std::max<size_t>(1, 2 * cols), c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(cnt.p, 0, sizeof(uint32_t) * std::max<size_t>(1, 4 * cols), c->stream);
    if (e == hipSuccess) e = enqueue_beds_collect(c, r, vax.p, cur.dev());
    if (e == hipSuccess) {
        const Series q = burden_query(c, where, first_step, r.t_done, 0xFFFFFFFFu, nullptr);
        hipLaunchKernelGGL(k_beds_totals, dim3(grid_capped(c, c->beds.n, TPB, BEDS_GRID)), dim3(TPB), 0, c->stream, c->d, q, beds_kept(c), first_step, last_step,
                           wide.p, cnt.p, cnt.p + cols);
        hipLaunchKernelGGL(k_beds_totals, dim3(grid_capped(c, r.log_len, TPB, BEDS_GRID)), dim3(TPB), 0, c->stream, c->d, q, cur.dev(), first_step, last_step,
                           wide.p + cols, cnt.p + 2 * cols, cnt.p + 3 * cols);
        e = hipGetLastError();
    }
    const hipError_t es = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = es;
    std::vector<unsigned long long> h_wide(2 * cols);
    std::vector<uint32_t> h_cnt(4 * cols);
    if (e == hipSuccess && cols) e = hipMemcpy(h_wide.data(), wide.p, sizeof(unsigned long long) * 2 * cols, hipMemcpyDeviceToHost);
    if (e == hipSuccess && cols) e = hipMemcpy(h_cnt.data(), cnt.p, sizeof(uint32_t) * 4 * cols, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(c, ESIM_ENODEVICE, who + ": " + hipGetErrorString(e));
    for (size_t k = 0; k < cols; ++k) {
        if (bed_steps_b) bed_steps_b[k] = h_wide[k];
        if (bed_steps_c) bed_steps_c[k] = h_wide[cols + k];
        if (admissions_b) admissions_b[k] = h_cnt[k];
        if (deaths_b) deaths_b[k] = h_cnt[cols + k];
        if (admissions_c) admissions_c[k] = h_cnt[2 * cols + k];
        if (deaths_c) deaths_c[k] = h_cnt[3 * cols + k];
    }
    return ESIM_OK;
}

extern "C" int esim_burden_compare_series(esim_ctx *ctx, int where, int what, uint32_t first_step, uint32_t n_rows, uint32_t stride, int cumulative, uint32_t *baseline,
                                          uint32_t *current)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    const std::string who = "esim_burden_compare_series";
    if (!beds_rows_args(where, what, n_rows, stride, cumulative)) return fail(c, ESIM_EINVAL, who + BEDS_ROWS_ARGS);
    if (int rc = burden_ready(c, who)) return rc;
    if (where == ESIM_BY_GROUP && !c->grp.lab) return fail(c, ESIM_ESTATE, who + ": by group without labels (esim_set_groups)");
    if (!c->beds.held) return fail(c, ESIM_ESTATE, who + ": no burden baseline is kept (esim_burden_baseline_keep)");
    if (!beds_rows_inside(c, first_step, n_rows, stride, true))
        return fail(c, ESIM_ERANGE, who + ": first_step 0, or rows outside the steps of the burden baseline or of the run as it stands");
    DevTmp<uint32_t> vax, rows_b, rows_c;
    BurdenRun r;
    if (int rc = burden_run(c, who, &vax, &r)) return rc;
    const size_t words = (size_t)n_rows * curve_cols(c, where);
    BedsTmp cur;
    if (cur.alloc(c, r.log_len) != hipSuccess || rows_b.alloc(words) != hipSuccess || rows_c.alloc(words) != hipSuccess) {
        (void)hipGetLastError();
        return flows_unwind(c, fail(c, ESIM_ENOMEM, who + ": no device memory for the list (12 B per log entry) and the rows (ask for fewer)"));
    }
    hipError_t e = enqueue_beds_collect(c, r, vax.p, cur.dev());
    if (e == hipSuccess) e = enqueue_beds_rows(c, beds_kept(c), c->beds.n, c->beds.steps, where, what, first_step, n_rows, stride, cumulative != 0, rows_b.p);
    if (e == hipSuccess) e = enqueue_beds_rows(c, cur.dev(), r.log_len, r.t_done, where, what, first_step, n_rows, stride, cumulative != 0, rows_c.p);
    const hipError_t es = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = es;
    if (e == hipSuccess && baseline && words) e = hipMemcpy(baseline, rows_b.p, sizeof(uint32_t) * words, hipMemcpyDeviceToHost);
    if (e == hipSuccess && current && words) e = hipMemcpy(current, rows_c.p, sizeof(uint32_t) * words, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(c, ESIM_ENODEVICE, who + ": " + hipGetErrorString(e));
    return ESIM_OK;
}

extern "C" int esim_ensemble_begin_burden_series(esim_ctx *ctx, int where, int what, uint32_t first_step, uint32_t n_rows, uint32_t stride, uint32_t min_count)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    const std::string who = "esim_ensemble_begin_burden_series";
    if (!beds_rows_args(where, what, n_rows, stride, 0)) return fail(c, ESIM_EINVAL, who + BEDS_ROWS_ARGS);
    if (int rc = burden_ready(c, who)) return rc;
    if (int rc = ensrows_begin_check(c, who, where)) return rc;
    if (first_step == 0u) return fail(c, ESIM_ERANGE, who + ": first_step is 1-based");
    HIP_TRY(c, hipSetDevice(c->P.device));
    const uint32_t cols = curve_cols(c, where);
    Ensemble::Par par;
    par.burden_what = what; par.first = first_step; par.stride = stride; par.min_hit = min_count;
    return ens_begin(c, who, Ensemble::ENS_BURDEN_SERIES, where, n_rows, cols, par);
}

extern "C" int esim_ensemble_begin_burden_paired(esim_ctx *ctx, int where, int what, uint32_t first_step, uint32_t n_rows, uint32_t stride, int cumulative,
                                                 uint32_t min_baseline, uint32_t min_averted)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    const std::string who = "esim_ensemble_begin_burden_paired";
    if (!beds_rows_args(where, what, n_rows, stride, cumulative) || min_averted == 0u) return fail(c, ESIM_EINVAL, who + BEDS_ROWS_ARGS + "; or min_averted 0");
    if (int rc = burden_ready(c, who)) return rc;
    if (int rc = ensrows_begin_check(c, who, where)) return rc;             // (no baseline is asked for: every member keeps its own before its policy run)
    if (first_step == 0u) return fail(c, ESIM_ERANGE, who + ": first_step is 1-based");
    HIP_TRY(c, hipSetDevice(c->P.device));
    const uint32_t cols = curve_cols(c, where);
    Ensemble::Par par;
    par.burden_what = what; par.first = first_step; par.stride = stride; par.min_defined = min_baseline; par.min_averted = min_averted; par.cumulative = cumulative != 0;
    return ens_begin(c, who, Ensemble::ENS_BURDEN_PAIRED, where, n_rows, cols, par);
}
