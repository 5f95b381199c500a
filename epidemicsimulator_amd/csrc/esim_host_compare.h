// esim_host_compare.h -- the paired comparison of two runs: esim_baseline_keep / _info / _drop (the exposure steps of a finished
// run kept on the device, beside the snapshot), esim_compare and esim_compare_series (the run as it stands against it), and the
// paired kind of the ensemble accumulators over rows, esim_ensemble_begin_paired / esim_ensemble_read_paired, with what
// esim_ensemble_fold does with it in force (the kernels: esim_kernels_compare.h).  Every draw is a pure function of
// (seed, global citizen, step, slot): two runs under one seed and the same index cases share their random numbers, so a citizen
// exposed in one and not in the other is an effect of what differs between them.  No step kernel is involved.
namespace {

// What every call here refuses alike, behind its own argument checks: the rule of esim_restart, and no shard.
int compare_check(esim_ctx_impl *c, const std::string &who)
{
    if (!c->uploaded) return fail(c, ESIM_ESTATE, who + ": no population uploaded");
    if (c->comm.world > 1 || c->d.n_global != c->d.n)
        return fail(c, ESIM_ESTATE, who + ": the context has a communicator of several ranks, or holds a shard (the rule of esim_restart)");
    return ESIM_OK;
}

// `where` of the comparison calls: one column, by the area of the household, by group.
bool compare_where(int where) { return where == ESIM_BY_ALL || where == ESIM_AREA_HOME || where == ESIM_BY_GROUP; }

uint32_t compare_cols(const esim_ctx_impl *c, int where) { return where == ESIM_BY_ALL ? 1u : where == ESIM_BY_GROUP ? c->grp.n : c->d.n_areas; }

// The one wait of a call: the control block read back, its sticky error reported as the series calls report it; *log_len = the
// entries of the exposure log.
int compare_wait(esim_ctx_impl *c, uint32_t *log_len)
{
    Ctrl h; int rc;
    if ((rc = read_ctrl(c, &h)) || (rc = ctrl_error(c, h))) return rc;
    *log_len = std::min<uint32_t>(h.log_len, c->d.n);
    return ESIM_OK;
}

// plane[citizen] = the exposure step of the run as it stands, on the context's stream.
hipError_t enqueue_plane(esim_ctx_impl *c, uint32_t log_len, uint32_t *plane)
{
    const hipError_t e = hipMemsetAsync(plane, 0xFF, sizeof(uint32_t) * std::max<size_t>(1, c->d.n), c->stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_compare_plane, dim3(grid_capped(c, log_len, TPB, 4096)), dim3(TPB), 0, c->stream, c->d, c->host_t - 1u, log_len, plane);
    return hipGetLastError();
}

// The event rows of the baseline and of the plane `cur` into two zeroed tables, summed up over the rows where asked for.
hipError_t enqueue_compare_rows(esim_ctx_impl *c, int where, uint32_t first_step, uint32_t n_rows, uint32_t stride, bool cumulative, uint32_t cols,
                                const uint32_t *cur, uint32_t *rows_b, uint32_t *rows_c)
{
    const size_t words = (size_t)n_rows * cols;
    hipError_t e = hipMemsetAsync(rows_b, 0, sizeof(uint32_t) * std::max<size_t>(1, words), c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(rows_c, 0, sizeof(uint32_t) * std::max<size_t>(1, words), c->stream);
    if (e != hipSuccess) return e;
    CompareRows r;
    r.base = c->base.plane; r.cur = cur; r.where = (uint32_t)where; r.first = first_step; r.n_rows = n_rows; r.stride = stride; r.n_cols = cols;
    r.grp = where == ESIM_BY_GROUP ? c->grp.lab : nullptr; r.rows_b = rows_b; r.rows_c = rows_c;
    hipLaunchKernelGGL(k_compare_rows, dim3(grid_capped(c, ((size_t)c->d.n + 3u) / 4u, TPB, 4096)), dim3(TPB), 0, c->stream, c->d, r);
    if (cumulative) hipLaunchKernelGGL(k_compare_prefix, dim3(grid_for(cols, TPB, 0xFFFFFFFFu)), dim3(TPB), 0, c->stream, rows_b, rows_c, n_rows, cols);
    return hipGetLastError();
}

// Do the rows [first_step + i * stride, + stride), i < n_rows, start inside both runs?
bool rows_inside(const esim_ctx_impl *c, uint32_t first_step, uint32_t n_rows, uint32_t stride)
{
    return (uint64_t)first_step + (uint64_t)(n_rows - 1u) * stride <= std::min(c->host_t - 1u, c->base.steps);
}

// One member folded into the accumulators of the paired kind: the checks, the one wait, the current run's plane in temporary
// device memory, the rows of both runs into the kept planes, the fold kernel.
int fold_paired(esim_ctx_impl *c)
{
    Rows &r = c->ens.rows;
    const Ensemble::Par &par = c->ens.par;
    const std::string who = "esim_ensemble_fold";
    const int where = c->ens.where;
    if (int rc = compare_check(c, who)) return rc;
    if (where == ESIM_BY_GROUP && (!c->grp.lab || c->grp.n != r.n_cols)) return fail(c, ESIM_ESTATE, who + ": the accumulators were begun for other columns");
    if (!c->base.held) return fail(c, ESIM_ESTATE, who + ": no baseline is kept (esim_baseline_keep)");
    if (!rows_inside(c, par.first, r.n_rows, par.stride)) return fail(c, ESIM_ERANGE, who + ": rows outside the steps of the baseline or of the run as it stands");
    HIP_TRY(c, hipSetDevice(c->P.device));
    uint32_t log_len = 0;
    if (int rc = compare_wait(c, &log_len)) return rc;
    DevTmp<uint32_t> cur;
    if (cur.alloc(c->d.n) != hipSuccess) { (void)hipGetLastError(); return fail(c, ESIM_ENOMEM, who + ": no device memory for the exposure steps (4 B per citizen)"); }
    hipError_t e = enqueue_plane(c, log_len, cur.p);
    if (e == hipSuccess) e = enqueue_compare_rows(c, where, par.first, r.n_rows, par.stride, par.cumulative, r.n_cols, cur.p, r.p0, r.p1);
    if (e == hipSuccess) {
        const uint64_t cells = (uint64_t)r.n_rows * r.n_cols;
        hipLaunchKernelGGL(k_ensemble_fold_paired, dim3(grid_capped(c, (size_t)(cells >> 2), TPB, 2048)), dim3(TPB), 0, c->stream, r.p0, r.p1, cells, par.min_defined, par.min_averted, ratio_acc(r));
        e = members_keep(c);
        if (e == hipSuccess) e = hipGetLastError();
    }
    const hipError_t es = hipStreamSynchronize(c->stream);           // (the temporary plane goes when the call returns)
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return fail(c, ESIM_ENODEVICE, who + ": " + hipGetErrorString(e));
    return ESIM_OK;
}

}  // namespace

extern "C" int esim_baseline_keep(esim_ctx *ctx)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    const std::string who = "esim_baseline_keep";
    if (int rc = compare_check(c, who)) return rc;
    HIP_TRY(c, hipSetDevice(c->P.device));
    uint32_t log_len = 0;
    if (int rc = compare_wait(c, &log_len)) return rc;
    Baseline &b = c->base;
    if (!b.plane) {
        if (dev_alloc(c, &b.plane, c->d.n)) { (void)hipGetLastError(); return fail(c, ESIM_ENOMEM, who + ": no device memory for the exposure steps (4 B per citizen)"); }
    }
    b.held = false;
    const hipError_t e = enqueue_plane(c, log_len, b.plane);
    if (e != hipSuccess) return fail(c, ESIM_ENODEVICE, who + ": " + hipGetErrorString(e));
    b.held = true; b.steps = c->host_t - 1u; b.n_cases = log_len; b.P = c->P;
    return ESIM_OK;
}

extern "C" int esim_baseline_info(esim_ctx *ctx, uint32_t *steps, uint32_t *n_cases, esim_params *p)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    if (!c->uploaded || !c->base.held) return fail(c, ESIM_ESTATE, "esim_baseline_info: no baseline is kept (esim_baseline_keep)");
    if (steps) *steps = c->base.steps;
    if (n_cases) *n_cases = c->base.n_cases;
    if (p) *p = c->base.P;
    return ESIM_OK;
}

extern "C" int esim_baseline_drop(esim_ctx *ctx)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    if (!c->uploaded || !c->base.held) return fail(c, ESIM_ESTATE, "esim_baseline_drop: no baseline is kept (esim_baseline_keep)");
    c->base.held = false;                                            // (the plane stays for the next keep)
    return ESIM_OK;
}

extern "C" int esim_compare(esim_ctx *ctx, int where, uint32_t first_step, uint32_t last_step, uint64_t *counts, int64_t *delay, uint32_t *first_divergence, uint8_t *cls)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    const std::string who = "esim_compare";
    if (!compare_where(where)) return fail(c, ESIM_EINVAL, who + ": `where` must be ESIM_BY_ALL, ESIM_AREA_HOME or ESIM_BY_GROUP");
    if (int rc = compare_check(c, who)) return rc;
    if (where == ESIM_BY_GROUP && !c->grp.lab) return fail(c, ESIM_ESTATE, who + ": by group without labels (esim_set_groups)");
    if (!c->base.held) return fail(c, ESIM_ESTATE, who + ": no baseline is kept (esim_baseline_keep)");
    if (last_step < first_step || last_step > std::min(c->host_t - 1u, c->base.steps))
        return fail(c, ESIM_ERANGE, who + ": last_step before first_step, or beyond the steps of the baseline or of the run as it stands");
    HIP_TRY(c, hipSetDevice(c->P.device));
    uint32_t log_len = 0;
    if (int rc = compare_wait(c, &log_len)) return rc;
    const size_t n = c->d.n;
    const uint32_t cols = compare_cols(c, where);
    DevTmp<uint32_t> cur, cnt, div; DevTmp<unsigned long long> dly; DevTmp<uint8_t> d_cls;
    if (cur.alloc(n) != hipSuccess || cnt.alloc((size_t)cols * ESIM_CMP_N) != hipSuccess || dly.alloc(cols) != hipSuccess || div.alloc(1) != hipSuccess ||
        (cls && d_cls.alloc(n) != hipSuccess)) {
        (void)hipGetLastError();
        return fail(c, ESIM_ENOMEM, who + ": no device memory for the exposure steps (4 B per citizen, 1 more for the classes) and the tables");
    }
    hipError_t e = enqueue_plane(c, log_len, cur.p);
    if (e == hipSuccess) e = hipMemsetAsync(cnt.p, 0, sizeof(uint32_t) * (size_t)cols * ESIM_CMP_N, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(dly.p, 0, sizeof(unsigned long long) * cols, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(div.p, 0xFF, sizeof(uint32_t), c->stream);
    if (e == hipSuccess && cls) e = hipMemsetAsync(d_cls.p, 0, std::max<size_t>(1, n), c->stream);
    if (e == hipSuccess) {
        Compare q;
        q.base = c->base.plane; q.cur = cur.p; q.where = (uint32_t)where; q.first = first_step; q.last = last_step; q.n_cols = cols;
        // stretches of whole trips, about 4096 of them at most: short enough to stay inside the LDS window of areas
        q.per_block = (uint32_t)std::max<uint64_t>(4u * COMPARE_QUAD, (((uint64_t)n + 4095u) / 4096u + COMPARE_QUAD - 1u) / COMPARE_QUAD * COMPARE_QUAD);
        q.grp = where == ESIM_BY_GROUP ? c->grp.lab : nullptr; q.counts = cnt.p; q.delay = dly.p; q.first_div = div.p; q.cls = cls ? d_cls.p : nullptr;
        hipLaunchKernelGGL(k_compare_count, dim3((uint32_t)std::max<uint64_t>(1u, ((uint64_t)n + q.per_block - 1u) / q.per_block)), dim3(TPB), 0, c->stream, c->d, q);
        e = hipGetLastError();
    }
    // the two tables come back through the pinned mirror of the census tables (20 B per area, or per group: room for either),
    // one after the other: by area they are megabytes, which a copy into pageable memory takes several times longer over
    uint32_t *mirror = where == ESIM_BY_GROUP ? c->pin.grp : c->pin.area;
    const size_t n_cnt = (size_t)cols * ESIM_CMP_N;
    if (e == hipSuccess && counts) e = hipMemcpyAsync(mirror, cnt.p, sizeof(uint32_t) * n_cnt, hipMemcpyDeviceToHost, c->stream);
    hipError_t es = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = es;
    if (e == hipSuccess && counts) std::copy(mirror, mirror + n_cnt, counts);
    if (e == hipSuccess && delay) {
        e = hipMemcpyAsync(mirror, dly.p, sizeof(int64_t) * cols, hipMemcpyDeviceToHost, c->stream);
        es = hipStreamSynchronize(c->stream);
        if (e == hipSuccess) e = es;
        if (e == hipSuccess) std::memcpy(delay, mirror, sizeof(int64_t) * cols);
    }
    if (e == hipSuccess && first_divergence) e = hipMemcpy(first_divergence, div.p, sizeof(uint32_t), hipMemcpyDeviceToHost);
    if (e == hipSuccess && cls && n) e = hipMemcpy(cls, d_cls.p, n, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(c, ESIM_ENODEVICE, who + ": " + hipGetErrorString(e));
    return ESIM_OK;
}

extern "C" int esim_compare_series(esim_ctx *ctx, int where, uint32_t first_step, uint32_t n_rows, uint32_t stride, int cumulative, uint32_t *baseline, uint32_t *current)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    const std::string who = "esim_compare_series";
    if (!compare_where(where) || stride == 0 || n_rows == 0)
        return fail(c, ESIM_EINVAL, who + ": `where` must be ESIM_BY_ALL, ESIM_AREA_HOME or ESIM_BY_GROUP; stride 0 or no rows");
    if (int rc = compare_check(c, who)) return rc;
    if (where == ESIM_BY_GROUP && !c->grp.lab) return fail(c, ESIM_ESTATE, who + ": by group without labels (esim_set_groups)");
    if (!c->base.held) return fail(c, ESIM_ESTATE, who + ": no baseline is kept (esim_baseline_keep)");
    if (!rows_inside(c, first_step, n_rows, stride)) return fail(c, ESIM_ERANGE, who + ": rows outside the steps of the baseline or of the run as it stands");
    HIP_TRY(c, hipSetDevice(c->P.device));
    uint32_t log_len = 0;
    if (int rc = compare_wait(c, &log_len)) return rc;
    const uint32_t cols = compare_cols(c, where);
    const size_t words = (size_t)n_rows * cols;
    DevTmp<uint32_t> cur, rows_b, rows_c;
    if (cur.alloc(c->d.n) != hipSuccess || rows_b.alloc(words) != hipSuccess || rows_c.alloc(words) != hipSuccess) {
        (void)hipGetLastError();
        return fail(c, ESIM_ENOMEM, who + ": no device memory for the exposure steps (4 B per citizen) and the rows (ask for fewer)");
    }
    hipError_t e = enqueue_plane(c, log_len, cur.p);
    if (e == hipSuccess) e = enqueue_compare_rows(c, where, first_step, n_rows, stride, cumulative != 0, cols, cur.p, rows_b.p, rows_c.p);
    const hipError_t es = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = es;
    if (e == hipSuccess && baseline && words) e = hipMemcpy(baseline, rows_b.p, sizeof(uint32_t) * words, hipMemcpyDeviceToHost);
    if (e == hipSuccess && current && words) e = hipMemcpy(current, rows_c.p, sizeof(uint32_t) * words, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(c, ESIM_ENODEVICE, who + ": " + hipGetErrorString(e));
    return ESIM_OK;
}

extern "C" int esim_ensemble_begin_paired(esim_ctx *ctx, int where, uint32_t first_step, uint32_t n_rows, uint32_t stride, int cumulative, uint32_t min_baseline, uint32_t min_averted)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    const std::string who = "esim_ensemble_begin_paired";
    if (!compare_where(where) || stride == 0 || n_rows == 0 || min_averted == 0)
        return fail(c, ESIM_EINVAL, who + ": `where` must be ESIM_BY_ALL, ESIM_AREA_HOME or ESIM_BY_GROUP; stride 0, no rows or min_averted 0");
    if (int rc = ensrows_begin_check(c, who, where)) return rc;
    HIP_TRY(c, hipSetDevice(c->P.device));
    const uint32_t cols = compare_cols(c, where);
    Ensemble::Par par;
    par.first = first_step; par.stride = stride; par.min_defined = min_baseline; par.min_averted = min_averted; par.cumulative = cumulative != 0;
    return ens_begin(c, who, Ensemble::ENS_PAIRED, where, n_rows, cols, par);
}

extern "C" int esim_ensemble_read_paired(esim_ctx *ctx, uint32_t first_row, uint32_t n, uint32_t *members, uint32_t *defined, uint32_t *hit,
                                         uint64_t *sum_baseline, uint64_t *sum_current, uint64_t *sumsq_baseline, uint64_t *sumsq_current, uint64_t *sum_cross)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    return ens_read(c, READ_PAIRED, first_row, n, members, { { defined, &Rows::defined }, { hit, &Rows::hit } },
                    { { sum_baseline, &Rows::sum }, { sum_current, &Rows::sum_o }, { sumsq_baseline, &Rows::sumsq }, { sumsq_current, &Rows::sumsq_o }, { sum_cross, &Rows::cross } });
}
