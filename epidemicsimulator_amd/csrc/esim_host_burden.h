// esim_host_burden.h -- hospital burden over a finished run: the severity tables (esim_burden_set / _drop / _get),
// esim_burden_outcomes, esim_burden_series on the series engine's rows, esim_burden_summary on curve_enqueue with the events
// kernel exchanged, and the peaks kind of the ensemble accumulators over the occupancy curve (esim_ensemble_begin_burden_peaks,
// fold_burden_peaks).  The kernels: esim_kernels_burden.h.  Every launch of the family is in this file.  Everything a call
// computes lives in temporary device memory; the tables are the only state kept.
namespace {

// Workgroups of the three kernels at most: each stages up to 8.5 KB of tables in LDS before its first entry, and k_burden_events
// ends with up to 2 * BURDEN_LDS_COLS adds to the global tables -- four workgroups a compute unit, eight trips on a log of 2 M.
const uint32_t BURDEN_GRID = 1024u;

void burden_forget(esim_ctx_impl *c)
{
    if (c->burden.tab) (void)hipStreamSynchronize(c->stream);     // (a fold on the stream may still be reading them)
    dev_free(c, c->burden.tab);
    c->burden = BurdenState();
    c->beds.held = false;                                         // (a kept burden baseline was drawn under these tables; its list stays for the next keep)
}

// What every call that computes refuses alike, in front of its own argument checks.
int burden_ready(esim_ctx_impl *c, const std::string &who)
{
    if (!c->uploaded) return fail(c, ESIM_ESTATE, who + ": no population uploaded");
    if (c->comm.world > 1 || c->d.n_global != c->d.n)
        return fail(c, ESIM_ESTATE, who + ": the context has a communicator of several ranks or holds a shard (sharded burden is not built)");
    const BurdenState &b = c->burden;
    if (!b.set) return fail(c, ESIM_ESTATE, who + ": no severity tables in force (esim_burden_set)");
    if (b.n_groups != 1u && (!c->grp.lab || c->grp.n != b.n_groups))
        return fail(c, ESIM_ESTATE, who + ": the severity tables need the labels of esim_set_groups with the same number of groups");
    return ESIM_OK;
}

// The tables as the kernels take them, with the seam of a rollback under another seed.
Burden burden_dev(const esim_ctx_impl *c)
{
    const BurdenState &s = c->burden;
    Burden b;
    b.tab = s.tab; b.n_groups = s.n_groups; b.n_delay = s.n_delay; b.n_stay = s.n_stay; b.delay_unit = s.delay_unit; b.stay_unit = s.stay_unit;
    b.grp = s.n_groups != 1u ? c->grp.lab : nullptr;
    b.seam_step = c->seam.step; b.old_seed_lo = (uint32_t)c->seam.seed; b.old_seed_hi = (uint32_t)(c->seam.seed >> 32);
    return b;
}

// What the kernels read of the run: the steps run, the window's first step, the column key and the vaccination replay.
Series burden_query(const esim_ctx_impl *c, int where, uint32_t first, uint32_t t_done, uint32_t t_all, const uint32_t *vax)
{
    Series q = Series();
    q.first = first; q.t_done = t_done; q.t_all = t_all; q.vax_of = vax; q.n_cols = curve_cols(c, where);
    q.key = where == ESIM_BY_ALL ? CURVE_BY_ALL : where == ESIM_BY_GROUP ? (uint32_t)KEY_GROUP : (uint32_t)KEY_HOME;
    q.grp = where == ESIM_BY_GROUP ? c->grp.lab : nullptr;
    return q;
}

// The front half of the calls that walk the log outside curve_enqueue: the wait for the stream, the run's shape, the log's
// length, and the vaccination replay enqueued into `vax` once a programme has run.
struct BurdenRun { uint32_t t_done = 0, log_len = 0, t_all = 0xFFFFFFFFu; bool replay = false; };
int burden_run(esim_ctx_impl *c, const std::string &who, DevTmp<uint32_t> *vax, BurdenRun *r)
{
    r->t_done = c->host_t - 1u;
    HIP_TRY(c, hipSetDevice(c->P.device));
    Ctrl h; int rc;
    if ((rc = read_ctrl(c, &h)) || (rc = ctrl_error(c, h))) return rc;
    RunShape shape;
    if ((rc = run_shape(c, r->t_done, &shape))) return rc;
    r->replay = shape.trigger != 0u; r->t_all = shape.t_all;
    r->log_len = std::min<uint32_t>(h.log_len, c->d.n);
    if (r->replay) {
        if (vax->alloc(c->d.n) != hipSuccess) { (void)hipGetLastError(); return fail(c, ESIM_ENOMEM, who + ": no device memory for the vaccination replay (4 B per citizen)"); }
        const hipError_t e = enqueue_vax_replay(c, shape.trigger, r->t_done, vax->p);
        if (e != hipSuccess) return flows_unwind(c, fail(c, ESIM_ENODEVICE, who + ": " + hipGetErrorString(e)));
    }
    return ESIM_OK;
}

// The [cols] tables of admissions and deaths beside the curve's own, and curve_enqueue's enqueuer that fills them.
struct BurdenCounts { DevTmp<uint32_t> tab; uint32_t cols = 0; };

void burden_events(esim_ctx_impl *c, const Series &q, uint32_t last, uint32_t log_len, const PairTable &t, void *user)
{
    BurdenCounts *n = (BurdenCounts *)user;
    hipLaunchKernelGGL(k_burden_events, dim3(grid_capped(c, log_len, TPB, BURDEN_GRID)), dim3(TPB), 0, c->stream, c->d, q, burden_dev(c), last, log_len, t, n->tab.p, n->tab.p + n->cols);
}

// The occupancy curve's summary into w->t and the counts into n, on the stream, as curve_enqueue leaves a status curve's.
int burden_enqueue(esim_ctx_impl *c, const std::string &who, const CurveSpec &s, CurveWork *w, BurdenCounts *n)
{
    n->cols = curve_cols(c, s.where);
    if (s.last > c->host_t - 1u) return fail(c, ESIM_ERANGE, who + ": last_step lies beyond the steps run so far");
    HIP_TRY(c, hipSetDevice(c->P.device));
    if (n->tab.alloc(2 * (size_t)n->cols) != hipSuccess) { (void)hipGetLastError(); return fail(c, ESIM_ENOMEM, who + ": no device memory for the tables (8 B per column)"); }
    HIP_TRY(c, hipMemsetAsync(n->tab.p, 0, sizeof(uint32_t) * std::max<size_t>(1, 2 * (size_t)n->cols), c->stream));
    return curve_enqueue(c, who, s, w, burden_events, n);
}

const char *BURDEN_WHERE = ": `where` must be ESIM_BY_ALL, ESIM_AREA_HOME or ESIM_BY_GROUP";

// One member's occupancy summary folded into the accumulators of the burden-peaks kind.
int fold_burden_peaks(esim_ctx_impl *c)
{
    const Ensemble::Par &par = c->ens.par;
    const std::string who = "esim_ensemble_fold";
    const CurveSpec s = { c->ens.where, CURVE_MASK_I, par.first, par.last, par.threshold };
    if (int rc = burden_ready(c, who)) return rc;
    if (int rc = curve_check(c, who, s)) return rc;
    if (curve_cols(c, s.where) != c->ens.rows.n_cols) return fail(c, ESIM_ESTATE, who + ": the accumulators were begun for other columns");
    CurveWork w;
    BurdenCounts n;
    if (int rc = burden_enqueue(c, who, s, &w, &n)) return rc;
    return fold_peaks_tables(c, who, w);
}

}  // namespace

extern "C" int esim_burden_set(esim_ctx *ctx, const esim_burden_params *p)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    const std::string who = "esim_burden_set";
    if (!p || !p->admit_thr || !p->death_thr || (p->n_delay && !p->delay_cdf) || (p->n_stay && !p->stay_cdf)) return fail(c, ESIM_EINVAL, who + ": null parameters or tables");
    if (p->n_groups == 0u || p->n_groups > (uint32_t)ESIM_MAX_GROUPS) return fail(c, ESIM_EINVAL, who + ": n_groups must be in 1..ESIM_MAX_GROUPS (1024)");
    if (p->n_delay > (uint32_t)ESIM_BURDEN_BINS || p->n_stay > (uint32_t)ESIM_BURDEN_BINS) return fail(c, ESIM_EINVAL, who + ": a CDF has more than ESIM_BURDEN_BINS (64) entries");
    if (p->delay_unit == 0u || p->delay_unit > 65535u || p->stay_unit == 0u || p->stay_unit > 65535u) return fail(c, ESIM_EINVAL, who + ": delay_unit and stay_unit must be in 1..65535");
    for (uint32_t i = 1; i < p->n_delay; ++i) if (p->delay_cdf[i] < p->delay_cdf[i - 1u]) return fail(c, ESIM_EINVAL, who + ": delay_cdf is not ascending");
    for (uint32_t i = 1; i < p->n_stay; ++i) if (p->stay_cdf[i] < p->stay_cdf[i - 1u]) return fail(c, ESIM_EINVAL, who + ": stay_cdf is not ascending");
    if (!c->uploaded) return fail(c, ESIM_ESTATE, who + ": no population uploaded");
    if (c->comm.world > 1 || c->d.n_global != c->d.n)
        return fail(c, ESIM_ESTATE, who + ": the context has a communicator of several ranks or holds a shard (sharded burden is not built)");
    if (p->n_groups != 1u && (!c->grp.lab || c->grp.n != p->n_groups))
        return fail(c, ESIM_ESTATE, who + ": tables of several groups need the labels of esim_set_groups with the same number of groups");
    HIP_TRY(c, hipSetDevice(c->P.device));
    const size_t g = p->n_groups, words = 2 * g + 2 * (size_t)ESIM_BURDEN_BINS;
    std::vector<uint32_t> host(words, 0xFFFFFFFFu);               // (CDF entries beyond the count are never read)
    std::copy(p->admit_thr, p->admit_thr + g, host.begin());
    std::copy(p->death_thr, p->death_thr + g, host.begin() + g);
    std::copy(p->delay_cdf, p->delay_cdf + p->n_delay, host.begin() + 2 * g);
    std::copy(p->stay_cdf, p->stay_cdf + p->n_stay, host.begin() + 2 * g + ESIM_BURDEN_BINS);
    uint32_t *tab = nullptr;
    if (int rc = dev_alloc(c, &tab, words)) { (void)hipGetLastError(); return rc; }
    const hipError_t e = hipMemcpy(tab, host.data(), sizeof(uint32_t) * words, hipMemcpyHostToDevice);
    if (e != hipSuccess) { dev_free(c, tab); return fail(c, ESIM_ENODEVICE, who + ": " + hipGetErrorString(e)); }
    burden_forget(c);                                             // (the tables replaced, behind whatever still reads them)
    BurdenState &b = c->burden;
    b.set = true; b.n_groups = p->n_groups; b.n_delay = p->n_delay; b.n_stay = p->n_stay; b.delay_unit = p->delay_unit; b.stay_unit = p->stay_unit;
    b.host.swap(host); b.tab = tab;
    return ESIM_OK;
}

extern "C" int esim_burden_drop(esim_ctx *ctx)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    if (c->uploaded) (void)hipSetDevice(c->P.device);
    burden_forget(c);
    return ESIM_OK;
}

extern "C" int esim_burden_get(esim_ctx *ctx, uint32_t *n_groups, uint32_t *admit_thr, uint32_t *death_thr, uint32_t *delay_unit, uint32_t *n_delay, uint32_t *delay_cdf,
                               uint32_t *stay_unit, uint32_t *n_stay, uint32_t *stay_cdf)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    const BurdenState &b = c->burden;
    if (!c->uploaded || !b.set) return fail(c, ESIM_ESTATE, "esim_burden_get: no population uploaded, or no severity tables in force (esim_burden_set)");
    const size_t g = b.n_groups;
    if (n_groups) *n_groups = b.n_groups;
    if (admit_thr) std::copy(b.host.begin(), b.host.begin() + g, admit_thr);
    if (death_thr) std::copy(b.host.begin() + g, b.host.begin() + 2 * g, death_thr);
    if (delay_unit) *delay_unit = b.delay_unit;
    if (n_delay) *n_delay = b.n_delay;
    if (delay_cdf) std::copy(b.host.begin() + 2 * g, b.host.begin() + 2 * g + b.n_delay, delay_cdf);
    if (stay_unit) *stay_unit = b.stay_unit;
    if (n_stay) *n_stay = b.n_stay;
    if (stay_cdf) std::copy(b.host.begin() + 2 * g + ESIM_BURDEN_BINS, b.host.begin() + 2 * g + ESIM_BURDEN_BINS + b.n_stay, stay_cdf);
    return ESIM_OK;
}

extern "C" int esim_burden_outcomes(esim_ctx *ctx, uint32_t *admit_step, uint32_t *end_step, uint8_t *died)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    const std::string who = "esim_burden_outcomes";
    if (int rc = burden_ready(c, who)) return rc;
    const size_t N = c->d.n;
    DevTmp<uint32_t> vax, d_admit, d_end; DevTmp<uint8_t> d_died;
    BurdenRun r;
    if (int rc = burden_run(c, who, &vax, &r)) return rc;
    if ((admit_step && d_admit.alloc(N) != hipSuccess) || (end_step && d_end.alloc(N) != hipSuccess) || (died && d_died.alloc(N) != hipSuccess)) {
        (void)hipGetLastError();
        return flows_unwind(c, fail(c, ESIM_ENOMEM, who + ": no device memory for the outcomes (9 B per citizen)"));
    }
    hipError_t e = hipSuccess;
    if (admit_step) e = hipMemsetAsync(d_admit.p, 0xFF, sizeof(uint32_t) * std::max<size_t>(1, N), c->stream);
    if (e == hipSuccess && end_step) e = hipMemsetAsync(d_end.p, 0xFF, sizeof(uint32_t) * std::max<size_t>(1, N), c->stream);
    if (e == hipSuccess && died) e = hipMemsetAsync(d_died.p, 0, std::max<size_t>(1, N), c->stream);
    if (e == hipSuccess) {
        const Series q = burden_query(c, ESIM_BY_ALL, 1u, r.t_done, r.t_all, r.replay ? vax.p : nullptr);
        hipLaunchKernelGGL(k_burden_outcomes, dim3(grid_capped(c, r.log_len, TPB, BURDEN_GRID)), dim3(TPB), 0, c->stream, c->d, q, burden_dev(c), r.log_len, d_admit.p, d_end.p, d_died.p);
        e = hipGetLastError();
    }
    const hipError_t es = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = es;
    if (e == hipSuccess && admit_step && N) e = hipMemcpy(admit_step, d_admit.p, sizeof(uint32_t) * N, hipMemcpyDeviceToHost);
    if (e == hipSuccess && end_step && N) e = hipMemcpy(end_step, d_end.p, sizeof(uint32_t) * N, hipMemcpyDeviceToHost);
    if (e == hipSuccess && died && N) e = hipMemcpy(died, d_died.p, N, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(c, ESIM_ENODEVICE, who + ": " + hipGetErrorString(e));
    return ESIM_OK;
}

extern "C" int esim_burden_series(esim_ctx *ctx, int where, int what, uint32_t first_step, uint32_t n_rows, uint32_t stride, uint32_t *out)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    const std::string who = "esim_burden_series";
    if (!out || what < ESIM_BURDEN_ADMISSIONS || what > ESIM_BURDEN_DEATHS || stride == 0 || n_rows == 0)
        return fail(c, ESIM_EINVAL, who + ": null output, unknown `what`, stride 0 or no rows");
    if (where != ESIM_BY_ALL && where != ESIM_AREA_HOME && where != ESIM_BY_GROUP) return fail(c, ESIM_EINVAL, who + BURDEN_WHERE);
    if (int rc = burden_ready(c, who)) return rc;
    if (where == ESIM_BY_GROUP && !c->grp.lab) return fail(c, ESIM_ESTATE, who + ": by group without labels (esim_set_groups)");
    if (first_step == 0 || (uint64_t)first_step + (uint64_t)(n_rows - 1u) * stride > c->host_t - 1u)
        return fail(c, ESIM_ERANGE, who + ": rows outside the steps run so far");
    DevTmp<uint32_t> vax, rows;
    BurdenRun r;
    if (int rc = burden_run(c, who, &vax, &r)) return rc;
    const uint32_t cols = curve_cols(c, where);
    const size_t words = (size_t)n_rows * cols;
    if (rows.alloc(words) != hipSuccess) { (void)hipGetLastError(); return flows_unwind(c, fail(c, ESIM_ENOMEM, who + ": no device memory for the rows (ask for fewer)")); }
    hipError_t e = hipMemsetAsync(rows.p, 0, sizeof(uint32_t) * std::max<size_t>(1, words), c->stream);
    if (e == hipSuccess) {
        Series q = burden_query(c, where, first_step, r.t_done, r.t_all, r.replay ? vax.p : nullptr);
        q.n_rows = n_rows; q.stride = stride; q.p0 = rows.p;
        hipLaunchKernelGGL(k_burden_rows, dim3(grid_capped(c, r.log_len, TPB, BURDEN_GRID)), dim3(TPB), 0, c->stream, c->d, q, burden_dev(c), (uint32_t)what, r.log_len);
        if (what == ESIM_BURDEN_OCCUPANCY)
            hipLaunchKernelGGL(k_series_prefix, dim3(grid_for(cols, TPB, 0xFFFFFFFFu)), dim3(TPB), 0, c->stream, q, nullptr, nullptr);
        e = hipGetLastError();
    }
    const hipError_t es = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = es;
    if (e == hipSuccess && words) e = hipMemcpy(out, rows.p, sizeof(uint32_t) * words, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(c, ESIM_ENODEVICE, who + ": " + hipGetErrorString(e));
    return ESIM_OK;
}

extern "C" int esim_burden_summary(esim_ctx *ctx, int where, uint32_t first_step, uint32_t last_step, uint32_t threshold, uint32_t *peak, uint32_t *peak_step,
                                   uint32_t *steps_at_least, uint32_t *first_at_least, uint32_t *last_at_least, uint64_t *bed_steps, uint32_t *admissions, uint32_t *deaths)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    const std::string who = "esim_burden_summary";
    const CurveSpec s = { where, CURVE_MASK_I, first_step, last_step, threshold };
    if (where != ESIM_BY_ALL && where != ESIM_AREA_HOME && where != ESIM_BY_GROUP) return fail(c, ESIM_EINVAL, who + BURDEN_WHERE);
    if (threshold == 0u) return fail(c, ESIM_EINVAL, who + ": threshold 0");
    if (int rc = burden_ready(c, who)) return rc;
    if (int rc = curve_check(c, who, s)) return rc;
    CurveWork w;
    BurdenCounts n;
    if (int rc = burden_enqueue(c, who, s, &w, &n)) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (int rc = pairs_end(c, who, &w.p)) return rc;
    const size_t cols = w.cols;
    std::vector<unsigned long long> wide(2 * cols);
    std::vector<uint32_t> words(3 * cols), counts(2 * cols);
    HIP_TRY(c, hipMemcpy(wide.data(), w.wide.p, sizeof(unsigned long long) * 2 * cols, hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(words.data(), w.words.p, sizeof(uint32_t) * 3 * cols, hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(counts.data(), n.tab.p, sizeof(uint32_t) * 2 * cols, hipMemcpyDeviceToHost));
    for (size_t k = 0; k < cols; ++k) {
        const uint32_t top = (uint32_t)(wide[k] >> 32), n_at = words[k];
        if (peak) peak[k] = top;
        if (peak_step) peak_step[k] = top ? ~(uint32_t)wide[k] : ESIM_NEVER;
        if (steps_at_least) steps_at_least[k] = n_at;
        if (first_at_least) first_at_least[k] = words[cols + k];
        if (last_at_least) last_at_least[k] = n_at ? words[2 * cols + k] : ESIM_NEVER;
        if (bed_steps) bed_steps[k] = wide[cols + k];
        if (admissions) admissions[k] = counts[k];
        if (deaths) deaths[k] = counts[cols + k];
    }
    return ESIM_OK;
}

extern "C" int esim_ensemble_begin_burden_peaks(esim_ctx *ctx, int where, uint32_t first_step, uint32_t last_step, uint32_t threshold, uint32_t min_peak)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    const std::string who = "esim_ensemble_begin_burden_peaks";
    if (min_peak == 0u) return fail(c, ESIM_EINVAL, who + ": min_peak 0");
    if (where != ESIM_BY_ALL && where != ESIM_AREA_HOME && where != ESIM_BY_GROUP) return fail(c, ESIM_EINVAL, who + BURDEN_WHERE);
    if (threshold == 0u) return fail(c, ESIM_EINVAL, who + ": threshold 0");
    const CurveSpec s = { where, CURVE_MASK_I, first_step, last_step, threshold };
    if (int rc = burden_ready(c, who)) return rc;
    if (int rc = curve_check(c, who, s)) return rc;
    return peaks_kind_begin(c, who, Ensemble::ENS_BURDEN_PEAKS, s, min_peak);
}
