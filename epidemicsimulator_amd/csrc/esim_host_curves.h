// esim_host_curves.h -- the shape of the epidemic curve per column: esim_curve_summary, and the peaks kind of the ensemble
// accumulators, esim_ensemble_begin_peaks / esim_ensemble_read_peaks with what esim_ensemble_fold does while it is in force
// (DESIGN 26).  The kernels: esim_kernels_curves.h around esim_curves.h; the pair engine: esim_host_flows.h; the run's shape and
// the vaccination replay: esim_host_outputs.h.  Everything a call computes lives in temporary device memory.
namespace {

// What a summary is taken of.
struct CurveSpec { int where; uint32_t mask, first, last, threshold; };

// One call's device memory: the replay, the pair engine, the tile aggregates and the per-column tables.
struct CurveWork {
    DevTmp<uint32_t> vax, agg, words;           // words: steps, first, last [cols] each
    DevTmp<unsigned long long> wide;            // best, person [cols] each
    PairWork p;
    CurveTabs t;
    uint32_t cols = 0;
};

const uint32_t CURVE_MASK_E = 1u << ESIM_EXPOSED, CURVE_MASK_I = 1u << ESIM_INFECTED;

// The arguments both entry points refuse alike; the window's end is checked by whoever knows the steps run.
int curve_check(esim_ctx_impl *c, const std::string &who, const CurveSpec &s)
{
    if (s.where != ESIM_BY_ALL && s.where != ESIM_AREA_HOME && s.where != ESIM_BY_GROUP)
        return fail(c, ESIM_EINVAL, who + ": `where` must be ESIM_BY_ALL, ESIM_AREA_HOME or ESIM_BY_GROUP (curves by the area stood in are not built)");
    if (s.mask != CURVE_MASK_E && s.mask != CURVE_MASK_I && s.mask != (CURVE_MASK_E | CURVE_MASK_I))
        return fail(c, ESIM_EINVAL, who + ": the status mask must be Exposed, Infected or both (the other statuses are monotone)");
    if (s.threshold == 0u) return fail(c, ESIM_EINVAL, who + ": threshold 0");
    if (!c->uploaded) return fail(c, ESIM_ESTATE, who + ": no population uploaded");
    if (c->comm.world > 1 || c->d.n_global != c->d.n)
        return fail(c, ESIM_ESTATE, who + ": the context has a communicator of several ranks or holds a shard (sharded curves are not built)");
    if (s.where == ESIM_BY_GROUP && !c->grp.lab) return fail(c, ESIM_ESTATE, who + ": by group without labels (esim_set_groups)");
    if (s.first == 0u || s.last < s.first) return fail(c, ESIM_ERANGE, who + ": first_step is 1-based, and last_step may not lie before it");
    return ESIM_OK;
}

// What puts a curve's change points into the pair table between pairs_begin and pairs_sorted: nullptr for the status curves of
// k_curve_events, or another family's enqueuer with its own launch (esim_host_burden.h).  q: as k_curve_events reads it.
typedef void (*CurveEvents)(esim_ctx_impl *c, const Series &q, uint32_t last, uint32_t log_len, const PairTable &t, void *user);

uint32_t curve_cols(const esim_ctx_impl *c, int where) { return where == ESIM_BY_ALL ? 1u : where == ESIM_BY_GROUP ? c->grp.n : c->d.n_areas; }

// The summary of the run as it stands into w->t, on the context's stream: the change points of every case's interval into the
// pair table, compacted and sorted by (column, step), scanned per column and reduced.  The stream is waited for twice on the
// way -- for the control block and the records, and for the number of distinct change points -- and not behind the reduction:
// the caller waits.  A failure behind the first launch waits for the stream (flows_unwind): the kernels use the work struct's memory.
int curve_enqueue(esim_ctx_impl *c, const std::string &who, const CurveSpec &s, CurveWork *w, CurveEvents events = nullptr, void *user = nullptr)
{
    const uint32_t t_done = c->host_t - 1u;
    if (s.last > t_done) return fail(c, ESIM_ERANGE, who + ": last_step lies beyond the steps run so far");
    HIP_TRY(c, hipSetDevice(c->P.device));
    const Dev &d = c->d;
    Ctrl h; int rc;
    if ((rc = read_ctrl(c, &h)) || (rc = ctrl_error(c, h))) return rc;
    RunShape shape;
    if ((rc = run_shape(c, t_done, &shape))) return rc;
    const bool replay = shape.trigger != 0u;
    const uint32_t log_len = std::min<uint32_t>(h.log_len, d.n), cols = curve_cols(c, s.where);
    w->cols = cols;
    if ((replay && w->vax.alloc(d.n) != hipSuccess) || w->wide.alloc(2 * (size_t)cols) != hipSuccess || w->words.alloc(3 * (size_t)cols) != hipSuccess) {
        (void)hipGetLastError();
        return fail(c, ESIM_ENOMEM, who + ": no device memory for the vaccination replay (4 B per citizen) and the tables (28 B per column)");
    }
    uint32_t *vax = w->vax.p;
    w->t.best = w->wide.p; w->t.person = w->wide.p + cols;
    w->t.steps = w->words.p; w->t.first = w->words.p + cols; w->t.last = w->words.p + 2 * (size_t)cols;
    if ((rc = pairs_begin(c, who, &w->p, (uint32_t)std::min<uint64_t>(2ull * log_len, 0xFFFFFFFFull)))) return rc;   // (two change points a case; beyond 2^30 it refuses)
    hipError_t e = hipMemsetAsync(w->wide.p, 0, sizeof(unsigned long long) * 2 * (size_t)cols, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(w->words.p, 0, sizeof(uint32_t) * 3 * (size_t)cols, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(w->t.first, 0xFF, sizeof(uint32_t) * (size_t)cols, c->stream);
    if (e == hipSuccess && replay) e = enqueue_vax_replay(c, shape.trigger, t_done, vax);
    if (e != hipSuccess) return flows_unwind(c, fail(c, ESIM_ENODEVICE, who + ": " + hipGetErrorString(e)));
    Series q = Series();
    q.first = s.first; q.t_done = t_done; q.t_all = shape.t_all; q.vax_of = replay ? vax : nullptr; q.n_cols = cols;
    q.key = s.where == ESIM_BY_ALL ? CURVE_BY_ALL : s.where == ESIM_BY_GROUP ? (uint32_t)KEY_GROUP : (uint32_t)KEY_HOME;
    q.grp = s.where == ESIM_BY_GROUP ? c->grp.lab : nullptr;
    if (events) events(c, q, s.last, log_len, w->p.t, user);
    else hipLaunchKernelGGL(k_curve_events, dim3(grid_capped(c, log_len, TPB, 4096)), dim3(TPB), 0, c->stream, d, q, s.mask, s.last, log_len, w->p.t);
    if ((rc = pairs_sorted(c, &w->p))) return flows_unwind(c, rc);
    if (w->p.dropped) {                                                      // (ESIM_PAIR_LOG2 too small: nothing is reduced)
        (void)hipStreamSynchronize(c->stream);
        return pairs_end(c, who, &w->p);
    }
    const uint32_t n = w->p.n;
    if (w->agg.alloc(3 * (size_t)curve_tiles(n)) != hipSuccess) {
        (void)hipGetLastError();
        return flows_unwind(c, fail(c, ESIM_ENOMEM, who + ": no device memory for the tile aggregates of the scan"));
    }
    curve_scan_enqueue(w->p.out_key.p, w->p.out_cnt.p, n, w->agg.p, c->stream);
    if (n) curve_reduce_enqueue(w->p.out_key.p, w->p.out_cnt.p, n, cols, s.last, s.threshold, w->t, c->stream, grid_capped(c, n, 256u, CURVE_REDUCE_GRID));
    if ((e = hipGetLastError()) != hipSuccess) return flows_unwind(c, fail(c, ESIM_ENODEVICE, who + ": " + hipGetErrorString(e)));
    return ESIM_OK;
}

}  // namespace

extern "C" int esim_curve_summary(esim_ctx *ctx, int where, uint32_t status_mask, uint32_t first_step, uint32_t last_step, uint32_t threshold,
                                  uint32_t *peak, uint32_t *peak_step, uint32_t *steps_at_least, uint32_t *first_at_least, uint32_t *last_at_least, uint64_t *person_steps)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    const std::string who = "esim_curve_summary";
    const CurveSpec s = { where, status_mask, first_step, last_step, threshold };
    if (int rc = curve_check(c, who, s)) return rc;
    CurveWork w;
    if (int rc = curve_enqueue(c, who, s, &w)) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (int rc = pairs_end(c, who, &w.p)) return rc;
    const size_t cols = w.cols;
    std::vector<unsigned long long> wide(2 * cols);
    std::vector<uint32_t> words(3 * cols);
    HIP_TRY(c, hipMemcpy(wide.data(), w.wide.p, sizeof(unsigned long long) * 2 * cols, hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(words.data(), w.words.p, sizeof(uint32_t) * 3 * cols, hipMemcpyDeviceToHost));
    for (size_t k = 0; k < cols; ++k) {
        const uint32_t top = (uint32_t)(wide[k] >> 32), n_at = words[k];
        if (peak) peak[k] = top;
        if (peak_step) peak_step[k] = top ? ~(uint32_t)wide[k] : ESIM_NEVER;
        if (steps_at_least) steps_at_least[k] = n_at;
        if (first_at_least) first_at_least[k] = words[cols + k];
        if (last_at_least) last_at_least[k] = n_at ? words[2 * cols + k] : ESIM_NEVER;
        if (person_steps) person_steps[k] = wide[cols + k];
    }
    return ESIM_OK;
}

namespace {
// Behind curve_enqueue: the member's tables in w folded into the accumulators, kept where members are kept, and the wait.
int fold_peaks_tables(esim_ctx_impl *c, const std::string &who, CurveWork &w)
{
    const Rows &r = c->ens.rows;
    PeakAcc a;
    a.defined = r.defined; a.hit = r.hit; a.members = r.members;
    a.sum_peak = r.sum; a.sq_peak = r.sumsq; a.sum_step = r.sum_o; a.sq_step = r.sumsq_o; a.sum_dur = r.sum_d; a.sq_dur = r.sumsq_d;
    hipLaunchKernelGGL(k_ensemble_fold_peaks, dim3(grid_capped(c, r.n_cols, TPB, 2048)), dim3(TPB), 0, c->stream, w.t, r.n_cols, c->ens.par.min_hit, a);
    hipError_t e = members_keep(c, &w.t);
    if (e == hipSuccess) e = hipGetLastError();
    const hipError_t es = hipStreamSynchronize(c->stream);                   // (the temporary tables go when the call returns)
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return fail(c, ESIM_ENODEVICE, who + ": " + hipGetErrorString(e));
    return pairs_end(c, who, &w.p);
}

// One member folded into the accumulators of the peaks kind: its summary in temporary memory, the fold kernel, the wait.
int fold_peaks(esim_ctx_impl *c)
{
    const Ensemble::Par &par = c->ens.par;
    const std::string who = "esim_ensemble_fold";
    const CurveSpec s = { c->ens.where, par.status_mask, par.first, par.last, par.threshold };
    if (int rc = curve_check(c, who, s)) return rc;
    if (curve_cols(c, s.where) != c->ens.rows.n_cols) return fail(c, ESIM_ESTATE, who + ": the accumulators were begun for other columns");
    CurveWork w;
    if (int rc = curve_enqueue(c, who, s, &w)) return rc;
    return fold_peaks_tables(c, who, w);
}

// The begin of the two peaks kinds behind their callers' checks: one row of columns; a fold of `kind` summarises the status curve
// of the mask, or the occupancy curve of esim_burden_summary (esim_host_burden.h).
int peaks_kind_begin(esim_ctx_impl *c, const std::string &who, Ensemble::Kind kind, const CurveSpec &s, uint32_t min_peak)
{
    HIP_TRY(c, hipSetDevice(c->P.device));
    Ensemble::Par par;
    par.status_mask = s.mask; par.first = s.first; par.last = s.last; par.threshold = s.threshold; par.min_hit = min_peak;
    return ens_begin(c, who, kind, s.where, 1u, curve_cols(c, s.where), par);
}
}  // namespace

extern "C" int esim_ensemble_begin_peaks(esim_ctx *ctx, int where, uint32_t status_mask, uint32_t first_step, uint32_t last_step, uint32_t threshold, uint32_t min_peak)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    const std::string who = "esim_ensemble_begin_peaks";
    if (min_peak == 0u) return fail(c, ESIM_EINVAL, who + ": min_peak 0");
    const CurveSpec s = { where, status_mask, first_step, last_step, threshold };
    if (int rc = curve_check(c, who, s)) return rc;
    return peaks_kind_begin(c, who, Ensemble::ENS_PEAKS, s, min_peak);
}

extern "C" int esim_ensemble_read_peaks(esim_ctx *ctx, uint32_t *members, uint32_t *defined, uint32_t *hit, uint64_t *sum_peak, uint64_t *sumsq_peak,
                                        uint64_t *sum_step, uint64_t *sumsq_step, uint64_t *sum_duration, uint64_t *sumsq_duration)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    return ens_read(c, READ_PEAKS, 0u, 1u, members, { { defined, &Rows::defined }, { hit, &Rows::hit } },
                    { { sum_peak, &Rows::sum }, { sumsq_peak, &Rows::sumsq }, { sum_step, &Rows::sum_o }, { sumsq_step, &Rows::sumsq_o }, { sum_duration, &Rows::sum_d },
                      { sumsq_duration, &Rows::sumsq_d } });
}
