// esim_host_members.h -- ensemble quantile maps: esim_ensemble_keep_members and the store of the members' values
// beside the accumulators in force; what the folds of every kind call to fill it (members_full in front, members_keep behind
// the fold kernel) and the begins to end it (members_end); esim_ensemble_members_info, esim_ensemble_read_members,
// esim_ensemble_quantiles and esim_ensemble_exceedance.  The kernels: esim_kernels_members.h around esim_members.h.
namespace {

// A begin of any kind succeeded: keeping ends, and no member has been folded since.
void members_end(esim_ctx_impl *c)
{
    dev_free(c, c->ens.store.planes);            // (hipFree waits for whatever still writes it)
    c->ens.store = Ensemble::Store();
    c->ens.folds = 0u;
}

// In front of a fold, on the host, before anything is enqueued: a store that is full refuses the member.
int members_full(esim_ctx_impl *c)
{
    const Ensemble::Store &s = c->ens.store;
    if (s.planes && s.kept >= s.capacity)
        return fail(c, ESIM_ERANGE, "esim_ensemble_fold: the store of esim_ensemble_keep_members is full (" + std::to_string(s.capacity) + " members); nothing was folded");
    return ESIM_OK;
}

// Behind the fold kernel of a member, on the context's stream: the member's value per cell into the next slot -- one launch, or
// for the series and the settings kind one device-to-device copy of plane 0.  No wait.  Without a store this counts the fold
// and returns.  t: the peaks kind's tables of the member.
hipError_t members_keep(esim_ctx_impl *c, const CurveTabs *t = nullptr)
{
    Ensemble &e = c->ens;
    Ensemble::Store &s = e.store;
    e.folds += 1u;
    if (!s.planes) return hipSuccess;
    const size_t cells = (size_t)s.n_rows * s.n_cols;
    uint32_t *slot = s.planes + (size_t)s.kept * cells;
    s.kept += 1u;
    if (!cells) return hipSuccess;
    const Rows &r = e.rows;
    switch (e.kind) {
    case Ensemble::ENS_CENSUS: case Ensemble::ENS_ARRIVAL: {
        const uint32_t grid = grid_capped(c, cells, TPB, 2048);
        if (e.kind == Ensemble::ENS_ARRIVAL) hipLaunchKernelGGL(k_members_keep_arrival, dim3(grid), dim3(TPB), 0, c->stream, c->arrival, e.n, e.par.horizon, slot);
        else hipLaunchKernelGGL(k_members_keep_census, dim3(grid), dim3(TPB), 0, c->stream, e.where == ESIM_BY_GROUP ? c->grp.cnt : c->area_cnt, e.n, e.par.status_mask, slot);
        return hipGetLastError();
    }
    case Ensemble::ENS_PAIRED: case Ensemble::ENS_BURDEN_PAIRED:
        hipLaunchKernelGGL(k_members_keep_paired, dim3(grid_capped(c, cells, TPB, 2048)), dim3(TPB), 0, c->stream, r.p0, r.p1, (uint64_t)cells, slot);
        return hipGetLastError();
    case Ensemble::ENS_PEAKS: case Ensemble::ENS_BURDEN_PEAKS:
        hipLaunchKernelGGL(k_members_keep_peaks, dim3(grid_capped(c, cells, TPB, 2048)), dim3(TPB), 0, c->stream, *t, r.n_cols, s.what, slot);
        return hipGetLastError();
    default:                                     // (the series, the settings and the burden-series kind: plane 0 as it is)
        return hipMemcpyAsync(slot, r.p0, sizeof(uint32_t) * cells, hipMemcpyDeviceToDevice, c->stream);
    }
}

// What the three reads refuse alike: no store or nothing kept, rows outside it.
int members_read_check(esim_ctx_impl *c, const std::string &who, uint32_t first_row, uint32_t n_rows)
{
    const Ensemble::Store &s = c->ens.store;
    if (!c->uploaded || !c->ens.valid || !s.planes)
        return fail(c, ESIM_ESTATE, who + ": no members are kept (esim_ensemble_keep_members behind the begin in force; by group, since esim_set_groups)");
    if (!s.kept) return fail(c, ESIM_ESTATE, who + ": no member has been folded into the store yet");
    if ((uint64_t)first_row + n_rows > s.n_rows) return fail(c, ESIM_ERANGE, who + ": rows outside the store");
    return ESIM_OK;
}

// The cells the accumulators in force settle without a look at the planes (esim_members.h).  The store holds exactly the
// members the accumulators hold: it was opened in front of the first fold, and a full store refuses the fold.
MemberSkip members_skip(const esim_ctx_impl *c)
{
    const Ensemble &e = c->ens;
    MemberSkip k = { nullptr, 0u, nullptr };
    const Rows &r = e.rows;
    switch (e.kind) {
    case Ensemble::ENS_ARRIVAL: k.never = r.hit; break;
    case Ensemble::ENS_CENSUS: case Ensemble::ENS_SERIES: case Ensemble::ENS_SETTINGS: case Ensemble::ENS_BURDEN_SERIES: k.zero = r.sum; break;
    case Ensemble::ENS_PEAKS: case Ensemble::ENS_BURDEN_PEAKS:
        if (e.store.what == ESIM_KEEP_PEAK_STEP) k.never = r.defined;
        else k.zero = e.store.what == ESIM_KEEP_DURATION ? r.sum_d : r.sum;
        break;
    default: break;                              // (a difference of 0 says nothing about the sums of the paired kinds)
    }
    return k;
}

// The tail of the two calls that compute: the wait, n * cells words back, signed kinds as the numbers they are.
int members_deliver(esim_ctx_impl *c, const std::string &who, const uint32_t *dev, size_t words, bool unkey, uint32_t *out)
{
    hipError_t e = hipGetLastError();
    const hipError_t es = hipStreamSynchronize(c->stream);          // (the temporary output goes when the call returns)
    if (e == hipSuccess) e = es;
    if (e == hipSuccess && words) e = hipMemcpy(out, dev, sizeof(uint32_t) * words, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(c, ESIM_ENODEVICE, who + ": " + hipGetErrorString(e));
    if (unkey) for (size_t i = 0; i < words; ++i) out[i] = (uint32_t)members_unkey(out[i]);
    return ESIM_OK;
}

}  // namespace

extern "C" int esim_ensemble_keep_members(esim_ctx *ctx, uint32_t capacity, int what)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    const std::string who = "esim_ensemble_keep_members";
    if (capacity == 0u || capacity > (uint32_t)ESIM_MEMBERS_MAX || what < ESIM_KEEP_VALUE || what > ESIM_KEEP_DURATION)
        return fail(c, ESIM_EINVAL, who + ": capacity must be in 1..ESIM_MEMBERS_MAX (256), `what` one of ESIM_KEEP_*");
    Ensemble &e = c->ens;
    const int keep = ENS_KIND[e.kind].keep;
    if (!c->uploaded || !e.valid || e.kind == Ensemble::ENS_NONE)
        return fail(c, ESIM_ESTATE, who + ": no population uploaded, or no begin in force since the upload (or, by group, since esim_set_groups)");
    if (keep == KEEP_NONE) return fail(c, ESIM_ESTATE, who + ": the reproduction kind is in force (a ratio per cell is not kept)");
    if (e.folds) return fail(c, ESIM_ESTATE, who + ": a member has been folded since the begin (keep in front of the first fold)");
    if (what != ESIM_KEEP_VALUE && keep != KEEP_SUMMARY) return fail(c, ESIM_EINVAL, who + ": only the peaks kind has a `what` beside ESIM_KEEP_VALUE");
    HIP_TRY(c, hipSetDevice(c->P.device));
    Ensemble::Store s;
    s.capacity = capacity; s.what = what; s.n_rows = e.rows.n_rows; s.n_cols = e.rows.n_cols;
    s.is_signed = keep == KEEP_SIGNED;
    s.has_never = keep == KEEP_NEVER || (keep == KEEP_SUMMARY && what == ESIM_KEEP_PEAK_STEP);
    const size_t cells = (size_t)s.n_rows * s.n_cols;
    if (dev_alloc(c, &s.planes, (size_t)capacity * cells)) {
        (void)hipGetLastError();
        return fail(c, ESIM_ENOMEM, who + ": no device memory for the store (capacity x rows x columns x 4 B)");
    }
    dev_free(c, e.store.planes);                 // (an earlier store of this begin, which holds nothing)
    e.store = s;
    return ESIM_OK;
}

extern "C" int esim_ensemble_members_info(esim_ctx *ctx, uint32_t *capacity, uint32_t *kept, int *what, int *is_signed)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    const Ensemble::Store &s = c->ens.store;
    if (!c->uploaded || !c->ens.valid || !s.planes) return fail(c, ESIM_ESTATE, "esim_ensemble_members_info: no members are kept (esim_ensemble_keep_members)");
    if (capacity) *capacity = s.capacity;
    if (kept) *kept = s.kept;
    if (what) *what = s.what;
    if (is_signed) *is_signed = s.is_signed ? 1 : 0;
    return ESIM_OK;
}

extern "C" int esim_ensemble_read_members(esim_ctx *ctx, uint32_t first_member, uint32_t n_members, uint32_t first_row, uint32_t n_rows, uint32_t *out)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    const std::string who = "esim_ensemble_read_members";
    if (!out) return fail(c, ESIM_EINVAL, who + ": null output");
    if (int rc = members_read_check(c, who, first_row, n_rows)) return rc;
    const Ensemble::Store &s = c->ens.store;
    if ((uint64_t)first_member + n_members > s.kept) return fail(c, ESIM_ERANGE, who + ": members outside those kept");
    HIP_TRY(c, hipSetDevice(c->P.device));
    Ctrl h; int rc;
    if ((rc = read_ctrl(c, &h))) return rc;                        // (the wait for the folds enqueued so far)
    const size_t plane = (size_t)s.n_rows * s.n_cols, at = (size_t)first_row * s.n_cols, words = (size_t)n_rows * s.n_cols;
    for (uint32_t m = 0; m < n_members && words; ++m)
        HIP_TRY(c, hipMemcpy(out + (size_t)m * words, s.planes + (size_t)(first_member + m) * plane + at, sizeof(uint32_t) * words, hipMemcpyDeviceToHost));
    if (s.is_signed) for (size_t i = 0; i < (size_t)n_members * words; ++i) out[i] = (uint32_t)members_unkey(out[i]);
    return ctrl_error(c, h);
}

extern "C" int esim_ensemble_quantiles(esim_ctx *ctx, uint32_t first_row, uint32_t n_rows, const uint32_t *ranks, uint32_t n_ranks, uint32_t *out)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    const std::string who = "esim_ensemble_quantiles";
    if (!out || !ranks || n_ranks == 0u || n_ranks > (uint32_t)ESIM_RANKS_MAX) return fail(c, ESIM_EINVAL, who + ": null output or ranks, no ranks or more than ESIM_RANKS_MAX (16)");
    if (int rc = members_read_check(c, who, first_row, n_rows)) return rc;
    const Ensemble::Store &s = c->ens.store;
    MemberRanks r; bool bad_rank;
    if (!members_rank_list(ranks, n_ranks, s.kept, &r, &bad_rank)) return fail(c, ESIM_ERANGE, who + ": a rank is not below the members kept");
    HIP_TRY(c, hipSetDevice(c->P.device));
    const size_t plane = (size_t)s.n_rows * s.n_cols, at = (size_t)first_row * s.n_cols, cells = (size_t)n_rows * s.n_cols;
    DevTmp<uint32_t> d_out;
    if (d_out.alloc(cells * n_ranks) != hipSuccess) { (void)hipGetLastError(); return fail(c, ESIM_ENOMEM, who + ": no device memory for the output"); }
    members_select_enqueue(s.planes, plane, s.kept, at, cells, members_skip(c), r, d_out.p, cells, c->stream,
                           grid_capped(c, cells, members_select_per_block(s.kept), MEMBERS_GRID));
    return members_deliver(c, who, d_out.p, cells * n_ranks, s.is_signed, out);
}

extern "C" int esim_ensemble_exceedance(esim_ctx *ctx, uint32_t first_row, uint32_t n_rows, const int64_t *thresholds, uint32_t n_thresholds, uint32_t *out)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    const std::string who = "esim_ensemble_exceedance";
    if (!out || !thresholds || n_thresholds == 0u || n_thresholds > (uint32_t)ESIM_RANKS_MAX)
        return fail(c, ESIM_EINVAL, who + ": null output or thresholds, no thresholds or more than ESIM_RANKS_MAX (16)");
    if (int rc = members_read_check(c, who, first_row, n_rows)) return rc;
    const Ensemble::Store &s = c->ens.store;
    HIP_TRY(c, hipSetDevice(c->P.device));
    const size_t plane = (size_t)s.n_rows * s.n_cols, at = (size_t)first_row * s.n_cols, cells = (size_t)n_rows * s.n_cols;
    DevTmp<uint32_t> d_out;
    if (d_out.alloc(cells * n_thresholds) != hipSuccess) { (void)hipGetLastError(); return fail(c, ESIM_ENOMEM, who + ": no device memory for the output"); }
    members_exceed_enqueue(s.planes, plane, s.kept, at, cells, members_skip(c), members_threshold_keys(thresholds, n_thresholds, s.is_signed, s.has_never),
                           d_out.p, cells, c->stream, grid_capped(c, cells, MEMBERS_TPB, MEMBERS_GRID));
    return members_deliver(c, who, d_out.p, cells * n_thresholds, false, out);
}
