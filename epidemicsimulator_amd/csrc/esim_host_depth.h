// esim_host_depth.h -- curve-based ensemble statistics over the store of esim_ensemble_keep_members:
// esim_ensemble_depth, the modified band depth of every kept member per column over a window of rows, and esim_ensemble_band,
// the envelope of the most central members and the deepest member's curve.  The kernels: esim_depth.h.  The checks, the cells
// the accumulators settle and the tail of both calls are those of esim_host_members.h.
namespace {

// What both calls hold on the device: depth [kept * n_cols] with trivial [n_cols] behind it, and total [kept].
struct DepthTabs {
    DevTmp<uint32_t> depth;
    DevTmp<unsigned long long> total;
    uint32_t *trivial = nullptr;
};

// The window's rows checked and the tables filled on the context's stream; no wait.
int depth_tables(esim_ctx_impl *c, const std::string &who, uint32_t first_row, uint32_t n_rows, DepthTabs *t)
{
    if (int rc = members_read_check(c, who, first_row, n_rows)) return rc;
    const Ensemble::Store &s = c->ens.store;
    if (!depth_fits(n_rows, s.kept)) return fail(c, ESIM_ERANGE, who + ": rows x C(members kept, 2) does not fit 32 bits");
    HIP_TRY(c, hipSetDevice(c->P.device));
    const size_t plane = (size_t)s.n_rows * s.n_cols, at = (size_t)first_row * s.n_cols, cells = (size_t)n_rows * s.n_cols, table = (size_t)s.kept * s.n_cols;
    if (t->depth.alloc(table + s.n_cols) != hipSuccess || t->total.alloc(s.kept) != hipSuccess) {
        (void)hipGetLastError();
        return fail(c, ESIM_ENOMEM, who + ": no device memory for the depth table");
    }
    t->trivial = t->depth.p + table;
    HIP_TRY(c, hipMemsetAsync(t->depth.p, 0, sizeof(uint32_t) * (table + s.n_cols), c->stream));
    HIP_TRY(c, hipMemsetAsync(t->total.p, 0, sizeof(unsigned long long) * s.kept, c->stream));
    depth_count_enqueue(s.planes, plane, s.kept, at, cells, s.n_cols, members_skip(c), t->depth.p, t->trivial, c->stream,
                        grid_capped(c, cells, depth_count_per_block(s.kept), MEMBERS_GRID));
    depth_total_enqueue(t->depth.p, t->trivial, s.kept, s.n_cols, t->total.p, c->stream, grid_capped(c, depth_tiles(s.kept, s.n_cols), 1, MEMBERS_GRID));
    return ESIM_OK;
}

}  // namespace

extern "C" int esim_ensemble_depth(esim_ctx *ctx, uint32_t first_row, uint32_t n_rows, uint32_t *depth, uint64_t *total)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    const std::string who = "esim_ensemble_depth";
    DepthTabs t;
    if (int rc = depth_tables(c, who, first_row, n_rows, &t)) return rc;
    const Ensemble::Store &s = c->ens.store;
    if (int rc = members_deliver(c, who, t.depth.p, depth ? (size_t)s.kept * s.n_cols : 0u, false, depth)) return rc;
    return members_deliver(c, who, (const uint32_t *)t.total.p, total ? 2u * (size_t)s.kept : 0u, false, (uint32_t *)total);
}

extern "C" int esim_ensemble_band(esim_ctx *ctx, uint32_t first_row, uint32_t n_rows, uint32_t need, int pooled, uint32_t *lo, uint32_t *hi, uint32_t *median,
                                  uint32_t *deepest, uint32_t *n_in)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    const std::string who = "esim_ensemble_band";
    if (pooled != 0 && pooled != 1) return fail(c, ESIM_EINVAL, who + ": pooled must be 0 or 1");
    if (int rc = members_read_check(c, who, first_row, n_rows)) return rc;
    const Ensemble::Store &s = c->ens.store;
    if (need == 0u || need > s.kept) return fail(c, ESIM_ERANGE, who + ": need is not in 1..the members kept");
    DepthTabs t;
    if (int rc = depth_tables(c, who, first_row, n_rows, &t)) return rc;
    const size_t plane = (size_t)s.n_rows * s.n_cols, at = (size_t)first_row * s.n_cols, cells = (size_t)n_rows * s.n_cols;
    const bool planes = lo || hi || median;
    // thr, deepest, n_in [n_cols] each, then the planes asked for
    DevTmp<uint32_t> d_out;
    if (d_out.alloc(3u * (size_t)s.n_cols + (planes ? 3u * cells : 0u)) != hipSuccess) { (void)hipGetLastError(); return fail(c, ESIM_ENOMEM, who + ": no device memory for the output"); }
    uint32_t *d_thr = d_out.p, *d_deepest = d_thr + s.n_cols, *d_n_in = d_deepest + s.n_cols, *d_lo = d_n_in + s.n_cols, *d_hi = d_lo + cells, *d_median = d_hi + cells;
    DepthPool pool = DepthPool();
    uint32_t pool_in = 0u;
    if (pooled) {                                                   // one set of members for every column: ranked here, from the totals
        std::vector<uint64_t> totals(s.kept);
        if (int rc = members_deliver(c, who, (const uint32_t *)t.total.p, 2u * (size_t)s.kept, false, (uint32_t *)totals.data())) return rc;
        pool = depth_pool(totals.data(), s.kept, need, &pool_in);
    } else if (s.n_cols) {
        MemberRanks r = MemberRanks();
        r.n = 1u; r.r[0] = s.kept - need;                           // the need-th largest of the column's depths
        const MemberSkip none = { nullptr, 0u, nullptr };
        members_select_enqueue(t.depth.p, s.n_cols, s.kept, 0u, s.n_cols, none, r, d_thr, s.n_cols, c->stream, grid_capped(c, s.n_cols, members_select_per_block(s.kept), MEMBERS_GRID));
        depth_pick_enqueue(t.depth.p, s.kept, s.n_cols, d_thr, d_deepest, d_n_in, c->stream, grid_capped(c, s.n_cols, MEMBERS_TPB, MEMBERS_GRID));
    }
    if (planes)
        depth_band_enqueue(s.planes, plane, s.kept, at, cells, s.n_cols, members_skip(c), t.depth.p, d_thr, d_deepest, pool, lo ? d_lo : nullptr, hi ? d_hi : nullptr,
                           median ? d_median : nullptr, c->stream, grid_capped(c, cells, MEMBERS_TPB, MEMBERS_GRID));
    if (int rc = members_deliver(c, who, d_lo, lo ? cells : 0u, s.is_signed, lo)) return rc;
    if (int rc = members_deliver(c, who, d_hi, hi ? cells : 0u, s.is_signed, hi)) return rc;
    if (int rc = members_deliver(c, who, d_median, median ? cells : 0u, s.is_signed, median)) return rc;
    if (pooled) {
        for (uint32_t col = 0u; col < s.n_cols; ++col) {
            if (deepest) deepest[col] = pool.deepest;
            if (n_in) n_in[col] = pool_in;
        }
        return ESIM_OK;
    }
    if (int rc = members_deliver(c, who, d_deepest, deepest ? s.n_cols : 0u, false, deepest)) return rc;
    return members_deliver(c, who, d_n_in, n_in ? s.n_cols : 0u, false, n_in);
}
