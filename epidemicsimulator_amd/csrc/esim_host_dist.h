// esim_host_dist.h -- ensemble distances over the store of esim_ensemble_keep_members: esim_ensemble_distances, the
// members kept compared pair by pair over a window of rows, and esim_ensemble_distances_info, what the kernel of the last call
// did.  The kernels: esim_dist.h.  The checks and the cells the accumulators settle are those of esim_host_members.h.
extern "C" int esim_ensemble_distances(esim_ctx *ctx, uint32_t first_row, uint32_t n_rows, int metric, uint32_t never_as, uint64_t *out, uint64_t *live_cells)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    const std::string who = "esim_ensemble_distances";
    if (metric != ESIM_DIST_L1 && metric != ESIM_DIST_DIFFER) return fail(c, ESIM_EINVAL, who + ": metric must be ESIM_DIST_L1 or ESIM_DIST_DIFFER");
    if (int rc = members_read_check(c, who, first_row, n_rows)) return rc;
    const Ensemble::Store &s = c->ens.store;
    HIP_TRY(c, hipSetDevice(c->P.device));
    const size_t plane = (size_t)s.n_rows * s.n_cols, at = (size_t)first_row * s.n_cols, cells = (size_t)n_rows * s.n_cols, matrix = (size_t)s.kept * s.kept;
    DevTmp<unsigned long long> d_out;                               // the matrix, the kernel's counts behind it
    if (d_out.alloc(matrix + DIST_STATS) != hipSuccess) { (void)hipGetLastError(); return fail(c, ESIM_ENOMEM, who + ": no device memory for the matrix"); }
    HIP_TRY(c, hipMemsetAsync(d_out.p, 0, sizeof(unsigned long long) * (matrix + DIST_STATS), c->stream));
    const uint32_t grid = grid_capped(c, dist_items(s.kept, cells), 1, DIST_GRID);
    const uint32_t grid_mirror = grid_capped(c, matrix, DIST_TPB, DIST_GRID);
    dist_enqueue(s.planes, plane, s.kept, at, cells, members_skip(c), metric, s.has_never ? never_as : MEMBERS_NEVER, d_out.p, d_out.p + matrix, c->stream, grid, grid_mirror);
    uint64_t stats[DIST_STATS];
    if (int rc = members_deliver(c, who, (const uint32_t *)(d_out.p + matrix), 2u * DIST_STATS, false, (uint32_t *)stats)) return rc;
    if (int rc = members_deliver(c, who, (const uint32_t *)d_out.p, out ? 2u * matrix : 0u, false, (uint32_t *)out)) return rc;
    for (uint32_t k = 0u; k < DIST_STATS; ++k) c->ens.dist_stats[k] = stats[k];
    if (live_cells) *live_cells = stats[0];
    return ESIM_OK;
}

extern "C" int esim_ensemble_distances_info(esim_ctx *ctx, uint64_t *tiles, uint64_t *tiles_32bit, uint64_t *tiles_partial)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    if (tiles) *tiles = c->ens.dist_stats[1];
    if (tiles_32bit) *tiles_32bit = c->ens.dist_stats[2];
    if (tiles_partial) *tiles_partial = c->ens.dist_stats[3];
    return ESIM_OK;
}
