// esim_host_arms.h -- policy grids over the store of esim_ensemble_keep_members: esim_ensemble_arms, the members kept
// read as replicates of arms run on common random numbers (slot = replicate * n_arms + arm) -- per cell and arm the replicates
// in which the arm is best, in which it alone is, its regret against the best arm of the same replicate and its sum, and per
// member the sum over the window.  The kernel: esim_arms.h.  The checks, the cells the accumulators settle and the tail of the
// call are those of esim_host_members.h.
extern "C" int esim_ensemble_arms(esim_ctx *ctx, uint32_t n_arms, int maximize, uint32_t never_as, uint32_t first_row, uint32_t n_rows, uint32_t *best, uint32_t *sole,
                                  uint64_t *regret, uint64_t *sum, uint64_t *totals, uint64_t *live_cells)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    const std::string who = "esim_ensemble_arms";
    if (n_arms == 0u || n_arms > (uint32_t)ESIM_ARMS_MAX) return fail(c, ESIM_EINVAL, who + ": n_arms must be in 1..ESIM_ARMS_MAX (16)");
    if (maximize != 0 && maximize != 1) return fail(c, ESIM_EINVAL, who + ": maximize must be 0 or 1");
    if (int rc = members_read_check(c, who, 0u, 0u)) return rc;      // the state first: a store, and something in it
    const Ensemble::Store &s = c->ens.store;
    if (s.is_signed) return fail(c, ESIM_ESTATE, who + ": the store is signed (a paired kind is a difference of two arms already: a grid of them has no meaning)");
    if (int rc = members_read_check(c, who, first_row, n_rows)) return rc;
    if (s.kept % n_arms != 0u)
        return fail(c, ESIM_ERANGE, who + ": the " + std::to_string(s.kept) + " members kept are no whole number of replicates of " + std::to_string(n_arms) + " arms");
    HIP_TRY(c, hipSetDevice(c->P.device));
    const size_t plane = (size_t)s.n_rows * s.n_cols, at = (size_t)first_row * s.n_cols, cells = (size_t)n_rows * s.n_cols, table = (size_t)n_arms * cells;
    // only the tables asked for: 24 B an arm and cell otherwise.  The totals and the kernel's counts always.
    DevTmp<uint32_t> d32;
    DevTmp<unsigned long long> d64;
    const size_t n32 = ((best ? 1u : 0u) + (sole ? 1u : 0u)) * table, n64 = ((regret ? 1u : 0u) + (sum ? 1u : 0u)) * table;
    if (d32.alloc(n32) != hipSuccess || d64.alloc(n64 + s.kept + ARMS_STATS) != hipSuccess) {
        (void)hipGetLastError();
        return fail(c, ESIM_ENOMEM, who + ": no device memory for the tables (24 B per arm and cell with every output)");
    }
    ArmsOut o;
    o.best = best ? d32.p : nullptr;
    o.sole = sole ? d32.p + (best ? table : 0u) : nullptr;
    o.regret = regret ? d64.p : nullptr;
    o.sum = sum ? d64.p + (regret ? table : 0u) : nullptr;
    o.totals = d64.p + n64;
    o.stats = o.totals + s.kept;
    HIP_TRY(c, hipMemsetAsync(o.totals, 0, sizeof(unsigned long long) * (s.kept + ARMS_STATS), c->stream));
    if (!totals) o.totals = nullptr;                                // (the kernel then sums none)
    arms_enqueue(s.planes, plane, n_arms, s.kept / n_arms, at, cells, members_skip(c), maximize != 0, s.has_never ? never_as : MEMBERS_NEVER, o, c->stream,
                 grid_capped(c, cells, MEMBERS_TPB, MEMBERS_GRID));
    uint64_t stats[ARMS_STATS];
    if (int rc = members_deliver(c, who, (const uint32_t *)o.stats, 2u * ARMS_STATS, false, (uint32_t *)stats)) return rc;
    if (int rc = members_deliver(c, who, o.best, best ? table : 0u, false, best)) return rc;
    if (int rc = members_deliver(c, who, o.sole, sole ? table : 0u, false, sole)) return rc;
    if (int rc = members_deliver(c, who, (const uint32_t *)o.regret, regret ? 2u * table : 0u, false, (uint32_t *)regret)) return rc;
    if (int rc = members_deliver(c, who, (const uint32_t *)o.sum, sum ? 2u * table : 0u, false, (uint32_t *)sum)) return rc;
    if (int rc = members_deliver(c, who, (const uint32_t *)o.totals, totals ? 2u * (size_t)s.kept : 0u, false, (uint32_t *)totals)) return rc;
    if (totals) arms_totals_finish(totals, s.kept, stats);
    if (live_cells) *live_cells = stats[ARMS_LIVE];
    return ESIM_OK;
}
