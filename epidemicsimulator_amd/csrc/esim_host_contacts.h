// esim_host_contacts.h -- contact-hours at risk: esim_contact_hours, on top of tree_enqueue / tree_finish (the kernels:
// esim_kernels_contacts.h).  The call works in temporary device memory that lives as long as the call, and leaves the
// context as it is.
namespace {

// Bits of one launch of k_contact_route_mark: the (bus step, route) items of a window are replayed in stretches of bus steps
// whose bit set stays below this (64 MB).
const uint64_t CONTACT_BITS_MAX = 1ull << 29;
// Workgroups of k_contact_route, each with 8 B per rider of the longest route in global memory (at most 256 MB together).
const uint32_t CONTACT_ROUTE_GRID = 2048u;

}  // namespace

extern "C" int esim_contact_hours(esim_ctx *ctx, int where, uint32_t setting_mask, uint32_t first_step, uint32_t last_step, uint64_t *hours, uint64_t *transmissions,
                                  uint32_t *per_case)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    const std::string who = "esim_contact_hours";
    if ((where != ESIM_BY_ALL && where != ESIM_BY_GROUP) || setting_mask == 0u || (setting_mask >> ESIM_N_SETTINGS) != 0u)
        return fail(c, ESIM_EINVAL, who + ": a `where` that is neither ESIM_BY_ALL nor ESIM_BY_GROUP, or a setting mask that is empty or names a setting beyond ESIM_SETTING_TRANSPORT");
    if (int rc = tree_check(c, who)) return rc;
    if (where == ESIM_BY_GROUP && !c->grp.lab) return fail(c, ESIM_ESTATE, who + ": by group without labels (esim_set_groups)");
    if (first_step == 0 || last_step < first_step || last_step > c->host_t - 1u)
        return fail(c, ESIM_ERANGE, who + ": steps outside 1 .. the steps run so far, or last_step before first_step");
    HIP_TRY(c, hipSetDevice(c->P.device));
    const Dev &d = c->d;
    if (per_case && ((uint64_t)d.infected_time + 1u) * 3u * c->longest_list > 0xFFFFFFFFull)
        return fail(c, ESIM_ERANGE, who + ": per_case is 32 bits wide: (infected_time + 1) x 3 x the longest member list (" + std::to_string(c->longest_list) + ") does not fit");
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the counters are 64 bits wide");
    Contact k;
    k.first = first_step; k.last = last_step; k.mask = setting_mask;
    k.n_cols = where == ESIM_BY_ALL ? 1u : c->grp.n;
    k.grp = where == ESIM_BY_GROUP ? (const uint16_t *)c->grp.lab : nullptr;
    const size_t cells = (size_t)k.n_cols * k.n_cols, plane = (size_t)ESIM_N_SETTINGS * cells, lds = plane * sizeof(unsigned long long);
    const uint32_t t_done = c->host_t - 1u;
    k.stride = t_done + 1u;
    DevTmp<unsigned long long> tab;
    DevTmp<uint32_t> pre, cases, bus_steps, bits, tmp;
    const bool long_routes = ((setting_mask >> ESIM_SETTING_TRANSPORT) & 1u) && d.max_route > d.bus_capacity && (hours || per_case);
    if (tab.alloc(2 * plane) != hipSuccess || pre.alloc(4 * (size_t)k.stride) != hipSuccess || (per_case && cases.alloc(d.n) != hipSuccess)) {
        (void)hipGetLastError();
        return fail(c, ESIM_ENOMEM, who + ": no device memory for the tables (64 B per cell, 16 B per step, 4 B per citizen for per_case)");
    }
    k.hours = tab.p; k.trans = tab.p + plane; k.pre = pre.p; k.per_case = per_case ? cases.p : nullptr; k.bus_steps = nullptr;
    TreeWork w;
    if (int rc = tree_enqueue(c, who, &w, false)) return rc;
    // (from here on the stream is waited for before the host vectors of w and of this call go away)
    auto leave = [&](int rc, const std::string &what) { (void)hipGetLastError(); (void)hipStreamSynchronize(c->stream); return fail(c, rc, who + ": " + what); };
    // the four prefix counts over the steps, one per (work bit, bus bit) combination, and the bus steps of the window
    std::vector<uint32_t> h_pre(4 * (size_t)k.stride, 0u), h_bus_steps;
    for (uint32_t s = 1; s <= t_done; ++s) {
        const uint32_t comb = (w.s.shape.aw[s] ? 1u : 0u) | (w.s.h_bus[s] ? 2u : 0u);
        for (uint32_t cb = 0; cb < 4u; ++cb) h_pre[cb * (size_t)k.stride + s] = h_pre[cb * (size_t)k.stride + s - 1u] + (cb == comb ? 1u : 0u);
        if ((comb & 2u) && s >= first_step && s <= last_step) h_bus_steps.push_back(s);
    }
    const uint32_t n_bus = (uint32_t)h_bus_steps.size(), log_len = w.s.log_len;
    hipError_t e = hipMemcpyAsync(pre.p, h_pre.data(), sizeof(uint32_t) * h_pre.size(), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(tab.p, 0, sizeof(unsigned long long) * std::max<size_t>(1, 2 * plane), c->stream);
    if (e == hipSuccess && per_case) e = hipMemsetAsync(cases.p, 0, sizeof(uint32_t) * std::max<size_t>(1, d.n), c->stream);
    if (e != hipSuccess) return leave(ESIM_ENODEVICE, hipGetErrorString(e));
    if (hours || per_case) {
        const int mode = pairtab_mode(where, lds);
        if ((setting_mask >> ESIM_SETTING_HOUSEHOLD) & 1u) {
            const dim3 grid(grid_capped(c, log_len, TPB, 4096));
            if (mode == PAIRTAB_ONE_CELL) hipLaunchKernelGGL(k_contact_home<PAIRTAB_ONE_CELL>, grid, dim3(TPB), 0, c->stream, d, w.s.q, k, log_len);
            else if (mode == PAIRTAB_LDS) hipLaunchKernelGGL(k_contact_home<PAIRTAB_LDS>, dim3(grid_capped(c, log_len, TPB * HH_SAR_PER_LANE, 4096, TPB)), dim3(TPB), lds, c->stream, d, w.s.q, k, log_len);
            else hipLaunchKernelGGL(k_contact_home<PAIRTAB_GLOBAL>, grid, dim3(TPB), 0, c->stream, d, w.s.q, k, log_len);
        }
        if (setting_mask & ~(1u << ESIM_SETTING_HOUSEHOLD)) {
            const dim3 grid(grid_capped(c, log_len, TPB / 64u, 4096));
            if (mode == PAIRTAB_ONE_CELL) hipLaunchKernelGGL(k_contact_wide<PAIRTAB_ONE_CELL>, grid, dim3(TPB), 0, c->stream, d, w.s.q, k, log_len);
            else if (mode == PAIRTAB_LDS) hipLaunchKernelGGL(k_contact_wide<PAIRTAB_LDS>, grid, dim3(TPB), lds, c->stream, d, w.s.q, k, log_len);
            else hipLaunchKernelGGL(k_contact_wide<PAIRTAB_GLOBAL>, grid, dim3(TPB), 0, c->stream, d, w.s.q, k, log_len);
        }
    }
    if (long_routes && n_bus && d.n_routes) {
        // the bus steps of the window in stretches whose (step, route) bit set fits CONTACT_BITS_MAX
        const uint32_t per = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(n_bus, CONTACT_BITS_MAX / d.n_routes));
        const size_t n_words = (size_t)(((uint64_t)per * d.n_routes + 31u) / 32u);
        // (a workgroup takes 64 words of the bit set a trip; tmp below is sized by the grid as clamped)
        const uint32_t route_grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(CONTACT_ROUTE_GRID, (256ull << 20) / (8ull * d.max_route)));
        const uint32_t grid = grid_clamp(c, n_words, 64u, route_grid, __builtin_FILE(), __builtin_LINE());
        if (n_words > 0xFFFFFFFFull || bus_steps.alloc(n_bus) != hipSuccess || bits.alloc(n_words) != hipSuccess || tmp.alloc((size_t)grid * 2u * d.max_route) != hipSuccess)
            return leave(ESIM_ENOMEM, "no device memory for the routes longer than a bus (a bit per route and bus step of the window, 64 MB at most, and 8 B per rider of the longest route per workgroup)");
        k.bus_steps = bus_steps.p;
        e = hipMemcpyAsync(bus_steps.p, h_bus_steps.data(), sizeof(uint32_t) * n_bus, hipMemcpyHostToDevice, c->stream);
        for (uint32_t lo = 0; lo < n_bus && e == hipSuccess; lo += per) {
            const uint32_t hi = std::min(n_bus, lo + per);
            e = hipMemsetAsync(bits.p, 0, sizeof(uint32_t) * n_words, c->stream);
            if (e != hipSuccess) break;
            hipLaunchKernelGGL(k_contact_route_mark, dim3(grid_capped(c, log_len, TPB, 4096)), dim3(TPB), 0, c->stream, d, w.s.q, k, log_len, lo, hi, bits.p);
            hipLaunchKernelGGL(k_contact_route, dim3(grid), dim3(64), 0, c->stream, d, w.s.q, k, lo, bits.p, (uint32_t)n_words, tmp.p);
        }
        if (e != hipSuccess) return leave(ESIM_ENODEVICE, hipGetErrorString(e));
    }
    if (transmissions) hipLaunchKernelGGL(k_contact_trans, dim3(grid_capped(c, log_len, TPB, 4096)), dim3(TPB), 0, c->stream, d, w.s.q, w.t, k, log_len);
    const int rc = tree_finish(c, who, &w);
    if (rc && rc != ESIM_ESIM) return rc;
    if (hours) HIP_TRY(c, hipMemcpy(hours, k.hours, sizeof(uint64_t) * plane, hipMemcpyDeviceToHost));
    if (transmissions) HIP_TRY(c, hipMemcpy(transmissions, k.trans, sizeof(uint64_t) * plane, hipMemcpyDeviceToHost));
    if (per_case && d.n) HIP_TRY(c, hipMemcpy(per_case, cases.p, sizeof(uint32_t) * (size_t)d.n, hipMemcpyDeviceToHost));
    return rc;
}
