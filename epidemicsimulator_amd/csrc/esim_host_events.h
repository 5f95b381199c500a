// esim_host_events.h -- superspreading events: esim_transmission_events, the transmissions of every (gathering, step) counted,
// listed by key or by size and binned per setting, on top of tree_enqueue / tree_finish and the pair engine of esim_host_flows.h;
// esim_routes, the table that names a route ordinal.  The kernels: esim_kernels_events.h; DESIGN 21.  The events work in
// temporary device memory that lives as long as the call, and leave the context as it is.
extern "C" int esim_transmission_events(esim_ctx *ctx, uint32_t setting_mask, uint32_t first_step, uint32_t last_step, uint32_t min_size, int order,
                                        uint32_t *step, uint8_t *setting, uint32_t *place, uint32_t *bus, uint32_t *size, uint32_t cap, uint32_t *n_out,
                                        uint32_t *sizes)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    const std::string who = "esim_transmission_events";
    if (!n_out) return fail(c, ESIM_EINVAL, who + ": null n_out");
    if (min_size == 0u || (order != ESIM_EVENTS_BY_KEY && order != ESIM_EVENTS_BY_SIZE))
        return fail(c, ESIM_EINVAL, who + ": min_size 0 (every event has a transmission), or an order that is neither ESIM_EVENTS_BY_KEY nor ESIM_EVENTS_BY_SIZE");
    if (int rc = flows_check(c, who, setting_mask, first_step, last_step)) return rc;
    if (c->host_t - 1u >= EVENT_MAX_STEPS) return fail(c, ESIM_ERANGE, who + ": more than 2^30 steps run: the key of an event has 30 bits for its step");
    HIP_TRY(c, hipSetDevice(c->P.device));
    const bool by_size = order == ESIM_EVENTS_BY_SIZE, lists = step || setting || place || bus || size;
    DevTmp<uint32_t> hist, out, by_cnt;
    DevTmp<uint8_t> out_set;
    DevTmp<unsigned long long> by_key;
    const size_t bins = (size_t)ESIM_N_SETTINGS * ESIM_EVENT_BINS;
    if (sizes && hist.alloc(bins) != hipSuccess) { (void)hipGetLastError(); return fail(c, ESIM_ENOMEM, who + ": no device memory for the size table (4 KB)"); }
    TreeWork w;
    PairWork p;
    if (int rc = tree_enqueue(c, who, &w, false, true)) return rc;
    const uint32_t log_len = w.s.log_len;
    if (int rc = pairs_begin(c, who, &p, log_len)) return flows_unwind(c, rc);
    hipLaunchKernelGGL(k_event_keys, dim3(grid_capped(c, log_len, TPB, 4096)), dim3(TPB), 0, c->stream, c->d, w.s.q, w.t, setting_mask, first_step, last_step, log_len, p.t);
    if (sizes) {
        const hipError_t e = hipMemsetAsync(hist.p, 0, sizeof(uint32_t) * bins, c->stream);
        if (e != hipSuccess) return flows_unwind(c, fail(c, ESIM_ENODEVICE, who + ": " + hipGetErrorString(e)));
        // (a workgroup walks 8 slots per lane at least before it hands over its 1024 counters)
        hipLaunchKernelGGL(k_event_hist, dim3(grid_capped(c, p.t.cap, PAIR_TPB * 8u, 1024, PAIR_TPB)), dim3(PAIR_TPB), 0, c->stream, p.t, hist.p);
    }
    if (int rc = pairs_compacted(c, &p, min_size)) return flows_unwind(c, rc);
    // the events to deliver: by key all of them or none, by size the first `cap`
    const uint32_t n = p.n, m = !lists || p.dropped ? 0u : by_size ? std::min(cap, n) : n <= cap ? n : 0u;
    if (m) {
        const uint32_t n_sort = pair_pow2(n);
        if (out.alloc(4 * (size_t)m) != hipSuccess || out_set.alloc(m) != hipSuccess || (by_size && (by_key.alloc(n_sort) != hipSuccess || by_cnt.alloc(n_sort) != hipSuccess))) {
            (void)hipGetLastError();
            return flows_unwind(c, fail(c, ESIM_ENOMEM, who + ": no device memory for the list (17 B per event delivered, and 12 B per event for the order by size)"));
        }
        pairs_sort_enqueue(p.out_key.p, p.out_cnt.p, n_sort, c->stream);
        if (by_size) {
            hipLaunchKernelGGL(k_event_rekey, dim3(grid_capped(c, n_sort, PAIR_TPB, 4096)), dim3(PAIR_TPB), 0, c->stream, p.out_cnt.p, n, n_sort, by_key.p, by_cnt.p);
            pairs_sort_enqueue(by_key.p, by_cnt.p, n_sort, c->stream);
        }
        EventOut o;
        o.step = step ? out.p : nullptr; o.place = place ? out.p + m : nullptr; o.bus = bus ? out.p + 2 * (size_t)m : nullptr; o.size = size ? out.p + 3 * (size_t)m : nullptr;
        o.setting = setting ? out_set.p : nullptr;
        hipLaunchKernelGGL(k_event_split, dim3(grid_capped(c, m, PAIR_TPB, 4096)), dim3(PAIR_TPB), 0, c->stream, c->d, p.out_key.p, p.out_cnt.p, n, by_size ? by_key.p : nullptr, m, o);
    }
    {
        const hipError_t e = hipEventRecord(p.ev[3], c->stream);
        if (e != hipSuccess) return flows_unwind(c, fail(c, ESIM_ENODEVICE, who + ": " + hipGetErrorString(e)));
    }
    const int rc = tree_finish(c, who, &w);
    if (rc && rc != ESIM_ESIM) return rc;
    if (int full = pairs_end(c, who, &p)) return full;
    *n_out = n;
    if (sizes) HIP_TRY(c, hipMemcpy(sizes, hist.p, sizeof(uint32_t) * bins, hipMemcpyDeviceToHost));
    if (!by_size && n > cap) return fail(c, ESIM_ERANGE, who + ": buffers too small (n_out holds the size needed)");
    if (m) {
        const size_t bytes = sizeof(uint32_t) * (size_t)m;
        if (step) HIP_TRY(c, hipMemcpy(step, out.p, bytes, hipMemcpyDeviceToHost));
        if (place) HIP_TRY(c, hipMemcpy(place, out.p + m, bytes, hipMemcpyDeviceToHost));
        if (bus) HIP_TRY(c, hipMemcpy(bus, out.p + 2 * (size_t)m, bytes, hipMemcpyDeviceToHost));
        if (size) HIP_TRY(c, hipMemcpy(size, out.p + 3 * (size_t)m, bytes, hipMemcpyDeviceToHost));
        if (setting) HIP_TRY(c, hipMemcpy(setting, out_set.p, m, hipMemcpyDeviceToHost));
    }
    return rc;
}

extern "C" int esim_routes(esim_ctx *ctx, uint32_t *home_area, uint32_t *work_area, uint32_t *n_riders, uint32_t cap, uint32_t *n_out)
{
    esim_ctx_impl *c = CTX(ctx);
    if (!c || !n_out) return fail(c, ESIM_EINVAL, "esim_routes: null argument");
    if (!c->uploaded) return fail(c, ESIM_ESTATE, "esim_routes: no population uploaded");
    const size_t n = c->route_tab.size() / 3u;
    *n_out = (uint32_t)n;
    if (n > cap) return fail(c, ESIM_ERANGE, "esim_routes: buffers too small (n_out holds the size needed)");
    if (home_area && n) std::memcpy(home_area, c->route_tab.data(), sizeof(uint32_t) * n);
    if (work_area && n) std::memcpy(work_area, c->route_tab.data() + n, sizeof(uint32_t) * n);
    if (n_riders && n) std::memcpy(n_riders, c->route_tab.data() + 2 * n, sizeof(uint32_t) * n);
    return ESIM_OK;
}
