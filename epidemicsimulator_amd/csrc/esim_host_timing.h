// esim_host_timing.h -- timing and diagnostics: read-outs of Timing's event timers, counters of the forms, diagnostics builds.
extern "C" int esim_vax_chunk_stats(esim_ctx *ctx, uint64_t *steps, uint64_t *cuts)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    if (steps) *steps = c->vax_chunk_steps;
    if (cuts) *cuts = c->vax_chunk_cuts;
    return ESIM_OK;
}

extern "C" int esim_vax_repair_stats(esim_ctx *ctx, uint64_t *repairs)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    if (repairs) *repairs = c->vax_chunk_repairs;
    return ESIM_OK;
}

extern "C" int esim_chunk_timing(esim_ctx *ctx, double *total_ms, uint64_t *steps, uint64_t *chunks)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    if (total_ms) *total_ms = c->tm.chunk_ms;
    if (steps) *steps = c->tm.chunk_steps;
    if (chunks) *chunks = c->tm.chunk_count;
    c->tm.chunk_ms = 0; c->tm.chunk_steps = 0; c->tm.chunk_count = 0;
    return ESIM_OK;
}

extern "C" int esim_enable_chunk_kernel_timing(esim_ctx *ctx, int enable)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    if (int rc = drain(c)) return rc;
    c->tm.kdetail = enable != 0;
    c->tm.kd_used = 0;
    for (int i = 0; i < ESIM_CK_N; ++i) { c->tm.kd_ms[i] = 0; c->tm.kd_calls[i] = 0; }
    return ESIM_OK;
}

extern "C" int esim_chunk_kernel_timings(esim_ctx *ctx, double ms[ESIM_CK_N], uint64_t calls[ESIM_CK_N])
{
    esim_ctx_impl *c = CTX(ctx);
    if (!c || !ms || !calls) return ESIM_EINVAL;
    if (int rc = drain(c)) return rc;
    kd_resolve(c);
    for (int i = 0; i < ESIM_CK_N; ++i) { ms[i] = c->tm.kd_ms[i]; calls[i] = c->tm.kd_calls[i]; c->tm.kd_ms[i] = 0; c->tm.kd_calls[i] = 0; }
    return ESIM_OK;
}

extern "C" int esim_pipeline_timing(esim_ctx *ctx, double *mean_step_ms, uint64_t *steps_timed, uint64_t *steps_run)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    if (int rc = drain(c)) return rc;
    double acc = 0;
    const size_t n = c->tm.pkev_used / 2;
    for (size_t i = 0; i < n; ++i) { float ms; HIP_TRY(c, hipEventElapsedTime(&ms, c->tm.pkev[2 * i], c->tm.pkev[2 * i + 1])); acc += ms; }
    if (mean_step_ms) *mean_step_ms = n ? acc / (double)n : 0.0;
    if (steps_timed) *steps_timed = n;
    if (steps_run) *steps_run = c->tm.pipe_steps;
    c->tm.pkev_used = 0; c->tm.pipe_steps = 0;
    return ESIM_OK;
}

extern "C" int esim_debug_counters(esim_ctx *ctx, uint32_t out[16])
{
    esim_ctx_impl *c = CTX(ctx);
    if (!c || !c->uploaded || !out) return ESIM_EINVAL;
    HIP_TRY(c, hipSetDevice(c->P.device));
    Ctrl h;
    const int rc = read_ctrl(c, &h);
    if (rc) return rc;
    const uint32_t v[16] = { h.t, h.chunk_ok, h.chunk_parallel, h.chunk_pairs, h.n_items, h.items_per_wave, h.n_units, h.chunk_bus,
                             h.n_route_pairs_big, h.n_newexp, h.log_len, h.n_susceptible, h.lockdown, h.mask, h.at_work, h.bus_dir };
    std::memcpy(out, v, sizeof v);
    return ESIM_OK;
}

extern "C" int esim_debug_launches(esim_ctx *ctx, char *sites, uint32_t *counts, uint32_t cap, uint32_t *out_n, int reset)
{
    esim_ctx_impl *c = CTX(ctx);
    if (!c || !out_n) return ESIM_EINVAL;
    LaunchLog &l = c->launches;
    if (l.overflow)
        return fail(c, ESIM_ERANGE, "esim_debug_launches: more than " + std::to_string(LAUNCH_SITES_MAX) + " launch sites were sized under ESIM_GRID_CAP (LAUNCH_SITES_MAX): records were lost");
    *out_n = l.n;
    if (cap < l.n || (l.n && (!sites || !counts))) {
        if (cap < l.n) return fail(c, ESIM_ERANGE, "esim_debug_launches: " + std::to_string(l.n) + " sites are recorded, cap is smaller");
        return ESIM_EINVAL;
    }
    for (uint32_t i = 0; i < l.n; ++i) {
        const LaunchLog::Site &s = l.site[i];
        const char *base = std::strrchr(s.file, '/');
        std::snprintf(sites + (size_t)i * ESIM_LAUNCH_SITE_CHARS, ESIM_LAUNCH_SITE_CHARS, "%s:%u", base ? base + 1 : s.file, s.line);
        counts[3 * i] = s.launches; counts[3 * i + 1] = s.clipped; counts[3 * i + 2] = s.max_trips;
    }
    if (reset) l = LaunchLog();
    return ESIM_OK;
}

#ifdef ESIM_COUNT_WORK
// counting build only (not in include/esim.h): what the chunk pass worked on since the last call (WK_* in esim_kernels_common.h)
extern "C" int esim_work_counters(esim_ctx *ctx, unsigned long long *out, uint32_t n)
{
    esim_ctx_impl *c = CTX(ctx);
    if (!c || !c->uploaded || !out) return ESIM_EINVAL;
    if (int rc = drain(c)) return rc;
    unsigned long long h[WK_N];
    HIP_TRY(c, hipMemcpy(h, c->d.work_cnt, sizeof h, hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemset(c->d.work_cnt, 0, sizeof h));
    for (uint32_t i = 0; i < n; ++i) out[i] = i < WK_N ? h[i] : 0ull;
    return ESIM_OK;
}
#endif

#ifdef ESIM_WAVE_PROFILE
// diagnostics build only (not in include/esim.h): rows of per-wavefront timers, and the timer's rate in kHz
extern "C" int esim_prof_read(esim_ctx *ctx, uint32_t *out, uint32_t n_words, int *clock_khz)
{
    esim_ctx_impl *c = CTX(ctx);
    if (!c || !c->uploaded || !out) return ESIM_EINVAL;
    if (int rc = drain(c)) return rc;
    HIP_TRY(c, hipMemcpy(out, c->d.prof_buf, sizeof(uint32_t) * std::min<uint32_t>(n_words, 16384u * 16u), hipMemcpyDeviceToHost));
    if (clock_khz) HIP_TRY(c, hipDeviceGetAttribute(clock_khz, hipDeviceAttributeWallClockRate, c->P.device));
    return ESIM_OK;
}
#endif

extern "C" int esim_enable_phase_timing(esim_ctx *ctx, int enable)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    c->tm.phase = enable != 0;
    return ESIM_OK;
}

extern "C" int esim_phase_timings(esim_ctx *ctx, double out[4])
{
    esim_ctx_impl *c = CTX(ctx);
    if (!c || !out) return ESIM_EINVAL;
    out[0] = c->tm.phase_s[0]; out[1] = c->tm.phase_s[1]; out[2] = c->tm.phase_s[2];
    out[3] = out[0] + out[1] + out[2];
    return ESIM_OK;
}

extern "C" int esim_enable_kernel_timing(esim_ctx *ctx, int enable)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    c->tm.kernel = enable > 0;
    if (enable > 0) c->tm.stride = (uint32_t)enable;   // time every `enable`-th step
    c->tm.kev_used = 0;
    if (enable > 0) {                                     // (the events the timed runs record: made here, not inside a timed call)
        HIP_TRY(c, hipSetDevice(c->P.device));
        Timing::make_pair(c->tm.cev); Timing::make_pair(c->tm.sev);
    }
    return ESIM_OK;
}

extern "C" int esim_small_kernel_timing(esim_ctx *ctx, double *total_ms, uint64_t *steps)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    if (total_ms) *total_ms = c->tm.small_ms;
    if (steps) *steps = c->tm.small_steps;
    c->tm.small_ms = 0; c->tm.small_steps = 0;
    return ESIM_OK;
}

extern "C" int esim_kernel_timings(esim_ctx *ctx, double *step_ms, uint32_t *out_n)
{
    esim_ctx_impl *c = CTX(ctx);
    if (!c || !step_ms) return ESIM_EINVAL;
    if (int rc = drain(c)) return rc;
    double acc = 0;
    const size_t n = c->tm.kev_used / 2;
    for (size_t i = 0; i < n; ++i) { float ms; HIP_TRY(c, hipEventElapsedTime(&ms, c->tm.kev[2 * i], c->tm.kev[2 * i + 1])); acc += ms; }
    *step_ms = n ? acc / n : 0.0;
    if (out_n) *out_n = (uint32_t)n;
    c->tm.kev_used = 0;
    return ESIM_OK;
}
