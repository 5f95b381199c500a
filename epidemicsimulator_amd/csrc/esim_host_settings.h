// esim_host_settings.h -- exposures by setting: esim_exposure_settings, esim_setting_series, esim_building_exposures (the kernels:
// esim_kernels_setting.h).  All three derive the setting of every logged exposure in temporary device memory that
// lives as long as the call, and leave the context as it is.
namespace {

// The second global bit per step, beside RunShape::aw: 1 while everybody who uses public transport is on a bus.  Stateful like
// the at-work bit -- the schedule arm of step s runs iff the record of step s - 1 has no lockdown (citizen.rs:176-206), so a
// lockdown that starts during a bus hour keeps the riders on their bus until it ends.
int bus_shape(esim_ctx_impl *c, uint32_t t_done, std::vector<uint8_t> *bus)
{
    std::vector<esim_step_result> rec((size_t)t_done + 1u);
    if (t_done) HIP_TRY(c, hipMemcpy(rec.data() + 1, c->d.records + 1, sizeof(esim_step_result) * t_done, hipMemcpyDeviceToHost));
    bus->assign((size_t)t_done + 1u, 0);
    for (uint32_t s = 1; s <= t_done; ++s) {
        uint8_t cur = (*bus)[s - 1u];
        if (s == 1u || !rec[s - 1u].lockdown) {
            const uint32_t hr = s % 24u;
            cur = hr == c->P.start_hour - 1u || hr == c->P.end_hour - 1u;
        }
        (*bus)[s] = cur;
    }
    return ESIM_OK;
}

// What the three calls refuse alike, behind their own argument checks.
int settings_check(esim_ctx_impl *c, const std::string &who)
{
    if (!c->uploaded) return fail(c, ESIM_ESTATE, who + ": no population uploaded");
    if (c->comm.world > 1 || c->d.n_global != c->d.n)
        return fail(c, ESIM_ESTATE, who + ": the context has a communicator of several ranks, or holds a shard (a household draw is replayed from the whole population's log)");
    if (c->household_work)
        return fail(c, ESIM_ESTATE, who + ": the population has a household that is the work place of a citizen who does not live in it; the replay counts only the residents among the Infected of a household and would credit exposures to the wrong setting");
    if (c->draw_seam.twice)
        return fail(c, ESIM_ESTATE, who + ": the run was branched from a snapshot that itself lay on a branch under another seed, exposure_chance or mask_effectiveness; a history mixed twice is not built");
    return ESIM_OK;
}

// The temporaries of one call, and what the host copies to the device from: all of it lives until the call has waited.
struct SettingWork {
    DevTmp<uint32_t> te, vax, bad;
    DevTmp<uint8_t> set, aw, bus;
    DevTmp<uint64_t> lut;
    RunShape shape;
    std::vector<uint8_t> h_bus;
    uint64_t h_lut[512];
    uint32_t log_len = 0;
    Setting q;
};

// The setting of every exposure, enqueued on the context's stream: one wait in front (the control block, and the records behind
// it), then the log scattered into the exposure step per citizen, the vaccinations replayed once a programme has run, and the
// household draw of every building exposure drawn again.
int settings_enqueue(esim_ctx_impl *c, const std::string &who, SettingWork *w)
{
    const Dev &d = c->d;
    const uint32_t t_done = c->host_t - 1u;
    Ctrl h; int rc;
    if ((rc = read_ctrl(c, &h)) || (rc = ctrl_error(c, h))) return rc;
    if ((rc = run_shape(c, t_done, &w->shape)) || (rc = bus_shape(c, t_done, &w->h_bus))) return rc;
    const bool replay = w->shape.trigger != 0u, seam = c->draw_seam.step != 0u;
    if (w->te.alloc(d.n) != hipSuccess || w->set.alloc(d.n) != hipSuccess || w->bad.alloc(1) != hipSuccess || w->aw.alloc((size_t)t_done + 1u) != hipSuccess ||
        w->bus.alloc((size_t)t_done + 1u) != hipSuccess || (replay && w->vax.alloc(d.n) != hipSuccess) || (seam && w->lut.alloc(512) != hipSuccess)) {
        (void)hipGetLastError();
        return fail(c, ESIM_ENOMEM, who + ": no device memory for the exposure steps and settings (5 B per citizen, 4 more once a vaccination programme has run)");
    }
    w->log_len = std::min<uint32_t>(h.log_len, d.n);
    Setting &q = w->q;
    q.t_done = t_done; q.t_all = w->shape.t_all; q.seam_step = 0u; q.old_seed_lo = q.old_seed_hi = 0u; q.old_thr = nullptr;
    q.te_of = w->te.p; q.vax_of = replay ? w->vax.p : nullptr; q.at_work = w->aw.p; q.on_bus = w->bus.p; q.setting = w->set.p; q.unexplained = w->bad.p;
    hipError_t e = hipMemsetAsync(w->te.p, 0xFF, sizeof(uint32_t) * std::max<size_t>(1, d.n), c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(w->bad.p, 0, sizeof(uint32_t), c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(w->aw.p, w->shape.aw.data(), (size_t)t_done + 1u, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(w->bus.p, w->h_bus.data(), (size_t)t_done + 1u, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess && seam) {
        // the LUT the entries up to the seam were drawn under, from the two doubles of then
        esim_params old = c->P;
        old.exposure_chance = c->draw_seam.chance; old.mask_effectiveness = c->draw_seam.mask_effectiveness;
        esim_threshold_lut(&old, w->h_lut);
        e = hipMemcpyAsync(w->lut.p, w->h_lut, sizeof w->h_lut, hipMemcpyHostToDevice, c->stream);
        q.seam_step = c->draw_seam.step; q.old_seed_lo = (uint32_t)c->draw_seam.seed; q.old_seed_hi = (uint32_t)(c->draw_seam.seed >> 32); q.old_thr = w->lut.p;
    }
    if (e == hipSuccess && replay) e = enqueue_vax_replay(c, w->shape.trigger, t_done, w->vax.p);
    if (e != hipSuccess) { (void)hipStreamSynchronize(c->stream); return fail(c, ESIM_ENODEVICE, who + ": " + hipGetErrorString(e)); }
    hipLaunchKernelGGL(k_setting_scatter, dim3(grid_capped(c, w->log_len, TPB, 4096)), dim3(TPB), 0, c->stream, d, q, w->log_len);
    hipLaunchKernelGGL(k_setting_attr, dim3(grid_capped(c, d.n, TPB, 4096)), dim3(TPB), 0, c->stream, d, q);
    return ESIM_OK;
}

// The tail of the three calls: the wait, and the audit's result -- ESIM_ESIM where an exposure has no draw that explains it.
int settings_finish(esim_ctx_impl *c, const std::string &who, SettingWork *w)
{
    uint32_t bad = 0;
    hipError_t e = hipGetLastError();
    const hipError_t es = hipStreamSynchronize(c->stream);           // (the host vectors of *w are done with here, too)
    if (e == hipSuccess) e = es;
    if (e == hipSuccess) e = hipMemcpy(&bad, w->bad.p, sizeof bad, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(c, ESIM_ENODEVICE, who + ": " + hipGetErrorString(e));
    if (bad) return fail(c, ESIM_ESIM, who + ": " + std::to_string(bad) + " building exposures of the log are unexplained: neither the household draw nor a work-side draw can have exposed the citizen in that step (they carry ESIM_SETTING_NONE)");
    return ESIM_OK;
}

}  // namespace

extern "C" int esim_exposure_settings(esim_ctx *ctx, uint8_t *setting, uint32_t *building)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    const std::string who = "esim_exposure_settings";
    if (int rc = settings_check(c, who)) return rc;
    HIP_TRY(c, hipSetDevice(c->P.device));
    SettingWork w;
    if (int rc = settings_enqueue(c, who, &w)) return rc;
    const size_t n = c->d.n;
    if (building) hipLaunchKernelGGL(k_setting_building, dim3(grid_capped(c, n, TPB, 4096)), dim3(TPB), 0, c->stream, c->d, w.q);
    const int rc = settings_finish(c, who, &w);
    if (rc && rc != ESIM_ESIM) return rc;
    if (setting && n) HIP_TRY(c, hipMemcpy(setting, w.set.p, n, hipMemcpyDeviceToHost));
    if (building && n) HIP_TRY(c, hipMemcpy(building, w.te.p, sizeof(uint32_t) * n, hipMemcpyDeviceToHost));
    return rc;
}

extern "C" int esim_setting_series(esim_ctx *ctx, int where, uint32_t setting_mask, uint32_t first_step, uint32_t n_rows, uint32_t stride, uint32_t *out)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    const std::string who = "esim_setting_series";
    if (!out || (where != ESIM_BY_SETTING && where != ESIM_AREA_HOME && where != ESIM_BY_GROUP) || setting_mask == 0u || (setting_mask >> ESIM_N_SETTINGS) != 0u ||
        stride == 0 || n_rows == 0)
        return fail(c, ESIM_EINVAL, who + ": null output, unknown `where` (a bus has no area: not ESIM_AREA_CURRENT), a setting mask that is empty or names a setting beyond ESIM_SETTING_TRANSPORT, stride 0 or no rows");
    if (int rc = settings_check(c, who)) return rc;
    if (where == ESIM_BY_GROUP && !c->grp.lab) return fail(c, ESIM_ESTATE, who + ": by group without labels (esim_set_groups)");
    if (first_step == 0 || (uint64_t)first_step + (uint64_t)(n_rows - 1u) * stride > c->host_t - 1u)
        return fail(c, ESIM_ERANGE, who + ": rows outside the steps run so far");
    HIP_TRY(c, hipSetDevice(c->P.device));
    SettingRows r;
    r.where = (uint32_t)where; r.mask = setting_mask; r.first = first_step; r.n_rows = n_rows; r.stride = stride;
    r.n_cols = where == ESIM_BY_SETTING ? (uint32_t)ESIM_N_SETTINGS : where == ESIM_BY_GROUP ? c->grp.n : c->d.n_areas;
    r.grp = where == ESIM_BY_GROUP ? c->grp.lab : nullptr;
    const size_t words = (size_t)n_rows * r.n_cols;
    DevTmp<uint32_t> rows;
    if (rows.alloc(words) != hipSuccess) { (void)hipGetLastError(); return fail(c, ESIM_ENOMEM, who + ": no device memory for the rows (ask for fewer)"); }
    r.rows = rows.p;
    SettingWork w;
    if (int rc = settings_enqueue(c, who, &w)) return rc;
    HIP_TRY(c, hipMemsetAsync(rows.p, 0, sizeof(uint32_t) * std::max<size_t>(1, words), c->stream));
    hipLaunchKernelGGL(k_setting_rows, dim3(grid_capped(c, w.log_len, TPB, 4096)), dim3(TPB), 0, c->stream, c->d, w.q, r, w.log_len);
    const int rc = settings_finish(c, who, &w);
    if (rc && rc != ESIM_ESIM) return rc;
    if (words) HIP_TRY(c, hipMemcpy(out, rows.p, sizeof(uint32_t) * words, hipMemcpyDeviceToHost));
    return rc;
}

extern "C" int esim_building_exposures(esim_ctx *ctx, uint32_t first_step, uint32_t last_step, uint32_t *counts)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    const std::string who = "esim_building_exposures";
    if (!counts) return fail(c, ESIM_EINVAL, who + ": null output");
    if (int rc = settings_check(c, who)) return rc;
    if (first_step == 0 || last_step < first_step || last_step > c->host_t - 1u)
        return fail(c, ESIM_ERANGE, who + ": steps outside 1 .. the steps run so far, or last_step before first_step");
    HIP_TRY(c, hipSetDevice(c->P.device));
    const size_t nb = c->d.n_bld;
    DevTmp<uint32_t> tab;
    if (tab.alloc(nb) != hipSuccess) { (void)hipGetLastError(); return fail(c, ESIM_ENOMEM, who + ": no device memory for the building table"); }
    SettingWork w;
    if (int rc = settings_enqueue(c, who, &w)) return rc;
    HIP_TRY(c, hipMemsetAsync(tab.p, 0, sizeof(uint32_t) * std::max<size_t>(1, nb), c->stream));
    hipLaunchKernelGGL(k_setting_tally, dim3(grid_capped(c, w.log_len, TPB, 4096)), dim3(TPB), 0, c->stream, c->d, w.q, first_step, last_step, w.log_len, tab.p);
    const int rc = settings_finish(c, who, &w);
    if (rc && rc != ESIM_ESIM) return rc;
    if (nb) HIP_TRY(c, hipMemcpy(counts, tab.p, sizeof(uint32_t) * nb, hipMemcpyDeviceToHost));
    return rc;
}
