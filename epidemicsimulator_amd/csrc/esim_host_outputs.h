// esim_host_outputs.h -- read-backs: records, state, exposure log; census and series by area and group; ensemble accumulators.
extern "C" int esim_read_records(esim_ctx *ctx, uint32_t first_step, uint32_t n, esim_step_result *out)
{
    esim_ctx_impl *c = CTX(ctx);
    if (!c || !c->uploaded) return fail(c, ESIM_ESTATE, "no population uploaded");
    if (!out || first_step == 0 || (uint64_t)first_step + n > (uint64_t)c->P.max_steps + 1) return fail(c, ESIM_EINVAL, "esim_read_records: bad range");
    if (int rc = drain(c)) return rc;
    HIP_TRY(c, hipMemcpy(out, &c->d.records[first_step], sizeof(esim_step_result) * n, hipMemcpyDeviceToHost));
    return device_error(c);
}

extern "C" int esim_synchronize(esim_ctx *ctx)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    if (int rc = drain(c)) return rc;
    return ESIM_OK;
}

extern "C" int esim_download_state(esim_ctx *ctx, uint8_t *status, uint16_t *timer, uint32_t *current_building,
                                   uint8_t *on_bus, uint8_t *eligible)
{
    esim_ctx_impl *c = CTX(ctx);
    if (!c || !c->uploaded) return fail(c, ESIM_ESTATE, "no population uploaded");
    HIP_TRY(c, hipSetDevice(c->P.device));
    const uint32_t N = c->d.n;
    DevTmp<uint8_t> d_status, d_bus, d_elig; DevTmp<uint16_t> d_timer; DevTmp<uint32_t> d_cur;
    if ((status && d_status.alloc(N) != hipSuccess) || (on_bus && d_bus.alloc(N) != hipSuccess) || (eligible && d_elig.alloc(N) != hipSuccess) ||
        (timer && d_timer.alloc(N) != hipSuccess) || (current_building && d_cur.alloc(N) != hipSuccess)) return fail(c, ESIM_ENOMEM, "esim_download_state: hipMalloc");
    hipLaunchKernelGGL(k_decode_state, dim3(grid_clamp(c, N, TPB, c->tune.grid_citizens, __builtin_FILE(), __builtin_LINE())), dim3(TPB), 0, c->stream, c->d, d_status.p, d_timer.p, d_cur.p, d_bus.p, d_elig.p);
    hipError_t e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess && status) e = hipMemcpy(status, d_status.p, N, hipMemcpyDeviceToHost);
    if (e == hipSuccess && on_bus) e = hipMemcpy(on_bus, d_bus.p, N, hipMemcpyDeviceToHost);
    if (e == hipSuccess && eligible) e = hipMemcpy(eligible, d_elig.p, N, hipMemcpyDeviceToHost);
    if (e == hipSuccess && timer) e = hipMemcpy(timer, d_timer.p, 2 * (size_t)N, hipMemcpyDeviceToHost);
    if (e == hipSuccess && current_building) e = hipMemcpy(current_building, d_cur.p, 4 * (size_t)N, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(c, ESIM_ENODEVICE, std::string("esim_download_state: ") + hipGetErrorString(e));
    return ESIM_OK;
}

extern "C" int esim_download_exposure_log(esim_ctx *ctx, uint32_t *citizen, uint32_t *step, uint8_t *on_bus, uint32_t cap, uint32_t *n_out)
{
    esim_ctx_impl *c = CTX(ctx);
    if (!c || !c->uploaded || !n_out) return fail(c, ESIM_ESTATE, "no population uploaded");
    HIP_TRY(c, hipSetDevice(c->P.device));
    Ctrl h;
    const int rc = read_ctrl(c, &h);
    if (rc) return rc;
    const uint32_t t_done = c->host_t - 1u;                       // steps run so far
    // log_off[TE_BIAS + s] = first entry of step s; the entries before step 1 are the seeds (simulator_builder.rs:1268-1287)
    std::vector<uint32_t> off((size_t)t_done + 2u);
    HIP_TRY(c, hipMemcpy(off.data(), c->d.log_off + TE_BIAS + 1u, sizeof(uint32_t) * (t_done + 1u), hipMemcpyDeviceToHost));
    off[t_done + 1u] = h.log_len;
    const uint32_t first = t_done ? off[0] : h.log_len, n = h.log_len - first;
    *n_out = n;
    if (n > cap || (n && (!citizen || !step || !on_bus))) return fail(c, ESIM_ERANGE, "esim_download_exposure_log: buffers too small (n_out holds the size needed)");
    if (n == 0) return ESIM_OK;
    DevTmp<uint32_t> d_c; DevTmp<uint8_t> d_b;
    if (d_c.alloc(n) != hipSuccess || d_b.alloc(n) != hipSuccess) return fail(c, ESIM_ENOMEM, "esim_download_exposure_log: hipMalloc");
    hipLaunchKernelGGL(k_export_log, dim3(grid_capped(c, n, TPB, 2048)), dim3(TPB), 0, c->stream, c->d, first, n, d_c.p, d_b.p);
    hipError_t e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = hipMemcpy(citizen, d_c.p, sizeof(uint32_t) * (size_t)n, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(on_bus, d_b.p, n, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(c, ESIM_ENODEVICE, std::string("esim_download_exposure_log: ") + hipGetErrorString(e));
    for (uint32_t s = 1; s <= t_done; ++s)
        for (uint32_t i = off[s - 1u]; i < off[s] && i - first < n; ++i) step[i - first] = s;
    return ESIM_OK;
}

// ---- per-Output-Area read-backs ----------------------------------------------------------------------------------------
namespace {
// the count table of esim_area_census zeroed and counted on the context's stream (esim_ensemble_fold reads it where it is)
int enqueue_area_census(esim_ctx_impl *c, int where)
{
    const Dev &d = c->d;
    const size_t n_out = (size_t)d.n_areas * 5u;
    // stretches of whole workgroup passes, about 8192 of them at most: short enough to stay inside the LDS window of areas
    const uint32_t per_block = (uint32_t)std::max<uint64_t>(4096u, (((uint64_t)d.n + 8191u) / 8192u + TPB - 1u) / TPB * TPB);
    const uint32_t grid = (uint32_t)std::max<uint64_t>(1u, ((uint64_t)d.n + per_block - 1u) / per_block);
    HIP_TRY(c, hipMemsetAsync(c->area_cnt, 0, sizeof(uint32_t) * std::max<size_t>(1, n_out), c->stream));
    hipLaunchKernelGGL(k_area_census, dim3(grid), dim3(TPB), 0, c->stream, d, where == ESIM_AREA_HOME ? 1 : 0, per_block, c->area_cnt);
    return ESIM_OK;
}

// the count table of esim_group_census, the same way: four citizens per lane and trip, at most 1024 workgroups (four per
// compute unit: every one of them ends with up to 4 * n_groups adds to the global table)
int enqueue_group_census(esim_ctx_impl *c)
{
    const Dev &d = c->d;
    HIP_TRY(c, hipMemsetAsync(c->grp.cnt, 0, sizeof(uint32_t) * (size_t)c->grp.n * 5u, c->stream));
    hipLaunchKernelGGL(k_group_census, dim3(grid_capped(c, ((size_t)d.n + 3u) / 4u, TPB, 1024)), dim3(TPB), 0, c->stream, d, c->grp.lab, c->grp.n, c->grp.cnt);
    hipLaunchKernelGGL(k_group_finish, dim3(grid_for(c->grp.n, TPB, 0xFFFFFFFFu)), dim3(TPB), 0, c->stream, c->grp.size, c->grp.n, c->grp.cnt);
    return ESIM_OK;
}

// the table of esim_area_arrival filled with ESIM_NEVER and lowered on the context's stream, for the steps run so far as the
// host knows them (esim_ensemble_fold reads it where it is).  The log's length is the device's to know: the grid covers the
// longest log there can be, a lane per citizen, capped at 1024 workgroups, and strides over what the control block says.
int enqueue_arrival(esim_ctx_impl *c, int where)
{
    const Dev &d = c->d;
    const size_t room = std::max<size_t>(ESIM_MAX_GROUPS, d.n_areas);
    if (!c->arrival) { if (int rc = dev_alloc(c, &c->arrival, room)) return rc; }
    const bool by_group = where == ESIM_BY_GROUP;
    const uint32_t n_keys = by_group ? c->grp.n : d.n_areas;
    HIP_TRY(c, hipMemsetAsync(c->arrival, 0xFF, sizeof(uint32_t) * std::max<size_t>(1, n_keys), c->stream));
    hipLaunchKernelGGL(k_area_arrival, dim3(grid_capped(c, d.n, TPB, 1024)), dim3(TPB), 0, c->stream, d, by_group ? c->grp.lab : nullptr, n_keys,
                       c->host_t - 1u, c->arrival);
    return ESIM_OK;
}

// `where` of the arrival calls: by household area or by group; the area a citizen stands in is not built.
int arrival_check(esim_ctx_impl *c, int where, const std::string &who)
{
    if (where != ESIM_AREA_HOME && where != ESIM_BY_GROUP) return fail(c, ESIM_EINVAL, who + ": `where` must be ESIM_AREA_HOME or ESIM_BY_GROUP");
    if (!c->uploaded) return fail(c, ESIM_ESTATE, who + ": no population uploaded");
    if (where == ESIM_BY_GROUP && (!c->grp.lab || c->comm.world > 1)) return fail(c, ESIM_ESTATE, who + ": by group without labels (esim_set_groups)");
    return ESIM_OK;
}

// What the series derive from the records of the steps run (rec[1 .. t_done]): the at-work bit after the schedule arm of every
// step (citizen.rs:176-206: the arm of step s runs iff no lockdown was in force, i.e. the record of step s - 1 has none) and
// the steps at which it changes; the step that started the vaccination programme (0: none) and the first one that vaccinated
// the whole eligible set (0xFFFFFFFF: none).  The rate that decides the latter is the one the step was drawn under: the old one up to
// the seam of an esim_rollback, the one in force behind it.
struct RunShape { std::vector<uint8_t> aw; std::vector<uint32_t> tog; uint32_t trigger = 0, t_all = 0xFFFFFFFFu; };
int run_shape(esim_ctx_impl *c, uint32_t t_done, RunShape *r)
{
    std::vector<esim_step_result> rec((size_t)t_done + 1u);
    HIP_TRY(c, hipMemcpy(rec.data() + 1, c->d.records + 1, sizeof(esim_step_result) * t_done, hipMemcpyDeviceToHost));
    r->aw.assign((size_t)t_done + 1u, 0);
    for (uint32_t s = 1; s <= t_done; ++s) {
        uint8_t cur = r->aw[s - 1u];
        if (s == 1u || !rec[s - 1u].lockdown) {
            const uint32_t hr = s % 24u;
            if (hr == c->P.start_hour) cur = 1; else if (hr == c->P.end_hour) cur = 0;
        }
        r->aw[s] = cur;
        if (cur != r->aw[s - 1u]) r->tog.push_back(s);
        if (!r->trigger && rec[s].vaccination_active) r->trigger = s;
        if (r->trigger && r->t_all == 0xFFFFFFFFu && rec[s].eligible_count <= (s <= c->seam.step ? c->seam.rate : c->P.vaccination_rate)) r->t_all = s;
    }
    return ESIM_OK;
}

// vax_of[c] = the step at whose end citizen c was set Vaccinated, on the context's stream (steps that vaccinated the whole
// eligible set apart: RunShape::t_all).  Across the seam of an esim_rollback the choice is walked in two launches: the steps up to
// the seam under the seed and rate they were drawn with, the later ones under those in force.
hipError_t enqueue_vax_replay(esim_ctx_impl *c, uint32_t trigger, uint32_t t_done, uint32_t *d_vax)
{
    const hipError_t e = hipMemsetAsync(d_vax, 0xFF, sizeof(uint32_t) * (size_t)c->d.n, c->stream);
    if (e != hipSuccess) return e;
    auto walk = [&](const Dev &d, uint32_t first, uint32_t last) {
        if (first <= last)
            hipLaunchKernelGGL(k_area_vax_replay, dim3(std::min<uint32_t>(last - first + 1u, 1024u)), dim3(FIN_TPB), 0, c->stream, d, trigger, first, last, d_vax);
    };
    const uint32_t seam = std::min(c->seam.step, t_done);
    if (seam >= trigger) {
        Dev old = c->d;
        old.seed_lo = (uint32_t)c->seam.seed; old.seed_hi = (uint32_t)(c->seam.seed >> 32); old.vaccination_rate = c->seam.rate;
        walk(old, trigger, seam);
    }
    walk(c->d, std::max(trigger, seam + 1u), t_done);
    return e;
}

// The tail of both census calls: the count table to its pinned mirror, one wait (the control block's read-back: the table is in
// the mirror behind it), the mirror to the caller.
int census_readback(esim_ctx_impl *c, const uint32_t *table, uint32_t *mirror, size_t n_out, uint32_t *counts)
{
    if (n_out) HIP_TRY(c, hipMemcpyAsync(mirror, table, sizeof(uint32_t) * n_out, hipMemcpyDeviceToHost, c->stream));
    Ctrl h;
    if (int rc = read_ctrl(c, &h)) return rc;
    std::memcpy(counts, mirror, sizeof(uint32_t) * n_out);
    return ctrl_error(c, h);
}

// What one of the three series entry points asks of the engine (esim_kernels_series.h): its name, how its ESIM_ESTATE text
// calls the status rows, the column key, the status or SERIES_EVENTS, and whether event rows leave out public transport.
struct SeriesSpec { const char *who, *rows; uint32_t key, what; bool skip_bus, pieces; };

// What the engine works out before it enqueues anything: which of its passes the rows need and how much room they take.
struct SeriesPlan {
    bool events, by_group, stood, sus, two, replay, count_occ;
    uint32_t t_done, cols, log_len;
    size_t words, occ_words;                                  // (occupancy of plane 0, then of plane 1)
    RunShape shape;
};

// Where the engine works: the row plane(s) and its temporaries on the device -- a call's own or the caller's -- and the host
// memory the at-work bits are copied from, which has to stay as it is until the stream has run the copy.
struct SeriesBufs { uint32_t *p0, *p1, *occ, *tog, *vax; uint8_t *aw; const uint8_t *h_aw; };

// The first half of the engine: the window checked against the steps run, the one wait for the stream (the control block and the
// records behind it), the run's shape derived from the records on the host.
int series_plan(esim_ctx_impl *c, const SeriesSpec &s, uint32_t first_step, uint32_t n_rows, uint32_t stride, SeriesPlan *p)
{
    const std::string who = s.who;
    p->events = s.what == SERIES_EVENTS; p->by_group = s.key == KEY_GROUP; p->stood = s.key == KEY_STOOD; p->sus = s.what == ESIM_SUSCEPTIBLE;
    p->two = p->stood && !p->events && !s.pieces;             // (an event is credited to one column of plane 0)
    p->t_done = c->host_t - 1u;                               // steps run so far
    if (first_step == 0 || (uint64_t)first_step + (uint64_t)(n_rows - 1u) * stride > p->t_done)
        return fail(c, ESIM_ERANGE, who + ": rows outside the steps run so far");
    HIP_TRY(c, hipSetDevice(c->P.device));
    const Dev &d = c->d;
    Ctrl h; int rc;
    if ((rc = read_ctrl(c, &h)) || (rc = ctrl_error(c, h))) return rc;
    if ((rc = run_shape(c, p->t_done, &p->shape))) return rc;
    p->replay = !p->events && p->shape.trigger != 0u;
    if (p->replay && d.n_global != d.n)
        return fail(c, ESIM_ESTATE, who + ": the " + s.rows + " rows of a shard cannot be derived once a vaccination programme has run (the choice depends on the other shards' citizens)");
    p->cols = p->by_group ? c->grp.n : d.n_areas;
    p->words = (size_t)n_rows * p->cols;
    p->count_occ = p->sus && !p->by_group;                    // (a group's occupancy is its size)
    p->occ_words = (size_t)p->cols * (p->two ? 2u : 1u);
    p->log_len = std::min<uint32_t>(h.log_len, d.n);
    return ESIM_OK;
}

// The second half: n_rows rows of one column per area / group, [row * columns + column], counted from the exposure log and the
// citizen words into one plane, or two for the status rows by the area stood in, and summed up over the steps by k_series_prefix,
// which leaves the result in plane 0 -- all on the context's stream, nothing waited for.  Status rows are derived by replaying
// the vaccinations once a programme has run.
hipError_t series_enqueue(esim_ctx_impl *c, const SeriesSpec &s, uint32_t first_step, uint32_t n_rows, uint32_t stride, const SeriesPlan &p, const SeriesBufs &b)
{
    const Dev &d = c->d;
    const RunShape &shape = p.shape;
    hipError_t e = hipMemsetAsync(b.p0, 0, sizeof(uint32_t) * std::max<size_t>(1, p.words), c->stream);
    if (e == hipSuccess && p.two) e = hipMemsetAsync(b.p1, 0, sizeof(uint32_t) * std::max<size_t>(1, p.words), c->stream);
    if (e == hipSuccess && p.stood) e = hipMemcpyAsync(b.aw, b.h_aw, shape.aw.size(), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess && s.pieces && !shape.tog.empty()) e = hipMemcpyAsync(b.tog, shape.tog.data(), sizeof(uint32_t) * shape.tog.size(), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess && p.count_occ) e = hipMemsetAsync(b.occ, 0, sizeof(uint32_t) * std::max<size_t>(1, p.occ_words), c->stream);
    if (e == hipSuccess && p.replay) e = enqueue_vax_replay(c, shape.trigger, p.t_done, b.vax);
    if (e != hipSuccess) return e;
    Series q;
    q.what = s.what; q.first = first_step; q.n_rows = n_rows; q.stride = stride; q.t_done = p.t_done; q.t_all = shape.t_all;
    q.vax_of = p.replay ? b.vax : nullptr; q.at_work = p.stood ? b.aw : nullptr; q.p0 = b.p0; q.p1 = p.two ? b.p1 : nullptr;
    q.n_cols = p.cols; q.key = s.key; q.grp = p.by_group ? c->grp.lab : nullptr; q.skip_bus = s.skip_bus;
    q.n_tog = s.pieces ? (uint32_t)shape.tog.size() : 0u; q.tog = s.pieces ? b.tog : nullptr;
    const uint32_t *occ0 = !p.sus ? nullptr : p.by_group ? c->grp.size : b.occ, *occ1 = p.sus && p.two ? b.occ + p.cols : nullptr;
    if (s.what != ESIM_VACCINATED)
        hipLaunchKernelGGL(k_series_log, dim3(grid_capped(c, p.log_len, TPB, 4096)), dim3(TPB), 0, c->stream, d, q, p.log_len);
    if (p.replay && (s.what == ESIM_VACCINATED || p.sus))         // (nobody is Vaccinated before a programme has run)
        hipLaunchKernelGGL(k_series_vax, dim3(grid_capped(c, d.n, TPB, 4096)), dim3(TPB), 0, c->stream, d, q);
    if (p.count_occ) hipLaunchKernelGGL(k_area_occupancy, dim3(grid_capped(c, d.n, TPB, 4096)), dim3(TPB), 0, c->stream, d, b.occ, p.two ? b.occ + p.cols : nullptr);
    if (!p.events)
        hipLaunchKernelGGL(k_series_prefix, dim3(grid_for(p.cols, TPB, 0xFFFFFFFFu)), dim3(TPB), 0, c->stream, q, occ0, occ1);
    return hipSuccess;
}

// The series behind their own argument checks: the engine's two halves in buffers that live as long as the call, the wait for
// the rows, and plane 0 copied out.
int series_rows(esim_ctx_impl *c, const SeriesSpec &s, uint32_t first_step, uint32_t n_rows, uint32_t stride, uint32_t *out)
{
    const std::string who = s.who;
    SeriesPlan p;
    if (int rc = series_plan(c, s, first_step, n_rows, stride, &p)) return rc;
    DevTmp<uint8_t> d_aw; DevTmp<uint32_t> d_vax, d_p0, d_p1, d_occ, d_tog;
    if (d_p0.alloc(p.words) != hipSuccess || (s.pieces && d_tog.alloc(p.shape.tog.size()) != hipSuccess) || (p.two && d_p1.alloc(p.words) != hipSuccess) || (p.stood && d_aw.alloc(p.shape.aw.size()) != hipSuccess) ||
        (p.count_occ && d_occ.alloc(p.occ_words) != hipSuccess) || (p.replay && d_vax.alloc(c->d.n) != hipSuccess)) {
        (void)hipGetLastError();
        return fail(c, ESIM_ENOMEM, who + ": no device memory for the rows (ask for fewer)");
    }
    const SeriesBufs b = { d_p0.p, d_p1.p, d_occ.p, d_tog.p, d_vax.p, d_aw.p, p.shape.aw.data() };
    hipError_t e = series_enqueue(c, s, first_step, n_rows, stride, p, b);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);     // (the host vectors above are done with here, too)
    else (void)hipStreamSynchronize(c->stream);
    if (e == hipSuccess && p.words) e = hipMemcpy(out, d_p0.p, sizeof(uint32_t) * p.words, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(c, ESIM_ENODEVICE, who + ": " + hipGetErrorString(e));
    return ESIM_OK;
}

// (where, what) of esim_ensemble_begin_series as the series entry point whose rows a member contributes.
SeriesSpec fold_spec(int where, int what)
{
    const char *who = "esim_ensemble_fold";
    if (where == ESIM_BY_GROUP) return {who, "status", KEY_GROUP, (uint32_t)what, false, false};                       // esim_group_series
    if (where == ESIM_AREA_CURRENT && what == (int)SERIES_EVENTS) return {who, "status", KEY_STOOD, SERIES_EVENTS, true, false};   // esim_area_series(EXPOSURES)
    return {who, "status", where == ESIM_AREA_CURRENT ? KEY_STOOD : KEY_HOME, (uint32_t)what, false, false};          // esim_area_status_series
}

// One member's rows, as the engine leaves them in the kept planes, folded into the accumulators of a series kind.
int fold_series(esim_ctx_impl *c)
{
    Rows &r = c->ens.rows;
    const Ensemble::Par &par = c->ens.par;
    const SeriesSpec s = fold_spec(c->ens.where, par.status);
    SeriesPlan p;
    if (int rc = series_plan(c, s, par.first, r.n_rows, par.stride, &p)) return rc;
    if (p.cols != r.n_cols || p.two != r.two) return fail(c, ESIM_ESTATE, "esim_ensemble_fold: the accumulators were begun for other columns");
    if (p.replay && !r.vax) {
        if (int rc = dev_alloc(c, &r.vax, c->d.n)) { (void)hipGetLastError(); return rc; }
    }
    if (p.stood) std::memcpy(c->pin.aw, p.shape.aw.data(), p.shape.aw.size());   // (the stream is idle behind series_plan's wait)
    const SeriesBufs b = { r.p0, r.p1, r.occ, nullptr, r.vax, r.aw, c->pin.aw };
    const hipError_t e = series_enqueue(c, s, par.first, r.n_rows, par.stride, p, b);
    if (e != hipSuccess) return fail(c, ESIM_ENODEVICE, std::string("esim_ensemble_fold: ") + hipGetErrorString(e));
    const uint64_t cells = (uint64_t)p.words;
    hipLaunchKernelGGL(k_ensemble_fold_rows, dim3(grid_capped(c, (size_t)(cells >> 2), TPB, 2048)), dim3(TPB), 0, c->stream,
                       r.p0, cells, par.min_hit, r.hit, r.sum, r.sumsq, r.members);
    HIP_TRY(c, members_keep(c));
    HIP_TRY(c, hipGetLastError());
    return ESIM_OK;
}

// One member's census, counted where the census calls count it, folded into the one row of the census kind.
int fold_census(esim_ctx_impl *c)
{
    const Ensemble &e = c->ens;
    const bool by_group = e.where == ESIM_BY_GROUP;
    HIP_TRY(c, hipSetDevice(c->P.device));
    if (int rc = by_group ? enqueue_group_census(c) : enqueue_area_census(c, e.where)) return rc;
    hipLaunchKernelGGL(k_ensemble_fold, dim3(grid_for(e.n, TPB, 0xFFFFFFFFu)), dim3(TPB), 0, c->stream,
                       by_group ? c->grp.cnt : c->area_cnt, e.n, e.par.status_mask, e.par.min_hit, e.rows.hit, e.rows.sum, e.rows.sumsq, e.rows.members);
    HIP_TRY(c, members_keep(c));
    HIP_TRY(c, hipGetLastError());
    return ESIM_OK;
}

// The same for the arrival kind: a member contributes its arrival steps, reached = arrival <= horizon.
int fold_arrival(esim_ctx_impl *c)
{
    const Ensemble &e = c->ens;
    HIP_TRY(c, hipSetDevice(c->P.device));
    if (int rc = enqueue_arrival(c, e.where)) return rc;
    hipLaunchKernelGGL(k_ensemble_fold_arrival, dim3(grid_for(e.n, TPB, 0xFFFFFFFFu)), dim3(TPB), 0, c->stream,
                       c->arrival, e.n, e.par.horizon, e.rows.hit, e.rows.sum, e.rows.sumsq, e.rows.members);
    HIP_TRY(c, members_keep(c));
    HIP_TRY(c, hipGetLastError());
    return ESIM_OK;
}

void burden_forget(esim_ctx_impl *c);      // (esim_host_burden.h: the severity tables dropped)
}  // namespace

extern "C" int esim_area_census(esim_ctx *ctx, int where, uint32_t *counts)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    if (!counts || (where != ESIM_AREA_CURRENT && where != ESIM_AREA_HOME)) return fail(c, ESIM_EINVAL, "esim_area_census: null output or unknown `where`");
    if (!c->uploaded) return fail(c, ESIM_ESTATE, "esim_area_census: no population uploaded");
    HIP_TRY(c, hipSetDevice(c->P.device));
    if (int rc = enqueue_area_census(c, where)) return rc;
    return census_readback(c, c->area_cnt, c->pin.area, (size_t)c->d.n_areas * 5u, counts);
}

// The step of the first exposure per Output Area (of the household) or per group, from the exposure log where it lies.
extern "C" int esim_area_arrival(esim_ctx *ctx, int where, uint32_t *step_out)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    if (!step_out) return fail(c, ESIM_EINVAL, "esim_area_arrival: null output");
    if (int rc = arrival_check(c, where, "esim_area_arrival")) return rc;
    HIP_TRY(c, hipSetDevice(c->P.device));
    if (int rc = enqueue_arrival(c, where)) return rc;
    const bool by_group = where == ESIM_BY_GROUP;
    HIP_TRY(c, hipGetLastError());
    return census_readback(c, c->arrival, by_group ? c->pin.grp : c->pin.area, by_group ? c->grp.n : c->d.n_areas, step_out);
}

// ---- per-Output-Area accumulators over the members of an ensemble ------------------------------------------------------
extern "C" int esim_ensemble_begin(esim_ctx *ctx, int where, uint32_t status_mask, uint32_t min_cases)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    if ((where != ESIM_AREA_CURRENT && where != ESIM_AREA_HOME && where != ESIM_BY_GROUP) || status_mask == 0u || (status_mask >> 5) != 0u)
        return fail(c, ESIM_EINVAL, "esim_ensemble_begin: unknown `where`, or a status mask that is empty or names a status beyond ESIM_VACCINATED");
    if (!c->uploaded) return fail(c, ESIM_ESTATE, "esim_ensemble_begin: no population uploaded");
    if (where == ESIM_BY_GROUP && (!c->grp.lab || c->comm.world > 1)) return fail(c, ESIM_ESTATE, "esim_ensemble_begin: by group without labels (esim_set_groups)");
    HIP_TRY(c, hipSetDevice(c->P.device));
    Ensemble::Par par;
    par.status_mask = status_mask; par.min_hit = min_cases;
    return ens_begin(c, "esim_ensemble_begin", Ensemble::ENS_CENSUS, where, 1u, where == ESIM_BY_GROUP ? c->grp.n : c->d.n_areas, par);
}

extern "C" int esim_ensemble_begin_arrival(esim_ctx *ctx, int where, uint32_t horizon)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    if (int rc = arrival_check(c, where, "esim_ensemble_begin_arrival")) return rc;
    HIP_TRY(c, hipSetDevice(c->P.device));
    Ensemble::Par par;
    par.horizon = horizon;
    return ens_begin(c, "esim_ensemble_begin_arrival", Ensemble::ENS_ARRIVAL, where, 1u, where == ESIM_BY_GROUP ? c->grp.n : c->d.n_areas, par);
}

extern "C" int esim_ensemble_read(esim_ctx *ctx, uint32_t *members, uint32_t *hit, uint64_t *sum, uint64_t *sumsq)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    return ens_read(c, READ_CELLS, 0u, 1u, members, { { hit, &Rows::hit } }, { { sum, &Rows::sum }, { sumsq, &Rows::sumsq } });
}

// ---- the same over the rows of a series: [n_rows][n_cols] accumulators, a member's rows left on the device ---------------
extern "C" int esim_ensemble_begin_series(esim_ctx *ctx, int where, int what, uint32_t first_step, uint32_t n_rows, uint32_t stride, uint32_t min_cases)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    if ((where != ESIM_AREA_CURRENT && where != ESIM_AREA_HOME && where != ESIM_BY_GROUP) || what < ESIM_SUSCEPTIBLE || what > (int)SERIES_EVENTS || stride == 0 || n_rows == 0)
        return fail(c, ESIM_EINVAL, "esim_ensemble_begin_series: unknown `where` or `what`, stride 0 or no rows");
    if (!c->uploaded) return fail(c, ESIM_ESTATE, "esim_ensemble_begin_series: no population uploaded");
    if (c->comm.world > 1) return fail(c, ESIM_ESTATE, "esim_ensemble_begin_series: the context has a communicator of several ranks (the rule of esim_restart)");
    if (where == ESIM_BY_GROUP && !c->grp.lab) return fail(c, ESIM_ESTATE, "esim_ensemble_begin_series: by group without labels (esim_set_groups)");
    if (first_step == 0) return fail(c, ESIM_ERANGE, "esim_ensemble_begin_series: first_step is 1-based");
    HIP_TRY(c, hipSetDevice(c->P.device));
    const SeriesSpec s = fold_spec(where, what);
    const uint32_t cols = where == ESIM_BY_GROUP ? c->grp.n : c->d.n_areas;
    const bool two = s.key == KEY_STOOD && s.what != SERIES_EVENTS;
    Ensemble::Par par;
    par.status = what; par.first = first_step; par.stride = stride; par.min_hit = min_cases;
    return ens_begin(c, "esim_ensemble_begin_series", Ensemble::ENS_SERIES, where, n_rows, cols, par, two);
}

extern "C" int esim_ensemble_read_series(esim_ctx *ctx, uint32_t first_row, uint32_t n, uint32_t *members, uint32_t *hit, uint64_t *sum, uint64_t *sumsq)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    return ens_read(c, READ_SERIES, first_row, n, members, { { hit, &Rows::hit } }, { { sum, &Rows::sum }, { sumsq, &Rows::sumsq } });
}

extern "C" int esim_area_series(esim_ctx *ctx, int what, uint32_t first_step, uint32_t n_rows, uint32_t stride, uint32_t *out)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    if (!out || (what != ESIM_SERIES_INFECTED && what != ESIM_SERIES_EXPOSURES) || stride == 0 || n_rows == 0)
        return fail(c, ESIM_EINVAL, "esim_area_series: null output, unknown `what`, stride 0 or no rows");
    if (!c->uploaded) return fail(c, ESIM_ESTATE, "esim_area_series: no population uploaded");
    // the Infected by the area stood in; building exposures by the area stood in at the exposure
    const SeriesSpec s = {"esim_area_series", "Infected", KEY_STOOD, what == ESIM_SERIES_INFECTED ? (uint32_t)ESIM_INFECTED : SERIES_EVENTS, true, what == ESIM_SERIES_INFECTED};
    return series_rows(c, s, first_step, n_rows, stride, out);
}

extern "C" int esim_area_status_series(esim_ctx *ctx, int where, int what, uint32_t first_step, uint32_t n_rows, uint32_t stride, uint32_t *out)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    const bool incidence = what == ESIM_AREA_SERIES_INCIDENCE;
    if (!out || (where != ESIM_AREA_HOME && (where != ESIM_AREA_CURRENT || incidence)) || what < ESIM_SUSCEPTIBLE || what > ESIM_AREA_SERIES_INCIDENCE ||
        stride == 0 || n_rows == 0)
        return fail(c, ESIM_EINVAL, "esim_area_status_series: null output, unknown `where` or `what` (incidence rows: by ESIM_AREA_HOME only), stride 0 or no rows");
    if (!c->uploaded) return fail(c, ESIM_ESTATE, "esim_area_status_series: no population uploaded");
    const SeriesSpec s = {"esim_area_status_series", "status", where == ESIM_AREA_CURRENT ? KEY_STOOD : KEY_HOME, (uint32_t)what, false, false};   // (INCIDENCE = SERIES_EVENTS)
    return series_rows(c, s, first_step, n_rows, stride, out);
}

// ---- read-backs by citizen group ---------------------------------------------------------------------------------------
extern "C" int esim_set_groups(esim_ctx *ctx, const uint16_t *group, uint32_t n_groups)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    if (!c->uploaded) return fail(c, ESIM_ESTATE, "esim_set_groups: no population uploaded");
    if (c->comm.world > 1) return fail(c, ESIM_ESTATE, "esim_set_groups: the context has a communicator of several ranks (sharded groups are not built)");
    HIP_TRY(c, hipSetDevice(c->P.device));
    const uint32_t N = c->d.n;
    std::vector<uint32_t> size;
    if (group) {
        if (n_groups == 0 || n_groups > ESIM_MAX_GROUPS) return fail(c, ESIM_EINVAL, "esim_set_groups: n_groups must be in 1..ESIM_MAX_GROUPS (1024)");
        size.assign(n_groups, 0u);
        for (uint32_t i = 0; i < N; ++i) {
            if (group[i] >= n_groups) return fail(c, ESIM_EINVAL, "esim_set_groups: a label is not below n_groups");
            size[group[i]]++;
        }
    }
    uint16_t *lab = nullptr; uint32_t *sz = nullptr, *cnt = nullptr;
    if (group) {
        int rc;
        if (!c->pin.grp) HIP_TRY(c, hipHostMalloc((void **)&c->pin.grp, sizeof(uint32_t) * ESIM_MAX_GROUPS * 5u, hipHostMallocDefault));
        if ((rc = dev_alloc(c, &lab, N)) || (rc = dev_alloc(c, &sz, n_groups)) || (rc = dev_alloc(c, &cnt, (size_t)n_groups * 5u))) {
            dev_free(c, lab); dev_free(c, sz); dev_free(c, cnt);
            return rc;
        }
        hipError_t e = N ? hipMemcpy(lab, group, sizeof(uint16_t) * (size_t)N, hipMemcpyHostToDevice) : hipSuccess;
        if (e == hipSuccess) e = hipMemcpy(sz, size.data(), sizeof(uint32_t) * n_groups, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            dev_free(c, lab); dev_free(c, sz); dev_free(c, cnt);
            return fail(c, ESIM_ENODEVICE, std::string("esim_set_groups: ") + hipGetErrorString(e));
        }
    }
    // the tables being replaced may still be read by work on the stream (a fold)
    if (c->grp.lab) HIP_TRY(c, hipStreamSynchronize(c->stream));
    dev_free(c, c->grp.lab); dev_free(c, c->grp.size); dev_free(c, c->grp.cnt);
    c->grp.lab = lab; c->grp.size = sz; c->grp.cnt = cnt; c->grp.n = group ? n_groups : 0u;
    c->grp.sizes = size;
    if (c->ens.where == ESIM_BY_GROUP) c->ens.valid = false;
    if (c->burden.set && c->burden.n_groups != 1u && c->burden.n_groups != c->grp.n) burden_forget(c);   // (tables per group of labels that are gone)
    return ESIM_OK;
}

extern "C" int esim_group_census(esim_ctx *ctx, uint32_t *counts)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    if (!counts) return fail(c, ESIM_EINVAL, "esim_group_census: null output");
    if (!c->uploaded || !c->grp.lab || c->comm.world > 1) return fail(c, ESIM_ESTATE, "esim_group_census: no population uploaded, or no labels (esim_set_groups)");
    HIP_TRY(c, hipSetDevice(c->P.device));
    if (int rc = enqueue_group_census(c)) return rc;
    return census_readback(c, c->grp.cnt, c->pin.grp, (size_t)c->grp.n * 5u, counts);
}

extern "C" int esim_group_series(esim_ctx *ctx, int what, uint32_t first_step, uint32_t n_rows, uint32_t stride, uint32_t *out)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    if (!out || what < ESIM_SUSCEPTIBLE || what > ESIM_GROUP_SERIES_EXPOSURES || stride == 0 || n_rows == 0)
        return fail(c, ESIM_EINVAL, "esim_group_series: null output, unknown `what`, stride 0 or no rows");
    if (!c->uploaded || !c->grp.lab || c->comm.world > 1) return fail(c, ESIM_ESTATE, "esim_group_series: no population uploaded, or no labels (esim_set_groups)");
    const SeriesSpec s = {"esim_group_series", "status", KEY_GROUP, (uint32_t)what, false, false};   // (EXPOSURES = SERIES_EVENTS)
    return series_rows(c, s, first_step, n_rows, stride, out);
}
