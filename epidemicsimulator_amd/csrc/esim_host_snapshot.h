// esim_host_snapshot.h -- forecast ensembles: esim_snapshot keeps the state at rest on the device, esim_rollback goes back to it
// under other parameters; esim_snapshot_info, esim_snapshot_drop.  What a snapshot holds is what a checkpoint holds
// (esim_host_ckpt.h): the control block, hist, log_off, the citizen words, the exposure log, exp_step and the records.
namespace {

// What esim_snapshot and esim_rollback refuse alike.
int snapshot_check(esim_ctx_impl *c, const std::string &who)
{
    if (!c->uploaded) return fail(c, ESIM_ESTATE, who + ": no population uploaded");
    if (c->comm.world > 1) return fail(c, ESIM_ESTATE, who + ": the context has a communicator of several ranks (sharded snapshots are not built)");
    return ESIM_OK;
}

// The control block as a context at rest at that step starts from it: the normalisation of esim_checkpoint_restore.
void ctrl_at_rest(Ctrl *h)
{
    h->chunk_ok = 0; h->chunk_parallel = 0; h->chunk_done = 0; h->n_items = 0; h->n_newexp = 0; h->n_units = 0; h->unit_next = 0;
    h->n_route_pairs_big = 0; h->prev_n_items = 0; h->prev_per_wave = 0; h->items_per_wave = 0; h->small_done = 0;
    h->future_t0 = 0; h->n_riders = 0; h->peer_error = 0;
    for (int z = 0; z < 5; ++z) h->counts[z] = 0;
    for (uint32_t z = 0; z < MARK_SLOTS; ++z) { h->n_touched_bld[z] = 0; h->n_touched_room[z] = 0; h->n_touched_route[z] = 0; h->n_touched_route_big[z] = 0; }
}

// The snapshot's buffers: allocated at the first snapshot and kept; the log's prefix grows when a snapshot needs more (the old
// one goes back through the context's allocation list: hipFree waits for the work that still reads it).  Nothing of the
// context changes when an allocation fails.
int snapshot_room(esim_ctx_impl *c, uint32_t log_len)
{
    Snapshot &s = c->snap;
    if (!s.words) {
        uint32_t *w = nullptr, *hi = nullptr, *lo = nullptr, *ex = nullptr; esim_step_result *re = nullptr;
        int rc;
        if ((rc = dev_alloc(c, &w, c->d.n)) || (rc = dev_alloc(c, &hi, TE_SLOTS)) || (rc = dev_alloc(c, &lo, TE_SLOTS + 1u)) ||
            (rc = dev_alloc(c, &ex, 2u * ((size_t)c->cap_steps + 2u))) || (rc = dev_alloc(c, &re, (size_t)c->cap_steps + 1u))) {
            dev_free(c, w); dev_free(c, hi); dev_free(c, lo); dev_free(c, ex); dev_free(c, re);
            (void)hipGetLastError();
            return rc;
        }
        s.words = w; s.hist = hi; s.log_off = lo; s.exp_step = ex; s.records = re;
    }
    if (log_len > s.log_cap || !s.log) {
        uint32_t *grown = nullptr;
        if (int rc = dev_alloc(c, &grown, log_len)) { (void)hipGetLastError(); return rc; }
        dev_free(c, s.log);
        s.log = grown; s.log_cap = log_len;
    }
    return ESIM_OK;
}

void launch_words(esim_ctx_impl *c, uint32_t *dst, const uint32_t *src)
{
    if (c->d.n) hipLaunchKernelGGL(k_snapshot_words, dim3(grid_capped(c, ((size_t)c->d.n + 3u) / 4u, TPB, 2048)), dim3(TPB), 0, c->stream, dst, src, c->d.n);
}

// bytes of the prefixes a state at rest with host_t as its next step has written (what esim_checkpoint_save pulls)
size_t exp_prefix(uint32_t host_t) { return sizeof(uint32_t) * 2u * ((size_t)host_t + 1u); }
size_t rec_prefix(uint32_t host_t) { return sizeof(esim_step_result) * (size_t)host_t; }

}  // namespace

extern "C" int esim_snapshot(esim_ctx *ctx)
{
    esim_ctx_impl *c = CTX(ctx);
    if (!c) return fail(c, ESIM_EINVAL, "esim_snapshot: null argument");
    if (int rc = snapshot_check(c, "esim_snapshot")) return rc;
    if (c->host_t <= 1u) return fail(c, ESIM_ESTATE, "esim_snapshot: no step has run (step 0 is what esim_restart rebuilds)");
    if (c->seam.step) return fail(c, ESIM_ESTATE, "esim_snapshot: the run was branched from a snapshot under another seed or vaccination_rate; a history mixed twice is not built");
    HIP_TRY(c, hipSetDevice(c->P.device));
    // The control block at rest: esim_run and esim_step leave it in the pinned mirror, so nothing is read back here.  After
    // any other way to this step (a checkpoint restore, an injected error) it is read once, 200 bytes.
    if (c->rest_t != c->host_t) {
        Ctrl now;
        if (int rc = read_ctrl(c, &now)) return rc;
        c->rest_t = c->host_t;
    }
    Ctrl h = *c->pin.ctrl;
    if (h.error) return fail(c, ESIM_ESTATE, "esim_snapshot: a device-side error is pending on this context (code " + std::to_string(-(int)h.error) + ")");
    if (h.t != c->host_t || h.log_len > c->d.n) return fail(c, ESIM_ESTATE, "esim_snapshot: the control block is not the one of a context at rest at this step");
    if (int rc = snapshot_room(c, h.log_len)) return rc;
    Snapshot &s = c->snap;
    const Dev &d = c->d;
    const uint32_t host_t = c->host_t;
    s.step = 0;                                                     // (whatever fails below leaves no snapshot)
    launch_words(c, s.words, d.cit);
    HIP_TRY(c, hipMemcpyAsync(s.hist, d.hist, sizeof(uint32_t) * TE_SLOTS, hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(s.log_off, d.log_off, sizeof(uint32_t) * (TE_SLOTS + 1u), hipMemcpyDeviceToDevice, c->stream));
    if (h.log_len) HIP_TRY(c, hipMemcpyAsync(s.log, d.log, sizeof(uint32_t) * (size_t)h.log_len, hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(s.exp_step, d.exp_step, exp_prefix(host_t), hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(s.records, d.records, rec_prefix(host_t), hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(c, hipGetLastError());
    ctrl_at_rest(&h);
    s.h = h; s.P = c->P;
    s.last_chunk_pairs = c->last_chunk_pairs; s.quiet = c->quiet; s.repair_armed = c->repair_armed; s.elig_seen = c->elig_seen || h.have_elig != 0u;
    s.vax_chunk_steps = c->vax_chunk_steps; s.vax_chunk_cuts = c->vax_chunk_cuts; s.vax_chunk_repairs = c->vax_chunk_repairs;
    s.step = host_t - 1u;
    c->snap_draw_seam = c->draw_seam;
    return ESIM_OK;
}

extern "C" int esim_rollback(esim_ctx *ctx, const esim_params *p)
{
    esim_ctx_impl *c = CTX(ctx);
    if (!c) return fail(c, ESIM_EINVAL, "esim_rollback: null argument");
    const std::string who = "esim_rollback";
    if (int rc = snapshot_check(c, who)) return rc;
    Snapshot &s = c->snap;
    if (!s.step) return fail(c, ESIM_ESTATE, who + ": no snapshot (esim_snapshot; esim_upload_population, esim_restart_seeded and esim_snapshot_drop drop it)");
    const esim_params q = p ? *p : s.P;
    if (int rc = check_params(c, &q, who)) return rc;
    if (q.device != c->P.device) return fail(c, ESIM_EINVAL, who + ": device must be the context's device");
    if (q.exposed_time != s.P.exposed_time || q.infected_time != s.P.infected_time || q.start_hour != s.P.start_hour || q.end_hour != s.P.end_hour)
        return fail(c, ESIM_EINVAL, who + ": exposed_time, infected_time and the working hours must be the snapshot's (the state is a function of them)");
    if (q.max_steps > c->cap_steps) return fail(c, ESIM_ERANGE, who + ": max_steps above the max_steps the context was created with (the record log's capacity)");
    if (q.max_steps < s.step) return fail(c, ESIM_ERANGE, who + ": max_steps below the snapshot's step");
    HIP_TRY(c, hipSetDevice(c->P.device));
    // the staging block is the source of the previous restart's or rollback's copies (restart_enqueue)
    if (c->rs.ev_used) HIP_TRY(c, hipEventSynchronize(c->rs.ev));
    c->P = q;
    params_to_dev(c);
    // (esim_reset's copy of the seeds' words: an esim_restart since the snapshot may have left them under other times)
    for (uint32_t sc : c->init_log) c->init_state[sc] = CW_MAKE(seed_te(c), c->init_state[sc] & CW_FLAGS);
    const Dev &d = c->d;
    const uint32_t host_t = s.step + 1u;
    Ctrl &h = c->rs.stage->h;
    h = s.h;
    esim_threshold_lut(&c->P, c->rs.stage->lut);
    HIP_TRY(c, hipMemcpyAsync(d.ctrl, &h, sizeof h, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(const_cast<uint64_t *>(d.thr), c->rs.stage->lut, sizeof c->rs.stage->lut, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipEventRecord(c->rs.ev, c->stream));
    c->rs.ev_used = true;
    launch_words(c, d.cit, s.words);
    HIP_TRY(c, hipMemsetAsync(c->cnt_base, 0, c->cnt_bytes, c->stream));
    // exp_step is added to, not written, by the steps: what the abandoned future left behind the snapshot's step goes; its
    // records go with it (nothing reads them before they are written again, but a read-back beyond the steps run would)
    HIP_TRY(c, hipMemsetAsync(d.exp_step, 0, sizeof(uint32_t) * 2 * ((size_t)c->cap_steps + 2), c->stream));
    HIP_TRY(c, hipMemsetAsync(d.records, 0, sizeof(esim_step_result) * ((size_t)c->cap_steps + 1), c->stream));
    HIP_TRY(c, hipMemcpyAsync(d.exp_step, s.exp_step, exp_prefix(host_t), hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d.records, s.records, rec_prefix(host_t), hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d.hist, s.hist, sizeof(uint32_t) * TE_SLOTS, hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d.log_off, s.log_off, sizeof(uint32_t) * (TE_SLOTS + 1u), hipMemcpyDeviceToDevice, c->stream));
    if (s.h.log_len) HIP_TRY(c, hipMemcpyAsync(d.log, s.log, sizeof(uint32_t) * (size_t)s.h.log_len, hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(c, hipGetLastError());
    // the host's view set to match: what it was when the snapshot was taken, so that the branch is scheduled as the run itself was
    rewind_host(c);
    c->stop_flag_dev = s.h.stop_when_done;                          // (the snapshot's flag is now the device's: esim_run compares against it)
    c->host_t = host_t;
    c->last_chunk_pairs = s.last_chunk_pairs; c->quiet = s.quiet; c->repair_armed = s.repair_armed; c->elig_seen = s.elig_seen;
    c->vax_chunk_steps = s.vax_chunk_steps; c->vax_chunk_cuts = s.vax_chunk_cuts; c->vax_chunk_repairs = s.vax_chunk_repairs;
    if (q.seed != s.P.seed || q.vaccination_rate != s.P.vaccination_rate) { c->seam.step = s.step; c->seam.seed = s.P.seed; c->seam.rate = s.P.vaccination_rate; }
    // the draw seam (rewind_host cleared it): the one the snapshot's own history has, if any, and one at the snapshot's step when
    // the branch draws its exposures under other values than the snapshot's
    const bool redrawn = q.seed != s.P.seed || q.exposure_chance != s.P.exposure_chance || q.mask_effectiveness != s.P.mask_effectiveness;
    c->draw_seam = c->snap_draw_seam;
    if (redrawn && c->draw_seam.step) c->draw_seam.twice = true;
    else if (redrawn) { c->draw_seam.step = s.step; c->draw_seam.seed = s.P.seed; c->draw_seam.chance = s.P.exposure_chance; c->draw_seam.mask_effectiveness = s.P.mask_effectiveness; }
    if (q.bus_capacity != s.P.bus_capacity) c->draw_seam.two_capacities = true;
    return ESIM_OK;
}

extern "C" int esim_snapshot_info(esim_ctx *ctx, uint32_t *step, esim_params *p)
{
    esim_ctx_impl *c = CTX(ctx);
    if (!c) return fail(c, ESIM_EINVAL, "esim_snapshot_info: null argument");
    if (step) *step = c->snap.step;
    if (p) { if (c->snap.step) *p = c->snap.P; else std::memset(p, 0, sizeof *p); }
    return ESIM_OK;
}

extern "C" int esim_snapshot_drop(esim_ctx *ctx)
{
    esim_ctx_impl *c = CTX(ctx);
    if (!c) return fail(c, ESIM_EINVAL, "esim_snapshot_drop: null argument");
    Snapshot &s = c->snap;
    if (s.words) {
        // the buffers may still be read or written by work on the stream (the snapshot's own copies, a rollback's)
        if (int rc = drain(c)) return rc;
        for (void *q : { (void *)s.words, (void *)s.hist, (void *)s.log_off, (void *)s.exp_step, (void *)s.records, (void *)s.log }) dev_free(c, q);
    }
    s = Snapshot();
    c->snap_draw_seam = DrawSeam();
    return ESIM_OK;
}
