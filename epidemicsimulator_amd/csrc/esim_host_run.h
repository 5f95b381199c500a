// esim_host_run.h -- the step scheduler: sequential steps, the chunk pass's launchers and forms, bursts; esim_step, esim_run.
namespace {

int enqueue_begin(esim_ctx_impl *c, bool time_kernel)
{
    Dev &d = c->d;
    if (c->tm.phase) HIP_TRY(c, hipEventRecord(c->tm.ev[0], c->stream));
    if (time_kernel) HIP_TRY(c, hipEventRecord(c->tm.kev[c->tm.kev_used + 0], c->stream));
    hipLaunchKernelGGL(k_infected, dim3(c->tune.grid_infected), dim3(TPB), 0, c->stream, d);
    if (d.n_shards > 1) {
        const uint32_t n = (uint32_t)std::max<size_t>(XA_HEADER, std::max(d.n_shared_bld, d.n_shared_room));
        hipLaunchKernelGGL(k_pack_a, dim3(grid_for(n, TPB, 1u << 20)), dim3(TPB), 0, c->stream, d);
    }
    if (c->tm.phase) HIP_TRY(c, hipEventRecord(c->tm.ev[1], c->stream));
    return ESIM_OK;
}

int enqueue_exposures(esim_ctx_impl *c)
{
    Dev &d = c->d;
    if (d.n_shards > 1) {
        const uint32_t n = (uint32_t)std::max<size_t>(XA_HEADER, std::max(d.n_shared_bld, d.n_shared_room));
        hipLaunchKernelGGL(k_unpack_a, dim3(grid_for(n, TPB, 1u << 20)), dim3(TPB), 0, c->stream, d);
    }
    hipLaunchKernelGGL(k_expose, dim3(c->tune.grid_expose), dim3(TPB), 0, c->stream, d);
    if (d.n_shards > 1) hipLaunchKernelGGL(k_pack_b, dim3(VACC_WINDOW / TPB), dim3(TPB), 0, c->stream, d);
    if (c->tm.phase) HIP_TRY(c, hipEventRecord(c->tm.ev[2], c->stream));
    return ESIM_OK;
}

int enqueue_finish(esim_ctx_impl *c, bool time_kernel, int mode = -1)
{
    Dev &d = c->d;
    if (mode < 0) mode = d.n_shards > 1 ? 1 : 0;
    hipLaunchKernelGGL(k_finish, dim3(1), dim3(FIN_TPB), 0, c->stream, d, mode);
    if (time_kernel) { HIP_TRY(c, hipEventRecord(c->tm.kev[c->tm.kev_used + 1], c->stream)); c->tm.kev_used += 2; }
    if (c->tm.phase) {
        HIP_TRY(c, hipEventRecord(c->tm.ev[3], c->stream));
        HIP_TRY(c, hipEventSynchronize(c->tm.ev[3]));
        float ms;
        for (int i = 0; i < 3; ++i) { HIP_TRY(c, hipEventElapsedTime(&ms, c->tm.ev[i], c->tm.ev[i + 1])); c->tm.phase_s[i] += ms * 1e-3; }
    }
    c->host_t++;
    HIP_TRY(c, hipGetLastError());
    return ESIM_OK;
}

int check_budget(esim_ctx_impl *c, uint32_t n_steps)
{
    if (!c || !c->uploaded) return fail(c, ESIM_ESTATE, "no population uploaded");
    if ((uint64_t)c->host_t + n_steps - 1 > c->P.max_steps)
        return fail(c, ESIM_ERANGE, "step budget exhausted: max_steps reached (DiseaseModel::max_time_step)");
    return ESIM_OK;
}

bool want_kernel_timing(esim_ctx_impl *c)
{
    Timing &t = c->tm;
    if (!t.kernel || (c->host_t % t.stride) != 0) return false;
    if (t.kev_used + 2 > t.kev.size()) {
        for (int i = 0; i < 2; ++i) { hipEvent_t e; if (hipEventCreate(&e) != hipSuccess) return false; t.kev.push_back(e); }
    }
    return true;
}

// Per-kernel timing of the chunk pass: an event in front of every kernel (kind = which one), ESIM_CK_N closes a sequence.
// kd_resolve turns consecutive events into durations once the stream has drained.
void kd_mark(esim_ctx_impl *c, int kind)
{
    Timing &t = c->tm;
    if (!t.kdetail) return;
    if (t.kd_used == t.kdev.size()) { hipEvent_t e; if (hipEventCreate(&e) != hipSuccess) return; t.kdev.push_back(e); t.kd_kind.push_back(0); }
    if (hipEventRecord(t.kdev[t.kd_used], c->stream) != hipSuccess) return;
    t.kd_kind[t.kd_used++] = kind;
}

void kd_resolve(esim_ctx_impl *c)
{
    Timing &t = c->tm;
    for (size_t i = 0; i + 1 < t.kd_used; ++i) {
        if (t.kd_kind[i] >= ESIM_CK_N) continue;
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, t.kdev[i], t.kdev[i + 1]) == hipSuccess) { t.kd_ms[t.kd_kind[i]] += ms; t.kd_calls[t.kd_kind[i]]++; }
    }
    t.kd_used = 0;
}

// The device time of chunk passes (esim_chunk_timing), while kernel timing is on: an event in front of what is enqueued and one
// behind it; the caller reads the time between them once the stream has passed the second.
int chunk_time_begin(esim_ctx_impl *c) { if (c->tm.kernel) { Timing::make_pair(c->tm.cev); HIP_TRY(c, hipEventRecord(c->tm.cev[0], c->stream)); } return ESIM_OK; }
int chunk_time_end(esim_ctx_impl *c) { if (c->tm.kernel) HIP_TRY(c, hipEventRecord(c->tm.cev[1], c->stream)); return ESIM_OK; }

// After a burst of chunk passes that started at step `first` and can have advanced `span` steps at most: the control block and
// the records of those steps come back with one wait (esim_run hands the records on from the mirror).
int burst_readback(esim_ctx_impl *c, uint32_t first, uint32_t span, Ctrl *h)
{
    const Dev &d = c->d;
    Pinned &pin = c->pin;
    ht_mark(c, "kernels enqueued");
    HIP_TRY(c, hipMemcpyAsync(pin.ctrl, d.ctrl, sizeof(Ctrl), hipMemcpyDeviceToHost, c->stream));
    const bool rec = pin.track && first == pin.first + pin.valid && (size_t)first + span <= pin.rec_n;
    if (rec) HIP_TRY(c, hipMemcpyAsync(pin.rec + first, d.records + first, sizeof(esim_step_result) * span, hipMemcpyDeviceToHost, c->stream));
    ht_mark(c, "copies enqueued");
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    ht_mark(c, "stream drained");
    *h = *pin.ctrl;
    if (rec && h->t >= first) pin.valid += std::min<uint32_t>(h->t - first, span);
    pin.ctrl_fresh = true;
    if (c->tm.kdetail) kd_resolve(c);
    return ESIM_OK;
}

// Sequential steps (three kernels per step, or the persistent single-workgroup kernel while few citizens
// are Infected): the only form that can vaccinate.
int run_sequential(esim_ctx_impl *c, uint32_t n_steps, bool allow_early_stop, uint32_t *executed)
{
    Dev &d = c->d; Timing &t = c->tm;
    c->pin.ctrl_fresh = false;               // (whatever a burst read back is out of date once more steps are enqueued)
    c->quiet = false;
    uint32_t remaining = n_steps, total = 0; int rc;
    const bool persistent = c->tune.small_max > 0 && !t.phase;
    while (remaining > 0) {
        if (persistent) {
            if (t.kernel) { Timing::make_pair(t.sev); HIP_TRY(c, hipEventRecord(t.sev[0], c->stream)); }
            hipLaunchKernelGGL(k_small, dim3(1), dim3(FIN_TPB), 0, c->stream, d, remaining, c->tune.small_max, 0);
            if (t.kernel) HIP_TRY(c, hipEventRecord(t.sev[1], c->stream));
            Ctrl h;
            if ((rc = read_ctrl(c, &h))) return rc;
            if (t.kernel && h.small_done) { float ms; HIP_TRY(c, hipEventElapsedTime(&ms, t.sev[0], t.sev[1])); t.small_ms += ms; t.small_steps += h.small_done; }
            c->host_t += h.small_done; total += h.small_done; remaining -= h.small_done;
            if ((rc = ctrl_error(c, h))) return rc;
            if (h.finished && allow_early_stop) break;
        }
        if (remaining == 0) break;
        const uint32_t chunk = std::min<uint32_t>(remaining, persistent ? 32u : remaining);
        for (uint32_t s = 0; s < chunk; ++s) {
            const bool tk = want_kernel_timing(c);
            if ((rc = enqueue_begin(c, tk))) return rc;
            if ((rc = enqueue_exposures(c))) return rc;
            if ((rc = enqueue_finish(c, tk, 0))) return rc;
        }
        total += chunk; remaining -= chunk;
    }
    if (executed) *executed = total;
    return ESIM_OK;
}

// A chunk with few Infected is nothing but the latency of its kernels: those run on 64 workgroups instead of 1024 then (measured
// on york, whose chunks are all of that kind: 3.56 instead of 4.0 ms for the 5000 steps).  The choice follows what the last
// read-back showed, so bursts are kept short while it is in force (the epidemic may double within a hundred steps).
bool tiny_chunk(const esim_ctx_impl *c) { return c->tune.tiny_pairs && c->last_chunk_pairs <= c->tune.tiny_pairs && c->d.world == 1u && c->d.n_shards == 1u; }
bool small_chunk(const esim_ctx_impl *c) { return c->tune.small_grid && c->last_chunk_pairs < 4096u && c->tune.grid_chunk > c->tune.small_grid && !c->tune.grid_chunk_env; }

// ---- the kernels of one time-parallel chunk.  They take the chunk (first step, length, whether it may run this way) from the
// control block as k_decide left it, and do nothing when it may not.  Each kernel's launch configuration stands in its
// launcher here and nowhere else; a launcher places the event of esim_enable_chunk_kernel_timing in front of its kernel.
// Sharded chunks place none (kd false): nothing resolves the events there.
struct ChunkPass {
    esim_ctx_impl *c;
    uint32_t limit_t;             // the last step the call may run
    bool kd;
    uint32_t n_ahead() const { return (uint32_t)c->xf_n; }
    void mark(int kind) const { if (kd) kd_mark(c, kind); }
    // the Infected census of the next n steps; their decisions and how many of them form the chunk (parallel: one pass may draw it)
    void future(uint32_t n) const { mark(ESIM_CK_FUTURE); hipLaunchKernelGGL(k_future, dim3(1), dim3(FIN_TPB), 0, c->stream, c->d, n, limit_t); }
    void decide(uint32_t n, int parallel, int vax_in_census) const { mark(ESIM_CK_DECIDE); hipLaunchKernelGGL(k_decide, dim3(1), dim3(64), 0, c->stream, c->d, n, limit_t, parallel, vax_in_census); }
    // the plan of the chunk's vaccinations; unsharded, one more workgroup makes the census ahead (a sharded chunk's k_future has)
    void vax_plan(int sharded) const { mark(ESIM_CK_VAX); hipLaunchKernelGGL(k_chunk_vax<false>, dim3(FREE_MAX + (sharded ? 0u : 1u)), dim3(FIN_TPB), 0, c->stream, c->d, n_ahead(), limit_t, sharded); }
    // bus exposures of citizens the plan vaccinates later: lost finds them, vax_repair walks the plan again (one ESIM_CK_VAX_REPAIR)
    void lost() const { mark(ESIM_CK_VAX_REPAIR); hipLaunchKernelGGL(k_chunk_lost, dim3(1), dim3(FIN_TPB), 0, c->stream, c->d); }
    void vax_repair(int sharded) const { hipLaunchKernelGGL(k_chunk_vax<true>, dim3(FREE_MAX), dim3(FIN_TPB), 0, c->stream, c->d, n_ahead(), limit_t, sharded); }
    // marks -> fold -> draw -> units: the item map is built by k_chunk_marks and torn down by k_chunk_scatter (few: small_chunk's grids)
    void front(bool few) const
    {
        const Tuning &t = c->tune;
        const uint32_t g = few ? t.small_grid : t.grid_chunk, g_draw = g * (few ? t.small_mult : t.draw_mult), g_units = g * (few ? t.small_mult : t.units_mult);
        mark(ESIM_CK_MARKS); hipLaunchKernelGGL(k_chunk_marks, dim3(g), dim3(TPB), 0, c->stream, c->d);
        mark(ESIM_CK_FOLD); hipLaunchKernelGGL(k_chunk_fold, dim3(g), dim3(TPB), 0, c->stream, c->d);
        mark(ESIM_CK_DRAW); hipLaunchKernelGGL(k_chunk_draw, dim3(g_draw), dim3(TPB), 0, c->stream, c->d, g * (TPB / 64u));
        mark(ESIM_CK_UNITS); hipLaunchKernelGGL(k_chunk_units, dim3(g_units), dim3(TPB), 0, c->stream, c->d);
    }
    // (k_chunk_count and k_chunk_scatter run on the same grid: their workgroups pair up)
    void count() const { mark(ESIM_CK_COUNT); hipLaunchKernelGGL(k_chunk_count, dim3(COUNT_GRID), dim3(TPB), 0, c->stream, c->d); }
    void scatter() const { mark(ESIM_CK_SCATTER); hipLaunchKernelGGL(k_chunk_scatter, dim3(COUNT_GRID), dim3(TPB), 0, c->stream, c->d); }
    // the books of the chunk.  alone (0 / 1): the counts, the log scatter and the clean-up too, in this one workgroup; then_next
    // (0 / 1): also prepare the chunk after it (census ahead + decisions: what k_future and k_decide do), for steps up to limit_t
    void books(int alone, int then_next) const { mark(ESIM_CK_BOOKS); hipLaunchKernelGGL(k_chunk_books, dim3(1), dim3(FIN_TPB), 0, c->stream, c->d, alone, then_next, n_ahead(), limit_t); }
    void vax_final() const { mark(ESIM_CK_VAX_FINAL); hipLaunchKernelGGL(k_chunk_vax_final, dim3(FREE_MAX), dim3(TPB), 0, c->stream, c->d); }
};

// One time-parallel chunk while no vaccination programme runs.  While few citizens are Infected the books, the log scatter,
// the clean-up and the preparation of the next chunk are ONE single-workgroup kernel (a kernel boundary costs more than these
// steps); with many, the scatter and clean-up need the whole chip.
void enqueue_parallel_chunk(esim_ctx_impl *c, int then_next, uint32_t limit_t)
{
    const ChunkPass p{ c, limit_t, true };
    const bool alone = c->last_chunk_pairs < 1024u;
    p.front(small_chunk(c));
    if (!alone) p.count();
    p.books(alone ? 1 : 0, then_next);
    if (!alone) p.scatter();
    p.mark(ESIM_CK_N);
}

// One time-parallel chunk under a vaccination programme: census ahead, the plan of the chunk's vaccinations and what it does
// to the Infected census, the decisions, then the pass itself in its wide form.  Every kernel takes the chunk from the
// control block; a chunk that cannot run (no plan possible, a step that must run sequentially first) is a no-op.
void enqueue_vax_chunk(esim_ctx_impl *c, uint32_t limit_t)
{
    const ChunkPass p{ c, limit_t, true };
    const Tuning &t = c->tune;
    // Nobody is Exposed or Infected any more (the last read-back said so, and nobody is infected from outside): what is left of the
    // run is the vaccination programme.  No marks, no draws, nothing to scatter: the plan, the decisions, the census the
    // vaccinations move, the books, the words (York: the last 3400 of its 5000 steps are of this kind).
    const bool quiet = c->quiet && c->d.world == 1u;
    p.vax_plan(0);
    p.decide(p.n_ahead(), 1, 0);
    if (!quiet) {
        p.front(small_chunk(c));
        if (c->d.world == 1u && t.vax_repair && (c->repair_armed || t.vax_repair_always)) { p.lost(); p.vax_repair(0); }
    }
    p.count();
    p.books(0, 0);
    if (!quiet) p.scatter();
    p.vax_final();
    p.mark(ESIM_CK_N);
}

// A burst of chunks without a programme: the census ahead and the decisions of the first, then every chunk prepares its successor.
void enqueue_free_burst(esim_ctx_impl *c, uint32_t bursts, uint32_t limit_t)
{
    const ChunkPass p{ c, limit_t, true };
    if (tiny_chunk(c)) {
        // few Infected: every chunk of the burst is ONE launch of one workgroup (esim_kernels_tiny.h); a chunk that has
        // outgrown that form does not advance, which the read-back sees
        for (uint32_t g = 0; g < bursts; ++g) {
            p.mark(ESIM_CK_TINY);
            hipLaunchKernelGGL(k_chunk_tiny, dim3(1), dim3(FIN_TPB), 0, c->stream, c->d, g == 0u ? 1 : 0, g + 1u < bursts ? 1 : 0, p.n_ahead(), limit_t);
        }
        p.mark(ESIM_CK_N);
        return;
    }
    p.future(p.n_ahead());
    p.decide(p.n_ahead(), 1, 0);
    for (uint32_t g = 0; g < bursts; ++g) enqueue_parallel_chunk(c, g + 1u < bursts ? 1 : 0, limit_t);
}

// One pipelined chunk.  Precondition: k_future ran for the current step.  k_decide finds how many of the next n_ahead
// steps can run before a vaccination programme would start; those run as one k_pipe each and k_batch_finish writes their
// books.  *executed = steps run.
int run_chunk(esim_ctx_impl *c, uint32_t n_ahead, uint32_t *executed, Ctrl *state_before)
{
    Dev &d = c->d; Timing &t = c->tm;
    c->pin.ctrl_fresh = false;
    ChunkPass{ c, c->P.max_steps, false }.decide(n_ahead, c->tune.time_parallel ? 1 : 0, 0);
    Ctrl h; int rc;
    if ((rc = read_ctrl(c, &h))) return rc;
    *state_before = h;
    if ((rc = ctrl_error(c, h))) return rc;
    const uint32_t n = h.chunk_ok, t0 = h.t;
    c->last_chunk_pairs = h.chunk_pairs;
    *executed = 0;
    if (n == 0) return ESIM_OK;
    if (h.chunk_parallel) {
        // every step of the chunk in one pass: marks of all steps, draws of all (item, step) pairs, then the books
        if ((rc = chunk_time_begin(c))) return rc;
        enqueue_parallel_chunk(c, 0, 0u);
        if ((rc = chunk_time_end(c))) return rc;
        if (t.kernel) { float ms; HIP_TRY(c, hipEventSynchronize(t.cev[1])); HIP_TRY(c, hipEventElapsedTime(&ms, t.cev[0], t.cev[1])); t.chunk_ms += ms; }
        HIP_TRY(c, hipGetLastError());
        // (what was executed is read, not assumed)
        Ctrl after;
        if ((rc = read_ctrl(c, &after)) || (rc = ctrl_error(c, after))) return rc;
        const uint32_t ran = after.t - t0;
        t.chunk_steps += ran; t.chunk_count += ran ? 1u : 0u;      // (this form counts its steps whether it is timed or not)
        *executed = ran;
        return ESIM_OK;
    }
    hipLaunchKernelGGL(k_infected_dec, dim3(c->tune.grid_infected), dim3(TPB), 0, c->stream, d, t0, 0u);
    for (uint32_t j = 0; j < n; ++j) {
        bool tk = t.kernel && ((t0 + j) % t.stride) == 0;
        if (tk && t.pkev_used + 2 > t.pkev.size())
            for (int i = 0; i < 2 && tk; ++i) { hipEvent_t e; if (hipEventCreate(&e) != hipSuccess) tk = false; else t.pkev.push_back(e); }
        if (tk) HIP_TRY(c, hipEventRecord(t.pkev[t.pkev_used], c->stream));
        hipLaunchKernelGGL(k_pipe, dim3(c->tune.grid_expose + c->tune.grid_infected), dim3(TPB), 0, c->stream, d, t0 + j, j, c->tune.grid_expose, j + 1 < n ? 1 : 0);
        if (tk) { HIP_TRY(c, hipEventRecord(t.pkev[t.pkev_used + 1], c->stream)); t.pkev_used += 2; }
    }
    hipLaunchKernelGGL(k_batch_finish, dim3(1), dim3(FIN_TPB), 0, c->stream, d, t0, n);
    HIP_TRY(c, hipGetLastError());
    t.pipe_steps += n;
    *executed = n;
    return ESIM_OK;
}

// One burst of `bursts` chunk passes (planned ones under a programme: vax) from the step the host stands at: they go on the
// stream, the control block and the records come back with one wait, the host moves on to the step the device reached (*done more).
int run_burst(esim_ctx_impl *c, uint32_t remaining, uint32_t bursts, bool vax, Ctrl *h, uint32_t *done)
{
    const uint32_t first = c->host_t, limit_t = first + remaining - 1u, n_ahead = (uint32_t)c->xf_n;
    int rc;
    if ((rc = chunk_time_begin(c))) return rc;
    if (!vax) enqueue_free_burst(c, bursts, limit_t);
    else for (uint32_t g = 0; g < bursts; ++g) enqueue_vax_chunk(c, limit_t);
    if ((rc = chunk_time_end(c))) return rc;
    if ((rc = burst_readback(c, first, std::min<uint32_t>(remaining, bursts * n_ahead), h))) return rc;
    HIP_TRY(c, hipGetLastError());
    if ((rc = ctrl_error(c, *h))) return rc;
    *done = h->t - first;
    c->last_chunk_pairs = h->chunk_pairs;
    Timing &t = c->tm;
    if (*done && t.kernel) { float ms; HIP_TRY(c, hipEventElapsedTime(&ms, t.cev[0], t.cev[1])); t.chunk_ms += ms; t.chunk_steps += *done; t.chunk_count += (*done + n_ahead - 1u) / n_ahead; }
    c->host_t = h->t;
    return ESIM_OK;
}

// Runs up to n_steps steps of an unsharded context: pipelined chunks while no vaccination programme runs,
// sequential steps from the step that starts it.
int run_steps(esim_ctx_impl *c, uint32_t n_steps, bool allow_early_stop, uint32_t *executed)
{
    Dev &d = c->d;
    const uint32_t n_ahead_max = (uint32_t)c->xf_n;
    uint32_t remaining = n_steps, total = 0; int rc;
    bool stalled = false, probing = false;
    uint32_t backoff = 0, sync_chunks_left = 0;
    // a vaccination programme runs: chunks with their vaccinations planned, or sequential steps (short runs: sequential)
    const bool vax_ok = c->tune.time_parallel && c->tune.vax_chunks && d.n_shards == 1u;
    bool sequential_only = !c->tune.pipeline || c->tm.phase, vax_regime = vax_ok && c->elig_seen;
    if (c->elig_seen && (!vax_ok || n_steps < 8u)) sequential_only = true;
    // a programme runs from here on: planned chunks where they can run and the rest of the call is worth a burst, else sequential steps
    auto programme_started = [&]() { c->elig_seen = true; if (vax_ok && remaining >= 8u) vax_regime = true; else sequential_only = true; };
    uint32_t vax_fail = 0;
    while (remaining > 0) {
        c->pin.ctrl_fresh = false;
        if (sequential_only) {
            uint32_t done = 0;
            if ((rc = run_sequential(c, remaining, allow_early_stop, &done))) return rc;
            total += done;
            break;
        }
        if (vax_regime) {
            // bursts of planned chunks; whatever stops one (a cut: the step at ctrl->t must run sequentially; no plan possible;
            // a chunk that does not fit the one-pass form) is answered with sequential steps, more of them when it keeps happening
            const uint32_t bursts = vax_fail ? 1u : std::min<uint32_t>((remaining + n_ahead_max - 1u) / n_ahead_max + 1u, 8u);   // (one more than fit: cuts)
            Ctrl h;
            uint32_t done = 0;
            if ((rc = run_burst(c, remaining, bursts, true, &h, &done))) return rc;
            c->quiet = h.quiet != 0u;
            if (h.vax_cuts > c->vax_chunk_cuts) c->repair_armed = true;   // (a chunk was cut: from now on the plan is repaired instead)
            c->vax_chunk_steps += done; c->vax_chunk_cuts = h.vax_cuts; c->vax_chunk_repairs = h.vax_repairs;
            total += done; remaining -= done;
            if (h.finished && allow_early_stop) break;
            if (remaining == 0) break;
            if (done) { vax_fail = 0; continue; }                       // (cut chunks advance less; the next one starts at the cut)
            if (std::getenv("ESIM_DEBUG"))
                std::fprintf(stderr, "[esim] vax burst without progress at t=%u: chunk_ok=%u parallel=%u vax_chunk=%u cut=%u pairs=%u fits_flag=%u elig=%u bursts=%u\n",
                             h.t, h.chunk_ok, h.chunk_parallel, h.vax_chunk, h.chunk_cut, h.chunk_pairs, 0u, h.elig_count, bursts);
            vax_fail = std::min<uint32_t>(vax_fail + 1u, 8u);
            uint32_t seq = 0;
            const uint32_t want = std::min<uint32_t>(remaining, vax_fail <= 1u ? 1u : (vax_fail <= 3u ? 8u : n_ahead_max));
            if ((rc = run_sequential(c, want, allow_early_stop, &seq))) return rc;
            total += seq; remaining -= seq;
            if (seq < want) break;                                       // the run ended
            continue;
        }
        if (c->tune.time_parallel && !stalled && sync_chunks_left == 0) {
            // Chunks are enqueued back to back without waiting for their k_decide: every kernel takes the chunk from the
            // control block and is a no-op when the chunk cannot run time-parallel (then the steps simply do not advance,
            // which the read-back sees, and the synchronous path further down takes over for one chunk).
            const uint32_t bursts = std::min<uint32_t>((remaining + n_ahead_max - 1u) / n_ahead_max, probing ? 1u : (small_chunk(c) ? 4u : 16u));   // (the form of a chunk's book-keeping is chosen from what the last read-back showed)
            Ctrl h;
            uint32_t done = 0;
            if ((rc = run_burst(c, remaining, bursts, false, &h, &done))) return rc;
            total += done; remaining -= done;
            if (h.finished) break;
            const bool all = done >= std::min<uint32_t>(remaining + done, bursts * n_ahead_max);
            if (done == 0) { backoff = std::min<uint32_t>(64u, backoff ? backoff * 2u : 1u); sync_chunks_left = backoff; probing = true; }
            else { backoff = 0; probing = !all; }
            if (!all) stalled = true;   // something other than a full time-parallel chunk is next
            continue;
        }
        stalled = false;
        if (sync_chunks_left) --sync_chunks_left;
        const uint32_t n_ahead = std::min<uint32_t>(remaining, n_ahead_max);
        ChunkPass{ c, c->P.max_steps, false }.future(n_ahead);
        uint32_t done = 0;
        Ctrl before;
        if ((rc = run_chunk(c, n_ahead, &done, &before))) return rc;
        c->host_t = before.t + done; total += done; remaining -= done;
        if (before.finished) break;
        if (done < n_ahead && remaining > 0) {
            if (before.have_elig || before.vacc_active) { programme_started(); continue; }
            // the next step starts the vaccination programme (or a limit was hit): one sequential step, then look again
            uint32_t one = 0;
            if ((rc = run_sequential(c, 1, allow_early_stop, &one))) return rc;
            total += one; remaining -= one;
            if (one == 0) break;
            Ctrl h;
            if ((rc = read_ctrl(c, &h))) return rc;
            if (h.have_elig) programme_started();   // that step started the programme
        }
        if (allow_early_stop && done > 0) {
            // a chunk may have ended the run (disease gone): k_batch_finish set `finished`
            Ctrl h;
            if ((rc = read_ctrl(c, &h))) return rc;
            if (h.finished) { c->host_t = h.t; break; }
        }
    }
    if (executed) *executed = total;
    return ESIM_OK;
}

}  // namespace

extern "C" int esim_step(esim_ctx *ctx, esim_step_result *out)
{
    esim_ctx_impl *c = CTX(ctx);
    int rc = check_budget(c, 1);
    if (rc) return rc;
    if (c->d.n_shards > 1) return fail(c, ESIM_ESTATE, "esim_step: a sharded population runs with esim_run_sharded");
    HIP_TRY(c, hipSetDevice(c->P.device));
    c->rest_t = 0;
    if ((rc = run_steps(c, 1, false, nullptr))) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (out) HIP_TRY(c, hipMemcpy(out, &c->d.records[c->host_t - 1], sizeof *out, hipMemcpyDeviceToHost));
    if ((rc = device_error(c))) return rc;
    c->rest_t = c->host_t;                           // (device_error has just read the control block at rest into the pinned mirror)
    return ESIM_OK;
}

extern "C" int esim_run(esim_ctx *ctx, uint32_t n_steps, int stop_when_done, esim_step_result *out_array, uint32_t *n_done)
{
    esim_ctx_impl *c = CTX(ctx);
    if (c && c->tm.host_trace) { c->tm.ht.clear(); ht_mark(c, "enter"); }
    int rc = check_budget(c, n_steps);
    if (rc) return rc;
    if (c->d.n_shards > 1) return fail(c, ESIM_ESTATE, "esim_run: a sharded population runs with esim_run_sharded");
    HIP_TRY(c, hipSetDevice(c->P.device));
    Pinned &pin = c->pin;
    const uint32_t first = c->host_t;
    const uint32_t flag = stop_when_done ? 1u : 0u;
    if (flag != c->stop_flag_dev) {                  // (the flag lives in the control block; written only when it changes)
        HIP_TRY(c, hipMemcpyAsync(&c->d.ctrl->stop_when_done, &flag, sizeof flag, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        c->stop_flag_dev = flag;
    }
    // bursts of chunk passes bring their records back together with the control block (burst_readback); whatever other forms
    // ran is fetched below
    pin.track = out_array != nullptr; pin.first = first; pin.valid = 0; pin.ctrl_fresh = false;
    c->rest_t = 0;
    rc = run_steps(c, n_steps, stop_when_done != 0, nullptr);
    pin.track = false;
    if (rc) return rc;
    Ctrl h;
    if (pin.ctrl_fresh) h = *pin.ctrl;
    else if ((rc = read_ctrl(c, &h))) return rc;
    if ((rc = ctrl_error(c, h))) return rc;
    const uint32_t done = h.steps_done >= first ? h.steps_done - first + 1 : 0;
    if (std::getenv("ESIM_DEBUG"))
        std::fprintf(stderr, "[esim] esim_run(%u steps from %u): done %u, t=%u steps_done=%u finished=%u chunk_ok=%u parallel=%u, records mirrored %u, control block %s\n",
                     n_steps, first, done, h.t, h.steps_done, h.finished, h.chunk_ok, h.chunk_parallel, pin.valid, pin.ctrl_fresh ? "from the burst" : "read now");
    c->host_t = first + done;
    c->rest_t = c->host_t;                           // (the pinned mirror holds the control block at rest, whichever way it came)
    if (out_array && done) {
        const uint32_t have = std::min(pin.valid, done);
        if (have < done) {
            HIP_TRY(c, hipMemcpyAsync(pin.rec + first + have, c->d.records + first + have, sizeof(esim_step_result) * (done - have), hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));
        }
        std::memcpy(out_array, pin.rec + first, sizeof(esim_step_result) * done);
    }
    if (n_done) *n_done = done;
    if (c->tm.host_trace) {
        ht_mark(c, "exit");
        std::fprintf(stderr, "[esim host trace] esim_run(%u):", n_steps);
        for (size_t i = 1; i < c->tm.ht.size(); ++i) std::fprintf(stderr, " %s +%.1f us;", c->tm.ht[i].first, c->tm.ht[i].second - c->tm.ht[i - 1].second);
        std::fprintf(stderr, " total %.1f us\n", c->tm.ht.back().second - c->tm.ht.front().second);
    }
    return ESIM_OK;
}

extern "C" int esim_set_pipeline(esim_ctx *ctx, int enable)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    c->tune.pipeline = enable != 0;            // 0: sequential steps only
    c->tune.time_parallel = enable >= 2;       // 1: one kernel per step (k_pipe); 2: all steps of a chunk in one pass
    c->tune.vax_chunks = enable >= 3;          // 3 (default): ... also while a vaccination programme runs, its vaccinations planned per chunk
    return ESIM_OK;
}

extern "C" int esim_set_small_step_limit(esim_ctx *ctx, uint32_t max_infected)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    c->tune.small_max = max_infected;
    return ESIM_OK;
}

extern "C" int esim_set_tiny_chunk_limit(esim_ctx *ctx, uint32_t max_pairs)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    c->tune.tiny_pairs = max_pairs;
    return ESIM_OK;
}
