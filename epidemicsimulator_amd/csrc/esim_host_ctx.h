// esim_host_ctx.h -- the context behind an esim_ctx, by concern; the helpers every host part uses; esim_create / esim_destroy.
namespace {

thread_local std::string g_create_error;

// Event timing, six mechanisms, and every event they use: clear() is what going back to step 0 forgets, destroy() frees the events.
struct Timing {
    bool phase = false, kernel = false;                 // esim_enable_phase_timing / esim_enable_kernel_timing
    uint32_t stride = 16;                               // kernel timing looks at every stride-th step
    hipEvent_t ev[5] = { nullptr, nullptr, nullptr, nullptr, nullptr };   // phases of a sequential step
    double phase_s[3] = { 0, 0, 0 };
    std::vector<hipEvent_t> kev; size_t kev_used = 0;   // two per timed step: before k_infected, after k_finish
    hipEvent_t cev[2] = { nullptr, nullptr }; double chunk_ms = 0; uint64_t chunk_steps = 0, chunk_count = 0;   // bursts of chunk passes
    std::vector<hipEvent_t> pkev; size_t pkev_used = 0; uint64_t pipe_steps = 0;   // sampled k_pipe launches
    hipEvent_t sev[2] = { nullptr, nullptr }; double small_ms = 0; uint64_t small_steps = 0;   // k_small
    // per-kernel device time of the chunk pass (esim_enable_chunk_kernel_timing): an event in front of every kernel of a chunk
    bool kdetail = false;
    std::vector<hipEvent_t> kdev; std::vector<int> kd_kind; size_t kd_used = 0;
    double kd_ms[ESIM_CK_N] = { 0 }; uint64_t kd_calls[ESIM_CK_N] = { 0 };
    bool host_trace = false;                            // ESIM_TRACE_HOST: esim_run prints where its host time went (stderr)
    std::vector<std::pair<const char *, double>> ht;

    static void make_pair(hipEvent_t (&e)[2]) { if (!e[0]) { (void)hipEventCreate(&e[0]); (void)hipEventCreate(&e[1]); } }
    void clear()
    {
        phase_s[0] = phase_s[1] = phase_s[2] = 0;
        kev_used = 0; pkev_used = 0; pipe_steps = 0;
        small_ms = 0; small_steps = 0; chunk_ms = 0; chunk_steps = 0; chunk_count = 0;
    }
    void destroy()
    {
        for (auto &e : ev) if (e) (void)hipEventDestroy(e);
        for (auto &e : cev) if (e) (void)hipEventDestroy(e);
        for (auto &e : sev) if (e) (void)hipEventDestroy(e);
        for (auto *v : { &kev, &pkev, &kdev }) { for (auto &e : *v) (void)hipEventDestroy(e); v->clear(); }
    }
};

// The exchange between shards (esim_comm_*): RCCL owned by the library, or a caller's all-reduce.
struct Comm {
    int rank = 0, world = 1;
    ncclComm_t nccl = nullptr;
    esim_allreduce_fn fn = nullptr; void *user = nullptr;
    std::vector<uint32_t> stage;
    uint32_t *xr = nullptr; size_t xr_n = 0;      // records exchange (sharded chunks)
    uint64_t chunk_steps = 0, step_steps = 0;     // steps run as sharded chunks / as coupled steps
    uint64_t calls = 0;
    double timeout_s = 60.0;                      // deadline of a host wait on a stream that holds collectives (esim_comm_set_timeout)
};

// Pinned host mirrors: control block and records come back with ONE stream wait (two blocking copies cost more than a small chunk).
struct Pinned {
    Ctrl *ctrl = nullptr;
    esim_step_result *rec = nullptr; size_t rec_n = 0;
    uint32_t first = 0, valid = 0;                // records [first, first + valid) of the call in flight are in rec
    bool track = false;
    bool ctrl_fresh = false;                      // ctrl holds the control block as it stands (nothing was enqueued since)
    uint32_t *area = nullptr; size_t area_n = 0;  // esim_area_census: mirror of the count table, [n_areas * 5]
    uint32_t *grp = nullptr;                      // esim_group_census: the same, [ESIM_MAX_GROUPS * 5]
    uint8_t *aw = nullptr;                        // a series fold: the at-work bit per step as run_shape derived it, [cap_steps + 1], on its way to the device
};

// esim_restart: the distinct seeds on the device; control block and threshold LUT staged in pinned memory, an event behind their copies.
// esim_restart_seeded: the list that replaces them goes through a pinned buffer of its own, behind the same event.
struct RestartStaging {
    uint32_t *seeds_dev = nullptr; size_t seeds_cap = 0;      // room of the device list, in seeds
    struct Block { Ctrl h; uint64_t lut[512]; } *stage = nullptr;
    uint32_t *seeds_stage = nullptr; size_t seeds_stage_n = 0;
    hipEvent_t ev = nullptr; bool ev_used = false;
};

// esim_ensemble_*: accumulators over the members of an ensemble, on the device.  One kind is in force at a time (`kind`; the table
// of esim_host_ensemble.h says per kind which buffers of `rows` it owns, which reader reads it and what is kept of a member;
// DESIGN 34), begun by ens_begin, which assigns every field below but `store` and `folds` -- nothing survives from the kind
// before.  where, n: the column key and the columns (n_areas, n_groups by group, four settings, one); valid == false: the labels
// a kind by group was begun for are gone.
struct Ensemble {
    enum Kind { ENS_NONE = 0, ENS_CENSUS, ENS_ARRIVAL, ENS_SERIES, ENS_SETTINGS, ENS_REPRODUCTION, ENS_PAIRED, ENS_PEAKS, ENS_BURDEN_PEAKS, ENS_BURDEN_SERIES,
                ENS_BURDEN_PAIRED, ENS_KINDS };
    Kind kind = ENS_NONE;                         // ENS_NONE: no begin since the upload, and no buffer below is allocated
    int where = ESIM_AREA_HOME; uint32_t n = 0; bool valid = false;
    // The buffers, [n_rows][n_cols] cells each where the kind owns them (the census and the arrival kind: one row): the counters
    // and sums a fold adds to, the row plane(s) a fold leaves a member's rows in, and the series engine's small temporaries -- all
    // kept from the begin on, so that a fold allocates nothing proportional to rows x columns.  vax: the 4 B per citizen of the
    // vaccination replay, allocated by the first fold of the series kind that needs them and carried from begin to begin.
    struct Rows {
        uint32_t *hit = nullptr, *defined = nullptr, *members = nullptr, *p0 = nullptr, *p1 = nullptr, *occ = nullptr, *vax = nullptr;
        unsigned long long *sum = nullptr, *sumsq = nullptr;                         // of the value: cases, count, peak; baseline or cohort size
        unsigned long long *sum_o = nullptr, *sumsq_o = nullptr, *cross = nullptr;   // of the second plane (offspring, current run) and of the product; peaks: of the peak's step
        unsigned long long *sum_d = nullptr, *sumsq_d = nullptr;                     // peaks: of the duration
        uint8_t *aw = nullptr;
        uint32_t n_rows = 0, n_cols = 0;
        bool two = false;                         // the series kind: p1 is allocated too (status rows by the area stood in)
    } rows;
    // What the begin in force was given, under one name per meaning; a begin assigns all of it (the fields of other kinds: 0).
    struct Par {
        uint32_t status_mask = 0;                 // census, peaks: the statuses counted
        uint32_t setting_mask = 0;                // settings
        uint32_t horizon = 0;                     // arrival: reached = arrival step <= horizon
        int status = 0;                           // series: the status of the rows, or SERIES_EVENTS
        int burden_what = 0;                      // burden series, burden paired: ESIM_BURDEN_*
        uint32_t first = 0, stride = 0;           // the kinds over rows: row i starts at step first + i * stride
        uint32_t last = 0, threshold = 0;         // peaks, burden peaks: the window [first, last], the threshold of the duration
        uint32_t min_hit = 0;                     // hit where the value >= this: min_cases, min_count, min_peak
        uint32_t min_defined = 0;                 // defined where the first plane >= this: min_cohort, min_baseline
        uint32_t r_num = 0, r_den = 0;            // reproduction: hit where offspring / cases >= r_num / r_den
        uint32_t min_averted = 0;                 // paired, burden paired: hit where baseline - current >= this
        bool cumulative = false;                  // ... rows summed up from `first` on
    } par;
    // esim_ensemble_keep_members (esim_host_members.h): the members' values beside the accumulators in force, [capacity][n_rows *
    // n_cols] keys (signed values with the top bit flipped), `kept` slots filled in the order of the folds.  planes == nullptr: no
    // store.  folds: the members folded since the begin, kept or not (a store may only be opened in front of the first).
    struct Store {
        uint32_t *planes = nullptr;
        uint32_t capacity = 0, kept = 0, n_rows = 0, n_cols = 0;
        int what = 0;
        bool is_signed = false, has_never = false;
    } store;
    uint32_t folds = 0;
    uint8_t *merge_stage = nullptr; size_t merge_stage_bytes = 0;   // esim_ensemble_merge / _load (esim_host_merge.h): where a piece of the other ensemble lands, kept from call to call
    uint64_t dist_stats[4] = { 0u, 0u, 0u, 0u };  // esim_ensemble_distances (esim_host_dist.h): the counts of the last call's kernel (esim_dist.h)
};

// esim_set_groups: a label per citizen, the groups' sizes and the count table of esim_group_census [n * 5] (nullptr: no labels).
struct Groups {
    uint16_t *lab = nullptr; uint32_t n = 0;
    uint32_t *size = nullptr, *cnt = nullptr;
    std::vector<uint32_t> sizes;                  // the groups' sizes on the host (what esim_ensemble_merge compares)
};

// esim_burden_set: the severity tables in force, on the host as they were given and on the device as the kernels
// read them: admit_thr [n_groups], death_thr [n_groups], delay_cdf [ESIM_BURDEN_BINS], stay_cdf [ESIM_BURDEN_BINS] in one
// allocation.  set == false: none.
struct BurdenState {
    bool set = false;
    uint32_t n_groups = 0, n_delay = 0, n_stay = 0, delay_unit = 0, stay_unit = 0;
    std::vector<uint32_t> host;
    uint32_t *tab = nullptr;
};

// esim_baseline_keep: the exposure step of every citizen of a finished run, one uint32 per citizen on the device (0 for an index
// case, ESIM_NEVER for a citizen the log did not hold), with the steps run, the parameters then in force and the number of log
// entries.  The plane is allocated at the first keep and reused; held == false: none is kept (dropped, or never taken).
struct Baseline {
    uint32_t *plane = nullptr;
    bool held = false;
    uint32_t steps = 0, n_cases = 0;
    esim_params P;
};

// esim_burden_baseline_keep: the admitted cases of a finished run as a list on the device -- three planes of `cap`
// entries in one allocation (citizen, admit_step, end_step | died << 31) and the two counts --, with the steps run, the entries,
// the deaths among them and the parameters then in force (the seed among them).  Allocated at the first keep, grown when a
// later run needs more; held == false: none is kept.  Independent of Baseline.
struct BedsBaseline {
    uint32_t *list = nullptr, *count = nullptr;
    size_t cap = 0;
    uint32_t *tmp = nullptr, *tmp_count = nullptr;      // the scratch list of the run as it stands (esim_burden_compare, the folds): kept between calls
    size_t tmp_cap = 0;
    bool held = false;
    uint32_t steps = 0, n = 0, n_died = 0;
    esim_params P;
};

// esim_snapshot: the state at rest after `step` completed steps, kept on the device, with the parameters then in force; the
// control block stays on the host, normalised as esim_checkpoint_restore normalises it (esim_rollback stages it from there).
// The buffers are allocated at the first snapshot and kept; step == 0: none is held (dropped, or never taken).
struct Snapshot {
    uint32_t step = 0;
    esim_params P;
    Ctrl h;
    uint32_t *words = nullptr, *hist = nullptr, *log_off = nullptr, *exp_step = nullptr;   // [n], [TE_SLOTS], [TE_SLOTS + 1], [2 * (cap_steps + 2)]
    esim_step_result *records = nullptr;                                                    // [cap_steps + 1]
    uint32_t *log = nullptr; size_t log_cap = 0;                                            // the log's prefix: grown when a snapshot needs more
    // what the host knew of the run then, beside the control block (esim_rollback sets the host's view to match)
    uint32_t last_chunk_pairs = 0; bool quiet = false, repair_armed = false, elig_seen = false;
    uint64_t vax_chunk_steps = 0, vax_chunk_cuts = 0, vax_chunk_repairs = 0;
};

// esim_rollback with another seed or vaccination_rate: the steps up to and including `step` drew their vaccinations under the
// old values, the later ones under those in force (run_shape and the vaccination replay).  step == 0: no seam.
struct Seam { uint32_t step = 0, rate = 0; uint64_t seed = 0; };

// The same for the exposure draws, which esim_exposure_settings and its kin replay after the fact: a rollback under another seed,
// exposure_chance or mask_effectiveness leaves the entries of the log up to and including `step` drawn under the snapshot's three
// values, kept here, and the later ones under those in force.  A record of its own beside Seam: nothing that hangs on Seam (the
// refusals of esim_snapshot and of the checkpoint calls) reads it.  step == 0: none.  twice: the snapshot itself lay on a
// branch with such a seam and the rollback changed the values again -- three parameter sets, which the replay does not follow.
// two_capacities: a rollback changed bus_capacity, the buses of the history were filled under two values (esim_transmission_tree
// and its kin, which replay the bus assignment, refuse that).
struct DrawSeam { uint32_t step = 0; bool twice = false, two_capacities = false; uint64_t seed = 0; double chance = 0.0, mask_effectiveness = 0.0; };

// What picks the form and the grids of the kernels: esim_set_* and the tuning knobs of the environment (read at upload).
struct Tuning {
    uint32_t grid_citizens = 1, grid_infected = 1, grid_expose = 1;
    uint32_t grid_chunk = 1024;
    bool grid_chunk_env = false;                // ESIM_GRID_CHUNK is set: the grid it names holds for chunks with few Infected too
    bool pipeline = true;                       // run chunks of steps as one kernel per step while no vaccination programme runs
    bool time_parallel = true;                  // draw all steps of a chunk in one pass when its marks fit the hash map
    bool vax_chunks = true;                     // time-parallel chunks also under a vaccination programme (their vaccinations planned ahead, k_chunk_vax)
    bool vax_repair = true;                     // planned chunks: repair the plan after bus exposures instead of cutting the chunk (ESIM_VAX_REPAIR=0: cut)
    bool vax_repair_always = false;             // ESIM_VAX_REPAIR=2: from the start
    uint32_t tiny_pairs = 2048;                 // chunks with at most this many (Infected, step) pairs at the last read-back run as ONE kernel (k_chunk_tiny; 0: off)
    uint32_t small_grid = 64, small_mult = 4;   // chunks with few Infected: workgroups of the marks / fold kernels, multiplier of the draw kernels (0: off)
    uint32_t draw_mult = 4, units_mult = 4;     // k_chunk_draw / k_chunk_units run this many times the marks grid: more, shorter wavefronts than the chip holds at once
    uint32_t small_max = 128;                   // infected-slice length up to which the persistent single-workgroup kernel runs a step
    uint32_t pair_log2 = 0;                     // ESIM_PAIR_LOG2: the pair table of esim_area_flows / esim_lineage_areas has 1 << this many slots (0: sized by the log)
    uint32_t merge_piece = 0;                   // ESIM_MERGE_PIECE: the cells a piece of esim_ensemble_merge / _load stages (0: unset, MERGE_PIECE_CELLS; tests only)
    uint32_t grid_cap = 0;                      // ESIM_GRID_CAP: the grids of the output kernels hold at most this many workgroups (0: unset, as in production)
};

// What grid_capped sized while ESIM_GRID_CAP is set, per launch site (esim_debug_launches): a fixed table, a site more than it
// holds is an error of the call that reads it.
const uint32_t LAUNCH_SITES_MAX = 128;
struct LaunchLog {
    struct Site { const char *file; uint32_t line, launches, clipped, max_trips; } site[LAUNCH_SITES_MAX];
    uint32_t n = 0;
    bool overflow = false;
};

// What the pair engine (esim_host_flows.h) did in the last call that used it: esim_pair_stats.
struct PairStats {
    double ms[3] = { 0.0, 0.0, 0.0 };           // insert (the emptying of the table included), compact, sort (the read of the count included)
    uint32_t distinct = 0, capacity = 0, dropped = 0;
};

struct esim_ctx_impl {
    esim_params P;
    Dev d;
    bool uploaded = false;
    bool household_work = false;          // the uploaded population has a Household that is the work place of a citizen who does not live in it: the replays refuse it (settings_check)
    hipStream_t stream = nullptr;
    std::string err;
    // host copies needed for reset
    std::vector<uint32_t> init_state;
    std::vector<uint32_t> init_log;       // distinct seeds
    size_t cnt_bytes = 0;
    uint32_t *cnt_base = nullptr;
    uint32_t n_routes = 0;
    std::vector<uint32_t> route_tab;      // esim_routes: home area, work area and riders of every route, [3][n_routes]
    uint32_t longest_list = 0;            // members of the longest household, work place, room or route (esim_contact_hours: the range of per_case)
    size_t xa_n = 0, xb_n = 0, xf_n = 0;
    uint64_t pop_hash = 0;        // of the uploaded population arrays: a checkpoint only goes back into the population it came from
    uint64_t pop_hash_head = 0;   // the same hash before it mixes the seeds (esim_restart_seeded finishes it with its own list)
    uint32_t cap_steps = 0;       // capacity of the record log (max_steps at esim_create)
    uint32_t *area_cnt = nullptr; // esim_area_census: the count table on the device, [n_areas * 5]
    uint32_t *arrival = nullptr;  // esim_area_arrival: first exposure step per area or group, [max(n_areas, ESIM_MAX_GROUPS)] (nullptr before the first call)
    std::vector<void *> allocs;   // device allocations
    // where the run stands, as the host knows it (rewind_host takes it back to step 0)
    uint32_t host_t = 1;                        // next time step to enqueue
    uint32_t last_chunk_pairs = 0;              // Infected during the chunk last looked at (picks the form of the chunk's book-keeping)
    uint32_t stop_flag_dev = 0;                 // what ctrl->stop_when_done holds (written only when it changes)
    bool quiet = false;                         // Ctrl::quiet at the last read-back of a burst of chunk passes
    bool repair_armed = false;                  // ... its two kernels are enqueued from the first cut of a run on (York never has one: 11 us a chunk saved)
    bool elig_seen = false;                     // the last control block read back had an eligible set (a vaccination programme runs)
    uint32_t rest_t = 0;                        // host_t for which pin.ctrl is known to hold the control block at rest (0: not known; esim_snapshot)
    uint64_t vax_chunk_steps = 0, vax_chunk_cuts = 0, vax_chunk_repairs = 0;
    Timing tm;
    PairStats pair_stats;
    Comm comm;
    Pinned pin;
    RestartStaging rs;
    Ensemble ens;
    Groups grp;
    Snapshot snap;
    Baseline base;
    BedsBaseline beds;
    BurdenState burden;
    Seam seam;
    DrawSeam draw_seam;               // of the history the context stands on
    DrawSeam snap_draw_seam;          // of the history under the snapshot held (esim_snapshot copies it, esim_rollback starts from it)
    Tuning tune;
    LaunchLog launches;
};

#define CTX(c) (reinterpret_cast<esim_ctx_impl *>(c))

void comm_release(esim_ctx_impl *c);     // (esim_host_shard.h)
int wait_stream(esim_ctx_impl *c);

int fail(esim_ctx_impl *c, int code, const std::string &msg)
{
    if (c) c->err = msg; else g_create_error = msg;
    return code;
}

#define HIP_TRY(c, expr)                                                                         \
    do {                                                                                         \
        hipError_t e_ = (expr);                                                                  \
        if (e_ != hipSuccess)                                                                    \
            return fail(c, ESIM_ENODEVICE, std::string(#expr) + ": " + hipGetErrorString(e_));   \
    } while (0)

int alloc_failed(esim_ctx_impl *c, hipError_t e) { return fail(c, ESIM_ENOMEM, std::string("hipMalloc: ") + hipGetErrorString(e)); }

template <class T> int dev_alloc(esim_ctx_impl *c, T **p, size_t n)
{
    void *q = nullptr;
    hipError_t e = hipMalloc(&q, sizeof(T) * (n ? n : 1));
    if (e != hipSuccess) return alloc_failed(c, e);
    c->allocs.push_back(q);
    *p = (T *)q;
    return ESIM_OK;
}

// an allocation with its initial content: every byte 0, or 0xFF where a table's empty value is all ones
template <class T> int dev_alloc_fill(esim_ctx_impl *c, T **p, size_t n, int byte = 0)
{
    if (int rc = dev_alloc(c, p, n)) return rc;
    if (n) HIP_TRY(c, hipMemset(*p, byte, sizeof(T) * n));
    return ESIM_OK;
}

template <class T> int dev_upload(esim_ctx_impl *c, const T **p, const T *host, size_t n)
{
    T *q = nullptr;
    int rc = dev_alloc(c, &q, n);
    if (rc) return rc;
    if (n) HIP_TRY(c, hipMemcpy(q, host, sizeof(T) * n, hipMemcpyHostToDevice));
    *p = q;
    return ESIM_OK;
}

void free_device(esim_ctx_impl *c)
{
    for (void *p : c->allocs) (void)hipFree(p);
    c->allocs.clear();
    c->ens.store = Ensemble::Store();           // (the members kept were one of them)
    c->uploaded = false;
}

// one allocation back (buffers that are re-sized: the commuter segments, the records exchange); every device pointer of a
// context is one of its own allocations: any other pointer is left alone
void dev_free(esim_ctx_impl *c, void *p)
{
    auto it = std::find(c->allocs.begin(), c->allocs.end(), p);
    if (it == c->allocs.end()) return;
    c->allocs.erase(it);
    (void)hipFree(p);
}

// A device buffer that lives as long as one call: freed when its scope ends, whichever way the call leaves.
template <class T> struct DevTmp {
    T *p = nullptr;
    DevTmp() = default; DevTmp(const DevTmp &) = delete; DevTmp &operator=(const DevTmp &) = delete;
    ~DevTmp() { (void)hipFree(p); }
    hipError_t alloc(size_t n) { return hipMalloc((void **)&p, sizeof(T) * std::max<size_t>(1, n)); }
};

// the context's device made current and its stream drained
int drain(esim_ctx_impl *c) { HIP_TRY(c, hipSetDevice(c->P.device)); HIP_TRY(c, hipStreamSynchronize(c->stream)); return ESIM_OK; }

uint32_t grid_for(size_t items, uint32_t per_block, uint32_t cap)
{
    size_t g = (items + per_block - 1) / per_block;
    return (uint32_t)std::max<size_t>(1, std::min<size_t>(g, cap));
}

// The grid of an output launch: `grid` as the launch site sized it, or ESIM_GRID_CAP workgroups where that is fewer -- the
// kernels loop with a grid stride, so a test reaches the second and later trips with a small world.  With the knob unset
// (production) this returns `grid` and touches nothing.  With it set, the site's record counts the launch, whether it was
// clipped, and the trips of its longest loop.
uint32_t grid_clamp(esim_ctx_impl *c, size_t items, uint32_t per_block, uint32_t grid, const char *file, uint32_t line)
{
    const uint32_t knob = c->tune.grid_cap;
    if (!knob) return grid;
    const uint32_t g = std::min(grid, knob);
    LaunchLog &l = c->launches;
    uint32_t i = 0;
    while (i < l.n && !(l.site[i].line == line && std::strcmp(l.site[i].file, file) == 0)) ++i;
    if (i == l.n) {
        if (l.n == LAUNCH_SITES_MAX) { l.overflow = true; return g; }
        l.site[l.n++] = LaunchLog::Site{ file, line, 0u, 0u, 0u };
    }
    LaunchLog::Site &s = l.site[i];
    const size_t per_trip = (size_t)g * per_block;
    s.launches += 1u;
    s.clipped += g < grid ? 1u : 0u;
    s.max_trips = std::max(s.max_trips, (uint32_t)std::min<size_t>(0xFFFFFFFFu, (items + per_trip - 1) / per_trip));
    return g;
}

// grid_for for a launch whose kernel loops over its items: every such launch of the output families is sized here.
// per_trip: the items a workgroup takes per trip of its loop where that is not per_block -- a site that sizes its grid for
// several trips a lane (per_block = TPB * 32 with a loop that strides by TPB) -- so that the record counts the trips made.
uint32_t grid_capped(esim_ctx_impl *c, size_t items, uint32_t per_block, uint32_t cap, uint32_t per_trip = 0, const char *file = __builtin_FILE(),
                     uint32_t line = __builtin_LINE())
{
    return grid_clamp(c, items, per_trip ? per_trip : per_block, grid_for(items, per_block, cap), file, line);
}

static inline void ht_mark(esim_ctx_impl *c, const char *what)
{
    if (!c->tm.host_trace) return;
    timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts);
    c->tm.ht.emplace_back(what, ts.tv_sec * 1e6 + ts.tv_nsec * 1e-3);
}

// The control block through the pinned mirror: an asynchronous copy and one wait.  Every read-back of it goes through the
// mirror (burst_readback and sync_status fill it alongside other work), so that no copy is ever aimed at memory the call
// does not own.
int read_ctrl(esim_ctx_impl *c, Ctrl *h)
{
    HIP_TRY(c, hipMemcpyAsync(c->pin.ctrl, c->d.ctrl, sizeof(Ctrl), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    *h = *c->pin.ctrl;
    return ESIM_OK;
}

// The sticky device-side error of a control block read back, as the call's return code.  A sharded run returns the lowest code
// any shard raised (Ctrl::peer_error, summed by k_status_unpack), the same on every rank.
int ctrl_error(esim_ctx_impl *c, const Ctrl &h)
{
    if (!h.error) return ESIM_OK;
    const int code = -(int)(h.peer_error ? err_decode(h.peer_error) : h.error);
    return fail(c, code, "device-side error " + std::to_string(code) + " (S underflow / vaccination window exhausted / a chunk table check; raised at check " +
                         std::to_string(h.err_where) + ", esim_device.h ERR_AT_*)");
}

// The control block's error state as it stands.
int device_error(esim_ctx_impl *c)
{
    Ctrl h;
    const int rc = read_ctrl(c, &h);
    return rc ? rc : ctrl_error(c, h);
}

}  // namespace

extern "C" void esim_default_params(esim_params *p)
{
    if (!p) return;
    p->exposure_chance = 0.00055; p->mask_effectiveness = 0.70;            // disease.rs:120,127
    p->lockdown_threshold = 0.0034; p->vaccination_threshold = 0.005;      // interventions.rs:74-75
    p->mask_pt_threshold = 0.001; p->mask_everywhere_threshold = 0.0022;   // interventions.rs:55-56
    p->exposed_time = 4 * 24; p->infected_time = 14 * 24;                  // disease.rs:122-123
    p->vaccination_rate = 85 * 18;                                         // disease.rs:125
    p->bus_capacity = 20;                                                  // config.rs:37
    p->start_hour = 9; p->end_hour = 17;                                   // citizen.rs:154-155
    p->seed = 0x5EED2011ull;
    p->device = 0;
    p->max_steps = 5000;                                                   // disease.rs:124
}

// ceil(q * 2^32): `uniform < q` (citizen.rs:242) for uniform = w * 2^-32 (w a 32-bit word) is exactly
// `w < ceil(q * 2^32)`, because scaling a double by 2^32 is exact.
extern "C" int esim_threshold_lut(const esim_params *p, uint64_t out[512])
{
    if (!p || !out) return ESIM_EINVAL;
    for (int row = 0; row < 2; ++row) {
        // DiseaseModel::get_exposure_chance, disease.rs:131-154 (is_vaccinated = false: only
        // Susceptible citizens are ever tested, simulator.rs:337,436)
        double chance = p->exposure_chance - (row ? p->exposure_chance * p->mask_effectiveness : 0.0) - 0.0;
        if (std::signbit(chance)) chance = 0.0;
        for (int n = 0; n < 256; ++n) {
            const double q = 1.0 - std::pow(1.0 - chance, (double)n);      // binomial, citizen.rs:47-49
            const double scaled = std::ceil(std::ldexp(q, 32));
            out[row * 256 + n] = scaled <= 0.0 ? 0ull : (uint64_t)scaled;
        }
    }
    return ESIM_OK;
}

namespace {
// What esim_create and esim_restart accept as parameters (the device ordinal and the record log's capacity apart).
int check_params(esim_ctx_impl *c, const esim_params *p, const std::string &who)
{
    if (p->exposed_time + p->infected_time + 2u > TE_BIAS)
        return fail(c, ESIM_ERANGE, who + ": exposed_time + infected_time + 2 exceeds the state encoding (512)");
    if (p->vaccination_rate > VACC_MAX_RATE)
        return fail(c, ESIM_ERANGE, who + ": vaccination_rate above 8192 is not supported");
    if (p->bus_capacity == 0 || p->start_hour == 0 || p->end_hour == 0 || p->start_hour > 24 || p->end_hour > 24)
        return fail(c, ESIM_EINVAL, who + ": bad bus_capacity / working hours");
    {
        // the schedule is evaluated once for everybody, which needs the four arms of citizen.rs:177-205 to
        // fall on four different hours
        const uint32_t h[4] = { (p->start_hour + 23u) % 24u, p->start_hour % 24u, (p->end_hour + 23u) % 24u, p->end_hour % 24u };
        for (int a = 0; a < 4; ++a) for (int b = a + 1; b < 4; ++b)
            if (h[a] == h[b]) return fail(c, ESIM_EINVAL, who + ": start_hour-1, start_hour, end_hour-1, end_hour must be distinct");
        if (p->start_hour > 23 || p->end_hour > 23) return fail(c, ESIM_EINVAL, who + ": working hours must be in 1..23");
    }
    if (p->max_steps == 0 || p->max_steps > ESIM_MAX_STEP)
        return fail(c, ESIM_ERANGE, who + ": max_steps must be in 1..7600");
    // (NaN fails both comparisons; esim_threshold_lut would cast ceil(NaN) to uint64_t)
    if (!(p->exposure_chance >= 0.0 && p->exposure_chance <= 1.0))
        return fail(c, ESIM_EINVAL, who + ": exposure_chance must be a probability");
    return ESIM_OK;
}

// Everything in Dev that is derived from the parameters.
void params_to_dev(esim_ctx_impl *c)
{
    Dev &d = c->d;
    d.exposed_time = c->P.exposed_time; d.infected_time = c->P.infected_time;
    d.vaccination_rate = c->P.vaccination_rate; d.bus_capacity = c->P.bus_capacity;
    d.start_hour = c->P.start_hour; d.end_hour = c->P.end_hour;
    d.seed_lo = (uint32_t)c->P.seed; d.seed_hi = (uint32_t)(c->P.seed >> 32);
    d.thr_lockdown = c->P.lockdown_threshold; d.thr_vacc = c->P.vaccination_threshold;
    d.thr_mask_pt = c->P.mask_pt_threshold; d.thr_mask_all = c->P.mask_everywhere_threshold;
    d.max_steps = c->P.max_steps;
    c->xf_n =std::min<uint32_t>(FREE_MAX, c->P.exposed_time + 1u);
    d.xf_n = (uint32_t)c->xf_n;
}
}  // namespace

extern "C" int esim_create(const esim_params *p, esim_ctx **out)
{
    if (!p || !out) return fail(nullptr, ESIM_EINVAL, "esim_create: null argument");
    if (int rc = check_params(nullptr, p, "esim_create")) return rc;
    int n_dev = 0;
    hipError_t e = hipGetDeviceCount(&n_dev);
    if (e != hipSuccess || n_dev <= 0)
        return fail(nullptr, ESIM_ENODEVICE, std::string("esim_create: no HIP device (") + hipGetErrorString(e) + ")");
    if (p->device < 0 || p->device >= n_dev) return fail(nullptr, ESIM_EINVAL, "esim_create: device ordinal out of range");
    e = hipSetDevice(p->device);
    if (e != hipSuccess) return fail(nullptr, ESIM_ENODEVICE, std::string("hipSetDevice: ") + hipGetErrorString(e));
    esim_ctx_impl *c = new esim_ctx_impl();
    c->P = *p;
    c->cap_steps = p->max_steps;
    if (const char *e = std::getenv("ESIM_COMM_TIMEOUT_S")) { const double v = std::atof(e); if (v > 0.0) c->comm.timeout_s = v; }
    std::memset(&c->d, 0, sizeof c->d);
    e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e != hipSuccess) { delete c; return fail(nullptr, ESIM_ENODEVICE, std::string("hipStreamCreate: ") + hipGetErrorString(e)); }
    for (auto &ev : c->tm.ev) (void)hipEventCreate(&ev);
    *out = reinterpret_cast<esim_ctx *>(c);
    return ESIM_OK;
}

extern "C" void esim_destroy(esim_ctx *ctx)
{
    if (ctx) comm_release(CTX(ctx));
    if (!ctx) return;
    esim_ctx_impl *c = CTX(ctx);
    (void)hipSetDevice(c->P.device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    free_device(c);
    c->tm.destroy();
    for (void *p : { (void *)c->pin.ctrl, (void *)c->pin.rec, (void *)c->pin.area, (void *)c->pin.grp, (void *)c->pin.aw, (void *)c->rs.stage, (void *)c->rs.seeds_stage })
        if (p) (void)hipHostFree(p);
    if (c->rs.ev) (void)hipEventDestroy(c->rs.ev);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

extern "C" const char *esim_last_error(const esim_ctx *ctx)
{
    if (!ctx) return g_create_error.c_str();
    return reinterpret_cast<const esim_ctx_impl *>(ctx)->err.c_str();
}
