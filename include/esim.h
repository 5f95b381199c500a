/*
 * esim.h -- C ABI of libesim: the MI355X (gfx950) implementation of the reference
 * `sim` crate's per-timestep Citizen update loop.
 *
 * The reference (NoSuchThingAsRandom/EpidemicSimulator) has no FFI or plugin
 * interface: its boundary for this path is the Rust API `Simulator::step` /
 * `Simulator::simulate` (sim/src/simulator.rs:108,131).  Each entry point below names
 * the reference item it replaces.  A Rust shim implementing `Simulator` over this ABI
 * is shown in INTEGRATION.md.
 *
 * Conventions: every function returns ESIM_OK (0) or a negative ESIM_E* code and
 * never unwinds across the boundary; esim_last_error() gives the text.  The caller
 * owns every buffer it passes (the library copies in/out and retains no host
 * pointer).  A context is used from one host thread at a time (the reference
 * `Simulator` is !Send: it owns a ThreadRng, simulator.rs:102); any number of
 * contexts may be used at once, each from its own thread.  All compute runs
 * on the GPU; there is no CPU fallback -- without a usable HIP device
 * esim_create() fails with ESIM_ENODEVICE.
 */
#ifndef ESIM_H
#define ESIM_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ESIM_OK          0
#define ESIM_EINVAL     -1   /* bad argument / population contract violated */
#define ESIM_ENODEVICE  -2   /* no HIP device / HIP runtime error */
#define ESIM_ENOMEM     -3
#define ESIM_ESTATE     -4   /* call out of order (e.g. step before upload) */
#define ESIM_ERANGE     -5   /* step budget / encoding range exceeded */
#define ESIM_ESIM       -6   /* the reference's own error path (S underflow, statistics.rs:275-287) */
#define ESIM_ETIMEDOUT  -7   /* sharded run: no progress within the deadline (a peer left or died); the RCCL communicator was aborted */

/* DiseaseStatus codes, sim/src/disease.rs:36-44 */
enum { ESIM_SUSCEPTIBLE = 0, ESIM_EXPOSED = 1, ESIM_INFECTED = 2, ESIM_RECOVERED = 3, ESIM_VACCINATED = 4 };
/* BuildingType, sim/src/models/building.rs:46-53 (only the three the builder creates) */
enum { ESIM_HOUSEHOLD = 0, ESIM_WORKPLACE = 1, ESIM_SCHOOL = 2 };
/* MaskStatus, sim/src/interventions.rs:26-30 */
enum { ESIM_MASK_NONE = 0, ESIM_MASK_PUBLIC_TRANSPORT = 1, ESIM_MASK_EVERYWHERE = 2 };

#define ESIM_NO_ROOM 0xFFFFFFFFu
#define ESIM_FLAG_USES_PUBLIC_TRANSPORT 1u  /* Citizen::uses_public_transport, citizen.rs:132 */
#define ESIM_FLAG_MASK_COMPLIANT        2u  /* Citizen::is_mask_compliant, citizen.rs:131 */

/* Compile-time constants of the reference gathered into one runtime struct:
 * DiseaseModel::covid() (sim/src/disease.rs:118-129), InterventionThresholds and
 * MaskStatus::get_threshold (sim/src/interventions.rs:50-57,71-78), BUS_CAPACITY
 * (sim/src/config.rs:37), start/end_working_hour (sim/src/models/citizen.rs:154-155). */
typedef struct esim_params {
    double   exposure_chance;            /* 0.00055 */
    double   mask_effectiveness;         /* 0.70 */
    double   lockdown_threshold;         /* 0.0034 */
    double   vaccination_threshold;      /* 0.005 */
    double   mask_pt_threshold;          /* 0.001 */
    double   mask_everywhere_threshold;  /* 0.0022 */
    uint32_t exposed_time;               /* 96 */
    uint32_t infected_time;              /* 336 */
    uint32_t vaccination_rate;           /* 1530 */
    uint32_t bus_capacity;               /* 20 */
    uint32_t start_hour;                 /* 9 */
    uint32_t end_hour;                   /* 17 */
    uint64_t seed;                       /* Philox4x32-10 key (replaces thread_rng, simulator.rs:630) */
    int32_t  device;                     /* HIP device ordinal */
    uint32_t max_steps;                  /* capacity of the device-side record log; DiseaseModel::max_time_step = 5000 */
} esim_params;

/* What SimulatorBuilder::build (sim/src/simulator_builder.rs:1162-1292) leaves behind,
 * flattened to borrowed structure-of-arrays.  Citizens are indexed by
 * CitizenID::global_index (citizen.rs:52-57), buildings by a dense index over all
 * Output Areas (BuildingID, building.rs:62-67), rooms by a dense index over all
 * School classes and offices (School::occupant_to_class, building.rs:341).
 * Sharding (multi-GPU): a shard holds the citizens of a contiguous Output Area range;
 * citizen_id_base / n_citizens_global keep the Philox counters global, and the
 * shared_* tables name the buildings / rooms whose members live on several shards. */
typedef struct esim_population {
    uint32_t n_citizens, n_buildings, n_areas, n_rooms, n_seeds;
    uint32_t citizen_id_base;        /* global index of local citizen 0 (0 when unsharded) */
    uint32_t n_citizens_global;      /* == n_citizens when unsharded */
    uint32_t n_shared_buildings;     /* 0 when unsharded */
    uint32_t n_shared_rooms;         /* 0 when unsharded */
    const uint32_t *home_building;   /* [n_citizens] Citizen::household_code, citizen.rs:116 */
    const uint32_t *work_building;   /* [n_citizens] Citizen::workplace_code (== home when none), citizen.rs:118 */
    const uint32_t *room;            /* [n_citizens] class/office of a school member, else ESIM_NO_ROOM */
    const uint8_t  *flags;           /* [n_citizens] ESIM_FLAG_* */
    const uint16_t *age;             /* [n_citizens] or NULL -- carried for API fidelity, never read per step */
    const uint8_t  *occupation;      /* [n_citizens] or NULL -- idem (simulator_builder.rs:296-300) */
    const uint32_t *building_area;   /* [n_buildings] OutputAreaID::index of the building, building.rs:63 */
    const uint8_t  *building_type;   /* [n_buildings] ESIM_HOUSEHOLD/WORKPLACE/SCHOOL */
    const uint32_t *room_building;   /* [n_rooms] the School each room belongs to */
    const uint32_t *seeds;           /* [n_seeds] local indices starting Infected(0), simulator_builder.rs:1111-1140 */
    const int32_t  *shared_building_local; /* [n_shared_buildings] local building index or -1 */
    const int32_t  *shared_room_local;     /* [n_shared_rooms] local room index or -1 */
} esim_population;

/* One StatisticEntry (sim/src/statistics.rs:208-215) plus what the step decided. */
typedef struct esim_step_result {
    uint32_t time_step, susceptible, exposed, infected, recovered, vaccinated;
    uint32_t exposures_building;     /* successful Citizen::expose calls via buildings, simulator.rs:337-345 */
    uint32_t exposures_bus;          /* ... via PublicTransport, simulator.rs:436-446 */
    uint32_t lockdown;               /* InterventionStatus::lockdown_enabled() after this step */
    uint32_t vaccination_active;     /* vaccination_program_started() after this step */
    uint32_t mask_status;            /* ESIM_MASK_* after this step */
    uint32_t n_riders;               /* citizens on public transport this step */
    uint32_t vaccinated_now;         /* citizens set Vaccinated at the end of this step, simulator.rs:524-553 */
    uint32_t eligible_count;         /* |citizens_eligible_for_vaccine| after this step */
    uint32_t disease_exists;         /* StatisticsRecorder::disease_exists(), statistics.rs:289-291 */
    uint32_t reserved;
} esim_step_result;

typedef struct esim_ctx esim_ctx;

/* DiseaseModel::covid() + Default for InterventionThresholds/InterventionStatus. */
void esim_default_params(esim_params *p);

/* Replaces Simulator::from(SimulatorBuilder) (simulator.rs:601-644): creates the device
 * context; esim_upload_population copies the population to HBM and builds the derived
 * tables (route lists, probability-threshold LUT).  The parameters are checked before the device is touched: ESIM_ERANGE for
 * exposed_time + infected_time + 2 > 512, vaccination_rate > 8192, max_steps outside 1..7600; ESIM_EINVAL for bus_capacity 0,
 * working hours outside 1..23 or with start_hour-1, start_hour, end_hour-1, end_hour not four different hours, and for an
 * exposure_chance that is no probability (NaN, negative, above 1). */
int  esim_create(const esim_params *p, esim_ctx **out);
int  esim_upload_population(esim_ctx *ctx, const esim_population *pop);
/* Back to time step 0 with the uploaded population (all Susceptible, seeds Infected(0)). */
int  esim_reset(esim_ctx *ctx);
/* Back to time step 0 with the uploaded population, as esim_reset, but with the parameters *p in force from here on
 * (seed, exposure_chance, mask_effectiveness, the four thresholds, exposed/infected_time, vaccination_rate, bus_capacity,
 * the hours) and without any host->device traffic proportional to the population: the initial state is rebuilt by
 * kernels on the context's stream.  p->device must be the context's device and p->max_steps at most the max_steps the
 * context was created with (the record log's capacity); p is validated exactly as esim_create validates it, and a refused
 * *p leaves the context as it was.  Nothing waits for the device: the call may return before the work is done, every later
 * call of this context is ordered behind it.  The only host->device copies are the control block and the threshold LUT
 * (4.4 KB).  A context with a communicator of more than one rank returns ESIM_ESTATE (the shards would have to agree on
 * the parameters).  The initially infected citizens stay those in force (the uploaded population's, or the list of the last
 * esim_restart_seeded).  esim_reset afterwards goes back to step 0 under the parameters of the last restart.  Checkpoints: their header is written from the parameters in
 * force, so one saved after a restart goes back only into a context created with, or restarted to, the same parameters. */
int  esim_restart(esim_ctx *ctx, const esim_params *p);
/* esim_restart with other index cases: the citizens seeds[0 .. n_seeds) (local indices, as esim_population.seeds) start
 * Infected(0) instead of the ones in force -- what SimulatorBuilder::apply_initial_infections (simulator_builder.rs:1111-1142)
 * draws anew for every run of the reference.  Duplicates count once, the first occurrence fixes the order in the exposure log
 * (as esim_upload_population treats them); the list may be longer or shorter than the uploaded one, up to n_citizens, or empty.
 * Host->device traffic: what esim_restart copies plus 4 B per distinct seed, from pinned memory; nothing waits for the stream
 * (a list longer than any before makes room on the device first, which does wait for the work still reading the old one).
 * The list stays in force for esim_reset and esim_restart until the next esim_restart_seeded or upload.  Checkpoints: the
 * population hash is finished with the list as given, so a checkpoint saved afterwards goes back into every context whose
 * seeds in force are that same list -- a fresh context uploaded with a population that carries it included -- and no other.
 * Refused, leaving the context as it was: everything esim_restart refuses; seeds == NULL with n_seeds > 0 or an index
 * >= n_citizens (ESIM_EINVAL); n_seeds > n_citizens (ESIM_ERANGE).
 * esim_get_seeds: the distinct seeds in force, in log order; *n_out = their number, ESIM_ERANGE (with *n_out set) when cap is
 * too small.  Pure host code. */
int  esim_restart_seeded(esim_ctx *ctx, const esim_params *p, const uint32_t *seeds, uint32_t n_seeds);
int  esim_get_seeds(esim_ctx *ctx, uint32_t *out, uint32_t cap, uint32_t *n_out);

/* Replaces Simulator::step (simulator.rs:131-152).  out->disease_exists == 0 is the
 * reference's Ok(false). */
int  esim_step(esim_ctx *ctx, esim_step_result *out);
/* Replaces the loop of Simulator::simulate (simulator.rs:114-123): runs up to n_steps on the
 * device without host round trips; stops early when the disease is gone iff stop_when_done.
 * out_array has room for n_steps entries; *n_done receives the number written. */
int  esim_run(esim_ctx *ctx, uint32_t n_steps, int stop_when_done,
              esim_step_result *out_array, uint32_t *n_done);

/* Pipelined chunks.  A citizen exposed in step t is Infected no earlier than t + exposed_time + 1 (disease.rs:47-71).  Hence,
 * while no vaccination programme runs, the Infected census -- and with it every intervention decision (interventions.rs:110-184),
 * the schedule (citizen.rs:176-206) and who marks which building -- is known for the next n <= exposed_time + 1 steps (at most
 * 96): esim_run and esim_run_sharded run such chunks of steps by themselves.
 * esim_set_pipeline(ctx, level): 0 = sequential steps only; 1 = chunks run as one kernel per step (k_pipe);
 * 2 = additionally to 1, when the chunk's marks fit the hash map, ALL steps of a chunk are drawn in one
 * pass (a citizen's exposure step is the earliest step at which any of its draws succeeds -- one atomicMin on
 * the citizen word per successful draw); 3 (default) = as 2, and chunks keep running under a vaccination programme
 * (esim_vax_chunk_stats).  Any level above 3 runs as 3.  esim_chunk_timing: device time (ms), steps and number of such chunks
 * since the last call (measured while kernel timing is enabled). */
/* ---- the exchange between shards, owned by the library ("library owns streams / RCCL communicators") ----
 * esim_comm_unique_id     -- ncclGetUniqueId on one rank (cap >= 128 bytes); the caller carries it to the other ranks
 *                            (the Rust caller over whatever it launches its processes with; bench.py over torch.distributed)
 * esim_comm_init_rccl     -- collective over all ranks: an RCCL communicator on the context's device; every exchange is then
 *                            an ncclAllReduce enqueued on the context's stream between its kernels
 * esim_comm_init_callback -- instead: the caller's own SUM all-reduce over the ranks, in place, of `n_u32` uint32 in HOST memory
 *                            at `host_ptr` (the library stages the device buffer through it with the stream drained; `which`
 *                            names the buffer: 0 A, 1 B, 2 F, 3 plan liveness, 4 commuter records, 5 cuts, 6 records, 7 status,
 *                            8 the set-up's layout check, 9 which shards have members in each shared building);
 *                            returns 0 on success.  For transports other than RCCL and for tests with several ranks on one GPU.
 * esim_run_sharded        -- replaces the loop of Simulator::simulate (simulator.rs:114-123) for this rank's shard: n_steps
 *                            time steps, every rank calling it with the same n_steps; records of these steps hold the census
 *                            of the WHOLE population on every rank. */
/* Set-up.  esim_comm_init_* come AFTER esim_upload_population (a new upload invalidates the communicator) and are collective:
 * the ranks' shards are checked against each other with one small all-reduce -- rank r must hold the r-th stretch of the global
 * citizen ids of ONE world (same n_citizens_global, shared tables of the same size), else ESIM_EINVAL on every rank that sees
 * the mismatch.  world <= 31.
 * Failure semantics (the reference bubbles a failed step() up to main, run/src/main.rs:306-308): the shards' device-side error
 * words are summed in the same collectives that carry the data, and before every read-back of the control block, so ALL ranks
 * return from esim_run_sharded together and with the same ESIM_E* code (records of that call are then undefined); the host's
 * waits on a stream that holds RCCL collectives have a deadline (esim_comm_set_timeout, default 60 s, or ESIM_COMM_TIMEOUT_S):
 * on expiry the communicator is aborted (ncclCommAbort) and the call returns ESIM_ETIMEDOUT -- exit with an error then.
 * esim_run_sharded has no early stop (a shard cannot know that the disease is gone elsewhere): it always runs n_steps.
 * esim_debug_inject_error: diagnostics -- raises a sticky device-side error on this context (tests of the above). */
typedef int (*esim_allreduce_fn)(void *user, int which, void *host_ptr, size_t n_u32);
int  esim_comm_unique_id(void *out, size_t cap);
int  esim_comm_init_rccl(esim_ctx *ctx, const void *unique_id, size_t id_bytes, int rank, int world);
int  esim_comm_init_callback(esim_ctx *ctx, esim_allreduce_fn fn, void *user, int rank, int world);
int  esim_comm_set_timeout(esim_ctx *ctx, double seconds);
int  esim_debug_inject_error(esim_ctx *ctx, int code);
int  esim_comm_stats(esim_ctx *ctx, uint64_t *collectives);
int  esim_run_sharded(esim_ctx *ctx, uint32_t n_steps, uint32_t *n_done);
/* How the steps of sharded runs were executed so far: as time-parallel chunks (one round of exchanges per chunk) / as coupled
 * steps (two exchanges per step). */
int  esim_shard_stats(esim_ctx *ctx, uint64_t *chunk_steps, uint64_t *coupled_steps);
int  esim_set_pipeline(esim_ctx *ctx, int level);
int  esim_chunk_timing(esim_ctx *ctx, double *total_ms, uint64_t *steps, uint64_t *chunks);
/* Device time of the chunk pass per KERNEL (HIP events in front of every kernel of a chunk on the context's stream, resolved at
 * the read-back that ends a burst; a kernel's figure includes the boundary to the next one): accumulated ms and launches since
 * the last call, indexed by ESIM_CK_*.  The reference's three phase timers (simulator.rs:137-143) map onto them as
 * "Generate Exposures" = marks + fold, "Apply Exposures" = draw + units, "Apply Interventions" = everything else (plan,
 * decisions, counts, books, scatter) -- apportioned: a chunk pass works on up to 96 steps at once.  ESIM_CK_TINY: a whole chunk
 * with few Infected in one launch (census ahead, decisions, marks, draws, books): the Python binding shares it out over the
 * three labels by the kernel's own stage timers (entries and keys 10 %, draws 40 %, census, decisions and books 50 %).
 * ESIM_CK_VAX_ADJ and ESIM_CK_MAP_CLEAR always report 0 (their kernels served the persistent item map, which is gone; the
 * indices are kept so that the others keep theirs). */
enum { ESIM_CK_MARKS = 0, ESIM_CK_FOLD, ESIM_CK_DRAW, ESIM_CK_UNITS, ESIM_CK_COUNT, ESIM_CK_BOOKS, ESIM_CK_SCATTER, ESIM_CK_VAX, ESIM_CK_VAX_ADJ,
       ESIM_CK_VAX_FINAL, ESIM_CK_DECIDE, ESIM_CK_FUTURE, ESIM_CK_MAP_CLEAR, ESIM_CK_TINY, ESIM_CK_VAX_REPAIR, ESIM_CK_N };
int  esim_enable_chunk_kernel_timing(esim_ctx *ctx, int enable);
int  esim_chunk_kernel_timings(esim_ctx *ctx, double ms[ESIM_CK_N], uint64_t calls[ESIM_CK_N]);
/* Steps run as time-parallel chunks under a vaccination programme (pipeline level 3: the chunk's vaccinations are planned
 * ahead, simulator.rs:524-553 being a pure function of the step and of citizens_eligible_for_vaccine), and how many of those
 * chunks were cut short because a citizen the plan had chosen left the eligible set on a bus first (simulator.rs:447-449). */
int  esim_vax_chunk_stats(esim_ctx *ctx, uint64_t *steps, uint64_t *cuts);
/* Planned chunks in which a citizen was exposed on a bus before the step the plan vaccinates it in, and whose plan was REPAIRED
 * for the steps behind that exposure (k_chunk_vax<true>: walked again with the eligible set as it truly stood) instead of the
 * chunk being cut there; a chunk is still cut -- behind the step concerned -- when a newly chosen citizen is Infected or
 * exposed later in the chunk.  Sharded runs do the same with two more exchanges per planned chunk (the steps in which a shard lost
 * a citizen, callback `which` 10; the candidates' liveness a second time, `which` 3).  ESIM_VAX_REPAIR=0 switches it off. */
int  esim_vax_repair_stats(esim_ctx *ctx, uint64_t *repairs);
/* Record log read-back: records first..first+n-1 (1-based time steps) of the steps run so far, by whichever call.
 * esim_synchronize waits for all work of this context. */
int  esim_read_records(esim_ctx *ctx, uint32_t first_step, uint32_t n, esim_step_result *out);
int  esim_synchronize(esim_ctx *ctx);

/* Per-citizen state in reference terms, for visualisation / lookup-table sync / checkpoints
 * (replaces reading Simulator.output_areas[..].citizens, run/src/main.rs:246-259,
 * visualisation/src/citizen_connections.rs:40-62).  Any pointer may be NULL.
 *   status  ESIM_* code           (Citizen::disease_status)
 *   timer   Exposed(t)/Infected(t) payload, 0 otherwise
 *   current_building               (Citizen::current_building_position)
 *   on_bus  0 None, 1 (home OA, work OA), 2 (work OA, home OA)   (Citizen::on_public_transport)
 *   eligible member of Simulator::citizens_eligible_for_vaccine  (simulator.rs:97) */
int  esim_download_state(esim_ctx *ctx, uint8_t *status, uint16_t *timer,
                         uint32_t *current_building, uint8_t *on_bus, uint8_t *eligible);
/* Every exposure so far, in time order: the citizen (local index), the time step and whether it happened on public
 * transport -- the calls of StatisticsRecorder::add_exposure (statistics.rs:181-195) that feed exposures.json's
 * per-Output-Area series (statistics.rs:119-136).  A building exposure is credited to the Output Area the citizen stands
 * in at that step (simulator.rs:324 only exposes members whose current area is the building's).  Order inside a time
 * step is unspecified.  *n_out = number of exposures; ESIM_ERANGE (with *n_out set) when cap is too small. */
int  esim_download_exposure_log(esim_ctx *ctx, uint32_t *citizen, uint32_t *step, uint8_t *on_bus, uint32_t cap, uint32_t *n_out);
/* The census by Output Area, counted on the device -- what visualisation draws from output_areas[..].citizens
 * (run/src/main.rs:246-259, visualisation/src/citizen_connections.rs:40-62) without a per-citizen download.
 * counts[area * 5 + status], status = ESIM_SUSCEPTIBLE .. ESIM_VACCINATED, after the last completed step (after
 * esim_reset: everybody Susceptible, the seeds Infected at home).  ESIM_AREA_CURRENT: the Output Area of the building the
 * citizen stands in (what esim_download_state reports as current_building, through building_area); ESIM_AREA_HOME: the
 * area of its household.  Leaves the simulation state as it is.  A sharded context counts its own citizens in its own
 * population's area indices and starts no collective. */
enum { ESIM_AREA_CURRENT = 0, ESIM_AREA_HOME = 1 };
int  esim_area_census(esim_ctx *ctx, int where, uint32_t *counts /* [n_areas * 5] */);
/* When the epidemic reached every Output Area -- the arrival-time map -- from the exposure log where it lies on the device:
 * step_out[a] = the first time step at which a citizen whose household lies in area a was exposed, in a building or on
 * public transport; 0 for the area of an initially infected citizen; ESIM_NEVER for an area not reached in the steps run so
 * far.  where = ESIM_AREA_HOME, or ESIM_BY_GROUP: the same by the citizen's label, [n_groups] (ESIM_ESTATE without labels).
 * ESIM_AREA_CURRENT is not built: ESIM_EINVAL.  Leaves the simulation state as it is.  A sharded context describes its own
 * citizens and starts no collective. */
#define ESIM_NEVER 0xFFFFFFFFu
int  esim_area_arrival(esim_ctx *ctx, int where, uint32_t *step_out /* [n_areas] or [n_groups] */);
/* Per-Output-Area accumulators over the members of an ensemble (runs of one population that differ in seed or parameters,
 * one after another on this context); they live on the device and survive esim_reset and esim_restart.  A new
 * esim_upload_population drops them.  20 bytes per area, allocated at the first begin.
 * begin: zero them and fix what a member contributes -- x[area] = number of citizens whose status after the member's last
 *        completed step is in status_mask (bit s = ESIM_* code s), by ESIM_AREA_HOME or ESIM_AREA_CURRENT.
 * fold:  count x for the state as it stands (as esim_area_census counts) and add, WITHOUT any download or host wait:
 *        members += 1; hit[area] += (x >= min_cases); sum[area] += x; sumsq[area] += x * x.
 * read:  copy out; any pointer may be NULL.
 * The usual risk map ("reached by the epidemic") is the mask Exposed | Infected | Recovered by home area with min_cases 1.
 * ESIM_ESTATE before a population is uploaded, and for fold or read before begin; ESIM_EINVAL for an empty mask, a bit beyond
 * ESIM_VACCINATED or an unknown `where`.  where = ESIM_BY_GROUP: by citizen group instead of by area (esim_set_groups, below).
 * begin_arrival: zero them and fix instead that a member contributes its arrival step, x = what esim_area_arrival(where)
 *        would return: fold then does members += 1 and, where x != ESIM_NEVER and x <= horizon, hit += 1; sum += x;
 *        sumsq += x * x -- again without download or host wait.  hit / members is P(reached by the horizon), sum / hit the mean
 *        arrival step among the members that reached the entry.  horizon = ESIM_NEVER: whatever steps ran.  `where` and the
 *        errors are those of esim_area_arrival; read and the invalidation by esim_set_groups are the same for both kinds. */
int  esim_ensemble_begin(esim_ctx *ctx, int where, uint32_t status_mask, uint32_t min_cases);
int  esim_ensemble_begin_arrival(esim_ctx *ctx, int where, uint32_t horizon);
int  esim_ensemble_fold(esim_ctx *ctx);
int  esim_ensemble_read(esim_ctx *ctx, uint32_t *members, uint32_t *hit /* [n_areas] */,
                        uint64_t *sum /* [n_areas] */, uint64_t *sumsq /* [n_areas] */);
/* Space-time ensembles: the same accumulators over the rows of a series -- P(area a has at least k Infected after step s),
 * the mean and variance of incidence per area and day, a fan chart per age band -- folded on the device, where the series
 * engine leaves a member's rows.
 * begin_series: fix what a member contributes and allocate.  x[row * n_cols + col] is, cell for cell, what the series call that
 *        (where, what) names would return for the member with the same first_step, n_rows and stride:
 *          where = ESIM_AREA_HOME or ESIM_AREA_CURRENT, what = ESIM_SUSCEPTIBLE .. ESIM_VACCINATED
 *                                                     esim_area_status_series(where, what)
 *          where = ESIM_AREA_HOME,    what = 5        esim_area_status_series(ESIM_AREA_HOME, ESIM_AREA_SERIES_INCIDENCE)
 *          where = ESIM_AREA_CURRENT, what = 5        esim_area_series(ESIM_SERIES_EXPOSURES)
 *          where = ESIM_BY_GROUP,     what = 0 .. 5   esim_group_series(what)
 *        n_cols = n_areas, or n_groups by group.  Held on the device from here on: hit (u32), sum and sumsq (u64) per cell --
 *        20 B per cell -- and the member counter, zeroed on the stream; the row plane the engine writes into, 4 B per cell, two
 *        of them for status rows by ESIM_AREA_CURRENT; 8 B per column of occupancy and 1 B per step of the record log's
 *        capacity (also pinned on the host); and, from the first fold under a vaccination programme on, the 4 B per citizen
 *        of the vaccination replay.  A fold allocates nothing proportional to rows x columns.  A begin with the same n_rows,
 *        n_cols and number of planes zeroes what is there; any other shape is allocated first and the earlier one freed then,
 *        so ESIM_ENOMEM leaves the context and every earlier accumulator as they were.  The accumulators of the other two
 *        kinds are left alone, and theirs leave these alone: one kind is in force at a time, a begin of any kind replaces it.
 *        ESIM_EINVAL: a null context, an unknown `where` or `what`, stride 0, no rows.  ESIM_ESTATE: before a population is
 *        uploaded; by group without labels; on a context whose communicator has more than one rank (the rule of
 *        esim_restart).  ESIM_ERANGE: first_step == 0.  ESIM_ENOMEM: no device memory.
 * fold:  esim_ensemble_fold with this kind in force runs the series engine for the state as it stands into the kept planes and
 *        then one pass over the cells: members += 1; hit[cell] += (x >= min_cases); sum[cell] += x; sumsq[cell] += x * x.
 *        Nothing proportional to rows x columns goes to the host.  Unlike the other two kinds it WAITS FOR THE STREAM ONCE, in
 *        front of its own work: the at-work bit of every step and the step that started the vaccination programme are derived
 *        on the host from the records (64 B per step run), as the series calls derive them.  ESIM_ERANGE, with nothing folded
 *        and members as it was, when the last row's step lies beyond the steps the member has run (a member that stopped early
 *        has no rows behind its last step); a sticky device-side error and the ESIM_ESTATE of a shard under a vaccination
 *        programme are reported as the series calls report them.  Leaves the simulation state, the records, the snapshot and
 *        the group labels as they are.
 * read_series: rows [first_row, first_row + n) of the accumulators, hit[(r - first_row) * n_cols + col] and the same for sum and
 *        sumsq; any pointer may be NULL.  ESIM_ERANGE for rows outside the accumulators; ESIM_ESTATE when no series kind is in
 *        force -- and esim_ensemble_read is ESIM_ESTATE while one is.
 * Lifetime as above: kept through esim_reset, esim_restart, esim_restart_seeded, esim_rollback and esim_snapshot, dropped by a
 * new upload and by esim_destroy, invalidated by esim_set_groups when begun by group. */
int  esim_ensemble_begin_series(esim_ctx *ctx, int where, int what, uint32_t first_step, uint32_t n_rows, uint32_t stride,
                                uint32_t min_cases);
int  esim_ensemble_read_series(esim_ctx *ctx, uint32_t first_row, uint32_t n, uint32_t *members, uint32_t *hit /* [n * n_cols] */,
                               uint64_t *sum /* [n * n_cols] */, uint64_t *sumsq /* [n * n_cols] */);
/* The same picture for the steps already run, derived after the fact from what the device holds (exposure log, citizen
 * words, the records' lockdown flags): a run that never asks pays nothing.  Row i describes step
 * s_i = first_step + i * stride (1-based, s_i <= steps run so far), out[i * n_areas + area]:
 *   ESIM_SERIES_INFECTED   citizens Infected after step s_i, by the area they stand in then -- column ESIM_INFECTED of
 *                          what esim_area_census(ESIM_AREA_CURRENT) would have returned had it been called after step s_i
 *                          (a citizen set Vaccinated at the end of a step is not Infected after it; the record's `infected`
 *                          is the census before that, simulator.rs:178);
 *   ESIM_SERIES_EXPOSURES  building exposures (not public transport) of steps [s_i, s_i + stride), clipped to the steps
 *                          run, credited to the area the citizen stands in at that step (statistics.rs:186-190,
 *                          simulator.rs:324) -- with stride 1, the dense form of exposures.json's "OutputArea" series
 *                          (statistics.rs:119-136).
 * ESIM_ERANGE: first_step == 0 or the last row's step beyond the steps run; ESIM_ENOMEM: no device memory for the rows
 * (ask for fewer).  The step at which somebody was vaccinated is not kept per citizen: under a vaccination programme the
 * Infected rows walk the choice of simulator.rs:524-553 again for the steps run (4 B per citizen of temporary device
 * memory); a sharded context cannot (the choice depends on the other shards' citizens) and returns ESIM_ESTATE for the
 * Infected rows once a programme has run.  Otherwise a sharded context describes its own citizens, as above. */
enum { ESIM_SERIES_INFECTED = 0, ESIM_SERIES_EXPOSURES = 1 };
int  esim_area_series(esim_ctx *ctx, int what, uint32_t first_step, uint32_t n_rows, uint32_t stride,
                      uint32_t *out /* [n_rows * n_areas] */);
/* All five statuses per Output Area over the steps already run, and the new cases by area of residence -- the attack-rate map
 * (Recovered by household area), the vaccination-coverage map and the surveillance view of incidence over time -- derived after
 * the fact like the rows above and addressed like them: row i describes step s_i = first_step + i * stride,
 * out[i * n_areas + area].
 *   what = ESIM_SUSCEPTIBLE .. ESIM_VACCINATED, where = ESIM_AREA_CURRENT or ESIM_AREA_HOME
 *                          column `what` of what esim_area_census(where) would have returned had it been called after step
 *                          s_i, i.e. the state after the step's vaccinations (the convention of the area and group tables);
 *   what = ESIM_AREA_SERIES_INCIDENCE, where = ESIM_AREA_HOME only
 *                          exposures of steps [s_i, s_i + stride), clipped to the steps run, credited to the Output Area of
 *                          the exposed citizen's household: buildings AND public transport; the initially infected citizens
 *                          are not counted.  (By the area stood in it is ESIM_EINVAL: esim_area_series(ESIM_SERIES_EXPOSURES)
 *                          is that table, and a bus has no area.)
 * ESIM_EINVAL: a null context or output, an unknown `where` (ESIM_BY_GROUP included) or `what`, stride 0, no rows; ESIM_ESTATE
 * before a population is uploaded; ESIM_ERANGE: first_step == 0 or the last row's step beyond the steps run; ESIM_ENOMEM: no
 * device memory for the rows (ask for fewer).  A sharded context describes its own citizens and starts no collective; its
 * status rows return ESIM_ESTATE once a vaccination programme has run (the rule of esim_area_series), its incidence rows stay
 * available.  Leaves the simulation state, the records, the ensemble accumulators and the group labels as they are.
 * Limits (temporary device memory): n_rows * n_areas * 4 B for rows by household area and for incidence, twice that for rows by
 * the area stood in (one plane per value of the at-work bit) plus 1 B per step run; 4 B per area and plane of occupancy for
 * the Susceptible rows; 4 B per citizen for the status rows once a vaccination programme has run (the choice of
 * simulator.rs:524-553 is walked again).
 * The work per exposure-log entry and per vaccinated citizen does not depend on the number of steps run. */
enum { ESIM_AREA_SERIES_INCIDENCE = 5 };       /* `what` of esim_area_status_series, beside the five status codes */
int  esim_area_status_series(esim_ctx *ctx, int where, int what, uint32_t first_step, uint32_t n_rows, uint32_t stride,
                             uint32_t *out /* [n_rows * n_areas] */);
/* Stratified outputs: the same read-backs by citizen GROUP -- an age band, an occupation, any label of the caller's.
 * esim_set_groups copies one label per local citizen to the device (2 B per citizen; no host pointer is kept) and counts the
 * groups' sizes once.  1 <= n_groups <= ESIM_MAX_GROUPS; a label >= n_groups is ESIM_EINVAL (checked on the host during the
 * copy) and leaves the context as it was; group == NULL drops the labels.  ESIM_ESTATE before a population is uploaded and on
 * a context whose communicator has more than one rank (the rule of esim_restart: sharded groups are not built, and the other
 * group calls answer the same there).  The labels survive esim_reset, esim_restart and esim_checkpoint_restore; a new
 * esim_upload_population drops them.  They are no simulation state: no checkpoint holds them, the population hash does not
 * cover them.  A later call replaces them and invalidates ensemble accumulators begun by group (fold and read then return
 * ESIM_ESTATE until the next begin).
 * esim_group_census: counts[g * 5 + status] after the last completed step, with the semantics of esim_area_census (after
 * esim_reset: everybody Susceptible, the seeds Infected).  Leaves the simulation state as it is.  ESIM_ESTATE without labels.
 * esim_group_series: row i describes step s_i = first_step + i * stride, addressed as esim_area_series addresses its rows
 * and with its ESIM_ERANGE / ESIM_ENOMEM rules, out[i * n_groups + g]:
 *   what = ESIM_SUSCEPTIBLE .. ESIM_VACCINATED   citizens of group g with that status after step s_i -- that column of what
 *                          esim_group_census would have returned after s_i, i.e. the state after the step's vaccinations
 *                          (the convention of the area tables);
 *   ESIM_GROUP_SERIES_EXPOSURES   exposures of steps [s_i, s_i + stride), clipped to the steps run, by the group of the
 *                          exposed citizen: buildings AND public transport (a group has no location); the initially
 *                          infected citizens are not counted.
 * Limits: a row buffer of (n_rows + 1) * n_groups * 4 B on the device, and, once a vaccination programme has run, 4 B per
 * citizen of temporary device memory for the status rows (the choice of simulator.rs:524-553 is walked again, as for
 * esim_area_series).
 * Ensembles: esim_ensemble_begin with where = ESIM_BY_GROUP sizes the accumulators by n_groups, x[g] = the citizens of group
 * g whose status is in status_mask; fold and read then run over n_groups entries.  ESIM_ESTATE without labels. */
#define ESIM_MAX_GROUPS 1024
enum { ESIM_BY_GROUP = 2 };                    /* `where` of esim_ensemble_begin, beside ESIM_AREA_CURRENT and ESIM_AREA_HOME */
enum { ESIM_GROUP_SERIES_EXPOSURES = 5 };      /* `what` of esim_group_series, beside the five status codes */
int  esim_set_groups(esim_ctx *ctx, const uint16_t *group /* [n_citizens] */, uint32_t n_groups);
int  esim_group_census(esim_ctx *ctx, uint32_t *counts /* [n_groups * 5] */);
int  esim_group_series(esim_ctx *ctx, int what, uint32_t first_step, uint32_t n_rows, uint32_t stride,
                       uint32_t *out /* [n_rows * n_groups] */);
/* Where infections happen: every exposure by SETTING -- household, work place, school, public transport -- and by the building
 * credited (the reference's ID::Building / ID::PublicTransport tally, statistics.rs:105-106,181-195), derived after the fact
 * from what the device holds: a run that never asks pays nothing, and no step kernel knows of it.  Every draw is a pure function
 * of (seed, global citizen, step, slot), and a building exposure of citizen c in step ts can only have come through the list of
 * its household or through its work-side list, so one replay of the household draw decides it.  The rule, per entry of the
 * exposure log (the initially infected citizens are in the log and get ESIM_SETTING_NONE):
 *   1. exposed on public transport -> ESIM_SETTING_TRANSPORT, no building;
 *   2. n_home = the residents of the household that are Infected in step ts (their exposure steps taken from the log; still
 *      Infected in the step at whose end they were vaccinated, which is walked again as for the series) and stand in it: not on
 *      a bus and not at work in that step, both global bits per step derived from the records' lockdown flags;
 *   3. c takes the household draw iff n_home > 0 and it stands in the household's area (always, except a commuter to another
 *      area while at work); the draw succeeds iff its Philox word of slot 0 lies below thresholds[row][n_home & 255], row as
 *      the step drew it (esim_threshold_lut; 256 Infected give threshold 0, the `as u8` of citizen.rs:239);
 *   4. success -> ESIM_SETTING_HOUSEHOLD, the household's building;
 *   5. otherwise the work side: ESIM_SETTING_SCHOOL for a school member, else ESIM_SETTING_WORKPLACE, the work building --
 *      legal only for a citizen with a work place that is in its home area or at work in that step.  An entry for which
 *      neither side is possible is UNEXPLAINED: they are counted on the device, carry ESIM_SETTING_NONE, and the call returns
 *      ESIM_ESIM with their number in esim_last_error after delivering everything else.  On a correct run there is none: the
 *      calls double as an audit of the log.
 * The tie is a stated contract: when the household draw and a work-side draw both succeed in one step, the HOUSEHOLD is
 * credited.  (The reference credits whichever building its hash map visits first: no rule.  The work side is never replayed by these three
 * calls; esim_transmission_tree and its kin, below, walk it.)
 * After an esim_rollback under another seed, exposure_chance or mask_effectiveness the entries up to the snapshot's step are
 * replayed under the snapshot's values and the later ones under those in force; a snapshot taken on such a branch and rolled
 * back to under yet other values is ESIM_ESTATE here (a history mixed twice is not built).
 * esim_exposure_settings: setting[c] and building[c] per citizen; ESIM_SETTING_NONE / ESIM_NO_ROOM for a citizen never
 *        exposed and for the initially infected, ESIM_NO_ROOM for public transport.  Either pointer may be NULL; with both
 *        NULL the audit still runs and its result is returned.
 * esim_setting_series: event rows addressed and clipped exactly as the incidence rows of esim_area_status_series -- row i holds
 *        the exposures of steps [first_step + i * stride, + stride), buildings and public transport, the initially infected
 *        not counted -- restricted to the settings whose bit (1 << ESIM_SETTING_*) is in setting_mask:
 *          where = ESIM_BY_SETTING   4 columns, out[i * 4 + setting]
 *          where = ESIM_AREA_HOME    n_areas columns, by the Output Area of the household
 *          where = ESIM_BY_GROUP     n_groups columns (ESIM_ESTATE without labels)
 *        ESIM_AREA_CURRENT is ESIM_EINVAL (a bus has no area), and so are an empty mask and a bit beyond ESIM_SETTING_TRANSPORT.
 * esim_building_exposures: counts[b] = the exposures of steps [first_step, last_step] credited to building b, the hot-spot map;
 *        public transport is not counted.  ESIM_ERANGE: first_step == 0, last_step < first_step or beyond the steps run.
 * All three: ESIM_EINVAL for a null context or output and unknown arguments; ESIM_ESTATE before an upload and on a context
 * whose communicator has more than one rank (the rule of esim_restart) or that holds a shard; ESIM_ESTATE, too, on a
 * population in which a Household is the work_building of a citizen who does not live in it (found once, at the upload): rule 2
 * counts the residents only, the workers standing in such a household would be missing from n_home, and exposures would be
 * credited to the wrong setting, most of them without becoming unexplained.  esim_run, the records, the exposure log and every
 * output that replays no draw (the census, the series, the arrival times, esim_curve_summary) take such a population as any
 * other; every call below that builds on the settings -- the tree, the chains, the household and place outbreaks, the flows,
 * the events, the contact-hours, the ensemble kinds that fold them -- refuses it in the same way.  ESIM_ERANGE / ESIM_ENOMEM as
 * the series calls give them; a sticky device-side error is reported as the series calls report it.  They leave the
 * simulation state, the records, the snapshot, the ensemble accumulators and the labels as they are.  Temporary device memory,
 * freed when the call returns: 4 B per citizen for the exposure steps, 1 B per citizen for the setting, 1 B per step for each
 * of the two bits, 4 B per citizen for the vaccination replay once a programme has run, 4 KB for the earlier LUT behind a
 * seam, and the rows or the building table (4 B per cell).  The work per exposure is one walk over its household. */
enum { ESIM_SETTING_HOUSEHOLD = 0, ESIM_SETTING_WORKPLACE = 1, ESIM_SETTING_SCHOOL = 2, ESIM_SETTING_TRANSPORT = 3, ESIM_N_SETTINGS = 4 };
#define ESIM_SETTING_NONE 0xFFu
enum { ESIM_BY_SETTING = 3 };                  /* `where` of esim_setting_series, beside ESIM_AREA_HOME and ESIM_BY_GROUP */
int  esim_exposure_settings(esim_ctx *ctx, uint8_t *setting /* [n_citizens] or NULL */, uint32_t *building /* [n_citizens] or NULL */);
int  esim_setting_series(esim_ctx *ctx, int where, uint32_t setting_mask, uint32_t first_step, uint32_t n_rows, uint32_t stride,
                         uint32_t *out /* [n_rows * n_cols] */);
int  esim_building_exposures(esim_ctx *ctx, uint32_t first_step, uint32_t last_step, uint32_t *counts /* [n_buildings] */);
/* Who infected whom: the transmission tree, the offspring of every citizen, the reproduction number by cohort and the
 * who-acquires-infection-from-whom matrix between citizen groups, derived after the fact like the settings above and on top of
 * them.  (The reference cannot say: its exposure chance is 1 - (1 - p)^n over the n Infected present, no infector is recorded.)
 * The rule, per entry (c, ts) of the exposure log with ts >= 1, its setting and building as esim_exposure_settings gives them,
 * the tie rule included.  The CANDIDATES are the citizens that are Infected after the tick of step ts and stand where the
 * exposure is credited.  Infected in ts: the exposure step comes from the log, exposed_time + 1 steps later the
 * infected_time + 1 Infected steps follow; an Infected citizen is still Infected in the step at whose end it was vaccinated;
 * the index cases are Infected from step 1.
 *   household         the residents of c's household that are Infected in ts and at home: not on a bus and not at work in that
 *                     step (the n_home of rule 2 above);
 *   work place        the workers of c's work building that are Infected in ts, at work and not on a bus (the bus hour before
 *                     end_hour has both bits set: an Infected rider marks no building then);
 *   school            the participants of c's own ROOM under the same predicate (the school draws one copy of the room per
 *                     Infected in it: the infector is somebody of that room, not of the school);
 *   public transport  the Infected riders of c's bus: the riders of c's route (home area, work area) ordered by (key, position in
 *                     the route), key = word 0 of Philox4x32-10 over (global citizen, ts, ESIM_SLOT_BUS_ORDER, 0) under the seed --
 *                     the step is the counter word itself --, bus = rank / bus_capacity; a route of at most bus_capacity riders is
 *                     one bus and needs no keys.
 * With k candidates in ascending local citizen index and u the 32-bit Philox word of (seed, global citizen c, ts, slot 5 =
 * ESIM_SLOT_INFECTOR), the infector is candidate number ((uint64_t)u * k) >> 32.  This is a stated contract as the tie rule is:
 * given that the exposure happened, every Infected present is equally likely to be its source, and the draw makes the tree
 * reproducible.  k = 0 means the log holds an exposure nobody can have caused: such entries are counted on the device, get
 * ESIM_NO_INFECTOR, and the call returns ESIM_ESIM with their number in esim_last_error after delivering everything else -- the
 * audit of the settings, now for the work side and the buses too.  Index cases and citizens never exposed: ESIM_NO_INFECTOR.
 * Generation: 0 for an index case, the infector's + 1 otherwise, ESIM_NEVER for a citizen never exposed or unexplained.
 * After an esim_rollback under another seed the bus keys and the pick of the entries up to the snapshot's step use the
 * snapshot's seed, as the household replay does.  After a rollback that changed bus_capacity these calls are ESIM_ESTATE (a bus
 * replay under two capacities is not built) until an esim_restart, esim_reset or upload; on a sharded context, on a history
 * mixed twice and on a population with a household that is somebody else's work place they are ESIM_ESTATE as the calls above.
 * esim_transmission_tree: infector[c], n_candidates[c] (the k of c's exposure, 0 where there is none) and generation[c] per
 *        citizen.  Any pointer may be NULL; with all three NULL the audit still runs and its result is returned.
 * esim_offspring: counts[j] = the citizens exposed in steps [first_step, last_step] whose infector is j.  ESIM_ERANGE as
 *        esim_building_exposures gives it.
 * esim_reproduction_series: row i is the COHORT exposed in steps [first_step + i * stride, + stride), clipped to the steps run;
 *        first_step 0 is allowed here and only here: the index cases are the cohort of step 0.  cases[i * n_cols + col] is the
 *        size of the cohort, offspring[...] the citizens whose infector lies in that cohort and column -- the column is the
 *        infector's.  offspring / cases is the case reproduction number of the cohort.  Either output may be NULL, not both.
 *          where = ESIM_BY_ALL       one column
 *          where = ESIM_AREA_HOME    n_areas columns, by the Output Area of the household
 *          where = ESIM_BY_GROUP     n_groups columns (ESIM_ESTATE without labels)
 *        Any other `where`, ESIM_AREA_CURRENT included, is ESIM_EINVAL, as are stride 0 and no rows; ESIM_ERANGE for rows outside
 *        the steps run.  A row is COMPLETE -- later steps add nothing to it -- once the last Infected step of a citizen exposed
 *        in the row's last step s has run: s + exposed_time + 1 + infected_time <= the steps run so far.
 * esim_mixing_matrix: counts[g_infector * n_groups + g_infectee] over the transmissions of steps [first_step, last_step] whose
 *        setting has its bit in setting_mask.  ESIM_ESTATE without labels; the mask's errors are those of esim_setting_series,
 *        ESIM_ERANGE as esim_building_exposures gives it.
 * All four leave the simulation state, the records, the snapshot, the ensemble accumulators and the labels as they are.
 * Temporary device memory, freed when the call returns: that of the settings above; 4 B per citizen each for the infector, k and
 * the generation; 4 B per entry of the exposure log for the queue of the exposures outside households; the rows or the table
 * (4 B per cell).  The work per exposure is one walk, by a whole wavefront, over the members of the place credited; on a route
 * longer than a bus every Infected rider is ranked against all riders of the route. */
#define ESIM_NO_INFECTOR 0xFFFFFFFFu
enum { ESIM_BY_ALL = 4 };                      /* `where` of esim_reproduction_series, beside ESIM_AREA_HOME and ESIM_BY_GROUP */
int  esim_transmission_tree(esim_ctx *ctx, uint32_t *infector /* [n_citizens] or NULL */, uint32_t *n_candidates /* [n_citizens] or NULL */,
                            uint32_t *generation /* [n_citizens] or NULL */);
int  esim_offspring(esim_ctx *ctx, uint32_t first_step, uint32_t last_step, uint32_t *counts /* [n_citizens] */);
int  esim_reproduction_series(esim_ctx *ctx, int where, uint32_t first_step, uint32_t n_rows, uint32_t stride,
                              uint32_t *cases /* [n_rows * n_cols] or NULL */, uint32_t *offspring /* [n_rows * n_cols] or NULL */);
int  esim_mixing_matrix(esim_ctx *ctx, uint32_t setting_mask, uint32_t first_step, uint32_t last_step,
                        uint32_t *counts /* [n_groups * n_groups] */);
/* Ensemble maps of transmission: two more kinds of the accumulators over rows of esim_ensemble_begin_series, for the two
 * transmission outputs that are rows already -- "how often does an area see at least k household-acquired cases in the week
 * after the lockdown", "in how many futures is R at least 1 in this area this week" -- folded on the device where the replay
 * leaves a member's rows.  One kind of accumulator is in force at a time (census, arrival, series, settings, reproduction); a
 * begin of any kind replaces it.  Lifetime as for esim_ensemble_begin_series: kept through esim_reset, esim_restart,
 * esim_restart_seeded, esim_snapshot and esim_rollback, dropped by a new upload and by esim_destroy, invalidated by
 * esim_set_groups when begun by group.  A begin with the kind, n_rows and n_cols in force zeroes what is there; any other shape
 * is allocated first and the earlier one freed then, so ESIM_ENOMEM leaves the context and every earlier accumulator as they
 * were.  A run that never asks pays nothing.
 * begin_settings: x[row * n_cols + col] is, cell for cell, what esim_setting_series(where, setting_mask, first_step, n_rows,
 *        stride) would return for the member; where = ESIM_BY_SETTING (4 columns), ESIM_AREA_HOME or ESIM_BY_GROUP.  The
 *        accumulators are those of the series kind -- hit (u32), sum and sumsq (u64) per cell, 20 B, and the member counter --
 *        beside one row plane of 4 B per cell; a fold adds members += 1; hit += (x >= min_cases); sum += x; sumsq += x * x, and
 *        esim_ensemble_read_series reads them.  ESIM_EINVAL: a null context, any other `where`, a mask that is empty or names a
 *        setting beyond ESIM_SETTING_TRANSPORT, stride 0, no rows.  ESIM_ESTATE: before a population is uploaded; by group
 *        without labels; on a context whose communicator has more than one rank.  ESIM_ERANGE: first_step == 0.
 * begin_reproduction: a member contributes the cohort rows of esim_reproduction_series(where, first_step, n_rows, stride), c =
 *        cases[cell] and o = offspring[cell]; where = ESIM_BY_ALL (one column), ESIM_AREA_HOME or ESIM_BY_GROUP; first_step 0
 *        is allowed, as there.  A fold adds members += 1 once and per cell
 *          if c >= min_cohort:  defined += 1, and hit += 1 iff (uint64_t)o * r_den >= (uint64_t)c * r_num
 *          always:              sum_cases += c; sum_offspring += o; sumsq_cases += c * c; sumsq_offspring += o * o;
 *                               sum_cross += c * o
 *        in integers: two u32 and five u64 per cell, 48 B, beside two row planes of 4 B per cell each.  sum_offspring /
 *        sum_cases is the pooled R of the cell, hit / defined is P(R >= r_num / r_den) among the members that had a cohort
 *        there, and the five sums give the delta-method variance of the ratio over members.  A row whose cohort can still
 *        infect (esim_reproduction_series: not COMPLETE) biases R down; the window is the caller's to choose.  ESIM_EINVAL: a
 *        null context, any other `where`, stride 0, no rows, min_cohort == 0, r_den == 0.  ESIM_ESTATE as begin_settings.
 * fold:  esim_ensemble_fold with one of the two in force first makes the checks of the series call the kind stands for --
 *        ESIM_ESTATE on a sharded context, on a history mixed twice and, the reproduction kind, after a rollback under another
 *        bus_capacity; ESIM_ERANGE when the last row lies beyond the steps the member has run -- and on any of them folds
 *        nothing and leaves members as it was.  Then, on the context's stream: the kept plane(s) zeroed, the replay of the
 *        settings (and of the tree, without generations), the rows into the kept planes, one pass over the cells.  It WAITS FOR
 *        THE STREAM, as every call on top of the replay does, and reports the audits their way: the member IS folded, then
 *        ESIM_ESIM is returned with the count in esim_last_error.  Nothing proportional to rows x columns goes to the host or is
 *        allocated; the replay's temporaries are those of esim_setting_series / esim_reproduction_series without their rows.
 *        Leaves the simulation state, the records, the exposure log, the snapshot and the labels as they are.
 * read_reproduction: rows [first_row, first_row + n) of the accumulators of the reproduction kind, [(r - first_row) * n_cols +
 *        col] each; members is one counter; any pointer may be NULL.  ESIM_ERANGE for rows outside the accumulators; ESIM_ESTATE
 *        when another kind is in force -- and esim_ensemble_read and esim_ensemble_read_series are ESIM_ESTATE while this one
 *        is (esim_ensemble_read_series serves the settings kind). */
int  esim_ensemble_begin_settings(esim_ctx *ctx, int where, uint32_t setting_mask, uint32_t first_step, uint32_t n_rows,
                                  uint32_t stride, uint32_t min_cases);
int  esim_ensemble_begin_reproduction(esim_ctx *ctx, int where, uint32_t first_step, uint32_t n_rows, uint32_t stride,
                                      uint32_t min_cohort, uint32_t r_num, uint32_t r_den);
int  esim_ensemble_read_reproduction(esim_ctx *ctx, uint32_t first_row, uint32_t n, uint32_t *members,
                                     uint32_t *defined /* [n * n_cols] */, uint32_t *hit /* [n * n_cols] */,
                                     uint64_t *sum_cases /* [n * n_cols] */, uint64_t *sum_offspring /* [n * n_cols] */,
                                     uint64_t *sumsq_cases /* [n * n_cols] */, uint64_t *sumsq_offspring /* [n * n_cols] */,
                                     uint64_t *sum_cross /* [n * n_cols] */);
/* Transmission chains: which introduction a case descends from, how large the outbreak is that a citizen started, and when
 * during their infectious period people transmit -- functions of the tree above, computed where it lies, so that nothing of
 * size [n_citizens] has to go to the host for them.  Per entry (c, ts) of the exposure log; infector, generation and setting
 * as esim_transmission_tree and esim_exposure_settings define them, the tie rule and the seam of a rollback included.
 *   lineage[c]      the ordinal, in the order of esim_get_seeds, of the index case at the root of c's chain.  An index case
 *                   carries its own ordinal; a citizen never exposed, and one whose chain passes through an exposure without a
 *                   candidate (generation == ESIM_NEVER), carries ESIM_NO_LINEAGE.
 *   descendants[c]  the citizens in the subtree below c, c itself not counted: 0 for a citizen that infected nobody or was
 *                   never exposed.  A subtree that reaches no index case still counts inside itself.
 *   outbreak of index case i:  size[i] = descendants[seed i]; depth[i] the largest generation among the citizens of lineage i
 *                   (0 when it infected nobody); last_step[i] the last exposure step among them (0 when none).
 *   infectious age of a transmission:  a = ts - onset(infector), onset = te + exposed_time + 1 for an infector whose exposure
 *                   step te is in the log, 0 for an index case (Infected from step 1).  0 <= a <= infected_time on a correct
 *                   run, and esim_create enforces exposed_time + infected_time + 2 <= 512, so ESIM_AGE_BINS bins always
 *                   suffice.  For an infector that is not an index case the GENERATION INTERVAL -- from its own exposure to
 *                   the exposure it caused -- is a + exposed_time + 1.
 * esim_transmission_chains: lineage and descendants per citizen.  Either pointer may be NULL; with both NULL the audits still
 *        run and their result is returned.
 * esim_outbreaks: size, depth and last_step per index case, [cap] each, any may be NULL.  *n_out receives the number of
 *        distinct seeds in force; ESIM_ERANGE, with *n_out set, when cap is smaller (the rule of esim_get_seeds); ESIM_EINVAL
 *        for a null n_out.  12 B per seed go to the host and nothing per citizen.
 * esim_transmission_ages: counts[setting * ESIM_AGE_BINS + a] over the transmissions of steps [first_step, last_step] (the
 *        step is the infectee's).  ESIM_EINVAL for a null output, ESIM_ERANGE as esim_offspring gives it.  A transmission with
 *        a outside 0 .. infected_time is impossible on a correct run: such entries are skipped and counted on the device, and
 *        the call returns ESIM_ESIM with their number in esim_last_error after delivering everything else, as the exposures
 *        without a candidate are reported above.
 * The audits of the calls above run in all three (ESIM_ESIM after delivering everything else), and esim_transmission_chains
 * and esim_outbreaks add one: an exposure whose chain does not end at an index case is counted and reported the same way.
 * Refused as the four calls above: ESIM_ESTATE before an upload, on a sharded context, on a history mixed twice and after a
 * rollback under another bus_capacity.  All three leave the simulation state, the records, the exposure log, the snapshot, the
 * ensemble accumulators and the labels as they are, and derive the tree anew (nothing is kept between calls).
 * Temporary device memory, freed when the call returns: that of esim_transmission_tree; 4 B per citizen each for the lineage
 * and the descendants (esim_transmission_ages: neither); 12 B per seed and the 8 KB of the age table.  Lineage and descendants
 * take one launch each per window of exposed_time + 1 steps, as the generations do: with exposed_time == 0 that is a launch
 * per step. */
#define ESIM_NO_LINEAGE 0xFFFFFFFFu
#define ESIM_AGE_BINS   512
int  esim_transmission_chains(esim_ctx *ctx, uint32_t *lineage /* [n_citizens] or NULL */, uint32_t *descendants /* [n_citizens] or NULL */);
int  esim_outbreaks(esim_ctx *ctx, uint32_t *size, uint32_t *depth, uint32_t *last_step /* [cap] each, any may be NULL */,
                    uint32_t cap, uint32_t *n_out);
int  esim_transmission_ages(esim_ctx *ctx, uint32_t first_step, uint32_t last_step, uint32_t *counts /* [ESIM_N_SETTINGS * ESIM_AGE_BINS] */);
/* Household outbreaks: the household is the one setting with a fixed contact list, so the outputs above get a denominator there --
 * the household SECONDARY ATTACK RATE (of the housemates still Susceptible when a case became infectious, the share that case
 * infected at home) and the FINAL-SIZE distribution (how many households of size n ended with k cases, and how many of those
 * were introduced from outside).  Computed on the device from the resident lists, the exposure log, the vaccination replay and
 * the tree; nothing of size [n_citizens] goes to the host.  (The reference cannot give them: it records no infector.)  Settings,
 * infectors and the tie rule are those of esim_exposure_settings and esim_transmission_tree, the seam of a rollback included.
 *   household      a building with at least one resident (a citizen whose home_building it is); its size is their number.
 *   case           a citizen in the exposure log, the index cases included.  Its cohort step te is its exposure step, 0 for an
 *                  index case; onset = te + exposed_time + 1, 0 for an index case; its first infectious step f = max(onset, 1)
 *                  -- the conventions of esim_reproduction_series and esim_transmission_ages.
 *   at risk        housemate m != j of case j is at risk from j iff m is Susceptible after step f_j - 1 ("after step 0": the
 *                  initial state; the state after a step includes that step's vaccinations, as in the area and group tables).
 *                  With sus_until[m] the smaller of (exposure step of m) - 1 and (step at whose end m was set Vaccinated) - 1,
 *                  whichever exist -- -1 for an index case, unbounded for a citizen never touched --: sus_until[m] >= f_j - 1.
 *                  A case with f_j beyond the steps run has not become infectious and contributes nothing.
 *   secondary case an at-risk housemate m of j with infector[m] == j and setting[m] == ESIM_SETTING_HOUSEHOLD.  Everybody that
 *                  j infected at home is at risk from j by construction: secondary <= at_risk cell for cell.
 *   per household  cases[b]: its residents that are cases; introductions[b]: of those, the index cases and the cases whose
 *                  setting is not ESIM_SETTING_HOUSEHOLD (work place, school, transport, unexplained entries); first_step[b]:
 *                  the smallest cohort step among its cases, ESIM_NEVER without one.  All 0 / ESIM_NEVER for a building
 *                  nobody lives in.
 * esim_household_outbreaks: the three per building, any may be NULL.
 * esim_household_final_sizes: final_size[min(size, 63) * ESIM_HH_BINS + min(cases, 63)] counts the households, introductions[...]
 *        the same with min(introductions, 63) as the second index; either may be NULL.  32 KB go to the host and nothing per
 *        building or per citizen.
 * esim_household_sar: the pairs (case j, housemate at risk from j) in at_risk, those that are secondary cases in secondary, over
 *        the cases whose cohort step lies in [first_step, last_step] and that have become infectious (f_j <= the steps run).
 *          where = ESIM_BY_ALL       one cell
 *          where = ESIM_BY_GROUP     n_groups x n_groups, index g_case * n_groups + g_contact (ESIM_ESTATE without labels)
 *        Any other `where` is ESIM_EINVAL.  first_step 0 is allowed, as for the reproduction rows, and brings in the index cases.
 *        ESIM_ERANGE for last_step < first_step or last_step beyond the steps run.  Either output may be NULL, not both
 *        (ESIM_EINVAL).  secondary / at_risk is the secondary attack rate.  A cohort is COMPLETE -- later steps add no secondary
 *        case to it -- once the last Infected step of a citizen exposed in step last_step has run: last_step + exposed_time + 1 +
 *        infected_time <= the steps run so far.  The counters are 64 bits wide, on the device too: a cell holds up to cases x
 *        (household size - 1).
 * esim_household_outbreaks and esim_household_final_sizes are refused as esim_exposure_settings is (ESIM_ESTATE before an upload,
 * on a sharded context, on a history mixed twice), esim_household_sar as esim_transmission_tree is (also after a rollback under
 * another bus_capacity).  The audits of those calls run too: ESIM_ESIM after delivering everything else; with all outputs NULL
 * the first two still run theirs.  All three leave the simulation state, the records, the exposure log, the snapshot, the
 * ensemble accumulators and the labels as they are.  Temporary device memory, freed when the call returns: that of
 * esim_exposure_settings, 12 B per building and 32 KB for the two tables (the first two); that of esim_transmission_tree and
 * 16 B per cell (esim_household_sar).  The work is one pass over the residents, or one walk over its household per case. */
#define ESIM_HH_BINS 64
int  esim_household_outbreaks(esim_ctx *ctx, uint32_t *cases, uint32_t *introductions, uint32_t *first_step /* [n_buildings] each, any may be NULL */);
int  esim_household_final_sizes(esim_ctx *ctx, uint32_t *final_size /* [ESIM_HH_BINS * ESIM_HH_BINS] or NULL */, uint32_t *introductions /* same shape, or NULL */);
int  esim_household_sar(esim_ctx *ctx, int where, uint32_t first_step, uint32_t last_step,
                        uint64_t *at_risk, uint64_t *secondary /* [n_cols * n_cols] each, either may be NULL, not both */);
/* Work place and school outbreaks: a work place and a school room have a fixed member list too -- the lists the draws themselves
 * use -- and they are the two settings the interventions act on.  The same outputs as for the household, per place: how many
 * places had an outbreak, how large against their size, how many of their cases were brought in from outside, and which share
 * of the members still Susceptible a case infected there.  Case, cohort step te, first infectious step f = max(te +
 * exposed_time + 1, 1), "Susceptible after step f - 1" (sus_until[m] >= f_j - 1), settings, infectors, the tie rule and the
 * seam of a rollback are those of the household block above, unchanged.
 *   kind           ESIM_PLACE_WORK    the non-school buildings with at least one worker; members: the citizens whose work place it
 *                                     is (work_building != home_building, not a School) -- the `workers` of
 *                                     esim_transmission_tree.  Arrays [n_buildings].
 *                  ESIM_PLACE_ROOM    the school rooms; members: their participants.  Arrays [n_rooms].
 *                  ESIM_PLACE_SCHOOL  the school buildings; members: the participants of all their rooms together
 *                                     (room_building).  Arrays [n_buildings].
 *                  A building or room without a member is no place: counts 0, first_step ESIM_NEVER, not in the tables.
 *   per place      members[p]: the number of members; cases[p]: the members that are cases; introductions[p]: of those, the index
 *                  cases and the cases whose setting is not the place's OWN -- ESIM_SETTING_WORKPLACE for ESIM_PLACE_WORK,
 *                  ESIM_SETTING_SCHOOL for ESIM_PLACE_ROOM and ESIM_PLACE_SCHOOL (a work-side exposure of a member can only have
 *                  happened in its own work building or room, so the setting alone decides); first_step[p]: the smallest cohort
 *                  step among its cases.
 *   bin(x)         x for x < 16, else min(31, 12 + floor(log2 x)): 16..31 -> 16, 32..63 -> 17, ...; exact where rooms and case
 *                  counts are small, logarithmic where work places are large.
 * esim_place_outbreaks: the four per place, any may be NULL.
 * esim_place_sizes: final_size[bin(members) * ESIM_PLACE_BINS + bin(cases)] counts the places, introduced[...] the same with
 *        bin(introductions) as the second index; either may be NULL.
 * esim_place_sar (ESIM_PLACE_WORK and ESIM_PLACE_ROOM only; ESIM_PLACE_SCHOOL is ESIM_EINVAL: the infector of a school exposure is
 *        somebody of the room): a pair is (case j, member m != j of j's place); m is at risk from j iff m is Susceptible after
 *        step f_j - 1; m is a secondary case of j iff, in addition, infector[m] == j and setting[m] is the place's own.  Counted
 *        over the cases with cohort step in [first_step, last_step] and f_j <= the steps run; first_step 0 is allowed;
 *        completeness of a cohort as for esim_household_sar.  secondary <= at_risk cell for cell, by construction.
 *          where = ESIM_BY_ALL       one cell
 *          where = ESIM_BY_GROUP     n_groups x n_groups, index g_case * n_groups + g_contact (ESIM_ESTATE without labels)
 *        The counters are 64 bits wide, on the device too.  Either output may be NULL, not both.
 * Errors follow the household calls.  ESIM_EINVAL: a null context, an unknown `kind` or `where`, both outputs of esim_place_sar
 * NULL.  ESIM_ESTATE: before an upload, on a context with more than one rank or a shard, on a history mixed twice, by group
 * without labels; esim_place_sar also after a rollback under another bus_capacity, as the tree calls are -- the first two calls
 * need only the settings and return ESIM_OK then.  ESIM_ERANGE: as esim_household_sar.  The audits run: ESIM_ESIM after delivering
 * everything else; with all outputs NULL the first two calls still run theirs.  A sticky device error comes back as the calls
 * underneath report it.  All three leave the simulation state, the records, the exposure log, the snapshot, the ensemble
 * accumulators and the labels as they are.  Temporary device memory, freed when the call returns: that of
 * esim_exposure_settings (esim_place_sar: of esim_transmission_tree), 16 B per building or room of the kind (ESIM_PLACE_SCHOOL:
 * per room and per building), 8 KB for the two tables, 16 B per cell.  The work is one pass over the member list; for
 * esim_place_sar the members of a place are staged once on the chip and its cases run against them there, PER GATHERING,
 * instead of one walk over the list per case. */
enum { ESIM_PLACE_WORK = 0, ESIM_PLACE_ROOM = 1, ESIM_PLACE_SCHOOL = 2 };
#define ESIM_PLACE_BINS 32
int  esim_place_outbreaks(esim_ctx *ctx, int kind, uint32_t *members, uint32_t *cases, uint32_t *introductions, uint32_t *first_step);
        /* [n_buildings] or [n_rooms] each, any may be NULL */
int  esim_place_sizes(esim_ctx *ctx, int kind, uint32_t *final_size, uint32_t *introduced);
        /* [ESIM_PLACE_BINS * ESIM_PLACE_BINS] each, either may be NULL */
int  esim_place_sar(esim_ctx *ctx, int kind, int where, uint32_t first_step, uint32_t last_step,
                    uint64_t *at_risk, uint64_t *secondary);   /* [n_cols * n_cols] each, not both NULL */
/* Contact-hours at risk: the denominator of the transmissions above, for every setting and not only the household -- how many
 * times a Susceptible citizen took a gathering's draw while a given Infected citizen was a candidate of it.  Derived after the
 * fact like the tree and on top of it; a run that never asks pays nothing.  This is a stated contract, as the tie rule and the
 * infector pick are.
 *   contact-hour   a triple (j, m, ts), j != m: in step ts citizen j is a CANDIDATE of a gathering exactly as
 *                  esim_transmission_tree defines candidates, and citizen m TAKES that gathering's draw.
 *   j Infected     the exposure step te comes from the log; the Infected steps are te + exposed_time + 1 .. + infected_time, for
 *                  an index case steps 1 .. infected_time; j is still Infected in the step at whose end it was vaccinated.
 *   m takes a draw m is Susceptible after step ts - 1: ts <= the smaller of its exposure step and the step at whose end it was set
 *                  Vaccinated (an index case: never), and
 *     household         j is a resident of m's household and at home: not (bus bit and uses transport), not (work bit and has a
 *                       work place); m is not (work bit, has a work place, and the work place is in another area);
 *     work place        j is a worker of m's non-school work building, the work bit is set, j is not (bus bit and uses transport);
 *                       m has a work place, and (its work place is in its home area, or the work bit is set);
 *     school            the same over the participants of m's own ROOM (a room draw uses the threshold of the Infected count of
 *                       the whole school and is taken once per Infected of the room: per contact-hour the school transmits far
 *                       more often than exposure_chance -- the reference's behaviour, which this output makes visible);
 *     public transport  the bus bit is set, j is a rider of m's route on m's bus of that step (rank by (key, position) /
 *                       bus_capacity, keys as for the tree; a route of at most bus_capacity riders is one bus); m is a rider and
 *                       was not exposed in a building in step ts itself -- buildings are drawn before buses.
 *                  A citizen exposed at home in ts still counts for its work-side draw of ts: both draws are taken, the tie rule
 *                  decides only the credit.  After a rollback under another seed the bus keys up to the seam use the snapshot's seed.
 * esim_contact_hours: hours[s * n_cols^2 + col(j) * n_cols + col(m)] = the contact-hours of setting s with ts in [first_step,
 *        last_step]; transmissions[...] = the transmissions of the tree with setting s, infector j, infectee m and the infectee's
 *        step in the same window: the mixing matrix split by setting.  Every transmission is one of the contact-hours:
 *        transmissions <= hours cell for cell.  per_case[j] = the contact-hours with j as the Infected side, summed over the
 *        settings of the mask and the window; beside esim_offspring it separates "had many contacts" from "was lucky".
 *          where = ESIM_BY_ALL       one column
 *          where = ESIM_BY_GROUP     n_groups columns (ESIM_ESTATE without labels)
 *        Any other `where`, an empty mask or a bit beyond ESIM_SETTING_TRANSPORT is ESIM_EINVAL; the planes of settings outside
 *        the mask stay 0.  ESIM_ERANGE for steps outside 1 .. the steps run so far or last_step < first_step, and, before any
 *        launch, where per_case is asked for and (infected_time + 1) x 3 x (the longest member list) does not fit its 32 bits.
 *        Any output may be NULL; with all three NULL the audits of the tree still run.  Refused as esim_transmission_tree is
 *        (ESIM_ESTATE before an upload, on a sharded context, on a history mixed twice, after a rollback under another
 *        bus_capacity); ESIM_ESIM from the audits after delivering everything else.  The call leaves the simulation state, the
 *        records, the exposure log, the snapshot, the ensemble accumulators and the labels as they are and keeps nothing between
 *        calls.  Temporary device memory, freed when the call returns: that of esim_transmission_tree, 64 B per cell, 16 B per
 *        step run, 4 B per citizen with per_case and, with routes longer than a bus in the mask, 4 B per bus step of the window,
 *        a bit per (route, bus step) up to 64 MB at a time and 8 B per rider of the longest route for each of up to 2048
 *        workgroups.  No kernel walks the steps of a pair: buildings, rooms and one-bus routes cost a difference of prefix counts
 *        per pair; longer routes one ranking of the route per (route, bus step) that has an Infected rider. */
int  esim_contact_hours(esim_ctx *ctx, int where, uint32_t setting_mask, uint32_t first_step, uint32_t last_step,
                        uint64_t *hours /* [4 * n_cols * n_cols] or NULL */, uint64_t *transmissions /* same, or NULL */,
                        uint32_t *per_case /* [n_citizens] or NULL */);
/* How the epidemic travels: which Output Area seeds which, how many of an area's cases were imported, and through which area and
 * setting the epidemic first entered every area -- computed on the device from the tree, the lineage and the home area of every
 * citizen, so that nothing of size [n_citizens] goes to the host.  (A dense [n_areas][n_areas] table would be 340 GB at the
 * 290 000 areas of uk64m: the two sparse outputs are aggregated in a hash table, compacted and sorted on the device.)
 *   area           of a citizen: the Output Area of its household, building_area[home_building].
 *   transmission   an entry (c, ts) of the exposure log with ts >= 1 and infector[c] != ESIM_NO_INFECTOR; its step is ts, the
 *                  infectee's.  Setting, infector, the tie rule and the seam of a rollback are those of esim_exposure_settings
 *                  and esim_transmission_tree.  An exposure without a candidate is no transmission and is not counted.
 *   case           a citizen in the exposure log, the index cases included; its cohort step is its exposure step, 0 for an index
 *                  case -- the convention of esim_reproduction_series, esim_outbreaks and esim_household_outbreaks.
 * esim_area_flows: the distinct pairs (area of the infector, area of the infectee) over the transmissions of steps [first_step,
 *        last_step] whose setting is in setting_mask, ascending by (src, dst), every pair once; count[i] is the number of such
 *        transmissions of pair i.  src, dst, count: [cap] each, any may be NULL.  *n_out receives the number of distinct pairs;
 *        ESIM_ERANGE, with *n_out set, when cap is smaller (the rule of esim_outbreaks; nothing is delivered then, and a call
 *        with cap 0 is the way to ask for the size); ESIM_EINVAL for a null n_out.  The mask is checked as esim_mixing_matrix
 *        checks it, the steps as esim_offspring checks them.  12 B per distinct pair go to the host and nothing per citizen.
 * esim_area_imports: over the same transmissions, local[a] those with both ends in a, imported[a] those with the infectee in a
 *        and the infector elsewhere, exported[a] those with the infector in a and the infectee elsewhere.  [n_areas] each, any
 *        may be NULL; with all three NULL the audits still run.  Mask and steps as above.  The diagonal of the flows is local,
 *        the rest of row a sums to exported[a], the rest of column a to imported[a].
 * esim_area_invasion: the between-area invasion tree.  first_case[a] is the case living in a with the smallest cohort step, of
 *        several in that step the one with the smallest local citizen index (a stated contract, as the tie rule of the settings
 *        is), ESIM_NO_INFECTOR for an area without a case; step[a] its cohort step, ESIM_NEVER without a case -- what
 *        esim_area_arrival(ESIM_AREA_HOME) returns; source_area[a] the area of its infector, ESIM_NO_AREA for an index case, for
 *        an area without a case and for an exposure without a candidate; setting[a] the setting of that transmission,
 *        ESIM_SETTING_NONE likewise.  [n_areas] each, any may be NULL.  An infector was exposed at least exposed_time + 1 steps
 *        before its infectee, and it is a case of its own area: step[source_area[a]] < step[a] wherever a source exists, no area
 *        is its own source, and the result is a forest rooted at the areas an index case lives in.
 * esim_lineage_areas: the distinct pairs (lineage ordinal, area) over all cases that have a lineage (esim_transmission_chains),
 *        the index cases included, ascending; count[i] is the number of cases of that lineage living in that area.  cap and
 *        n_out as for esim_area_flows.  The areas an introduction reached are the run lengths of `lineage`.
 * The first three are refused as esim_transmission_tree is, esim_lineage_areas as esim_transmission_chains is: ESIM_ESTATE before
 * an upload, on a sharded context, on a history mixed twice and after a rollback under another bus_capacity.  The audits of
 * those calls run too: ESIM_ESIM after delivering everything else.  All four leave the simulation state, the records, the
 * exposure log, the snapshot, the ensemble accumulators and the labels as they are.
 * Temporary device memory, freed when the call returns: that of esim_transmission_tree (esim_lineage_areas: of
 * esim_transmission_chains); 12 B per area (imports), 21 B per area (invasion); for the two sparse outputs a table of 12 B per
 * slot -- the smallest power of two >= twice the entries of the exposure log, at least 64, so that it is never more than half
 * full -- and a dense array of 12 B per entry of the log, rounded up to a power of two.  ESIM_PAIR_LOG2 in the environment (read
 * when a population is uploaded) forces 1 << value slots instead; a table that cannot hold every distinct pair then makes the
 * call ESIM_ENOMEM, with the knob and the number of keys dropped in esim_last_error.  The host reads the number of distinct
 * pairs once in the middle of these two calls, to size the launches of the sort.
 * esim_pair_stats: what the pair engine did in the last esim_area_flows or esim_lineage_areas of this context -- ms[0..2] the
 *        device time of insert (the emptying of the table included), compact and sort (the read of the count included), from
 *        HIP events; counts[0..2] the distinct pairs, the slots of the table and the keys dropped.  Either may be NULL. */
#define ESIM_NO_AREA 0xFFFFFFFFu
int  esim_area_flows(esim_ctx *ctx, uint32_t setting_mask, uint32_t first_step, uint32_t last_step,
                     uint32_t *src, uint32_t *dst, uint32_t *count /* [cap] each, any may be NULL */, uint32_t cap, uint32_t *n_out);
int  esim_area_imports(esim_ctx *ctx, uint32_t setting_mask, uint32_t first_step, uint32_t last_step,
                       uint32_t *local, uint32_t *imported, uint32_t *exported /* [n_areas] each, any may be NULL */);
int  esim_area_invasion(esim_ctx *ctx, uint32_t *first_case, uint32_t *step, uint32_t *source_area /* [n_areas] each, any may be NULL */,
                        uint8_t *setting /* [n_areas] or NULL */);
int  esim_lineage_areas(esim_ctx *ctx, uint32_t *lineage, uint32_t *area, uint32_t *count /* [cap] each, any may be NULL */,
                        uint32_t cap, uint32_t *n_out);
int  esim_pair_stats(esim_ctx *ctx, double *ms /* [3] or NULL */, uint32_t *counts /* [3] or NULL */);
/* Superspreading events: which gatherings drove the epidemic.  The exposure rule is per gathering -- 1 - (1 - p)^n over the n
 * Infected standing in one place in one step --, so the unit is the (place, step) event.
 *   transmission   as for esim_area_flows: a log entry (c, ts) with ts >= 1, a setting in the mask and an infector.
 *   gathering      the member list esim_transmission_tree walks for the candidates of c: the home building (household), the work
 *                  building (work place), c's own room (school; the index of esim_population.room), c's bus (public transport):
 *                  (route, bus number).  A route is named by its ordinal among the distinct (home area, work area) pairs that
 *                  have a rider, ascending by home area, then work area (esim_routes); the bus number is the rider's rank in
 *                  that step's order of the route / bus_capacity, and 0 on a route of at most bus_capacity riders.
 *   event          the transmissions of one step in one gathering; its size is their number.  An entry whose place cannot be
 *                  formed (an index outside the tables) is not counted.
 * esim_transmission_events: over the transmissions of steps [first_step, last_step] whose setting is in setting_mask,
 *        sizes[s * ESIM_EVENT_BINS + min(size, ESIM_EVENT_BINS - 1)] counts ALL events of setting s, whatever min_size is (bin 0
 *        stays 0; the sum over b of b * sizes[s][b] is the number of transmissions of s unless the last bin is occupied), and
 *        *n_out receives the number of events with size >= min_size (>= 1; 0 is ESIM_EINVAL).  They are listed in step[],
 *        setting[], place[] (building, room or route ordinal), bus[] (0 off public transport) and size[], [cap] each, any may be
 *        NULL:
 *          ESIM_EVENTS_BY_KEY   ascending by (step, setting, place, bus); ESIM_ERANGE, with *n_out set and no list delivered,
 *                               when cap is smaller than *n_out (the rule of esim_area_flows; cap 0 asks for the size);
 *          ESIM_EVENTS_BY_SIZE  descending by size, ties ascending by that key; the first min(cap, *n_out) are delivered and a
 *                               smaller cap is no error: the top-K list.
 *        With every list pointer NULL nothing is sorted; with sizes NULL too the audits still run.  ESIM_EINVAL for a null n_out
 *        or an unknown order; mask and steps are checked as esim_area_flows checks them, ESIM_ERANGE after more than 2^30 steps.
 *        Refusals and audits are those of esim_transmission_tree (ESIM_ESIM after delivering everything else).  The simulation
 *        state, the records, the exposure log, the snapshot, the ensemble accumulators and the labels stay as they are, and
 *        nothing is kept between calls.  Temporary device memory: that of esim_transmission_tree and 4 B per citizen for the
 *        buses, the pair table and dense array of esim_area_flows (ESIM_PAIR_LOG2 holds here too), 4 KB for the size table,
 *        17 B per event delivered and, by size, 12 B per event of the list.  esim_pair_stats reports this call too: the sort
 *        time includes the second sort and the split into arrays.
 * esim_routes: the route table, 12 B per route and nothing per citizen: home_area[r], work_area[r], n_riders[r], [cap] each, any
 *        may be NULL.  *n_out receives the number of routes; ESIM_ERANGE, with *n_out set, when cap is smaller (the rule of
 *        esim_get_seeds); ESIM_EINVAL for a null n_out, ESIM_ESTATE before an upload. */
#define ESIM_EVENT_BINS 256
enum { ESIM_EVENTS_BY_KEY = 0, ESIM_EVENTS_BY_SIZE = 1 };
int  esim_transmission_events(esim_ctx *ctx, uint32_t setting_mask, uint32_t first_step, uint32_t last_step, uint32_t min_size, int order,
                              uint32_t *step, uint8_t *setting, uint32_t *place, uint32_t *bus, uint32_t *size /* [cap] each, any may be NULL */,
                              uint32_t cap, uint32_t *n_out, uint32_t *sizes /* [ESIM_N_SETTINGS * ESIM_EVENT_BINS] or NULL */);
int  esim_routes(esim_ctx *ctx, uint32_t *home_area, uint32_t *work_area, uint32_t *n_riders /* [cap] each, any may be NULL */, uint32_t cap, uint32_t *n_out);
/* Checkpoint / resume (the reference has none for the simulation state): everything a step reads that is
 * not part of the uploaded population -- the citizen words, the census histogram, the exposure log, the control block,
 * the records so far.  Restore goes into a context that holds the SAME population (or shard) and parameters; the run
 * continues bit for bit as if it had not been interrupted. */
int  esim_checkpoint_size(esim_ctx *ctx, size_t *bytes);
int  esim_checkpoint_save(esim_ctx *ctx, void *buf, size_t cap);
int  esim_checkpoint_restore(esim_ctx *ctx, const void *buf, size_t bytes);
/* Forecast ensembles: given the epidemic as it stands at step T, what happens next under other policies or other random
 * futures.  esim_snapshot keeps, ON THE DEVICE, the state at rest after the last completed step together with the parameters in
 * force: what a checkpoint holds (the control block, the census histogram, the log offsets, the citizen words, the exposure log,
 * the per-step exposure counts and the records so far).  One snapshot per context, a later call replaces it.  Memory: 4 B per
 * citizen, the prefixes of the log, the exposure counts and the records, and the small tables; allocated at the first call and
 * kept.  Nothing proportional to the population moves to the host and nothing waits for the stream (the control block is taken
 * from the host's pinned mirror, where esim_run and esim_step leave it; after any other way to this step it is read once, 200
 * bytes).  The snapshot is self-contained: it survives esim_reset, esim_restart and further running; esim_upload_population,
 * esim_restart_seeded (the seeds in force belong to the state) and esim_snapshot_drop drop it.
 * ESIM_ESTATE: before an upload; at step 0 (that state is esim_restart's to rebuild); with a sticky device-side error pending;
 * on a context whose communicator has more than one rank (the rule of esim_restart); on a branch with a seam (below).
 * ESIM_ENOMEM: no device memory (the context and an earlier snapshot are then as they were).
 * esim_rollback goes back to the snapshot's step with *p in force from the next step on; p == NULL: the snapshot's own
 * parameters.  May differ from the snapshot's: seed, exposure_chance, mask_effectiveness, the four thresholds, vaccination_rate,
 * bus_capacity.  Must equal the snapshot's, else ESIM_EINVAL: exposed_time, infected_time, start_hour, end_hour (the state and
 * everything derived from the history afterwards is a function of them) and device.  max_steps follows the rule of
 * esim_restart and may not lie below the snapshot's step (ESIM_ERANGE).  *p is validated as esim_create validates it (its
 * exposure_chance must be a probability, ESIM_EINVAL); a refused
 * call leaves the context and the snapshot as they were; ESIM_ESTATE without a snapshot.  Host->device traffic: the control
 * block and the threshold LUT (4.4 KB, from pinned memory); everything else is restored on the device, and nothing waits.  The
 * records and log entries of the steps up to the snapshot's stay readable, those behind it are the branch's.
 * The seam: the vaccination choice of a step is drawn from the seed and vaccination_rate in force, and the series calls walk it
 * again after the fact.  After a rollback that changed either, the steps up to and including the snapshot's were drawn under the
 * old values and the later ones under the new: the context keeps that one seam (step, old seed, old rate) until esim_reset,
 * esim_restart, an upload or a rollback to the snapshot's own seed and rate, and the series calls honour it.  One seam is all
 * there is: every branch leaves from the one snapshot, esim_snapshot on a branch with a seam is ESIM_ESTATE (a history mixed
 * twice is not built), and so are esim_checkpoint_size and esim_checkpoint_save while the seam is in force (their header names
 * one parameter set).
 * esim_snapshot_info: the snapshot's step (0: none) and parameters; either pointer may be NULL.  Pure host code.
 * esim_snapshot_drop: frees the snapshot's device memory (esim_destroy and a new upload free it too). */
int  esim_snapshot(esim_ctx *ctx);
int  esim_rollback(esim_ctx *ctx, const esim_params *p);
int  esim_snapshot_info(esim_ctx *ctx, uint32_t *step, esim_params *p);
int  esim_snapshot_drop(esim_ctx *ctx);
/* Paired policy comparison: cases averted against a kept baseline run.  Every draw is a pure function of (seed, global citizen,
 * step, slot), so two runs of one population under the same seed and index cases share their random numbers by construction:
 * a citizen exposed in one run and not in the other is an effect of what differs between them, not noise.  No step kernel is
 * involved: a run that never asks pays nothing, and every output is an exact integer.
 * esim_baseline_keep turns the exposure log as it stands into one uint32 per citizen ON THE DEVICE: its exposure step, 0 for an
 *        index case, ESIM_NEVER for a citizen the log does not hold.  The step comes from the entry's position in the log (the
 *        citizen word loses it once the citizen is vaccinated).  Kept with it: the steps run, the parameters in force and the
 *        number of log entries.  4 B per citizen, allocated at the first keep and reused; one baseline per context, a later keep
 *        replaces it.  Everything runs on the context's stream behind one read of the control block; nothing proportional to the
 *        population goes to the host.  The baseline is kept through esim_reset, esim_restart, esim_restart_seeded, esim_snapshot,
 *        esim_rollback and esim_checkpoint_restore, and dropped by a new upload, esim_baseline_drop and esim_destroy.  It is no
 *        simulation state: no checkpoint holds it.  ESIM_ESTATE before an upload and on a context whose communicator has more
 *        than one rank or that holds a shard (the rule of esim_restart); ESIM_ENOMEM without device memory; a sticky device-side
 *        error is reported as the series calls report it.
 * esim_baseline_info: the steps, the log entries and the parameters of the baseline kept; any pointer may be NULL.  Pure host code.
 * esim_baseline_drop: forgets it (the plane stays for the next keep).  Both are ESIM_ESTATE without a baseline.
 * esim_compare: the run as it stands against the baseline.  A citizen is a CASE of a run in the window when its exposure step s
 *        satisfies first_step <= s <= last_step; first_step 0 takes the index cases in, as esim_reproduction_series does.  With b
 *        the baseline's step and c the current run's, counts[col * ESIM_CMP_N + class]:
 *          ESIM_CMP_BOTH     a case in both runs           ESIM_CMP_EARLIER  of BOTH, c < b
 *          ESIM_CMP_AVERTED  a case in the baseline only   ESIM_CMP_LATER    of BOTH, c > b
 *          ESIM_CMP_ADDED    a case in the current run only
 *        delay[col] is the sum of c - b over BOTH, signed.  where = ESIM_BY_ALL (one column), ESIM_AREA_HOME (n_areas columns, by
 *        the Output Area of the household) or ESIM_BY_GROUP (n_groups columns, ESIM_ESTATE without labels); any other `where` is
 *        ESIM_EINVAL.  *first_divergence is the smallest step at which the two histories differ: the minimum, over the citizens
 *        with b != c, of the smaller of the two steps, ESIM_NEVER counting as infinite; ESIM_NEVER for identical histories.  It is
 *        not restricted to the window.  cls[citizen] is 0 for neither, 1 BOTH, 2 AVERTED, 3 ADDED.  Any output may be NULL; with
 *        all of them NULL the call still runs and returns its status.  ESIM_ERANGE when last_step < first_step or last_step lies
 *        beyond the steps of either run; ESIM_ESTATE without a baseline; the other errors are those of esim_baseline_keep.  A
 *        refused call leaves the outputs untouched.
 * esim_compare_series: the event rows of both runs from the two planes, baseline[i * n_cols + col] and current[...]: row i holds
 *        the cases of steps [first_step + i * stride, + stride), the index cases at step 0; with cumulative != 0 it holds the
 *        steps [first_step, first_step + (i + 1) * stride), a prefix over the rows summed on the device.  `where` as above.
 *        Either output may be NULL.  ESIM_EINVAL for stride 0 or no rows; ESIM_ERANGE when the last row's first step lies beyond
 *        the steps of either run (rows are clipped to the steps run, as the incidence rows of esim_area_status_series are; unlike
 *        them first_step 0 is allowed).  Averted by row is baseline - current, left to the caller: no signed plane exists.
 * Both calls leave the simulation state, the records, the exposure log, the snapshot, the labels, the ensemble accumulators and
 * the baseline as they are.  Temporary device memory, freed when the call returns: 4 B per citizen for the current run's plane
 * (1 B more with cls), and the tables (28 B per column) or the rows (8 B per cell).
 * Paired ensemble accumulators: one more kind of the accumulators over rows, beside series, settings and reproduction; one kind
 * is in force at a time.  A member contributes the two row planes of esim_compare_series(where, first_step, n_rows, stride,
 * cumulative), b = baseline[cell] and c = current[cell].  esim_ensemble_fold with this kind in force adds members += 1 once and
 * per cell
 *          if b >= min_baseline:  defined += 1, and hit += 1 iff b - c >= min_averted as signed (min_averted >= 1)
 *          always:                sum_baseline += b; sum_current += c; sumsq_baseline += b * b; sumsq_current += c * c;
 *                                 sum_cross += b * c
 *        in integers, 48 B per cell beside two row planes of 4 B per cell: the mean averted is (sum_baseline - sum_current) /
 *        members, and the variance of the PAIRED difference, (sumsq_baseline - 2 sum_cross + sumsq_current) / members - mean^2,
 *        follows from unsigned sums alone.  hit / defined is P(at least min_averted cases averted).  The fold is ESIM_ESTATE
 *        without a baseline and ESIM_ERANGE when the last row lies beyond either run, with nothing folded; it waits for the
 *        stream.  The accumulators do not own the baseline: every member keeps its own before its policy run.  ESIM_EINVAL for a
 *        null context, an unknown `where`, stride 0, no rows, min_averted 0.  Lifetime, shape changes, ESIM_ENOMEM and the other
 *        ESIM_ESTATE cases are those of esim_ensemble_begin_reproduction.
 * esim_ensemble_read_paired: rows [first_row, first_row + n) of these accumulators, addressed as esim_ensemble_read_reproduction
 *        addresses its own; ESIM_ESTATE while another kind is in force -- and the other reads are ESIM_ESTATE while this one is. */
enum { ESIM_CMP_BOTH = 0, ESIM_CMP_AVERTED, ESIM_CMP_ADDED, ESIM_CMP_EARLIER, ESIM_CMP_LATER, ESIM_CMP_N };
int  esim_baseline_keep(esim_ctx *ctx);
int  esim_baseline_info(esim_ctx *ctx, uint32_t *steps, uint32_t *n_cases, esim_params *p);
int  esim_baseline_drop(esim_ctx *ctx);
int  esim_compare(esim_ctx *ctx, int where, uint32_t first_step, uint32_t last_step,
                  uint64_t *counts /* [n_cols * ESIM_CMP_N] or NULL */, int64_t *delay /* [n_cols] or NULL */,
                  uint32_t *first_divergence /* or NULL */, uint8_t *cls /* [n_citizens] or NULL */);
int  esim_compare_series(esim_ctx *ctx, int where, uint32_t first_step, uint32_t n_rows, uint32_t stride, int cumulative,
                         uint32_t *baseline /* [n_rows * n_cols] or NULL */, uint32_t *current /* same, or NULL */);
int  esim_ensemble_begin_paired(esim_ctx *ctx, int where, uint32_t first_step, uint32_t n_rows, uint32_t stride, int cumulative,
                                uint32_t min_baseline, uint32_t min_averted);
int  esim_ensemble_read_paired(esim_ctx *ctx, uint32_t first_row, uint32_t n, uint32_t *members, uint32_t *defined /* [n * n_cols] */,
                               uint32_t *hit /* [n * n_cols] */, uint64_t *sum_baseline, uint64_t *sum_current, uint64_t *sumsq_baseline,
                               uint64_t *sumsq_current, uint64_t *sum_cross /* [n * n_cols] each */);

/* The shape of the epidemic curve per column.  x_s[col] is the number of citizens of column `col` whose status after
 * step s is in status_mask -- the state after that step's vaccinations, the convention of every area and group table.  Three masks
 * are allowed: 1 << ESIM_EXPOSED, 1 << ESIM_INFECTED, and both together ("active"): together the two statuses are one interval
 * per case.  Every other mask is ESIM_EINVAL (the other statuses are monotone: the census and the arrival map describe them).
 *          where = ESIM_BY_ALL       one column
 *          where = ESIM_AREA_HOME    n_areas columns, by the Output Area of the household
 *          where = ESIM_BY_GROUP     n_groups columns, by the labels of esim_set_groups (ESIM_ESTATE without labels)
 *        ESIM_AREA_CURRENT and anything else is ESIM_EINVAL.  Cell for cell x_s is the row of step s of
 *        esim_area_status_series(ESIM_AREA_HOME, what) or esim_group_series(what) at stride 1, for the mask of both the sum of the
 *        two rows; the index cases are Infected after steps 0 .. infected_time.
 * esim_curve_summary: over the steps s in [first_step, last_step],
 *          peak[col]            max x_s
 *          peak_step[col]       the smallest s that attains it; ESIM_NEVER where the peak is 0
 *          steps_at_least[col]  the number of steps with x_s >= threshold
 *          first_at_least[col], last_at_least[col]   the smallest and the largest such s; ESIM_NEVER without one
 *          person_steps[col]    the sum of x_s
 *        Any output may be NULL; with all of them NULL the call still runs and returns its status.  ESIM_EINVAL also for threshold
 *        0; ESIM_ESTATE before an upload and on a context with more than one rank or that holds a shard; ESIM_ERANGE for
 *        first_step 0, last_step < first_step, or last_step beyond the steps run; ESIM_ENOMEM without device memory (or with a
 *        pair table, ESIM_PAIR_LOG2, too small for the change points); a sticky device-side error is reported as the series calls
 *        report it.  A refused call leaves the outputs untouched.  The call leaves the simulation state, the records, the exposure
 *        log, the snapshot, the baseline, the labels and the ensemble accumulators as they are and keeps nothing between calls;
 *        after an esim_rollback under another seed or vaccination rate the vaccinations are replayed across the seam, as the
 *        series calls replay them.  Nothing proportional to steps x columns is built: every case adds +1 at the first step of its
 *        interval and -1 behind the last one to a sparse table keyed by (column, step), the distinct keys are sorted, a segmented
 *        scan turns the changes into counts and a reduction per column takes the summary.  Temporary device memory, freed when the
 *        call returns: 4 B per citizen for the vaccination replay once a programme has run; the pair table (12 B per slot, the
 *        smallest power of two >= 4 x the log's entries) and the dense array (12 B per pair, 2 x the log's entries rounded up to a
 *        power of two); 28 B per column for the tables and 12 B per 2048 pairs for the scan.  esim_pair_stats reports this call.
 * Peaks ensemble accumulators: one more kind of the accumulators over rows, beside series, settings, reproduction and paired; one
 * kind is in force at a time.  esim_ensemble_fold with this kind in force computes the member's esim_curve_summary(where,
 * status_mask, first_step, last_step, threshold) on the device, adds members += 1 once and per column
 *          defined += (peak >= 1);  hit += (peak >= min_peak)
 *          sum_peak += peak; sumsq_peak += peak^2; sum_duration += steps_at_least; sumsq_duration += steps_at_least^2   (every member)
 *          sum_step += peak_step; sumsq_step += peak_step^2                                                           (defined members)
 *        in integers, 56 B per column; nothing per column goes to the host.  The fold is ESIM_ERANGE, with nothing folded, when
 *        last_step lies beyond the member's steps; it waits for the stream.  ESIM_EINVAL and ESIM_ERANGE as esim_curve_summary, and
 *        ESIM_EINVAL for min_peak 0.  Lifetime, replacement of the kind in force, ESIM_ENOMEM, the ESIM_ESTATE cases and the
 *        invalidation by esim_set_groups are those of esim_ensemble_begin_reproduction.
 * esim_ensemble_read_peaks: the accumulators, [n_cols] each, any pointer NULL; ESIM_ESTATE while another kind is in force -- and
 *        the other reads are ESIM_ESTATE while this one is. */
int  esim_curve_summary(esim_ctx *ctx, int where, uint32_t status_mask, uint32_t first_step, uint32_t last_step, uint32_t threshold,
                        uint32_t *peak, uint32_t *peak_step, uint32_t *steps_at_least, uint32_t *first_at_least, uint32_t *last_at_least,
                        uint64_t *person_steps /* [n_cols] each, any may be NULL */);
int  esim_ensemble_begin_peaks(esim_ctx *ctx, int where, uint32_t status_mask, uint32_t first_step, uint32_t last_step,
                               uint32_t threshold, uint32_t min_peak);
int  esim_ensemble_read_peaks(esim_ctx *ctx, uint32_t *members, uint32_t *defined, uint32_t *hit, uint64_t *sum_peak, uint64_t *sumsq_peak,
                              uint64_t *sum_step, uint64_t *sumsq_step, uint64_t *sum_duration, uint64_t *sumsq_duration);

/* Ensemble quantile maps: the members of an ensemble kept on the device, one value x per cell and member, and order
 * statistics and exceedance counts per cell taken there -- for the distributions whose mean and variance mislead (an area
 * reached in 3 members of 32), and for thresholds chosen after the folds.
 * keep:  esim_ensemble_keep_members comes after a begin of any kind but the reproduction kind and before that begin's first fold.
 *        It allocates capacity * n_rows * n_cols * 4 B (n_rows = 1 for the kinds without rows); from then on every fold that
 *        raises the member counter also writes the member's x into the next slot, one more launch or device-to-device copy on
 *        the context's stream and no wait.  x per kind: the census kind, the count the fold adds to sum; arrival, the arrival
 *        step, ESIM_NEVER where the entry was not reached by the horizon; series and settings, the cell of the member's rows;
 *        paired, baseline - current as a signed number (is_signed = 1); peaks, by `what`: the peak (ESIM_KEEP_VALUE), its step
 *        (ESIM_KEEP_PEAK_STEP, ESIM_NEVER without a peak) or steps_at_least (ESIM_KEEP_DURATION).  Every other kind takes
 *        ESIM_KEEP_VALUE only.  ESIM_EINVAL: capacity 0 or above ESIM_MEMBERS_MAX, an unknown `what`, or one the kind does not
 *        have; ESIM_ESTATE: no population, no valid begin in force, the reproduction kind, or a member folded since the begin;
 *        ESIM_ENOMEM: the store does not fit.  A refusal leaves the accumulators and an earlier store as they were.  With the
 *        store full, the fold is ESIM_ERANGE with nothing folded and nothing enqueued.  A fold that returns an error with
 *        nothing folded keeps nothing; one that returns an audit's ESIM_ESIM with the member folded keeps the member.
 * info:  capacity, members kept, `what` and whether x is signed, any pointer NULL; ESIM_ESTATE without a store.
 * read:  out[(m * n_rows + r) * n_cols + col] = x of member first_member + m (in the order of the folds) in row first_row + r;
 *        signed kinds as int32 bit patterns.
 * quantiles:  out[(q * n_rows + r) * n_cols + col] = the ranks[q]-th smallest (0-based) x of the cell over the members kept;
 *        the order is signed for the paired kind and unsigned otherwise, so that ESIM_NEVER sorts last: a quantile of
 *        ESIM_NEVER says that the entry was not reached in at least that share of the members.  Ranks need be neither sorted
 *        nor distinct.
 * exceedance:  out[(t * n_rows + r) * n_cols + col] = the members kept with x >= thresholds[t], compared as signed numbers for
 *        the paired kind and as unsigned ones otherwise; for the kinds in which ESIM_NEVER occurs (arrival, the step of the
 *        peak) a member at ESIM_NEVER is >= every threshold.
 *        The three are ESIM_ESTATE without a store or with nothing kept; ESIM_ERANGE for rows or members outside the store or a
 *        rank >= the members kept; ESIM_EINVAL for a null output, no ranks or thresholds, or more than ESIM_RANKS_MAX.  They
 *        wait for the stream and leave everything as it is.
 * The store lives as long as the accumulators beside it: kept through esim_reset, esim_restart, esim_restart_seeded,
 * esim_snapshot and esim_rollback; ended by a begin of any kind, a new upload, esim_destroy, and esim_set_groups when begun by
 * group; not part of a checkpoint. */
#define ESIM_MEMBERS_MAX 256
#define ESIM_RANKS_MAX   16
enum { ESIM_KEEP_VALUE = 0, ESIM_KEEP_PEAK_STEP = 1, ESIM_KEEP_DURATION = 2 };
int  esim_ensemble_keep_members(esim_ctx *ctx, uint32_t capacity, int what);
int  esim_ensemble_members_info(esim_ctx *ctx, uint32_t *capacity, uint32_t *kept, int *what, int *is_signed);
int  esim_ensemble_read_members(esim_ctx *ctx, uint32_t first_member, uint32_t n_members, uint32_t first_row, uint32_t n_rows, uint32_t *out);
int  esim_ensemble_quantiles(esim_ctx *ctx, uint32_t first_row, uint32_t n_rows, const uint32_t *ranks, uint32_t n_ranks, uint32_t *out);
int  esim_ensemble_exceedance(esim_ctx *ctx, uint32_t first_row, uint32_t n_rows, const int64_t *thresholds, uint32_t n_thresholds, uint32_t *out);

/* Curve-based ensemble statistics: the members kept by esim_ensemble_keep_members ranked as whole curves, for the
 * questions a band stitched from per-cell quantiles answers wrongly (no single member stays inside it, and its median peaks
 * lower and wider than any member does).  The store holds kept = M members, n_rows rows and n_cols columns.
 * curve:  the curve of member i in column c is its keys x[i][r][c] over the rows r of a window [first_row, first_row + n_rows).
 *        Keys order as the store orders them: unsigned, signed kinds with the top bit flipped, ESIM_NEVER largest.
 * depth:  modified band depth with bands of two curves (Lopez-Pintado and Romo 2009), stated so that ties are safe.  For a cell
 *        (r, c) and member i, below = the members whose key is < x[i], above = the members whose key is > x[i]; the pairs {j, k}
 *        of the M members (i itself included) with min(x[j], x[k]) <= x[i] <= max(x[j], x[k]) number exactly
 *        C(M, 2) - C(below, 2) - C(above, 2).  depth[i * n_cols + c] is the sum of that count over the rows of the window, an
 *        exact integer; depth / (n_rows * C(M, 2)) is the modified band depth; total[i] is the sum of depth[i][c] over c, in 64
 *        bits.  With M = 1 every depth is 0.  ESIM_ERANGE for a window whose n_rows * C(M, 2) does not fit 32 bits.
 * central region, for need in 1..M.  Per column (pooled = 0): thr[c] is the need-th largest of depth[.][c]; member i is in if
 *        depth[i][c] >= thr[c], ties at the threshold all in; n_in[c] >= need counts the members that are in; deepest[c] is the
 *        smallest member index whose depth is the maximum.  Pooled (pooled = 1): the same with total[.] in place of
 *        depth[.][c] -- one set of members and one deepest member for all columns, one coherent future for the whole map.
 * band:  lo[r * n_cols + c] and hi[r * n_cols + c] are the minimum and maximum key over the members that are in,
 *        median[r * n_cols + c] is the key of member deepest[c]; signed kinds come back as the numbers they are, as
 *        esim_ensemble_quantiles returns them, and a plane may hold ESIM_NEVER for the arrival and peak-step stores, where it
 *        means what it means there.
 *        Both calls are ESIM_ESTATE without a store or with nothing kept (a store invalidated by esim_set_groups or ended by a
 *        new begin included); ESIM_ERANGE for rows outside the store and for need 0 or above the members kept; ESIM_EINVAL for a
 *        pooled that is not 0 or 1.  Any output may be NULL, all of them too: the call still validates.  They wait for the
 *        stream and leave everything as it is; their tables on the device (4 B per member and column) go when they return. */
int  esim_ensemble_depth(esim_ctx *ctx, uint32_t first_row, uint32_t n_rows,
                         uint32_t *depth /* [kept * n_cols] or NULL */, uint64_t *total /* [kept] or NULL */);
int  esim_ensemble_band(esim_ctx *ctx, uint32_t first_row, uint32_t n_rows, uint32_t need, int pooled,
                        uint32_t *lo, uint32_t *hi, uint32_t *median /* [n_rows * n_cols] each, any may be NULL */,
                        uint32_t *deepest, uint32_t *n_in /* [n_cols] each, any may be NULL */);

/* Ensemble distances: the members kept by esim_ensemble_keep_members compared pair by pair, for ensembles with more
 * than one centre -- the medoid, k-medoids clusters with their weights, silhouettes and the nearest real run to any member all
 * follow from this M x M table on the host (M = kept <= ESIM_MEMBERS_MAX).
 * out:   out[i * M + j], for the keys x[i][r][c] of the store over the rows r of a window [first_row, first_row + n_rows) and all
 *        columns c:  ESIM_DIST_L1, the sum of |x[i] - x[j]|;  ESIM_DIST_DIFFER, the number of cells with x[i] != x[j].  Exact
 *        integers in 64 bits over the full range of the keys; symmetric, the diagonal 0, both triangles written.  A signed
 *        store (the paired kinds) gives the distances of the signed values.
 * never_as:  for the stores in which ESIM_NEVER occurs (arrival, the step of the peak) a key equal to ESIM_NEVER is replaced by
 *        never_as before it is compared -- the horizon, for instance; ESIM_NEVER leaves it as it is.  Ignored by every other store.
 * live_cells:  may be NULL; the cells of the window that the accumulators do not settle (every member holds the same key there,
 *        the planes are not read): what the kernel compared.  0 where nothing is launched (no rows, or one member).
 *        ESIM_EINVAL for an unknown metric; ESIM_ESTATE without a store or with nothing kept; ESIM_ERANGE for rows outside the
 *        store.  n_rows == 0 or kept <= 1 gives zeros.  out may be NULL: the call still validates and counts.  It waits for
 *        the stream and leaves everything as it is; its matrix on the device goes when it returns.
 * info:  what the kernel of the context's last esim_ensemble_distances did, any pointer NULL: the tiles of 64 packed live cells it
 *        compared (per pair of member tiles), those of them summed in 32-bit accumulators, and those compared partially full. */
#define ESIM_DIST_L1     0
#define ESIM_DIST_DIFFER 1
int  esim_ensemble_distances(esim_ctx *ctx, uint32_t first_row, uint32_t n_rows, int metric, uint32_t never_as,
                             uint64_t *out /* [kept * kept] or NULL */, uint64_t *live_cells /* may be NULL */);
int  esim_ensemble_distances_info(esim_ctx *ctx, uint64_t *tiles, uint64_t *tiles_32bit, uint64_t *tiles_partial);

/* Policy grids: the members kept by esim_ensemble_keep_members read as a grid of n_arms policies run over
 * S = kept / n_arms random futures on common random numbers -- the draws are a function of (seed, citizen, step, slot), so the
 * arms of one replicate share theirs.  The store is read replicate-major, arms adjacent: slot = s * n_arms + a, the order in
 * which the arms of one replicate are folded one after the other and which a merge of contiguous blocks of replicates keeps.
 * For a cell (r, c) of the window of rows [first_row, first_row + n_rows) and all columns, k[s][a] is the key of slot
 * s * n_arms + a there and b[s] the smallest of k[s][.], the largest with maximize = 1.
 * never_as:  for the stores in which ESIM_NEVER occurs (arrival, the step of the peak) a key equal to ESIM_NEVER is replaced by
 *        never_as first, the rule of esim_ensemble_distances; ESIM_NEVER leaves it as it is.  Ignored by every other store.
 * best, sole, regret, sum:  indexed [(a * n_rows + r) * n_cols + c], each may be NULL.
 *        best    the replicates s with k[s][a] == b[s]; ties all count, so the arms of a cell may sum to more than S.
 *        sole    those of them in which no other arm attains b[s]: sole <= best, the arms' sole sum to at most S; with
 *                n_arms = 1, sole = best = S.
 *        regret  the sum over s of |k[s][a] - b[s]|, in 64 bits: what choosing arm a costs against the best arm of the same future.
 *        sum     the sum over s of k[s][a], in 64 bits.  best / S, sole / S, regret / S and sum / S are P(best), P(best alone),
 *                the expected regret and the mean of the arm.
 * totals:  may be NULL; totals[s * n_arms + a] is the sum of k[s][a] over ALL cells of the window, in 64 bits modulo 2^64: the
 *        whole-map figure per run, from which the pooled P(best) and the pooled regret follow on the host.
 * live_cells:  may be NULL; the cells of the window that the accumulators do not settle, as esim_ensemble_distances reports
 *        them.  A settled cell (every member holds the same key) is not read: best = S, sole = 0 (S with one arm), regret = 0,
 *        sum = S times the key, and the key in every member's total.
 *        Decided on the host before anything is enqueued: ESIM_EINVAL for n_arms 0 or above ESIM_ARMS_MAX or maximize not 0 or
 *        1; ESIM_ESTATE without a store, with nothing kept, or with a SIGNED store (the paired kinds are a difference of two
 *        arms already: a grid of them has no meaning); ESIM_ERANGE for rows outside the store or kept % n_arms != 0.
 *        n_rows == 0 gives zeros.  With every output NULL the call still validates.  It waits for the stream and leaves the
 *        accumulators and the store as they are; its tables on the device go when it returns. */
#define ESIM_ARMS_MAX 16
int  esim_ensemble_arms(esim_ctx *ctx, uint32_t n_arms, int maximize, uint32_t never_as,
                        uint32_t first_row, uint32_t n_rows,
                        uint32_t *best, uint32_t *sole,          /* [n_arms * n_rows * n_cols] each, or NULL */
                        uint64_t *regret, uint64_t *sum,         /* [n_arms * n_rows * n_cols] each, or NULL */
                        uint64_t *totals,                        /* [kept] or NULL */
                        uint64_t *live_cells);                   /* may be NULL */

/* Ensembles on several contexts: the unit of parallelism of an ensemble is the member.  Several contexts -- on several
 * devices, or several on one -- each upload the population, make the same begin (and the same esim_ensemble_keep_members) and
 * fold their share of the members; merging them gives, bit for bit, the ensemble folded in sequence on one context, because every
 * accumulator is an integer count or sum.  Every statistic behind the accumulators and the kept members works on the result
 * unchanged.  The contexts share nothing.
 * merge: adds every accumulator of src's kind in force into dst's (the counters and sums the kind owns and the member counter),
 *        appends src's kept members behind dst's in their order, adds src's folds to dst's, and leaves src exactly as it was.  A
 *        member's temporaries (the row planes, the series engine's small buffers) are not merged.  Both contexts must describe
 *        the same ensemble: the kind, where, n_rows, n_cols, every parameter of the begin, the population without its seeds and
 *        its number of citizens, by group the number of groups and their sizes, for the burden kinds the severity tables in
 *        force, and the store -- none on both sides, or the same `what` on both.  Checked on the host before anything is
 *        enqueued; a refused call leaves both contexts untouched:
 *          ESIM_EINVAL  a null context, dst == src
 *          ESIM_ESTATE  no upload or no begin in force on either side; a descriptor that differs (esim_last_error of dst names the
 *                       first field that does); a communicator of several ranks or a shard (the rule of esim_restart)
 *          ESIM_ERANGE  dst keeps more members with src's than its store takes
 *        A src without a member folded is a valid call that changes nothing.  The call waits for src's stream on the host, then
 *        enqueues on dst's stream and does not wait for it: src's accumulators and kept members must stay as they are (no fold,
 *        begin, upload or destroy on src) until dst has been waited for -- any read-out of dst, or esim_synchronize.  After a
 *        HIP failure mid-way the call returns ESIM_ENODEVICE and dst's accumulators are undefined until its next begin.
 *        src's accumulators come to dst's device piece by piece through a staging buffer of bounded size that dst keeps
 *        (hipMemcpyPeerAsync; between two contexts of one device that is a device-to-device copy).
 * save_size, save:  the ensemble in force as bytes -- a magic word, a version, the descriptor above, members, folds and kept, the
 *        accumulators, the kept planes; little-endian.  ESIM_ESTATE as merge; ESIM_ERANGE for a buffer smaller than save_size.
 *        save waits for the stream.
 * load:  a merge from bytes: it needs a begin of the same descriptor in force and ADDS.  Behind a fresh begin (and
 *        esim_ensemble_keep_members where the blob has a store) it restores; an ensemble saved, loaded later and folded further is
 *        the ensemble folded without the break.  No length is taken from the blob on trust: `bytes` must be exactly what the
 *        descriptor in force implies with the blob's kept members.  ESIM_EINVAL for a buffer that is no blob of this version,
 *        is truncated or longer, or was saved from another ensemble (the codes of esim_checkpoint_restore); ESIM_ERANGE when
 *        the store in force has no room for the blob's members; ESIM_ESTATE as merge.  A refused call leaves the context
 *        untouched.  It waits for the stream before it returns: the buffer is the caller's again.
 * Threads: one host thread at a time per context, any number of contexts at once -- contexts hold no state in common, and every
 * entry point makes its context's device current for the calling thread.  A merge uses both of its contexts. */
int  esim_ensemble_merge(esim_ctx *dst, esim_ctx *src);
int  esim_ensemble_save_size(esim_ctx *ctx, size_t *bytes);
int  esim_ensemble_save(esim_ctx *ctx, void *buf, size_t cap);
int  esim_ensemble_load(esim_ctx *ctx, const void *buf, size_t bytes);

/* Hospital burden: admissions, bed occupancy and deaths laid over a finished run.  In the model's SEIR(+V) rules
 * nothing that happens to a case after its onset feeds back into transmission, so severity is drawn after the fact, one Philox
 * block per case under the contract below, as the infector draw is.  No step kernel is touched; a run that never asks pays nothing.
 * Steps are hours.
 * Parameters: esim_burden_params holds thresholds per group (the labels of esim_set_groups; Population.age_bands gives age bands)
 *        and two CDFs, all uint32: admit_thr[n_groups], death_thr[n_groups]; delay_cdf[n_delay] and stay_cdf[n_stay], ascending,
 *        n_delay, n_stay <= ESIM_BURDEN_BINS (a count of 0 is a fixed delay of 0 / a fixed stay of one unit); 1 <= delay_unit,
 *        stay_unit <= 65535.  esim_burden_set copies them to the device.  With n_groups > 1 it needs labels with the same n_groups
 *        (ESIM_ESTATE otherwise); with n_groups == 1 no labels are needed: everybody is group 0.  ESIM_EINVAL: a null table,
 *        n_groups 0 or above ESIM_MAX_GROUPS, a count above ESIM_BURDEN_BINS, a CDF that descends, a unit of 0 or above 65535.
 *        The tables stay in force through esim_reset, esim_restart, esim_restart_seeded, esim_snapshot and esim_rollback; they are
 *        dropped by an upload, by esim_burden_drop, and (tables of several groups) by an esim_set_groups with another group count;
 *        not part of a checkpoint.  esim_burden_get returns the tables in force (any pointer NULL; the CDF outputs hold
 *        ESIM_BURDEN_BINS entries, of which the counts are written); ESIM_ESTATE without tables.
 * Cases: a citizen of the exposure log with an onset: onset = ts + exposed_time + 1 for the exposure step ts, 0 for an index case
 *        -- the first step after which the citizen is Infected.  onset <= t_done must hold (t_done: the steps run), and a
 *        citizen vaccinated at the end of step v is a case only if v - 1 >= onset: it was Infected after at least one step.  A
 *        citizen vaccinated while Exposed is no case; a later vaccination changes nothing about a case's outcome.
 * Draw:  for a case with global id g = citizen_id_base + c in group k, (w0, w1, w2, w3) = Philox4x32-10 over the counter
 *        (g, onset, ESIM_SLOT_BURDEN = 6, 0) under the seed, the raw block.  After an esim_rollback under another seed the
 *        snapshot's seed applies where onset <= the snapshot's step, the new one otherwise.
 *          admitted    iff w0 < admit_thr[k]
 *          admit_step  = onset + delay_unit * #{i : delay_cdf[i] <= w1}
 *          end_step    = admit_step + stay_unit * (1 + #{i : stay_cdf[i] <= w2})
 *          died        iff admitted and w3 < death_thr[k], at end_step
 *        An admitted case occupies a bed after the steps admit_step .. end_step - 1.  All of it is determined at onset:
 *        admit_step and end_step may lie beyond the steps run.
 * esim_burden_outcomes: per citizen, admit_step and end_step (ESIM_NEVER where the citizen is no admitted case) and died (1 / 0);
 *        any output may be NULL.
 * esim_burden_series: rows [n_rows][n_cols] under the row conventions of esim_area_status_series.  what = ESIM_BURDEN_ADMISSIONS /
 *        ESIM_BURDEN_DEATHS: event rows, a row sums the admissions (deaths) of the `stride` steps from its step on;
 *        ESIM_BURDEN_OCCUPANCY: the beds occupied after the row's step.  where = ESIM_BY_ALL (one column), ESIM_AREA_HOME or
 *        ESIM_BY_GROUP.  ESIM_ERANGE for first_step 0 and for rows beyond the steps run: what happens later appears in
 *        esim_burden_outcomes and in no row.
 * esim_burden_summary: esim_curve_summary of the occupancy curve over [first_step, last_step] -- peak, peak_step, steps_at_least,
 *        first_at_least, last_at_least as there, bed_steps the sum of the curve -- and the admissions and the deaths whose step
 *        lies inside the window, [n_cols] each, any NULL.  Arguments are checked as esim_curve_summary checks them; the pair
 *        engine, scan and reduction are the same, and esim_pair_stats reports the call.
 * esim_ensemble_begin_burden_peaks: the peaks kind of the ensemble accumulators over the occupancy curve: esim_ensemble_fold
 *        summarises the member as esim_burden_summary does and folds it as the peaks kind folds a status curve;
 *        esim_ensemble_read_peaks reads it, esim_ensemble_keep_members, quantiles and exceedance work behind it unchanged.
 * Every call is ESIM_ESTATE before an upload, without tables in force, with tables of several groups whose labels are gone, on a
 * context that holds a shard or has a communicator of several ranks; a refused call leaves its outputs untouched.  The calls
 * leave the simulation state, the records and the exposure log as they are.  Temporary device memory as esim_curve_summary, plus
 * 8 B per column (summary), 4 B per cell (series), 9 B per citizen (outcomes). */
#define ESIM_BURDEN_BINS 64
enum { ESIM_BURDEN_ADMISSIONS = 0, ESIM_BURDEN_OCCUPANCY = 1, ESIM_BURDEN_DEATHS = 2 };   /* `what` of esim_burden_series */
typedef struct esim_burden_params {
    uint32_t n_groups;
    const uint32_t *admit_thr, *death_thr;         /* [n_groups] each */
    uint32_t delay_unit, n_delay;
    const uint32_t *delay_cdf;                     /* [n_delay] */
    uint32_t stay_unit, n_stay;
    const uint32_t *stay_cdf;                      /* [n_stay] */
} esim_burden_params;
int  esim_burden_set(esim_ctx *ctx, const esim_burden_params *p);
int  esim_burden_drop(esim_ctx *ctx);
int  esim_burden_get(esim_ctx *ctx, uint32_t *n_groups, uint32_t *admit_thr, uint32_t *death_thr, uint32_t *delay_unit, uint32_t *n_delay,
                     uint32_t *delay_cdf, uint32_t *stay_unit, uint32_t *n_stay, uint32_t *stay_cdf);
int  esim_burden_outcomes(esim_ctx *ctx, uint32_t *admit_step, uint32_t *end_step, uint8_t *died /* [n_citizens] each, any may be NULL */);
int  esim_burden_series(esim_ctx *ctx, int where, int what, uint32_t first_step, uint32_t n_rows, uint32_t stride, uint32_t *out /* [n_rows * n_cols] */);
int  esim_burden_summary(esim_ctx *ctx, int where, uint32_t first_step, uint32_t last_step, uint32_t threshold,
                         uint32_t *peak, uint32_t *peak_step, uint32_t *steps_at_least, uint32_t *first_at_least, uint32_t *last_at_least,
                         uint64_t *bed_steps, uint32_t *admissions, uint32_t *deaths /* [n_cols] each, any may be NULL */);
int  esim_ensemble_begin_burden_peaks(esim_ctx *ctx, int where, uint32_t first_step, uint32_t last_step, uint32_t threshold, uint32_t min_peak);

/* Hospital burden across runs: a run's ADMITTED CASES AS A LIST ON THE DEVICE that outlives the run -- one entry
 * (citizen, admit_step, end_step, died) of 12 B for every case the contract above admits, under the tables and labels in force and
 * the steps run; admit_step and end_step may lie beyond the run, the consumers clip them.  The order of a list is unspecified;
 * every output below is an integer sum over it, exact and reproducible.  No step kernel is touched and no existing output changes.
 * esim_burden_baseline_keep: collects the list of the run as it stands and keeps it: 12 B per entry of the exposure log, allocated
 *        at the first keep and grown when a later run needs more; one baseline per context, a later keep replaces it.  Kept with
 *        it: the steps run, the entries, the deaths among them and the parameters in force (the seed among them).  Independent
 *        of esim_baseline_keep.  It is kept through esim_reset, esim_restart, esim_restart_seeded, esim_snapshot, esim_rollback and
 *        esim_checkpoint_restore; dropped by an upload, esim_burden_baseline_drop and esim_destroy, and whenever the severity
 *        tables are replaced or dropped (esim_burden_set, esim_burden_drop, the esim_set_groups that drops tables of several
 *        groups): a comparison of two severity models is not what this is.  An esim_set_groups with the SAME group count keeps
 *        tables and baseline: the entries kept were drawn under the labels in force at the keep, and a caller who then sets other
 *        labels compares outcomes under two labelings.  Not part of a checkpoint.  Errors: those of esim_burden_outcomes, and
 *        ESIM_ENOMEM.  A keep that fails behind its checks (ESIM_ENOMEM, ESIM_ENODEVICE) leaves NO baseline kept: the earlier
 *        one is given up before the new one is collected, as esim_baseline_keep does.
 * esim_burden_baseline_info: the steps, the entries, the deaths among them and the parameters of the baseline kept; any pointer
 *        may be NULL.  esim_burden_baseline_drop forgets it (the allocation stays for the next keep).  Both are ESIM_ESTATE
 *        without a baseline.
 * esim_burden_baseline_read: the entries in no particular order, under the sized-call convention of esim_outbreaks: *n_out = the
 *        entries; ESIM_ERANGE with nothing written where cap is smaller; any array may be NULL.
 * esim_burden_compare: over the window [first_step, last_step], per column, the three totals of esim_burden_summary for both runs:
 *        bed_steps = the sum over the entries of |[admit_step, end_step - 1] cut to the window|, admissions = the entries with
 *        admit_step inside, deaths = the entries that died with end_step inside.  Each _b output is, cell for cell, what
 *        esim_burden_summary returned for that window at the moment of the keep, each _c output what it returns now; [n_cols]
 *        each, any NULL.  where = ESIM_BY_ALL, ESIM_AREA_HOME or ESIM_BY_GROUP (the labels in force NOW make the columns of both
 *        runs).  ESIM_ERANGE for first_step 0, last_step < first_step, or a last_step beyond the steps of either run;
 *        ESIM_ESTATE without a baseline.
 * esim_burden_compare_series: the rows of esim_burden_series(where, what, ...) for both runs, the baseline clipped at its own
 *        steps run, the current run at its own; either output may be NULL.  cumulative != 0: the prefix over the rows of the
 *        event kinds, summed on the device; ESIM_EINVAL with ESIM_BURDEN_OCCUPANCY.  ESIM_ERANGE for first_step 0 and when
 *        the last row's step lies beyond either run.
 * PAIRING: a case's Philox block is keyed by (citizen, onset).  A citizen who is a case in both runs with the same onset has the
 *        same outcome in both; a citizen whose onset shifts draws a different outcome.  The difference of two runs under one
 *        seed is therefore unbiased, and its variance is reduced only for the cases whose onset does not move.
 * esim_ensemble_begin_burden_series: accumulators [n_rows][n_cols] over the rows of esim_burden_series: esim_ensemble_fold makes
 *        the member's rows and adds members += 1 once and, per cell with value v, sum += v, sumsq += v * v, hit += 1 iff
 *        v >= min_count (beds against a capacity).  Read by esim_ensemble_read_series; esim_ensemble_keep_members, quantiles
 *        and exceedance work behind it unchanged.  A fold is ESIM_ERANGE, with nothing folded, when the last row lies beyond
 *        the member's steps.
 * esim_ensemble_begin_burden_paired: the paired kind's accumulators over the two row planes of esim_burden_compare_series; read by
 *        esim_ensemble_read_paired, the kept members are baseline - current, signed.  A fold is ESIM_ESTATE without a burden
 *        baseline: every member keeps its own before its policy run.  min_averted >= 1.
 * Every call that computes is ESIM_ESTATE in the cases esim_burden_outcomes names; a refused call leaves its outputs untouched.
 * Device memory beside the baseline: 12 B per log entry for the list of the run as it stands, allocated by the first call that
 * compares or folds and kept for the next (grown when a log is longer; freed by an upload and esim_destroy).  Temporary, freed
 * when the call returns: 4 B per citizen for the vaccination replay once a programme has run, 32 B per column (compare), 8 B per
 * cell (compare_series). */
int  esim_burden_baseline_keep(esim_ctx *ctx);
int  esim_burden_baseline_info(esim_ctx *ctx, uint32_t *steps, uint32_t *n_admitted, uint32_t *n_died, esim_params *p);
int  esim_burden_baseline_drop(esim_ctx *ctx);
int  esim_burden_baseline_read(esim_ctx *ctx, uint32_t *citizen, uint32_t *admit_step, uint32_t *end_step, uint8_t *died /* [cap] each, any may be NULL */,
                               uint32_t cap, uint32_t *n_out);
int  esim_burden_compare(esim_ctx *ctx, int where, uint32_t first_step, uint32_t last_step, uint64_t *bed_steps_b, uint64_t *bed_steps_c,
                         uint32_t *admissions_b, uint32_t *admissions_c, uint32_t *deaths_b, uint32_t *deaths_c /* [n_cols] each, any may be NULL */);
int  esim_burden_compare_series(esim_ctx *ctx, int where, int what, uint32_t first_step, uint32_t n_rows, uint32_t stride, int cumulative,
                                uint32_t *baseline /* [n_rows * n_cols] or NULL */, uint32_t *current /* same, or NULL */);
int  esim_ensemble_begin_burden_series(esim_ctx *ctx, int where, int what, uint32_t first_step, uint32_t n_rows, uint32_t stride, uint32_t min_count);
int  esim_ensemble_begin_burden_paired(esim_ctx *ctx, int where, int what, uint32_t first_step, uint32_t n_rows, uint32_t stride, int cumulative,
                                       uint32_t min_baseline, uint32_t min_averted);

/* GPU time per phase since the last reset, seconds, in the reference's timer labels
 * (simulator.rs:137,140,143; statistics.rs:138-140):
 *   out[0] "Generate Exposures", out[1] "Apply Exposures", out[2] "Apply Interventions", out[3] total.
 * Only measured while phase timing is enabled (it inserts events between phases). */
int  esim_enable_phase_timing(esim_ctx *ctx, int enable);
int  esim_phase_timings(esim_ctx *ctx, double out[4]);

/* Mean device time (ms) of a multi-workgroup time step -- HIP event before k_infected to HIP event after
 * k_finish on the context's stream -- over the steps timed since the last call.
 * esim_enable_kernel_timing(ctx, n) brackets every n-th such step (n = 0: off) and every launch of the
 * persistent kernel (esim_small_kernel_timing). */
int  esim_enable_kernel_timing(esim_ctx *ctx, int enable);
int  esim_kernel_timings(esim_ctx *ctx, double *step_ms, uint32_t *out_n);

/* While few citizens are Infected a time step is a handful of dependent memory round trips; a persistent
 * single-workgroup kernel then advances many steps per launch (workgroup barriers instead of kernel
 * boundaries).  It hands over to the multi-workgroup kernels whenever a step has more than `max_infected`
 * Infected citizens (default 128; 0 disables it).  esim_small_kernel_timing: accumulated duration (ms) and
 * steps of those launches while kernel timing is enabled, then resets the accumulators. */
int  esim_set_small_step_limit(esim_ctx *ctx, uint32_t max_infected);
int  esim_small_kernel_timing(esim_ctx *ctx, double *total_ms, uint64_t *steps);
/* The same idea for time-parallel chunks: while the chunk last read back had at most `max_pairs` (Infected citizen, step) pairs, a
 * chunk is ONE launch of one workgroup (k_chunk_tiny: census ahead, decisions, marks, draws and books of up to 64 Infected; a
 * chunk that has outgrown it does not advance and is run in the wide form next).  Default 2048; 0 disables it. */
int  esim_set_tiny_chunk_limit(esim_ctx *ctx, uint32_t max_pairs);
/* Pipelined steps: mean duration (ms) of the sampled k_pipe launches, how many were sampled, how many steps ran
 * pipelined since the last call. */
int  esim_pipeline_timing(esim_ctx *ctx, double *mean_step_ms, uint64_t *steps_timed, uint64_t *steps_run);

/* Diagnostics: the control block's view of the last chunk (t, chunk_ok, chunk_parallel, chunk_pairs, n_items,
 * items_per_wave, n_units, chunk_bus (steps of the chunk with riders on a bus), n_route_pairs_big (of the last chunk
 * whose books ran; 0 after one of the one-workgroup form, which does not count them), n_newexp, log_len, n_susceptible, lockdown, mask,
 * at_work, bus_dir). */
int  esim_debug_counters(esim_ctx *ctx, uint32_t out[16]);
/* Diagnostics of the tests: ESIM_GRID_CAP=<workgroups> in the environment (read at esim_upload_population, at least 1, kept per
 * context) caps the grid of every output kernel that loops over its items with a grid stride, so that a small world reaches
 * the second and later trips of those loops.  Production never sets it: unset, every grid is what its launch site asks for
 * and nothing is recorded.  While it is set, every such launch site keeps a record, which this call reads: sites[i] is the
 * site's name, "<file>:<line>" of the host code that sized the grid, NUL-terminated in ESIM_LAUNCH_SITE_CHARS bytes;
 * counts[3 * i + 0 .. 2] are the launches it sized, how many of them the cap clipped, and the largest
 * trips = ceil(items / (grid * items a workgroup takes per trip of its loop)) among them.  *out_n: the number of sites recorded; cap: the room of
 * sites and counts, in sites (ESIM_ERANGE when smaller than *out_n, which is set; cap = 0 with NULL arrays asks for the
 * number alone while nothing is recorded).  reset != 0 empties the records after reading them.  The records live in a fixed
 * table of 128 sites: a launch site beyond it makes this call fail with ESIM_ERANGE rather than drop the record silently.
 * The call waits for nothing and touches no device. */
#define ESIM_LAUNCH_SITE_CHARS 48
int  esim_debug_launches(esim_ctx *ctx, char *sites, uint32_t *counts, uint32_t cap, uint32_t *out_n, int reset);

const char *esim_last_error(const esim_ctx *ctx);   /* ctx may be NULL: last esim_create error */
void esim_destroy(esim_ctx *ctx);

/* The exposure-probability LUT the kernels use: thresholds[mask][n & 255] =
 * ceil(q * 2^32) with q = 1 - (1 - p_eff)^(n as u8) (citizen.rs:47-49,239;
 * disease.rs:131-154).  mask 0: p_eff = p, mask 1: p_eff = p - p*mask_effectiveness.
 * Pure host arithmetic; exported so parity tests can pin it. */
int  esim_threshold_lut(const esim_params *p, uint64_t out[512]);

/* ---- synthetic populations: stands in for load_census_data + osm_data +
 * SimulatorBuilder, whose inputs are not available.  Pure host code. ---- */
typedef struct esim_synth_spec {
    uint32_t n_citizens, n_areas, citizens_per_school, n_seeds;
    uint64_t seed;
    double   area_jitter;     /* per-area census population = mean * (1 +- jitter) */
    double   p_public_transport, p_mask_compliant;
    double   p_work_from_home; /* extra share of adults without a workplace (0: only what the build leaves at home) */
    double   p_teaching;       /* census group 9 "Elementary", mapped to Teaching */
    /* the OSM side of SimulatorBuilder's inputs, per Output Area: log-normal counts round(median * exp(sigma z)) */
    double   household_buildings_median, household_buildings_sigma;   /* dwellings; household size = pop / count + 1, output_area.rs:139 */
    double   p_area_without_households;                               /* such areas get no citizens, simulator_builder.rs:226-235 */
    double   workplace_buildings_median, workplace_buildings_sigma;   /* possible workplace buildings, simulator_builder.rs:717 */
    double   p_area_without_workplaces;                               /* "No Workplace buildings exist", simulator_builder.rs:827-835 */
    double   workplace_floor_median, workplace_floor_sigma;           /* floor area of one, m^2 (RawBuilding::size) */
    uint32_t teacher_candidate_schools;                               /* MAX_ITEMS_RETURNED = 200, osm_data/src/quadtree.rs:544 */
    uint32_t reserved;
} esim_synth_spec;
/* presets: "york", "yh_census", "syn3m5", "uk64m"  */
int  esim_synth_preset(const char *name, esim_synth_spec *out);
/* Follows SimulatorBuilder::build (simulator_builder.rs:1162-1292) on synthetic census / OSM inputs: Output Areas are the
 * cells of a near-square map in row-major order, households stand at points of their cell, students go to the closest
 * school, teachers to the closest one lacking class teachers (else they are its secondary staff), workers to a
 * workplace of their occupation inside their home area.  Allocates the arrays of *out (shared_* left empty); release
 * with esim_synth_free. */
int  esim_synth_create(const esim_synth_spec *spec, esim_population *out);
/* The shard `shard` of `n_shards` of the same world: the whole world is generated and cut (esim_shard_population) into
 * bands of the map with about the same expected work each (esim_shard_cuts, by_work = 1); citizen_id_base and n_citizens_global are set, Philox
 * counters stay global.  Commuters to a school across a cut make that school (and its rooms) shared. */
int  esim_synth_create_shard(const esim_synth_spec *spec, uint32_t shard, uint32_t n_shards, esim_population *out);
void esim_synth_free(esim_population *pop);
/* Cuts the shard of Output Areas [area_begin, area_end) out of a whole population:
 * citizens living there, every building/room they reference (remote ones become ghosts),
 * and shared tables laid out identically on every shard of the same `cuts`
 * (cuts[0..n_shards] are the area boundaries of all shards).  Release with esim_synth_free. */
int  esim_shard_population(const esim_population *whole, const uint32_t *cuts, uint32_t n_shards,
                           uint32_t shard, esim_population *out);
/* Area boundaries cuts_out[0..n_shards] of n_shards bands of the map: by_work == 0, about the same number of citizens each;
 * otherwise about the same expected work each -- a citizen is drawn for by the shard it lives on, in every list it is a member of
 * (household, work place, class room), so its weight is 1 + the sizes of those lists, a band's the sum over its residents.
 * Static weights: where the epidemic will sit is not known before the run. */
int  esim_shard_cuts(const esim_population *whole, uint32_t n_shards, int by_work, uint32_t *cuts_out);

#ifdef __cplusplus
}
#endif
#endif
