// esim_kernels_setting.h -- exposures by setting (household, work place, school, public transport), derived after the fact from
// the exposure log.  Every draw is a pure function of (seed, global citizen id, step, slot), and a building exposure
// of citizen c in step ts can only have come through the household list or through the work-side list of c: one replay of the
// household draw decides it.  k_setting_scatter turns the log into the exposure step per citizen; k_setting_attr counts, for
// every exposed citizen, the residents of its household that were Infected and at home in that step and draws slot
// ESIM_SLOT_HOME again; k_setting_rows and k_setting_tally count what it found.  A tie -- household and work-side draw both
// successful in one step -- is credited to the household: the work side is never replayed here.  Nothing here writes
// simulation state.
#pragma once

#define SETTING_TE_NONE 0xFFFFFFFFu    // exposure step of a citizen the log does not hold

struct Setting {
    uint32_t t_done;                // steps run so far
    uint32_t t_all;                 // first step that vaccinated the whole eligible set (0xFFFFFFFF: none)
    uint32_t seam_step;             // entries up to this step were drawn under the old seed and LUT (0: no seam)
    uint32_t old_seed_lo, old_seed_hi;
    const uint64_t *old_thr;        // [2][256], or nullptr without a seam
    uint32_t *te_of;                // [n] TE_BIAS + exposure step from the log (the seeds: below TE_BIAS + 1), SETTING_TE_NONE: never
    const uint32_t *vax_of;         // [n] step at whose end a citizen was set Vaccinated (k_area_vax_replay), or nullptr
    const uint8_t *at_work, *on_bus; // [t_done + 1] the two global bits of every step
    uint8_t *setting;               // [n] ESIM_SETTING_*, ESIM_SETTING_NONE
    uint32_t *unexplained;          // building exposures that neither side can have drawn
};

// te_of[c] = the exposure step of citizen c (biased), from the position of its log entry.  A lane per entry.
__global__ __launch_bounds__(TPB) void k_setting_scatter(Dev d, Setting q, uint32_t log_len)
{
    for (uint32_t i = blockIdx.x * TPB + threadIdx.x; i < log_len; i += gridDim.x * TPB) {
        const uint32_t c = d.log[i];
        if (c < d.n) q.te_of[c] = log_te(d, i, q.t_done + TE_BIAS);
    }
}

// Does step ts lie in the infected_time + 1 Infected steps of citizen m, which follow the Exposed ones behind its exposure step
// (status_of)?
__device__ __forceinline__ bool in_infected_steps(const Dev &d, const Setting &q, uint32_t m, int ts)
{
    const uint32_t tm = q.te_of[m];
    if (tm == SETTING_TE_NONE) return false;
    const int inf = (int)tm - (int)TE_BIAS + (int)d.exposed_time + 1;
    return ts >= inf && ts <= inf + (int)d.infected_time;
}

// Was citizen m, whose word is w, set Vaccinated at the end of a step before ts?  (It is still Infected in that step itself.)
__device__ __forceinline__ bool vaccinated_before(const Setting &q, uint32_t m, uint32_t w, int ts)
{
    if (CW_TE(w) != TE_VACCINATED) return false;
    const uint32_t own = q.vax_of ? q.vax_of[m] : 0xFFFFFFFFu, v = q.t_all < own ? q.t_all : own;
    return v != 0xFFFFFFFFu && (uint32_t)ts > v;
}

// Was resident m Infected in step ts and standing in its household's building?  Infected during the infected_time + 1 steps
// behind the Exposed ones, still so in the step at whose end it was vaccinated; away while on a bus or at work.
__device__ __forceinline__ bool infected_at_home(const Dev &d, const Setting &q, uint32_t m, int ts, bool work_hour, bool bus_hour)
{
    if (!in_infected_steps(d, q, m, ts)) return false;
    const uint32_t w = d.cit[m];
    if ((bus_hour && (w & FL_USES_PT)) || (work_hour && (w & FL_HAS_WORK))) return false;
    return !vaccinated_before(q, m, w, ts);
}

// A lane per citizen: households are tiny and, in a home-sorted population, neighbouring lanes walk the same few words.
__global__ __launch_bounds__(TPB) void k_setting_attr(Dev d, Setting q)
{
    for (uint32_t c = blockIdx.x * TPB + threadIdx.x; c < d.n; c += gridDim.x * TPB) {
        const uint32_t te = q.te_of[c];
        uint32_t out = ESIM_SETTING_NONE;
        const int ts = (int)te - (int)TE_BIAS;
        if (te != SETTING_TE_NONE && ts >= 1 && ts <= (int)q.t_done) {        // (the index cases lie before step 1)
            const uint32_t w = d.cit[c];
            if (w & CW_BUS_EXPOSED) out = ESIM_SETTING_TRANSPORT;
            else {
                const bool work_hour = q.at_work[ts] != 0u, bus_hour = q.on_bus[ts] != 0u;
                const uint32_t b = d.home[c];
                uint32_t n_home = 0u;
                if (b < d.n_bld) {
                    const uint32_t lo = d.res_off[b], hi = d.res_off[b + 1u];
                    if (lo <= hi && hi <= d.n)
                        for (uint32_t r = lo; r < hi; ++r) {
                            const uint32_t m = d.res_idx ? d.res_idx[r] : r;
                            if (m < d.n && infected_at_home(d, q, m, ts, work_hour, bus_hour)) ++n_home;
                        }
                }
                // the `here` rule of member_pairs, kind 0: a commuter to another area is away while the at-work bit is 1
                const bool here = !(work_hour && (w & FL_HAS_WORK) && !(w & FL_SAME_AREA));
                bool hit = false;
                if (n_home && here) {
                    const bool old = (uint32_t)ts <= q.seam_step && q.old_thr;
                    const uint64_t seed = old ? ((uint64_t)q.old_seed_hi << 32) | q.old_seed_lo : ((uint64_t)d.seed_hi << 32) | d.seed_lo;
                    const uint32_t mask = ts >= 2 ? d.records[ts - 1].mask_status : (uint32_t)ESIM_MASK_NONE;
                    const uint32_t row = (!(w & FL_MASK_COMPLIANT) && mask == ESIM_MASK_EVERYWHERE) ? 1u : 0u;
                    const uint64_t thr = (old ? q.old_thr : d.thr)[row * 256u + (n_home & 255u)];   // `as u8`, citizen.rs:239
                    hit = esim_u32(seed, d.id_base + c, (uint32_t)ts, ESIM_SLOT_HOME) < thr;
                }
                if (hit) out = ESIM_SETTING_HOUSEHOLD;
                else if ((w & FL_HAS_WORK) && ((w & FL_SAME_AREA) || work_hour)) out = (w & FL_WORK_SCHOOL) ? ESIM_SETTING_SCHOOL : ESIM_SETTING_WORKPLACE;
                else atomicAdd(q.unexplained, 1u);
            }
        }
        q.setting[c] = (uint8_t)out;
    }
}

// The building an exposure of citizen c with that setting is credited to; ESIM_NO_ROOM: none.
__device__ __forceinline__ uint32_t setting_building(const Dev &d, uint32_t c, uint32_t s)
{
    return s == ESIM_SETTING_HOUSEHOLD ? d.home[c] : (s == ESIM_SETTING_WORKPLACE || s == ESIM_SETTING_SCHOOL) ? d.work[c] : ESIM_NO_ROOM;
}

// esim_exposure_settings: the building credited per citizen, written over the exposure steps (a lane reads its own entries only).
__global__ __launch_bounds__(TPB) void k_setting_building(Dev d, Setting q)
{
    for (uint32_t c = blockIdx.x * TPB + threadIdx.x; c < d.n; c += gridDim.x * TPB) q.te_of[c] = setting_building(d, c, q.setting[c]);
}

struct SettingRows {
    uint32_t where, mask, first, n_rows, stride, n_cols;
    const uint16_t *grp;            // [n] labels, ESIM_BY_GROUP only
    uint32_t *rows;                 // [n_rows][n_cols], zeroed by the caller
};

// Event rows, addressed as the incidence rows of the series engine: a lane per log entry, one add at the row of its step.  By
// setting there are four columns a row and the log is in time order, so a wavefront's entries fall into a handful of cells: the
// lanes of a cell are counted by its first one (a ballot per cell), one atomic per cell and wavefront.  Every lane of a wavefront
// makes the same trips.
__global__ __launch_bounds__(TPB) void k_setting_rows(Dev d, Setting q, SettingRows r, uint32_t log_len)
{
    const uint32_t lane = threadIdx.x & 63u;
    const size_t cells = (size_t)r.n_rows * r.n_cols;
    for (uint64_t i0 = (uint64_t)blockIdx.x * TPB; i0 < (uint64_t)log_len; i0 += (uint64_t)gridDim.x * TPB) {
        const uint64_t i = i0 + threadIdx.x;
        size_t cell = ~(size_t)0;
        if (i < (uint64_t)log_len) {
            const uint32_t c = d.log[i];
            if (c < d.n) {
                const uint32_t s = q.setting[c], te = q.te_of[c];
                const int ts = (int)te - (int)TE_BIAS;
                if (s < ESIM_N_SETTINGS && ((r.mask >> s) & 1u) && te != SETTING_TE_NONE && ts >= (int)r.first && ts <= (int)q.t_done) {
                    const uint64_t row = (uint64_t)((uint32_t)ts - r.first) / r.stride;
                    const uint32_t col = r.where == ESIM_BY_SETTING ? s : r.where == ESIM_BY_GROUP ? (uint32_t)r.grp[c] : d.home[c] < d.n_bld ? d.bld_area[d.home[c]] : 0xFFFFFFFFu;
                    if (row < r.n_rows && col < r.n_cols) cell = (size_t)row * r.n_cols + col;
                }
            }
        }
        const bool live = cell < cells;
        if (r.where != ESIM_BY_SETTING) { if (live) atomicAdd(&r.rows[cell], 1u); continue; }
        unsigned long long todo = __ballot(live);
        while (todo) {                                                // (wave-uniform: every lane sees the same ballots)
            const uint32_t lead = (uint32_t)__ffsll((long long)todo) - 1u;
            const uint32_t lo = __shfl((uint32_t)cell, lead, 64), hi = __shfl((uint32_t)((uint64_t)cell >> 32), lead, 64);
            const unsigned long long same = __ballot(live && (uint32_t)cell == lo && (uint32_t)((uint64_t)cell >> 32) == hi);
            if (lane == lead) atomicAdd(&r.rows[cell], (uint32_t)__popcll(same));
            todo &= ~same;
        }
    }
}

// esim_building_exposures: counts[b] += 1 per exposure of steps [first, last] credited to building b.  A lane per log entry.
__global__ __launch_bounds__(TPB) void k_setting_tally(Dev d, Setting q, uint32_t first, uint32_t last, uint32_t log_len, uint32_t *counts)
{
    for (uint32_t i = blockIdx.x * TPB + threadIdx.x; i < log_len; i += gridDim.x * TPB) {
        const uint32_t c = d.log[i];
        if (c >= d.n) continue;
        const uint32_t te = q.te_of[c];
        const int ts = (int)te - (int)TE_BIAS;
        if (te == SETTING_TE_NONE || ts < (int)first || ts > (int)last) continue;
        const uint32_t b = setting_building(d, c, q.setting[c]);
        if (b < d.n_bld) atomicAdd(&counts[b], 1u);
    }
}
