// esim_kernels_area_status.h -- esim_area_status_series: per-Output-Area rows of all five statuses over the steps already
// run, by the area a citizen stands in or by the area of its household, and of the exposures by household area.  The interval
// logic is that of k_group_series; the spatial part is new.  Where everybody with a work place stands is one global bit per
// step (RunShape::aw), so instead of cutting a citizen's interval at every change of that bit (k_area_series) the rows are
// counted twice, once per value of the bit:
//   plane 0: everybody in the area of its household (where it stands while the bit is 0);
//   plane 1: everybody with a work place in the area of that, the others at home (where it stands while the bit is 1).
// An interval adds +1 at its first row and -1 behind its last one to both planes, whatever happens to the bit inside it, and
// k_area_status_prefix, a lane per area, sums both columns and keeps, row by row, the plane the bit of that step selects.
// The work per log entry and per vaccinated citizen does not grow with the length of the run.  Nothing writes simulation state.
#pragma once

struct AreaStatus {
    uint32_t what, first, n_rows, stride;
    uint32_t t_done;                // steps run so far
    uint32_t t_all;                 // first step that vaccinated the whole eligible set (0xFFFFFFFF: none)
    const uint32_t *vax_of;         // [n] step at whose end a citizen was set Vaccinated (k_area_vax_replay), or nullptr
    const uint8_t *at_work;         // [t_done + 1], read where p1 is given
    uint32_t *p0;                   // [n_rows][n_areas] plane 0, and the result
    uint32_t *p1;                   // [n_rows][n_areas] plane 1, or nullptr: rows by household area
};

// A citizen has the status during the steps [p, e], first <= p <= e <= t_done; a0 / a1 < n_areas are its areas in the two
// planes.  +1 at the first row inside, -1 behind the last one; an interval that reaches the last row has nothing behind it.
__device__ __forceinline__ void planes_add(const AreaStatus &q, uint32_t n_areas, uint32_t p, uint32_t e, uint32_t a0, uint32_t a1)
{
    const uint64_t i_lo = ((uint64_t)(p - q.first) + q.stride - 1u) / q.stride;
    uint64_t i_hi = (uint64_t)(e - q.first) / q.stride;
    if (i_lo >= q.n_rows) return;
    if (i_hi >= q.n_rows) i_hi = q.n_rows - 1u;
    if (i_lo > i_hi) return;
    const bool closed = i_hi + 1u < q.n_rows;
    atomicAdd(&q.p0[i_lo * n_areas + a0], 1u);
    if (closed) atomicSub(&q.p0[(i_hi + 1u) * n_areas + a0], 1u);
    if (!q.p1) return;
    atomicAdd(&q.p1[i_lo * n_areas + a1], 1u);
    if (closed) atomicSub(&q.p1[(i_hi + 1u) * n_areas + a1], 1u);
}

// The two areas of citizen c; false where the population's tables do not hold them.
__device__ __forceinline__ bool plane_areas(const Dev &d, uint32_t c, uint32_t w, uint32_t *a0, uint32_t *a1)
{
    *a0 = d.bld_area[d.home[c]];
    *a1 = (w & FL_HAS_WORK) ? d.bld_area[d.work[c]] : *a0;
    return *a0 < d.n_areas && *a1 < d.n_areas;
}

// The step (capped by t_all) at whose end a citizen whose word is Vaccinated was vaccinated; 0xFFFFFFFF: not known.
__device__ __forceinline__ uint32_t vax_step(const AreaStatus &q, uint32_t c)
{
    const uint32_t v = q.vax_of ? q.vax_of[c] : 0xFFFFFFFFu;
    return q.t_all < v ? q.t_all : v;
}

// A lane per exposure-log entry (the seeds are in the log), its exposure step ts taken from the entry's position (log_te).
// INCIDENCE: one add at (row of ts, household area), buildings and public transport alike, the seeds not.  EXPOSED, INFECTED,
// RECOVERED: the interval of k_group_series -- Exposed after the steps ts .. ts + exposed_time, Infected after the
// infected_time + 1 steps that follow, Recovered from then on; a citizen that was vaccinated leaves its interval with the step
// before the one at whose end it was vaccinated.  SUSCEPTIBLE collects everybody who is NOT Susceptible: the three as one.
__global__ __launch_bounds__(TPB) void k_area_status_log(Dev d, AreaStatus q, uint32_t log_len)
{
    for (uint32_t i = blockIdx.x * TPB + threadIdx.x; i < log_len; i += gridDim.x * TPB) {
        const uint32_t c = d.log[i];
        if (c >= d.n) continue;
        const uint32_t w = d.cit[c];
        uint32_t a0, a1;
        if (!plane_areas(d, c, w, &a0, &a1)) continue;
        const int ts = (int)log_te(d, i, q.t_done + TE_BIAS) - (int)TE_BIAS;   // exposure step; seeds: -(exposed_time + 1)
        if (q.what == ESIM_AREA_SERIES_INCIDENCE) {
            if (ts < (int)q.first || ts > (int)q.t_done) continue;
            const uint64_t row = (uint64_t)((uint32_t)ts - q.first) / q.stride;
            if (row < q.n_rows) atomicAdd(&q.p0[row * d.n_areas + a0], 1u);
            continue;
        }
        const int inf = ts + (int)d.exposed_time + 1, rec = inf + (int)d.infected_time + 1;
        int p, e = (int)q.t_done;
        if (q.what == ESIM_EXPOSED) { p = ts; e = inf - 1; }
        else if (q.what == ESIM_INFECTED) { p = inf; e = rec - 1; }
        else if (q.what == ESIM_RECOVERED) p = rec;
        else p = ts;                                                  // SUSCEPTIBLE: not Susceptible from the exposure on
        if (CW_TE(w) == TE_VACCINATED) {
            const uint32_t v = vax_step(q, c);
            if (v != 0xFFFFFFFFu && (int)v - 1 < e) e = (int)v - 1;
        }
        if (e > (int)q.t_done) e = (int)q.t_done;
        if (p < (int)q.first) p = (int)q.first;
        if (e < p) continue;
        planes_add(q, d.n_areas, (uint32_t)p, (uint32_t)e, a0, a1);
    }
}

// A lane per citizen, for the VACCINATED (and SUSCEPTIBLE) rows: +1 from the vaccinating step on.
__global__ __launch_bounds__(TPB) void k_area_status_vax(Dev d, AreaStatus q)
{
    for (uint32_t c = blockIdx.x * TPB + threadIdx.x; c < d.n; c += gridDim.x * TPB) {
        const uint32_t w = d.cit[c];
        if (CW_TE(w) != TE_VACCINATED) continue;
        const uint32_t v = vax_step(q, c);
        uint32_t a0, a1;
        if (v == 0xFFFFFFFFu || v > q.t_done || !plane_areas(d, c, w, &a0, &a1)) continue;
        planes_add(q, d.n_areas, v < q.first ? q.first : v, q.t_done, a0, a1);
    }
}

// tab[key] += the number of citizens in a run of neighbouring lanes with the same key, added by the run's first lane (the
// trick of k_area_census: citizens are normally home-sorted).  Every lane of the wavefront calls it.
__device__ __forceinline__ void run_add(uint32_t *tab, uint32_t key, bool valid, uint32_t lane)
{
    const uint32_t prev = __shfl_up(key, 1, 64);
    const bool head = valid && (lane == 0u || prev != key);
    const unsigned long long heads = __ballot(head), live = __ballot(valid);
    const unsigned long long above = lane == 63u ? 0ull : heads & (~0ull << (lane + 1u));
    const unsigned long long run = (above ? (above & (0ull - above)) - 1ull : ~0ull) & (~0ull << lane);   // this lane up to the next head
    if (head) atomicAdd(&tab[key], (uint32_t)__popcll(run & live));
}

// What the SUSCEPTIBLE rows are taken from: occ0[a] = the residents of area a, occ1[a] = who stands in a while everybody with
// a work place is at work (occ1 may be nullptr; both zeroed by the caller).  One pass over the citizens, the same trip count
// for every lane of a wavefront; lanes without a citizen, or with an area the tables do not hold, carry the key 0xFFFFFFFF.
__global__ __launch_bounds__(TPB) void k_area_occupancy(Dev d, uint32_t *occ0, uint32_t *occ1)
{
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t c0 = (uint64_t)blockIdx.x * TPB; c0 < (uint64_t)d.n; c0 += (uint64_t)gridDim.x * TPB) {
        const uint64_t c = c0 + threadIdx.x;
        uint32_t a0 = 0xFFFFFFFFu, a1 = 0xFFFFFFFFu;
        if (c < (uint64_t)d.n && !plane_areas(d, (uint32_t)c, d.cit[c], &a0, &a1)) a0 = a1 = 0xFFFFFFFFu;
        run_add(occ0, a0, a0 != 0xFFFFFFFFu, lane);
        if (occ1) run_add(occ1, a1, a1 != 0xFFFFFFFFu, lane);
    }
}

// Difference rows to counts, a lane per area walking down its column in both planes; row r keeps the plane that the at-work
// bit of its step selects, in place in plane 0.  With occ0 given (SUSCEPTIBLE) what has been summed is everybody who is not
// Susceptible, and the row is the plane's occupancy minus that.
__global__ __launch_bounds__(TPB) void k_area_status_prefix(AreaStatus q, uint32_t n_areas, const uint32_t *occ0, const uint32_t *occ1)
{
    const uint32_t a = blockIdx.x * TPB + threadIdx.x;
    if (a >= n_areas) return;
    const uint32_t o0 = occ0 ? occ0[a] : 0u, o1 = occ1 ? occ1[a] : 0u;
    uint32_t acc0 = 0u, acc1 = 0u;
    for (uint32_t r = 0; r < q.n_rows; ++r) {
        const size_t at = (size_t)r * n_areas + a;
        bool work = false;
        acc0 += q.p0[at];
        if (q.p1) { acc1 += q.p1[at]; work = q.at_work[q.first + r * q.stride] != 0u; }
        const uint32_t v = work ? acc1 : acc0;
        q.p0[at] = occ0 ? (work ? o1 : o0) - v : v;
    }
}
