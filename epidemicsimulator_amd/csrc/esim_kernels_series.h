// esim_kernels_series.h -- the series engine: rows over the steps already run, one column per key, behind esim_area_series,
// esim_group_series and esim_area_status_series.  Status rows: a lane per exposure-log entry derives the steps
// [p, e] during which its citizen has the status, cuts them at the vaccinating step, clips them to the window and adds +1 at
// the first row inside and -1 behind the last one; a lane per citizen does the same for the Vaccinated; a lane per column sums
// the differences.  Event rows: one add at the row of the exposure step, no sum.  The three entry points differ in the column
// key only.  Where everybody with a work place stands is one global bit per step (RunShape::aw), so the rows by the area stood
// in are counted twice, once per value of the bit, whatever the bit does inside an interval:
//   plane 0: everybody in the area of its household (where it stands while the bit is 0);
//   plane 1: everybody with a work place in the area of that, the others at home (where it stands while the bit is 1),
// and the sum keeps, row by row, the plane the bit of that step selects.  The work per log entry and per vaccinated citizen
// does not grow with the length of the run.  (One special case is left: esim_area_series(INFECTED) still counts that table in
// one plane, cutting a commuter's interval wherever the bit changes -- Series::tog, the piece walk of k_series_log.)  Nothing
// here writes simulation state.
#pragma once

enum { KEY_GROUP = 0, KEY_HOME = 1, KEY_STOOD = 2 };   // the column of a citizen: its label, the area of its household, the area it stands in
#define SERIES_EVENTS 5u           // `what` behind the five statuses: exposures by the step they happened in

struct Series {
    uint32_t what, first, n_rows, stride;
    uint32_t t_done;                // steps run so far
    uint32_t t_all;                 // first step that vaccinated the whole eligible set (0xFFFFFFFF: none)
    const uint32_t *vax_of;         // [n] step at whose end a citizen was set Vaccinated (k_area_vax_replay), or nullptr
    const uint8_t *at_work;         // [t_done + 1], KEY_STOOD only
    uint32_t *p0;                   // [n_rows][n_cols] plane 0, and the result
    uint32_t *p1;                   // [n_rows][n_cols] plane 1: status rows of KEY_STOOD, else nullptr
    uint32_t n_cols;                // groups or areas
    uint32_t key;                   // KEY_*
    const uint16_t *grp;            // [n] labels, KEY_GROUP only
    uint32_t skip_bus;              // event rows leave out the exposures on public transport
    uint32_t n_tog;                 // esim_area_series(INFECTED) only: one plane, a commuter's interval cut where the at-work bit changes
    const uint32_t *tog;            // [n_tog] steps s with at_work[s] != at_work[s - 1], ascending, or nullptr
};

// The two areas of citizen c; false where the population's tables do not hold them.
__device__ __forceinline__ bool plane_areas(const Dev &d, uint32_t c, uint32_t w, uint32_t *a0, uint32_t *a1)
{
    *a0 = d.bld_area[d.home[c]];
    *a1 = (w & FL_HAS_WORK) ? d.bld_area[d.work[c]] : *a0;
    return *a0 < d.n_areas && *a1 < d.n_areas;
}

// The column key: the columns of citizen c (word w) in plane 0 and plane 1, the same where there is one plane; false where
// they are not below n_cols.
__device__ __forceinline__ bool series_cols(const Dev &d, const Series &q, uint32_t c, uint32_t w, uint32_t *k0, uint32_t *k1)
{
    if (q.key != KEY_GROUP) return plane_areas(d, c, w, k0, k1);   // (n_cols = n_areas)
    *k0 = *k1 = q.grp[c];
    return *k0 < q.n_cols;
}

// The steps [p, e] after which a citizen exposed in step ts has the status (status_of's bounds), vaccinations apart: Exposed
// after ts .. ts + exposed_time, Infected after the infected_time + 1 steps that follow, Recovered from then on.  SUSCEPTIBLE
// collects everybody who is NOT Susceptible: the three as one.
__device__ __forceinline__ void status_interval(uint32_t what, int ts, uint32_t exposed_time, uint32_t infected_time, int *p, int *e)
{
    const int inf = ts + (int)exposed_time + 1, rec = inf + (int)infected_time + 1;
    *p = ts; *e = 0x7FFFFFFF;
    if (what == ESIM_EXPOSED) *e = inf - 1;
    else if (what == ESIM_INFECTED) { *p = inf; *e = rec - 1; }
    else if (what == ESIM_RECOVERED) *p = rec;
}

// The step (capped by t_all) at whose end a citizen whose word is Vaccinated was vaccinated; 0xFFFFFFFF: not known.
__device__ __forceinline__ uint32_t vax_step(const Series &q, uint32_t c)
{
    const uint32_t v = q.vax_of ? q.vax_of[c] : 0xFFFFFFFFu;
    return q.t_all < v ? q.t_all : v;
}

// [p, e] cut to the window's steps [first, t_done]; false where nothing is left.
__device__ __forceinline__ bool clip(const Series &q, int *p, int *e)
{
    if (*e > (int)q.t_done) *e = (int)q.t_done;
    if (*p < (int)q.first) *p = (int)q.first;
    return *p <= *e;
}

// A citizen has the status during the steps [p, e], first <= p <= e <= t_done; k0 / k1 < n_cols are its columns in the two
// planes.  +1 at the first row inside, -1 behind the last one; an interval that reaches the last row has nothing behind it.
__device__ __forceinline__ void rows_add(const Series &q, uint32_t p, uint32_t e, uint32_t k0, uint32_t k1)
{
    const uint64_t i_lo = ((uint64_t)(p - q.first) + q.stride - 1u) / q.stride;
    uint64_t i_hi = (uint64_t)(e - q.first) / q.stride;
    if (i_lo >= q.n_rows) return;
    if (i_hi >= q.n_rows) i_hi = q.n_rows - 1u;
    if (i_lo > i_hi) return;
    const bool closed = i_hi + 1u < q.n_rows;
    atomicAdd(&q.p0[i_lo * q.n_cols + k0], 1u);
    if (closed) atomicSub(&q.p0[(i_hi + 1u) * q.n_cols + k0], 1u);
    if (!q.p1) return;
    atomicAdd(&q.p1[i_lo * q.n_cols + k1], 1u);
    if (closed) atomicSub(&q.p1[(i_hi + 1u) * q.n_cols + k1], 1u);
}

// A lane per exposure-log entry (the seeds are in the log), its exposure step ts taken from the entry's position (log_te).
// Event rows: one add at the row of ts, the seeds not; with two columns the one the at-work bit of step ts selects (the area
// stood in at the exposure).  Status rows: status_interval, which a citizen that was vaccinated leaves with the step before
// the one at whose end it was vaccinated.
__global__ __launch_bounds__(TPB) void k_series_log(Dev d, Series q, uint32_t log_len)
{
    for (uint32_t i = blockIdx.x * TPB + threadIdx.x; i < log_len; i += gridDim.x * TPB) {
        const uint32_t c = d.log[i];
        if (c >= d.n) continue;
        const uint32_t w = d.cit[c];
        uint32_t k0, k1;
        if (!series_cols(d, q, c, w, &k0, &k1)) continue;
        const int ts = (int)log_te(d, i, q.t_done + TE_BIAS) - (int)TE_BIAS;   // exposure step; seeds: -(exposed_time + 1)
        if (q.what == SERIES_EVENTS) {
            if ((q.skip_bus && (w & CW_BUS_EXPOSED)) || ts < (int)q.first || ts > (int)q.t_done) continue;
            const uint64_t row = (uint64_t)((uint32_t)ts - q.first) / q.stride;
            if (row < q.n_rows) atomicAdd(&q.p0[row * q.n_cols + (q.key == KEY_STOOD && q.at_work[ts] ? k1 : k0)], 1u);
            continue;
        }
        int p, e;
        status_interval(q.what, ts, d.exposed_time, d.infected_time, &p, &e);
        if (CW_TE(w) == TE_VACCINATED) {
            const uint32_t v = vax_step(q, c);
            if (v != 0xFFFFFFFFu && (int)v - 1 < e) e = (int)v - 1;
        }
        if (!clip(q, &p, &e)) continue;
        if (!q.tog || k0 == k1) { rows_add(q, (uint32_t)p, (uint32_t)e, k0, k1); continue; }
        uint32_t k = 0u, k_hi = q.n_tog;                          // the piece walk: the first change of the at-work bit behind step p
        while (k < k_hi) { const uint32_t mid = (k + k_hi) >> 1; if (q.tog[mid] > (uint32_t)p) k_hi = mid; else k = mid + 1u; }
        for (uint32_t s = (uint32_t)p;;) {
            const uint32_t nxt = k < q.n_tog ? q.tog[k] : 0xFFFFFFFFu;
            const uint32_t pe = nxt - 1u < (uint32_t)e ? nxt - 1u : (uint32_t)e;
            rows_add(q, s, pe, q.at_work[s] ? k1 : k0, 0u);
            if (pe >= (uint32_t)e) break;
            s = nxt; ++k;
        }
    }
}

// A lane per citizen, for the VACCINATED (and SUSCEPTIBLE) rows: +1 from the vaccinating step on.
__global__ __launch_bounds__(TPB) void k_series_vax(Dev d, Series q)
{
    for (uint32_t c = blockIdx.x * TPB + threadIdx.x; c < d.n; c += gridDim.x * TPB) {
        const uint32_t w = d.cit[c];
        if (CW_TE(w) != TE_VACCINATED) continue;
        const uint32_t v = vax_step(q, c);
        uint32_t k0, k1;
        int p = (int)v, e = (int)q.t_done;
        if (v > q.t_done || !clip(q, &p, &e) || !series_cols(d, q, c, w, &k0, &k1)) continue;   // (0xFFFFFFFF: not known)
        rows_add(q, (uint32_t)p, (uint32_t)e, k0, k1);
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

// What the SUSCEPTIBLE rows by area are taken from: occ0[a] = the residents of area a, occ1[a] = who stands in a while
// everybody with a work place is at work (occ1 may be nullptr; both zeroed by the caller).  One pass over the citizens, the same
// trip count for every lane of a wavefront; lanes without a citizen, or with an area the tables do not hold, carry the key
// 0xFFFFFFFF.  (The groups' occupancy is their size, counted by esim_set_groups.)
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

// Difference rows to counts, a lane per column walking down it in both planes; row r keeps the plane that the at-work bit of
// its step selects, in place in plane 0.  With occ0 given (SUSCEPTIBLE) what has been summed is everybody who is not
// Susceptible, and the row is the plane's occupancy minus that.
__global__ __launch_bounds__(TPB) void k_series_prefix(Series q, const uint32_t *occ0, const uint32_t *occ1)
{
    const uint32_t a = blockIdx.x * TPB + threadIdx.x;
    if (a >= q.n_cols) return;
    const uint32_t o0 = occ0 ? occ0[a] : 0u, o1 = occ1 ? occ1[a] : 0u;
    uint32_t acc0 = 0u, acc1 = 0u;
    for (uint32_t r = 0; r < q.n_rows; ++r) {
        const size_t at = (size_t)r * q.n_cols + a;
        bool work = false;
        acc0 += q.p0[at];
        if (q.p1) { acc1 += q.p1[at]; work = q.at_work[q.first + r * q.stride] != 0u; }
        const uint32_t v = work ? acc1 : acc0;
        q.p0[at] = occ0 ? (work ? o1 : o0) - v : v;
    }
}
