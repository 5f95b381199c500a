// esim_kernels_household.h -- household outbreaks: on top of the settings of esim_kernels_setting.h and the tree of
// esim_kernels_tree.h, the cases and introductions of every household, the final-size tables over all households, and the
// household secondary attack rate -- of the housemates still Susceptible when a case became infectious, the ones it infected at
// home.  The first two are the same for every setting with a fixed member list, so they stand here once, for the residents of a
// building, the workers of a non-school building and the participants of a school room: k_list_members is a
// segmented reduction over a member list, a lane per entry; k_list_tables bins the places, a lane per place and a table per
// workgroup in LDS.  k_hh_sar walks the household of every case, a lane per log entry; its counting modes: esim_kernels_pairtab.h.
// Nothing here writes simulation state.
#pragma once

#define HH_CELLS ((uint32_t)ESIM_HH_BINS * ESIM_HH_BINS)           // counters of one final-size table of the households
#define PLACE_CELLS ((uint32_t)ESIM_PLACE_BINS * ESIM_PLACE_BINS)  // ... of the work places, rooms or schools
// Cases a lane of the LDS form walks at least before its workgroup hands over its table.  A walk is a chain of dependent loads,
// so the grid has to stay wide: 4 measured as fast as 1, 32 (an eighth of the workgroups) a quarter slower.
#ifndef HH_SAR_PER_LANE
#define HH_SAR_PER_LANE 4u
#endif

// The rows of the places of one member list: households, work places, rooms, or the schools that k_place_schools adds up.
struct Place {
    uint32_t n_places;                        // n_bld (households, work places, schools) or n_room (rooms)
    uint32_t *members;                        // [n_places] zeroed by the caller; nullptr for the households, whose sizes res_off holds
    uint32_t *cases, *intro, *first;          // [n_places] zeroed, zeroed, filled with ESIM_NEVER by the caller
    uint32_t *final_size, *intro_size;        // [HH_CELLS] (households) or [PLACE_CELLS] each, adjacent, zeroed by the caller
};

// The three member lists: the residents of the buildings (every citizen once, household after household: in the home-sorted
// layout entry r is citizen r and res_idx is null), the workers of the non-school buildings, the participants of the rooms.
enum { LIST_HOME = 0, LIST_WORK = 1, LIST_ROOM = 2 };
template <int LIST> __device__ __forceinline__ const uint32_t *list_off(const Dev &d) { return LIST == LIST_HOME ? d.res_off : LIST == LIST_ROOM ? d.room_off : d.wrk_off; }
template <int LIST> __device__ __forceinline__ const uint32_t *list_idx(const Dev &d) { return LIST == LIST_HOME ? d.res_idx : LIST == LIST_ROOM ? d.room_idx : d.wrk_idx; }
template <int LIST> __device__ __forceinline__ uint32_t list_len(const Dev &d) { return LIST == LIST_HOME ? d.n : LIST == LIST_ROOM ? d.n_room_idx : d.n_wrk_idx; }
template <int LIST> __device__ __forceinline__ uint32_t list_at(const uint32_t *idx, uint64_t r) { return LIST == LIST_HOME && !idx ? (uint32_t)r : idx[r]; }
template <int LIST> __device__ __forceinline__ uint32_t list_own() { return LIST == LIST_HOME ? ESIM_SETTING_HOUSEHOLD : LIST == LIST_ROOM ? ESIM_SETTING_SCHOOL : ESIM_SETTING_WORKPLACE; }
// The place citizen m is a member of, from the citizen: 0xFFFFFFFF where it is a member of no place of the list.
template <int LIST> __device__ __forceinline__ uint32_t list_place(const Dev &d, uint32_t m)
{
    if (LIST == LIST_HOME) return d.home[m];
    const uint32_t w = d.cit[m];
    if (!(w & FL_HAS_WORK) || ((w & FL_WORK_SCHOOL) != 0u) != (LIST == LIST_ROOM)) return 0xFFFFFFFFu;
    return LIST == LIST_ROOM ? d.room[m] : d.work[m];
}

// The size bin of the tables.  Households: the size itself, the last bin open-ended.  Places: exact below 16, then one bin per
// power of two, the last one open-ended.
template <bool HOME> __device__ __forceinline__ uint32_t list_bin(uint32_t x)
{
    if (HOME) return x < ESIM_HH_BINS - 1u ? x : ESIM_HH_BINS - 1u;
    if (x < 16u) return x;
    const uint32_t b = 12u + (31u - (uint32_t)__clz((int)x));
    return b < ESIM_PLACE_BINS - 1u ? b : ESIM_PLACE_BINS - 1u;
}

// The last step f at which a case that becomes infectious in f still finds citizen m Susceptible: m is Susceptible after step
// f - 1 iff f <= the smaller of its exposure step and the step at whose end it was set Vaccinated (vaccinated_before's rule).
// 0 for an index case: at risk from nobody.  0xFFFFFFFF for a citizen never touched.
__device__ __forceinline__ uint32_t hh_susceptible_end(const Dev &d, const Setting &q, uint32_t m)
{
    const uint32_t te = q.te_of[m];
    uint32_t end = te == SETTING_TE_NONE ? 0xFFFFFFFFu : te > TE_BIAS ? te - TE_BIAS : 0u;
    if (CW_TE(d.cit[m]) == TE_VACCINATED) {
        const uint32_t own = q.vax_of ? q.vax_of[m] : 0xFFFFFFFFu, v = q.t_all < own ? q.t_all : own;
        if (v < end) end = v;
    }
    return end;
}

// Per place of a list: its cases, its introductions and the smallest cohort step among its cases; for a list other than the
// residents its members too.  A lane per entry r of the list.  The place comes from the citizen and is checked against the list
// it was found in (p < n_places, off[p] <= r < off[p + 1] <= the list's length).  Neighbouring lanes share a place: the lanes of
// a run are reduced by run_sums and counted by the run's first lane, so a place costs three atomics per wavefront it touches,
// whether it has two members or ten thousand.  The number of members is the list's own length and is stored by the lane that
// holds the place's first entry.  Every lane of a wavefront makes the same trips.
template <int LIST>
__global__ __launch_bounds__(TPB) void k_list_members(Dev d, Setting q, Place h)
{
    const uint32_t n_list = list_len<LIST>(d);
    const uint32_t *off = list_off<LIST>(d), *idx = list_idx<LIST>(d);
    for (uint64_t r0 = (uint64_t)blockIdx.x * TPB; r0 < (uint64_t)n_list; r0 += (uint64_t)gridDim.x * TPB) {
        const uint64_t r = r0 + threadIdx.x;
        uint32_t p = 0xFFFFFFFFu, step = ESIM_NEVER, size = 0u;
        bool is_case = false, is_intro = false, is_first = false;
        if (r < (uint64_t)n_list) {
            const uint32_t m = list_at<LIST>(idx, r);
            const uint32_t pm = m < d.n ? list_place<LIST>(d, m) : 0xFFFFFFFFu;
            if (pm < h.n_places) {
                const uint32_t lo = off[pm], hi = off[pm + 1u];
                if ((uint64_t)lo <= r && r < (uint64_t)hi && hi <= n_list) {
                    p = pm;
                    is_first = r == (uint64_t)lo;
                    size = hi - lo;
                    const int ts = tree_step(q, m);
                    if (ts >= 0) {
                        is_case = true;
                        is_intro = ts == 0 || q.setting[m] != list_own<LIST>();
                        step = (uint32_t)ts;
                    }
                }
            }
        }
        const RunSums run = run_sums(p, is_case, is_intro, step);
        if (LIST != LIST_HOME && is_first) h.members[p] = size;
        if (run.head) {
            if (run.n_cases) atomicAdd(&h.cases[p], run.n_cases);
            if (run.n_intro) atomicAdd(&h.intro[p], run.n_intro);
            if (run.step != ESIM_NEVER) atomicMin(&h.first[p], run.step);
        }
    }
}

// The two tables of bins x bins over the places, a lane per place (HOME: a household is a building somebody lives in, its size
// from res_off; else a place is one with a member).  Almost every place falls into a few dozen cells: a workgroup counts in a
// table of its own in LDS (32 KB for the households, 8 KB else) and hands its non-zero counters to the global tables once, at
// the end; the caller caps the grid so that this stays small beside the walk.
template <bool HOME>
__global__ __launch_bounds__(TPB) void k_list_tables(Dev d, Place h)
{
    constexpr uint32_t BINS = HOME ? ESIM_HH_BINS : ESIM_PLACE_BINS, CELLS = BINS * BINS;
    __shared__ uint32_t tab[2u * CELLS];
    for (uint32_t k = threadIdx.x; k < 2u * CELLS; k += TPB) tab[k] = 0u;
    __syncthreads();
    for (uint64_t p = (uint64_t)blockIdx.x * TPB + threadIdx.x; p < (uint64_t)h.n_places; p += (uint64_t)gridDim.x * TPB) {
        uint32_t size;
        if (HOME) {
            const uint32_t lo = d.res_off[p], hi = d.res_off[p + 1u];
            if (lo >= hi || hi > d.n) continue;                           // (a building nobody lives in is no household)
            size = hi - lo;
        } else {
            size = h.members[p];
            if (!size) continue;                                          // (without a member it is no place)
        }
        const uint32_t row = list_bin<HOME>(size) * BINS;
        atomicAdd(&tab[row + list_bin<HOME>(h.cases[p])], 1u);
        atomicAdd(&tab[CELLS + row + list_bin<HOME>(h.intro[p])], 1u);
    }
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < 2u * CELLS; k += TPB) {
        const uint32_t v = tab[k];
        if (v) atomicAdd(k < CELLS ? &h.final_size[k] : &h.intro_size[k - CELLS], v);
    }
}

// The pairs (case j, housemate m at risk from j), a lane per entry of the log: one walk over j's household.  Counted are the
// cases the window counts (sar_counted_f).  All counters are 64 bits wide, on the device too: a cell holds up to cases x
// (household size - 1).  MODE: PAIRTAB_ONE_CELL, PAIRTAB_LDS (2 * n_cols^2 counters of dynamic LDS) or PAIRTAB_GLOBAL.
template <int MODE>
__global__ __launch_bounds__(TPB) void k_hh_sar(Dev d, Setting q, Tree t, SarWindow s, uint32_t log_len)
{
    extern __shared__ unsigned long long hh_pairs[];
    const uint32_t cells = s.n_cols * s.n_cols;
    if (MODE == PAIRTAB_LDS) pairtab_clear(hh_pairs, 2u * cells);
    unsigned long long n_at = 0ull, n_sec = 0ull;
    for (uint64_t i = (uint64_t)blockIdx.x * TPB + threadIdx.x; i < (uint64_t)log_len; i += (uint64_t)gridDim.x * TPB) {
        const uint32_t j = d.log[i];
        if (j >= d.n) continue;
        const uint32_t f = sar_counted_f(s, tree_step(q, j), d.exposed_time, q.t_done);
        if (!f) continue;                                                           // (not counted, or not infectious yet: no pairs)
        const uint32_t b = d.home[j];
        if (b >= d.n_bld) continue;
        const uint32_t lo = d.res_off[b], hi = d.res_off[b + 1u];
        if (lo > hi || hi > d.n) continue;
        uint32_t row = 0u;
        if (MODE != PAIRTAB_ONE_CELL) {
            const uint32_t gj = s.grp[j];
            if (gj >= s.n_cols) continue;
            row = gj * s.n_cols;
        }
        for (uint32_t r = lo; r < hi; ++r) {
            const uint32_t m = list_at<LIST_HOME>(d.res_idx, r);
            if (m >= d.n || m == j || f > hh_susceptible_end(d, q, m)) continue;
            const bool sec = t.infector[m] == j && q.setting[m] == ESIM_SETTING_HOUSEHOLD;
            if (MODE == PAIRTAB_ONE_CELL) { ++n_at; n_sec += sec ? 1ull : 0ull; continue; }
            const uint32_t gm = s.grp[m];
            if (gm >= s.n_cols) continue;
            pairtab_add<MODE>(hh_pairs, s.at_risk, row + gm, 1ull);
            if (sec) pairtab_add<MODE>(hh_pairs, s.at_risk, cells + row + gm, 1ull);
        }
    }
    if (MODE == PAIRTAB_ONE_CELL) {
        pairtab_wave_add(s.at_risk, n_at);
        pairtab_wave_add(s.secondary, n_sec);
    }
    if (MODE == PAIRTAB_LDS) pairtab_flush(hh_pairs, s.at_risk, 2u * cells);
}
