// esim_kernels_household.h -- household outbreaks: on top of the settings of esim_kernels_setting.h and the tree of
// esim_kernels_tree.h, the cases and introductions of every household, the final-size tables over all households, and the
// household secondary attack rate -- of the housemates still Susceptible when a case became infectious, the ones it infected at
// home.  k_hh_residents is a segmented reduction over the residents, a lane per resident; k_hh_tables bins the households, a
// lane per building and a table per workgroup in LDS; k_hh_sar walks the household of every case, a lane per log entry.
// Nothing here writes simulation state.
#pragma once

#define HH_CELLS ((uint32_t)ESIM_HH_BINS * ESIM_HH_BINS)           // counters of one final-size table
// k_hh_sar keeps its two pair tables in LDS while their 2 * n_cols^2 64-bit counters fit here (n_cols <= 45), a fifth of a
// compute unit's LDS, so that five workgroups still share one; beyond it every pair goes to the global tables.  (-DHH_LDS_BYTES=0u,
// the global form everywhere, was measured against it: DESIGN 19.)
#ifndef HH_LDS_BYTES
#define HH_LDS_BYTES 32768u
#endif
// Cases a lane of the LDS form walks at least before its workgroup hands over its table.  A walk is a chain of dependent loads,
// so the grid has to stay wide: 4 measured as fast as 1, 32 (an eighth of the workgroups) a quarter slower.
#ifndef HH_SAR_PER_LANE
#define HH_SAR_PER_LANE 4u
#endif

struct Household {
    uint32_t *cases, *intro, *first;     // [n_bld] zeroed, zeroed, filled with ESIM_NEVER by the caller
    uint32_t *final_size, *intro_size;   // [HH_CELLS] each, zeroed by the caller
};

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

// Per household: its cases, its introductions and the smallest cohort step among its cases.  A lane per entry r of the resident
// lists, which hold every citizen once, household after household: in the home-sorted layout r is the citizen itself, in any
// other res_idx[r].  The building comes from the citizen and is checked against the list it was found in (b < n_bld,
// res_off[b] <= r < res_off[b + 1] <= n).  Neighbouring lanes share a household: the lanes of a run are counted by its first
// lane (a ballot per count, k_area_census's way) and their steps reduced with six guarded shuffles, so a household costs three
// atomics per wavefront it touches, whether it has two residents or ten thousand.  Every lane of a wavefront makes the same trips.
__global__ __launch_bounds__(TPB) void k_hh_residents(Dev d, Setting q, Household h)
{
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t r0 = (uint64_t)blockIdx.x * TPB; r0 < (uint64_t)d.n; r0 += (uint64_t)gridDim.x * TPB) {
        const uint64_t r = r0 + threadIdx.x;
        uint32_t b = 0xFFFFFFFFu, step = ESIM_NEVER;
        bool is_case = false, is_intro = false;
        if (r < (uint64_t)d.n) {
            const uint32_t m = d.res_idx ? d.res_idx[r] : (uint32_t)r;
            const uint32_t hb = m < d.n ? d.home[m] : 0xFFFFFFFFu;
            if (hb < d.n_bld) {
                const uint32_t lo = d.res_off[hb], hi = d.res_off[hb + 1u];
                if ((uint64_t)lo <= r && r < (uint64_t)hi && hi <= d.n) {
                    b = hb;
                    const int ts = tree_step(q, m);
                    if (ts >= 0) {
                        is_case = true;
                        is_intro = ts == 0 || q.setting[m] != ESIM_SETTING_HOUSEHOLD;
                        step = (uint32_t)ts;
                    }
                }
            }
        }
        const uint32_t prev = __shfl_up(b, 1, 64);
        const bool head = b != 0xFFFFFFFFu && (lane == 0u || prev != b);
        const unsigned long long heads = __ballot(head);
        const unsigned long long above = lane == 63u ? 0ull : heads & (~0ull << (lane + 1u));
        const uint32_t next = above ? (uint32_t)__ffsll((long long)above) - 1u : 64u;            // the first lane of the next run
        const unsigned long long run = (next == 64u ? ~0ull : (1ull << next) - 1ull) & (~0ull << lane);
        const uint32_t n_cases = (uint32_t)__popcll(__ballot(is_case) & run), n_intro = (uint32_t)__popcll(__ballot(is_intro) & run);
#pragma unroll
        for (uint32_t o = 1u; o < 64u; o <<= 1) {                                                 // the smallest step from this lane to the end of its run
            const uint32_t v = __shfl_down(step, o, 64);
            if (lane + o < next && v < step) step = v;
        }
        if (head) {
            if (n_cases) atomicAdd(&h.cases[b], n_cases);
            if (n_intro) atomicAdd(&h.intro[b], n_intro);
            if (step != ESIM_NEVER) atomicMin(&h.first[b], step);
        }
    }
}

// The two tables of ESIM_HH_BINS x ESIM_HH_BINS bins over the households, a lane per building.  Almost every household falls
// into a few dozen cells: a workgroup counts in a table of its own in LDS (32 KB) and hands its non-zero counters to the global
// tables once, at the end; the caller caps the grid so that this stays small beside the walk.
__global__ __launch_bounds__(TPB) void k_hh_tables(Dev d, Household h)
{
    __shared__ uint32_t tab[2u * HH_CELLS];
    for (uint32_t k = threadIdx.x; k < 2u * HH_CELLS; k += TPB) tab[k] = 0u;
    __syncthreads();
    for (uint64_t b = (uint64_t)blockIdx.x * TPB + threadIdx.x; b < (uint64_t)d.n_bld; b += (uint64_t)gridDim.x * TPB) {
        const uint32_t lo = d.res_off[b], hi = d.res_off[b + 1u];
        if (lo >= hi || hi > d.n) continue;                               // (a building nobody lives in is no household)
        const uint32_t size = hi - lo, n_cases = h.cases[b], n_intro = h.intro[b], top = ESIM_HH_BINS - 1u;
        const uint32_t row = (size < top ? size : top) * ESIM_HH_BINS;
        atomicAdd(&tab[row + (n_cases < top ? n_cases : top)], 1u);
        atomicAdd(&tab[HH_CELLS + row + (n_intro < top ? n_intro : top)], 1u);
    }
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < 2u * HH_CELLS; k += TPB) {
        const uint32_t v = tab[k];
        if (v) atomicAdd(k < HH_CELLS ? &h.final_size[k] : &h.intro_size[k - HH_CELLS], v);
    }
}

struct HouseholdSar {
    uint32_t first, last;                    // cohort steps of the cases counted
    uint32_t n_cols;                         // 1, or the number of groups
    const uint16_t *grp;                     // [n] labels, or nullptr for one cell
    unsigned long long *at_risk, *secondary; // [n_cols * n_cols] each, zeroed by the caller
};

enum { HH_ONE_CELL = 0, HH_LDS = 1, HH_GLOBAL = 2 };

// The pairs (case j, housemate m at risk from j), a lane per entry of the log: one walk over j's household.  Counted are the
// cases of cohort steps [first, last] that have become infectious by the last step run.  All counters are 64 bits wide, on the
// device too: a cell holds up to cases x (household size - 1).
//   HH_ONE_CELL  a lane sums its pairs in registers, a wavefront adds its 64 sums up and issues one atomic pair at the end;
//   HH_LDS       cell [group of j][group of m] of a table of the workgroup's own in LDS (2 * n_cols^2 counters of dynamic LDS),
//                handed to the global tables once, at the end, non-zero counters only;
//   HH_GLOBAL    the same cell of the global tables directly, where the workgroup's table would not fit HH_LDS_BYTES.
template <int MODE>
__global__ __launch_bounds__(TPB) void k_hh_sar(Dev d, Setting q, Tree t, HouseholdSar s, uint32_t log_len)
{
    extern __shared__ unsigned long long hh_pairs[];
    const uint32_t cells = s.n_cols * s.n_cols;
    if (MODE == HH_LDS) {
        for (uint32_t k = threadIdx.x; k < 2u * cells; k += TPB) hh_pairs[k] = 0ull;
        __syncthreads();
    }
    unsigned long long n_at = 0ull, n_sec = 0ull;
    for (uint64_t i = (uint64_t)blockIdx.x * TPB + threadIdx.x; i < (uint64_t)log_len; i += (uint64_t)gridDim.x * TPB) {
        const uint32_t j = d.log[i];
        if (j >= d.n) continue;
        const int ts = tree_step(q, j);
        if (ts < (int)s.first || ts > (int)s.last) continue;
        const uint32_t f = ts == 0 ? 1u : (uint32_t)ts + d.exposed_time + 1u;       // the first infectious step
        if (f > q.t_done) continue;                                                 // (not infectious yet: no pairs)
        const uint32_t b = d.home[j];
        if (b >= d.n_bld) continue;
        const uint32_t lo = d.res_off[b], hi = d.res_off[b + 1u];
        if (lo > hi || hi > d.n) continue;
        uint32_t row = 0u;
        if (MODE != HH_ONE_CELL) {
            const uint32_t gj = s.grp[j];
            if (gj >= s.n_cols) continue;
            row = gj * s.n_cols;
        }
        for (uint32_t r = lo; r < hi; ++r) {
            const uint32_t m = d.res_idx ? d.res_idx[r] : r;
            if (m >= d.n || m == j || f > hh_susceptible_end(d, q, m)) continue;
            const bool sec = t.infector[m] == j && q.setting[m] == ESIM_SETTING_HOUSEHOLD;
            if (MODE == HH_ONE_CELL) { ++n_at; n_sec += sec ? 1ull : 0ull; continue; }
            const uint32_t gm = s.grp[m];
            if (gm >= s.n_cols) continue;
            if (MODE == HH_LDS) {
                atomicAdd(&hh_pairs[row + gm], 1ull);
                if (sec) atomicAdd(&hh_pairs[cells + row + gm], 1ull);
            } else {
                atomicAdd(&s.at_risk[row + gm], 1ull);
                if (sec) atomicAdd(&s.secondary[row + gm], 1ull);
            }
        }
    }
    if (MODE == HH_ONE_CELL) {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            n_at += __shfl_xor(n_at, o, 64);
            n_sec += __shfl_xor(n_sec, o, 64);
        }
        if ((threadIdx.x & 63u) == 0u) {
            if (n_at) atomicAdd(s.at_risk, n_at);
            if (n_sec) atomicAdd(s.secondary, n_sec);
        }
    }
    if (MODE == HH_LDS) {
        __syncthreads();
        for (uint32_t k = threadIdx.x; k < 2u * cells; k += TPB) {
            const unsigned long long v = hh_pairs[k];
            if (v) atomicAdd(k < cells ? &s.at_risk[k] : &s.secondary[k - cells], v);
        }
    }
}
