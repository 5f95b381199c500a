// esim_kernels_pairtab.h -- what the household, place and contact outputs share: a group-by-group table
// of 64-bit counters in its three counting modes, the window of the secondary attack rates with its rule for a counted case, and
// the reduction over the runs of a member list.  Needs esim_kernels_common.h only; nothing here writes simulation state.
#pragma once

// The three ways a kernel counts into cell [row group][column group] of a table of n_cols x n_cols 64-bit counters:
//   PAIRTAB_ONE_CELL  n_cols = 1: a lane sums in registers over its whole loop, a wavefront adds its 64 sums up and issues
//                     one atomic per table at the end (pairtab_wave_add);
//   PAIRTAB_LDS       a table of the workgroup's own in dynamic LDS (pairtab_clear), handed to the global table once, at the end,
//                     non-zero counters only (pairtab_flush);
//   PAIRTAB_GLOBAL    the same cell of the global table directly, where the workgroup's tables would not fit PAIRTAB_LDS_BYTES.
enum { PAIRTAB_ONE_CELL = 0, PAIRTAB_LDS = 1, PAIRTAB_GLOBAL = 2 };

// All tables of a kernel stay in LDS while their 64-bit counters fit here (two tables: n_cols <= 45; the four planes of the
// contact-hours: n_cols <= 32): 32 KB is a fifth of a compute unit's LDS, so that five workgroups still share one; beyond it
// every pair goes to the global tables.  (-DPAIRTAB_LDS_BYTES=0u, the global form everywhere, was measured against it: DESIGN 19.)
#ifndef PAIRTAB_LDS_BYTES
#define PAIRTAB_LDS_BYTES 32768u
#endif

// The mode of a call: `where` is ESIM_BY_ALL or ESIM_BY_GROUP, `bytes` what all tables of a workgroup take together.
static inline int pairtab_mode(int where, size_t bytes) { return where == ESIM_BY_ALL ? PAIRTAB_ONE_CELL : bytes <= PAIRTAB_LDS_BYTES ? PAIRTAB_LDS : PAIRTAB_GLOBAL; }

// The table of n counters of a workgroup of TPB cleared; every lane of the workgroup comes here.
__device__ __forceinline__ void pairtab_clear(unsigned long long *lds, uint32_t n)
{
    for (uint32_t k = threadIdx.x; k < n; k += TPB) lds[k] = 0ull;
    __syncthreads();
}

// cnt more at `cell` of the workgroup's table (PAIRTAB_LDS) or of the global one, which have the same layout.
template <int MODE>
__device__ __forceinline__ void pairtab_add(unsigned long long *lds, unsigned long long *global, uint32_t cell, unsigned long long cnt)
{
    if (MODE == PAIRTAB_LDS) atomicAdd(&lds[cell], cnt);
    else atomicAdd(&global[cell], cnt);
}

// The sum of v over the 64 lanes, in every lane.
__device__ __forceinline__ unsigned long long pairtab_wave_sum(unsigned long long v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// PAIRTAB_ONE_CELL's end: the lanes' sums of a wavefront added up and to *cell, one atomic where there is something to add.
__device__ __forceinline__ void pairtab_wave_add(unsigned long long *cell, unsigned long long v)
{
    v = pairtab_wave_sum(v);
    if ((threadIdx.x & 63u) == 0u && v) atomicAdd(cell, v);
}

// The workgroup's table of n counters handed to the global one, non-zero counters only; every lane of the workgroup comes here.
__device__ __forceinline__ void pairtab_flush(const unsigned long long *lds, unsigned long long *global, uint32_t n)
{
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < n; k += TPB) {
        const unsigned long long v = lds[k];
        if (v) atomicAdd(&global[k], v);
    }
}

// The window of a secondary attack rate (esim_household_sar, esim_place_sar) and its two tables.  The tables are ONE block of
// 2 * n_cols^2 counters, secondary == at_risk + n_cols^2: a cell of `secondary` is cell n_cols^2 + ... of `at_risk`, in LDS
// and in global memory alike, and one pairtab_flush hands both over.
struct SarWindow {
    uint32_t first, last;                    // cohort steps of the cases counted
    uint32_t n_cols;                         // 1, or the number of groups
    const uint16_t *grp;                     // [n] labels, or nullptr for one cell
    unsigned long long *at_risk, *secondary; // [n_cols * n_cols] each, adjacent, zeroed by the caller
};

// The first infectious step of a citizen of cohort step ts (tree_step: 0 an index case, -1 no case) where it is a case the
// window counts -- cohort step in [first, last], infectious by the last step run, t_done -- else 0: no case has f = 0.
__device__ __forceinline__ uint32_t sar_counted_f(const SarWindow &s, int ts, uint32_t exposed_time, uint32_t t_done)
{
    if (ts < (int)s.first || ts > (int)s.last) return 0u;
    const uint32_t f = ts == 0 ? 1u : (uint32_t)ts + exposed_time + 1u;
    return f <= t_done ? f : 0u;
}

// The runs of equal keys among the 64 lanes of a wavefront (a member list, a lane per entry, the key the entry's household or
// place; 0xFFFFFFFF: no entry, part of no run).  `head`: this lane is the first of its run; then n_cases and n_intro count the
// lanes of the run with the flag set and `step` is the smallest step among them -- in every lane, from the lane to the end of
// its run.  A ballot per count (k_area_census's way) and six guarded shuffles: a run costs its head three atomics, whether it
// has two lanes or 64.  Every lane of the wavefront comes here.
struct RunSums { bool head; uint32_t n_cases, n_intro, step; };
__device__ __forceinline__ RunSums run_sums(uint32_t key, bool is_case, bool is_intro, uint32_t step)
{
    const uint32_t lane = threadIdx.x & 63u, prev = __shfl_up(key, 1, 64);
    RunSums r;
    r.head = key != 0xFFFFFFFFu && (lane == 0u || prev != key);
    const unsigned long long heads = __ballot(r.head);
    const unsigned long long above = lane == 63u ? 0ull : heads & (~0ull << (lane + 1u));
    const uint32_t next = above ? (uint32_t)__ffsll((long long)above) - 1u : 64u;            // the first lane of the next run
    const unsigned long long run = (next == 64u ? ~0ull : (1ull << next) - 1ull) & (~0ull << lane);
    r.n_cases = (uint32_t)__popcll(__ballot(is_case) & run);
    r.n_intro = (uint32_t)__popcll(__ballot(is_intro) & run);
#pragma unroll
    for (uint32_t o = 1u; o < 64u; o <<= 1) {                                                 // the smallest step from this lane to the end of its run
        const uint32_t v = __shfl_down(step, o, 64);
        if (lane + o < next && v < step) step = v;
    }
    r.step = step;
    return r;
}
