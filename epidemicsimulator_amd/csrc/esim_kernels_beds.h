// esim_kernels_beds.h -- a run's admitted cases as a list on the device: one entry (citizen, admit_step, end_step |
// died << 31) for every log entry that burden_outcome (esim_kernels_burden.h, as it is) calls an admitted case.  k_beds_collect
// makes the list; the two consumers -- rows for the series engine's prefix sum, totals over a window -- walk it and use no
// Philox, stage no tables and replay no vaccinations, so that a list outlives the run it was taken from.  The order of a list is
// whatever the atomics made it: every consumer is an integer sum over its entries.  Nothing here writes simulation state.
#pragma once
#include "esim_kernels_burden.h"

#define BEDS_DIED 0x80000000u        // bit 31 of an entry's end word (end_step <= 7600 + 2 * 65535 * 64 < 2^31)
#define BEDS_LDS_CELLS 4096u         // k_beds_rows builds its rows in LDS up to this many cells (16 KB)

// Three planes of `cap` entries in one allocation, and n[0] = the entries, n[1] = the deaths among them.
struct BedsList { uint32_t *cit, *admit, *end, *n; uint32_t cap; };

static_assert(sizeof(Dev) + sizeof(Series) + sizeof(Burden) + sizeof(BedsList) + 64u <= 4096u, "the arguments of k_beds_collect must fit a kernel's argument segment");

// A lane per log entry, every lane of a workgroup making the same trips.  The admitted cases of a trip take their places in the
// list with ONE value-returning atomic per workgroup: every wavefront's ballot count goes to LDS, the first lane adds their sum
// to the list's count, and a case's place is that base, the counts of the wavefronts in front and its rank in its own ballot --
// every wavefront of every trip adding to the one count for itself made that address the kernel's critical path.  The counts in
// LDS alternate between two sets by trip, so that two barriers a trip are enough.  The deaths are counted per wavefront over
// all its trips and added once.
__global__ __launch_bounds__(TPB) void k_beds_collect(Dev d, Series q, Burden b, uint32_t log_len, BedsList l)
{
    __shared__ BurdenLds s;
    __shared__ uint32_t s_wave[2][TPB / 64u], s_base[2];
    burden_stage(b, &s);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t n_dead = 0u, set = 0u;
    for (uint64_t i0 = (uint64_t)blockIdx.x * TPB; i0 < (uint64_t)log_len; i0 += (uint64_t)gridDim.x * TPB, set ^= 1u) {
        const uint64_t i = i0 + threadIdx.x;
        const uint32_t c = i < (uint64_t)log_len ? d.log[i] : 0xFFFFFFFFu;
        BurdenOutcome o = BurdenOutcome();
        const bool in = c < d.n && burden_outcome(d, q, b, &s, (uint32_t)i, c, d.cit[c], &o) && o.admitted;
        const unsigned long long all = __ballot(in);
        n_dead += (uint32_t)__popcll(__ballot(in && o.died));
        if (lane == 0u) s_wave[set][wave] = (uint32_t)__popcll(all);
        __syncthreads();
        if (threadIdx.x == 0u) {
            uint32_t sum = 0u;
            for (uint32_t w = 0u; w < TPB / 64u; ++w) sum += s_wave[set][w];
            s_base[set] = sum ? atomicAdd(&l.n[0], sum) : 0u;
        }
        __syncthreads();
        uint32_t at = s_base[set] + (uint32_t)__popcll(all & ((1ull << lane) - 1ull));
        for (uint32_t w = 0u; w < wave; ++w) at += s_wave[set][w];
        if (!in || at >= l.cap) continue;                             // (cap = log_len: never reached)
        l.cit[at] = c; l.admit[at] = o.admit_step; l.end[at] = o.end_step | (o.died ? BEDS_DIED : 0u);
    }
    if (lane == 0u && n_dead) atomicAdd(&l.n[1], n_dead);
}

// tab[cell] += 1 for the valid lanes: burden_count where a cell fits its 32-bit key, a plain atomic beyond that.
__device__ __forceinline__ void beds_event(uint32_t *tab, uint64_t cell, bool valid, bool keyed, uint32_t lane)
{
    if (keyed) burden_count(tab, (uint32_t)cell, valid, lane);
    else if (valid) atomicAdd(&tab[cell], 1u);
}

// The rows of k_burden_rows from a list, under the same conventions and clipping (q.t_done: the steps of the run the list was
// taken from; q.p0 zeroed by the caller).  With at most BEDS_LDS_CELLS cells the rows are built in the workgroup's LDS and added
// to q.p0 at the end; with more, events by one atomic per wavefront and cell and the difference rows of the occupancy by
// rows_add as they are -- that many cells spread the adds.  Every lane of a workgroup makes the same trips.
__global__ __launch_bounds__(TPB) void k_beds_rows(Dev d, Series q, BedsList l, uint32_t what)
{
    __shared__ uint32_t s_rows[BEDS_LDS_CELLS];
    const uint32_t n = l.n[0] < l.cap ? l.n[0] : l.cap, lane = threadIdx.x & 63u;
    if ((uint64_t)blockIdx.x * TPB >= (uint64_t)n) return;            // (uniform: a workgroup without an entry)
    const uint64_t cells = (uint64_t)q.n_rows * q.n_cols;
    const bool local = cells <= (uint64_t)BEDS_LDS_CELLS, keyed = cells <= 0xFFFFFFFFull;
    Series ql = q;
    if (local) {
        for (uint32_t j = threadIdx.x; j < (uint32_t)cells; j += TPB) s_rows[j] = 0u;
        __syncthreads();
        ql.p0 = s_rows;
    }
    for (uint64_t i0 = (uint64_t)blockIdx.x * TPB; i0 < (uint64_t)n; i0 += (uint64_t)gridDim.x * TPB) {
        const uint64_t i = i0 + threadIdx.x;
        const uint32_t c = i < (uint64_t)n ? l.cit[i] : 0xFFFFFFFFu;
        uint32_t col = 0u;
        const bool in = c < d.n && burden_col(d, q, c, d.cit[c], &col);
        const uint32_t admit = in ? l.admit[i] : 0u, word = in ? l.end[i] : 0u, end = word & ~BEDS_DIED;
        if (what == BURDEN_OCCUPANCY) {
            int p = (int)admit, e = (int)(end - 1u);
            if (in && clip(q, &p, &e)) rows_add(ql, (uint32_t)p, (uint32_t)e, col, col);
            continue;                                                 // (uniform: `what` is the launch's)
        }
        const uint32_t step = what == BURDEN_DEATHS ? end : admit;
        const bool hit = in && (what != BURDEN_DEATHS || (word & BEDS_DIED)) && step >= q.first && step <= q.t_done;
        const uint64_t row = hit ? (uint64_t)(step - q.first) / q.stride : 0u;
        const bool add = hit && row < q.n_rows;
        const uint64_t cell = add ? row * q.n_cols + col : 0u;
        if (local) { if (add) atomicAdd(&s_rows[cell], 1u); }
        else beds_event(q.p0, cell, add, keyed, lane);
    }
    if (!local) return;                                               // (uniform)
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < (uint32_t)cells; j += TPB) {
        const uint32_t v = s_rows[j];
        if (v) atomicAdd(&q.p0[j], v);                                // (a difference row's -1 is 0xFFFFFFFF: the sum wraps as it must)
    }
}

// Per column over the window [first, last], last inside the run the list was taken from: bed_steps += |[admit_step,
// end_step - 1] cut to the window|, admissions += 1 with admit_step inside, deaths += 1 for a death with end_step inside --
// the three numbers of k_burden_events and the curve's sum.  With at most BURDEN_LDS_COLS columns in tables of the workgroup's
// LDS that are added to the global ones at the end; with more, the two counts by one atomic per wavefront and column and the
// bed-steps by a 64-bit atomic per entry.  q: key, grp and n_cols are read.
__global__ __launch_bounds__(TPB) void k_beds_totals(Dev d, Series q, BedsList l, uint32_t first, uint32_t last, unsigned long long *bed_steps, uint32_t *admissions,
                                                    uint32_t *deaths)
{
    __shared__ unsigned long long s_bed[BURDEN_LDS_COLS];
    __shared__ uint32_t s_cnt[2u * BURDEN_LDS_COLS];
    const uint32_t n = l.n[0] < l.cap ? l.n[0] : l.cap, lane = threadIdx.x & 63u;
    if ((uint64_t)blockIdx.x * TPB >= (uint64_t)n) return;            // (uniform: a workgroup without an entry)
    const bool local = q.n_cols <= BURDEN_LDS_COLS;
    if (local) {
        for (uint32_t j = threadIdx.x; j < q.n_cols; j += TPB) { s_bed[j] = 0ull; s_cnt[j] = 0u; s_cnt[q.n_cols + j] = 0u; }
        __syncthreads();
    }
    for (uint64_t i0 = (uint64_t)blockIdx.x * TPB; i0 < (uint64_t)n; i0 += (uint64_t)gridDim.x * TPB) {
        const uint64_t i = i0 + threadIdx.x;
        const uint32_t c = i < (uint64_t)n ? l.cit[i] : 0xFFFFFFFFu;
        uint32_t col = 0u;
        const bool in = c < d.n && burden_col(d, q, c, d.cit[c], &col);
        const uint32_t admit = in ? l.admit[i] : 0u, word = in ? l.end[i] : 1u, end = word & ~BEDS_DIED;
        const bool adm = in && admit >= first && admit <= last, dth = in && (word & BEDS_DIED) && end >= first && end <= last;
        const uint32_t p = admit < first ? first : admit, e = end - 1u > last ? last : end - 1u;      // (end_step >= admit_step + 1)
        const uint32_t beds = in && p <= e ? e - p + 1u : 0u;
        if (local) {
            if (beds) atomicAdd(&s_bed[col], (unsigned long long)beds);
            if (adm) atomicAdd(&s_cnt[col], 1u);
            if (dth) atomicAdd(&s_cnt[q.n_cols + col], 1u);
        } else {
            if (beds) atomicAdd(&bed_steps[col], (unsigned long long)beds);
            burden_count(admissions, col, adm, lane);
            burden_count(deaths, col, dth, lane);
        }
    }
    if (!local) return;                                               // (uniform)
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < q.n_cols; j += TPB) {
        if (s_bed[j]) atomicAdd(&bed_steps[j], s_bed[j]);
        if (s_cnt[j]) atomicAdd(&admissions[j], s_cnt[j]);
        if (s_cnt[q.n_cols + j]) atomicAdd(&deaths[j], s_cnt[q.n_cols + j]);
    }
}
