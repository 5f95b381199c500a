// esim_kernels_restart.h -- ensembles on one uploaded population: the initial state rebuilt on the device (esim_restart)
// and the per-Output-Area accumulators over the members of an ensemble (esim_ensemble_fold), by census or by arrival step.
// No stepping kernel is here.
#pragma once

// Every citizen back to Susceptible: the static flags are all of the word that survives.  A pure stream over 4 B per
// citizen, read and written once: 16 bytes per lane, a grid capped at 2048 workgroups that strides over the rest (the
// array comes from hipMalloc, so it starts on a 16-byte boundary); the up to three words behind the last whole uint4
// are written by the first lanes of workgroup 0.
__global__ __launch_bounds__(TPB) void k_restart_words(uint32_t *cit, uint32_t n)
{
    const uint32_t sus = TE_SUSCEPTIBLE << CW_TE_SHIFT;
    uint4 *v = reinterpret_cast<uint4 *>(cit);
    const uint32_t n4 = n >> 2, stride = gridDim.x * TPB;
    for (uint32_t i = blockIdx.x * TPB + threadIdx.x; i < n4; i += stride) {
        uint4 w = v[i];
        w.x = sus | (w.x & CW_FLAGS); w.y = sus | (w.y & CW_FLAGS); w.z = sus | (w.z & CW_FLAGS); w.w = sus | (w.w & CW_FLAGS);
        v[i] = w;
    }
    const uint32_t tail = (n4 << 2) + threadIdx.x;
    if (blockIdx.x == 0 && threadIdx.x < (n & 3u)) cit[tail] = sus | (cit[tail] & CW_FLAGS);
}

// After k_restart_words: the distinct seeds are Infected(0) before step 1, i.e. "exposed" at step -(exposed_time + 1);
// the census histogram and the log offsets are step functions of their index (all seeds sit in slot seed_te).
__global__ __launch_bounds__(TPB) void k_restart_books(uint32_t *cit, uint32_t n, const uint32_t *seeds, uint32_t n_seeds, uint32_t seed_te,
                                                       uint32_t *hist, uint32_t *log_off)
{
    const uint32_t i = blockIdx.x * TPB + threadIdx.x;
    if (i < TE_SLOTS) hist[i] = i == seed_te ? n_seeds : 0u;
    if (i <= TE_SLOTS) log_off[i] = i > seed_te ? n_seeds : 0u;
    if (i < n_seeds) {
        const uint32_t sc = seeds[i];
        if (sc < n) cit[sc] = CW_MAKE(seed_te, cit[sc] & CW_FLAGS);
    }
}

// One member of an ensemble folded into the per-area accumulators.  counts[area * 5 + status] is what k_area_census has
// just counted; x = the citizens of the area whose status is in `mask`.  A lane owns an area: plain loads and stores.
__global__ __launch_bounds__(TPB) void k_ensemble_fold(const uint32_t *counts, uint32_t n_areas, uint32_t mask, uint32_t min_cases,
                                                       uint32_t *hit, unsigned long long *sum, unsigned long long *sumsq, uint32_t *members)
{
    const uint32_t a = blockIdx.x * TPB + threadIdx.x;
    if (a == 0u) *members += 1u;
    if (a >= n_areas) return;
    uint32_t x = 0u;
#pragma unroll
    for (uint32_t s = 0; s < 5u; ++s) if ((mask >> s) & 1u) x += counts[(size_t)a * 5u + s];
    if (x >= min_cases) hit[a] += 1u;
    sum[a] += x;
    sumsq[a] += (unsigned long long)x * x;
}

// The same for accumulators begun with esim_ensemble_begin_arrival: x = the step at which the member's epidemic first
// reached the entry (k_area_arrival has just filled `first`), counted only where it did so by the horizon.
__global__ __launch_bounds__(TPB) void k_ensemble_fold_arrival(const uint32_t *first, uint32_t n, uint32_t horizon,
                                                               uint32_t *hit, unsigned long long *sum, unsigned long long *sumsq, uint32_t *members)
{
    const uint32_t a = blockIdx.x * TPB + threadIdx.x;
    if (a == 0u) *members += 1u;
    if (a >= n) return;
    const uint32_t x = first[a];
    if (x == ESIM_NEVER || x > horizon) return;
    hit[a] += 1u;
    sum[a] += x;
    sumsq[a] += (unsigned long long)x * x;
}
