// esim_kernels_members.h -- what esim_ensemble_keep_members puts around esim_members.h: a member's value per cell
// written into its slot of the store, for the kinds whose fold does not leave that value in a plane (the series and the settings
// kind do: their slot is a copy of plane 0).  A lane owns its cells and every kernel loops with a grid stride.  Nothing here
// writes simulation state or an accumulator.  esim_depth.h, the ranking of the kept members as whole curves, reads
// the same store and comes in here beside it, and so do esim_dist.h, the members compared pair by pair, and
// esim_arms.h, the members read as replicates of policy arms.
#pragma once
#include "esim_curves.h"
#include "esim_members.h"
#include "esim_depth.h"
#include "esim_dist.h"
#include "esim_arms.h"

// esim_ensemble_begin: what k_ensemble_fold adds to `sum`, the citizens of the area or group whose status is in `mask`.
__global__ __launch_bounds__(TPB) void k_members_keep_census(const uint32_t *counts, uint32_t n, uint32_t mask, uint32_t *slot)
{
    for (uint32_t a = blockIdx.x * TPB + threadIdx.x; a < n; a += gridDim.x * TPB) {
        uint32_t x = 0u;
#pragma unroll
        for (uint32_t s = 0; s < 5u; ++s) if ((mask >> s) & 1u) x += counts[(size_t)a * 5u + s];
        slot[a] = x;
    }
}

// esim_ensemble_begin_arrival: the arrival step, ESIM_NEVER where k_ensemble_fold_arrival counts nothing.
__global__ __launch_bounds__(TPB) void k_members_keep_arrival(const uint32_t *first, uint32_t n, uint32_t horizon, uint32_t *slot)
{
    for (uint32_t a = blockIdx.x * TPB + threadIdx.x; a < n; a += gridDim.x * TPB) {
        const uint32_t x = first[a];
        slot[a] = x > horizon ? ESIM_NEVER : x;
    }
}

// esim_ensemble_begin_paired: baseline - current as a signed number, stored as a key (members_key).
__global__ __launch_bounds__(TPB) void k_members_keep_paired(const uint32_t *b, const uint32_t *c, uint64_t cells, uint32_t *slot)
{
    for (uint64_t i = (uint64_t)blockIdx.x * TPB + threadIdx.x; i < cells; i += (uint64_t)gridDim.x * TPB)
        slot[i] = members_key((int32_t)(b[i] - c[i]));
}

// esim_ensemble_begin_peaks: one of the three values of the member's summary, decoded as esim_curve_summary decodes the tables.
__global__ __launch_bounds__(TPB) void k_members_keep_peaks(CurveTabs t, uint32_t n_cols, int what, uint32_t *slot)
{
    for (uint32_t col = blockIdx.x * TPB + threadIdx.x; col < n_cols; col += gridDim.x * TPB) {
        const unsigned long long best = t.best[col];
        const uint32_t peak = (uint32_t)(best >> 32);
        slot[col] = what == ESIM_KEEP_PEAK_STEP ? (peak ? ~(uint32_t)best : ESIM_NEVER) : what == ESIM_KEEP_DURATION ? t.steps[col] : peak;
    }
}
