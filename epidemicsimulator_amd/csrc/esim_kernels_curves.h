// esim_kernels_curves.h -- what esim_curve_summary and the peaks kind of the ensemble accumulators put around esim_curves.h
// (DESIGN 26): the change points of the curves from the exposure log into the pair table, and one member's summary folded into
// the accumulators.  Nothing here writes simulation state.
#pragma once
#include "esim_pairs.h"
#include "esim_curves.h"

#define CURVE_BY_ALL 0xFFu          // Series::key of the one-column curve, beside KEY_GROUP and KEY_HOME

// A lane per exposure-log entry, as k_series_log walks it: the steps [p, e] after which the citizen's status is in `mask` (Exposed,
// Infected or both: one interval per case) from status_interval, cut at the step before the one that vaccinated it and clipped
// to [q.first, last]; +1 under (column, p), and -1 under (column, e + 1) where that step is still inside.  q: first, t_done, t_all,
// vax_of, n_cols, key and grp are read.  The one column of CURVE_BY_ALL takes every entry of the log, as the groups together do: a
// citizen whose household's area the tables do not hold is counted by all and by group, and by no area.
__global__ __launch_bounds__(TPB) void k_curve_events(Dev d, Series q, uint32_t mask, uint32_t last, uint32_t log_len, PairTable t)
{
    const uint32_t lo = (mask >> ESIM_EXPOSED) & 1u ? ESIM_EXPOSED : ESIM_INFECTED, hi = (mask >> ESIM_INFECTED) & 1u ? ESIM_INFECTED : ESIM_EXPOSED;
    for (uint32_t i = blockIdx.x * TPB + threadIdx.x; i < log_len; i += gridDim.x * TPB) {
        const uint32_t c = d.log[i];
        if (c >= d.n) continue;
        const uint32_t w = d.cit[c];
        uint32_t col = 0u, other;
        if (q.key != CURVE_BY_ALL && !series_cols(d, q, c, w, &col, &other)) continue;
        const int ts = (int)log_te(d, i, q.t_done + TE_BIAS) - (int)TE_BIAS;   // exposure step; seeds: -(exposed_time + 1)
        int p, e, unused;
        status_interval(lo, ts, d.exposed_time, d.infected_time, &p, &unused);
        status_interval(hi, ts, d.exposed_time, d.infected_time, &unused, &e);
        if (CW_TE(w) == TE_VACCINATED) {
            const uint32_t v = vax_step(q, c);
            if (v != 0xFFFFFFFFu && (int)v - 1 < e) e = (int)v - 1;
        }
        if (e > (int)last) e = (int)last;
        if (p < (int)q.first) p = (int)q.first;
        if (p > e) continue;
        const uint64_t base = (uint64_t)col << 32;
        pair_add(t, base | (uint32_t)p, 1u);
        if ((uint32_t)e + 1u <= last) pair_add(t, base | ((uint32_t)e + 1u), 0xFFFFFFFFu);
    }
}

// The accumulators of esim_ensemble_begin_peaks, [n_cols] each but the member counter: 56 B per column.
struct PeakAcc {
    uint32_t *defined, *hit, *members;
    unsigned long long *sum_peak, *sq_peak, *sum_step, *sq_step, *sum_dur, *sq_dur;
};

// One member's tables, as k_curve_reduce has just left them, into the accumulators: a lane per column, which it owns.
__global__ __launch_bounds__(TPB) void k_ensemble_fold_peaks(CurveTabs t, uint32_t n_cols, uint32_t min_peak, PeakAcc a)
{
    if (blockIdx.x == 0u && threadIdx.x == 0u) *a.members += 1u;
    for (uint32_t col = blockIdx.x * TPB + threadIdx.x; col < n_cols; col += gridDim.x * TPB) {
        const unsigned long long best = t.best[col];
        const uint32_t peak = (uint32_t)(best >> 32), step = ~(uint32_t)best, dur = t.steps[col];
        if (!peak) continue;                                      // (no peak: no step at or above a threshold >= 1 either)
        a.defined[col] += 1u;
        if (peak >= min_peak) a.hit[col] += 1u;
        a.sum_peak[col] += peak; a.sq_peak[col] += (unsigned long long)peak * peak;
        a.sum_step[col] += step; a.sq_step[col] += (unsigned long long)step * step;
        if (dur) { a.sum_dur[col] += dur; a.sq_dur[col] += (unsigned long long)dur * dur; }
    }
}
