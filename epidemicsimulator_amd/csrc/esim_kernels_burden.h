// esim_kernels_burden.h -- hospital burden laid over a finished run: one Philox block per case, a pure function of
// (seed, citizen, onset step), decides whether the case is admitted, when, for how long, and whether it dies (the contract:
// include/esim.h).  A lane per exposure-log entry, as k_series_log and k_curve_events walk the log; the thresholds per group and
// the two CDFs are staged in LDS once per workgroup.  Three consumers: per-citizen outcomes, rows for the series engine's prefix
// sum, change points for the pair table of the curve summary.  Nothing here writes simulation state.
#pragma once
#include "esim_kernels_curves.h"

#define BURDEN_BINS 64u              // ESIM_BURDEN_BINS
#define BURDEN_GROUPS 1024u          // ESIM_MAX_GROUPS
#define BURDEN_LDS_COLS 64u          // k_burden_events counts admissions and deaths in LDS up to this many columns
enum { BURDEN_ADMISSIONS = 0, BURDEN_OCCUPANCY = 1, BURDEN_DEATHS = 2 };   // ESIM_BURDEN_*

// The tables in force, on the device: tab = admit_thr [n_groups], death_thr [n_groups], delay_cdf [BURDEN_BINS], stay_cdf [BURDEN_BINS].
struct Burden {
    const uint32_t *tab;
    uint32_t n_groups, n_delay, n_stay, delay_unit, stay_unit;
    const uint16_t *grp;             // [n] labels, or nullptr with one group
    uint32_t seam_step;              // a rollback under another seed: onsets up to this step draw under the old seed (0: no seam)
    uint32_t old_seed_lo, old_seed_hi;
};

static_assert(sizeof(Dev) + sizeof(Series) + sizeof(Burden) + sizeof(PairTable) + 64u <= 4096u, "the arguments of k_burden_events must fit a kernel's argument segment");

// The tables in LDS: 8 KB of thresholds and 512 B of CDFs.
struct BurdenLds { uint32_t thr[2u * BURDEN_GROUPS], cdf[2u * BURDEN_BINS]; };

// Every lane of the workgroup, once, in front of the kernel's loop.
__device__ __forceinline__ void burden_stage(const Burden &b, BurdenLds *s)
{
    const uint32_t g = b.n_groups < BURDEN_GROUPS ? b.n_groups : BURDEN_GROUPS;
    for (uint32_t i = threadIdx.x; i < 2u * g; i += blockDim.x) s->thr[i] = b.tab[i];
    for (uint32_t i = threadIdx.x; i < 2u * BURDEN_BINS; i += blockDim.x) s->cdf[i] = b.tab[2u * b.n_groups + i];
    __syncthreads();
}

// A case's outcome: admitted or not; the steps are meaningful where it is.
struct BurdenOutcome { bool admitted, died; uint32_t onset, admit_step, end_step; };

// The outcome of log entry i (citizen c, word w), false where the entry is no case: its onset lies beyond the steps run, or the
// citizen was vaccinated while Exposed.  The raw block of (global id, onset, ESIM_SLOT_BURDEN, 0) and the two table counts --
// branch-free loops over LDS: a CDF indexed dynamically in registers would live on the stack.  q: t_done, t_all and vax_of are read.
__device__ __forceinline__ bool burden_outcome(const Dev &d, const Series &q, const Burden &b, const BurdenLds *s, uint32_t i, uint32_t c, uint32_t w,
                                               BurdenOutcome *o)
{
    const int ts = (int)log_te(d, i, q.t_done + TE_BIAS) - (int)TE_BIAS;       // exposure step; seeds: -(exposed_time + 1)
    const int onset = ts + (int)d.exposed_time + 1;
    if (onset < 0 || onset > (int)q.t_done) return false;
    if (CW_TE(w) == TE_VACCINATED) {
        const uint32_t v = vax_step(q, c);
        if (v != 0xFFFFFFFFu && (int)v - 1 < onset) return false;              // (never Infected after a step)
    }
    const uint32_t k = b.grp ? b.grp[c] : 0u;
    if (k >= b.n_groups || k >= BURDEN_GROUPS) return false;
    const bool old = b.seam_step != 0u && (uint32_t)onset <= b.seam_step;
    const philox_out r = philox4x32_10(d.id_base + c, (uint32_t)onset, ESIM_SLOT_BURDEN, 0u, old ? b.old_seed_lo : d.seed_lo, old ? b.old_seed_hi : d.seed_hi);
    uint32_t n_d = 0u, n_s = 0u;
    for (uint32_t j = 0u; j < b.n_delay; ++j) n_d += s->cdf[j] <= r.w1 ? 1u : 0u;
    for (uint32_t j = 0u; j < b.n_stay; ++j) n_s += s->cdf[BURDEN_BINS + j] <= r.w2 ? 1u : 0u;
    o->onset = (uint32_t)onset;
    o->admitted = r.w0 < s->thr[k];
    o->admit_step = (uint32_t)onset + b.delay_unit * n_d;                      // (at most 7600 + 65535 * 64)
    o->end_step = o->admit_step + b.stay_unit * (1u + n_s);
    o->died = o->admitted && r.w3 < s->thr[b.n_groups + k];
    return true;
}

// admit_step[c], end_step[c] and died[c] of every admitted case; a citizen that is none is not written (the host pre-fills with
// ESIM_NEVER and 0).  Any output may be nullptr.
__global__ __launch_bounds__(TPB) void k_burden_outcomes(Dev d, Series q, Burden b, uint32_t log_len, uint32_t *admit_step, uint32_t *end_step, uint8_t *died)
{
    __shared__ BurdenLds s;
    burden_stage(b, &s);
    for (uint32_t i = blockIdx.x * TPB + threadIdx.x; i < log_len; i += gridDim.x * TPB) {
        const uint32_t c = d.log[i];
        if (c >= d.n) continue;
        BurdenOutcome o;
        if (!burden_outcome(d, q, b, &s, i, c, d.cit[c], &o) || !o.admitted) continue;
        if (admit_step) admit_step[c] = o.admit_step;
        if (end_step) end_step[c] = o.end_step;
        if (died && o.died) died[c] = 1u;
    }
}

// The column of citizen c under q.key: the one column, the household's area, or the label.
__device__ __forceinline__ bool burden_col(const Dev &d, const Series &q, uint32_t c, uint32_t w, uint32_t *col)
{
    uint32_t other;
    *col = 0u;
    return q.key == CURVE_BY_ALL || series_cols(d, q, c, w, col, &other);
}

// Rows of q.p0.  Admissions and deaths: one add at the row of the step, as the event rows of k_series_log (a row sums the steps
// of its stride).  Occupancy: the difference rows of rows_add over the steps admit_step .. end_step - 1, which k_series_prefix sums.
__global__ __launch_bounds__(TPB) void k_burden_rows(Dev d, Series q, Burden b, uint32_t what, uint32_t log_len)
{
    __shared__ BurdenLds s;
    burden_stage(b, &s);
    for (uint32_t i = blockIdx.x * TPB + threadIdx.x; i < log_len; i += gridDim.x * TPB) {
        const uint32_t c = d.log[i];
        if (c >= d.n) continue;
        const uint32_t w = d.cit[c];
        uint32_t col;
        BurdenOutcome o;
        if (!burden_col(d, q, c, w, &col) || !burden_outcome(d, q, b, &s, i, c, w, &o) || !o.admitted) continue;
        if (what == BURDEN_OCCUPANCY) {
            int p = (int)o.admit_step, e = (int)(o.end_step - 1u);
            if (clip(q, &p, &e)) rows_add(q, (uint32_t)p, (uint32_t)e, col, col);
            continue;
        }
        if (what == BURDEN_DEATHS && !o.died) continue;
        const uint32_t step = what == BURDEN_DEATHS ? o.end_step : o.admit_step;
        if (step < q.first || step > q.t_done) continue;
        const uint64_t row = (uint64_t)(step - q.first) / q.stride;
        if (row < q.n_rows) atomicAdd(&q.p0[row * q.n_cols + col], 1u);
    }
}

// tab[key] += the lanes of the wavefront that are `valid` and hold that key: one atomic per distinct key of the wavefront, so
// that the one column of ESIM_BY_ALL is not one address for every case.  Every lane of the wavefront calls it.
__device__ __forceinline__ void burden_count(uint32_t *tab, uint32_t key, bool valid, uint32_t lane)
{
    unsigned long long left = __ballot(valid);
    while (left) {
        const uint32_t lead = (uint32_t)__ffsll((long long)left) - 1u;
        const uint32_t k = __shfl(key, (int)lead, 64);
        const unsigned long long same = __ballot(valid && key == k);
        if (lane == lead) atomicAdd(&tab[k], (uint32_t)__popcll(same));
        left &= ~same;
    }
}

// The change points of the occupancy curve into the pair table, clipped to [q.first, last] as k_curve_events clips: +1 under
// (column, admit_step), -1 under (column, end_step).  The admitted cases whose admission, and the deaths whose step, lies inside
// the window are counted into the [n_cols] tables: with at most BURDEN_LDS_COLS columns (one column, a handful of groups: few
// addresses for every case of the run) in a table of the workgroup's LDS that is added to the global one at the end, with more
// by one atomic per wavefront and column.  Every lane of a workgroup makes the same trips.
__global__ __launch_bounds__(TPB) void k_burden_events(Dev d, Series q, Burden b, uint32_t last, uint32_t log_len, PairTable t, uint32_t *admissions, uint32_t *deaths)
{
    __shared__ BurdenLds s;
    __shared__ uint32_t s_cnt[2u * BURDEN_LDS_COLS];
    const bool local = q.n_cols <= BURDEN_LDS_COLS;
    if (local) for (uint32_t j = threadIdx.x; j < 2u * q.n_cols; j += TPB) s_cnt[j] = 0u;
    burden_stage(b, &s);                                          // (its barrier covers the table above)
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t i0 = (uint64_t)blockIdx.x * TPB; i0 < (uint64_t)log_len; i0 += (uint64_t)gridDim.x * TPB) {
        const uint64_t i = i0 + threadIdx.x;
        const uint32_t c = i < (uint64_t)log_len ? d.log[i] : 0xFFFFFFFFu;
        uint32_t col = 0u;
        BurdenOutcome o = BurdenOutcome();
        bool in = c < d.n;
        if (in) {
            const uint32_t w = d.cit[c];
            in = burden_col(d, q, c, w, &col) && burden_outcome(d, q, b, &s, (uint32_t)i, c, w, &o) && o.admitted;
        }
        const bool adm = in && o.admit_step >= q.first && o.admit_step <= last, dth = in && o.died && o.end_step >= q.first && o.end_step <= last;
        if (local) {
            if (adm) atomicAdd(&s_cnt[col], 1u);
            if (dth) atomicAdd(&s_cnt[q.n_cols + col], 1u);
        } else {
            burden_count(admissions, col, adm, lane);
            burden_count(deaths, col, dth, lane);
        }
        if (!in) continue;
        const uint32_t p = o.admit_step < q.first ? q.first : o.admit_step;
        const uint32_t e = o.end_step - 1u > last ? last : o.end_step - 1u;      // (end_step >= admit_step + 1)
        if (p > e) continue;
        const uint64_t base = (uint64_t)col << 32;
        pair_add(t, base | p, 1u);
        if (e + 1u <= last) pair_add(t, base | (e + 1u), 0xFFFFFFFFu);
    }
    if (!local) return;                                           // (uniform)
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < 2u * q.n_cols; j += TPB) {
        const uint32_t v = s_cnt[j];
        if (v) atomicAdd(j < q.n_cols ? &admissions[j] : &deaths[j - q.n_cols], v);
    }
}
