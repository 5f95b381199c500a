// esim_kernels_restart.h -- ensembles on one uploaded population: the initial state rebuilt on the device (esim_restart)
// and the per-Output-Area accumulators over the members of an ensemble (esim_ensemble_fold), by census, by arrival step or
// over the rows of a series, of the exposures by setting or of the cohort reproduction rows.
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

// The same over the rows of a series (esim_ensemble_begin_series): x[cell] is what the series engine has just left in plane 0,
// cells = n_rows * n_cols, and every cell has accumulators of its own.  A pure stream: four cells per lane and trip, 16-byte
// loads of x and hit, 16-byte loads and stores of sum and sumsq, two cells each (the arrays come from hipMalloc, so every one
// starts on a 16-byte boundary); a grid capped by the caller strides over the rest, and the up to three cells behind the last
// whole four are taken by the first lanes of workgroup 0.  A cell with x == 0 adds nothing to sum and sumsq, and nothing to hit
// unless min_cases == 0: what would not change is neither read nor written, so a window in which the epidemic has hardly
// arrived costs the 4 B per cell of x and little else.  With min_cases == 0 every cell counts as hit, zero or not.
__global__ __launch_bounds__(TPB) void k_ensemble_fold_rows(const uint32_t *x, uint64_t cells, uint32_t min_cases,
                                                            uint32_t *hit, unsigned long long *sum, unsigned long long *sumsq, uint32_t *members)
{
    if (blockIdx.x == 0u && threadIdx.x == 0u) *members += 1u;
    const uint4 *x4 = reinterpret_cast<const uint4 *>(x);
    uint4 *h4 = reinterpret_cast<uint4 *>(hit);
    ulonglong2 *s2 = reinterpret_cast<ulonglong2 *>(sum), *q2 = reinterpret_cast<ulonglong2 *>(sumsq);
    const uint64_t n4 = cells >> 2, stride = (uint64_t)gridDim.x * TPB;
    for (uint64_t i = (uint64_t)blockIdx.x * TPB + threadIdx.x; i < n4; i += stride) {
        const uint4 v = x4[i];
        const uint32_t hx = v.x >= min_cases, hy = v.y >= min_cases, hz = v.z >= min_cases, hw = v.w >= min_cases;
        if (hx | hy | hz | hw) {
            uint4 h = h4[i];
            h.x += hx; h.y += hy; h.z += hz; h.w += hw;
            h4[i] = h;
        }
        if (v.x | v.y) {
            ulonglong2 s = s2[2u * i], q = q2[2u * i];
            s.x += v.x; s.y += v.y; q.x += (unsigned long long)v.x * v.x; q.y += (unsigned long long)v.y * v.y;
            s2[2u * i] = s; q2[2u * i] = q;
        }
        if (v.z | v.w) {
            ulonglong2 s = s2[2u * i + 1u], q = q2[2u * i + 1u];
            s.x += v.z; s.y += v.w; q.x += (unsigned long long)v.z * v.z; q.y += (unsigned long long)v.w * v.w;
            s2[2u * i + 1u] = s; q2[2u * i + 1u] = q;
        }
    }
    const uint64_t tail = (n4 << 2) + threadIdx.x;
    if (blockIdx.x == 0u && threadIdx.x < (uint32_t)(cells & 3u)) {
        const uint32_t v = x[tail];
        if (v >= min_cases) hit[tail] += 1u;
        if (v) { sum[tail] += v; sumsq[tail] += (unsigned long long)v * v; }
    }
}

// The accumulators of esim_ensemble_begin_reproduction, [cells] each but the member counter: two counters and five sums a cell.
struct RatioAcc {
    uint32_t *defined, *hit, *members;
    unsigned long long *sum_c, *sum_o, *sq_c, *sq_o, *cross;
};

// hit of one cell with a cohort: offspring / cases >= r_num / r_den, in integers (both products fit 64 bits).
__device__ __forceinline__ uint32_t ratio_hit(uint32_t c, uint32_t o, uint32_t r_num, uint32_t r_den)
{
    return (unsigned long long)o * r_den >= (unsigned long long)c * r_num;
}

// The five sums of cells 2 * j and 2 * j + 1, 16 bytes each way.
__device__ __forceinline__ void ratio_pair(const RatioAcc &a, uint64_t j, uint32_t c0, uint32_t c1, uint32_t o0, uint32_t o1)
{
    ulonglong2 *sc = reinterpret_cast<ulonglong2 *>(a.sum_c) + j, *so = reinterpret_cast<ulonglong2 *>(a.sum_o) + j;
    ulonglong2 *qc = reinterpret_cast<ulonglong2 *>(a.sq_c) + j, *qo = reinterpret_cast<ulonglong2 *>(a.sq_o) + j, *x = reinterpret_cast<ulonglong2 *>(a.cross) + j;
    ulonglong2 vsc = *sc, vso = *so, vqc = *qc, vqo = *qo, vx = *x;
    vsc.x += c0; vsc.y += c1; vso.x += o0; vso.y += o1;
    vqc.x += (unsigned long long)c0 * c0; vqc.y += (unsigned long long)c1 * c1;
    vqo.x += (unsigned long long)o0 * o0; vqo.y += (unsigned long long)o1 * o1;
    vx.x += (unsigned long long)c0 * o0; vx.y += (unsigned long long)c1 * o1;
    *sc = vsc; *so = vso; *qc = vqc; *qo = vqo; *x = vx;
}

// What decides `defined` and `hit` of one cell of the two-plane fold: the reproduction kind's rule and the paired kind's.  The
// five sums are the same for both.
struct RatioRule {                  // esim_ensemble_begin_reproduction: a cohort of at least min_cohort cases; o / c >= r_num / r_den
    uint32_t min_cohort, r_num, r_den;
    __device__ __forceinline__ uint32_t defined(uint32_t c) const { return c >= min_cohort; }
    __device__ __forceinline__ uint32_t hit(uint32_t c, uint32_t o) const { return ratio_hit(c, o, r_num, r_den); }
};
struct PairedRule {                 // esim_ensemble_begin_paired: c = the baseline's cases, o = the current run's; b - c >= min_averted as signed
    uint32_t min_baseline, min_averted;
    __device__ __forceinline__ uint32_t defined(uint32_t c) const { return c >= min_baseline; }
    __device__ __forceinline__ uint32_t hit(uint32_t c, uint32_t o) const { return (long long)c - (long long)o >= (long long)min_averted; }
};

// The same over two row planes (esim_ensemble_begin_reproduction: c[cell] and o[cell] are the cases and the offspring
// k_tree_rows has just left in the two kept planes; esim_ensemble_begin_paired: the baseline's and the current run's event rows).
// Per cell: defined += rule.defined(c); hit += 1 where that holds and rule.hit(c, o); the five sums always.  The shape of
// k_ensemble_fold_rows: a lane owns its cells (plain
// loads and stores), four cells per lane and trip, 16-byte loads of both planes and of defined and hit, 16-byte loads and stores
// of the sums, two cells each; a grid capped by the caller strides over the rest, and the up to three cells behind the last
// whole four are taken by the first lanes of workgroup 0.  Four cells whose c | o is all zero are neither read nor written in the
// accumulators -- nor are the counters of four cells without a cohort, the hits of four cells without a hit and the sums of two
// zero cells: before the epidemic has arrived a window costs the 8 B per cell of the planes and little else.  A cell with
// offspring but no cases (a cohort the window's column does not hold) still adds to the sums: nothing here relies on o > 0
// implying c > 0.
template <class Rule>
__device__ __forceinline__ void fold_two_planes(const uint32_t *c, const uint32_t *o, uint64_t cells, const Rule rule, const RatioAcc &a)
{
    if (blockIdx.x == 0u && threadIdx.x == 0u) *a.members += 1u;
    const uint4 *c4 = reinterpret_cast<const uint4 *>(c), *o4 = reinterpret_cast<const uint4 *>(o);
    uint4 *d4 = reinterpret_cast<uint4 *>(a.defined), *h4 = reinterpret_cast<uint4 *>(a.hit);
    const uint64_t n4 = cells >> 2, stride = (uint64_t)gridDim.x * TPB;
    for (uint64_t i = (uint64_t)blockIdx.x * TPB + threadIdx.x; i < n4; i += stride) {
        const uint4 vc = c4[i], vo = o4[i];
        if (!(vc.x | vc.y | vc.z | vc.w | vo.x | vo.y | vo.z | vo.w)) continue;
        const uint32_t dx = rule.defined(vc.x), dy = rule.defined(vc.y), dz = rule.defined(vc.z), dw = rule.defined(vc.w);
        if (dx | dy | dz | dw) {
            uint4 d = d4[i];
            d.x += dx; d.y += dy; d.z += dz; d.w += dw;
            d4[i] = d;
            const uint32_t hx = dx & rule.hit(vc.x, vo.x), hy = dy & rule.hit(vc.y, vo.y);
            const uint32_t hz = dz & rule.hit(vc.z, vo.z), hw = dw & rule.hit(vc.w, vo.w);
            if (hx | hy | hz | hw) {
                uint4 h = h4[i];
                h.x += hx; h.y += hy; h.z += hz; h.w += hw;
                h4[i] = h;
            }
        }
        if (vc.x | vc.y | vo.x | vo.y) ratio_pair(a, 2u * i, vc.x, vc.y, vo.x, vo.y);
        if (vc.z | vc.w | vo.z | vo.w) ratio_pair(a, 2u * i + 1u, vc.z, vc.w, vo.z, vo.w);
    }
    const uint64_t tail = (n4 << 2) + threadIdx.x;
    if (blockIdx.x == 0u && threadIdx.x < (uint32_t)(cells & 3u)) {
        const uint32_t vc = c[tail], vo = o[tail];
        if (rule.defined(vc)) { a.defined[tail] += 1u; if (rule.hit(vc, vo)) a.hit[tail] += 1u; }
        if (vc | vo) {
            a.sum_c[tail] += vc; a.sum_o[tail] += vo;
            a.sq_c[tail] += (unsigned long long)vc * vc; a.sq_o[tail] += (unsigned long long)vo * vo; a.cross[tail] += (unsigned long long)vc * vo;
        }
    }
}

// The cohort rows: defined += (c >= min_cohort), min_cohort >= 1; hit += 1 where that holds and o / c >= r_num / r_den.
__global__ __launch_bounds__(TPB) void k_ensemble_fold_ratio(const uint32_t *c, const uint32_t *o, uint64_t cells, uint32_t min_cohort, uint32_t r_num, uint32_t r_den, RatioAcc a)
{
    fold_two_planes(c, o, cells, RatioRule{min_cohort, r_num, r_den}, a);
}

// The paired rows (esim_ensemble_begin_paired): b[cell] and c[cell] are the event rows of the kept baseline and of the run as it
// stands, as k_compare_rows has just left them.  defined += (b >= min_baseline); hit += 1 where that holds and b - c >=
// min_averted as signed, min_averted >= 1; the sums are those of b, c, b * b, c * c and b * c.
__global__ __launch_bounds__(TPB) void k_ensemble_fold_paired(const uint32_t *b, const uint32_t *c, uint64_t cells, uint32_t min_baseline, uint32_t min_averted, RatioAcc a)
{
    fold_two_planes(b, c, cells, PairedRule{min_baseline, min_averted}, a);
}
