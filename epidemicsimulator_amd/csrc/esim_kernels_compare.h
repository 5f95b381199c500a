// esim_kernels_compare.h -- the paired comparison of two runs of one population: the exposure step of every citizen
// as one uint32 plane (k_compare_plane: the kept baseline, and the run as it stands), the comparison of two such planes by
// column (k_compare_count), and the event rows of both (k_compare_rows, k_compare_prefix).  A plane holds the exposure step, 0
// for an index case and ESIM_NEVER for a citizen the log does not hold.  Nothing here writes simulation state, and no step
// kernel knows of it.
#pragma once

#ifndef COMPARE_AREA_WINDOW
#define COMPARE_AREA_WINDOW 256u   // areas whose counters a workgroup of k_compare_count keeps in LDS (-DCOMPARE_AREA_WINDOW=2 tested)
#endif
#define COMPARE_LDS_COLS 1024u     // columns of the LDS table: every group (ESIM_MAX_GROUPS), or the window of areas
#define COMPARE_QUAD (TPB * 4u)    // citizens a workgroup takes per trip, four per lane
static_assert(COMPARE_AREA_WINDOW >= 1u && COMPARE_AREA_WINDOW <= COMPARE_LDS_COLS, "the window of areas lives in the LDS table");
static_assert(COMPARE_LDS_COLS >= ESIM_MAX_GROUPS, "by group every column is in LDS");

// plane[c] = the exposure step of citizen c from the position of its log entry (log_te: the citizen word loses the step once
// the citizen is vaccinated), 0 for the index cases.  The plane is filled with ESIM_NEVER by the caller.  A lane per entry.
__global__ __launch_bounds__(TPB) void k_compare_plane(Dev d, uint32_t t_done, uint32_t log_len, uint32_t *plane)
{
    for (uint32_t i = blockIdx.x * TPB + threadIdx.x; i < log_len; i += gridDim.x * TPB) {
        const uint32_t c = d.log[i];
        if (c >= d.n) continue;
        const uint32_t te = log_te(d, i, t_done + TE_BIAS);
        plane[c] = te > TE_BIAS ? te - TE_BIAS : 0u;
    }
}

// Four neighbouring entries of a plane from citizen c0 on (c0 a multiple of 4: 16 bytes in one load); entries behind the last
// citizen read as ESIM_NEVER without touching memory.
__device__ __forceinline__ uint4 plane_quad(const uint32_t *plane, uint64_t c0, uint64_t n)
{
    if (c0 + 3u < n) return *reinterpret_cast<const uint4 *>(plane + c0);
    uint4 v = make_uint4(ESIM_NEVER, ESIM_NEVER, ESIM_NEVER, ESIM_NEVER);
    if (c0 < n) v.x = plane[c0];
    if (c0 + 1u < n) v.y = plane[c0 + 1u];
    if (c0 + 2u < n) v.z = plane[c0 + 2u];
    return v;
}

// The column of citizen c; ESIM_NEVER where the population's tables do not hold one.
__device__ __forceinline__ uint32_t compare_key(const Dev &d, uint32_t where, const uint16_t *grp, uint64_t c)
{
    if (where == ESIM_BY_ALL) return 0u;
    if (where == ESIM_BY_GROUP) return grp[c];
    const uint32_t h = d.home[c];
    return h < d.n_bld ? d.bld_area[h] : ESIM_NEVER;
}

struct Compare {
    const uint32_t *base, *cur;     // [n] the baseline's plane and the current run's
    uint32_t where;                 // ESIM_BY_ALL, ESIM_AREA_HOME, ESIM_BY_GROUP
    uint32_t first, last;           // the window of steps, first <= last
    uint32_t n_cols, per_block;     // per_block: a multiple of COMPARE_QUAD
    const uint16_t *grp;            // [n] labels, ESIM_BY_GROUP only
    uint32_t *counts;               // [n_cols][ESIM_CMP_N], zeroed by the caller
    unsigned long long *delay;      // [n_cols] sum of c - b over BOTH, two's complement, zeroed by the caller
    uint32_t *first_div;            // one word, ESIM_NEVER from the caller
    uint8_t *cls;                   // [n] zeroed by the caller, or nullptr
};

struct CompareShared {
    unsigned long long delay[COMPARE_LDS_COLS];
    uint32_t cnt[COMPARE_LDS_COLS * ESIM_CMP_N];
    uint32_t base;
};

// cls of one citizen: 0 neither, 1 BOTH, 2 AVERTED, 3 ADDED.  (ESIM_NEVER - first exceeds every last - first.)
__device__ __forceinline__ uint32_t compare_cls(uint32_t b, uint32_t c, uint32_t first, uint32_t span)
{
    const bool in_b = b - first <= span && b >= first, in_c = c - first <= span && c >= first;
    return in_b ? (in_c ? 1u : 2u) : (in_c ? 3u : 0u);
}

// One of the four citizens of every lane of a wavefront, `key` its column where it is a case: the lanes with a case are counted by
// column, the lanes of one column by its first lane (a ballot per class), into the workgroup's LDS table where the column lies in
// it and into the global table where it does not.  Every lane of the wavefront calls it.
__device__ __forceinline__ void compare_tally(const Compare &q, CompareShared &sm, uint32_t n_lds, uint32_t key, uint32_t cls, uint32_t sb, uint32_t sc, uint32_t lane)
{
    const bool live = cls != 0u && key < q.n_cols;
    if (!__ballot(live)) return;
    const bool both = live && cls == 1u;
    unsigned long long todo = __ballot(live);
    while (todo) {                                                    // (wave-uniform: every lane sees the same ballots)
        const uint32_t lead = (uint32_t)__ffsll((long long)todo) - 1u;
        const uint32_t k = __shfl(key, lead, 64);
        const bool mine = live && key == k;
        const unsigned long long same = __ballot(mine);
        uint32_t n[ESIM_CMP_N];
        n[ESIM_CMP_BOTH] = (uint32_t)__popcll(__ballot(mine && both));
        n[ESIM_CMP_AVERTED] = (uint32_t)__popcll(__ballot(mine && cls == 2u));
        n[ESIM_CMP_ADDED] = (uint32_t)__popcll(__ballot(mine && cls == 3u));
        n[ESIM_CMP_EARLIER] = (uint32_t)__popcll(__ballot(mine && both && sc < sb));
        n[ESIM_CMP_LATER] = (uint32_t)__popcll(__ballot(mine && both && sc > sb));
        long long dl = 0;
        if (n[ESIM_CMP_EARLIER] | n[ESIM_CMP_LATER]) {                // the signed sum of c - b over the column's lanes
            dl = mine && both ? (long long)sc - (long long)sb : 0ll;
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) dl += __shfl_xor(dl, o, 64);
        }
        if (lane == lead) {
            const uint32_t rel = k - sm.base;
            if (rel < n_lds) {
#pragma unroll
                for (uint32_t j = 0; j < ESIM_CMP_N; ++j) if (n[j]) atomicAdd(&sm.cnt[rel * ESIM_CMP_N + j], n[j]);
                if (dl) atomicAdd(&sm.delay[rel], (unsigned long long)dl);
            } else {                                                  // outside the window: a population that is not home-sorted
#pragma unroll
                for (uint32_t j = 0; j < ESIM_CMP_N; ++j) if (n[j]) atomicAdd(&q.counts[(size_t)k * ESIM_CMP_N + j], n[j]);
                if (dl) atomicAdd(&q.delay[k], (unsigned long long)dl);
            }
        }
        todo &= ~same;
    }
}

// The comparison: a pure stream over the citizens, 16-byte loads of both planes, four citizens per lane.  A workgroup takes a
// contiguous stretch of per_block citizens.  Almost nobody is a case of either run: a wavefront whose ballot finds none issues
// nothing further, and home building, bld_area and label are fetched for cases only.  The counts and the delay are gathered in
// LDS -- by all and by group every column, by area a window of COMPARE_AREA_WINDOW areas from the area of the stretch's first
// citizen on (citizens are normally home-sorted), keys outside it going to the global table directly -- and flushed once.  The
// first divergence is kept per lane, reduced once per wavefront and lowered with one atomicMin.
__global__ __launch_bounds__(TPB) void k_compare_count(Dev d, Compare q)
{
    __shared__ CompareShared sm;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t n = d.n;
    const uint64_t lo = (uint64_t)blockIdx.x * q.per_block;
    const uint64_t hi = lo + q.per_block < n ? lo + q.per_block : n;
    const uint32_t window = q.where == ESIM_AREA_HOME ? COMPARE_AREA_WINDOW : COMPARE_LDS_COLS;
    const uint32_t n_lds = q.n_cols < window ? q.n_cols : window;
    for (uint32_t i = threadIdx.x; i < n_lds * ESIM_CMP_N; i += TPB) sm.cnt[i] = 0u;
    for (uint32_t i = threadIdx.x; i < n_lds; i += TPB) sm.delay[i] = 0ull;
    if (threadIdx.x == 0) {
        uint32_t b = 0u;
        if (q.where == ESIM_AREA_HOME && lo < hi) { b = compare_key(d, q.where, q.grp, lo); if (b >= q.n_cols) b = 0u; }
        sm.base = b;
    }
    __syncthreads();
    const uint32_t span = q.last - q.first;
    uint32_t div = ESIM_NEVER;
    for (uint64_t q0 = lo; q0 < hi; q0 += COMPARE_QUAD) {             // the same trip count for every lane of the workgroup
        const uint64_t c0 = q0 + (uint64_t)threadIdx.x * 4u;
        const uint4 b = plane_quad(q.base, c0, hi), c = plane_quad(q.cur, c0, hi);
        const uint32_t m0 = b.x < c.x ? b.x : c.x, m1 = b.y < c.y ? b.y : c.y, m2 = b.z < c.z ? b.z : c.z, m3 = b.w < c.w ? b.w : c.w;
        if (b.x != c.x && m0 < div) div = m0;
        if (b.y != c.y && m1 < div) div = m1;
        if (b.z != c.z && m2 < div) div = m2;
        if (b.w != c.w && m3 < div) div = m3;
        const uint32_t k0 = compare_cls(b.x, c.x, q.first, span), k1 = compare_cls(b.y, c.y, q.first, span);
        const uint32_t k2 = compare_cls(b.z, c.z, q.first, span), k3 = compare_cls(b.w, c.w, q.first, span);
        const uint32_t packed = k0 | (k1 << 8) | (k2 << 16) | (k3 << 24);
        if (!__ballot(packed != 0u)) continue;
        if (q.cls && packed) {
            if (c0 + 3u < n) *reinterpret_cast<uint32_t *>(q.cls + c0) = packed;
            else for (uint32_t j = 0; j < 4u && c0 + j < n; ++j) q.cls[c0 + j] = (uint8_t)(packed >> (8u * j));
        }
        // the columns of the lane's cases, fetched together: four independent chains of loads instead of one behind the other
        const uint32_t y0 = k0 ? compare_key(d, q.where, q.grp, c0) : ESIM_NEVER, y1 = k1 ? compare_key(d, q.where, q.grp, c0 + 1u) : ESIM_NEVER;
        const uint32_t y2 = k2 ? compare_key(d, q.where, q.grp, c0 + 2u) : ESIM_NEVER, y3 = k3 ? compare_key(d, q.where, q.grp, c0 + 3u) : ESIM_NEVER;
        compare_tally(q, sm, n_lds, y0, k0, b.x, c.x, lane);
        compare_tally(q, sm, n_lds, y1, k1, b.y, c.y, lane);
        compare_tally(q, sm, n_lds, y2, k2, b.z, c.z, lane);
        compare_tally(q, sm, n_lds, y3, k3, b.w, c.w, lane);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { const uint32_t v = __shfl_xor(div, o, 64); if (v < div) div = v; }
    if (lane == 0u && div != ESIM_NEVER) atomicMin(q.first_div, div);
    __syncthreads();
    const uint32_t base = sm.base;
    for (uint32_t i = threadIdx.x; i < n_lds * ESIM_CMP_N; i += TPB) {
        const uint32_t v = sm.cnt[i];
        if (v) atomicAdd(&q.counts[(size_t)(base + i / ESIM_CMP_N) * ESIM_CMP_N + i % ESIM_CMP_N], v);   // (only columns that were seen have a count)
    }
    for (uint32_t i = threadIdx.x; i < n_lds; i += TPB) {
        const unsigned long long v = sm.delay[i];
        if (v) atomicAdd(&q.delay[base + i], v);
    }
}

struct CompareRows {
    const uint32_t *base, *cur;     // [n] the two planes
    uint32_t where, first, n_rows, stride, n_cols;
    const uint16_t *grp;            // [n] labels, ESIM_BY_GROUP only
    uint32_t *rows_b, *rows_c;      // [n_rows][n_cols] each, zeroed by the caller
};

// The row of exposure step s, or ESIM_NEVER: row i holds the steps [first + i * stride, + stride).
__device__ __forceinline__ uint32_t compare_row(const CompareRows &r, uint32_t s)
{
    if (s == ESIM_NEVER || s < r.first) return ESIM_NEVER;
    const uint32_t row = (s - r.first) / r.stride;
    return row < r.n_rows ? row : ESIM_NEVER;
}

// One citizen's two adds, the column fetched once.
__device__ __forceinline__ void compare_rows_add(const Dev &d, const CompareRows &r, uint64_t c, uint32_t row_b, uint32_t row_c)
{
    if ((row_b & row_c) == ESIM_NEVER) return;
    const uint32_t key = compare_key(d, r.where, r.grp, c);
    if (key >= r.n_cols) return;
    if (row_b != ESIM_NEVER) atomicAdd(&r.rows_b[(size_t)row_b * r.n_cols + key], 1u);
    if (row_c != ESIM_NEVER) atomicAdd(&r.rows_c[(size_t)row_c * r.n_cols + key], 1u);
}

// The event rows of both runs in one pass over the citizens, loaded as k_compare_count loads them: one add per case and plane
// at the row of its step, the index cases at step 0.  A wavefront without a case in the window issues nothing further.
__global__ __launch_bounds__(TPB) void k_compare_rows(Dev d, CompareRows r)
{
    const uint64_t n = d.n;
    for (uint64_t q0 = (uint64_t)blockIdx.x * COMPARE_QUAD; q0 < n; q0 += (uint64_t)gridDim.x * COMPARE_QUAD) {
        const uint64_t c0 = q0 + (uint64_t)threadIdx.x * 4u;
        const uint4 b = plane_quad(r.base, c0, n), c = plane_quad(r.cur, c0, n);
        const uint32_t b0 = compare_row(r, b.x), b1 = compare_row(r, b.y), b2 = compare_row(r, b.z), b3 = compare_row(r, b.w);
        const uint32_t c0r = compare_row(r, c.x), c1 = compare_row(r, c.y), c2 = compare_row(r, c.z), c3 = compare_row(r, c.w);
        if (!__ballot((b0 & b1 & b2 & b3 & c0r & c1 & c2 & c3) != ESIM_NEVER)) continue;
        compare_rows_add(d, r, c0, b0, c0r);
        compare_rows_add(d, r, c0 + 1u, b1, c1);
        compare_rows_add(d, r, c0 + 2u, b2, c2);
        compare_rows_add(d, r, c0 + 3u, b3, c3);
    }
}

// Cumulative rows: the prefix over the rows of both tables, a lane per column (the accesses coalesce across columns).
__global__ __launch_bounds__(TPB) void k_compare_prefix(uint32_t *rows_b, uint32_t *rows_c, uint32_t n_rows, uint32_t n_cols)
{
    const uint32_t a = blockIdx.x * TPB + threadIdx.x;
    if (a >= n_cols) return;
    uint32_t acc_b = 0u, acc_c = 0u;
    for (uint32_t r = 0; r < n_rows; ++r) {
        const size_t at = (size_t)r * n_cols + a;
        acc_b += rows_b[at]; acc_c += rows_c[at];
        rows_b[at] = acc_b; rows_c[at] = acc_c;
    }
}
