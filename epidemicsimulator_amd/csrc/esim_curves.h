// esim_curves.h -- epidemic curves from sorted change points: a segmented scan and a reduction per column.  Nothing
// but integers, atomics and lane intrinsics, so that a probe can include this header alone (tests/native/curves_probe.hip).
//
// The input is what esim_pairs.h leaves: n pairs (key, delta), ascending by key = (column << 32) | step, keys unique; delta is
// the net change of the column's count at that step, modulo 2^32 (a change of -1 is 0xFFFFFFFF, a change of 0 may occur).  A
// column is a segment, and an element is a HEAD where its column differs from that of the element before it.
//
//   scan     val[i] = the sum of the deltas from the head of i's segment up to i: the count from step s_i on.  Reduce, then scan:
//            k_curve_tile   a workgroup per tile of CURVE_TILE elements leaves the tile's aggregate (f, v): f = the tile holds a
//                           head, v = the sum of the deltas behind its last head (of all of them without one);
//            k_curve_carry  one wavefront walks the aggregates, 64 tiles a trip, and leaves per tile the sum that reaches into it
//                           from the tiles before: carry[t + 1] = f[t] ? v[t] : carry[t] + v[t].  A segment may span any number
//                           of tiles;
//            k_curve_scan   the tile again: the scan inside the wavefront by lane shuffles, the heads by one ballot, the four
//                           wavefronts of a trip combined through LDS, and the carry added to the elements in front of the
//                           tile's first head on the way out.
//            Three launches on one stream, so that no workgroup waits for another one: nothing spins.
//   reduce   k_curve_reduce: element i holds the value val[i] from step s_i through len_i steps -- up to the next key of its
//            column, or to last_step -- and a column's summary is a reduction over its elements: the peak and its first step
//            (one 64-bit maximum of (v << 32) | ~s), the steps at or above a threshold with the first and the last of them, and
//            the sum of v * len.  The steps in front of a column's first key count as 0, and a column without a key keeps what
//            the caller filled the tables with.  Every run of equal columns inside a wavefront is combined first (the idea of
//            run_add), so that the tables see one set of atomics per (wavefront, column).
#pragma once
#include <stdint.h>

// Elements a workgroup scans: a multiple of 64.  Up to 256 a workgroup has a lane per element, beyond it makes CURVE_TILE / 256
// trips.  2048: a run of 4 M change points is 2048 tiles, which one wavefront carries in 32 trips; a smaller tile lengthens that
// serial walk, a larger one leaves the chip's 256 compute units fewer workgroups than it can hold.
#ifndef CURVE_TILE
#define CURVE_TILE 2048u
#endif
#define CURVE_TPB (CURVE_TILE < 256u ? CURVE_TILE : 256u)
#define CURVE_WAVES (CURVE_TPB / 64u)
static_assert(CURVE_TILE >= 64u && CURVE_TILE % 64u == 0u && CURVE_TILE % CURVE_TPB == 0u, "CURVE_TILE: a multiple of 64, and of 256 beyond 256");

#define CURVE_NEVER 0xFFFFFFFFu

// The per-column tables of k_curve_reduce, [n_cols] each.  The caller fills `first` with CURVE_NEVER and the others with 0.
struct CurveTabs {
    unsigned long long *best;       // (peak << 32) | ~(its first step); the peak is 0 where nothing was ever counted
    uint32_t *steps;                // steps with a count >= threshold
    uint32_t *first, *last;         // the smallest and the largest of them (last: meaningful where steps != 0)
    unsigned long long *person;     // the sum of the count over the steps
};

// The lane where the segment of `lane` starts inside the wavefront: the highest head at or below it, lane 0 without one.
__device__ __forceinline__ uint32_t curve_start(unsigned long long heads, uint32_t lane)
{
    const unsigned long long below = heads & ((2ull << lane) - 1ull);
    return below ? 63u - (uint32_t)__clzll((long long)below) : 0u;
}

// Inclusive segmented sum over the wavefront: x summed from the start of the lane's segment (curve_start) up to the lane.
__device__ __forceinline__ uint32_t curve_wave_sum(uint32_t x, uint32_t start, uint32_t lane)
{
#pragma unroll
    for (uint32_t off = 1u; off < 64u; off <<= 1) {
        const uint32_t t = __shfl_up(x, off, 64);
        if (lane >= start + off) x += t;
    }
    return x;
}

// One tile, by every lane of its workgroup: the scan of the elements [base, base + CURVE_TILE) below n with `carry` reaching in
// from the tiles before.  out (may be nullptr, may be delta) gets the values; *any_head and *run are the tile's aggregate, the
// same in every lane -- *run with the carry in it where the tile has no head.
__device__ __forceinline__ void curve_tile_scan(const unsigned long long *key, const uint32_t *delta, uint32_t n, uint64_t base, uint32_t carry, uint32_t *out,
                                                bool *any_head, uint32_t *run)
{
    __shared__ uint32_t s_v[2][CURVE_WAVES], s_f[2][CURVE_WAVES];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t running = carry;
    bool seen = false;
    for (uint32_t r = 0u; r < CURVE_TILE / CURVE_TPB; ++r) {
        const uint64_t i = base + (uint64_t)r * CURVE_TPB + threadIdx.x;
        const bool live = i < (uint64_t)n;
        const uint32_t col = live ? (uint32_t)(key[i] >> 32) : CURVE_NEVER;
        uint32_t prev = __shfl_up(col, 1, 64);
        if (lane == 0u && live && i > 0u) prev = (uint32_t)(key[i - 1u] >> 32);
        const bool head = live && (i == 0u || prev != col);
        const unsigned long long heads = __ballot(head);
        uint32_t x = curve_wave_sum(live ? delta[i] : 0u, curve_start(heads, lane), lane);
        const uint32_t buf = r & 1u;                              // (two buffers: one barrier a trip is enough)
        if (lane == 63u) { s_v[buf][wave] = x; s_f[buf][wave] = heads != 0ull; }
        __syncthreads();
        uint32_t c = running, mine = 0u;
#pragma unroll
        for (uint32_t u = 0u; u < CURVE_WAVES; ++u) {
            if (u == wave) mine = c;
            const uint32_t f = s_f[buf][u], v = s_v[buf][u];
            c = f ? v : c + v;
            seen = seen || f != 0u;
        }
        running = c;
        const uint32_t first_head = heads ? (uint32_t)__ffsll((long long)heads) - 1u : 64u;
        if (lane < first_head) x += mine;
        if (out && live) out[i] = x;
    }
    *any_head = seen; *run = running;
}

// The aggregates of the tiles: agg_f[t], agg_v[t].  A workgroup per tile.
__global__ __launch_bounds__(CURVE_TPB) void k_curve_tile(const unsigned long long *key, const uint32_t *delta, uint32_t n, uint32_t *agg_f, uint32_t *agg_v)
{
    bool f; uint32_t v;
    curve_tile_scan(key, delta, n, (uint64_t)blockIdx.x * CURVE_TILE, 0u, nullptr, &f, &v);
    if (threadIdx.x == 0u) { agg_f[blockIdx.x] = f; agg_v[blockIdx.x] = v; }
}

// carry[t] = what reaches into tile t, t < tiles.  One wavefront.
__global__ __launch_bounds__(64) void k_curve_carry(const uint32_t *agg_f, const uint32_t *agg_v, uint32_t tiles, uint32_t *carry)
{
    const uint32_t lane = threadIdx.x;
    uint32_t running = 0u;
    for (uint32_t t0 = 0u; t0 < tiles; t0 += 64u) {
        const uint32_t t = t0 + lane;
        const bool live = t < tiles;
        const unsigned long long heads = __ballot(live && agg_f[t] != 0u);
        uint32_t x = curve_wave_sum(live ? agg_v[t] : 0u, curve_start(heads, lane), lane);
        const uint32_t first_head = heads ? (uint32_t)__ffsll((long long)heads) - 1u : 64u;
        if (lane < first_head) x += running;                      // x: what stands behind tile t
        const uint32_t before = __shfl_up(x, 1, 64);
        if (live) carry[t] = lane == 0u ? running : before;
        running = __shfl(x, 63, 64);
    }
}

// val[i] for every element; val may be delta (a lane reads its element before it writes it, and nobody else reads it).
__global__ __launch_bounds__(CURVE_TPB) void k_curve_scan(const unsigned long long *key, const uint32_t *delta, uint32_t n, const uint32_t *carry, uint32_t *val)
{
    bool f; uint32_t v;
    curve_tile_scan(key, delta, n, (uint64_t)blockIdx.x * CURVE_TILE, carry[blockIdx.x], val, &f, &v);
}

// The reduction per column.  Elements whose column is not below n_cols are left out (the callers insert none).  Every lane of a
// wavefront makes the same trips.
__global__ __launch_bounds__(256) void k_curve_reduce(const unsigned long long *key, const uint32_t *val, uint32_t n, uint32_t n_cols, uint32_t last_step, uint32_t threshold,
                                                      CurveTabs t)
{
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t i0 = (uint64_t)blockIdx.x * 256u; i0 < (uint64_t)n; i0 += (uint64_t)gridDim.x * 256u) {
        const uint64_t i = i0 + threadIdx.x;
        const bool live = i < (uint64_t)n;
        const unsigned long long k = live ? key[i] : ~0ull;
        const uint32_t col = (uint32_t)(k >> 32), s = (uint32_t)k;
        unsigned long long next = __shfl_down(k, 1, 64);
        if (lane == 63u) next = i + 1u < (uint64_t)n ? key[i + 1u] : ~0ull;
        const bool tail = lane == 63u || (uint32_t)(next >> 32) != col;       // the last lane of its run in this wavefront
        const bool use = live && col < n_cols;
        const uint32_t v = use ? val[i] : 0u;
        const uint32_t len = ((uint32_t)(next >> 32) == col ? (uint32_t)next : last_step + 1u) - s;
        const bool at = use && v >= threshold;
        unsigned long long best = use ? ((unsigned long long)v << 32) | (uint32_t)~s : 0ull;
        uint32_t cnt = at ? len : 0u, fst = at ? s : CURVE_NEVER, lst = at ? s + len - 1u : 0u;
        unsigned long long person = (unsigned long long)v * len;
        const uint32_t prev = __shfl_up(col, 1, 64);
        const uint32_t start = curve_start(__ballot(lane == 0u || prev != col), lane);
#pragma unroll
        for (uint32_t off = 1u; off < 64u; off <<= 1) {
            const unsigned long long b = __shfl_up(best, off, 64), p = __shfl_up(person, off, 64);
            const uint32_t c = __shfl_up(cnt, off, 64), f = __shfl_up(fst, off, 64), l = __shfl_up(lst, off, 64);
            if (lane >= start + off) {
                best = b > best ? b : best; person += p;
                cnt += c; fst = f < fst ? f : fst; lst = l > lst ? l : lst;
            }
        }
        if (tail && use) {
            if (best) atomicMax(&t.best[col], best);
            if (cnt) { atomicAdd(&t.steps[col], cnt); atomicMin(&t.first[col], fst); atomicMax(&t.last[col], lst); }
            if (person) atomicAdd(&t.person[col], person);
        }
    }
}

static inline uint32_t curve_tiles(uint32_t n) { return (uint32_t)(((uint64_t)n + CURVE_TILE - 1u) / CURVE_TILE); }

// The launches that scan the n sorted pairs in place (cnt: the deltas in, the values out) on `stream`; agg holds
// 3 * curve_tiles(n) words.
static inline void curve_scan_enqueue(const unsigned long long *key, uint32_t *cnt, uint32_t n, uint32_t *agg, hipStream_t stream)
{
    const uint32_t tiles = curve_tiles(n);
    if (!tiles) return;
    uint32_t *agg_f = agg, *agg_v = agg + tiles, *carry = agg + 2u * (size_t)tiles;
    hipLaunchKernelGGL(k_curve_tile, dim3(tiles), dim3(CURVE_TPB), 0, stream, key, cnt, n, agg_f, agg_v);
    hipLaunchKernelGGL(k_curve_carry, dim3(1), dim3(64), 0, stream, agg_f, agg_v, tiles, carry);
    hipLaunchKernelGGL(k_curve_scan, dim3(tiles), dim3(CURVE_TPB), 0, stream, key, cnt, n, carry, cnt);
}

// The launch that reduces the n scanned pairs into the tables on `stream`, with at most max_blocks workgroups (the kernel loops).
const uint32_t CURVE_REDUCE_GRID = 4096u;
static inline void curve_reduce_enqueue(const unsigned long long *key, const uint32_t *val, uint32_t n, uint32_t n_cols, uint32_t last_step, uint32_t threshold,
                                        const CurveTabs &t, hipStream_t stream, uint32_t max_blocks = CURVE_REDUCE_GRID)
{
    if (!n) return;
    const uint32_t blocks = (uint32_t)(((uint64_t)n + 255u) / 256u);
    hipLaunchKernelGGL(k_curve_reduce, dim3(blocks < max_blocks ? blocks : max_blocks), dim3(256), 0, stream, key, val, n, n_cols, last_step, threshold, t);
}
