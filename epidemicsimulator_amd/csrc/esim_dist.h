// esim_dist.h -- the kept members of an ensemble compared pair by pair: out[i * M + j], in 64 bits, the distance of
// member i and member j summed over a window of cells.  Built like esim_depth.h, on esim_members.h and on nothing else, so that
// a probe can include this header alone (tests/native/dist_probe.hip).
//
// The input is the store of esim_members.h: M planes [member][cell] of keys, plane m at planes + m * plane_stride, a window
// [first_cell, first_cell + n_cells).  A key equal to MEMBERS_NEVER is replaced by `never_as` before it is compared.
//
//   DIST_L1      the sum over the window's cells of |key_i - key_j| (a signed store's flipped top bit keeps the difference)
//   DIST_DIFFER  the number of the window's cells in which key_i != key_j
//
// k_dist<R, METRIC>: a thread owns pairs, not cells.  A workgroup of 256 threads takes a pair of member tiles (I, J >= I) of
// 16 R members each (R = 1, 2, 4: up to 16, up to 32, and 64 members a tile; only R = 4 has several tiles) and a slice of the
// window's cells; thread (ti, tj) = (tid / 16, tid % 16) owns the R x R pairs of the members ti + 16 a of tile I with the
// members tj + 16 b of tile J, in registers.  Slots from M on are padding: their rows of the tile hold zeros or what an earlier
// tile pair left, they take no part in the tile's key range, and they never reach `out`.
//   staging    the workgroup walks its cells 256 a trip, a lane a cell.  A cell that members_trivial settles gives 0 to every
//              pair: its planes are not read.  The live cells are ranked by a ballot per wavefront and a count per wavefront in
//              LDS, and packed densely into the tile s[member row][DIST_T cells] -- a sum over cells does not care which cell
//              is which.  The tile is flushed (compared) when it is full and once more, partially, behind the loop.
//   layout     a row holds DIST_T + 4 words, so that row r starts r 16-byte slots further round the 64 banks.  A thread reads 4
//              consecutive cells of each of its 2 R members with 16-byte reads.  Of the lanes of a wavefront, those with the
//              same ti (same tj) read one address -- a broadcast --, and the 16 lanes that ds_read_b128 serves in a cycle hold
//              at most 2 consecutive ti and 16 different tj: rows ti + 16 a and tj + 16 b lie in different slots for
//              different ti and tj.  No bank conflict by the rule (a/4) mod 64 per group of 16 lanes.
//   32 bits    while staging, the tile's smallest and largest key (after never_as) are taken with LDS atomics.  Where
//              (max - min) * DIST_T < 2^32 the tile is summed in 32-bit accumulators, |a - b| + acc in one instruction
//              (dist_sad), added into the thread's 64-bit ones at the tile's end; else a 64-bit inner loop runs.  The branch is
//              uniform per workgroup.  DIST_DIFFER always fits 32 bits a tile.
//   write-back every workgroup adds its partial block once per (tile pair, slice), the pairs i < j < M only, with atomicAdd on
//              unsigned long long into `out`, zeroed by the caller; k_dist_mirror then copies the upper triangle into the lower
//              one.  The diagonal stays 0.
//   stats      stats[0] the live cells of the window (counted by the workgroups of tile pair 0), stats[1] the tiles flushed,
//              stats[2] those of them summed in 32 bits, stats[3] those flushed partially; zeroed by the caller.
//
// Both kernels loop with a grid stride; dist_enqueue takes the largest grid from the caller.
#pragma once
#include <type_traits>
#include "esim_members.h"

#define DIST_L1 0
#define DIST_DIFFER 1
#define DIST_TPB 256u
#define DIST_T 64u                              // the cells of a tile
#define DIST_ROW (DIST_T + 4u)                  // the words of a member's row of the tile
#define DIST_STATS 4u
#define DIST_NARROW_RANGE ((uint32_t)((1ull << 32) / DIST_T))      // a tile whose max - min is below this sums in 32 bits

const uint32_t DIST_GRID = 1024u;

// The members of a tile for M members, and the pairs (I, J >= I) of tiles.
__host__ __device__ static inline uint32_t dist_tile_members(uint32_t M) { return M <= 16u ? 16u : M <= 32u ? 32u : 64u; }
__host__ __device__ static inline uint32_t dist_tile_pairs(uint32_t M)
{
    const uint32_t t = (M + dist_tile_members(M) - 1u) / dist_tile_members(M);
    return t * (t + 1u) / 2u;
}
// What the grid strides over: (tile pair, trip of 256 cells).
static inline uint64_t dist_items(uint32_t M, uint64_t n_cells) { return (uint64_t)dist_tile_pairs(M) * ((n_cells + DIST_TPB - 1u) / DIST_TPB); }

// |a - b| + acc in one instruction.  (__usad compiles to max, min, subtract and add for gfx950: the instruction is asked for by name.)
__device__ __forceinline__ uint32_t dist_sad(uint32_t a, uint32_t b, uint32_t acc)
{
    uint32_t r;
    asm("v_sad_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(acc));
    return r;
}

// The first nq quads of cells of the tile into the thread's accumulators.
template <uint32_t R, int METRIC, bool WIDE>
__device__ __forceinline__ void dist_tile(const uint32_t *sa, const uint32_t *sb, uint32_t nq, unsigned long long (&acc)[R][R])
{
    typedef typename std::conditional<WIDE, unsigned long long, uint32_t>::type sum_t;
    sum_t t[R][R];
#pragma unroll
    for (uint32_t a = 0u; a < R; ++a)
#pragma unroll
        for (uint32_t b = 0u; b < R; ++b) t[a][b] = 0u;
    for (uint32_t q = 0u; q < nq; ++q) {
        uint4 A[R], B[R];
#pragma unroll
        for (uint32_t a = 0u; a < R; ++a) A[a] = *(const uint4 *)(sa + a * 16u * DIST_ROW + q * 4u);
#pragma unroll
        for (uint32_t b = 0u; b < R; ++b) B[b] = *(const uint4 *)(sb + b * 16u * DIST_ROW + q * 4u);
#pragma unroll
        for (uint32_t a = 0u; a < R; ++a) {
#pragma unroll
            for (uint32_t b = 0u; b < R; ++b) {
                if (METRIC == DIST_DIFFER) {
                    t[a][b] += (A[a].x != B[b].x ? 1u : 0u) + (A[a].y != B[b].y ? 1u : 0u) + (A[a].z != B[b].z ? 1u : 0u) + (A[a].w != B[b].w ? 1u : 0u);
                } else if (WIDE) {
                    t[a][b] += (sum_t)(max(A[a].x, B[b].x) - min(A[a].x, B[b].x)) + (sum_t)(max(A[a].y, B[b].y) - min(A[a].y, B[b].y));
                    t[a][b] += (sum_t)(max(A[a].z, B[b].z) - min(A[a].z, B[b].z)) + (sum_t)(max(A[a].w, B[b].w) - min(A[a].w, B[b].w));
                } else {
                    t[a][b] = (sum_t)dist_sad(A[a].w, B[b].w, dist_sad(A[a].z, B[b].z, dist_sad(A[a].y, B[b].y, dist_sad(A[a].x, B[b].x, (uint32_t)t[a][b]))));
                }
            }
        }
    }
#pragma unroll
    for (uint32_t a = 0u; a < R; ++a)
#pragma unroll
        for (uint32_t b = 0u; b < R; ++b) acc[a][b] += t[a][b];
}

template <uint32_t R, int METRIC>
__global__ __launch_bounds__(DIST_TPB) void k_dist(const uint32_t *planes, uint64_t plane_stride, uint32_t M, uint64_t first_cell, uint64_t n_cells, MemberSkip skip,
                                                   uint32_t never_as, unsigned long long *out, unsigned long long *stats)
{
    constexpr uint32_t MT = 16u * R;
    __shared__ __attribute__((aligned(16))) uint32_t s[2u * MT * DIST_ROW];
    __shared__ uint32_t s_cnt[2][DIST_TPB / 64u];                  // the live cells of a trip per wavefront, by the trip's parity
    __shared__ uint32_t s_rng[2][2];                               // the smallest and the largest key of a tile, by the tile's parity
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, ti = tid >> 4, tj = tid & 15u;
    for (uint32_t k = tid; k < 2u * MT * DIST_ROW; k += DIST_TPB) s[k] = 0u;
    if (tid < 2u) { s_rng[tid][0] = MEMBERS_NEVER; s_rng[tid][1] = 0u; }
    __syncthreads();
    const uint32_t tiles_m = (M + MT - 1u) / MT, n_pairs = tiles_m * (tiles_m + 1u) / 2u;
    const uint64_t n_trips = (n_cells + DIST_TPB - 1u) / DIST_TPB;
    uint64_t slices = gridDim.x / n_pairs;                         // the slices of the window's trips a tile pair is cut into
    slices = slices < 1u ? 1u : slices < n_trips ? slices : n_trips;
    uint32_t trip_no = 0u, tile_no = 0u;                           // (uniform: every thread makes the same trips and flushes)
    for (uint64_t w = blockIdx.x; w < n_pairs * slices; w += gridDim.x) {
        const uint32_t p = (uint32_t)(w % n_pairs);
        const uint64_t slice = w / n_pairs;
        uint32_t I = 0u, J = p;
        while (J >= tiles_m - I) { J -= tiles_m - I; ++I; }
        J += I;
        const bool diag = I == J;
        const uint32_t n_i = min(MT, M - I * MT), n_j = diag ? 0u : min(MT, M - J * MT);
        uint32_t *const row_i = s, *const row_j = diag ? s : s + MT * DIST_ROW;
        const uint32_t *const sa = row_i + ti * DIST_ROW, *const sb = row_j + tj * DIST_ROW;
        unsigned long long acc[R][R];
#pragma unroll
        for (uint32_t a = 0u; a < R; ++a)
#pragma unroll
            for (uint32_t b = 0u; b < R; ++b) acc[a][b] = 0ull;
        unsigned long long n_live = 0ull;
        uint32_t fill = 0u, n_tiles = 0u, n_narrow = 0u, n_partial = 0u;
        // One flush: the first `cells` columns of the tile, every thread.  Behind it the tile may be written again.
        auto flush = [&](uint32_t cells) {
            __syncthreads();
            const uint32_t par = tile_no & 1u;
            const bool narrow = METRIC == DIST_DIFFER || s_rng[par][1] - s_rng[par][0] < DIST_NARROW_RANGE;
            if (tid == 0u) { s_rng[par ^ 1u][0] = MEMBERS_NEVER; s_rng[par ^ 1u][1] = 0u; }     // (of the tile before: nobody reads it any more)
            if (narrow) dist_tile<R, METRIC, false>(sa, sb, (cells + 3u) / 4u, acc);
            else dist_tile<R, METRIC, true>(sa, sb, (cells + 3u) / 4u, acc);
            n_tiles += 1u; n_narrow += narrow ? 1u : 0u; n_partial += cells < DIST_T ? 1u : 0u;
            tile_no += 1u;
            __syncthreads();
        };
        for (uint64_t trip = slice; trip < n_trips; trip += slices) {
            const uint64_t i = trip * DIST_TPB + tid;
            uint32_t same;
            bool live = i < n_cells && !members_trivial(skip, first_cell + i, &same);
            const unsigned long long votes = __ballot(live);
            uint32_t *const cnt = s_cnt[trip_no & 1u];
            trip_no += 1u;
            if (lane == 0u) cnt[wave] = (uint32_t)__popcll(votes);
            __syncthreads();
            uint32_t pos = fill + (uint32_t)__popcll(votes & ((1ull << lane) - 1ull)), total = fill;
#pragma unroll
            for (uint32_t k = 0u; k < DIST_TPB / 64u; ++k) { pos += k < wave ? cnt[k] : 0u; total += cnt[k]; }
            n_live += total - fill;
            for (;;) {
                if (live && pos < DIST_T) {                        // the cell into column pos of the tile
                    const uint32_t *pc = planes + first_cell + i;
                    uint32_t lo = MEMBERS_NEVER, hi = 0u;
#pragma unroll 8
                    for (uint32_t r = 0u; r < n_i; ++r) {
                        uint32_t k = pc[(uint64_t)(I * MT + r) * plane_stride];
                        k = k == MEMBERS_NEVER ? never_as : k;
                        lo = min(lo, k); hi = max(hi, k);
                        row_i[r * DIST_ROW + pos] = k;
                    }
#pragma unroll 8
                    for (uint32_t r = 0u; r < n_j; ++r) {
                        uint32_t k = pc[(uint64_t)(J * MT + r) * plane_stride];
                        k = k == MEMBERS_NEVER ? never_as : k;
                        lo = min(lo, k); hi = max(hi, k);
                        row_j[r * DIST_ROW + pos] = k;
                    }
                    if (METRIC != DIST_DIFFER) { atomicMin(&s_rng[tile_no & 1u][0], lo); atomicMax(&s_rng[tile_no & 1u][1], hi); }
                    live = false;
                }
                if (total < DIST_T) break;
                flush(DIST_T);
                total -= DIST_T; pos -= DIST_T;                    // (a lane that still waits has pos >= DIST_T)
            }
            fill = total;
        }
        if (fill) {
            __syncthreads();
            const uint32_t pad = ((fill + 3u) & ~3u) - fill, rows = diag ? MT : 2u * MT;      // the last quad's other columns: 0 in every row
            for (uint32_t k = tid; k < rows * pad; k += DIST_TPB) s[(k / pad) * DIST_ROW + fill + k % pad] = 0u;
            flush(fill);
        }
#pragma unroll
        for (uint32_t a = 0u; a < R; ++a) {
#pragma unroll
            for (uint32_t b = 0u; b < R; ++b) {
                const uint32_t i = I * MT + ti + 16u * a, j = J * MT + tj + 16u * b;
                if (i < j && j < M && acc[a][b]) atomicAdd(out + (uint64_t)i * M + j, acc[a][b]);
            }
        }
        if (tid == 0u) {
            if (p == 0u && n_live) atomicAdd(stats + 0, n_live);
            if (n_tiles) atomicAdd(stats + 1, (unsigned long long)n_tiles);
            if (n_narrow) atomicAdd(stats + 2, (unsigned long long)n_narrow);
            if (n_partial) atomicAdd(stats + 3, (unsigned long long)n_partial);
        }
    }
}

// The lower triangle from the upper one; the diagonal is the caller's zero.
__global__ __launch_bounds__(DIST_TPB) void k_dist_mirror(unsigned long long *out, uint32_t M)
{
    const uint32_t n = M * M;                                      // (M <= MEMBERS_MAX)
    for (uint32_t k = blockIdx.x * DIST_TPB + threadIdx.x; k < n; k += gridDim.x * DIST_TPB) {
        const uint32_t i = k / M, j = k % M;
        if (i > j) out[k] = out[j * M + i];
    }
}

// The two launches that fill out [M * M] and stats [DIST_STATS], both zeroed by the caller, on `stream`.  M in 1..MEMBERS_MAX,
// metric DIST_L1 or DIST_DIFFER (the caller checks both).
static inline void dist_enqueue(const uint32_t *planes, uint64_t plane_stride, uint32_t M, uint64_t first_cell, uint64_t n_cells, const MemberSkip &skip, int metric,
                                uint32_t never_as, unsigned long long *out, unsigned long long *stats, hipStream_t stream, uint32_t max_blocks = DIST_GRID,
                                uint32_t max_blocks_mirror = DIST_GRID)
{
    if (!n_cells || M < 2u || M > MEMBERS_MAX) return;
    const dim3 grid(members_grid(dist_items(M, n_cells), 1u, max_blocks));
#define DIST_LAUNCH(R) \
    do { \
        if (metric == DIST_DIFFER) hipLaunchKernelGGL((k_dist<R, DIST_DIFFER>), grid, dim3(DIST_TPB), 0, stream, planes, plane_stride, M, first_cell, n_cells, skip, never_as, out, stats); \
        else hipLaunchKernelGGL((k_dist<R, DIST_L1>), grid, dim3(DIST_TPB), 0, stream, planes, plane_stride, M, first_cell, n_cells, skip, never_as, out, stats); \
    } while (0)
    switch (dist_tile_members(M)) {
    case 16u: DIST_LAUNCH(1u); break;
    case 32u: DIST_LAUNCH(2u); break;
    default: DIST_LAUNCH(4u); break;
    }
#undef DIST_LAUNCH
    hipLaunchKernelGGL(k_dist_mirror, dim3(members_grid((uint64_t)M * M, DIST_TPB, max_blocks_mirror)), dim3(DIST_TPB), 0, stream, out, M);
}
