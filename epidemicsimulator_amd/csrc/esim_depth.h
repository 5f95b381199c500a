// esim_depth.h -- the kept members of an ensemble ranked as whole curves: modified band depth per member and column
// over a window of rows, and the envelope of the most central members.  Built like esim_members.h and on nothing else, so that
// a probe can include this header alone (tests/native/depth_probe.hip).
//
// The input is the store of esim_members.h: M planes [member][cell] of keys, cell = row * n_cols + column, a lane owns a cell and
// the lanes of a wavefront take consecutive cells.  A window is the cells [first_cell, first_cell + n_cells) of whole rows.
//
//   count    depth[m * n_cols + c] += pairs - C(below, 2) - C(above, 2) for every cell of column c in the window, below / above
//            the members whose key is smaller / larger than member m's and pairs = C(M, 2): the pairs {j, k} of members, m itself
//            included, whose band [min, max] holds m's key in that cell -- exact with ties.
//            M <= 64    k_depth_count_reg<P>, P = 8, 16, 32, 64: the keys of the cell in P registers with constant indices; a
//                       run-time loop over the member reloads its key (the line is in cache) and compares it with all P.  The
//                       slots from M on hold MEMBERS_NEVER and are taken out of `above` again.
//            M <= 256   k_depth_count_lds<P>, P = 128, 256: the keys of 64 cells staged in LDS column-major as
//                       k_members_select_lds stages them (bank = lane), compared by run-time loops.  No barrier.
//            A cell that the accumulators settle (MemberSkip: every member holds the same key) gives pairs to every member: its
//            planes are not read, it is counted in trivial[c], and k_depth_total adds trivial[c] * pairs.
//            Accumulation: with n_cols >= 64 the 64 lanes of a wavefront hold 64 different columns, one no-return atomic per
//            lane, member and trip on consecutive addresses.  Below that, lanes share columns: lane l sums the lanes l + n_cols,
//            l + 2 n_cols, ... by shuffles and the first n_cols lanes issue one atomic per (wavefront, member, column) and trip.
//   total    k_depth_total: depth[m][c] += trivial[c] * pairs, total[m] += the sum over c in 64 bits, an atomic per 256 columns.
//   pick     thr[c], the need-th largest of depth[.][c], is members_select_enqueue over the depth table itself (a plane layout
//            of one row); k_depth_pick then counts the members at or above it and finds the first deepest one, a lane per column.
//   band     k_depth_band: a lane per cell, the minimum and maximum key over the members that are in and the deepest member's
//            key.  In: depth[m][c] >= thr[c], or bit m of the mask of DepthPool where one set of members serves every column.
//
// Every kernel loops over its items with a grid stride; the enqueue functions take the largest grid from the caller.
#pragma once
#include "esim_members.h"

struct DepthPool { uint32_t on, deepest; uint32_t mask[MEMBERS_MAX / 32u]; };       // on = 0: per column, thr and deepest from the tables

__host__ __device__ static inline uint32_t depth_pairs(uint32_t n) { return n * (n - 1u) / 2u; }   // C(n, 2), n <= MEMBERS_MAX

// The window's largest depth fits 32 bits: n_rows * C(M, 2) <= 0xFFFFFFFF.
static inline bool depth_fits(uint32_t n_rows, uint32_t M) { return (uint64_t)n_rows * depth_pairs(M) <= 0xFFFFFFFFull; }

// One set of members for every column, from the M totals: those at or above the need-th largest (ties all in), the first deepest
// one, and how many are in.  need in 1..M.
static inline DepthPool depth_pool(const uint64_t *total, uint32_t M, uint32_t need, uint32_t *n_in)
{
    DepthPool p = DepthPool();
    p.on = 1u;
    uint64_t thr = 0u;
    for (uint32_t i = 0u; i < M; ++i) {          // the need-th largest: fewer than need are above it, at least need at or above
        uint32_t gt = 0u, ge = 0u;
        for (uint32_t j = 0u; j < M; ++j) { gt += total[j] > total[i] ? 1u : 0u; ge += total[j] >= total[i] ? 1u : 0u; }
        if (gt < need && need <= ge) { thr = total[i]; break; }
    }
    *n_in = 0u;
    for (uint32_t i = 0u; i < M; ++i) {
        if (total[i] >= thr) { p.mask[i >> 5] |= 1u << (i & 31u); *n_in += 1u; }
        if (total[i] > total[p.deepest]) p.deepest = i;
    }
    return p;
}

// contrib added to row[c] for the lanes of a wavefront, which hold consecutive cells; every lane of the wavefront calls this.
__device__ __forceinline__ void depth_add(uint32_t *row, uint32_t n_cols, uint32_t c, uint32_t contrib)
{
    if (n_cols >= 64u) {
        if (contrib) atomicAdd(row + c, contrib);
        return;
    }
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t sum = contrib;
    for (uint32_t d = n_cols; d < 64u; d += n_cols) {              // (the lanes l + k * n_cols hold the column of lane l)
        const uint32_t t = (uint32_t)__shfl((int)contrib, (int)((lane + d) & 63u));
        if (lane + d < 64u) sum += t;
    }
    if (lane < n_cols && sum) atomicAdd(row + c, sum);
}

template <uint32_t P>
__global__ __launch_bounds__(MEMBERS_TPB) void k_depth_count_reg(const uint32_t *planes, uint64_t plane_stride, uint32_t M, uint64_t first_cell, uint64_t n_cells,
                                                                 uint32_t n_cols, MemberSkip skip, uint32_t *depth, uint32_t *trivial)
{
    const uint64_t stride = (uint64_t)gridDim.x * MEMBERS_TPB;
    const uint32_t pairs = depth_pairs(M);
    // (every lane of a wavefront makes the same trips: the ballot and the shuffles below are taken by all 64)
    for (uint64_t i0 = (uint64_t)blockIdx.x * MEMBERS_TPB; i0 < n_cells; i0 += stride) {
        const uint64_t i = i0 + threadIdx.x;
        const bool live = i < n_cells;
        uint32_t fill;
        const bool same = live && members_trivial(skip, first_cell + i, &fill);
        const bool count = live && !same;
        const uint32_t c = (uint32_t)((first_cell + i) % n_cols);
        depth_add(trivial, n_cols, c, same ? 1u : 0u);
        if (!__any(count)) continue;
        const uint32_t *p = planes + first_cell + i;
        uint32_t v[P];
#pragma unroll
        for (uint32_t m = 0u; m < P; ++m) v[m] = count && m < M ? p[(uint64_t)m * plane_stride] : MEMBERS_NEVER;
        for (uint32_t m = 0u; m < M; ++m) {
            const uint32_t x = count ? p[(uint64_t)m * plane_stride] : 0u;
            uint32_t below = 0u, above = 0u;
#pragma unroll
            for (uint32_t k = 0u; k < P; ++k) { below += v[k] < x ? 1u : 0u; above += v[k] > x ? 1u : 0u; }
            above -= x != MEMBERS_NEVER ? P - M : 0u;              // (the padding is above every key but MEMBERS_NEVER)
            depth_add(depth + (uint64_t)m * n_cols, n_cols, c, count ? pairs - depth_pairs(below) - depth_pairs(above) : 0u);
        }
    }
}

template <uint32_t P>
__global__ __launch_bounds__(64) void k_depth_count_lds(const uint32_t *planes, uint64_t plane_stride, uint32_t M, uint64_t first_cell, uint64_t n_cells,
                                                        uint32_t n_cols, MemberSkip skip, uint32_t *depth, uint32_t *trivial)
{
    __shared__ uint32_t s[P * 64u];
    const uint32_t lane = threadIdx.x;
    uint32_t *col = s + lane;                                      // key m of the lane's cell: col[m * 64]
    const uint32_t pairs = depth_pairs(M);
    for (uint64_t i0 = (uint64_t)blockIdx.x * 64u; i0 < n_cells; i0 += (uint64_t)gridDim.x * 64u) {
        const uint64_t i = i0 + lane;
        const bool live = i < n_cells;
        uint32_t fill;
        const bool same = live && members_trivial(skip, first_cell + i, &fill);
        const bool count = live && !same;
        const uint32_t c = (uint32_t)((first_cell + i) % n_cols);
        depth_add(trivial, n_cols, c, same ? 1u : 0u);
        if (!__any(count)) continue;
        const uint32_t *p = planes + first_cell + i;
#pragma unroll 8
        for (uint32_t m = 0u; m < M; ++m) col[m * 64u] = count ? p[(uint64_t)m * plane_stride] : MEMBERS_NEVER;
        for (uint32_t m = 0u; m < M; ++m) {
            const uint32_t x = col[m * 64u];
            uint32_t below = 0u, above = 0u;
#pragma unroll 8
            for (uint32_t k = 0u; k < M; ++k) { const uint32_t y = col[k * 64u]; below += y < x ? 1u : 0u; above += y > x ? 1u : 0u; }
            depth_add(depth + (uint64_t)m * n_cols, n_cols, c, count ? pairs - depth_pairs(below) - depth_pairs(above) : 0u);
        }
    }
}

// The tiles of 256 columns of the depth table: what k_depth_total's grid strides over.
static inline uint64_t depth_tiles(uint32_t M, uint32_t n_cols) { return (uint64_t)M * ((n_cols + MEMBERS_TPB - 1u) / MEMBERS_TPB); }

__global__ __launch_bounds__(MEMBERS_TPB) void k_depth_total(uint32_t *depth, const uint32_t *trivial, uint32_t M, uint32_t n_cols, unsigned long long *total)
{
    __shared__ unsigned long long part[MEMBERS_TPB / 64u];
    const uint32_t per_member = (n_cols + MEMBERS_TPB - 1u) / MEMBERS_TPB, pairs = depth_pairs(M);
    const uint64_t tiles = (uint64_t)M * per_member;
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint32_t m = (uint32_t)(t / per_member), c = (uint32_t)(t % per_member) * MEMBERS_TPB + threadIdx.x;
        uint32_t d = 0u;
        if (c < n_cols) {
            const uint64_t at = (uint64_t)m * n_cols + c;
            d = depth[at] + trivial[c] * pairs;
            depth[at] = d;
        }
        uint32_t lo = d, hi = 0u;                                  // the wavefront's sum in two words
        for (uint32_t o = 32u; o > 0u; o >>= 1) {
            const uint32_t a = (uint32_t)__shfl_down((int)lo, o), b = (uint32_t)__shfl_down((int)hi, o);
            const uint32_t sum = lo + a;
            hi += b + (sum < lo ? 1u : 0u);
            lo = sum;
        }
        if ((threadIdx.x & 63u) == 0u) part[threadIdx.x >> 6] = ((unsigned long long)hi << 32) | lo;
        __syncthreads();
        if (threadIdx.x == 0u) {
            unsigned long long sum = 0ull;
            for (uint32_t w = 0u; w < MEMBERS_TPB / 64u; ++w) sum += part[w];
            if (sum) atomicAdd(total + m, sum);
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(MEMBERS_TPB) void k_depth_pick(const uint32_t *depth, uint32_t M, uint32_t n_cols, const uint32_t *thr, uint32_t *deepest, uint32_t *n_in)
{
    for (uint32_t c = blockIdx.x * MEMBERS_TPB + threadIdx.x; c < n_cols; c += gridDim.x * MEMBERS_TPB) {
        const uint32_t t = thr[c];
        uint32_t best = 0u, arg = 0u, n = 0u;
        for (uint32_t m = 0u; m < M; ++m) {
            const uint32_t d = depth[(uint64_t)m * n_cols + c];
            n += d >= t ? 1u : 0u;
            if (d > best) { best = d; arg = m; }                   // (the first of equals stays)
        }
        deepest[c] = arg;
        n_in[c] = n;
    }
}

__global__ __launch_bounds__(MEMBERS_TPB) void k_depth_band(const uint32_t *planes, uint64_t plane_stride, uint32_t M, uint64_t first_cell, uint64_t n_cells, uint32_t n_cols,
                                                            MemberSkip skip, const uint32_t *depth, const uint32_t *thr, const uint32_t *deepest, DepthPool pool,
                                                            uint32_t *lo, uint32_t *hi, uint32_t *median)
{
    const uint64_t stride = (uint64_t)gridDim.x * MEMBERS_TPB;
    for (uint64_t i = (uint64_t)blockIdx.x * MEMBERS_TPB + threadIdx.x; i < n_cells; i += stride) {
        uint32_t a = MEMBERS_NEVER, b = 0u, mid;
        if (members_trivial(skip, first_cell + i, &mid)) {
            a = b = mid;                                           // (need >= 1: somebody is in)
        } else {
            const uint32_t *p = planes + first_cell + i;
            const uint32_t c = (uint32_t)((first_cell + i) % n_cols);
            if (pool.on) {
#pragma unroll
                for (uint32_t w = 0u; w < MEMBERS_MAX / 32u; ++w) {
                    for (uint32_t bits = pool.mask[w]; bits; bits &= bits - 1u) {
                        const uint32_t x = p[(uint64_t)(w * 32u + (uint32_t)__ffs((int)bits) - 1u) * plane_stride];
                        a = min(a, x); b = max(b, x);
                    }
                }
                mid = p[(uint64_t)pool.deepest * plane_stride];
            } else {
                const uint32_t t = thr[c];
                for (uint32_t m = 0u; m < M; ++m) {
                    if (depth[(uint64_t)m * n_cols + c] < t) continue;
                    const uint32_t x = p[(uint64_t)m * plane_stride];
                    a = min(a, x); b = max(b, x);
                }
                mid = p[(uint64_t)deepest[c] * plane_stride];
            }
        }
        if (lo) lo[i] = a;
        if (hi) hi[i] = b;
        if (median) median[i] = mid;
    }
}

// The cells a workgroup of the count kernel takes per trip for M members: those of the selection kernels.
static inline uint32_t depth_count_per_block(uint32_t M) { return members_select_per_block(M); }

// The launch that adds the window's cells to depth [M * n_cols] and trivial [n_cols], both zeroed by the caller.  M in
// 1..MEMBERS_MAX, n_cols >= 1, the window made of whole rows.
static inline void depth_count_enqueue(const uint32_t *planes, uint64_t plane_stride, uint32_t M, uint64_t first_cell, uint64_t n_cells, uint32_t n_cols,
                                       const MemberSkip &skip, uint32_t *depth, uint32_t *trivial, hipStream_t stream, uint32_t max_blocks = MEMBERS_GRID)
{
    if (!n_cells || !n_cols || !M || M > MEMBERS_MAX) return;
    const dim3 grid(members_grid(n_cells, depth_count_per_block(M), max_blocks));
#define DEPTH_LAUNCH(kernel, tpb) hipLaunchKernelGGL(kernel, grid, dim3(tpb), 0, stream, planes, plane_stride, M, first_cell, n_cells, n_cols, skip, depth, trivial)
    switch (members_padded(M)) {
    case 8u: DEPTH_LAUNCH(k_depth_count_reg<8u>, MEMBERS_TPB); break;
    case 16u: DEPTH_LAUNCH(k_depth_count_reg<16u>, MEMBERS_TPB); break;
    case 32u: DEPTH_LAUNCH(k_depth_count_reg<32u>, MEMBERS_TPB); break;
    case 64u: DEPTH_LAUNCH(k_depth_count_reg<64u>, MEMBERS_TPB); break;
    case 128u: DEPTH_LAUNCH(k_depth_count_lds<128u>, 64u); break;
    default: DEPTH_LAUNCH(k_depth_count_lds<256u>, 64u); break;
    }
#undef DEPTH_LAUNCH
}

// The launch behind the count: the trivial cells' share into depth, and total [M], zeroed by the caller.
static inline void depth_total_enqueue(uint32_t *depth, const uint32_t *trivial, uint32_t M, uint32_t n_cols, unsigned long long *total, hipStream_t stream,
                                       uint32_t max_blocks = MEMBERS_GRID)
{
    if (!n_cols || !M) return;
    hipLaunchKernelGGL(k_depth_total, dim3(members_grid(depth_tiles(M, n_cols), 1u, max_blocks)), dim3(MEMBERS_TPB), 0, stream, depth, trivial, M, n_cols, total);
}

// The launch that reads thr [n_cols] and writes deepest and n_in [n_cols].
static inline void depth_pick_enqueue(const uint32_t *depth, uint32_t M, uint32_t n_cols, const uint32_t *thr, uint32_t *deepest, uint32_t *n_in, hipStream_t stream,
                                      uint32_t max_blocks = MEMBERS_GRID)
{
    if (!n_cols || !M) return;
    hipLaunchKernelGGL(k_depth_pick, dim3(members_grid(n_cols, MEMBERS_TPB, max_blocks)), dim3(MEMBERS_TPB), 0, stream, depth, M, n_cols, thr, deepest, n_in);
}

// The launch that writes the planes of the window, [n_cells] each, any nullptr; depth, thr and deepest are read where pool.on is 0.
static inline void depth_band_enqueue(const uint32_t *planes, uint64_t plane_stride, uint32_t M, uint64_t first_cell, uint64_t n_cells, uint32_t n_cols, const MemberSkip &skip,
                                      const uint32_t *depth, const uint32_t *thr, const uint32_t *deepest, const DepthPool &pool, uint32_t *lo, uint32_t *hi, uint32_t *median,
                                      hipStream_t stream, uint32_t max_blocks = MEMBERS_GRID)
{
    if (!n_cells || !n_cols || !M) return;
    hipLaunchKernelGGL(k_depth_band, dim3(members_grid(n_cells, MEMBERS_TPB, max_blocks)), dim3(MEMBERS_TPB), 0, stream,
                       planes, plane_stride, M, first_cell, n_cells, n_cols, skip, depth, thr, deepest, pool, lo, hi, median);
}
