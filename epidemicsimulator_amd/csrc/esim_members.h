// esim_members.h -- order statistics and exceedance counts per cell over the kept members of an ensemble.  Nothing
// but integers, LDS and lane intrinsics, so that a probe can include this header alone (tests/native/members_probe.hip).
//
// The input is M planes [member][cell] of 32-bit keys in device memory, plane m at planes + m * plane_stride: the lanes of a
// wavefront read consecutive cells of one member, a coalesced 256 B a load.  Keys order as unsigned numbers: the caller stores a
// signed value with its top bit flipped (members_key), and MEMBERS_NEVER, the largest key, sorts last.  A lane owns a cell.
//
//   select   out[q * out_stride + i] = the ranks.r[q]-th smallest (0-based) of the M keys of cell first_cell + i.
//            M <= 64    k_members_select_reg<P>, P = 8, 16, 32, 64 the padded size: the keys in P registers, a bitonic network of
//                       min / max pairs unrolled in full, so that every index into the register array is a constant; the slots
//                       from M on hold MEMBERS_NEVER and stay behind every rank < M.  The rank is picked by a chain of selects.
//            M <= 256   k_members_select_lds<P>, P = 128, 256: a wavefront (a workgroup of 64) stages a tile of 64 cells x P keys
//                       into LDS column-major -- lane l owns word m * 64 + l, bank l of 64, so that no access of the column sort
//                       conflicts -- and sorts its column in place by the same network with run-time loops.  No barrier: a lane
//                       touches its own column only.  P * 256 B of LDS a workgroup: 32 KB or 64 KB.
//   exceed   out[t * out_stride + i] = the members whose key is >= thr.t[t]: k_members_exceed streams the planes once with a
//            counter per threshold in registers, up to MEMBERS_RANKS_MAX thresholds a pass.
//
// Cells that need no sort: where the caller's accumulators say so -- skip.zero[cell] == 0: every member's key is skip.zero_key;
// skip.never[cell] == 0: every member's key is MEMBERS_NEVER -- the planes of the cell are not read (8 B or 4 B of accumulator
// instead of 4 * M B), and a wavefront whose 64 cells are all of that kind sorts nothing.  The results are those of the sort.
//
// Every kernel loops over its cells with a grid stride; the enqueue functions take the largest grid from the caller.
#pragma once
#include <stdint.h>

#define MEMBERS_MAX 256u
#define MEMBERS_RANKS_MAX 16u
#define MEMBERS_NEVER 0xFFFFFFFFu
#define MEMBERS_REG_MAX 64u         // up to here the register kernels, beyond it the LDS kernels
#define MEMBERS_TPB 256u            // the register and the exceedance kernels; the LDS kernels run one wavefront a workgroup

struct MemberRanks { uint32_t n; uint32_t r[MEMBERS_RANKS_MAX]; };                 // n in 1..MEMBERS_RANKS_MAX, r[q] < M
struct MemberThresholds { uint32_t n; uint32_t none; uint32_t t[MEMBERS_RANKS_MAX]; };   // keys; bit q of none: no key reaches threshold q
struct MemberSkip {
    const unsigned long long *zero; uint32_t zero_key;     // nullptr: unknown
    const uint32_t *never;                                 // nullptr: unknown
};

// A signed value as a key whose unsigned order is the signed order, and back.
__host__ __device__ static inline uint32_t members_key(int32_t v) { return (uint32_t)v ^ 0x80000000u; }
__host__ __device__ static inline int32_t members_unkey(uint32_t k) { return (int32_t)(k ^ 0x80000000u); }

// The padded size the kernels sort for M members: 8, 16, 32, 64, 128 or 256.
__host__ __device__ static inline uint32_t members_padded(uint32_t m)
{
    uint32_t p = 8u;
    while (p < m) p <<= 1;
    return p;
}

// Thresholds as the caller states them, as keys: signed values flipped, unsigned ones clamped to the keys there are.  A threshold
// above every key is met by nobody (its bit of `none`) -- but by the members at MEMBERS_NEVER where that value stands for "never"
// (has_never), which are >= every threshold.  n in 1..MEMBERS_RANKS_MAX.
static inline MemberThresholds members_threshold_keys(const int64_t *thresholds, uint32_t n, bool is_signed, bool has_never)
{
    MemberThresholds k = MemberThresholds();
    k.n = n;
    for (uint32_t q = 0u; q < n && q < MEMBERS_RANKS_MAX; ++q) {
        const int64_t t = thresholds[q];
        if (is_signed) {
            if (t > (int64_t)INT32_MAX) k.none |= 1u << q;
            else k.t[q] = t < (int64_t)INT32_MIN ? 0u : members_key((int32_t)t);
        } else if (t > (int64_t)0xFFFFFFFFll) {
            if (has_never) k.t[q] = MEMBERS_NEVER; else k.none |= 1u << q;
        } else {
            k.t[q] = t < 0 ? 0u : (uint32_t)t;
        }
    }
    return k;
}

// The ranks of a call as the kernels take them: false where there are none, too many, or one that is not below `kept`
// (*bad_rank says which of the two it was).
static inline bool members_rank_list(const uint32_t *ranks, uint32_t n, uint32_t kept, MemberRanks *out, bool *bad_rank)
{
    *bad_rank = false;
    if (!ranks || n == 0u || n > MEMBERS_RANKS_MAX) return false;
    *out = MemberRanks();
    out->n = n;
    for (uint32_t q = 0u; q < n; ++q) {
        if (ranks[q] >= kept) { *bad_rank = true; return false; }
        out->r[q] = ranks[q];
    }
    return true;
}

// What the accumulators say about a cell: true and *key = every member's key, or false.
__device__ __forceinline__ bool members_trivial(const MemberSkip &skip, uint64_t cell, uint32_t *key)
{
    if (skip.never && skip.never[cell] == 0u) { *key = MEMBERS_NEVER; return true; }
    if (skip.zero && skip.zero[cell] == 0ull) { *key = skip.zero_key; return true; }
    return false;
}

template <uint32_t P>
__global__ __launch_bounds__(MEMBERS_TPB) void k_members_select_reg(const uint32_t *planes, uint64_t plane_stride, uint32_t M, uint64_t first_cell, uint64_t n_cells,
                                                                    MemberSkip skip, MemberRanks ranks, uint32_t *out, uint64_t out_stride)
{
    const uint64_t stride = (uint64_t)gridDim.x * MEMBERS_TPB;
    // (every lane of a wavefront makes the same trips: the ballot below is taken by all 64)
    for (uint64_t i0 = (uint64_t)blockIdx.x * MEMBERS_TPB; i0 < n_cells; i0 += stride) {
        const uint64_t i = i0 + threadIdx.x;
        const bool live = i < n_cells;
        uint32_t fill = MEMBERS_NEVER;
        const bool sort = live && !members_trivial(skip, first_cell + i, &fill);
        uint32_t v[P];
        if (__any(sort)) {
            const uint32_t *p = planes + first_cell + i;
#pragma unroll
            for (uint32_t m = 0u; m < P; ++m) v[m] = sort && m < M ? p[(uint64_t)m * plane_stride] : MEMBERS_NEVER;
#pragma unroll
            for (uint32_t k = 2u; k <= P; k <<= 1) {
#pragma unroll
                for (uint32_t j = k >> 1; j > 0u; j >>= 1) {
#pragma unroll
                    for (uint32_t a = 0u; a < P; ++a) {
                        const uint32_t b = a ^ j;
                        if (b > a) {
                            const uint32_t lo = min(v[a], v[b]), hi = max(v[a], v[b]);
                            const bool up = (a & k) == 0u;
                            v[a] = up ? lo : hi; v[b] = up ? hi : lo;
                        }
                    }
                }
            }
        }
        if (!live) continue;
        for (uint32_t q = 0u; q < ranks.n; ++q) {
            uint32_t x = fill;
            if (sort) {
                const uint32_t r = ranks.r[q];
#pragma unroll
                for (uint32_t m = 0u; m < P; ++m) x = m == r ? v[m] : x;
            }
            out[(uint64_t)q * out_stride + i] = x;
        }
    }
}

template <uint32_t P>
__global__ __launch_bounds__(64) void k_members_select_lds(const uint32_t *planes, uint64_t plane_stride, uint32_t M, uint64_t first_cell, uint64_t n_cells,
                                                           MemberSkip skip, MemberRanks ranks, uint32_t *out, uint64_t out_stride)
{
    __shared__ uint32_t s[P * 64u];
    const uint32_t lane = threadIdx.x;
    uint32_t *col = s + lane;                                      // key m of the lane's cell: col[m * 64]
    for (uint64_t i0 = (uint64_t)blockIdx.x * 64u; i0 < n_cells; i0 += (uint64_t)gridDim.x * 64u) {
        const uint64_t i = i0 + lane;
        const bool live = i < n_cells;
        uint32_t fill = MEMBERS_NEVER;
        const bool sort = live && !members_trivial(skip, first_cell + i, &fill);
        if (__any(sort)) {
            const uint32_t *p = planes + first_cell + i;
#pragma unroll 8
            for (uint32_t m = 0u; m < P; ++m) col[m * 64u] = sort && m < M ? p[(uint64_t)m * plane_stride] : MEMBERS_NEVER;
            for (uint32_t k = 2u; k <= P; k <<= 1) {
                for (uint32_t j = k >> 1; j > 0u; j >>= 1) {
#pragma unroll 4
                    for (uint32_t t = 0u; t < P / 2u; ++t) {       // the pair (a, a | j): a runs over the indices with bit j clear
                        const uint32_t a = ((t & ~(j - 1u)) << 1) | (t & (j - 1u)), b = a | j;
                        const uint32_t x = col[a * 64u], y = col[b * 64u];
                        const uint32_t lo = min(x, y), hi = max(x, y);
                        const bool up = (a & k) == 0u;
                        col[a * 64u] = up ? lo : hi; col[b * 64u] = up ? hi : lo;
                    }
                }
            }
        }
        if (!live) continue;
        for (uint32_t q = 0u; q < ranks.n; ++q) out[(uint64_t)q * out_stride + i] = sort ? col[ranks.r[q] * 64u] : fill;
    }
}

__global__ __launch_bounds__(MEMBERS_TPB) void k_members_exceed(const uint32_t *planes, uint64_t plane_stride, uint32_t M, uint64_t first_cell, uint64_t n_cells,
                                                                MemberSkip skip, MemberThresholds thr, uint32_t *out, uint64_t out_stride)
{
    const uint64_t stride = (uint64_t)gridDim.x * MEMBERS_TPB;
    for (uint64_t i = (uint64_t)blockIdx.x * MEMBERS_TPB + threadIdx.x; i < n_cells; i += stride) {
        uint32_t cnt[MEMBERS_RANKS_MAX];
#pragma unroll
        for (uint32_t t = 0u; t < MEMBERS_RANKS_MAX; ++t) cnt[t] = 0u;
        uint32_t fill;
        if (members_trivial(skip, first_cell + i, &fill)) {
#pragma unroll
            for (uint32_t t = 0u; t < MEMBERS_RANKS_MAX; ++t) cnt[t] = fill >= thr.t[t] ? M : 0u;
        } else {
            const uint32_t *p = planes + first_cell + i;
#pragma unroll 4
            for (uint32_t m = 0u; m < M; ++m) {
                const uint32_t x = p[(uint64_t)m * plane_stride];
#pragma unroll
                for (uint32_t t = 0u; t < MEMBERS_RANKS_MAX; ++t) cnt[t] += x >= thr.t[t] ? 1u : 0u;
            }
        }
#pragma unroll
        for (uint32_t t = 0u; t < MEMBERS_RANKS_MAX; ++t)
            if (t < thr.n) out[(uint64_t)t * out_stride + i] = (thr.none >> t) & 1u ? 0u : cnt[t];
    }
}

// The largest grids the kernels are worth: the caller's bound clips them.
const uint32_t MEMBERS_GRID = 4096u;

static inline uint32_t members_grid(uint64_t items, uint32_t per_block, uint32_t max_blocks)
{
    const uint64_t g = (items + per_block - 1u) / per_block;
    return (uint32_t)(g < 1u ? 1u : g < max_blocks ? g : max_blocks);
}

// The cells a workgroup takes per trip for M members: what a caller's record of trips divides by.
static inline uint32_t members_select_per_block(uint32_t M) { return M <= MEMBERS_REG_MAX ? MEMBERS_TPB : 64u; }

// The launch that selects the ranks of the cells [first_cell, first_cell + n_cells) on `stream`.  M in 1..MEMBERS_MAX, every
// rank < M (the caller checks both); out holds ranks.n * out_stride words.
static inline void members_select_enqueue(const uint32_t *planes, uint64_t plane_stride, uint32_t M, uint64_t first_cell, uint64_t n_cells, const MemberSkip &skip,
                                          const MemberRanks &ranks, uint32_t *out, uint64_t out_stride, hipStream_t stream, uint32_t max_blocks = MEMBERS_GRID)
{
    if (!n_cells || !M || M > MEMBERS_MAX) return;
    const dim3 grid(members_grid(n_cells, members_select_per_block(M), max_blocks));
#define MEMBERS_LAUNCH(kernel, tpb) hipLaunchKernelGGL(kernel, grid, dim3(tpb), 0, stream, planes, plane_stride, M, first_cell, n_cells, skip, ranks, out, out_stride)
    switch (members_padded(M)) {
    case 8u: MEMBERS_LAUNCH(k_members_select_reg<8u>, MEMBERS_TPB); break;
    case 16u: MEMBERS_LAUNCH(k_members_select_reg<16u>, MEMBERS_TPB); break;
    case 32u: MEMBERS_LAUNCH(k_members_select_reg<32u>, MEMBERS_TPB); break;
    case 64u: MEMBERS_LAUNCH(k_members_select_reg<64u>, MEMBERS_TPB); break;
    case 128u: MEMBERS_LAUNCH(k_members_select_lds<128u>, 64u); break;
    default: MEMBERS_LAUNCH(k_members_select_lds<256u>, 64u); break;
    }
#undef MEMBERS_LAUNCH
}

// The launch that counts the members at or above each threshold; out holds thr.n * out_stride words.
static inline void members_exceed_enqueue(const uint32_t *planes, uint64_t plane_stride, uint32_t M, uint64_t first_cell, uint64_t n_cells, const MemberSkip &skip,
                                          const MemberThresholds &thr, uint32_t *out, uint64_t out_stride, hipStream_t stream, uint32_t max_blocks = MEMBERS_GRID)
{
    if (!n_cells || !M) return;
    hipLaunchKernelGGL(k_members_exceed, dim3(members_grid(n_cells, MEMBERS_TPB, max_blocks)), dim3(MEMBERS_TPB), 0, stream,
                       planes, plane_stride, M, first_cell, n_cells, skip, thr, out, out_stride);
}
