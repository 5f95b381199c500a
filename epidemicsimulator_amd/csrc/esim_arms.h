// esim_arms.h -- the kept members of an ensemble read as a grid of policies: S replicates of A arms run on common
// random numbers, slot = s * A + a.  Per cell and arm: in how many replicates the arm is the best one, in how many it alone,
// what it loses against the best arm of the same replicate, and its sum; per member the sum over the window.  Built like
// esim_depth.h and esim_dist.h, on esim_members.h and on nothing else, so that a probe can include this header alone
// (tests/native/arms_probe.hip).
//
// The input is the store of esim_members.h: M = S * A planes [member][cell] of keys, plane m at planes + m * plane_stride, a
// window [first_cell, first_cell + n_cells).  A key equal to MEMBERS_NEVER is replaced by `never_as` first.  With k[s][a] the key
// of slot s * A + a and b[s] the smallest of k[s][.] (the largest with `maximize`), out.X[a * n_cells + i] for cell first_cell + i:
//   best     the replicates with k[s][a] == b[s]                      sole    those of them in which no other arm attains b[s]
//   regret   the sum over s of |k[s][a] - b[s]|, in 64 bits           sum     the sum over s of k[s][a], in 64 bits
// and totals[s * A + a] the sum of k[s][a] over the cells of the window that are READ, modulo 2^64.
//
// k_arms<P>, P = 2, 4, 8, 16 the arms padded (A = 1 runs as P = 2): a lane owns a cell, a wavefront 64 consecutive cells.  A
// run-time loop goes over the replicates; inside it the P keys of one replicate sit in registers with constant indices, every
// key is read once, coalesced, and only one replicate is held at a time -- so M up to 256 needs no LDS tile and no second family
// of kernels.  With `maximize` the keys are complemented behind the replacement, so that one minimising path serves both senses:
// ~b = min ~k, the ties are the same and ~k - ~b = b - k.
//   accumulators  per arm best and sole (32 bits) and regret (64 bits), and ONE 64-bit sum of b[s] per lane: k = b + (k - b), so
//                 sum[a] = sum of b + regret[a] when minimising and sum of b - regret[a] when maximising -- no sum per arm.
//   padding       the slots from A on hold 0xFFFFFFFF, which leaves the minimum alone; where every real arm holds 0xFFFFFFFF too
//                 (ESIM_NEVER kept as it is, or 0 under `maximize`) they would tie with it, so ties are counted over a < A only.
//   settled cells a cell that members_trivial settles is not read: best = S, sole = 0 (S with one arm), regret = 0, sum = S * fill'
//                 with fill' the one key after the replacement.  fill' belongs into every member's total alike: the lanes sum it
//                 into stats[ARMS_COMMON], once per wavefront at the kernel's end, and the caller adds that to every total.
//   totals        in the same pass, the keys being in registers: per (replicate, arm) a wavefront sum -- the halves of the key
//                 apart, 16 bits each, so that 64 of them fit 32 bits and the six steps are v_add_u32 with a DPP operand -- and
//                 one LDS atomic per (wavefront, member) and trip into the workgroup's table of M 64-bit words; the table goes
//                 to `totals` with one global atomic per (workgroup, member) at the kernel's end.
//   stats         stats[ARMS_LIVE] the cells read, stats[ARMS_COMMON] as above; zeroed by the caller, like totals.
//
// The kernel loops with a grid stride in which every lane of a wavefront makes the same trips (the DPP sums and the ballot
// need all 64); arms_enqueue takes the largest grid from the caller.
#pragma once
#include "esim_members.h"

#define ARMS_MAX 16u
#define ARMS_STATS 2u
#define ARMS_LIVE 0
#define ARMS_COMMON 1

struct ArmsOut {
    uint32_t *best, *sole;                       // [A * n_cells] each, or nullptr
    unsigned long long *regret, *sum;            // [A * n_cells] each, or nullptr
    unsigned long long *totals;                  // [M], zeroed, or nullptr
    unsigned long long *stats;                   // [ARMS_STATS], zeroed
};

// The arms as the kernels pad them: 2, 4, 8 or 16.
__host__ __device__ static inline uint32_t arms_padded(uint32_t a)
{
    uint32_t p = 2u;
    while (p < a) p <<= 1;
    return p;
}

// The sum of v over the 64 lanes of the wavefront, in lane 63; v < 2^26 in every lane, and every lane takes part.
__device__ __forceinline__ uint32_t arms_wave_sum(uint32_t v)
{
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xF, 0xF, false);      // row_shr:1
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xF, 0xF, false);      // row_shr:2
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xF, 0xF, false);      // row_shr:4
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xF, 0xF, false);      // row_shr:8: lane 15 of a row holds the row
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xA, 0xF, false);      // row_bcast:15 into rows 1 and 3
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xC, 0xF, false);      // row_bcast:31 into rows 2 and 3
    return v;
}

template <uint32_t P>
__global__ __launch_bounds__(MEMBERS_TPB) void k_arms(const uint32_t *planes, uint64_t plane_stride, uint32_t A, uint32_t S, uint64_t first_cell, uint64_t n_cells,
                                                      MemberSkip skip, uint32_t maximize, uint32_t never_as, ArmsOut out)
{
    __shared__ unsigned long long s_tot[MEMBERS_MAX];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t flip = maximize ? 0xFFFFFFFFu : 0u;
    constexpr uint32_t U = P >= 8u ? 1u : 8u / P;                  // the replicates read together: 8 loads a lane in flight, 16 for P = 16
    if (out.totals) {
        for (uint32_t m = tid; m < MEMBERS_MAX; m += MEMBERS_TPB) s_tot[m] = 0ull;
        __syncthreads();
    }
    unsigned long long common = 0ull;            // the lane's settled cells: the sum of their one key
    uint32_t n_read = 0u;                        // (the same in every lane of the wavefront)
    const uint64_t stride = (uint64_t)gridDim.x * MEMBERS_TPB;
    // (every lane of a wavefront makes the same trips)
    for (uint64_t i0 = (uint64_t)blockIdx.x * MEMBERS_TPB; i0 < n_cells; i0 += stride) {
        const uint64_t i = i0 + tid;
        const bool live = i < n_cells;
        uint32_t fill = 0u;
        const bool read = live && !members_trivial(skip, first_cell + i, &fill);
        fill = fill == MEMBERS_NEVER ? never_as : fill;
        uint32_t best[P], sole[P];
        unsigned long long regret[P], bsum = 0ull;
#pragma unroll
        for (uint32_t a = 0u; a < P; ++a) { best[a] = 0u; sole[a] = 0u; regret[a] = 0ull; }
        const unsigned long long votes = __ballot(read);
        if (votes) {
            n_read += (uint32_t)__popcll(votes);
            const uint32_t *p = planes + first_cell + i;
            for (uint32_t s0 = 0u; s0 < S; s0 += U) {
                uint32_t k[U][P];                                  // U replicates' loads in flight
#pragma unroll
                for (uint32_t u = 0u; u < U; ++u) {
#pragma unroll
                    for (uint32_t a = 0u; a < P; ++a) {
                        uint32_t x = 0xFFFFFFFFu;
                        if (read && a < A && s0 + u < S) {
                            x = p[(uint64_t)((s0 + u) * A + a) * plane_stride];
                            x = (x == MEMBERS_NEVER ? never_as : x) ^ flip;
                        }
                        k[u][a] = x;
                    }
                }
#pragma unroll
                for (uint32_t u = 0u; u < U; ++u) {
                    const uint32_t s = s0 + u;
                    if (s >= S) break;                             // (uniform)
                    uint32_t b = k[u][0];
#pragma unroll
                    for (uint32_t a = 1u; a < P; ++a) b = min(b, k[u][a]);
                    uint32_t ties = 0u;
#pragma unroll
                    for (uint32_t a = 0u; a < P; ++a) ties += a < A && k[u][a] == b ? 1u : 0u;
#pragma unroll
                    for (uint32_t a = 0u; a < P; ++a) {
                        const bool eq = a < A && k[u][a] == b;
                        best[a] += eq ? 1u : 0u;
                        sole[a] += eq && ties == 1u ? 1u : 0u;
                        regret[a] += (unsigned long long)(k[u][a] - b);
                    }
                    bsum += (unsigned long long)(b ^ flip);
                    if (out.totals) {
#pragma unroll
                        for (uint32_t a = 0u; a < P; ++a) {
                            if (a < A) {                           // (uniform)
                                const uint32_t x = read ? k[u][a] ^ flip : 0u;
                                const uint32_t lo = arms_wave_sum(x & 0xFFFFu), hi = arms_wave_sum(x >> 16);
                                const unsigned long long t = ((unsigned long long)hi << 16) + lo;
                                if (lane == 63u && t) atomicAdd(&s_tot[s * A + a], t);
                            }
                        }
                    }
                }
            }
        }
        if (!live) continue;
        if (!read) common += fill;
#pragma unroll
        for (uint32_t a = 0u; a < P; ++a) {
            if (a < A) {
                const uint64_t at = (uint64_t)a * n_cells + i;
                if (out.best) out.best[at] = read ? best[a] : S;
                if (out.sole) out.sole[at] = read ? sole[a] : A == 1u ? S : 0u;
                if (out.regret) out.regret[at] = read ? regret[a] : 0ull;
                if (out.sum) out.sum[at] = !read ? (unsigned long long)S * fill : maximize ? bsum - regret[a] : bsum + regret[a];
            }
        }
    }
    // (behind the loop every lane is here again)
    for (uint32_t d = 32u; d > 0u; d >>= 1) common += __shfl_down(common, d, 64);
    if (lane == 0u) {
        if (n_read) atomicAdd(out.stats + ARMS_LIVE, (unsigned long long)n_read);
        if (common) atomicAdd(out.stats + ARMS_COMMON, common);
    }
    if (out.totals) {
        __syncthreads();
        for (uint32_t m = tid; m < A * S; m += MEMBERS_TPB)
            if (s_tot[m]) atomicAdd(out.totals + m, s_tot[m]);
    }
}

// What the caller does with the totals once they are on the host: the settled cells' keys into every member's, modulo 2^64.
static inline void arms_totals_finish(uint64_t *totals, uint32_t M, const uint64_t *stats)
{
    for (uint32_t m = 0u; m < M; ++m) totals[m] += stats[ARMS_COMMON];
}

// The launch that fills `out` for the window on `stream`: A in 1..ARMS_MAX, M = A * S in 1..MEMBERS_MAX (the caller checks both).
static inline void arms_enqueue(const uint32_t *planes, uint64_t plane_stride, uint32_t A, uint32_t S, uint64_t first_cell, uint64_t n_cells, const MemberSkip &skip,
                                bool maximize, uint32_t never_as, const ArmsOut &out, hipStream_t stream, uint32_t max_blocks = MEMBERS_GRID)
{
    if (!n_cells || !A || A > ARMS_MAX || !S || (uint64_t)A * S > MEMBERS_MAX) return;
    const dim3 grid(members_grid(n_cells, MEMBERS_TPB, max_blocks));
#define ARMS_LAUNCH(P) hipLaunchKernelGGL(k_arms<P>, grid, dim3(MEMBERS_TPB), 0, stream, planes, plane_stride, A, S, first_cell, n_cells, skip, maximize ? 1u : 0u, never_as, out)
    switch (arms_padded(A)) {
    case 2u: ARMS_LAUNCH(2u); break;
    case 4u: ARMS_LAUNCH(4u); break;
    case 8u: ARMS_LAUNCH(8u); break;
    default: ARMS_LAUNCH(16u); break;
    }
#undef ARMS_LAUNCH
}
