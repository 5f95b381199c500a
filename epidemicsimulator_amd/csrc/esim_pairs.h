// esim_pairs.h -- sparse counts of distinct 64-bit keys on the device: aggregate, compact, sort.  Nothing but integers,
// atomics and lane intrinsics, so that a probe can include this header alone (tests/native/pairs_probe.hip).
//
//   insert   pair_insert adds one key to an open-addressing table of `cap` slots (a power of two): a 64-bit finaliser picks the
//            slot, a linear probe of at most `cap` tries finds the key or an empty slot, a 64-bit atomicCAS claims it and an
//            atomicAdd counts.  A key that finds no slot bumps *overflow and is dropped: the loop cannot spin.  pair_add is the
//            same with a change other than +1 (esim_curves.h: the net change of a curve at a step).
//   compact  k_pairs_compact, a lane per slot: the occupied slots of a wavefront are counted with one ballot and reserved with
//            one atomic, and their (key, count) pairs go to a dense array -- in the order the wavefronts happened to arrive.
//            k_pairs_compact_min keeps only the slots that count at least min_count.
//   sort     ascending by key, which makes the output canonical.  Keys are unique after aggregation, so a bitonic network is
//            enough and stability does not arise.  The dense array is padded to a power of two with PAIR_EMPTY, which sorts
//            last.  k_pairs_sort_tile runs every step whose stride fits a tile of PAIR_SORT_TILE pairs in LDS,
//            k_pairs_sort_step one compare-exchange step in global memory for the larger strides.
//
// PAIR_EMPTY (~0ull) marks an empty slot and is no key: the callers never insert it.
#pragma once
#include <stdint.h>

#define PAIR_EMPTY (~0ull)
#define PAIR_TPB 256u
// Pairs a workgroup of k_pairs_sort_tile sorts in LDS: 2048 x (8 B key + 4 B count) = 24 KB, so that six workgroups share the
// 160 KB of a compute unit and its 24 wavefronts keep the LDS pipeline busy; every doubling saves one global step per outer
// stage, and the next one (48 KB, three workgroups) would halve the wavefronts that hide each other's barriers.
#ifndef PAIR_SORT_TILE
#define PAIR_SORT_TILE 2048u
#endif

struct PairTable {
    unsigned long long *key;    // [cap] filled with PAIR_EMPTY by the caller
    uint32_t *cnt;              // [cap] zeroed by the caller
    uint32_t cap;               // a power of two
    uint32_t *overflow;         // keys dropped because the table was full, zeroed by the caller
};

// The finaliser of MurmurHash3 (fmix64): every input bit reaches every output bit.
__device__ __forceinline__ uint64_t pair_mix(uint64_t k)
{
    k ^= k >> 33; k *= 0xFF51AFD7ED558CCDull;
    k ^= k >> 33; k *= 0xC4CEB9FE1A85EC53ull;
    return k ^ (k >> 33);
}

// Adds `delta` to the count of `key` (!= PAIR_EMPTY), modulo 2^32: a key may end at a net count of 0 and still holds its slot.
// A slot's key is written once and never changes, so the plain read in front of the CAS can only be stale in one way -- empty
// where a key stands by now --, and then the CAS returns that key.
__device__ __forceinline__ void pair_add(const PairTable &t, uint64_t key, uint32_t delta)
{
    const uint32_t mask = t.cap - 1u;
    uint32_t slot = (uint32_t)pair_mix(key) & mask;
    for (uint32_t tries = 0u; tries < t.cap; ++tries, slot = (slot + 1u) & mask) {
        unsigned long long cur = __atomic_load_n(&t.key[slot], __ATOMIC_RELAXED);
        if (cur == PAIR_EMPTY) {
            cur = atomicCAS(&t.key[slot], PAIR_EMPTY, (unsigned long long)key);
            if (cur == PAIR_EMPTY) cur = key;                                   // claimed
        }
        if (cur == key) { atomicAdd(&t.cnt[slot], delta); return; }
    }
    atomicAdd(t.overflow, 1u);
}

// Counts `key` (!= PAIR_EMPTY) once.
__device__ __forceinline__ void pair_insert(const PairTable &t, uint64_t key) { pair_add(t, key, 1u); }

// The occupied slots, dense: out_key / out_cnt [*n_out ...), *n_out zeroed by the caller; the arrays hold at least as many pairs
// as the table can (the callers size them by what can have been inserted).  Every lane of a wavefront makes the same trips.
__global__ __launch_bounds__(PAIR_TPB) void k_pairs_compact(PairTable t, unsigned long long *out_key, uint32_t *out_cnt, uint32_t out_cap, uint32_t *n_out)
{
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t s0 = (uint64_t)blockIdx.x * PAIR_TPB; s0 < (uint64_t)t.cap; s0 += (uint64_t)gridDim.x * PAIR_TPB) {
        const uint64_t s = s0 + threadIdx.x;
        const unsigned long long k = s < (uint64_t)t.cap ? t.key[s] : PAIR_EMPTY;
        const bool full = k != PAIR_EMPTY;
        const unsigned long long m = __ballot(full);
        if (!m) continue;
        const uint32_t lead = (uint32_t)__ffsll((long long)m) - 1u;
        uint32_t base = 0u;
        if (lane == lead) base = atomicAdd(n_out, (uint32_t)__popcll(m));
        base = __shfl(base, lead, 64);
        const uint32_t at = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        if (full && at < out_cap) { out_key[at] = k; out_cnt[at] = t.cnt[s]; }
    }
}

// The same for the slots that count at least min_count (>= 1): a caller that wants only the keys seen several times keeps the
// dense array, and the sort behind it, as small as they are.  min_count 1 delivers what k_pairs_compact does.
__global__ __launch_bounds__(PAIR_TPB) void k_pairs_compact_min(PairTable t, uint32_t min_count, unsigned long long *out_key, uint32_t *out_cnt, uint32_t out_cap,
                                                                uint32_t *n_out)
{
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t s0 = (uint64_t)blockIdx.x * PAIR_TPB; s0 < (uint64_t)t.cap; s0 += (uint64_t)gridDim.x * PAIR_TPB) {
        const uint64_t s = s0 + threadIdx.x;
        const unsigned long long k = s < (uint64_t)t.cap ? t.key[s] : PAIR_EMPTY;
        const uint32_t n = k != PAIR_EMPTY ? t.cnt[s] : 0u;
        const bool full = k != PAIR_EMPTY && n >= min_count;
        const unsigned long long m = __ballot(full);
        if (!m) continue;
        const uint32_t lead = (uint32_t)__ffsll((long long)m) - 1u;
        uint32_t base = 0u;
        if (lane == lead) base = atomicAdd(n_out, (uint32_t)__popcll(m));
        base = __shfl(base, lead, 64);
        const uint32_t at = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        if (full && at < out_cap) { out_key[at] = k; out_cnt[at] = n; }
    }
}

// Compare-exchange of the pairs at i < l in a bitonic stage of block size k: ascending where bit k of the index is clear.
#define PAIR_CMP_SWAP(KEY, CNT, i, l, up)                                              \
    do {                                                                               \
        const unsigned long long a_ = (KEY)[i], b_ = (KEY)[l];                         \
        if ((a_ > b_) == (up)) {                                                       \
            (KEY)[i] = b_; (KEY)[l] = a_;                                              \
            const uint32_t c_ = (CNT)[i]; (CNT)[i] = (CNT)[l]; (CNT)[l] = c_;          \
        }                                                                              \
    } while (0)

// Every step of the stages k_first .. k_last (block sizes, powers of two) whose stride is below the tile: stage k_first from
// stride j_first down, the later ones from k / 2.  A workgroup holds tile number blockIdx.x of min(n, PAIR_SORT_TILE) pairs in
// LDS; n is a power of two and the grid has n / tile workgroups.  The caller passes
//   (2, tile, 1)        the whole sort of every tile, and with n <= PAIR_SORT_TILE of everything;
//   (k, k, tile / 2)    the tail of an outer stage k > tile, behind its global steps.
__global__ __launch_bounds__(PAIR_TPB) void k_pairs_sort_tile(unsigned long long *key, uint32_t *cnt, uint32_t n, uint32_t k_first, uint32_t k_last, uint32_t j_first)
{
    __shared__ unsigned long long s_key[PAIR_SORT_TILE];
    __shared__ uint32_t s_cnt[PAIR_SORT_TILE];
    const uint32_t tile = n < PAIR_SORT_TILE ? n : PAIR_SORT_TILE;
    const uint64_t base = (uint64_t)blockIdx.x * tile;
    if (base + tile > (uint64_t)n) return;                                       // (block-uniform)
    for (uint32_t i = threadIdx.x; i < tile; i += PAIR_TPB) { s_key[i] = key[base + i]; s_cnt[i] = cnt[base + i]; }
    __syncthreads();
    for (uint32_t k = k_first; k <= k_last && k != 0u; k <<= 1) {
        for (uint32_t j = k == k_first ? j_first : k >> 1; j > 0u; j >>= 1) {
            if (j < tile)
                for (uint32_t p = threadIdx.x; p < tile / 2u; p += PAIR_TPB) {
                    const uint32_t i = ((p & ~(j - 1u)) << 1) | (p & (j - 1u)), l = i + j;
                    const bool up = ((base + i) & (uint64_t)k) == 0ull;
                    PAIR_CMP_SWAP(s_key, s_cnt, i, l, up);
                }
            __syncthreads();
        }
    }
    for (uint32_t i = threadIdx.x; i < tile; i += PAIR_TPB) { key[base + i] = s_key[i]; cnt[base + i] = s_cnt[i]; }
}

// One step of stage k at stride j in global memory, a lane per pair of slots.
__global__ __launch_bounds__(PAIR_TPB) void k_pairs_sort_step(unsigned long long *key, uint32_t *cnt, uint32_t n, uint32_t k, uint32_t j)
{
    for (uint64_t p = (uint64_t)blockIdx.x * PAIR_TPB + threadIdx.x; p < (uint64_t)(n >> 1); p += (uint64_t)gridDim.x * PAIR_TPB) {
        const uint64_t i = ((p & ~(uint64_t)(j - 1u)) << 1) | (p & (uint64_t)(j - 1u)), l = i + j;
        const bool up = (i & (uint64_t)k) == 0ull;
        PAIR_CMP_SWAP(key, cnt, i, l, up);
    }
}

// The smallest power of two >= x (x <= 2^31), at least 1.
static inline uint32_t pair_pow2(uint64_t x)
{
    uint32_t p = 1u;
    while ((uint64_t)p < x && p < 0x80000000u) p <<= 1;
    return p;
}

// The launches that sort the first n_sort pairs (a power of two; the pairs behind the real ones hold PAIR_EMPTY) on `stream`.
static inline void pairs_sort_enqueue(unsigned long long *key, uint32_t *cnt, uint32_t n_sort, hipStream_t stream)
{
    if (n_sort < 2u) return;
    const uint32_t tile = n_sort < PAIR_SORT_TILE ? n_sort : PAIR_SORT_TILE, tiles = n_sort / tile;
    const uint32_t steps = (uint32_t)(((uint64_t)(n_sort >> 1) + PAIR_TPB - 1u) / PAIR_TPB);
    const uint32_t grid = steps < 1u ? 1u : steps > 16384u ? 16384u : steps;
    hipLaunchKernelGGL(k_pairs_sort_tile, dim3(tiles), dim3(PAIR_TPB), 0, stream, key, cnt, n_sort, 2u, tile, 1u);
    for (uint32_t k = tile << 1; k <= n_sort && k != 0u; k <<= 1) {
        for (uint32_t j = k >> 1; j >= tile; j >>= 1)
            hipLaunchKernelGGL(k_pairs_sort_step, dim3(grid), dim3(PAIR_TPB), 0, stream, key, cnt, n_sort, k, j);
        hipLaunchKernelGGL(k_pairs_sort_tile, dim3(tiles), dim3(PAIR_TPB), 0, stream, key, cnt, n_sort, k, k, tile >> 1);
    }
}
