// Ranking the riders of a bus route by (Philox key, id): nothing but integers and lane intrinsics, so that a probe can include
// this header alone (tests/native/rank_probe.hip).
//
// The rank of rider `me` is the number of riders i with (key_i, i) < (key_me, me).  Said like that it costs two compares, a
// compare of the indices and a mask operation per rider looked at.  Keys are 32 random bits, so two riders of one route share
// a key about once in 10^7 pairs: both forms below count `key_i < key_me` only -- one broadcast or LDS read, one compare, one
// add-with-carry per rider -- and make up for the ties in a way that costs nothing per rider:
//   - the wavefront form checks that the 64 ranks it found are distinct (they are exactly when no two riders share a key) and
//     takes the exact loop when they are not;
//   - the workgroup form marks every rank it hands out in a bit set in LDS; a rank handed out twice sends the workgroup through
//     the exact loop.
#pragma once
#include <stdint.h>

// The exact loop: (key, lane) order, riders 0 .. n-1 in lanes 0 .. n-1.  n is wavefront-uniform.
__device__ __forceinline__ uint32_t rank_wave64_exact(uint32_t key, uint32_t lane, uint32_t n)
{
    uint32_t rank = 0u;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t ki = (uint32_t)__builtin_amdgcn_readlane((int)key, (int)i);   // i is uniform: a scalar broadcast
        rank += ki < key || (ki == key && i < lane);                                 // ids ascend with the lane
    }
    return rank;
}

// Wavefront form: riders 0 .. sz-1 (sz <= 64, the same in every lane) sit in lanes 0 .. sz-1 with their keys; returns to
// lane < sz the number of riders i < sz with (key_i, i) < (key, lane).  What lanes >= sz get is not a rank.  Has to be called
// by all 64 lanes of the wavefront together.  *exact_taken (if given) is set to 1 when the keys had a tie and the exact loop
// ran, to 0 otherwise.
__device__ __forceinline__ uint32_t rank_wave64(uint32_t key, uint32_t lane, uint32_t sz, uint32_t *exact_taken = nullptr)
{
    // sz as a scalar: the loop is steered by scalar compares and never touches exec
    uint32_t n = (uint32_t)__builtin_amdgcn_readfirstlane((int)sz);
    n = n < 64u ? n : 64u;
    // the lanes behind the route hold the largest key: no key is smaller than it, so they add nothing to anybody's count and the
    // loop can run in steps of four past sz
    const uint32_t kk = lane < n ? key : 0xFFFFFFFFu;
    uint32_t rank = 0u;
    for (uint32_t i = 0; i < n; i += 4u) {
        const uint32_t k0 = (uint32_t)__builtin_amdgcn_readlane((int)kk, (int)i);
        const uint32_t k1 = (uint32_t)__builtin_amdgcn_readlane((int)kk, (int)(i + 1u));
        const uint32_t k2 = (uint32_t)__builtin_amdgcn_readlane((int)kk, (int)(i + 2u));
        const uint32_t k3 = (uint32_t)__builtin_amdgcn_readlane((int)kk, (int)(i + 3u));
        rank += k0 < key;
        rank += k1 < key;
        rank += k2 < key;
        rank += k3 < key;
    }
    // Without a tie the ranks of lanes 0 .. n-1 are a permutation of 0 .. n-1; two riders with one key have counted the same
    // riders and hold the same rank.  Every lane sends its number to the lane its rank names (the lanes behind the route to
    // themselves) and asks that lane whose number arrived: with a permutation everybody gets its own back, of two lanes with
    // one rank at most one does.
    if (lane >= n) rank = lane;
    const int got = __builtin_amdgcn_ds_permute((int)(rank << 2), (int)lane);
    const int back = __builtin_amdgcn_ds_bpermute((int)(rank << 2), got);
    const bool tie = __builtin_amdgcn_ballot_w64((uint32_t)back != lane) != 0ull;
    if (exact_taken) *exact_taken = tie ? 1u : 0u;
    if (tie) rank = rank_wave64_exact(key, lane, n);
    return rank;
}

// Workgroup form: the riders' keys lie in LDS, s_key[q], q < sz (sz the same in every thread).
// rank_block: the number of riders q < sz with key_q < key -- the rank of a rider with that key if no other rider shares it.
__device__ __forceinline__ uint32_t rank_block(const uint32_t *s_key, uint32_t key, uint32_t sz)
{
    uint32_t rank = 0u;
#pragma unroll 4
    for (uint32_t q = 0; q < sz; ++q) rank += s_key[q] < key;
    return rank;
}
// rank_seen: marks `rank` (< sz) in the bit set s_seen ((sz + 31) / 32 words of LDS, zeroed by the caller before a barrier) and
// says whether it was marked already.  Riders who share a key were given the same rank by rank_block: if any thread of the
// workgroup is told so, all ranks of the route are to be taken from rank_block_exact instead.
__device__ __forceinline__ bool rank_seen(uint32_t *s_seen, uint32_t rank)
{
    const uint32_t bit = 1u << (rank & 31u);
    return (atomicOr(&s_seen[rank >> 5], bit) & bit) != 0u;
}
// rank_block_exact: the number of riders q < sz with (key_q, q) < (key, i).
__device__ __forceinline__ uint32_t rank_block_exact(const uint32_t *s_key, uint32_t key, uint32_t i, uint32_t sz)
{
    uint32_t rank = 0u;
    for (uint32_t q = 0; q < sz; ++q) { const uint32_t kq = s_key[q]; rank += kq < key || (kq == key && q < i); }
    return rank;
}
