// rank_probe.hip -- the two ranking routines of epidemicsimulator_amd/csrc/esim_rank.h on their own: keys and sz from the host, the
// ranks of the form asked for back, and whether the exact path (keys with a tie) was taken.  tests/test_rank_gpu.py compiles
// this file, loads it with ctypes and compares with numpy.lexsort.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "esim_rank.h"

#define PROBE_MAX 2048u            // riders of the workgroup form (CHUNK_ROUTE_MAX of the library)
#define PROBE_TPB 256u

// one wavefront: rider `lane` in lane `lane`, as route_pair_small holds them
__global__ __launch_bounds__(64) void k_rank_wave(const uint32_t *keys, uint32_t sz, uint32_t *ranks, uint32_t *exact)
{
    const uint32_t lane = threadIdx.x;
    const uint32_t key = lane < sz ? keys[lane] : 0u;
    uint32_t taken = 0u;
    const uint32_t rank = rank_wave64(key, lane, sz, &taken);
    if (lane < sz) ranks[lane] = rank;
    if (lane == 0u) *exact = taken;
}

// one workgroup: the keys in LDS, every thread the riders tid, tid + PROBE_TPB, ..., as route_pair_big walks them
__global__ __launch_bounds__(PROBE_TPB) void k_rank_block(const uint32_t *keys, uint32_t sz, uint32_t *ranks, uint32_t *exact)
{
    __shared__ uint32_t s_key[PROBE_MAX];
    __shared__ uint32_t s_seen[PROBE_MAX / 32u];
    for (uint32_t i = threadIdx.x; i < sz; i += PROBE_TPB) s_key[i] = keys[i];
    for (uint32_t i = threadIdx.x; i < (sz + 31u) / 32u; i += PROBE_TPB) s_seen[i] = 0u;
    __syncthreads();
    int tie = 0;
    for (uint32_t i = threadIdx.x; i < sz; i += PROBE_TPB) {
        const uint32_t rank = rank_block(s_key, s_key[i], sz);
        tie |= rank_seen(s_seen, rank) ? 1 : 0;
        ranks[i] = rank;
    }
    const int any_tie = __syncthreads_or(tie);
    if (any_tie)
        for (uint32_t i = threadIdx.x; i < sz; i += PROBE_TPB) ranks[i] = rank_block_exact(s_key, s_key[i], i, sz);
    if (threadIdx.x == 0u) *exact = any_tie ? 1u : 0u;
}

// form 0: wavefront (1 <= sz <= 64), form 1: workgroup (1 <= sz <= PROBE_MAX).  Returns 0, -1 for arguments out of range, or the
// HIP error.
extern "C" int rank_probe(const uint32_t *keys, uint32_t sz, int form, uint32_t *ranks, uint32_t *exact)
{
    if (!keys || !ranks || !exact || sz == 0u || (form != 0 && form != 1) || sz > (form == 0 ? 64u : PROBE_MAX)) return -1;
    uint32_t *d_keys = nullptr, *d_out = nullptr;                              // d_out: sz ranks, then the flag
    hipError_t e = hipMalloc(&d_keys, sz * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc(&d_out, (sz + 1u) * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMemcpy(d_keys, keys, sz * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(d_out, 0xFF, (sz + 1u) * sizeof(uint32_t));
    if (e == hipSuccess) {
        if (form == 0) k_rank_wave<<<1, 64>>>(d_keys, sz, d_out, d_out + sz);
        else k_rank_block<<<1, PROBE_TPB>>>(d_keys, sz, d_out, d_out + sz);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(ranks, d_out, sz * sizeof(uint32_t), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(exact, d_out + sz, sizeof(uint32_t), hipMemcpyDeviceToHost);
    (void)hipFree(d_keys); (void)hipFree(d_out);
    return (int)e;
}
