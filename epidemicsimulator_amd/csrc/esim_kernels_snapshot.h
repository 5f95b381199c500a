// esim_kernels_snapshot.h -- forecast ensembles: the citizen words kept on the device (esim_snapshot) and put back
// (esim_rollback).  Everything else a snapshot holds is small and moves with device-to-device copies.  No stepping kernel is here.
#pragma once

// dst[0 .. n) = src[0 .. n): a pure stream over 4 B per citizen read and 4 B written, in the style of k_restart_words -- 16
// bytes per lane, a grid capped at 2048 workgroups that strides over the rest (both arrays come from hipMalloc, so they start on
// a 16-byte boundary, and both hold at least n words); the up to three words behind the last whole uint4 are copied by the first
// lanes of workgroup 0.  The two arrays never overlap: one is the context's `cit`, the other the snapshot's own allocation.
__global__ __launch_bounds__(TPB) void k_snapshot_words(uint32_t *__restrict__ dst, const uint32_t *__restrict__ src, uint32_t n)
{
    uint4 *o = reinterpret_cast<uint4 *>(dst);
    const uint4 *v = reinterpret_cast<const uint4 *>(src);
    const uint32_t n4 = n >> 2, stride = gridDim.x * TPB;
    for (uint32_t i = blockIdx.x * TPB + threadIdx.x; i < n4; i += stride) o[i] = v[i];
    const uint32_t tail = (n4 << 2) + threadIdx.x;
    if (blockIdx.x == 0 && threadIdx.x < (n & 3u)) dst[tail] = src[tail];
}
