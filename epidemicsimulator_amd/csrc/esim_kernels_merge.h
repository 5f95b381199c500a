// esim_kernels_merge.h -- esim_ensemble_merge and esim_ensemble_load: a piece of another ensemble's accumulators,
// staged on this device, added cell by cell into the accumulators in force.  Integer adds only, so the sum does not depend on
// the order of the merges.  One kernel for every kind: a buffer the kind does not own is a null pointer.
//
// A lane takes four consecutive cells a trip: one 16 B access of every u32 counter and two of every u64 sum, a wavefront 1 KiB
// an instruction.  The host keeps a piece's first cell a multiple of four, so every such access is aligned.  The cells behind
// the last whole group of four, and the groups in which some cell has nothing to add, go cell by cell: a cell whose staged
// values are all zero is neither read nor written in the destination (by area, most cells of an ensemble are zero).
#pragma once

#define MERGE_TPB 64u                   // one wavefront a workgroup: no LDS, no barrier, nothing shared between lanes
#define MERGE_GRID 8192u                // workgroups at most: 32 wavefronts a compute unit, the rest by the grid stride
#define MERGE_LANE_CELLS 4u
#define MERGE_WORDS 2u                  // hit, defined
#define MERGE_WIDE 7u                   // sum, sumsq, sum_o, sumsq_o, cross, sum_d, sumsq_d

struct MergeArgs {
    const uint32_t *src_w[MERGE_WORDS]; uint32_t *dst_w[MERGE_WORDS];
    const unsigned long long *src_d[MERGE_WIDE]; unsigned long long *dst_d[MERGE_WIDE];
    const uint32_t *src_members; uint32_t *dst_members;     // the member counter: with the first piece only, else null
    uint64_t n;                                             // the cells of the piece
};

__global__ __launch_bounds__(MERGE_TPB) void k_ensemble_merge(MergeArgs a)
{
    if (a.dst_members && blockIdx.x == 0u && threadIdx.x == 0u) *a.dst_members += *a.src_members;
    const uint64_t groups = (a.n + MERGE_LANE_CELLS - 1u) / MERGE_LANE_CELLS, stride = (uint64_t)gridDim.x * MERGE_TPB;
    for (uint64_t g = (uint64_t)blockIdx.x * MERGE_TPB + threadIdx.x; g < groups; g += stride) {
        const uint64_t at = g * MERGE_LANE_CELLS;
        const bool whole = at + MERGE_LANE_CELLS <= a.n;
        uint32_t w[MERGE_WORDS][MERGE_LANE_CELLS];
        unsigned long long d[MERGE_WIDE][MERGE_LANE_CELLS];
        uint32_t live = 0u;                                 // bit k: cell at + k has something to add
#pragma unroll
        for (uint32_t b = 0u; b < MERGE_WORDS; ++b) {
            if (!a.src_w[b]) continue;
            if (whole) {
                const uint4 v = *reinterpret_cast<const uint4 *>(a.src_w[b] + at);
                w[b][0] = v.x; w[b][1] = v.y; w[b][2] = v.z; w[b][3] = v.w;
            } else {
#pragma unroll
                for (uint32_t k = 0u; k < MERGE_LANE_CELLS; ++k) w[b][k] = at + k < a.n ? a.src_w[b][at + k] : 0u;
            }
#pragma unroll
            for (uint32_t k = 0u; k < MERGE_LANE_CELLS; ++k) live |= w[b][k] ? 1u << k : 0u;
        }
#pragma unroll
        for (uint32_t b = 0u; b < MERGE_WIDE; ++b) {
            if (!a.src_d[b]) continue;
            if (whole) {
                const ulonglong2 lo = *reinterpret_cast<const ulonglong2 *>(a.src_d[b] + at), hi = *reinterpret_cast<const ulonglong2 *>(a.src_d[b] + at + 2u);
                d[b][0] = lo.x; d[b][1] = lo.y; d[b][2] = hi.x; d[b][3] = hi.y;
            } else {
#pragma unroll
                for (uint32_t k = 0u; k < MERGE_LANE_CELLS; ++k) d[b][k] = at + k < a.n ? a.src_d[b][at + k] : 0ull;
            }
#pragma unroll
            for (uint32_t k = 0u; k < MERGE_LANE_CELLS; ++k) live |= d[b][k] ? 1u << k : 0u;
        }
        if (!live) continue;
        if (whole && live == 0xFu) {
#pragma unroll
            for (uint32_t b = 0u; b < MERGE_WORDS; ++b) {
                if (!a.src_w[b]) continue;
                uint4 *p = reinterpret_cast<uint4 *>(a.dst_w[b] + at);
                uint4 v = *p;
                v.x += w[b][0]; v.y += w[b][1]; v.z += w[b][2]; v.w += w[b][3];
                *p = v;
            }
#pragma unroll
            for (uint32_t b = 0u; b < MERGE_WIDE; ++b) {
                if (!a.src_d[b]) continue;
                ulonglong2 *p = reinterpret_cast<ulonglong2 *>(a.dst_d[b] + at);
                ulonglong2 lo = p[0], hi = p[1];
                lo.x += d[b][0]; lo.y += d[b][1]; hi.x += d[b][2]; hi.y += d[b][3];
                p[0] = lo; p[1] = hi;
            }
            continue;
        }
#pragma unroll
        for (uint32_t k = 0u; k < MERGE_LANE_CELLS; ++k) {
            if (!((live >> k) & 1u)) continue;
#pragma unroll
            for (uint32_t b = 0u; b < MERGE_WORDS; ++b) if (a.src_w[b]) a.dst_w[b][at + k] += w[b][k];
#pragma unroll
            for (uint32_t b = 0u; b < MERGE_WIDE; ++b) if (a.src_d[b]) a.dst_d[b][at + k] += d[b][k];
        }
    }
}
