// esim_kernels_group.h -- read-backs by citizen group (esim_set_groups: one uint16 label per citizen, at most ESIM_MAX_GROUPS
// groups): the census by group as it stands (esim_group_census) and, after the fact, per-group rows over the steps already
// run (esim_group_series).  A citizen never changes group, so there are no at-work pieces here.  Nothing writes simulation state.
#pragma once

#define GROUP_COLS 4u              // the statuses k_group_census counts: Exposed .. Vaccinated (Susceptible is size - the rest)

// One citizen into the workgroup's LDS table.  Almost everybody is Susceptible on the real workloads and neighbouring lanes
// would all hit the same few counters: a Susceptible lane issues nothing, its count is derived by k_group_finish.
__device__ __forceinline__ void group_count(uint32_t *tab, uint32_t w, uint32_t g, uint32_t t, uint32_t et, uint32_t it)
{
    if (CW_TE(w) == TE_SUSCEPTIBLE) return;
    const uint32_t st = status_of(CW_TE(w), t, et, it);
    if (st != ESIM_SUSCEPTIBLE) atomicAdd(&tab[g * GROUP_COLS + st - 1u], 1u);
}

// counts[g * 5 + status], status = Exposed .. Vaccinated, after the last completed step (counts zeroed by the caller).  A pure
// stream over the citizen words (4 B) and the labels (2 B): four citizens per lane and trip (one uint4 and one uint2; both
// arrays come from hipMalloc), grid-stride; the up to three citizens behind the last whole four go to the first lanes of
// workgroup 0.  Every workgroup keeps the whole table in LDS (1024 groups x 4 statuses x 4 B = 16 KB) and adds its non-zero
// entries to the global table at the end: no global atomic per citizen.
__global__ __launch_bounds__(TPB) void k_group_census(Dev d, const uint16_t *grp, uint32_t n_groups, uint32_t *counts)
{
    __shared__ uint32_t tab[ESIM_MAX_GROUPS * GROUP_COLS];
    const uint32_t t = d.ctrl->t - 1u;           // last completed step
    const uint32_t n_tab = n_groups * GROUP_COLS, et = d.exposed_time, it = d.infected_time;
    for (uint32_t i = threadIdx.x; i < n_tab; i += TPB) tab[i] = 0u;
    __syncthreads();
    const uint4 *cit4 = reinterpret_cast<const uint4 *>(d.cit);
    const uint2 *grp4 = reinterpret_cast<const uint2 *>(grp);
    const uint32_t n4 = d.n >> 2, stride = gridDim.x * TPB;
    for (uint32_t i = blockIdx.x * TPB + threadIdx.x; i < n4; i += stride) {
        const uint4 w = cit4[i];
        const uint2 g = grp4[i];
        group_count(tab, w.x, g.x & 0xFFFFu, t, et, it);
        group_count(tab, w.y, g.x >> 16, t, et, it);
        group_count(tab, w.z, g.y & 0xFFFFu, t, et, it);
        group_count(tab, w.w, g.y >> 16, t, et, it);
    }
    const uint32_t tail = (n4 << 2) + threadIdx.x;
    if (blockIdx.x == 0 && threadIdx.x < (d.n & 3u)) group_count(tab, d.cit[tail], grp[tail], t, et, it);
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n_tab; i += TPB) {
        const uint32_t v = tab[i];
        if (v) atomicAdd(&counts[(i / GROUP_COLS) * 5u + 1u + i % GROUP_COLS], v);
    }
}

// Susceptible = the group's size minus the four counted statuses.  A lane per group.
__global__ __launch_bounds__(TPB) void k_group_finish(const uint32_t *size, uint32_t n_groups, uint32_t *counts)
{
    const uint32_t g = blockIdx.x * TPB + threadIdx.x;
    if (g >= n_groups) return;
    uint32_t *row = counts + (size_t)g * 5u;
    row[0] = size[g] - row[1] - row[2] - row[3] - row[4];
}
