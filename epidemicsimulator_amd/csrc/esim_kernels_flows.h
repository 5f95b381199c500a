// esim_kernels_flows.h -- how the epidemic travels between Output Areas: on top of the tree of esim_kernels_tree.h and
// the lineage of esim_kernels_chains.h, the distinct (area of infector, area of infectee) pairs with their counts, the local,
// imported and exported cases of every area, the first case of every area with where it came from, and the distinct (lineage,
// area) pairs.  The sparse counts go through the pair engine of esim_pairs.h; k_flow_imports and the two kernels of the invasion
// tree work on dense [n_areas] arrays.  The area of a citizen is that of its household.  Nothing here writes simulation state.
#pragma once
#include "esim_pairs.h"

// The Output Area citizen m (< d.n) lives in; ESIM_NO_AREA where the tables do not give one.
__device__ __forceinline__ uint32_t flow_area(const Dev &d, uint32_t m)
{
    const uint32_t b = d.home[m];
    const uint32_t a = b < d.n_bld ? d.bld_area[b] : ESIM_NO_AREA;
    return a < d.n_areas ? a : ESIM_NO_AREA;
}

// The transmission that log entry i stands for, if it counts: cohort step in [first, last], setting in the mask, an infector.
// *src and *dst receive the areas of infector and infectee; false where the entry is none, or an end has no area.
__device__ __forceinline__ bool flow_of_entry(const Dev &d, const Setting &q, const Tree &t, uint32_t mask, uint32_t first, uint32_t last, uint64_t i,
                                              uint32_t *src, uint32_t *dst)
{
    const uint32_t c = d.log[i];
    if (c >= d.n) return false;
    const int ts = tree_step(q, c);
    const uint32_t s = q.setting[c];
    if (ts < (int)first || ts > (int)last || s >= ESIM_N_SETTINGS || !((mask >> s) & 1u)) return false;
    const uint32_t from = t.infector[c];
    if (from >= d.n) return false;
    *src = flow_area(d, from);
    *dst = flow_area(d, c);
    return *src != ESIM_NO_AREA && *dst != ESIM_NO_AREA;
}

// esim_area_flows: key (src << 32) | dst, one insert per transmission.  A lane per log entry.  No pre-aggregation inside the
// wavefront: the log is in time order, not in area order, and a pair of areas sees a handful of transmissions in a run.
__global__ __launch_bounds__(TPB) void k_flow_pairs(Dev d, Setting q, Tree t, uint32_t mask, uint32_t first, uint32_t last, uint32_t log_len, PairTable tab)
{
    for (uint64_t i = (uint64_t)blockIdx.x * TPB + threadIdx.x; i < (uint64_t)log_len; i += (uint64_t)gridDim.x * TPB) {
        uint32_t src, dst;
        if (flow_of_entry(d, q, t, mask, first, last, i, &src, &dst)) pair_insert(tab, ((uint64_t)src << 32) | dst);
    }
}

// esim_area_imports: local[a] += 1 for a transmission inside a; otherwise imported[dst] and exported[src].  Any of the three may
// be nullptr.  A lane per log entry.
__global__ __launch_bounds__(TPB) void k_flow_imports(Dev d, Setting q, Tree t, uint32_t mask, uint32_t first, uint32_t last, uint32_t log_len,
                                                      uint32_t *local, uint32_t *imported, uint32_t *exported)
{
    for (uint64_t i = (uint64_t)blockIdx.x * TPB + threadIdx.x; i < (uint64_t)log_len; i += (uint64_t)gridDim.x * TPB) {
        uint32_t src, dst;
        if (!flow_of_entry(d, q, t, mask, first, last, i, &src, &dst)) continue;
        if (src == dst) { if (local) atomicAdd(&local[dst], 1u); continue; }
        if (imported) atomicAdd(&imported[dst], 1u);
        if (exported) atomicAdd(&exported[src], 1u);
    }
}

// esim_area_invasion, pass one: best[a] = the smallest (cohort step << 32) | citizen over the cases living in a, the index cases
// (cohort step 0) included -- the earliest case, and of several in one step the smallest citizen index.  best is filled with
// ~0 by the caller.  A lane per log entry.
__global__ __launch_bounds__(TPB) void k_flow_first(Dev d, Setting q, uint32_t log_len, unsigned long long *best)
{
    for (uint64_t i = (uint64_t)blockIdx.x * TPB + threadIdx.x; i < (uint64_t)log_len; i += (uint64_t)gridDim.x * TPB) {
        const uint32_t c = d.log[i];
        if (c >= d.n) continue;
        const int ts = tree_step(q, c);
        const uint32_t a = flow_area(d, c);
        if (ts < 0 || a == ESIM_NO_AREA) continue;
        atomicMin(&best[a], ((unsigned long long)(uint32_t)ts << 32) | c);
    }
}

// Pass two, a lane per area: the winner's step, the area of its infector and its setting.  An index case and an exposure
// without a candidate have no infector: ESIM_NO_AREA and ESIM_SETTING_NONE.  Any output may be nullptr.
__global__ __launch_bounds__(TPB) void k_flow_resolve(Dev d, Setting q, Tree t, const unsigned long long *best, uint32_t *first_case, uint32_t *step,
                                                      uint32_t *source_area, uint8_t *setting)
{
    for (uint64_t a = (uint64_t)blockIdx.x * TPB + threadIdx.x; a < (uint64_t)d.n_areas; a += (uint64_t)gridDim.x * TPB) {
        const unsigned long long v = best[a];
        uint32_t who = ESIM_NO_INFECTOR, ts = ESIM_NEVER, src = ESIM_NO_AREA, s = ESIM_SETTING_NONE;
        if (v != ~0ull && (uint32_t)v < d.n) {
            who = (uint32_t)v; ts = (uint32_t)(v >> 32);
            const uint32_t from = ts ? t.infector[who] : ESIM_NO_INFECTOR;
            if (from < d.n) { src = flow_area(d, from); s = q.setting[who]; }
        }
        if (first_case) first_case[a] = who;
        if (step) step[a] = ts;
        if (source_area) source_area[a] = src;
        if (setting) setting[a] = (uint8_t)s;
    }
}

// esim_lineage_areas: key (lineage ordinal << 32) | area, one insert per case that has a lineage, the index cases included.
// A lane per log entry.
__global__ __launch_bounds__(TPB) void k_flow_lineages(Dev d, Chain ch, uint32_t log_len, PairTable tab)
{
    for (uint64_t i = (uint64_t)blockIdx.x * TPB + threadIdx.x; i < (uint64_t)log_len; i += (uint64_t)gridDim.x * TPB) {
        const uint32_t c = d.log[i];
        if (c >= d.n) continue;
        const uint32_t l = ch.lineage[c], a = flow_area(d, c);
        if (l == ESIM_NO_LINEAGE || a == ESIM_NO_AREA) continue;
        pair_insert(tab, ((uint64_t)l << 32) | a);
    }
}
