// esim_kernels_events.h -- superspreading events: the transmissions of one step in one gathering -- a household, a work
// place, a school room, a bus -- counted as one event, on top of the tree of esim_kernels_tree.h (whose k_tree_route leaves the
// bus of every exposure on a long route) and the pair engine of esim_pairs.h.  k_event_keys inserts one 64-bit key per
// transmission, k_event_hist bins the table's counts per setting, k_event_rekey prepares the order by size for a second run of
// the same sort, k_event_split turns the delivered keys into plain arrays.  Nothing here writes simulation state.
#pragma once
#include "esim_pairs.h"

// key = (step << 34) | (setting << 32) | place: ascending keys are ascending (step, setting, place, bus), see event_place.
#define EVENT_STEP_SHIFT 34u
#define EVENT_MAX_STEPS 0x40000000u      // steps a key has room for (30 bits): the top key stays below PAIR_EMPTY

// (A probe that defines EVENT_ENGINE_ONLY gets the kernels that need nothing but the table: tests/native/events_probe.hip.)
#ifndef EVENT_ENGINE_ONLY
// The 32-bit place of the gathering citizen c was exposed in under setting s: the home or work building, c's own room, or, on
// public transport, the rank of the first seat of c's bus among all riders in route order, route_off[r] + bus * bus_capacity --
// below n_pt, one value per (route, bus), ascending with (route, bus).  false where an index lies outside the tables.
__device__ __forceinline__ bool event_place(const Dev &d, const uint32_t *bus, uint32_t c, uint32_t s, uint32_t *place)
{
    if (s == ESIM_SETTING_HOUSEHOLD) { *place = d.home[c]; return *place < d.n_bld; }
    if (s == ESIM_SETTING_WORKPLACE) { *place = d.work[c]; return *place < d.n_bld; }
    if (s == ESIM_SETTING_SCHOOL) { *place = d.room[c]; return *place < d.n_room; }
    const uint32_t r = d.route_of[c];
    if (r >= d.n_routes || d.bus_capacity == 0u) return false;
    const uint32_t off = d.route_off[r], end = d.route_off[r + 1u];
    if (off >= end || end > d.n_pt) return false;
    const uint64_t seat = (uint64_t)off + (uint64_t)bus[c] * d.bus_capacity;
    *place = (uint32_t)seat;
    return seat < (uint64_t)end;
}

// One insert per transmission of steps [first, last] whose setting is in the mask.  A lane per log entry; no pre-aggregation
// inside the wavefront, as in k_flow_pairs: most events have one transmission.
__global__ __launch_bounds__(TPB) void k_event_keys(Dev d, Setting q, Tree t, uint32_t mask, uint32_t first, uint32_t last, uint32_t log_len, PairTable tab)
{
    for (uint64_t i = (uint64_t)blockIdx.x * TPB + threadIdx.x; i < (uint64_t)log_len; i += (uint64_t)gridDim.x * TPB) {
        const uint32_t c = d.log[i];
        if (c >= d.n) continue;
        const int ts = tree_step(q, c);
        const uint32_t s = q.setting[c];
        if (ts < (int)first || ts > (int)last || ts < 1 || (uint32_t)ts >= EVENT_MAX_STEPS || s >= ESIM_N_SETTINGS || !((mask >> s) & 1u)) continue;
        if (t.infector[c] >= d.n) continue;
        uint32_t place;
        if (!event_place(d, t.bus, c, s, &place)) continue;
        pair_insert(tab, ((uint64_t)(uint32_t)ts << EVENT_STEP_SHIFT) | ((uint64_t)s << 32) | place);
    }
}

#endif

// sizes[setting][min(count, ESIM_EVENT_BINS - 1)] += 1 per occupied slot of the table.  A lane per slot; almost every event
// falls into the first few bins, so a workgroup counts in a table of its own in LDS (4 KB) and hands its non-zero counters over
// once, as k_list_tables does.
__global__ __launch_bounds__(PAIR_TPB) void k_event_hist(PairTable t, uint32_t *sizes)
{
    __shared__ uint32_t tab[ESIM_N_SETTINGS * ESIM_EVENT_BINS];
    for (uint32_t k = threadIdx.x; k < ESIM_N_SETTINGS * ESIM_EVENT_BINS; k += PAIR_TPB) tab[k] = 0u;
    __syncthreads();
    for (uint64_t s = (uint64_t)blockIdx.x * PAIR_TPB + threadIdx.x; s < (uint64_t)t.cap; s += (uint64_t)gridDim.x * PAIR_TPB) {
        const unsigned long long k = t.key[s];
        if (k == PAIR_EMPTY) continue;
        const uint32_t n = t.cnt[s], top = ESIM_EVENT_BINS - 1u;
        atomicAdd(&tab[((uint32_t)(k >> 32) & 3u) * ESIM_EVENT_BINS + (n < top ? n : top)], 1u);
    }
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < ESIM_N_SETTINGS * ESIM_EVENT_BINS; k += PAIR_TPB) {
        const uint32_t v = tab[k];
        if (v) atomicAdd(&sizes[k], v);
    }
}

// The order by size: of the n pairs sorted by key, pair i gets the key (~count << 32) | i -- descending by count, ties ascending
// by position and so by the first key -- and carries its count; the n_sort - n slots behind them get PAIR_EMPTY, which sorts
// last.  A lane per slot.
__global__ __launch_bounds__(PAIR_TPB) void k_event_rekey(const uint32_t *cnt, uint32_t n, uint32_t n_sort, unsigned long long *by_size, uint32_t *size)
{
    for (uint64_t i = (uint64_t)blockIdx.x * PAIR_TPB + threadIdx.x; i < (uint64_t)n_sort; i += (uint64_t)gridDim.x * PAIR_TPB) {
        const uint32_t v = i < (uint64_t)n ? cnt[i] : 0u;
        by_size[i] = i < (uint64_t)n ? ((unsigned long long)(~v) << 32) | (uint32_t)i : PAIR_EMPTY;
        size[i] = v;
    }
}

#ifndef EVENT_ENGINE_ONLY
struct EventOut {
    uint32_t *step, *place, *bus, *size;   // [m] each, any may be nullptr
    uint8_t *setting;                      // [m] or nullptr
};

// Delivered event j < m: the pair at j of the arrays sorted by key, or, with `by_size` (sorted), the pair its low word names.  A
// transport place is the seat base of the bus: the route r with route_off[r] <= seat < route_off[r + 1] by a binary search
// (every route has a rider, so the offsets ascend strictly), the bus number from the seats in front of it on the route.
__global__ __launch_bounds__(PAIR_TPB) void k_event_split(Dev d, const unsigned long long *key, const uint32_t *cnt, uint32_t n, const unsigned long long *by_size,
                                                          uint32_t m, EventOut o)
{
    for (uint64_t j = (uint64_t)blockIdx.x * PAIR_TPB + threadIdx.x; j < (uint64_t)m; j += (uint64_t)gridDim.x * PAIR_TPB) {
        const uint32_t i = by_size ? (uint32_t)by_size[j] : (uint32_t)j;
        if (i >= n) continue;
        const unsigned long long k = key[i];
        const uint32_t s = (uint32_t)(k >> 32) & 3u;
        uint32_t place = (uint32_t)k, bus = 0u;
        if (s == ESIM_SETTING_TRANSPORT && d.n_routes && d.bus_capacity) {
            uint32_t lo = 0u, hi = d.n_routes;                   // route_off[lo] <= place < route_off[hi]
            while (hi - lo > 1u) {
                const uint32_t mid = lo + ((hi - lo) >> 1);
                if (d.route_off[mid] <= place) lo = mid; else hi = mid;
            }
            bus = (place - d.route_off[lo]) / d.bus_capacity;
            place = lo;
        }
        if (o.step) o.step[j] = (uint32_t)(k >> EVENT_STEP_SHIFT);
        if (o.setting) o.setting[j] = (uint8_t)s;
        if (o.place) o.place[j] = place;
        if (o.bus) o.bus[j] = bus;
        if (o.size) o.size[j] = cnt[i];
    }
}
#endif
