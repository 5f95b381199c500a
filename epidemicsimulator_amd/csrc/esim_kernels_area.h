// esim_kernels_area.h -- per-Output-Area read-backs: the census by area as it stands (esim_area_census) and, after the
// fact, the step at which the epidemic first reached every
// area or citizen group (esim_area_arrival).  Nothing here writes simulation state.
#pragma once

#define AREA_WINDOW 256u           // areas whose counters a workgroup of k_area_census keeps in LDS

// counts[area * 5 + status] after the last completed step.  A workgroup takes a contiguous stretch of `per_block` citizens.
// Citizens are normally home-sorted and buildings grouped by area, so a stretch sees few areas and neighbouring lanes
// share one: a run of lanes with the same area is counted by its first lane (one ballot per status), into an LDS window
// of AREA_WINDOW areas that starts at the area of the stretch's first citizen; keys outside the window (commuters at work,
// a population in any other order) go to the global table directly.  The window is added to the global table at the end.
__global__ __launch_bounds__(TPB) void k_area_census(Dev d, int home_only, uint32_t per_block, uint32_t *counts)
{
    __shared__ uint32_t win[AREA_WINDOW * 5u];
    __shared__ uint32_t s_base;
    const Ctrl *ctrl = d.ctrl;
    const uint32_t t = ctrl->t - 1u;             // last completed step
    const bool at_work = !home_only && ctrl->at_work != 0u;
    const uint64_t lo = (uint64_t)blockIdx.x * per_block;
    const uint64_t hi = lo + per_block < (uint64_t)d.n ? lo + per_block : (uint64_t)d.n;
    for (uint32_t i = threadIdx.x; i < AREA_WINDOW * 5u; i += TPB) win[i] = 0u;
    if (threadIdx.x == 0) s_base = lo < hi ? d.bld_area[d.home[lo]] : 0u;
    __syncthreads();
    const uint32_t base = s_base, lane = threadIdx.x & 63u;
    for (uint64_t c0 = lo; c0 < hi; c0 += TPB) {                  // the same trip count for every lane of the workgroup
        const uint64_t c = c0 + threadIdx.x;
        const bool valid = c < hi;
        uint32_t area = 0xFFFFFFFFu, st = 7u;
        if (valid) {
            const uint32_t w = d.cit[c];
            st = status_of(CW_TE(w), t, d.exposed_time, d.infected_time);
            area = d.bld_area[(at_work && (w & FL_HAS_WORK)) ? d.work[c] : d.home[c]];
        }
        const uint32_t prev = __shfl_up(area, 1, 64);
        const bool head = valid && (lane == 0u || prev != area);
        const unsigned long long heads = __ballot(head);
        const unsigned long long above = lane == 63u ? 0ull : heads & (~0ull << (lane + 1u));
        const unsigned long long run = (above ? (above & (0ull - above)) - 1ull : ~0ull) & (~0ull << lane);   // this lane up to the next head
#pragma unroll
        for (uint32_t s = 0; s < 5u; ++s) {
            const unsigned long long m = __ballot(st == s) & run;  // (lanes without a citizen have st = 7)
            if (head && m) {
                const uint32_t a = area - base;
                if (a < AREA_WINDOW) atomicAdd(&win[a * 5u + s], (uint32_t)__popcll(m));
                else atomicAdd(&counts[(size_t)area * 5u + s], (uint32_t)__popcll(m));
            }
        }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < AREA_WINDOW * 5u; i += TPB) {
        const uint32_t v = win[i];
        if (v) atomicAdd(&counts[(size_t)(base + i / 5u) * 5u + i % 5u], v);   // (only areas that were seen have a count)
    }
}

// The exposure step (biased) of log entry i from its position: the entries of step k are [log_off[k], log_off[k + 1]).
// (The citizen word no longer holds it once the citizen has been vaccinated.)
__device__ __forceinline__ uint32_t log_te(const Dev &d, uint32_t i, uint32_t k_max)
{
    uint32_t lo = 0u, hi = k_max;                                 // the largest k <= k_max with log_off[k] <= i
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1u) >> 1;
        if (d.log_off[mid] <= i) lo = mid; else hi = mid - 1u;
    }
    return lo;
}

// ---- esim_area_arrival ------------------------------------------------------------------------------------------------
// first[key] = the earliest exposure step among the log's entries with that key (the table is filled with ESIM_NEVER by the
// caller), key = the Output Area of the citizen's household, or its label where grp is given.  A lane per exposure-log entry,
// grid-stride; the length of the log is read from the control block, so nobody has to wait for it on the host.  The step
// comes from the entry's position (log_te); the seeds, "exposed" before step 1, count as step 0.  The log is in time order:
// once a key has its first entry, almost every later one loses the comparison against a plain load of the table and issues
// nothing -- a stale value read there is never smaller than the true one, so it costs an atomic at most, never a result.
// The atomics stay near the number of keys reached instead of the number of entries.
__global__ __launch_bounds__(TPB) void k_area_arrival(Dev d, const uint16_t *grp, uint32_t n_keys, uint32_t t_done, uint32_t *first)
{
    const uint32_t log_len = d.ctrl->log_len < d.n ? d.ctrl->log_len : d.n;
    for (uint32_t i = blockIdx.x * TPB + threadIdx.x; i < log_len; i += gridDim.x * TPB) {
        const uint32_t c = d.log[i];
        if (c >= d.n) continue;
        const uint32_t te = log_te(d, i, t_done + TE_BIAS);
        const uint32_t s = te > TE_BIAS ? te - TE_BIAS : 0u;
        const uint32_t key = grp ? (uint32_t)grp[c] : d.bld_area[d.home[c]];
        if (key < n_keys && s < first[key]) atomicMin(&first[key], s);
    }
}

// Was the citizen a live vaccination candidate at the end of step t (eligible(), on the word as it stood THEN)?  A word
// that is Vaccinated now belonged to the eligible set from the trigger step on: only members are vaccinated, nobody
// Vaccinated is exposed, and the set never drops a vaccinated member (Q10).
__device__ __forceinline__ bool was_eligible(uint32_t w, uint32_t t, uint32_t trigger)
{
    const uint32_t te = CW_TE(w);
    if (te == TE_SUSCEPTIBLE || te == TE_VACCINATED) return true;
    if (te >= TE_RECOVERED) return false;
    if (te > t + TE_BIAS) return true;                            // exposed later: Susceptible at step t
    return te > trigger + TE_BIAS && !(w & CW_BUS_EXPOSED);
}

// The citizen word does not keep the step of a vaccination, and somebody Exposed or Infected can be vaccinated
// (simulator.rs:551).  The choice of simulator.rs:524-553 is a pure function of the step and of the eligible set, so it is
// walked again, a workgroup per step, exactly as finish_phase walks it: the first `vaccination_rate` distinct live
// candidates in candidate order.  vax_of[c] = the earliest step that chose c, for the citizens that are Vaccinated now.
// Steps that vaccinated the whole set (eligible_count <= rate) are the caller's (Series::t_all).  One shard only.
// The steps walked are t_first .. t_done, t_first >= trigger, under the seed and the rate of `d`: after an esim_rollback that
// changed either, the host launches the steps up to the seam with the old values in its copy of `d` and the later ones with
// those in force (enqueue_vax_replay).
struct AreaVaxShared {
    uint32_t tab_key[VACC_TABLE];
    uint32_t tab_idx[VACC_TABLE];
    uint32_t wsum[FIN_TPB / 64];
    uint32_t s_total;
};

__global__ __launch_bounds__(FIN_TPB) void k_area_vax_replay(Dev d, uint32_t trigger, uint32_t t_first, uint32_t t_done, uint32_t *vax_of)
{
    __shared__ AreaVaxShared sm;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    const uint32_t k = d.vaccination_rate;
    for (uint32_t t = t_first + blockIdx.x; t <= t_done; t += gridDim.x) {
        if (d.records[t].eligible_count <= k) continue;
        for (uint32_t i = tid; i < VACC_TABLE; i += FIN_TPB) { sm.tab_key[i] = 0xFFFFFFFFu; sm.tab_idx[i] = 0xFFFFFFFFu; }
        __syncthreads();
        uint32_t already = 0;
        for (uint32_t base = 0; already < k; base += VACC_BATCH) {
            uint32_t j[4], slot[4]; bool live[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint32_t i = base + tid * 4u + q;
                j[q] = vacc_candidate(d, i, t);
                live[q] = j[q] < d.n && was_eligible(d.cit[j[q]], t, trigger);
                slot[q] = 0;
                if (live[q]) {
                    uint32_t sl = (j[q] * 2654435761u) >> 18;        // 14 bits
                    for (;;) {
                        const uint32_t old = atomicCAS(&sm.tab_key[sl], 0xFFFFFFFFu, j[q]);
                        if (old == 0xFFFFFFFFu || old == j[q]) break;
                        sl = (sl + 1u) & (VACC_TABLE - 1u);
                    }
                    atomicMin(&sm.tab_idx[sl], i);
                    slot[q] = sl;
                }
            }
            __syncthreads();
            bool first[4]; uint32_t mine = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                first[q] = live[q] && sm.tab_idx[slot[q]] == base + tid * 4u + q;
                mine += first[q];
            }
            uint32_t incl = mine;                                    // scan of `mine` in candidate order
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) { const uint32_t v = __shfl_up(incl, o, 64); if (lane >= (uint32_t)o) incl += v; }
            if (lane == 63) sm.wsum[wv] = incl;
            __syncthreads();
            if (tid == 0) { uint32_t a = 0; for (uint32_t w = 0; w < FIN_TPB / 64; ++w) { const uint32_t v = sm.wsum[w]; sm.wsum[w] = a; a += v; } sm.s_total = a; }
            __syncthreads();
            uint32_t pos = already + sm.wsum[wv] + incl - mine;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (first[q]) {
                    if (pos < k && CW_TE(d.cit[j[q]]) == TE_VACCINATED) atomicMin(&vax_of[j[q]], t);
                    pos++;
                }
            }
            const uint32_t got = sm.s_total;
            __syncthreads();
            already += got < k - already ? got : k - already;
            if (base >= (1u << 26)) break;                           // (the run itself raised ESIM_ERANGE there)
        }
        __syncthreads();
    }
}
