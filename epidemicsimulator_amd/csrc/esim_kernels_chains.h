// esim_kernels_chains.h -- transmission chains: on top of the tree of esim_kernels_tree.h, the index case at the
// root of every citizen's chain (its LINEAGE), the size of the subtree below every citizen (its DESCENDANTS), the outbreak every
// index case started, and the infectious age of every transmission.  k_chain_roots numbers the index cases; k_chain_up hands the
// lineage down the tree and k_chain_down sums the subtrees up it, a launch per window of exposed_time + 1 steps as k_tree_gen;
// k_chain_outbreaks fills the per-seed table; k_chain_ages counts.  Nothing here writes simulation state.
#pragma once

#define CHAIN_AGES ((uint32_t)ESIM_N_SETTINGS * ESIM_AGE_BINS)     // counters of the age table

struct Chain {
    uint32_t *lineage, *desc;            // [n] ESIM_NO_LINEAGE / 0 before the passes (the caller's memsets)
    uint32_t *size, *depth, *last;       // [n_seeds] each, zeroed by the caller
    uint32_t *ages;                      // [CHAIN_AGES], zeroed by the caller
    uint32_t *bad_age, *unrooted;        // transmissions at an impossible infectious age; exposures whose chain reaches no index case
    uint32_t n_seeds;                    // the entries of the log before step 1, at most log_len
};

// The stretch [*lo, *hi) of the log that holds the entries of steps [s_lo, s_hi], as k_tree_gen takes it.
__device__ __forceinline__ void chain_window(const Dev &d, const Setting &q, uint32_t s_lo, uint32_t s_hi, uint32_t log_len, uint32_t *lo, uint32_t *hi)
{
    const uint32_t a = d.log_off[TE_BIAS + s_lo];
    uint32_t b = s_hi >= q.t_done ? log_len : d.log_off[TE_BIAS + s_hi + 1u];
    if (b > log_len) b = log_len;
    *lo = a < b ? a : b;
    *hi = b;
}

// The index cases: the entries of the log before step 1, in the order of esim_get_seeds.  Each is the root of its own lineage.
__global__ __launch_bounds__(TPB) void k_chain_roots(Dev d, Chain ch)
{
    const uint32_t i = blockIdx.x * TPB + threadIdx.x;
    if (i >= ch.n_seeds) return;
    const uint32_t c = d.log[i];
    if (c < d.n) ch.lineage[c] = i;
}

// Lineage going forward: the windows of k_tree_gen, by the same argument -- an infector was exposed at least exposed_time + 1
// steps before its infectee, so its lineage is finished when the infectee's window runs.  A lane per entry.  An exposure without
// a candidate has no infector to inherit from and keeps ESIM_NO_LINEAGE, as does everybody below it; they are counted, one
// atomic per wavefront.
__global__ __launch_bounds__(TPB) void k_chain_up(Dev d, Setting q, Tree t, Chain ch, uint32_t s_lo, uint32_t s_hi, uint32_t log_len)
{
    uint32_t lo, hi;
    chain_window(d, q, s_lo, s_hi, log_len, &lo, &hi);
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t i0 = (uint64_t)lo + (uint64_t)blockIdx.x * TPB; i0 < (uint64_t)hi; i0 += (uint64_t)gridDim.x * TPB) {
        const uint64_t i = i0 + threadIdx.x;
        bool lost = false;
        if (i < (uint64_t)hi) {
            const uint32_t c = d.log[i];
            if (c < d.n) {
                const uint32_t from = t.infector[c];
                const uint32_t l = from < d.n ? ch.lineage[from] : ESIM_NO_LINEAGE;
                ch.lineage[c] = l;
                lost = l == ESIM_NO_LINEAGE;
            }
        }
        const unsigned long long m = __ballot(lost);
        if (m && lane == (uint32_t)__ffsll((long long)m) - 1u) atomicAdd(ch.unrooted, (uint32_t)__popcll(m));
    }
}

// Descendants going backward: the same windows from the last to the first.  Every child of c lies in a later window, so desc[c]
// is complete when c's window runs, and c hands desc[c] + 1 to its infector: one atomic per entry of the log, and on an index
// case no more than it has direct children.
__global__ __launch_bounds__(TPB) void k_chain_down(Dev d, Setting q, Tree t, Chain ch, uint32_t s_lo, uint32_t s_hi, uint32_t log_len)
{
    uint32_t lo, hi;
    chain_window(d, q, s_lo, s_hi, log_len, &lo, &hi);
    for (uint64_t i = (uint64_t)lo + (uint64_t)blockIdx.x * TPB + threadIdx.x; i < (uint64_t)hi; i += (uint64_t)gridDim.x * TPB) {
        const uint32_t c = d.log[i];
        if (c >= d.n) continue;
        const uint32_t from = t.infector[c];
        if (from < d.n) atomicAdd(&ch.desc[from], ch.desc[c] + 1u);
    }
}

// The largest v over the 64 lanes (a lane that has nothing to add passes 0).
__device__ __forceinline__ uint32_t chain_wave_max(uint32_t v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const uint32_t w = __shfl_xor(v, o, 64);
        v = w > v ? w : v;
    }
    return v;
}

// The per-seed table, a lane per log entry.  size: gathered from desc at the seeds.  depth and last_step: the largest generation
// and exposure step of a lineage.  The log is in time order and the lineages are few, so the lanes of a wavefront that share a
// lineage are reduced first, as tree_rows_add groups the lanes of a cell: at most one atomicMax pair per distinct lineage of a
// wavefront (wave-uniform trips).
__global__ __launch_bounds__(TPB) void k_chain_outbreaks(Dev d, Setting q, Tree t, Chain ch, uint32_t log_len)
{
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t i0 = (uint64_t)blockIdx.x * TPB; i0 < (uint64_t)log_len; i0 += (uint64_t)gridDim.x * TPB) {
        const uint64_t i = i0 + threadIdx.x;
        uint32_t l = ESIM_NO_LINEAGE, g = 0u, ts = 0u;
        if (i < (uint64_t)log_len) {
            const uint32_t c = d.log[i];
            if (c < d.n) {
                if (i < (uint64_t)ch.n_seeds) ch.size[i] = ch.desc[c];
                l = ch.lineage[c];
                const uint32_t gc = t.gen[c];
                const int s = tree_step(q, c);
                g = gc == ESIM_NEVER ? 0u : gc;
                ts = s > 0 ? (uint32_t)s : 0u;
            }
        }
        const bool live = l < ch.n_seeds && (g | ts) != 0u;               // (an index case itself adds nothing to its row)
        unsigned long long todo = __ballot(live);
        while (todo) {
            const uint32_t lead = (uint32_t)__ffsll((long long)todo) - 1u;
            const uint32_t l0 = __shfl(l, lead, 64);
            const bool mine = live && l == l0;
            const unsigned long long same = __ballot(mine);
            const uint32_t g_max = chain_wave_max(mine ? g : 0u), ts_max = chain_wave_max(mine ? ts : 0u);
            // (both cells only grow: a wavefront that sees a value at least its own -- however stale -- has nothing to add, and
            // the few addresses are spared most of the atomics that would queue up on them)
            if (lane == lead) {
                if (g_max > *(volatile uint32_t *)&ch.depth[l0]) atomicMax(&ch.depth[l0], g_max);
                if (ts_max > *(volatile uint32_t *)&ch.last[l0]) atomicMax(&ch.last[l0], ts_max);
            }
            todo &= ~same;
        }
    }
}

// The infectious age of every transmission of steps [first, last] (the infectee's): a = ts - onset(infector), onset = the
// infector's exposure step + exposed_time + 1, 0 for an index case (Infected from step 1).  ages[setting * ESIM_AGE_BINS + a].
// A workgroup keeps the table in LDS (8 KB), its lanes stride over the log and add there, and at the end it hands its non-zero
// counters to the global table, one atomic each: the caller caps the grid so that this stays small beside the walk.  An age
// outside 0 .. infected_time cannot happen on a correct run: skipped and counted, one atomic per wavefront.
// -DESIM_AGES_GLOBAL (diagnostics build): every lane adds to the global table directly, to time one form against the other.
__global__ __launch_bounds__(TPB) void k_chain_ages(Dev d, Setting q, Tree t, Chain ch, uint32_t first, uint32_t last, uint32_t log_len)
{
#ifndef ESIM_AGES_GLOBAL
    __shared__ uint32_t h[CHAIN_AGES];
    for (uint32_t k = threadIdx.x; k < CHAIN_AGES; k += TPB) h[k] = 0u;
    __syncthreads();
#endif
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t a_max = d.infected_time < ESIM_AGE_BINS - 1u ? d.infected_time : ESIM_AGE_BINS - 1u;
    for (uint64_t i0 = (uint64_t)blockIdx.x * TPB; i0 < (uint64_t)log_len; i0 += (uint64_t)gridDim.x * TPB) {
        const uint64_t i = i0 + threadIdx.x;
        bool bad = false;
        if (i < (uint64_t)log_len) {
            const uint32_t c = d.log[i];
            if (c < d.n) {
                const int ts = tree_step(q, c);
                const uint32_t s = q.setting[c], from = t.infector[c];
                if (ts >= 1 && ts >= (int)first && ts <= (int)last && s < ESIM_N_SETTINGS && from < d.n) {
                    const int tf = tree_step(q, from);
                    const int a = tf < 0 ? -1 : ts - (tf == 0 ? 0 : tf + (int)d.exposed_time + 1);
                    if (a < 0 || a > (int)a_max) bad = true;
#ifndef ESIM_AGES_GLOBAL
                    else atomicAdd(&h[s * ESIM_AGE_BINS + (uint32_t)a], 1u);
#else
                    else atomicAdd(&ch.ages[s * ESIM_AGE_BINS + (uint32_t)a], 1u);
#endif
                }
            }
        }
        const unsigned long long m = __ballot(bad);
        if (m && lane == (uint32_t)__ffsll((long long)m) - 1u) atomicAdd(ch.bad_age, (uint32_t)__popcll(m));
    }
#ifndef ESIM_AGES_GLOBAL
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < CHAIN_AGES; k += TPB) {
        const uint32_t v = h[k];
        if (v) atomicAdd(&ch.ages[k], v);
    }
#endif
}
