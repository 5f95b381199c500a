// esim_kernels_books.h -- the books of a chunk: exposure counts, log entries and clean-up of a one-pass chunk (k_chunk_count,
// k_chunk_scatter, k_chunk_vax_final, k_chunk_books) and the census, records and control block of any chunk (k_batch_finish).
#pragma once
#include "esim_kernels_common.h"
#include "esim_kernels_plan.h"
#include "esim_kernels_marks.h"
// Exposures per step (statistics.rs:181) from the final citizen words -- the many-workgroup form, for chunks with many new
// exposures (k_chunk_books does it itself otherwise).
__global__ __launch_bounds__(TPB) void k_chunk_count(Dev d)
{
    Ctrl *ctrl = d.ctrl;
    if (!ctrl->chunk_parallel || ctrl->chunk_ok == 0u) return;
    const uint32_t tid = blockIdx.x * TPB + threadIdx.x, r = tid & (SUBQ - 1u), step = (gridDim.x * TPB) / SUBQ;
    const uint32_t n_new = newexp_len(d, HOT_NEWEXP, r);
    const uint32_t *list = newexp_list(d, r);
    const uint32_t t0 = ctrl->chunk_t0;
    // exposures per (step of the chunk, building | bus): counted in LDS, then added to one of EXP_ROWS rows of exp_part
    // (k_chunk_books adds the rows up and zeroes them) -- a hundred thousand atomics on the same dozen cache lines of one
    // global array are served one by one
    __shared__ uint32_t e_cnt[2u * FREE_MAX];
    __shared__ uint32_t s_cut;
    if (threadIdx.x < 2u * FREE_MAX) e_cnt[threadIdx.x] = 0u;
    if (threadIdx.x == 0) s_cut = 0xFFFFFFFFu;
    __syncthreads();
    for (uint32_t i = tid / SUBQ; i < n_new; i += step) {
        if (list[i] >= d.n) continue;
        const uint32_t w = d.cit[list[i]];
        const uint32_t j = CW_TE(w) - TE_BIAS - t0;
        if (j < FREE_MAX) atomicAdd(&e_cnt[2u * j + ((w & CW_BUS_EXPOSED) ? 1u : 0u)], 1u);
        // exposed on a bus although the plan vaccinates it later in the chunk: from this step on the plan is void (k_chunk_vax)
        if ((w & CW_BUS_EXPOSED) && CW_VAX_REL(w) != CW_VAX_NONE) { atomicMin(&s_cut, j); if (d.world > 1u) d.xc[j] = 1u; }
    }
    __syncthreads();
    if (threadIdx.x < 2u * FREE_MAX && e_cnt[threadIdx.x]) atomicAdd(&d.exp_part[(size_t)(blockIdx.x % EXP_ROWS) * 2u * FREE_MAX + threadIdx.x], e_cnt[threadIdx.x]);
    if (threadIdx.x == 0 && s_cut != 0xFFFFFFFFu) atomicMin(&ctrl->chunk_cut, s_cut);
    if (!ctrl->vax_chunk) return;
    // What the chunk's vaccinations do to the census of its later steps, from the words as the draws left them: one thread per
    // planned citizen, only the step that won counts.  A citizen vaccinated at the end of step j is Vaccinated from step j + 1
    // on instead of what its exposure step says (Susceptible; Exposed up to e_last; Infected up to i_last; Recovered after).
    // Difference arrays over the steps; events at or after a cut only touch steps that are not committed.
    __shared__ int dl[4][FREE_MAX + 2];
    for (uint32_t i = threadIdx.x; i < 4u * (FREE_MAX + 2u); i += TPB) (&dl[0][0])[i] = 0;
    __syncthreads();
    const uint32_t n = ctrl->chunk_ok;
    for (uint32_t j = blockIdx.x; j < n; j += gridDim.x) {
        const uint32_t cnt = d.vax_cnt[j];
        for (uint32_t i = threadIdx.x; i < cnt; i += TPB) {
            const uint32_t w = d.cit[d.vax_ev[(size_t)j * VACC_MAX_RATE + i]], te = CW_TE(w);
            if (CW_VAX_REL(w) != j) continue;                                  // (j = n - 1 only moves the totals after the chunk: index n)
            atomicAdd(&dl[3][j + 1u], 1);                                      // Vaccinated from j + 1 to the end
            // (exposed in a LATER step of this chunk: it was Susceptible when it was vaccinated -- only a citizen the repair of the plan
            // chose anew can look like this, and the chunk is then cut behind step j: that exposure never happened)
            if (te == TE_SUSCEPTIBLE || (te < TE_RECOVERED && te - TE_BIAS - t0 < n && te - TE_BIAS - t0 > j)) { atomicSub(&dl[0][j + 1u], 1); continue; }
            const int e_last = (int)te - (int)TE_BIAS + (int)d.exposed_time - (int)t0, i_last = e_last + 1 + (int)d.infected_time;
            const int lo = (int)j + 1;
            if (lo <= e_last) { atomicSub(&dl[1][lo], 1); atomicAdd(&dl[1][min(e_last, (int)n - 1) + 1], 1); }
            const int ilo = max(lo, e_last + 1);
            if (ilo <= i_last && ilo < (int)n) { atomicSub(&dl[2][ilo], 1); atomicAdd(&dl[2][min(i_last, (int)n - 1) + 1], 1); }
        }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < 4u * (FREE_MAX + 2u); i += TPB) { const int v = (&dl[0][0])[i]; if (v) atomicAdd(&d.vax_delta[i], (uint32_t)v); }
}

// The chunk's exposures enter the log grouped by step (after k_batch_finish wrote the offsets); the hash map and
// the count vectors are emptied for the next chunk.
__global__ __launch_bounds__(TPB) void k_chunk_scatter(Dev d)
{
    Ctrl *ctrl = d.ctrl;
    if (ctrl->chunk_done == 0u) return;
    // (the chunk as k_chunk_books noted it down: by now the control block may describe the next one)
    const uint32_t t0 = ctrl->prev_t0;
    const uint32_t n_items = min(ctrl->prev_n_items, d.items_cap);
    {
        const uint32_t tid = blockIdx.x * TPB + threadIdx.x, r = tid & (SUBQ - 1u), step = (gridDim.x * TPB) / SUBQ;
        const uint32_t n_new = newexp_len(d, HOT_PREV_NEWEXP, r);
        const uint32_t *list = newexp_list(d, r);
        const uint32_t n_eff = ctrl->prev_n_eff;
        for (uint32_t i = tid / SUBQ; i < n_new; i += step) {
            const uint32_t m = list[i];
            if (m >= d.n) continue;
            const uint32_t te = CW_TE(d.cit[m]);
            if (te - TE_BIAS - t0 < n_eff) d.log[d.log_off[te] + atomicAdd(&d.cursor[(blockIdx.x % EXP_ROWS) * FREE_MAX + te - TE_BIAS - t0], 1u)] = m;
            else {
                // exposed in a step that was not committed (a cut, or the disease was over before): Susceptible again; on a bus in
                // the very step of the cut: it will be again, and the next plan must know (CW_PLAN_SKIP)
                const bool again = ctrl->prev_cut && te - TE_BIAS - t0 == n_eff && (d.cit[m] & CW_BUS_EXPOSED);
                atomicOr(&d.cit[m], (TE_SUSCEPTIBLE << CW_TE_SHIFT) | (again ? CW_PLAN_SKIP : 0u));
                atomicAnd(&d.cit[m], ~CW_BUS_EXPOSED);
            }
        }
    }
    // the hash slots (and spilled count vectors) of the ids that were handed out: a thread per (wavefront of k_chunk_marks,
    // k-th id of its range), so that the whole clean-up is three dependent loads deep
    const uint32_t per_wave = ctrl->prev_per_wave, n_mw = per_wave ? n_items / per_wave : 0u;
    const uint32_t tid = blockIdx.x * TPB + threadIdx.x, nth = gridDim.x * TPB;
    for (uint32_t i = tid; i < n_mw * per_wave; i += nth) {
        const uint32_t w = i / per_wave, k = i - w * per_wave;
        if (k >= d.used_cnt[w]) continue;
        const uint32_t h = d.hitems[i];
        if (h >= d.hcap) continue;                                             // ITEM_UNUSED (or no slot at all)
        const uint32_t state = d.slot_state[h];
        if (state > ITEM_RECS && d.item_rec[i].id < d.n_bld + d.n_room)       // somebody spilled into the per-step counters
            for (uint32_t j = 0; j < FREE_MAX; ++j) d.vec[(size_t)h * FREE_MAX + j] = 0u;
        d.hkey[h] = HKEY_EMPTY;
        if (state) d.slot_state[h] = 0u;
    }
}

// The planned vaccinations of the chunk k_chunk_scatter has just finished (a kernel of its own: the scatter reads the exposure
// steps this one overwrites): those of committed steps happen (simulator.rs:551: whatever the citizen was, it is Vaccinated;
// an exposure step leaves the histogram as vaccinate() does), the others are forgotten.
__global__ __launch_bounds__(TPB) void k_chunk_vax_final(Dev d)
{
    Ctrl *ctrl = d.ctrl;
    if (!ctrl->prev_vax) return;
    const uint32_t n_eff = ctrl->prev_n_eff;
    // (the plan may reach beyond the chunk: the decisions can end a chunk early, k_decide)
    const uint32_t n = ctrl->prev_planned;
    for (uint32_t j = blockIdx.x; j < n; j += gridDim.x) {
        const uint32_t cnt = d.vax_cnt[j];
        for (uint32_t i = threadIdx.x; i < cnt; i += TPB) {
            const uint32_t c = d.vax_ev[(size_t)j * VACC_MAX_RATE + i];
            const uint32_t w = d.cit[c];
            if (CW_VAX_REL(w) != j) continue;                         // another step of the chunk won, or Vaccinated before
            if (j < n_eff) {
                const uint32_t te = CW_TE(w);
                if (te < TE_RECOVERED) atomicSub(&d.hist[te], 1u);
                d.cit[c] = CW_MAKE(TE_VACCINATED, w & (CW_BUS_EXPOSED | CW_FLAGS));
            } else atomicAnd(&d.cit[c], ~CW_VAX_MASK);
        }
    }
}

// ----------------------------------------------------------------------------- k_batch_finish
// The books of a pipelined chunk [t0, t0+n): census (simulator.rs:178) by sliding the Exposed / Infected
// windows over the exposure histogram, the StatisticEntry of every step (statistics.rs:208-215, adjusted
// by citizen_exposed :275-287), hist / log offsets, and the control block as it stands after the chunk.
// (body shared by the two launch forms below)
// e: this chunk's exposure counts [2 * step of the chunk + (bus ? 1 : 0)] when the caller holds them (else d.exp_step has them);
// lo_out: receives the first log position of every step of the chunk.
// vax: the chunk ran under a vaccination programme with its vaccinations planned (k_chunk_vax): the census moves by the
// prefix sums of Dev::vax_delta, and only the steps before Ctrl::chunk_cut are committed.  Returns the steps committed.
__device__ __forceinline__ uint32_t batch_finish_body(const Dev &d, uint32_t t0, uint32_t n, const uint32_t *e = nullptr, uint32_t *lo_out = nullptr, bool vax = false,
                                                       bool marks_left = true)
{
    __shared__ uint32_t P[BF_WIN + 1];                 // P[i + 1] = sum of H[0..i], P[0] = 0
    __shared__ uint32_t wtmp[FIN_TPB / 64];
    __shared__ uint32_t n_eff_s;
    __shared__ uint32_t cum[5][FREE_MAX + 2];          // prefix sums of the vaccination deltas (S, E, I, V) and of the bus exposures
    Ctrl *ctrl = d.ctrl;
    const uint32_t tid = threadIdx.x;
    const int et = (int)d.exposed_time, it = (int)d.infected_time;
    const int base_idx = (int)(t0 + TE_BIAS) - et - 1 - it;              // lowest histogram entry any census of the chunk reads
    uint32_t n_cut = vax ? min(n, ld(&ctrl->chunk_cut)) : n;
    if (vax && d.world > 1u) {                                            // sharded: the earliest cut of any shard (buffer C, summed)
        n_cut = n;
        for (uint32_t j = 0; j < n; ++j) if (ld(&d.xc[j])) { n_cut = j; break; }
    }
    // H[i] = citizens exposed in "step" base_idx + i: the histogram before the chunk, this chunk's exposure counters inside it
    {
        const int k = base_idx + (int)tid;
        uint32_t h = 0;
        if (k >= (int)(t0 + TE_BIAS)) { const uint32_t j = (uint32_t)(k - (int)(t0 + TE_BIAS)); if (j < n) h = e ? e[2u * j] + e[2u * j + 1u] : d.exp_step[2u * (t0 + j)] + d.exp_step[2u * (t0 + j) + 1u]; }
        else if (k >= 0) h = d.hist[k];
        P[tid + 1] = h;
        if (tid == 0) { P[0] = 0u; n_eff_s = n_cut; }
        // cum[q][i] = sum of delta[q][0..i] (i.e. what applies to step i); cum[4][i] = bus exposures of steps < i.
        // (all loads at once, then one wavefront per row scans it: a thread walking a row load by load took 15-25 us)
        for (uint32_t i = tid; i < 5u * (FREE_MAX + 2u); i += FIN_TPB) {
            const uint32_t q = i / (FREE_MAX + 2u), k = i - q * (FREE_MAX + 2u);
            uint32_t v = 0u;
            if (q < 4u) v = vax ? ld(&d.vax_delta[i]) : 0u;
            else if (k < n) v = e ? e[2u * k + 1u] : d.exp_step[2u * (t0 + k) + 1u];
            cum[q][k] = v;
        }
    }
    __syncthreads();
    if (tid < 5u * 64u) {
        const uint32_t q = tid >> 6, l = tid & 63u;
        uint32_t v0 = cum[q][l], v1 = 64u + l < FREE_MAX + 2u ? cum[q][64u + l] : 0u;
        const uint32_t own0 = v0, own1 = v1;
        for (uint32_t o = 1; o < 64u; o <<= 1) { const uint32_t y0 = __shfl_up(v0, o, 64), y1 = __shfl_up(v1, o, 64); if (l >= o) { v0 += y0; v1 += y1; } }
        v1 += __shfl(v0, 63, 64);
        if (q == 4u) { v0 -= own0; v1 -= own1; }                              // (exclusive: bus exposures of the steps before)
        cum[q][l] = v0;
        if (64u + l < FREE_MAX + 2u) cum[q][64u + l] = v1;
    }
    __syncthreads();
    block_scan_1024(P + 1, wtmp);
    const uint32_t S0 = ctrl->n_susceptible, V0 = ctrl->n_vaccinated, run0 = d.log_off[t0 + TE_BIAS];
    const uint32_t elig0 = ctrl->elig_count;
    const int top0 = (int)(t0 + TE_BIAS) - base_idx;                      // index of hist[t0 + TE_BIAS] in H
    esim_step_result r;
    uint32_t exps = 0;
    if (tid < n) {
        const uint32_t s = t0 + tid;
        const int ts = top0 + (int)tid;                                   // index of this step's own entry
        exps = P[ts + 1] - P[ts];
        const uint32_t S = S0 - (P[ts] - P[top0]) + cum[0][tid];           // Susceptible before this step's exposures
        const uint32_t E = P[ts] - P[ts - et] + cum[1][tid];               // exposed in steps s - et .. s - 1 (census precedes exposures)
        const uint32_t I = P[ts - et] - P[ts - et - 1 - it] + cum[2][tid];
        const uint32_t V = V0 + cum[3][tid];
        r.time_step = s;
        if (exps > S && tid < n_cut) ctrl->error = (uint32_t)(-ESIM_ESIM); // citizen_exposed underflow, statistics.rs:275-287
        r.susceptible = S - exps; r.exposed = E + exps; r.infected = I;
        r.recovered = d.n - S - V - E - I; r.vaccinated = V;
        r.exposures_building = e ? e[2u * tid] : d.exp_step[2u * s]; r.exposures_bus = e ? e[2u * tid + 1u] : d.exp_step[2u * s + 1u];
        if (e || tid >= n_cut) {                                          // (steps that are not committed will be counted again)
            d.exp_step[2u * s] = tid < n_cut ? r.exposures_building : 0u; d.exp_step[2u * s + 1u] = tid < n_cut ? r.exposures_bus : 0u;
        }
        if (lo_out) lo_out[tid] = run0 + (P[ts] - P[top0]);
        r.lockdown = d.dec[tid + 1u].lockdown; r.vaccination_active = vax ? 1u : 0u; r.mask_status = d.dec[tid + 1u].mask;
        r.n_riders = d.dec[tid].bus_dir ? d.n_pt : 0u;
        r.vaccinated_now = vax ? d.vax_now[tid] : 0u;
        r.eligible_count = vax ? elig0 - cum[4][tid + 1u] : 0u;            // after this step's bus exposures (simulator.rs:447-449)
        r.disease_exists = (r.exposed != 0u || r.infected != 0u || r.susceptible != 0u) ? 1u : 0u;   // statistics.rs:289-291
        r.reserved = 0u;
        if (!r.disease_exists && ctrl->stop_when_done) atomicMin(&n_eff_s, tid + 1u);
    }
    __syncthreads();
    const uint32_t n_eff = n_eff_s;
    if (tid < n_eff) {
        const uint32_t s = t0 + tid;
        const int ts = top0 + (int)tid;
        d.hist[s + TE_BIAS] = exps;
        d.log_off[s + TE_BIAS + 1u] = run0 + (P[ts + 1] - P[top0]);
        if (s <= d.max_steps) d.records[s] = r;
        if (tid + 1u == n_eff) ctrl->quiet = (r.exposed == 0u && r.infected == 0u) ? 1u : 0u;
    }
    if (tid == 0) {
        ctrl->n_susceptible = S0 - (P[top0 + (int)n_eff] - P[top0]) + cum[0][n_eff];
        ctrl->n_vaccinated = V0 + cum[3][n_eff];
        if (vax) ctrl->elig_count = elig0 - cum[4][n_eff];
        ctrl->log_len = run0 + (P[top0 + (int)n_eff] - P[top0]);
        ctrl->t = t0 + n_eff; ctrl->steps_done = t0 + n_eff - 1u;
        if (n_eff < n_cut) ctrl->finished = 1u;
        else if (n_cut < n) ctrl->vax_cuts += 1u;
        // (a chunk whose plan was repaired and that is cut all the same is cut BEHIND a step whose newly chosen citizen mattered later:
        // what the attempt saw in the step of the cut is then not what will happen in it, so nobody is marked CW_PLAN_SKIP)
        ctrl->prev_cut = (n_eff == n_cut && n_cut < n && !(vax && ctrl->repair_ran)) ? 1u : 0u;
        if (n_eff) {
            ctrl->lockdown = d.dec[n_eff].lockdown; ctrl->mask = d.dec[n_eff].mask;
            ctrl->at_work = d.dec[n_eff - 1u].at_work; ctrl->bus_dir = d.dec[n_eff - 1u].bus_dir;
        }
        // ring slots: a chunk run step by step leaves the marks of its last step (the next exposure pass clears them); a chunk
        // drawn in one pass leaves none -- and the lists k_chunk_marks emptied for it must not keep their old lengths, or a
        // sequential step that comes back to that slot would walk stale entries (a route ranked twice at once)
        const uint32_t keep = marks_left ? ((t0 + n - 1u) & (MARK_SLOTS - 1u)) : MARK_SLOTS;
        for (uint32_t z = 0; z < MARK_SLOTS; ++z)
            if (z != keep) { ctrl->n_touched_bld[z] = 0u; ctrl->n_touched_room[z] = 0u; ctrl->n_touched_route[z] = 0u; ctrl->n_touched_route_big[z] = 0u; }
    }
    return n_eff;
}

__global__ __launch_bounds__(FIN_TPB) void k_batch_finish(Dev d, uint32_t t0, uint32_t n)
{
    batch_finish_body(d, t0, n);
}

// The books of a one-pass chunk, in ONE workgroup so that nothing but kernel boundaries of the wide kernels is left on
// the chunk's critical path (a kernel boundary costs ~4.5 us here, and these steps are small):
//   exposures per step (statistics.rs:181) from the final citizen words of the newly exposed
//   census, records, histogram, log offsets, control block (batch_finish_body)
//   [scatter] the new log entries in step order; hash slots of the chunk's items emptied
//   [do_next] the census ahead and the decisions of the NEXT chunk (k_future + k_decide)
// It takes (t0, n) from the control block, so that the host can enqueue chunk after chunk without waiting; chunk_done tells
// k_chunk_scatter (the many-workgroup form of [scatter], used while many citizens are Infected) that the books were written.
struct BooksShared { uint32_t e_cnt[2 * FREE_MAX]; uint32_t lo_s[FREE_MAX], cur_s[FREE_MAX]; uint32_t win[BF_WIN]; uint32_t wtmp[FIN_TPB / 64]; };
__device__ __forceinline__ void books_body(const Dev &d, int fused, int do_next, uint32_t max_ahead, uint32_t limit_t, BooksShared &bs)
{
    uint32_t *e_cnt = bs.e_cnt, *lo_s = bs.lo_s, *cur_s = bs.cur_s, *win = bs.win, *wtmp = bs.wtmp;
    Ctrl *ctrl = d.ctrl;
    const uint32_t tid = threadIdx.x;
    const uint32_t pb0 = PROF_NOW();
    if (!ctrl->chunk_parallel || ctrl->chunk_ok == 0u) {
        if (tid == 0) {
            ctrl->chunk_done = 0u;
            // a plan was made but the chunk does not run: k_chunk_vax_final takes the plan's fields out of the words again
            ctrl->prev_vax = ld(&ctrl->vax_chunk); ctrl->prev_n_eff = 0u; ctrl->prev_planned = ld(&ctrl->vax_planned); ctrl->vax_chunk = 0u;
        }
        return;
    }
    const uint32_t t0 = ctrl->chunk_t0, n = ctrl->chunk_ok;
    const uint32_t n_items = min(ld(&ctrl->n_items), d.items_cap);
    if (tid < 2u * FREE_MAX) e_cnt[tid] = 0u;
    if (tid < FREE_MAX) cur_s[tid] = 0u;
    __syncthreads();
    // sub-list `thread & 63` of the newly exposed, every 16th entry of it
    const uint32_t r = tid & (SUBQ - 1u);
    const uint32_t n_new = newexp_len(d, HOT_NEWEXP, r);
    const uint32_t *list = newexp_list(d, r);
    if (fused) {
        for (uint32_t i = tid / SUBQ; i < n_new; i += FIN_TPB / SUBQ) {
            if (list[i] >= d.n) continue;
            const uint32_t w = d.cit[list[i]];
            const uint32_t j = CW_TE(w) - TE_BIAS - t0;
            if (j < FREE_MAX) atomicAdd(&e_cnt[2u * j + ((w & CW_BUS_EXPOSED) ? 1u : 0u)], 1u);
        }
    } else if (tid < 2u * n) {
        // k_chunk_count made them, in EXP_ROWS rows by workgroup.  k_chunk_scatter's workgroups visit the same citizens as their
        // namesakes there, so a row's counts are also what its workgroups will write into each step's stretch of the log: the
        // rows get their own write cursors (one shared cursor per step is a hundred thousand returning atomics on six lines)
        uint32_t a = 0u, run = 0u;
        uint32_t v[EXP_ROWS];
#pragma unroll
        for (uint32_t p = 0; p < EXP_ROWS; ++p) v[p] = d.exp_part[(size_t)p * 2u * FREE_MAX + tid];   // (all loads first: in flight together)
#pragma unroll
        for (uint32_t p = 0; p < EXP_ROWS; ++p) {
            d.exp_part[(size_t)p * 2u * FREE_MAX + tid] = 0u;
            a += v[p];
            if (!(tid & 1u)) d.cursor[p * FREE_MAX + (tid >> 1)] = run;      // (buildings + buses of the step, rows before this one)
            run += v[p] + __shfl_xor(v[p], 1, 64);
        }
        e_cnt[tid] = a;
    }
    __syncthreads();
    const uint32_t pb1 = PROF_NOW();
    const bool vax = ld(&ctrl->vax_chunk) != 0u;                              // (planned chunks always take the wide form: fused == 0)
    const uint32_t n_eff = batch_finish_body(d, t0, n, e_cnt, lo_s, vax, false);
    const uint32_t pb2 = PROF_NOW();
    if (!fused) {
        // k_chunk_scatter runs after this kernel, i.e. after the next chunk's decisions have reset what it reads: keep a copy
        if (tid < SUBQ) d.hot[(HOT_PREV_NEWEXP + tid) * HOT_STRIDE] = n_new;   // (thread r < 64 read sub-list r's length above)
        if (tid == 0) { ctrl->prev_t0 = t0; ctrl->prev_n_items = n_items; ctrl->prev_per_wave = ld(&ctrl->items_per_wave);
                        ctrl->prev_n = n; ctrl->prev_n_eff = n_eff; ctrl->prev_vax = vax ? 1u : 0u; ctrl->prev_planned = ld(&ctrl->vax_planned); ctrl->vax_chunk = 0u; }
        // (its per-step write cursors were set above, a row per EXP_ROWS-th workgroup)
    }
    if (tid == 0) ctrl->chunk_done = 1u;
    if (tid < 64u) {
        // totals of the split lists, for esim_debug_counters
        uint32_t a = ld(&d.hot[(HOT_NEWEXP + tid) * HOT_STRIDE]), b = ld(&d.hot[(HOT_UNITS + tid) * HOT_STRIDE]);
        for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o, 64); b += __shfl_xor(b, o, 64); }
        if (tid == 0) { ctrl->n_newexp = a; ctrl->n_units = b; ctrl->n_route_pairs_big = ld(&d.hot[HOT_BIGPAIRS * HOT_STRIDE]); }
    }
    __syncthreads();
    if (fused) {
        for (uint32_t i = tid / SUBQ; i < n_new; i += FIN_TPB / SUBQ) {
            const uint32_t m = list[i];
            if (m >= d.n) continue;
            const uint32_t j = CW_TE(d.cit[m]) - TE_BIAS - t0;
            if (j < FREE_MAX) d.log[lo_s[j] + atomicAdd(&cur_s[j], 1u)] = m;
        }
        // the ids each wavefront of k_chunk_marks handed out: thread t looks after the wavefronts t, t + 1024, ...; all loads
        // of a round are in flight together (this loop is nothing but memory latency)
        const uint32_t per_wave = ld(&ctrl->items_per_wave), n_mw = per_wave ? n_items / per_wave : 0u;
        for (uint32_t w0 = tid; w0 < n_mw; w0 += 4u * FIN_TPB) {
            uint32_t used[4], h[4][4];
#pragma unroll
            for (int a = 0; a < 4; ++a) { const uint32_t w = w0 + (uint32_t)a * FIN_TPB; used[a] = w < n_mw ? d.used_cnt[w] : 0u; }
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int k = 0; k < 4; ++k) h[a][k] = (uint32_t)k < used[a] ? d.hitems[(w0 + (uint32_t)a * FIN_TPB) * per_wave + (uint32_t)k] : ITEM_UNUSED;
            uint32_t st[4][4];
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int k = 0; k < 4; ++k) st[a][k] = h[a][k] < d.hcap ? d.slot_state[h[a][k]] : 0u;
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                const uint32_t base = (w0 + (uint32_t)a * FIN_TPB) * per_wave;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const uint32_t hs = h[a][k], state = st[a][k];
                    if (hs >= d.hcap) continue;
                    if (state > ITEM_RECS && d.item_rec[base + (uint32_t)k].id < d.n_bld + d.n_room)   // somebody spilled into the per-step counters
                        for (uint32_t j = 0; j < FREE_MAX; ++j) d.vec[(size_t)hs * FREE_MAX + j] = 0u;
                    d.hkey[hs] = HKEY_EMPTY;
                    if (state) d.slot_state[hs] = 0u;
                }
                for (uint32_t k = 4u; k < used[a]; ++k) {                     // (more than four ids per wavefront: many Infected)
                    const uint32_t hs = d.hitems[base + k];
                    if (hs >= d.hcap) continue;
                    const uint32_t state = d.slot_state[hs];
                    if (state > ITEM_RECS && d.item_rec[base + k].id < d.n_bld + d.n_room)
                        for (uint32_t j = 0; j < FREE_MAX; ++j) d.vec[(size_t)hs * FREE_MAX + j] = 0u;
                    d.hkey[hs] = HKEY_EMPTY;
                    if (state) d.slot_state[hs] = 0u;
                }
            }
        }
    }
    const uint32_t pb3 = PROF_NOW();
    if (do_next) {
        // the next chunk's census ahead and decisions
        __syncthreads();
        future_body(d, max_ahead, limit_t, win, wtmp);
        __syncthreads();
        const uint32_t pb4 = PROF_NOW();
        if (tid < 64u) decide_body(d, max_ahead, limit_t, 1);
        BOOKS_PROF(d, 4, pb4 - pb3);
    }
    BOOKS_PROF(d, 0, pb1 - pb0); BOOKS_PROF(d, 1, pb2 - pb1); BOOKS_PROF(d, 2, pb3 - pb2); BOOKS_PROF(d, 3, PROF_NOW() - pb3);
    (void)pb0; (void)pb1; (void)pb2; (void)pb3;
}

__global__ __launch_bounds__(FIN_TPB) void k_chunk_books(Dev d, int fused, int do_next, uint32_t max_ahead, uint32_t limit_t)
{
    __shared__ BooksShared bs;
    books_body(d, fused, do_next, max_ahead, limit_t, bs);
}
