// esim_kernels_plan.h -- the plan of a chunk of up to 96 time steps: the census ahead and the decisions (k_future, k_decide), the
// vaccinations planned inside a chunk and their repair (k_vax_live, k_chunk_lost, k_lost_global, k_chunk_vax), and what sharded
// chunks exchange before they decide (k_shared_pack, k_shard_prep).
#pragma once
#include "esim_kernels_common.h"
#include "esim_kernels_step.h"
// ------------------------------------------------------------------------------- chunk set-up
// A citizen exposed in step t is Infected no earlier than step t + exposed_time + 1 (disease.rs:47-71), so the
// Infected census of the next <= exposed_time + 1 steps is already fixed -- as long as nobody is vaccinated.
// k_future writes that vector for this shard (sharded runs SUM-all-reduce it); k_decide then runs the
// intervention state machine (interventions.rs:110-184 needs nothing but the infected fraction) and the
// schedule (citizen.rs:176-206) over the chunk and stops in front of the step that would start vaccinating.
// Inclusive prefix sum over BF_WIN values in shared memory, by a workgroup of FIN_TPB = BF_WIN threads.
#define BF_WIN 1024
__device__ __forceinline__ void block_scan_1024(uint32_t *v, uint32_t *wtmp)
{
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    uint32_t x = v[tid];
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const uint32_t y = __shfl_up(x, o, 64); if (lane >= (uint32_t)o) x += y; }
    if (lane == 63u) wtmp[wv] = x;
    __syncthreads();
    if (tid == 0) { uint32_t a = 0; for (uint32_t w = 0; w < FIN_TPB / 64; ++w) { const uint32_t y = wtmp[w]; wtmp[w] = a; a += y; } }
    __syncthreads();
    v[tid] = x + wtmp[wv];
    __syncthreads();
}

// (Control block, histogram and census vector are read past the caches: in k_chunk_books the same workgroup has just
// written them.)
__device__ __forceinline__ void future_body(const Dev &d, uint32_t max_ahead, uint32_t limit_t, uint32_t *win, uint32_t *wtmp)
{
    Ctrl *ctrl = d.ctrl;
    const uint32_t t0 = ld(&ctrl->t), tid = threadIdx.x;                   // t0: first step of the chunk
    const uint32_t n_ahead = steps_ahead(t0, limit_t, max_ahead);
    const int et = (int)d.exposed_time, it = (int)d.infected_time;
    const int base_idx = (int)(t0 + TE_BIAS) - et - 1 - it;               // lowest entry of the first Infected window
    { const int k = base_idx + (int)tid; win[tid] = (k >= 0 && k < (int)TE_SLOTS) ? ld(&d.hist[k]) : 0u; }
    __syncthreads();
    block_scan_1024(win, wtmp);                                            // win[i] = sum of hist[base_idx .. base_idx + i]
    if (tid < n_ahead) {
        // Infected window of step t0 + tid: entries [tid, tid + it] of the loaded range
        const uint32_t hi = win[tid + (uint32_t)it], lo = tid ? win[tid - 1u] : 0u;
        d.xf[tid] = hi - lo;
    }
    if (tid == 0) {
        ctrl->future_t0 = t0;
        // citizens Infected in at least one step of the chunk: exposure steps [first window's low end, last window's top]
        const uint32_t pairs = n_ahead ? win[n_ahead - 1u + (uint32_t)it] : 0u;
        ctrl->chunk_pairs = pairs;
        // Can this shard draw the chunk in one pass?  A citizen marks at most its home, its work building, its room and
        // its route.  The word after the census counts the shards that cannot, so that after the all-reduce every shard
        // takes the same form of the chunk (speculatively enqueued chunks advance on all shards or on none).
        const bool fits = d.items_cap && d.max_route <= CHUNK_ROUTE_MAX && d.n_routes < (1u << 25) &&
                          (unsigned long long)pairs * 4ull + 65536ull <= (unsigned long long)d.items_cap;
        d.xf[d.xf_n] = fits ? 0u : 1u;
    }
}

__global__ __launch_bounds__(FIN_TPB) void k_future(Dev d, uint32_t max_ahead, uint32_t limit_t)
{
    __shared__ uint32_t win[BF_WIN];
    __shared__ uint32_t wtmp[FIN_TPB / 64];
    future_body(d, max_ahead, limit_t, win, wtmp);
}

// Highest set bit index of m, -1 when m == 0.
__device__ __forceinline__ int top_bit(unsigned long long m) { return m ? 63 - __clzll((long long)m) : -1; }

// (g after f) for transition functions on the three mask states, two bits per state.
__device__ __forceinline__ uint32_t mask_compose(uint32_t g, uint32_t f)
{
    return ((g >> (2u * (f & 3u))) & 3u) | (((g >> (2u * ((f >> 2) & 3u))) & 3u) << 2) | (((g >> (2u * ((f >> 4) & 3u))) & 3u) << 4);
}

__device__ __forceinline__ void decide_body(const Dev &d, uint32_t max_ahead, uint32_t limit_t, int allow_parallel, int vax_in_census = 0)
{
    // One wavefront, no serial loop.  Lane l evaluates the (strict) threshold tests of steps l and 64 + l
    // (interventions.rs:116-170).  Then, per step j of the chunk:
    //   lockdown in force      = the lockdown test of step j - 1                     (interventions.rs:116-128)
    //   at_work / bus_dir      = set by the last step <= j that ran its schedule arm  (citizen.rs:176-206: a locked-down
    //                            step runs none), found with ballots and count-leading-zeros
    //   mask status in force   = the three-state machine of interventions.rs:142-180 applied to steps 0..j-1: an
    //                            exclusive scan of transition functions under composition
    Ctrl *ctrl = d.ctrl;
    const uint32_t lane = threadIdx.x;
    const uint32_t t0 = ld(&ctrl->t);
    const uint32_t n_ahead = steps_ahead(t0, limit_t, max_ahead);
    const uint32_t lim_in = n_ahead < FREE_MAX ? n_ahead : FREE_MAX;
    // under a vaccination programme only a chunk whose vaccinations are planned may run (k_chunk_vax); the Infected census ahead
    // then loses those the plan vaccinates before (prefix sums of xf_adj)
    const bool vax = ld(&ctrl->have_elig) != 0u;
    const bool ok = (vax ? (ld(&ctrl->vax_chunk) != 0u && ld(&ctrl->vax_fail) == 0u) : !ld(&ctrl->vacc_active)) && !ld(&ctrl->finished) && !ld(&ctrl->error) && ld(&ctrl->future_t0) == t0;
    uint32_t adj[2] = { 0u, 0u };
    if (vax && ok && !vax_in_census) {                    // (sharded: folded into buffer F before its all-reduce, k_shard_prep)
        uint32_t carry = 0u;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const uint32_t jj = 64u * r + lane;
            uint32_t x = jj < FREE_MAX ? ld(&d.xf_adj[jj]) : 0u;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) { const uint32_t y = __shfl_up(x, o, 64); if (lane >= (uint32_t)o) x += y; }
            adj[r] = x + carry;
            carry += __shfl(x, 63, 64);
        }
    }
    const uint32_t lock_init = ld(&ctrl->lockdown), mask_init = ld(&ctrl->mask), work_init = ld(&ctrl->at_work), bus_init = ld(&ctrl->bus_dir);
    unsigned long long m_vacc[2], m_lock[2];
    uint32_t f_mask[2];                                   // transition function of the lane's step in each round
    bool in[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const uint32_t j = 64u * r + lane;
        in[r] = j < lim_in && t0 + j <= d.max_steps;
        const double x = in[r] ? (double)(ld(&d.xf[j]) + adj[r]) / (double)d.n_global : 0.0;   // infected_percentage, statistics.rs:252
        m_vacc[r] = __ballot(in[r] && d.thr_vacc < x);
        m_lock[r] = __ballot(in[r] && d.thr_lockdown < x);
        const uint32_t from_none = (in[r] && d.thr_mask_pt < x) ? 1u : 0u;
        const uint32_t from_pt = !in[r] ? 1u : (x < d.thr_mask_pt ? 0u : (d.thr_mask_all < x ? 2u : 1u));
        const uint32_t from_all = (in[r] && x < d.thr_mask_all) ? 1u : 2u;
        f_mask[r] = from_none | (from_pt << 2) | (from_all << 4);
    }
    // steps before the one that starts the vaccination programme
    uint32_t n_ok = 0;
    if (ok) {
        const unsigned long long valid0 = __ballot(in[0]), valid1 = __ballot(in[1]);
        const uint32_t n_valid = (uint32_t)(__popcll(valid0) + __popcll(valid1));
        const uint32_t first_v = m_vacc[0] ? (uint32_t)__ffsll((long long)m_vacc[0]) - 1u : (m_vacc[1] ? 64u + (uint32_t)__ffsll((long long)m_vacc[1]) - 1u : n_valid);
        n_ok = (!vax && first_v < n_valid) ? first_v : n_valid;             // (a programme that runs cannot start again)
    }
    // exclusive scan of the mask transition functions (identity = 0b100100)
    uint32_t pre[2];
    uint32_t carry = 0x24u;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        uint32_t incl = f_mask[r];
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const uint32_t y = __shfl_up(incl, o, 64); if (lane >= (uint32_t)o) incl = mask_compose(incl, y); }
        uint32_t excl = __shfl_up(incl, 1, 64);
        if (lane == 0) excl = 0x24u;
        pre[r] = mask_compose(excl, carry);               // everything before this step, earlier round first
        carry = mask_compose(__shfl(incl, 63, 64), carry);
    }
    const Decision none = { 0u, 0u, 0u, 0u };
    Decision mine[2] = { none, none };
    unsigned long long run_mask[2];                       // steps that run their schedule arm (not locked down)
    uint32_t lockd[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const uint32_t j = 64u * r + lane;
        const bool prev_lock = j == 0 ? lock_init != 0u : (j == 64u ? ((m_lock[0] >> 63) & 1ull) != 0ull : ((m_lock[r] >> (lane - 1u)) & 1ull) != 0ull);
        lockd[r] = prev_lock ? 1u : 0u;
        run_mask[r] = __ballot(!prev_lock);
    }
    // at_work and bus_dir: last deciding step at or before j, over both rounds
    unsigned long long s1[2], s0[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const uint32_t h = (t0 + 64u * r + lane) % 24u;
        s1[r] = __ballot(!lockd[r] && h == d.start_hour);
        s0[r] = __ballot(!lockd[r] && h == d.end_hour);
    }
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const unsigned long long le = lane == 63u ? ~0ull : ((1ull << (lane + 1u)) - 1ull);
        // position: the latest "starts work" / "goes home" arm among the steps that ran
        int last1 = top_bit(s1[r] & le), last0 = top_bit(s0[r] & le);
        if (r == 1) { last1 = last1 >= 0 ? last1 + 64 : top_bit(s1[0]); last0 = last0 >= 0 ? last0 + 64 : top_bit(s0[0]); }
        const uint32_t at_work = last1 > last0 ? 1u : (last0 > last1 ? 0u : work_init);
        // bus: the latest step that ran any arm decides (every arm assigns on_public_transport)
        int last_run = top_bit(run_mask[r] & le);
        if (r == 1) last_run = last_run >= 0 ? last_run + 64 : top_bit(run_mask[0]);
        uint32_t bus_dir = bus_init;
        if (last_run >= 0) {
            const uint32_t hh = (t0 + (uint32_t)last_run) % 24u;
            bus_dir = hh == d.start_hour - 1u ? 1u : (hh == d.end_hour - 1u ? 2u : 0u);
        }
        const uint32_t msk = (pre[r] >> (2u * mask_init)) & 3u;
        mine[r] = Decision{ lockd[r], msk, at_work, bus_dir };
    }
    if (allow_parallel) {
        // A one-pass chunk registers at most CHUNK_BUS_STEPS steps with riders on a bus (two a day -- unless a lockdown froze
        // them there, Q8: then every step is one).  Rather than give up the form, the chunk ends in front of the step that
        // would be one too many.
        const unsigned long long b0 = __ballot(lane < n_ok && mine[0].bus_dir != 0u), b1 = __ballot(64u + lane < n_ok && mine[1].bus_dir != 0u);
        const unsigned long long lt_ = (1ull << lane) - 1ull;
        const uint32_t before0 = (uint32_t)__popcll(b0 & lt_), before1 = (uint32_t)(__popcll(b0) + __popcll(b1 & lt_));
        const unsigned long long over0 = __ballot(((b0 >> lane) & 1ull) && before0 == CHUNK_BUS_STEPS);
        const unsigned long long over1 = __ballot(((b1 >> lane) & 1ull) && before1 == CHUNK_BUS_STEPS);
        if (over0) n_ok = (uint32_t)__ffsll((long long)over0) - 1u;
        else if (over1) n_ok = 64u + (uint32_t)__ffsll((long long)over1) - 1u;
    }
    // what is in force after the chunk = what would be in force during step n_ok, except that position and bus
    // are those of step n_ok - 1 (k_batch_finish reads them from there)
    if (lane < n_ok) d.dec[lane] = mine[0];
    if (64u + lane < n_ok) d.dec[64u + lane] = mine[1];
    {
        // entry n_ok: lockdown / mask after the last step of the chunk; computed by the lane that owns step n_ok when
        // it exists in the arrays, else from the scan totals
        const uint32_t jn = n_ok;
        uint32_t lock_after, mask_after;
        if (jn == 0) { lock_after = lock_init; mask_after = mask_init; }
        else {
            const uint32_t jl = jn - 1u;                                  // last step of the chunk
            lock_after = (uint32_t)((m_lock[jl >> 6] >> (jl & 63u)) & 1ull);
            // mask after step jl = f_jl applied to the mask in force during jl
            const uint32_t f_last = __shfl(jl < 64u ? f_mask[0] : f_mask[1], (int)(jl & 63u), 64);
            const uint32_t pre_last = __shfl(jl < 64u ? pre[0] : pre[1], (int)(jl & 63u), 64);
            mask_after = (mask_compose(f_last, pre_last) >> (2u * mask_init)) & 3u;
        }
        const uint32_t aw_last = jn ? __shfl(jn - 1u < 64u ? mine[0].at_work : mine[1].at_work, (int)((jn - 1u) & 63u), 64) : work_init;
        const uint32_t bd_last = jn ? __shfl(jn - 1u < 64u ? mine[0].bus_dir : mine[1].bus_dir, (int)((jn - 1u) & 63u), 64) : bus_init;
        if (lane == 0) d.dec[jn] = Decision{ lock_after, mask_after, aw_last, bd_last };
    }
    const unsigned long long bus_m0 = __ballot(lane < n_ok && mine[0].bus_dir != 0u), bus_m1 = __ballot(64u + lane < n_ok && mine[1].bus_dir != 0u);
    for (uint32_t i = lane; i < HOT_RESET; i += 64u) d.hot[i * HOT_STRIDE] = 0u;
    if (lane == 0) {
        ctrl->chunk_ok = n_ok; ctrl->chunk_t0 = t0;
        // the log slice of everybody Infected in some step of the chunk (k_chunk_marks starts from it)
        const int lo_te = (int)(t0 + TE_BIAS) - (int)d.exposed_time - 1 - (int)d.infected_time;
        const int hi_te = (int)(t0 + n_ok + TE_BIAS) - (int)d.exposed_time - 2;
        ctrl->chunk_i0 = (hi_te < 0 || n_ok == 0u) ? 0u : ld(&d.log_off[lo_te < 0 ? 0 : lo_te]);
        ctrl->chunk_i1 = (hi_te < 0 || n_ok == 0u) ? 0u : ld(&d.log_off[hi_te + 1]);
        // riders are on a bus in at most CHUNK_BUS_STEPS steps of a one-pass chunk (two a day unless a lockdown froze them
        // there, Q8): that bounds the (route, bus step) pairs a wavefront of k_chunk_marks can register.  The same on all shards.
        const uint32_t bus_steps = (uint32_t)(__popcll(bus_m0) + __popcll(bus_m1));
        ctrl->chunk_parallel = (allow_parallel && ld(&d.xf[d.xf_n]) == 0u && bus_steps <= CHUNK_BUS_STEPS) ? 1u : 0u;
        ctrl->chunk_bus = bus_steps;
        ctrl->n_items = 0u; ctrl->n_newexp = 0u; ctrl->n_units = 0u; ctrl->unit_next = 0u;   // (n_route_pairs_big: the last chunk's, esim_debug_counters)
    }
    d.cursor[lane] = 0u;
    if (lane < FREE_MAX - 64u) d.cursor[64u + lane] = 0u;
    // (the plan's census adjustments have been used -- by this kernel, or folded into buffer F by k_shard_prep --: zero for the next plan)
    d.xf_adj[lane] = 0u;
    if (lane < FREE_MAX + 2u - 64u) d.xf_adj[64u + lane] = 0u;
}

// vax_in_census: the plan's census adjustments are already folded into buffer F (sharded chunks: k_shard_prep, before the all-reduce)
__global__ __launch_bounds__(64) void k_decide(Dev d, uint32_t max_ahead, uint32_t limit_t, int allow_parallel, int vax_in_census)
{
    decide_body(d, max_ahead, limit_t, allow_parallel, vax_in_census);
}

// ------------------------------------------------------------------ vaccination inside a chunk
// While a vaccination programme runs (simulator.rs:524-553) every step sets `vaccination_rate` citizens Vaccinated: the
// first k distinct members of citizens_eligible_for_vaccine in the candidate sequence of that step (RNG contract,
// DESIGN.md 2).  Candidates are pure functions of (i, step), and the eligible set only ever loses citizens that are exposed
// on public transport (simulator.rs:447-449, Q10) -- so who is vaccinated when is known for a whole chunk ahead, up to those
// few removals.  k_chunk_vax plans the chunk: workgroup j takes step t0 + j, walks its candidate sequence exactly as
// k_finish does, notes the chosen citizens (Dev::vax_ev) and leaves "Vaccinated at the end of step j" in their words
// (earliest step wins, atomicMax on the vax field).  Everything downstream reads the field: an Infected citizen stops
// marking after that step (k_chunk_marks), a Susceptible one takes no draw after it (member_pairs), the census moves
// (xf_adj for the Infected counts the decisions need, k_chunk_count for the records).  The plan is speculative in
// one respect only: a citizen it chose for step j may be exposed on a bus in a step s <= j of this very chunk, which removes
// it from the set before its turn.  k_chunk_count finds the earliest such step s* (Ctrl::chunk_cut); the chunk is then
// committed up to s* - 1 and the next chunk starts AT s*.  What happens in step s* itself does not depend on the plan from s*
// on, so everybody the cut chunk saw exposed on a bus in s* will be again: k_chunk_scatter marks them (CW_PLAN_SKIP) and the
// next plan leaves them out -- it cannot be cut at s* again.
// Sharded runs: a candidate's eligibility is known to the shard that owns the citizen.  k_vax_live writes, for every step of
// the chunk ahead, the liveness bits of its first PLAN_W candidates (own citizens only; the shards SUM-all-reduce buffer V, the
// bits being disjoint) and, in the header, this shard's eligible count, riders and whether it can plan at all.
// REPAIR (k_vax_live<true>, before k_chunk_vax<true> walks the steps from Ctrl::replan_from on again): the liveness as it truly stood
// in each of those steps (eligible by the final word, or exposed on a bus in a LATER step of the chunk); the other steps' rows are
// zeroed (the buffer is summed in place a second time).
template <bool REPAIR>
__global__ __launch_bounds__(TPB) void k_vax_live(Dev d, uint32_t max_ahead, uint32_t limit_t)
{
    Ctrl *ctrl = d.ctrl;
    const uint32_t j = blockIdx.y, i = blockIdx.x * TPB + threadIdx.x;
    const uint32_t t0 = ctrl->t;
    const uint32_t n_chunk = ctrl->chunk_ok, from = ctrl->replan_from;
    const uint32_t n_ahead = REPAIR ? ((ctrl->vax_chunk && ctrl->chunk_parallel && from < n_chunk) ? n_chunk : 0u)
                                    : (t0 > limit_t ? 0u : (limit_t - t0 + 1u < max_ahead ? limit_t - t0 + 1u : max_ahead));   // (steps_ahead, written out: see DESIGN.md 3.15)
    if (j == 0 && blockIdx.x == 0 && threadIdx.x < XV_HEADER) {
        const uint32_t k = threadIdx.x;
        d.xv[k] = k == 0 ? ctrl->elig_count : k == 1 ? d.n_pt : k == 2 ? ((ctrl->finished || ctrl->error) ? 1u : 0u) : 0u;
        if (k == 0 && !REPAIR) ctrl->vax_fail = 0u;
    }
    bool live = false;
    if (ctrl->have_elig && j < n_ahead && (!REPAIR || j >= from)) {
        const uint32_t cand = vacc_candidate(d, i, t0 + j);
        if (cand >= d.id_base && cand - d.id_base < d.n) {
            const uint32_t w = d.cit[cand - d.id_base];
            const uint32_t e = CW_TE(w) - TE_BIAS - t0;
            const bool later_bus = REPAIR && (w & CW_BUS_EXPOSED) && CW_TE(w) < TE_RECOVERED && e < n_chunk && e > j;
            live = (eligible(w, ctrl->trigger_step) || later_bus) && !(w & CW_PLAN_SKIP);
        }
    }
    const unsigned long long m = __ballot(live);
    if ((threadIdx.x & 63u) == 0) { uint32_t *row = d.xv + XV_HEADER + (size_t)j * (PLAN_W / 32u); row[i >> 5] = (uint32_t)m; row[(i >> 5) + 1u] = (uint32_t)(m >> 32); }
}

// sharded: the liveness of the candidates comes from buffer V (k_vax_live, all-reduced), every shard walks the same sequence
// and accepts the same candidates, and keeps the events of its own citizens.
// Launched with one workgroup more than there are steps, that one makes the census ahead (k_future's work: nothing the plan reads
// or writes, and a kernel boundary costs as much as the census).
// The citizens expose_min listed (exposed on a bus with a planned vaccination in their word) whose FINAL exposure is that one: they
// left the eligible set in that step, their planned vaccination is void (the field is cleared here, before any step is walked
// again: a walk may choose the same citizen anew for an EARLIER step), and the steps from the earliest such exposure on are the
// ones k_chunk_vax<true> walks again.
__global__ __launch_bounds__(FIN_TPB) void k_chunk_lost(Dev d)
{
    __shared__ uint32_t s_from;
    Ctrl *ctrl = d.ctrl;
    const uint32_t tid = threadIdx.x;
    const uint32_t n_chunk = ctrl->chunk_ok, t0 = ctrl->t;
    const uint32_t n_lost = d.hot[HOT_LOST * HOT_STRIDE];
    if (!ctrl->vax_chunk || !ctrl->chunk_parallel || n_chunk == 0u || n_lost == 0u) return;
    if (tid == 0) s_from = FREE_MAX + 1u;
    __syncthreads();
    uint32_t lo = FREE_MAX + 1u;
    auto look = [&](uint32_t m) {
        if (m >= d.n) return;
        const uint32_t w = d.cit[m], e = CW_TE(w) - TE_BIAS - t0;
        if (!(w & CW_BUS_EXPOSED) || CW_TE(w) >= TE_RECOVERED || e >= n_chunk || CW_VAX_REL(w) == CW_VAX_NONE) return;   // (listed twice: cleared already)
        lo = min(lo, e);
        atomicAnd(&d.cit[m], ~CW_VAX_MASK);
        if (d.world > 1u) d.xl[e] = 1u;
    };
    if (n_lost <= LOST_CAP) for (uint32_t i = tid; i < n_lost; i += FIN_TPB) look(d.lost_list[i]);
    else {
        // (more than the list holds: everybody exposed in the chunk is looked at)
        const uint32_t r = tid & (SUBQ - 1u), n_new = newexp_len(d, HOT_NEWEXP, r);
        const uint32_t *list = newexp_list(d, r);
        for (uint32_t i = tid / SUBQ; i < n_new; i += FIN_TPB / SUBQ) look(list[i]);
    }
    if (lo <= FREE_MAX) atomicMin(&s_from, lo);
    __syncthreads();
    if (d.world > 1u) return;                                                 // (sharded: the earliest step of ALL shards, k_lost_global)
    if (tid == 0 && s_from <= FREE_MAX) { ctrl->replan_from = s_from; ctrl->repair_ran = 1u; ctrl->vax_repairs += 1u; }
}

// Sharded: buffer L summed over the shards -- the plan is walked again from the earliest step in which ANY shard lost a citizen.
__global__ __launch_bounds__(64) void k_lost_global(Dev d)
{
    Ctrl *ctrl = d.ctrl;
    const uint32_t lane = threadIdx.x, n = ctrl->chunk_ok;
    if (!ctrl->vax_chunk || !ctrl->chunk_parallel || n == 0u) return;
    const unsigned long long m0 = __ballot(lane < n && d.xl[lane] != 0u), m1 = __ballot(64u + lane < n && d.xl[64u + lane] != 0u);
    if (lane == 0 && (m0 | m1)) {
        ctrl->replan_from = m0 ? (uint32_t)__ffsll((long long)m0) - 1u : 64u + (uint32_t)__ffsll((long long)m1) - 1u;
        ctrl->repair_ran = 1u; ctrl->vax_repairs += 1u;
    }
}

// REPAIR (k_chunk_vax<true>, after the draws of the chunk, before its counts; unsharded contexts): a citizen the
// plan vaccinates at the end of step f was exposed on a bus in step e <= f.  It left the eligible set with that exposure, so in
// every step from e on in which it was among the chosen the walk takes the next eligible candidate instead -- and nothing else
// changes: the chosen stay in the set (Q10), so every step's walk is a function of the words alone.  Round 2 cut the chunk at e
// and threw the draws of everything behind it away (uk64m's last 200 steps, with 17 000 bus exposures per 96 steps, cost 14 of
// the run's 33 ms that way).  Now the steps from the earliest such e on are walked AGAIN, with eligibility as it truly stood in
// each step (eligible by the final word, or exposed on a bus in a LATER step of this chunk): the lists of the chosen are rewritten,
// the lost citizens' fields are cleared, the newly chosen get theirs.  A newly chosen citizen (or one whose vaccination moves to
// an earlier step) is harmless when nothing it did behind that step mattered: it is not Infected in any later step of the chunk
// (its marks would have to go, and with them the counts others were drawn with) and was not exposed in a later one.  Otherwise the
// chunk is cut BEHIND that step (chunk_cut = j + 1): everything up to and including it stands.
template <bool REPAIR>
__global__ __launch_bounds__(FIN_TPB) void k_chunk_vax(Dev d, uint32_t max_ahead, uint32_t limit_t, int sharded)
{
    __shared__ FinishShared sm;
    __shared__ uint32_t n_local;
    if (blockIdx.x >= FREE_MAX) {
        if (REPAIR) return;
        __shared__ uint32_t win[BF_WIN];
        __shared__ uint32_t wtmp[FIN_TPB / 64];
        future_body(d, max_ahead, limit_t, win, wtmp);
        return;
    }
    Ctrl *ctrl = d.ctrl;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    const uint32_t j = blockIdx.x;
    const uint32_t t0 = ctrl->t;
    uint32_t n_chunk = 0u;
    if (REPAIR) {
        n_chunk = ctrl->chunk_ok;
        const uint32_t from = ctrl->replan_from;                              // (k_chunk_lost)
        if (!ctrl->vax_chunk || !ctrl->chunk_parallel || j >= n_chunk || j < from) return;
    }
    const uint32_t n_ahead = REPAIR ? n_chunk : steps_ahead(t0, limit_t, max_ahead);
    // (every workgroup -- and, sharded, every shard -- takes the same decision from the same words; nothing here writes them)
    const uint32_t elig_all = sharded ? d.xv[0] : ctrl->elig_count, riders_all = sharded ? d.xv[1] : d.n_pt;
    const bool plan = ctrl->have_elig && !ctrl->finished && !ctrl->error && !(sharded && d.xv[2]) &&
                      elig_all > d.vaccination_rate + riders_all;      // the set cannot shrink to the "whole set" case inside the chunk
    if (REPAIR) { if (tid == 0) { d.vax_cnt[j] = 0u; d.vax_now[j] = 0u; n_local = 0u; } }
    else if (tid == 0) {
        for (uint32_t q = 0; q < 4u; ++q) d.vax_delta[q * (FREE_MAX + 2u) + j] = 0u;                // (xf_adj: zero since the last k_decide)
        d.vax_cnt[j] = 0u; d.vax_now[j] = 0u;
        n_local = 0u;
        if (j == 0) {
            d.hot[HOT_LOST * HOT_STRIDE] = 0u; ctrl->replan_from = FREE_MAX + 1u; ctrl->repair_ran = 0u;
            ctrl->vax_chunk = plan ? 1u : 0u;
            ctrl->vax_planned = plan ? n_ahead : 0u;
            if (!sharded) ctrl->vax_fail = 0u;
            ctrl->chunk_cut = FREE_MAX + 1u;
            for (uint32_t z = FREE_MAX; z < FREE_MAX + 2u; ++z) for (uint32_t q = 0; q < 4u; ++q) d.vax_delta[q * (FREE_MAX + 2u) + z] = 0u;
        }
    }
    if (!plan || j >= n_ahead) return;
    const uint32_t t = t0 + j, k = d.vaccination_rate, tstep = ctrl->trigger_step;
    const uint32_t *bits = d.xv + XV_HEADER + (size_t)j * (PLAN_W / 32u);
    for (uint32_t i = tid; i < VACC_TABLE; i += FIN_TPB) { sm.tab_key[i] = 0xFFFFFFFFu; sm.tab_idx[i] = 0xFFFFFFFFu; }
    __syncthreads();
    uint32_t already = 0;
    for (uint32_t base = 0; already < k; base += VACC_BATCH) {
        uint32_t cj[4], slot[4], cw[4]; bool live[4], mine_c[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint32_t i = base + tid * 4u + q;
            cj[q] = vacc_candidate(d, i, t);
            mine_c[q] = cj[q] >= d.id_base && cj[q] - d.id_base < d.n;
            cw[q] = mine_c[q] ? d.cit[cj[q] - d.id_base] : 0u;
            if (sharded) live[q] = i < PLAN_W && ((bits[i >> 5] >> (i & 31u)) & 1u) != 0u;
            else if (REPAIR) {
                // as the set truly stood in this step: who is exposed on a bus in a LATER step of the chunk was still in it
                const uint32_t e = CW_TE(cw[q]) - TE_BIAS - t0;
                const bool later_bus = (cw[q] & CW_BUS_EXPOSED) && CW_TE(cw[q]) < TE_RECOVERED && e < n_chunk && e > j;
                live[q] = (eligible(cw[q], tstep) || later_bus) && !(cw[q] & CW_PLAN_SKIP);
            }
            else live[q] = eligible(cw[q], tstep) && !(cw[q] & CW_PLAN_SKIP);
            slot[q] = 0;
            if (live[q]) {
                uint32_t sl = (cj[q] * 2654435761u) >> 18;        // 14 bits
                for (;;) {
                    const uint32_t old = atomicCAS(&sm.tab_key[sl], 0xFFFFFFFFu, cj[q]);
                    if (old == 0xFFFFFFFFu || old == cj[q]) break;
                    sl = (sl + 1u) & (VACC_TABLE - 1u);
                }
                atomicMin(&sm.tab_idx[sl], i);
                slot[q] = sl;
            }
        }
        __syncthreads();
        bool first[4]; uint32_t mine = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) { first[q] = live[q] && sm.tab_idx[slot[q]] == base + tid * 4u + q; mine += first[q]; }
        uint32_t incl = mine;
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
                if (pos < k && mine_c[q]) {
                    const uint32_t c = cj[q] - d.id_base;
                    d.vax_ev[(size_t)j * VACC_MAX_RATE + atomicAdd(&n_local, 1u)] = c;      // (the order inside a step does not matter)
                    // unconditional (simulator.rs:551) -- but a citizen that is Vaccinated already stays what it is
                    if (CW_TE(cw[q]) != TE_VACCINATED) {
                        const uint32_t old = atomicMax(&d.cit[c], (cw[q] & ~CW_VAX_MASK) | CW_VAX_FIELD(j));
                        if (!REPAIR && CW_TE(cw[q]) < TE_RECOVERED && (CW_VAX_REL(old) == CW_VAX_NONE || CW_VAX_REL(old) > j)) {
                            // The Infected census ahead (buffer F) counts everybody whose exposure step makes it Infected; those the plan
                            // vaccinates before leave it: the stretch of the chunk in which this citizen would have been Infected behind
                            // step j goes into the difference array xf_adj (k_decide adds its prefix sums to F) -- for the step that WINS:
                            // a step that takes the citizen over from a later one takes that one's stretch out again (round 3: a
                            // kernel of its own did this from the final words).
                            const int a = (int)CW_TE(cw[q]) - (int)TE_BIAS + (int)d.exposed_time + 1 - (int)t0, hi = min(a + (int)d.infected_time, (int)n_ahead - 1);
                            const int lo = max(a, (int)j + 1);
                            if (lo <= hi) { atomicSub(&d.xf_adj[lo], 1u); atomicAdd(&d.xf_adj[hi + 1], 1u); }
                            if (CW_VAX_REL(old) != CW_VAX_NONE) {
                                const int lo2 = max(a, (int)CW_VAX_REL(old) + 1);
                                if (lo2 <= hi) { atomicAdd(&d.xf_adj[lo2], 1u); atomicSub(&d.xf_adj[hi + 1], 1u); }
                            }
                        }
                        if (REPAIR && (CW_VAX_REL(old) == CW_VAX_NONE || CW_VAX_REL(old) > j)) {
                            // newly chosen for this step (or moved here from a later one): harmless unless something it did behind
                            // step j mattered -- Infected in a later step of the chunk, or exposed in one
                            const uint32_t te = CW_TE(cw[q]);
                            bool bad = false;
                            if (te < TE_RECOVERED) {
                                const int e = (int)te - (int)TE_BIAS - (int)t0;                                  // exposure step (may lie before the chunk)
                                const int a = e + (int)d.exposed_time + 1, b = a + (int)d.infected_time;       // Infected in steps a .. b
                                if (e > (int)j && e < (int)n_chunk) bad = true;
                                if (max(a, (int)j + 1) <= min(b, (int)n_chunk - 1)) bad = true;
                            }
                            if (bad) { atomicMin(&ctrl->chunk_cut, j + 1u); if (d.world > 1u) d.xc[j + 1u] = 1u; }
                        }
                    }
                }
                pos++;
            }
        }
        const uint32_t got = sm.s_total;
        __syncthreads();
        already += got < k - already ? got : k - already;
        if (sharded && base + VACC_BATCH >= PLAN_W && already < k) {
            // the exchanged window was too short: no plan -- or, walking a step again: the chunk ends in front of this step
            if (tid == 0) { if (REPAIR) { atomicMin(&ctrl->chunk_cut, j); d.xc[j] = 1u; } else atomicAdd(&ctrl->vax_fail, 1u); }
            break;
        }
        if (base >= (1u << 26) && already < k) { if (tid == 0) ctrl->error = (uint32_t)(-ESIM_ERANGE); break; }   // every wave must reach an exit
    }
    __syncthreads();
    if (tid == 0) { d.vax_cnt[j] = n_local; d.vax_now[j] = already; }
}

// ---------------------------------------------------------------------- sharded chunks: the commuter exchange
// A building or school room whose members live on several shards is shared (esim_shard_population).  An Infected member
// standing in it matters to every shard that has members there: per chunk, each shard sends the citizen words of its own
// Infected whose work building is shared, with the building's and the room's index in the shared tables (k_shared_pack; an
// all-to-all delivers them), and k_chunk_marks enters the received ones into its map next to its own.  The slice walked is
// the one of the longest chunk that can follow (the decisions come later); an entry whose stretch misses the chunk is dropped
// by the receiver.
__global__ __launch_bounds__(TPB) void k_shared_pack(Dev d, uint32_t max_ahead, uint32_t limit_t)
{
    const Ctrl *ctrl = d.ctrl;
    const uint32_t t0 = ctrl->t;
    const uint32_t n_ahead = steps_ahead(t0, limit_t, max_ahead);
    if (n_ahead == 0u) return;
    const int lo_te = (int)(t0 + TE_BIAS) - (int)d.exposed_time - 1 - (int)d.infected_time;
    const int hi_te = (int)(t0 + n_ahead + TE_BIAS) - (int)d.exposed_time - 2;
    if (hi_te < 0) return;
    const uint32_t i0 = d.log_off[lo_te < 0 ? 0 : lo_te], i1 = d.log_off[hi_te + 1];
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t base = i0 + (blockIdx.x * TPB + threadIdx.x - lane); base < i1; base += gridDim.x * TPB) {
        const uint32_t i = base + lane;
        uint32_t w = 0u, sb = 0u, sr = 0xFFFFFFFFu;
        bool send = false;
        if (i < i1) {
            const uint32_t c = d.log[i];
            w = d.cit[c];
            if ((w & FL_HAS_WORK) && CW_TE(w) < TE_RECOVERED) {
                const int32_t k = d.shared_of_bld[d.work[c]];
                if (k >= 0) {
                    send = true; sb = (uint32_t)k;
                    if (w & FL_WORK_SCHOOL) { const int32_t q = d.shared_of_room[d.room[c]]; sr = q >= 0 ? (uint32_t)q : 0xFFFFFFFFu; }
                }
            }
        }
        if (!__ballot(send)) continue;
        // the record goes into the segment of every OTHER shard that has members in the building
        const uint32_t to = send ? d.shared_mask[sb] & ~(1u << d.rank) : 0u;
        for (uint32_t r = 0; r < d.world; ++r) {
            const unsigned long long mr = __ballot((to >> r) & 1u);
            if (!mr) continue;
            uint32_t *out = d.xs_out + (size_t)r * (1u + 3u * d.xs_cap);
            uint32_t pos = 0u;
            if (lane == 0) pos = atomicAdd(&out[0], (uint32_t)__popcll(mr));       // one atomic per wavefront and destination
            pos = __shfl(pos, 0, 64) + (uint32_t)__popcll(mr & ((1ull << lane) - 1ull));
            if (((to >> r) & 1u) && pos < d.xs_cap) { out[1u + 3u * pos] = w; out[2u + 3u * pos] = sb; out[3u + 3u * pos] = sr; }
        }
    }
}

// Before buffer F is all-reduced: this shard's "cannot draw the chunk in one pass" word also covers the commuters received (they
// claim items too) and a segment that overflowed anywhere; and the Infected census ahead loses those the plan vaccinates before
// (prefix sums of xf_adj), so that the sum over the shards is the census the decisions need.
__global__ __launch_bounds__(128) void k_shard_prep(Dev d, uint32_t max_ahead, uint32_t limit_t)
{
    Ctrl *ctrl = d.ctrl;
    if (threadIdx.x != 0) return;
    const uint32_t t0 = ctrl->t;
    const uint32_t n_ahead = steps_ahead(t0, limit_t, max_ahead);
    uint32_t n_remote = 0u; bool overflow = false;
    for (uint32_t r = 0; r < d.world; ++r) {
        const uint32_t cnt = d.xs[(size_t)r * (1u + 3u * d.xs_cap)];
        if (cnt > d.xs_cap) overflow = true;
        if (r != d.rank) n_remote += min(cnt, d.xs_cap);
    }
    // (what this shard saw: the segments it received and those it sent; the status exchange takes the maximum over the shards,
    // so that the segments grow alike everywhere)
    ctrl->xs_need = 0u;
    for (uint32_t r = 0; r < d.world; ++r) {
        if (r == d.rank) continue;
        const uint32_t o = d.xs_out[(size_t)r * (1u + 3u * d.xs_cap)];
        ctrl->xs_need = max(ctrl->xs_need, max(o, d.xs[(size_t)r * (1u + 3u * d.xs_cap)]));
        if (o > d.xs_cap) overflow = true;
    }
    // (a shard in a device-side error state makes the chunk a no-op on EVERY shard: the word is summed)
    const bool fits = d.xf[d.xf_n] == 0u && !overflow && !ctrl->error && !ctrl->finished &&
                      ((unsigned long long)ctrl->chunk_pairs + n_remote) * 4ull + 65536ull <= (unsigned long long)d.items_cap;
    d.xf[d.xf_n] = fits ? 0u : 1u;
    if (ctrl->vax_chunk && !ctrl->vax_fail) {
        uint32_t a = 0u;
        for (uint32_t j = 0; j < n_ahead; ++j) { a += d.xf_adj[j]; d.xf[j] += a; }
    }
    for (uint32_t j = 0; j < FREE_MAX + 2u; ++j) { d.xc[j] = 0u; d.xl[j] = 0u; }
}
