// esim_kernels_tree.h -- who infected whom: the infector of every logged exposure, derived after the fact on top of
// the settings of esim_kernels_setting.h.  The CANDIDATES of an exposure of citizen c in step ts are the citizens Infected in ts
// that stand where the exposure is credited -- its household, its work place, its own school room, its bus -- in ascending
// citizen index; the infector is candidate ((uint64_t)u * k) >> 32 with u the Philox word of slot ESIM_SLOT_INFECTOR.
// k_tree_home picks inside households, a lane per citizen, and queues every other exposure; k_tree_wide gives a whole wavefront
// to each queued one (a work place has thousands of workers), k_tree_route to each on a route longer than a bus, whose thousands
// of riders are put in their order of that step again; k_tree_gen turns infectors into generations; k_tree_offspring, k_tree_rows and k_tree_matrix count.  Nothing here writes
// simulation state.
#pragma once

#ifndef TREE_QCAP
#define TREE_QCAP 2048u             // Infected riders of one route a wavefront of k_tree_route keeps in LDS at a time (more: in rounds; -DTREE_QCAP=64 tested)
#endif
#define TREE_FLAG 0x80000000u       // on a queued rider: it shares the bus

struct Tree {
    uint32_t *infector, *n_cand, *gen;   // [n] ESIM_NO_INFECTOR / 0 / ESIM_NEVER where there is none
    uint32_t *queue;                     // [q_cap] citizens whose exposure a wavefront explains: k_tree_wide's from the front, k_tree_route's
    uint32_t q_cap;                      // (a route longer than a bus) from the back
    uint32_t *n_queue, *n_long;          // entries at the front, at the back
    uint32_t *orphans;                   // exposures without a candidate
    uint32_t *bus = nullptr;             // [n] zeroed by the caller, or nullptr: the bus number of an exposure on a route longer than a bus
};

// The seed an exposure of step ts was drawn under: the snapshot's up to the seam of a rollback.
__device__ __forceinline__ uint64_t tree_seed(const Dev &d, const Setting &q, int ts)
{
    const bool old = (uint32_t)ts <= q.seam_step && q.old_thr;
    return old ? ((uint64_t)q.old_seed_hi << 32) | q.old_seed_lo : ((uint64_t)d.seed_hi << 32) | d.seed_lo;
}

// The candidate an exposure of citizen c in step ts with k candidates picks.
__device__ __forceinline__ uint32_t tree_pick(const Dev &d, const Setting &q, uint32_t c, int ts, uint32_t k)
{
    const uint32_t u = esim_u32(tree_seed(d, q, ts), d.id_base + c, (uint32_t)ts, ESIM_SLOT_INFECTOR);
    return (uint32_t)(((uint64_t)u * k) >> 32);
}

// A lane per citizen, as k_setting_attr walks its household: count the candidates, pick, walk again up to the pick.  Exposures
// credited elsewhere are appended to the queue, one atomic per wavefront.  Every lane of a wavefront makes the same trips.
__global__ __launch_bounds__(TPB) void k_tree_home(Dev d, Setting q, Tree t)
{
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t c0 = (uint64_t)blockIdx.x * TPB; c0 < (uint64_t)d.n; c0 += (uint64_t)gridDim.x * TPB) {
        const uint64_t c64 = c0 + threadIdx.x;
        const uint32_t c = (uint32_t)c64;
        bool wide = false, route = false;
        if (c64 < (uint64_t)d.n) {
            const uint32_t s = q.setting[c], te = q.te_of[c];
            const int ts = (int)te - (int)TE_BIAS;
            uint32_t who = ESIM_NO_INFECTOR, k = 0u;
            if (s == ESIM_SETTING_HOUSEHOLD) {
                const bool work_hour = q.at_work[ts] != 0u, bus_hour = q.on_bus[ts] != 0u;
                const uint32_t b = d.home[c];
                uint32_t lo = 0u, hi = 0u;
                if (b < d.n_bld) { lo = d.res_off[b]; hi = d.res_off[b + 1u]; }
                if (lo > hi || hi > d.n) hi = lo;
                for (uint32_t r = lo; r < hi; ++r) {
                    const uint32_t m = d.res_idx ? d.res_idx[r] : r;
                    if (m < d.n && infected_at_home(d, q, m, ts, work_hour, bus_hour)) ++k;
                }
                if (k) {
                    uint32_t left = tree_pick(d, q, c, ts, k);
                    for (uint32_t r = lo; r < hi; ++r) {
                        const uint32_t m = d.res_idx ? d.res_idx[r] : r;
                        if (m < d.n && infected_at_home(d, q, m, ts, work_hour, bus_hour) && left-- == 0u) { who = m; break; }
                    }
                } else atomicAdd(t.orphans, 1u);
            } else if (s == ESIM_SETTING_TRANSPORT) {
                const uint32_t r = d.route_of[c];
                route = r < d.n_routes && d.route_off[r + 1u] - d.route_off[r] > d.bus_capacity;
                wide = !route;
            } else if (s < ESIM_N_SETTINGS) wide = true;
            t.infector[c] = who;
            t.n_cand[c] = k;
            t.gen[c] = (te != SETTING_TE_NONE && ts < 1) ? 0u : ESIM_NEVER;     // (the index cases lie before step 1)
        }
        for (int back = 0; back < 2; ++back) {
            const bool mine = back ? route : wide;
            const unsigned long long m = __ballot(mine);
            if (!m) continue;
            const uint32_t lead = (uint32_t)__ffsll((long long)m) - 1u;
            uint32_t base = 0u;
            if (lane == lead) base = atomicAdd(back ? t.n_long : t.n_queue, (uint32_t)__popcll(m));
            base = __shfl(base, lead, 64);
            const uint32_t at = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
            if (mine && at < t.q_cap) t.queue[back ? t.q_cap - 1u - at : at] = c;   // (front and back together hold at most the log's entries)
        }
    }
}

// Is member m of a work place or school room a candidate in step ts: Infected, at work and not on a bus?  (The bus hour before
// end_hour has both bits set; an Infected rider marks no building then.)
__device__ __forceinline__ bool infected_at_work(const Dev &d, const Setting &q, uint32_t m, int ts, bool work_hour, bool bus_hour)
{
    if (!work_hour || !in_infected_steps(d, q, m, ts)) return false;
    const uint32_t w = d.cit[m];
    if (!(w & FL_HAS_WORK) || (bus_hour && (w & FL_USES_PT))) return false;
    return !vaccinated_before(q, m, w, ts);
}

// Is rider m Infected in step ts?  (Everybody on a route rides while the bus bit is set.)
__device__ __forceinline__ bool infected_rider(const Dev &d, const Setting &q, uint32_t m, int ts)
{
    return in_infected_steps(d, q, m, ts) && !vaccinated_before(q, m, d.cit[m], ts);
}

// kind of a member list: 0 work place or room, 1 route
template <int KIND>
__device__ __forceinline__ bool tree_member_ok(const Dev &d, const Setting &q, uint32_t m, int ts, bool work_hour, bool bus_hour)
{
    return KIND == 0 ? infected_at_work(d, q, m, ts, work_hour, bus_hour) : infected_rider(d, q, m, ts);
}

// One member list [lo, hi) by one wavefront: the 64 lanes stride over it, ids read coalesced, the exposure step and the citizen
// word gathered; candidates counted with ballots, then the stretch that holds the pick is found the same way and the pick in it
// by its prefix popcount.  Returns the infector (wave-uniform) and the number of candidates.
template <int KIND>
__device__ __forceinline__ uint32_t tree_member_list(const Dev &d, const Setting &q, const uint32_t *idx, uint32_t lo, uint32_t hi, uint32_t c, int ts,
                                                     bool work_hour, bool bus_hour, uint32_t lane, uint32_t *k_out)
{
    uint32_t k = 0u;
    for (uint32_t b = lo; b < hi; b += 64u) {
        const uint32_t i = b + lane;
        const uint32_t m = i < hi ? idx[i] : 0xFFFFFFFFu;
        k += (uint32_t)__popcll(__ballot(m < d.n && tree_member_ok<KIND>(d, q, m, ts, work_hour, bus_hour)));
    }
    *k_out = k;
    if (!k) return ESIM_NO_INFECTOR;
    const uint32_t pick = tree_pick(d, q, c, ts, k);
    uint32_t seen = 0u;
    for (uint32_t b = lo; b < hi; b += 64u) {
        const uint32_t i = b + lane;
        const uint32_t m = i < hi ? idx[i] : 0xFFFFFFFFu;
        const bool ok = m < d.n && tree_member_ok<KIND>(d, q, m, ts, work_hour, bus_hour);
        const unsigned long long cand = __ballot(ok);
        const uint32_t here = (uint32_t)__popcll(cand);
        if (pick < seen + here) {
            const unsigned long long mine = __ballot(ok && (uint32_t)__popcll(cand & ((1ull << lane) - 1ull)) == pick - seen);
            return __shfl(m, (int)((uint32_t)__ffsll((long long)mine) - 1u), 64);
        }
        seen += here;
    }
    return ESIM_NO_INFECTOR;
}

// The key that orders the riders of a route in step ts (k_expose, route_pair_small / route_pair_big): the step is the counter
// word itself.
__device__ __forceinline__ uint32_t tree_bus_key(const Dev &d, uint64_t seed, uint32_t m, int ts)
{
    return philox4x32_10(d.id_base + m, (uint32_t)ts, ESIM_SLOT_BUS_ORDER, 0u, (uint32_t)seed, (uint32_t)(seed >> 32)).w0;
}

struct TreeShared {
    uint32_t key[CHUNK_ROUTE_MAX];      // the riders' keys, routes up to CHUNK_ROUTE_MAX riders (longer ones: drawn again)
    uint32_t rider[TREE_QCAP];          // positions in the route of the Infected riders of this round, ascending; TREE_FLAG: on c's bus
};

// Pass one over a route of sz riders from `off`: every rider's key drawn (and kept where the route fits), the riders in front of
// c counted, the Infected riders number [q_lo, q_lo + TREE_QCAP) queued in LDS by position.  Riders ascend with their position,
// so (key, position) orders as (key, citizen) does.  Returns the Infected riders of the route; *front: the rank of c.
__device__ __forceinline__ uint32_t tree_route_scan(const Dev &d, const Setting &q, TreeShared &sm, uint32_t off, uint32_t sz, uint32_t c, int ts,
                                                    uint64_t seed, bool keep, uint32_t q_lo, uint32_t lane, uint32_t *front)
{
    const uint32_t key_c = tree_bus_key(d, seed, c, ts);
    uint32_t n_inf = 0u, ahead = 0u;
    for (uint32_t b = 0u; b < sz; b += 64u) {
        const uint32_t i = b + lane;
        const uint32_t m = i < sz ? d.route_riders[off + i] : 0xFFFFFFFFu;
        const bool valid = m < d.n;
        const uint32_t key = valid ? tree_bus_key(d, seed, m, ts) : 0xFFFFFFFFu;
        if (keep && i < sz) sm.key[i] = key;
        ahead += (uint32_t)__popcll(__ballot(valid && (key < key_c || (key == key_c && m < c))));
        const bool inf = valid && infected_rider(d, q, m, ts);
        const unsigned long long im = __ballot(inf);
        const uint32_t slot = n_inf + (uint32_t)__popcll(im & ((1ull << lane) - 1ull));
        if (inf && slot >= q_lo && slot - q_lo < TREE_QCAP) sm.rider[slot - q_lo] = i;
        n_inf += (uint32_t)__popcll(im);
    }
    *front = ahead;
    __syncthreads();
    return n_inf;
}

// The nq queued Infected riders, 64 at a time, ranked against all riders of the route by the exact (key, position) compare: a
// lane is an Infected rider, the riders' keys are broadcast -- from LDS, or drawn again 64 at a time and shuffled.  Those whose
// rank falls into bus `bus` get TREE_FLAG; returns their number.
__device__ __forceinline__ uint32_t tree_route_rank(const Dev &d, TreeShared &sm, uint32_t off, uint32_t sz, int ts, uint64_t seed, bool keep,
                                                    uint32_t nq, uint32_t bus, uint32_t lane)
{
    uint32_t on_bus = 0u;
    for (uint32_t b = 0u; b < nq; b += 64u) {
        const bool have = b + lane < nq;
        const uint32_t pos = have ? sm.rider[b + lane] & ~TREE_FLAG : 0u;
        uint32_t rank = 0u;
        if (keep) {
            if (have) rank = rank_block_exact(sm.key, sm.key[pos], pos, sz);
        } else {
            const uint32_t mine = have ? d.route_riders[off + pos] : 0xFFFFFFFFu;
            const uint32_t key = mine < d.n ? tree_bus_key(d, seed, mine, ts) : 0xFFFFFFFFu;
            for (uint32_t jb = 0u; jb < sz; jb += 64u) {
                const uint32_t j = jb + lane;
                const uint32_t mj = j < sz ? d.route_riders[off + j] : 0xFFFFFFFFu;
                const uint32_t kj = mj < d.n ? tree_bus_key(d, seed, mj, ts) : 0xFFFFFFFFu;
                const uint32_t n = sz - jb < 64u ? sz - jb : 64u;
                for (uint32_t l = 0u; l < n; ++l) {
                    const uint32_t kl = __shfl(kj, (int)l, 64);
                    rank += kl < key || (kl == key && jb + l < pos);
                }
            }
        }
        const bool same = have && rank / d.bus_capacity == bus;
        if (have) sm.rider[b + lane] = pos | (same ? TREE_FLAG : 0u);
        on_bus += (uint32_t)__popcll(__ballot(same));
    }
    __syncthreads();
    return on_bus;
}

// The citizen at the pick-th flagged entry of the nq queued riders (wave-uniform).
__device__ __forceinline__ uint32_t tree_route_take(const Dev &d, const TreeShared &sm, uint32_t off, uint32_t nq, uint32_t pick, uint32_t lane)
{
    uint32_t seen = 0u;
    for (uint32_t b = 0u; b < nq; b += 64u) {
        const uint32_t e = b + lane < nq ? sm.rider[b + lane] : 0u;
        const bool ok = (e & TREE_FLAG) != 0u;
        const unsigned long long cand = __ballot(ok);
        const uint32_t here = (uint32_t)__popcll(cand);
        if (pick < seen + here) {
            const unsigned long long mine = __ballot(ok && (uint32_t)__popcll(cand & ((1ull << lane) - 1ull)) == pick - seen);
            const uint32_t pos = __shfl(e & ~TREE_FLAG, (int)((uint32_t)__ffsll((long long)mine) - 1u), 64);
            return d.route_riders[off + pos];
        }
        seen += here;
    }
    return ESIM_NO_INFECTOR;
}

// A route longer than a bus: the Infected riders of c's bus.  With more than TREE_QCAP Infected on the route they are ranked in
// rounds, once to count and once more up to the round that holds the pick.
__device__ __forceinline__ uint32_t tree_route_long(const Dev &d, const Setting &q, TreeShared &sm, uint32_t off, uint32_t sz, uint32_t c, int ts,
                                                    uint32_t lane, uint32_t *k_out, uint32_t *bus_out)
{
    const uint64_t seed = tree_seed(d, q, ts);
    const bool keep = sz <= CHUNK_ROUTE_MAX;
    uint32_t front = 0u, k = 0u;
    const uint32_t n_inf = tree_route_scan(d, q, sm, off, sz, c, ts, seed, keep, 0u, lane, &front);
    const uint32_t bus = front / d.bus_capacity;
    *bus_out = bus;
    for (uint32_t q_lo = 0u; q_lo < n_inf; q_lo += TREE_QCAP) {
        if (q_lo) (void)tree_route_scan(d, q, sm, off, sz, c, ts, seed, keep, q_lo, lane, &front);
        k += tree_route_rank(d, sm, off, sz, ts, seed, keep, n_inf - q_lo < TREE_QCAP ? n_inf - q_lo : TREE_QCAP, bus, lane);
    }
    *k_out = k;
    if (!k) return ESIM_NO_INFECTOR;
    const uint32_t pick = tree_pick(d, q, c, ts, k);
    if (n_inf <= TREE_QCAP) return tree_route_take(d, sm, off, n_inf, pick, lane);
    uint32_t seen = 0u;
    for (uint32_t q_lo = 0u; q_lo < n_inf; q_lo += TREE_QCAP) {
        const uint32_t nq = n_inf - q_lo < TREE_QCAP ? n_inf - q_lo : TREE_QCAP;
        (void)tree_route_scan(d, q, sm, off, sz, c, ts, seed, keep, q_lo, lane, &front);
        const uint32_t here = tree_route_rank(d, sm, off, sz, ts, seed, keep, nq, bus, lane);
        if (pick < seen + here) return tree_route_take(d, sm, off, nq, pick - seen, lane);
        seen += here;
    }
    return ESIM_NO_INFECTOR;
}

// One wavefront per exposure queued at the front: a work place, a school room, or a route that fills one bus at most.
__global__ __launch_bounds__(TPB) void k_tree_wide(Dev d, Setting q, Tree t)
{
    const uint32_t lane = threadIdx.x & 63u, wave = blockIdx.x * (TPB / 64u) + (threadIdx.x >> 6), n_waves = gridDim.x * (TPB / 64u);
    const uint32_t n_q = *t.n_queue < t.q_cap ? *t.n_queue : t.q_cap;
    for (uint32_t e = wave; e < n_q; e += n_waves) {
        const uint32_t c = t.queue[e];
        if (c >= d.n) continue;                                            // (wave-uniform, as everything below)
        const uint32_t s = q.setting[c], te = q.te_of[c];
        const int ts = (int)te - (int)TE_BIAS;
        if (te == SETTING_TE_NONE || ts < 1 || ts > (int)q.t_done) continue;
        const bool work_hour = q.at_work[ts] != 0u, bus_hour = q.on_bus[ts] != 0u;
        uint32_t who = ESIM_NO_INFECTOR, k = 0u;
        if (s == ESIM_SETTING_WORKPLACE) {
            const uint32_t b = d.work[c];
            if (b < d.n_bld) {
                const uint32_t lo = d.wrk_off[b], hi = d.wrk_off[b + 1u];
                if (lo <= hi && hi <= d.n_wrk_idx) who = tree_member_list<0>(d, q, d.wrk_idx, lo, hi, c, ts, work_hour, bus_hour, lane, &k);
            }
        } else if (s == ESIM_SETTING_SCHOOL) {
            const uint32_t r = d.room[c];
            if (r < d.n_room) {
                const uint32_t lo = d.room_off[r], hi = d.room_off[r + 1u];
                if (lo <= hi && hi <= d.n_room_idx) who = tree_member_list<0>(d, q, d.room_idx, lo, hi, c, ts, work_hour, bus_hour, lane, &k);
            }
        } else if (s == ESIM_SETTING_TRANSPORT) {
            const uint32_t r = d.route_of[c];
            if (r < d.n_routes) {
                const uint32_t off = d.route_off[r], end = d.route_off[r + 1u];
                // (a route of at most bus_capacity riders is one bus and needs no keys)
                if (off <= end && end <= d.n_pt && end - off <= d.bus_capacity) who = tree_member_list<1>(d, q, d.route_riders, off, end, c, ts, work_hour, bus_hour, lane, &k);
            }
        }
        if (lane == 0u) {
            t.infector[c] = who;
            t.n_cand[c] = k;
            if (!k) atomicAdd(t.orphans, 1u);
        }
    }
}

// One wavefront (a workgroup of 64, with its LDS) per exposure queued at the back: a route longer than a bus.
__global__ __launch_bounds__(64) void k_tree_route(Dev d, Setting q, Tree t)
{
    __shared__ TreeShared sm;
    const uint32_t lane = threadIdx.x;
    const uint32_t n_q = *t.n_long < t.q_cap ? *t.n_long : t.q_cap;
    for (uint32_t e = blockIdx.x; e < n_q; e += gridDim.x) {
        const uint32_t c = t.queue[t.q_cap - 1u - e];
        if (c >= d.n) continue;                                            // (block-uniform, as everything below that leaves early)
        const uint32_t te = q.te_of[c], r = d.route_of[c];
        const int ts = (int)te - (int)TE_BIAS;
        if (te == SETTING_TE_NONE || ts < 1 || ts > (int)q.t_done || r >= d.n_routes) continue;
        const uint32_t off = d.route_off[r], end = d.route_off[r + 1u];
        uint32_t who = ESIM_NO_INFECTOR, k = 0u, bus = 0u;
        if (off <= end && end <= d.n_pt && end - off > d.bus_capacity) who = tree_route_long(d, q, sm, off, end - off, c, ts, lane, &k, &bus);
        if (lane == 0u) {
            t.infector[c] = who;
            t.n_cand[c] = k;
            if (t.bus) t.bus[c] = bus;
            if (!k) atomicAdd(t.orphans, 1u);
        }
        __syncthreads();
    }
}

// Generations: the log is in time order and an infector was exposed at least exposed_time + 1 steps before its infectee, so a
// launch over the log entries of steps [s_lo, s_hi], s_hi - s_lo <= exposed_time, reads only values that earlier launches (or
// k_tree_home, for the index cases) have finished.  A lane per entry.
__global__ __launch_bounds__(TPB) void k_tree_gen(Dev d, Setting q, Tree t, uint32_t s_lo, uint32_t s_hi, uint32_t log_len)
{
    const uint32_t lo = d.log_off[TE_BIAS + s_lo] < log_len ? d.log_off[TE_BIAS + s_lo] : log_len;
    uint32_t hi = s_hi >= q.t_done ? log_len : d.log_off[TE_BIAS + s_hi + 1u];
    if (hi > log_len) hi = log_len;
    for (uint64_t i = (uint64_t)lo + (uint64_t)blockIdx.x * TPB + threadIdx.x; i < (uint64_t)hi; i += (uint64_t)gridDim.x * TPB) {
        const uint32_t c = d.log[i];
        if (c >= d.n) continue;
        const uint32_t from = t.infector[c];
        if (from >= d.n) continue;
        const uint32_t g = t.gen[from];
        t.gen[c] = g == ESIM_NEVER ? ESIM_NEVER : g + 1u;
    }
}

// The exposure step of citizen c for the cohorts: 0 for an index case, -1 where the log does not hold it.
__device__ __forceinline__ int tree_step(const Setting &q, uint32_t c)
{
    const uint32_t te = q.te_of[c];
    if (te == SETTING_TE_NONE) return -1;
    const int ts = (int)te - (int)TE_BIAS;
    return ts < 1 ? 0 : ts;
}

// esim_offspring: counts[j] += 1 per citizen exposed in steps [first, last] whose infector is j.  A lane per log entry.
__global__ __launch_bounds__(TPB) void k_tree_offspring(Dev d, Setting q, Tree t, uint32_t first, uint32_t last, uint32_t log_len, uint32_t *counts)
{
    for (uint64_t i = (uint64_t)blockIdx.x * TPB + threadIdx.x; i < (uint64_t)log_len; i += (uint64_t)gridDim.x * TPB) {
        const uint32_t c = d.log[i];
        if (c >= d.n) continue;
        const int ts = tree_step(q, c);
        if (ts < (int)first || ts > (int)last) continue;
        const uint32_t from = t.infector[c];
        if (from < d.n) atomicAdd(&counts[from], 1u);
    }
}

struct TreeRows {
    uint32_t where, first, n_rows, stride, n_cols;
    const uint16_t *grp;            // [n] labels, ESIM_BY_GROUP only
    uint32_t *cases, *offspring;    // [n_rows][n_cols] each, zeroed by the caller; either may be nullptr
};

// The cell of citizen m in the cohort rows: the row of its exposure step, its own column.  ~0: outside.
__device__ __forceinline__ size_t tree_cell(const Dev &d, const Setting &q, const TreeRows &r, uint32_t m)
{
    const int ts = tree_step(q, m);
    if (ts < (int)r.first || ts > (int)q.t_done) return ~(size_t)0;
    const uint64_t row = (uint64_t)((uint32_t)ts - r.first) / r.stride;
    const uint32_t col = r.where == ESIM_BY_ALL ? 0u : r.where == ESIM_BY_GROUP ? (uint32_t)r.grp[m] : d.home[m] < d.n_bld ? d.bld_area[d.home[m]] : 0xFFFFFFFFu;
    return row < r.n_rows && col < r.n_cols ? (size_t)row * r.n_cols + col : ~(size_t)0;
}

// One add per lane at `cell` (live lanes only).  With one column a row the log's time order puts a wavefront's entries into a
// handful of cells: the lanes of a cell are counted by its first one, as k_setting_rows does (wave-uniform trips).
__device__ __forceinline__ void tree_rows_add(uint32_t *rows, size_t cell, bool live, bool pre_count, uint32_t lane)
{
    if (!pre_count) { if (live) atomicAdd(&rows[cell], 1u); return; }
    unsigned long long todo = __ballot(live);
    while (todo) {
        const uint32_t lead = (uint32_t)__ffsll((long long)todo) - 1u;
        const uint32_t lo = __shfl((uint32_t)cell, lead, 64), hi = __shfl((uint32_t)((uint64_t)cell >> 32), lead, 64);
        const unsigned long long same = __ballot(live && (uint32_t)cell == lo && (uint32_t)((uint64_t)cell >> 32) == hi);
        if (lane == lead) atomicAdd(&rows[cell], (uint32_t)__popcll(same));
        todo &= ~same;
    }
}

// esim_reproduction_series: a lane per log entry; the citizen counts in `cases` at its own cohort and in `offspring` at its
// infector's.
__global__ __launch_bounds__(TPB) void k_tree_rows(Dev d, Setting q, Tree t, TreeRows r, uint32_t log_len)
{
    const uint32_t lane = threadIdx.x & 63u;
    const size_t cells = (size_t)r.n_rows * r.n_cols;
    const bool pre = r.where == ESIM_BY_ALL;
    for (uint64_t i0 = (uint64_t)blockIdx.x * TPB; i0 < (uint64_t)log_len; i0 += (uint64_t)gridDim.x * TPB) {
        const uint64_t i = i0 + threadIdx.x;
        size_t mine = ~(size_t)0, parent = ~(size_t)0;
        if (i < (uint64_t)log_len) {
            const uint32_t c = d.log[i];
            if (c < d.n) {
                mine = tree_cell(d, q, r, c);
                const uint32_t from = t.infector[c];
                if (from < d.n) parent = tree_cell(d, q, r, from);
            }
        }
        if (r.cases) tree_rows_add(r.cases, mine, mine < cells, pre, lane);
        if (r.offspring) tree_rows_add(r.offspring, parent, parent < cells, pre, lane);
    }
}

// esim_mixing_matrix: counts[g_infector * n_groups + g_infectee] += 1 per transmission of steps [first, last] whose setting is
// in the mask.  A lane per log entry.
__global__ __launch_bounds__(TPB) void k_tree_matrix(Dev d, Setting q, Tree t, uint32_t mask, uint32_t first, uint32_t last, const uint16_t *grp, uint32_t n_groups,
                                                     uint32_t log_len, uint32_t *counts)
{
    for (uint64_t i = (uint64_t)blockIdx.x * TPB + threadIdx.x; i < (uint64_t)log_len; i += (uint64_t)gridDim.x * TPB) {
        const uint32_t c = d.log[i];
        if (c >= d.n) continue;
        const int ts = tree_step(q, c);
        const uint32_t s = q.setting[c];
        if (ts < (int)first || ts > (int)last || s >= ESIM_N_SETTINGS || !((mask >> s) & 1u)) continue;
        const uint32_t from = t.infector[c];
        if (from >= d.n) continue;
        const uint32_t a = grp[from], b = grp[c];
        if (a < n_groups && b < n_groups) atomicAdd(&counts[(size_t)a * n_groups + b], 1u);
    }
}
