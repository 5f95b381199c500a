// esim_kernels_contacts.h -- contact-hours at risk: the denominator of the transmissions of esim_kernels_tree.h.  A
// contact-hour is a triple (j, m, ts): in step ts citizen j is a candidate of a gathering as the tree defines candidates, and
// citizen m, Susceptible after step ts - 1, takes that gathering's draw.  The pair form is the definition, not the algorithm:
// in a building, a room or a route that is one bus, presence depends only on the step's (work bit, bus bit) combination and on
// the two citizens' flags, so a pair costs two 4-bit sets and, for the combinations in both, a difference of prefix counts over
// the steps both are there for.  k_contact_home walks the household of every case, a lane per log entry; k_contact_wide gives
// a wavefront to the work-side list and the short route of every case; routes longer than a bus are replayed per (route, bus
// step) that has an Infected rider: k_contact_route_mark sets a bit per such item, k_contact_route ranks the riders of each
// once and multiplies, per bus, the Infected aboard with the Susceptible aboard.  k_contact_trans splits the mixing matrix by
// setting.  Nothing here writes simulation state.
#pragma once

// k_contact_home and k_contact_wide count in the modes of esim_kernels_pairtab.h: the four planes of `hours` are one table of
// 4 * n_cols^2 counters, in LDS while it fits PAIRTAB_LDS_BYTES (n_cols <= 32).
#define CONTACT_ROUTE_GROUPS 1024u    // k_contact_route counts the Susceptible of a bus by group in LDS up to this many groups
#define CONTACT_INF   0x80000000u     // on a rider's word: Infected in the step
#define CONTACT_TAKES 0x40000000u     // ... Susceptible and taking the bus draw
#define CONTACT_BUS   0x3FFFFFFFu     // ... its bus

struct Contact {
    uint32_t first, last;            // the window, last <= t_done
    uint32_t mask;                   // settings asked for
    uint32_t n_cols;                 // 1, or the number of groups
    const uint16_t *grp;             // [n] labels, or nullptr for one cell
    const uint32_t *pre;             // [4][stride] pre[c][s]: steps 1 .. s whose (work bit | bus bit << 1) is c
    uint32_t stride;                 // t_done + 1
    const uint32_t *bus_steps;       // the steps with the bus bit set inside the window, ascending
    unsigned long long *hours;       // [4][n_cols * n_cols] zeroed by the caller
    unsigned long long *trans;       // the same, or nullptr
    uint32_t *per_case;              // [n] zeroed by the caller, or nullptr
};

enum { CT_SET_WORK = 0xAu, CT_SET_BUS = 0xCu };        // the combinations with the work bit, with the bus bit

// The Infected steps of citizen j inside the window, [*f, *l] (empty: *f > *l): exposed_time + 1 steps behind its exposure
// step the infected_time + 1 Infected steps follow, from step 1 for an index case, up to the step at whose end it was vaccinated.
__device__ __forceinline__ void contact_infected_span(const Dev &d, const Setting &q, const Contact &k, uint32_t j, uint32_t w, uint32_t *f, uint32_t *l)
{
    *f = 1u; *l = 0u;
    const uint32_t te = q.te_of[j];
    if (te == SETTING_TE_NONE) return;
    const int inf = (int)te - (int)TE_BIAS + (int)d.exposed_time + 1, end = inf + (int)d.infected_time;
    if (end < 1) return;
    uint32_t lo = inf < 1 ? 1u : (uint32_t)inf, hi = (uint32_t)end;
    if (CW_TE(w) == TE_VACCINATED) {
        const uint32_t own = q.vax_of ? q.vax_of[j] : 0xFFFFFFFFu, v = q.t_all < own ? q.t_all : own;
        if (v < hi) hi = v;
    }
    *f = lo > k.first ? lo : k.first;
    *l = hi < k.last ? hi : k.last;
}

// The combinations in which citizen (word w) stands in its household as a candidate / takes the household draw, takes the
// work-side draw; a candidate at work needs the work bit and, for a rider, no bus bit.
__device__ __forceinline__ uint32_t contact_set_home_inf(uint32_t w) { return 0xFu & ~((w & FL_USES_PT) ? CT_SET_BUS : 0u) & ~((w & FL_HAS_WORK) ? CT_SET_WORK : 0u); }
__device__ __forceinline__ uint32_t contact_set_home_sus(uint32_t w) { return ((w & FL_HAS_WORK) && !(w & FL_SAME_AREA)) ? 0xFu & ~CT_SET_WORK : 0xFu; }
__device__ __forceinline__ uint32_t contact_set_work_inf(uint32_t w) { return !(w & FL_HAS_WORK) ? 0u : (w & FL_USES_PT) ? CT_SET_WORK & ~CT_SET_BUS : CT_SET_WORK; }
__device__ __forceinline__ uint32_t contact_set_work_sus(uint32_t w) { return !(w & FL_HAS_WORK) ? 0u : (w & FL_SAME_AREA) ? 0xFu : CT_SET_WORK; }

// The steps of [a, b] whose combination is in `set`.
__device__ __forceinline__ uint32_t contact_steps(const Contact &k, uint32_t set, uint32_t a, uint32_t b)
{
    if (a > b || !set) return 0u;
    if (set == 0xFu) return b - a + 1u;
    uint32_t n = 0u;
#pragma unroll
    for (uint32_t c = 0u; c < 4u; ++c)
        if ((set >> c) & 1u) n += k.pre[c * k.stride + b] - k.pre[c * k.stride + a - 1u];
    return n;
}

// The last step in which m takes the bus draw as a Susceptible: the step before its exposure where that was in a building
// (buildings are drawn before buses), its exposure step on a bus.
__device__ __forceinline__ uint32_t contact_bus_end(const Dev &d, const Setting &q, uint32_t m, uint32_t w)
{
    uint32_t end = hh_susceptible_end(d, q, m);
    const uint32_t te = q.te_of[m];
    if (te != SETTING_TE_NONE && te > TE_BIAS && !(w & CW_BUS_EXPOSED) && te - TE_BIAS - 1u < end) end = te - TE_BIAS - 1u;
    return end;
}

// cnt contact-hours of setting s between a case of row `row` (group * n_cols) and citizen m.
template <int MODE>
__device__ __forceinline__ void contact_add(const Contact &k, unsigned long long *lds, uint32_t s, uint32_t row, uint32_t m, uint32_t cnt)
{
    if (!cnt) return;
    const uint32_t gm = k.grp[m];
    if (gm >= k.n_cols) return;
    pairtab_add<MODE>(lds, k.hours, s * k.n_cols * k.n_cols + row + gm, cnt);
}

// Households: a lane per entry of the log, one walk over the household of case j.
template <int MODE>
__global__ __launch_bounds__(TPB) void k_contact_home(Dev d, Setting q, Contact k, uint32_t log_len)
{
    extern __shared__ unsigned long long ct_lds[];
    if (MODE == PAIRTAB_LDS) pairtab_clear(ct_lds, 4u * k.n_cols * k.n_cols);
    unsigned long long sum = 0ull;
    for (uint64_t i = (uint64_t)blockIdx.x * TPB + threadIdx.x; i < (uint64_t)log_len; i += (uint64_t)gridDim.x * TPB) {
        const uint32_t j = d.log[i];
        if (j >= d.n) continue;
        const uint32_t wj = d.cit[j];
        uint32_t f, l;
        contact_infected_span(d, q, k, j, wj, &f, &l);
        if (f > l) continue;
        const uint32_t b = d.home[j];
        if (b >= d.n_bld) continue;
        const uint32_t lo = d.res_off[b], hi = d.res_off[b + 1u];
        if (lo > hi || hi > d.n) continue;
        uint32_t row = 0u;
        if (MODE != PAIRTAB_ONE_CELL) {
            const uint32_t gj = k.grp[j];
            if (gj >= k.n_cols) continue;
            row = gj * k.n_cols;
        }
        const uint32_t set_j = contact_set_home_inf(wj);
        uint32_t mine = 0u;
        for (uint32_t r = lo; r < hi; ++r) {
            const uint32_t m = d.res_idx ? d.res_idx[r] : r;
            if (m >= d.n || m == j) continue;
            const uint32_t end = hh_susceptible_end(d, q, m);
            const uint32_t cnt = contact_steps(k, set_j & contact_set_home_sus(d.cit[m]), f, end < l ? end : l);
            if (MODE == PAIRTAB_ONE_CELL) { mine += cnt; continue; }
            if (cnt && k.grp[m] < k.n_cols) mine += cnt;
            contact_add<MODE>(k, ct_lds, ESIM_SETTING_HOUSEHOLD, row, m, cnt);
        }
        sum += mine;
        if (k.per_case && mine) atomicAdd(&k.per_case[j], mine);
    }
    if (MODE == PAIRTAB_ONE_CELL) pairtab_wave_add(&k.hours[ESIM_SETTING_HOUSEHOLD], sum);
    if (MODE == PAIRTAB_LDS) pairtab_flush(ct_lds, k.hours, 4u * k.n_cols * k.n_cols);
}

// One member list [lo, hi) of case j by one wavefront, ids read coalesced.  KIND 0: a work place or a room, 1: a route that is
// one bus.  Returns the lane's share of the contact-hours (counted into the cells already unless MODE is PAIRTAB_ONE_CELL).
template <int MODE, int KIND>
__device__ __forceinline__ uint32_t contact_member_list(const Dev &d, const Setting &q, const Contact &k, unsigned long long *lds, const uint32_t *idx, uint32_t lo, uint32_t hi,
                                                        uint32_t j, uint32_t set_j, uint32_t f, uint32_t l, uint32_t s, uint32_t row, uint32_t lane)
{
    uint32_t mine = 0u;
    for (uint32_t i = lo + lane; i < hi; i += 64u) {
        const uint32_t m = idx[i];
        if (m >= d.n || m == j) continue;
        const uint32_t wm = d.cit[m];
        const uint32_t end = KIND == 0 ? hh_susceptible_end(d, q, m) : contact_bus_end(d, q, m, wm);
        const uint32_t cnt = contact_steps(k, set_j & (KIND == 0 ? contact_set_work_sus(wm) : (uint32_t)CT_SET_BUS), f, end < l ? end : l);
        if (MODE == PAIRTAB_ONE_CELL) { mine += cnt; continue; }
        if (cnt && k.grp[m] < k.n_cols) mine += cnt;
        contact_add<MODE>(k, lds, s, row, m, cnt);
    }
    return mine;
}

// Work places, school rooms and routes of one bus: a wavefront per entry of the log.
template <int MODE>
__global__ __launch_bounds__(TPB) void k_contact_wide(Dev d, Setting q, Contact k, uint32_t log_len)
{
    extern __shared__ unsigned long long ct_lds[];
    if (MODE == PAIRTAB_LDS) pairtab_clear(ct_lds, 4u * k.n_cols * k.n_cols);
    const uint32_t lane = threadIdx.x & 63u, wave = blockIdx.x * (TPB / 64u) + (threadIdx.x >> 6), n_waves = gridDim.x * (TPB / 64u);
    unsigned long long sum[3] = { 0ull, 0ull, 0ull };                       // work place, school, transport
    for (uint32_t e = wave; e < log_len; e += n_waves) {
        const uint32_t j = d.log[e];
        if (j >= d.n) continue;                                            // (wave-uniform, as everything below)
        const uint32_t wj = d.cit[j];
        uint32_t f, l;
        contact_infected_span(d, q, k, j, wj, &f, &l);
        if (f > l) continue;
        uint32_t row = 0u;
        if (MODE != PAIRTAB_ONE_CELL) {
            const uint32_t gj = k.grp[j];
            if (gj >= k.n_cols) continue;
            row = gj * k.n_cols;
        }
        uint32_t mine = 0u;
        if (wj & FL_HAS_WORK) {
            const uint32_t set_j = contact_set_work_inf(wj);
            if ((wj & FL_WORK_SCHOOL) && ((k.mask >> ESIM_SETTING_SCHOOL) & 1u)) {
                const uint32_t r = d.room[j];
                if (r < d.n_room) {
                    const uint32_t lo = d.room_off[r], hi = d.room_off[r + 1u];
                    if (lo <= hi && hi <= d.n_room_idx) {
                        const uint32_t got = contact_member_list<MODE, 0>(d, q, k, ct_lds, d.room_idx, lo, hi, j, set_j, f, l, ESIM_SETTING_SCHOOL, row, lane);
                        sum[1] += got; mine += got;
                    }
                }
            } else if (!(wj & FL_WORK_SCHOOL) && ((k.mask >> ESIM_SETTING_WORKPLACE) & 1u)) {
                const uint32_t b = d.work[j];
                if (b < d.n_bld) {
                    const uint32_t lo = d.wrk_off[b], hi = d.wrk_off[b + 1u];
                    if (lo <= hi && hi <= d.n_wrk_idx) {
                        const uint32_t got = contact_member_list<MODE, 0>(d, q, k, ct_lds, d.wrk_idx, lo, hi, j, set_j, f, l, ESIM_SETTING_WORKPLACE, row, lane);
                        sum[0] += got; mine += got;
                    }
                }
            }
        }
        if ((wj & FL_USES_PT) && ((k.mask >> ESIM_SETTING_TRANSPORT) & 1u)) {
            const uint32_t r = d.route_of[j];
            if (r < d.n_routes) {
                const uint32_t off = d.route_off[r], end = d.route_off[r + 1u];
                if (off <= end && end <= d.n_pt && end - off <= d.bus_capacity) {
                    const uint32_t got = contact_member_list<MODE, 1>(d, q, k, ct_lds, d.route_riders, off, end, j, CT_SET_BUS, f, l, ESIM_SETTING_TRANSPORT, row, lane);
                    sum[2] += got; mine += got;
                }
            }
        }
        if (k.per_case) {
            const uint32_t all = (uint32_t)pairtab_wave_sum((unsigned long long)mine);
            if (lane == 0u && all) atomicAdd(&k.per_case[j], all);
        }
    }
    if (MODE == PAIRTAB_ONE_CELL) {
        const uint32_t plane[3] = { ESIM_SETTING_WORKPLACE, ESIM_SETTING_SCHOOL, ESIM_SETTING_TRANSPORT };
#pragma unroll
        for (int p = 0; p < 3; ++p) pairtab_wave_add(&k.hours[plane[p]], sum[p]);
    }
    if (MODE == PAIRTAB_LDS) pairtab_flush(ct_lds, k.hours, 4u * k.n_cols * k.n_cols);
}

// Routes longer than a bus: a bit per (bus step number i in [i_lo, i_hi) of the window's bus steps, route) in which a rider of
// the route is Infected.  A lane per entry of the log; bits[(i - i_lo) * n_routes + route].
__global__ __launch_bounds__(TPB) void k_contact_route_mark(Dev d, Setting q, Contact k, uint32_t log_len, uint32_t i_lo, uint32_t i_hi, uint32_t *bits)
{
    for (uint64_t e = (uint64_t)blockIdx.x * TPB + threadIdx.x; e < (uint64_t)log_len; e += (uint64_t)gridDim.x * TPB) {
        const uint32_t j = d.log[e];
        if (j >= d.n) continue;
        const uint32_t wj = d.cit[j];
        if (!(wj & FL_USES_PT)) continue;
        const uint32_t r = d.route_of[j];
        if (r >= d.n_routes || d.route_off[r + 1u] - d.route_off[r] <= d.bus_capacity) continue;
        uint32_t f, l;
        contact_infected_span(d, q, k, j, wj, &f, &l);
        if (f > l) continue;
        // the bus steps of the window before f, and up to l: positions in bus_steps
        const uint32_t base = k.pre[2u * k.stride + k.first - 1u] + k.pre[3u * k.stride + k.first - 1u];
        uint32_t a = k.pre[2u * k.stride + f - 1u] + k.pre[3u * k.stride + f - 1u] - base;
        uint32_t b = k.pre[2u * k.stride + l] + k.pre[3u * k.stride + l] - base;
        if (a < i_lo) a = i_lo;
        if (b > i_hi) b = i_hi;
        for (uint32_t i = a; i < b; ++i) {
            const uint64_t bit = (uint64_t)(i - i_lo) * d.n_routes + r;
            atomicOr(&bits[bit >> 5], 1u << (bit & 31u));
        }
    }
}

struct ContactShared {
    uint32_t key[CHUNK_ROUTE_MAX];          // the riders' keys, routes up to CHUNK_ROUTE_MAX riders (longer ones: ranked from global memory)
    uint32_t cnt[CONTACT_ROUTE_GROUPS];     // the Susceptible of one bus by group
};

// One (route, step) item by one wavefront: every rider's key drawn and every rider that matters ranked once, its bus and what
// it is kept in the workgroup's stretch of global memory (g_key, g_word: max_route words each); then per Infected rider the
// Susceptible of its bus that take the draw are counted into the cells.  Returns the item's contact-hours (wave-uniform): with one
// cell the caller adds them up over its items, so that the items do not queue on one address.
__device__ __forceinline__ unsigned long long contact_route_item(const Dev &d, const Setting &q, const Contact &k, ContactShared &sm, uint32_t *g_key, uint32_t *g_word,
                                                   uint32_t r, uint32_t ts, uint32_t lane)
{
    const uint32_t off = d.route_off[r], end = d.route_off[r + 1u];
    if (off > end || end > d.n_pt || end - off <= d.bus_capacity) return 0ull;
    const uint32_t sz = end - off;
    const bool keep = sz <= CHUNK_ROUTE_MAX;
    const uint64_t seed = tree_seed(d, q, (int)ts);
    for (uint32_t i = lane; i < sz; i += 64u) {
        const uint32_t m = d.route_riders[off + i];
        const uint32_t key = m < d.n ? tree_bus_key(d, seed, m, (int)ts) : 0xFFFFFFFFu;
        g_key[i] = key;
        if (keep) sm.key[i] = key;
    }
    __syncthreads();
    for (uint32_t i = lane; i < sz; i += 64u) {
        const uint32_t m = d.route_riders[off + i];
        uint32_t word = 0u;
        if (m < d.n) {
            if (infected_rider(d, q, m, (int)ts)) word = CONTACT_INF;
            else if (contact_bus_end(d, q, m, d.cit[m]) >= ts) word = CONTACT_TAKES;
        }
        if (word) word |= rank_block_exact(keep ? sm.key : g_key, g_key[i], i, sz) / d.bus_capacity;
        g_word[i] = word;
    }
    __syncthreads();
    unsigned long long total = 0ull;
    for (uint32_t b0 = 0u; b0 < sz; b0 += 64u) {
        const uint32_t mine = b0 + lane < sz ? g_word[b0 + lane] : 0u;
        unsigned long long todo = __ballot((mine & CONTACT_INF) != 0u);
        while (todo) {                                                // (wave-uniform: every lane sees the same ballots)
            const int src = __ffsll((long long)todo) - 1;
            todo &= todo - 1ull;
            const uint32_t bus = __shfl(mine, src, 64) & CONTACT_BUS, j = d.route_riders[off + b0 + (uint32_t)src];
            const uint32_t gj = k.grp ? (uint32_t)k.grp[j] : 0u;
            if (gj >= k.n_cols) continue;
            const bool hist = k.grp && k.n_cols <= CONTACT_ROUTE_GROUPS;
            if (hist) {
                for (uint32_t g = lane; g < k.n_cols; g += 64u) sm.cnt[g] = 0u;
                __syncthreads();
            }
            uint32_t aboard = 0u;
            for (uint32_t i0 = 0u; i0 < sz; i0 += 64u) {
                const uint32_t w = i0 + lane < sz ? g_word[i0 + lane] : 0u;
                const bool on = (w & CONTACT_TAKES) && (w & CONTACT_BUS) == bus;
                if (!k.grp) { aboard += (uint32_t)__popcll(__ballot(on)); continue; }
                const uint32_t gm = on ? (uint32_t)k.grp[d.route_riders[off + i0 + lane]] : 0xFFFFFFFFu;
                const bool counted = on && gm < k.n_cols;
                aboard += (uint32_t)__popcll(__ballot(counted));
                if (!counted) continue;
                if (hist) atomicAdd(&sm.cnt[gm], 1u);
                else atomicAdd(&k.hours[(size_t)ESIM_SETTING_TRANSPORT * k.n_cols * k.n_cols + (size_t)gj * k.n_cols + gm], 1ull);
            }
            if (hist) {
                __syncthreads();
                for (uint32_t g = lane; g < k.n_cols; g += 64u) {
                    const uint32_t v = sm.cnt[g];
                    if (v) atomicAdd(&k.hours[(size_t)ESIM_SETTING_TRANSPORT * k.n_cols * k.n_cols + (size_t)gj * k.n_cols + g], (unsigned long long)v);
                }
                __syncthreads();
            }
            total += aboard;
            if (k.per_case && lane == 0u && aboard) atomicAdd(&k.per_case[j], aboard);
        }
    }
    __syncthreads();
    return total;
}

// One wavefront (a workgroup of 64, with its LDS and its stretch of `tmp`: 2 * max_route words) per set bit of `bits`: the
// workgroups stride over the words 64 at a time.
__global__ __launch_bounds__(64) void k_contact_route(Dev d, Setting q, Contact k, uint32_t i_lo, const uint32_t *bits, uint32_t n_words, uint32_t *tmp)
{
    __shared__ ContactShared sm;
    const uint32_t lane = threadIdx.x;
    uint32_t *g_key = tmp + (size_t)blockIdx.x * 2u * d.max_route, *g_word = g_key + d.max_route;
    unsigned long long sum = 0ull;
    for (uint32_t w0 = blockIdx.x * 64u; w0 < n_words; w0 += gridDim.x * 64u) {
        const uint32_t word = w0 + lane < n_words ? bits[w0 + lane] : 0u;
        unsigned long long todo = __ballot(word != 0u);
        while (todo) {                                                // (block-uniform)
            const int src = __ffsll((long long)todo) - 1;
            todo &= todo - 1ull;
            uint32_t left = __shfl(word, src, 64);
            while (left) {
                const uint32_t bit = (uint32_t)__ffs((int)left) - 1u;
                left &= left - 1u;
                const uint64_t at = ((uint64_t)(w0 + (uint32_t)src) << 5) + bit;
                const uint32_t i = i_lo + (uint32_t)(at / d.n_routes), r = (uint32_t)(at % d.n_routes);
                sum += contact_route_item(d, q, k, sm, g_key, g_word, r, k.bus_steps[i], lane);
            }
        }
    }
    if (!k.grp && lane == 0u && sum) atomicAdd(&k.hours[ESIM_SETTING_TRANSPORT], sum);
}

// transmissions[s][col(infector)][col(infectee)] += 1 per transmission of the window whose setting s is in the mask.  A lane per
// log entry, as k_tree_matrix.  With one cell a plane is one address: a lane counts its entries in four registers over its whole
// grid-stride loop and the wavefront adds them up, four atomics per wavefront instead of one per transmission.
__global__ __launch_bounds__(TPB) void k_contact_trans(Dev d, Setting q, Tree t, Contact k, uint32_t log_len)
{
    uint32_t n0 = 0u, n1 = 0u, n2 = 0u, n3 = 0u;
    for (uint64_t i = (uint64_t)blockIdx.x * TPB + threadIdx.x; i < (uint64_t)log_len; i += (uint64_t)gridDim.x * TPB) {
        const uint32_t c = d.log[i];
        if (c >= d.n) continue;
        const int ts = tree_step(q, c);
        const uint32_t s = q.setting[c];
        if (ts < (int)k.first || ts > (int)k.last || s >= ESIM_N_SETTINGS || !((k.mask >> s) & 1u)) continue;
        const uint32_t from = t.infector[c];
        if (from >= d.n) continue;
        if (!k.grp) { n0 += s == 0u; n1 += s == 1u; n2 += s == 2u; n3 += s == 3u; continue; }
        const uint32_t a = k.grp[from], b = k.grp[c];
        if (a < k.n_cols && b < k.n_cols) atomicAdd(&k.trans[(size_t)s * k.n_cols * k.n_cols + (size_t)a * k.n_cols + b], 1ull);
    }
    if (k.grp) return;
    const unsigned long long v0 = pairtab_wave_sum(n0), v1 = pairtab_wave_sum(n1), v2 = pairtab_wave_sum(n2), v3 = pairtab_wave_sum(n3);
    if ((threadIdx.x & 63u) == 0u) {
        if (v0) atomicAdd(&k.trans[0], v0);
        if (v1) atomicAdd(&k.trans[1], v1);
        if (v2) atomicAdd(&k.trans[2], v2);
        if (v3) atomicAdd(&k.trans[3], v3);
    }
}
