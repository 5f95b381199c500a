// esim_kernels_places.h -- work place and school outbreaks: what esim_kernels_household.h gives the household, for the
// two other settings with a fixed member list -- the workers of a non-school building (wrk_off / wrk_idx) and the participants
// of a school room (room_off / room_idx).  k_place_members is a segmented reduction over a member list, a lane per entry;
// k_place_schools adds the rows of the rooms into their schools; k_place_tables bins the places, a table per workgroup in LDS;
// k_place_sar counts the pairs (case, member at risk) PER GATHERING: the members of a place are staged once in LDS and the
// cases x members run from there, where the per-case walks of k_hh_sar and k_contact_wide read a list again for every case.
// Nothing here writes simulation state.
#pragma once

#define PLACE_CELLS ((uint32_t)ESIM_PLACE_BINS * ESIM_PLACE_BINS)  // counters of one size table
// Members of a place that k_place_sar stages at a time: 12 B of LDS each (the susceptible end and the group of a member, the
// first infectious step and the group of a counted case), 24 KB at 2048, beside the pair tables of PLACE_LDS_BYTES.
#ifndef PLACE_TILE
#define PLACE_TILE 2048u
#endif
#ifndef PLACE_LDS_BYTES
#define PLACE_LDS_BYTES 32768u     // as HH_LDS_BYTES: the two pair tables stay in LDS up to 45 groups
#endif
#define PLACE_CHUNK 64u            // members a lane runs one case against before it takes its next (case, chunk) item
static_assert(PLACE_TILE % PLACE_CHUNK == 0u && PLACE_TILE >= TPB, "a tile is whole chunks, and no shorter than the places a workgroup scans at a time");

struct Place {
    uint32_t n_places;                        // n_bld (work places) or n_room (rooms)
    uint32_t *members, *cases, *intro, *first;  // [n_places] zeroed, zeroed, zeroed, filled with ESIM_NEVER by the caller
    uint32_t *final_size, *intro_size;        // [PLACE_CELLS] each, zeroed by the caller
};

// The size bin of the tables: exact below 16, then one bin per power of two, the last one open-ended.
__device__ __forceinline__ uint32_t place_bin(uint32_t x)
{
    if (x < 16u) return x;
    const uint32_t b = 12u + (31u - (uint32_t)__clz((int)x));
    return b < ESIM_PLACE_BINS - 1u ? b : ESIM_PLACE_BINS - 1u;
}

// The member list of the kind (ROOMS: the participants of the rooms, else the workers of the non-school buildings).
template <bool ROOMS> __device__ __forceinline__ const uint32_t *place_off(const Dev &d) { return ROOMS ? d.room_off : d.wrk_off; }
template <bool ROOMS> __device__ __forceinline__ const uint32_t *place_idx(const Dev &d) { return ROOMS ? d.room_idx : d.wrk_idx; }
template <bool ROOMS> __device__ __forceinline__ uint32_t place_idx_len(const Dev &d) { return ROOMS ? d.n_room_idx : d.n_wrk_idx; }
// The place citizen m is a member of, from the citizen: 0xFFFFFFFF where it is a member of no place of the kind.
template <bool ROOMS> __device__ __forceinline__ uint32_t place_of(const Dev &d, uint32_t m)
{
    const uint32_t w = d.cit[m];
    if (!(w & FL_HAS_WORK) || ((w & FL_WORK_SCHOOL) != 0u) != ROOMS) return 0xFFFFFFFFu;
    return ROOMS ? d.room[m] : d.work[m];
}

// Per place: its members, its cases, its introductions and the smallest cohort step among its cases.  A lane per entry r of the
// member list; the place comes from the citizen and is checked against the list it was found in (p < n_places, off[p] <= r <
// off[p + 1] <= the list's length).  Neighbouring lanes share a place: k_hh_residents' scheme, three atomics per run per
// wavefront; the number of members is the list's own length and is stored by the lane that holds the place's first entry.
template <bool ROOMS>
__global__ __launch_bounds__(TPB) void k_place_members(Dev d, Setting q, Place h)
{
    const uint32_t lane = threadIdx.x & 63u, n_list = place_idx_len<ROOMS>(d);
    const uint32_t *off = place_off<ROOMS>(d), *idx = place_idx<ROOMS>(d);
    const uint32_t own = ROOMS ? ESIM_SETTING_SCHOOL : ESIM_SETTING_WORKPLACE;
    for (uint64_t r0 = (uint64_t)blockIdx.x * TPB; r0 < (uint64_t)n_list; r0 += (uint64_t)gridDim.x * TPB) {
        const uint64_t r = r0 + threadIdx.x;
        uint32_t p = 0xFFFFFFFFu, step = ESIM_NEVER, size = 0u;
        bool is_case = false, is_intro = false, is_first = false;
        if (r < (uint64_t)n_list) {
            const uint32_t m = idx[r];
            const uint32_t pm = m < d.n ? place_of<ROOMS>(d, m) : 0xFFFFFFFFu;
            if (pm < h.n_places) {
                const uint32_t lo = off[pm], hi = off[pm + 1u];
                if ((uint64_t)lo <= r && r < (uint64_t)hi && hi <= n_list) {
                    p = pm;
                    is_first = r == (uint64_t)lo;
                    size = hi - lo;
                    const int ts = tree_step(q, m);
                    if (ts >= 0) {
                        is_case = true;
                        is_intro = ts == 0 || q.setting[m] != own;
                        step = (uint32_t)ts;
                    }
                }
            }
        }
        const uint32_t prev = __shfl_up(p, 1, 64);
        const bool head = p != 0xFFFFFFFFu && (lane == 0u || prev != p);
        const unsigned long long heads = __ballot(head);
        const unsigned long long above = lane == 63u ? 0ull : heads & (~0ull << (lane + 1u));
        const uint32_t next = above ? (uint32_t)__ffsll((long long)above) - 1u : 64u;            // the first lane of the next run
        const unsigned long long run = (next == 64u ? ~0ull : (1ull << next) - 1ull) & (~0ull << lane);
        const uint32_t n_cases = (uint32_t)__popcll(__ballot(is_case) & run), n_intro = (uint32_t)__popcll(__ballot(is_intro) & run);
#pragma unroll
        for (uint32_t o = 1u; o < 64u; o <<= 1) {                                                 // the smallest step from this lane to the end of its run
            const uint32_t v = __shfl_down(step, o, 64);
            if (lane + o < next && v < step) step = v;
        }
        if (is_first) h.members[p] = size;
        if (head) {
            if (n_cases) atomicAdd(&h.cases[p], n_cases);
            if (n_intro) atomicAdd(&h.intro[p], n_intro);
            if (step != ESIM_NEVER) atomicMin(&h.first[p], step);
        }
    }
}

// The rows of the schools: those of their rooms added into room_bld[r].  A lane per room.
__global__ __launch_bounds__(TPB) void k_place_schools(Dev d, Place rooms, Place schools)
{
    for (uint64_t r = (uint64_t)blockIdx.x * TPB + threadIdx.x; r < (uint64_t)d.n_room; r += (uint64_t)gridDim.x * TPB) {
        const uint32_t b = d.room_bld[r], size = rooms.members[r];
        if (b >= schools.n_places || !size) continue;
        atomicAdd(&schools.members[b], size);
        const uint32_t n_cases = rooms.cases[r], n_intro = rooms.intro[r], step = rooms.first[r];
        if (n_cases) atomicAdd(&schools.cases[b], n_cases);
        if (n_intro) atomicAdd(&schools.intro[b], n_intro);
        if (step != ESIM_NEVER) atomicMin(&schools.first[b], step);
    }
}

// The two tables of ESIM_PLACE_BINS x ESIM_PLACE_BINS bins over the places, a lane per place: k_hh_tables' scheme, the two
// tables of 4 KB each in LDS per workgroup, handed over once.
__global__ __launch_bounds__(TPB) void k_place_tables(Place h)
{
    __shared__ uint32_t tab[2u * PLACE_CELLS];
    for (uint32_t k = threadIdx.x; k < 2u * PLACE_CELLS; k += TPB) tab[k] = 0u;
    __syncthreads();
    for (uint64_t p = (uint64_t)blockIdx.x * TPB + threadIdx.x; p < (uint64_t)h.n_places; p += (uint64_t)gridDim.x * TPB) {
        const uint32_t size = h.members[p];
        if (!size) continue;                                              // (without a member it is no place)
        const uint32_t row = place_bin(size) * ESIM_PLACE_BINS;
        atomicAdd(&tab[row + place_bin(h.cases[p])], 1u);
        atomicAdd(&tab[PLACE_CELLS + row + place_bin(h.intro[p])], 1u);
    }
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < 2u * PLACE_CELLS; k += TPB) {
        const uint32_t v = tab[k];
        if (v) atomicAdd(k < PLACE_CELLS ? &h.final_size[k] : &h.intro_size[k - PLACE_CELLS], v);
    }
}

struct PlaceSar {
    uint32_t first, last;                    // cohort steps of the cases counted
    uint32_t n_cols;                         // 1, or the number of groups
    const uint16_t *grp;                     // [n] labels, or nullptr for one cell
    unsigned long long *at_risk, *secondary; // [n_cols * n_cols] each, zeroed by the caller
};

enum { PLACE_ONE_CELL = 0, PLACE_LDS = 1, PLACE_GLOBAL = 2 };

// The first infectious step of member m where it is a case the window counts (cohort step in [first, last], infectious by the
// last step run), else 0: no case has f = 0.
__device__ __forceinline__ uint32_t place_counted_f(const Dev &d, const Setting &q, const PlaceSar &s, uint32_t m)
{
    const int ts = tree_step(q, m);
    if (ts < (int)s.first || ts > (int)s.last) return 0u;
    const uint32_t f = ts == 0 ? 1u : (uint32_t)ts + d.exposed_time + 1u;
    return f <= q.t_done ? f : 0u;
}

// One more pair in cell (row / n_cols, gm) of the table `which` (0: at risk, 1: secondary).
template <int MODE>
__device__ __forceinline__ void place_add(const PlaceSar &s, unsigned long long *lds, uint32_t which, uint32_t cell)
{
    if (MODE == PLACE_LDS) atomicAdd(&lds[which * s.n_cols * s.n_cols + cell], 1ull);
    else atomicAdd(which ? &s.secondary[cell] : &s.at_risk[cell], 1ull);
}

// Whether member m is a secondary case its place counts: infected in the place's own setting by a member j of the same place
// that the window counts.  m is at risk from j by construction (it was Susceptible when j, Infected, exposed it); the check
// stays, so that secondary <= at_risk holds whatever the tree says.  *row: j's row of the tables.
template <bool ROOMS>
__device__ __forceinline__ bool place_secondary(const Dev &d, const Setting &q, const Tree &t, const PlaceSar &s, uint32_t p, uint32_t m, uint32_t end, uint32_t *row)
{
    if (q.setting[m] != (ROOMS ? ESIM_SETTING_SCHOOL : ESIM_SETTING_WORKPLACE)) return false;
    const uint32_t j = t.infector[m];
    if (j >= d.n || j == m || place_of<ROOMS>(d, j) != p) return false;
    const uint32_t f = place_counted_f(d, q, s, j);
    if (!f || f > end) return false;
    if (s.grp) {
        const uint32_t gj = s.grp[j];
        if (gj >= s.n_cols) return false;
        *row = gj * s.n_cols;
    }
    return true;
}

#ifndef PLACE_SAR_PER_CASE
struct PlaceShared {
    alignas(16) uint32_t m_end[PLACE_TILE];  // the staged members: susceptible end (0 behind the last one: at risk from nobody)
    uint32_t c_f[PLACE_TILE];                // the counted cases among a tile of members, compacted: first infectious step
    uint16_t m_grp[PLACE_TILE], c_grp[PLACE_TILE];
    uint32_t longer[TPB];                    // the places of the workgroup's stretch that a wavefront does not hold
    uint32_t n_longer, n_cases;
};

// A tile of a place's members staged by the workgroup: entries [lo, lo + cnt) of the list.  MEMBERS: their susceptible ends and
// groups go to m_end / m_grp (padded with 0 to whole chunks) and, with `sec`, the secondary cases among them are counted; CASES:
// the counted cases among them are appended to c_f / c_grp (sm.n_cases zeroed by the caller, behind a barrier).  A member whose
// label lies outside the groups is left out on either side, as k_hh_sar leaves it out.
template <int MODE, bool ROOMS, bool MEMBERS, bool CASES>
__device__ __forceinline__ void place_stage(const Dev &d, const Setting &q, const Tree &t, const PlaceSar &s, PlaceShared &sm, unsigned long long *lds,
                                            uint32_t p, uint32_t lo, uint32_t cnt, bool sec, unsigned long long *n_sec)
{
    const uint32_t *idx = place_idx<ROOMS>(d);
    const uint32_t padded = (cnt + PLACE_CHUNK - 1u) / PLACE_CHUNK * PLACE_CHUNK;
    for (uint32_t i = threadIdx.x; i < padded; i += TPB) {
        const uint32_t m = i < cnt ? idx[lo + i] : 0xFFFFFFFFu;
        uint32_t end = 0u, g = 0u, f = 0u;
        if (m < d.n) {
            g = MODE == PLACE_ONE_CELL ? 0u : (uint32_t)s.grp[m];
            if (g < s.n_cols) {
                end = hh_susceptible_end(d, q, m);
                if (CASES) f = place_counted_f(d, q, s, m);
            }
        }
        if (MEMBERS) {
            sm.m_end[i] = end;
            if (MODE != PLACE_ONE_CELL) sm.m_grp[i] = (uint16_t)g;
            uint32_t row = 0u;
            if (sec && m < d.n && g < s.n_cols && place_secondary<ROOMS>(d, q, t, s, p, m, end, &row)) {
                if (MODE == PLACE_ONE_CELL) ++*n_sec;
                else place_add<MODE>(s, lds, 1u, row + g);
            }
        }
        if (CASES && f) {
            const uint32_t at = atomicAdd(&sm.n_cases, 1u);
            sm.c_f[at] = f;
            if (MODE != PLACE_ONE_CELL) sm.c_grp[at] = (uint16_t)g;
        }
    }
}

// The staged cases against the staged members (`cnt` of them, padded to whole chunks): an item is a case and a chunk of
// PLACE_CHUNK members, neighbouring lanes take neighbouring cases of one chunk, so that the lanes of a wavefront read the same
// member at the same time (an LDS broadcast) and a place with few cases still fills the workgroup.
template <int MODE>
__device__ __forceinline__ void place_count(const PlaceSar &s, const PlaceShared &sm, unsigned long long *lds, uint32_t cnt, unsigned long long *n_at)
{
    const uint32_t n_cases = sm.n_cases, n_chunks = (cnt + PLACE_CHUNK - 1u) / PLACE_CHUNK, items = n_cases * n_chunks;
    for (uint32_t it = threadIdx.x; it < items; it += TPB) {
        const uint32_t c = it % n_cases, base = it / n_cases * PLACE_CHUNK, f = sm.c_f[c];
        if (MODE == PLACE_ONE_CELL) {
            const uint4 *ends = (const uint4 *)(sm.m_end + base);
            uint32_t mine = 0u;
#pragma unroll
            for (uint32_t k = 0u; k < PLACE_CHUNK / 4u; ++k) {
                const uint4 e = ends[k];
                mine += (f <= e.x) + (f <= e.y) + (f <= e.z) + (f <= e.w);
            }
            *n_at += mine;
        } else {
            const uint32_t row = (uint32_t)sm.c_grp[c] * s.n_cols;
            for (uint32_t k = 0u; k < PLACE_CHUNK; ++k)
                if (f <= sm.m_end[base + k]) place_add<MODE>(s, lds, 0u, row + sm.m_grp[base + k]);
        }
    }
}

// The pairs (case j, member m of j's place at risk from j), per gathering.  A workgroup takes TPB neighbouring places at a time
// and skips those without a case (pass one's counts) or without a second member.  A place of up to 64 members is held by one
// wavefront in registers, a lane per member, several such places per workgroup at once: every counted case is broadcast with
// a shuffle and every lane compares its own member.  A longer place is staged by the whole workgroup in LDS, PLACE_TILE
// members at a time, and its cases run against its members from there, tile against tile where it is longer than a tile: its
// list is read once, or once per tile of cases, and not once per case.  No pair (j, j) is counted: a case stops being
// Susceptible at its own exposure, before its first infectious step.  Counting as in k_hh_sar:
//   PLACE_ONE_CELL  a lane sums its pairs in registers, a wavefront adds its 64 sums up and issues one atomic pair at the end;
//   PLACE_LDS       cell [group of j][group of m] of a table of the workgroup's own in LDS (2 * n_cols^2 counters of dynamic
//                   LDS), handed to the global tables once, at the end, non-zero counters only;
//   PLACE_GLOBAL    the same cell of the global tables directly, where the table would not fit PLACE_LDS_BYTES.
template <int MODE, bool ROOMS>
__global__ __launch_bounds__(TPB) void k_place_sar(Dev d, Setting q, Tree t, Place h, PlaceSar s)
{
    extern __shared__ unsigned long long place_pairs[];
    __shared__ PlaceShared sm;
    const uint32_t cells = s.n_cols * s.n_cols, lane = threadIdx.x & 63u, n_list = place_idx_len<ROOMS>(d);
    const uint32_t *off = place_off<ROOMS>(d), *idx = place_idx<ROOMS>(d);
    if (MODE == PLACE_LDS) for (uint32_t k = threadIdx.x; k < 2u * cells; k += TPB) place_pairs[k] = 0ull;
    unsigned long long n_at = 0ull, n_sec = 0ull;
    for (uint64_t p0 = (uint64_t)blockIdx.x * TPB; p0 < (uint64_t)h.n_places; p0 += (uint64_t)gridDim.x * TPB) {
        if (threadIdx.x == 0u) sm.n_longer = 0u;
        __syncthreads();
        // this lane's place: its stretch of the list, 0 members where there is nothing to count
        const uint64_t mine = p0 + threadIdx.x;
        uint32_t lo = 0u, size = 0u;
        if (mine < (uint64_t)h.n_places && h.cases[mine] != 0u) {
            const uint32_t a = off[mine], b = off[mine + 1u];
            if (a < b && b <= n_list && b - a >= 2u) { lo = a; size = b - a; }
        }
        if (size > 64u) sm.longer[atomicAdd(&sm.n_longer, 1u)] = (uint32_t)(mine - p0);
        // the short places of this wavefront's 64, one after the other
        unsigned long long todo = __ballot(size >= 2u && size <= 64u);
        while (todo) {                                                    // (wave-uniform)
            const int src = __ffsll((long long)todo) - 1;
            todo &= todo - 1ull;
            const uint32_t p = (uint32_t)(p0 + (threadIdx.x - lane) + (uint32_t)src), p_lo = __shfl(lo, src, 64), p_size = __shfl(size, src, 64);
            const uint32_t m = lane < p_size ? idx[p_lo + lane] : 0xFFFFFFFFu;
            uint32_t end = 0u, g = 0u, f = 0u;
            if (m < d.n) {
                g = MODE == PLACE_ONE_CELL ? 0u : (uint32_t)s.grp[m];
                if (g < s.n_cols) {
                    end = hh_susceptible_end(d, q, m);
                    f = place_counted_f(d, q, s, m);
                    uint32_t row = 0u;
                    if (place_secondary<ROOMS>(d, q, t, s, p, m, end, &row)) {
                        if (MODE == PLACE_ONE_CELL) ++n_sec;
                        else place_add<MODE>(s, place_pairs, 1u, row + g);
                    }
                }
            }
            unsigned long long cases = __ballot(f != 0u);
            while (cases) {
                const int cj = __ffsll((long long)cases) - 1;
                cases &= cases - 1ull;
                const uint32_t fj = __shfl(f, cj, 64), gj = __shfl(g, cj, 64);
                if (fj > end) continue;                                   // (end is 0 on a lane without a member)
                if (MODE == PLACE_ONE_CELL) ++n_at;
                else place_add<MODE>(s, place_pairs, 0u, gj * s.n_cols + g);
            }
        }
        __syncthreads();
        // the longer places, each by the whole workgroup
        const uint32_t n_longer = sm.n_longer;
        for (uint32_t k = 0u; k < n_longer; ++k) {
            const uint32_t p = (uint32_t)p0 + sm.longer[k], p_lo = off[p], p_size = off[p + 1u] - p_lo;      // (checked above)
            const uint32_t n_tiles = (p_size + PLACE_TILE - 1u) / PLACE_TILE;
            for (uint32_t ct = 0u; ct < n_tiles; ++ct) {
                const uint32_t c_lo = ct * PLACE_TILE, c_cnt = p_size - c_lo < PLACE_TILE ? p_size - c_lo : PLACE_TILE;
                __syncthreads();                                          // (the tiles of the place or tile before are done with)
                if (threadIdx.x == 0u) sm.n_cases = 0u;
                __syncthreads();
                if (n_tiles == 1u) place_stage<MODE, ROOMS, true, true>(d, q, t, s, sm, place_pairs, p, p_lo, p_size, true, &n_sec);
                else place_stage<MODE, ROOMS, false, true>(d, q, t, s, sm, place_pairs, p, p_lo + c_lo, c_cnt, false, &n_sec);
                __syncthreads();
                if (n_tiles == 1u) { place_count<MODE>(s, sm, place_pairs, p_size, &n_at); continue; }
                for (uint32_t mt = 0u; mt < n_tiles; ++mt) {
                    const uint32_t m_lo = mt * PLACE_TILE, m_cnt = p_size - m_lo < PLACE_TILE ? p_size - m_lo : PLACE_TILE;
                    // (the secondary cases are counted where the members are staged for the first tile of cases, once per place)
                    if (ct == 0u || sm.n_cases) place_stage<MODE, ROOMS, true, false>(d, q, t, s, sm, place_pairs, p, p_lo + m_lo, m_cnt, ct == 0u, &n_sec);
                    __syncthreads();
                    if (sm.n_cases) place_count<MODE>(s, sm, place_pairs, m_cnt, &n_at);
                    __syncthreads();
                }
            }
        }
        __syncthreads();
    }
    if (MODE == PLACE_ONE_CELL) {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            n_at += __shfl_xor(n_at, o, 64);
            n_sec += __shfl_xor(n_sec, o, 64);
        }
        if (lane == 0u) {
            if (n_at) atomicAdd(s.at_risk, n_at);
            if (n_sec) atomicAdd(s.secondary, n_sec);
        }
    }
    if (MODE == PLACE_LDS) {
        __syncthreads();
        for (uint32_t k = threadIdx.x; k < 2u * cells; k += TPB) {
            const unsigned long long v = place_pairs[k];
            if (v) atomicAdd(k < cells ? &s.at_risk[k] : &s.secondary[k - cells], v);
        }
    }
}
#else
// Diagnostics build (make places-per-case): the same output per CASE, the baseline the per-gathering form is measured against
// -- k_hh_sar's walk over the work-side list of every case, a wavefront per entry of the log reading the list from global memory.
template <int MODE, bool ROOMS>
__global__ __launch_bounds__(TPB) void k_place_sar(Dev d, Setting q, Tree t, Place h, PlaceSar s, uint32_t log_len)
{
    extern __shared__ unsigned long long place_pairs[];
    const uint32_t cells = s.n_cols * s.n_cols, lane = threadIdx.x & 63u, n_list = place_idx_len<ROOMS>(d);
    const uint32_t *off = place_off<ROOMS>(d), *idx = place_idx<ROOMS>(d);
    if (MODE == PLACE_LDS) {
        for (uint32_t k = threadIdx.x; k < 2u * cells; k += TPB) place_pairs[k] = 0ull;
        __syncthreads();
    }
    const uint32_t wave = blockIdx.x * (TPB / 64u) + (threadIdx.x >> 6), n_waves = gridDim.x * (TPB / 64u);
    unsigned long long n_at = 0ull, n_sec = 0ull;
    for (uint32_t e = wave; e < log_len; e += n_waves) {
        const uint32_t j = d.log[e];
        if (j >= d.n) continue;                                           // (wave-uniform, as everything below)
        const uint32_t f = place_counted_f(d, q, s, j), p = place_of<ROOMS>(d, j);
        if (!f || p >= h.n_places) continue;
        const uint32_t lo = off[p], hi = off[p + 1u];
        if (lo > hi || hi > n_list) continue;
        uint32_t row = 0u;
        if (MODE != PLACE_ONE_CELL) {
            const uint32_t gj = s.grp[j];
            if (gj >= s.n_cols) continue;
            row = gj * s.n_cols;
        }
        for (uint32_t i = lo + lane; i < hi; i += 64u) {
            const uint32_t m = idx[i];
            if (m >= d.n || m == j || f > hh_susceptible_end(d, q, m)) continue;
            const bool sec = t.infector[m] == j && q.setting[m] == (ROOMS ? ESIM_SETTING_SCHOOL : ESIM_SETTING_WORKPLACE);
            if (MODE == PLACE_ONE_CELL) { ++n_at; n_sec += sec ? 1ull : 0ull; continue; }
            const uint32_t gm = s.grp[m];
            if (gm >= s.n_cols) continue;
            place_add<MODE>(s, place_pairs, 0u, row + gm);
            if (sec) place_add<MODE>(s, place_pairs, 1u, row + gm);
        }
    }
    if (MODE == PLACE_ONE_CELL) {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            n_at += __shfl_xor(n_at, o, 64);
            n_sec += __shfl_xor(n_sec, o, 64);
        }
        if (lane == 0u) {
            if (n_at) atomicAdd(s.at_risk, n_at);
            if (n_sec) atomicAdd(s.secondary, n_sec);
        }
    }
    if (MODE == PLACE_LDS) {
        __syncthreads();
        for (uint32_t k = threadIdx.x; k < 2u * cells; k += TPB) {
            const unsigned long long v = place_pairs[k];
            if (v) atomicAdd(k < cells ? &s.at_risk[k] : &s.secondary[k - cells], v);
        }
    }
}
#endif
