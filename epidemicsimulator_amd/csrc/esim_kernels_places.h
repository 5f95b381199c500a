// esim_kernels_places.h -- work place and school outbreaks: what esim_kernels_household.h gives the household, for the
// two other settings with a fixed member list -- the workers of a non-school building (wrk_off / wrk_idx) and the participants
// of a school room (room_off / room_idx).  The per-place rows and the tables are k_list_members and k_list_tables of
// esim_kernels_household.h; k_place_schools adds the rows of the rooms into their schools;
// k_place_sar counts the pairs (case, member at risk) PER GATHERING: the members of a place are staged once in LDS and the
// cases x members run from there, where the per-case walks of k_hh_sar and k_contact_wide read a list again for every case.
// Nothing here writes simulation state.
#pragma once

// Members of a place that k_place_sar stages at a time: 12 B of LDS each (the susceptible end and the group of a member, the
// first infectious step and the group of a counted case), 24 KB at 2048, beside the pair tables of PAIRTAB_LDS_BYTES.
#ifndef PLACE_TILE
#define PLACE_TILE 2048u
#endif
#define PLACE_CHUNK 64u            // members a lane runs one case against before it takes its next (case, chunk) item
static_assert(PLACE_TILE % PLACE_CHUNK == 0u && PLACE_TILE >= TPB, "a tile is whole chunks, and no shorter than the places a workgroup scans at a time");

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

// The member list of k_place_sar's kind (ROOMS: the participants of the rooms, else the workers of the non-school buildings).
constexpr int place_list(bool rooms) { return rooms ? LIST_ROOM : LIST_WORK; }

// Whether member m is a secondary case its place counts: infected in the place's own setting by a member j of the same place
// that the window counts.  m is at risk from j by construction (it was Susceptible when j, Infected, exposed it); the check
// stays, so that secondary <= at_risk holds whatever the tree says.  *row: j's row of the tables.
template <bool ROOMS>
__device__ __forceinline__ bool place_secondary(const Dev &d, const Setting &q, const Tree &t, const SarWindow &s, uint32_t p, uint32_t m, uint32_t end, uint32_t *row)
{
    if (q.setting[m] != list_own<place_list(ROOMS)>()) return false;
    const uint32_t j = t.infector[m];
    if (j >= d.n || j == m || list_place<place_list(ROOMS)>(d, j) != p) return false;
    const uint32_t f = sar_counted_f(s, tree_step(q, j), d.exposed_time, q.t_done);
    if (!f || f > end) return false;
    if (s.grp) {
        const uint32_t gj = s.grp[j];
        if (gj >= s.n_cols) return false;
        *row = gj * s.n_cols;
    }
    return true;
}

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
__device__ __forceinline__ void place_stage(const Dev &d, const Setting &q, const Tree &t, const SarWindow &s, PlaceShared &sm, unsigned long long *lds,
                                            uint32_t p, uint32_t lo, uint32_t cnt, bool sec, unsigned long long *n_sec)
{
    const uint32_t *idx = list_idx<place_list(ROOMS)>(d);
    const uint32_t padded = (cnt + PLACE_CHUNK - 1u) / PLACE_CHUNK * PLACE_CHUNK;
    for (uint32_t i = threadIdx.x; i < padded; i += TPB) {
        const uint32_t m = i < cnt ? idx[lo + i] : 0xFFFFFFFFu;
        uint32_t end = 0u, g = 0u, f = 0u;
        if (m < d.n) {
            g = MODE == PAIRTAB_ONE_CELL ? 0u : (uint32_t)s.grp[m];
            if (g < s.n_cols) {
                end = hh_susceptible_end(d, q, m);
                if (CASES) f = sar_counted_f(s, tree_step(q, m), d.exposed_time, q.t_done);
            }
        }
        if (MEMBERS) {
            sm.m_end[i] = end;
            if (MODE != PAIRTAB_ONE_CELL) sm.m_grp[i] = (uint16_t)g;
            uint32_t row = 0u;
            if (sec && m < d.n && g < s.n_cols && place_secondary<ROOMS>(d, q, t, s, p, m, end, &row)) {
                if (MODE == PAIRTAB_ONE_CELL) ++*n_sec;
                else pairtab_add<MODE>(lds, s.at_risk, s.n_cols * s.n_cols + row + g, 1ull);
            }
        }
        if (CASES && f) {
            const uint32_t at = atomicAdd(&sm.n_cases, 1u);
            sm.c_f[at] = f;
            if (MODE != PAIRTAB_ONE_CELL) sm.c_grp[at] = (uint16_t)g;
        }
    }
}

// The staged cases against the staged members (`cnt` of them, padded to whole chunks): an item is a case and a chunk of
// PLACE_CHUNK members, neighbouring lanes take neighbouring cases of one chunk, so that the lanes of a wavefront read the same
// member at the same time (an LDS broadcast) and a place with few cases still fills the workgroup.
template <int MODE>
__device__ __forceinline__ void place_count(const SarWindow &s, const PlaceShared &sm, unsigned long long *lds, uint32_t cnt, unsigned long long *n_at)
{
    const uint32_t n_cases = sm.n_cases, n_chunks = (cnt + PLACE_CHUNK - 1u) / PLACE_CHUNK, items = n_cases * n_chunks;
    for (uint32_t it = threadIdx.x; it < items; it += TPB) {
        const uint32_t c = it % n_cases, base = it / n_cases * PLACE_CHUNK, f = sm.c_f[c];
        if (MODE == PAIRTAB_ONE_CELL) {
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
                if (f <= sm.m_end[base + k]) pairtab_add<MODE>(lds, s.at_risk, row + sm.m_grp[base + k], 1ull);
        }
    }
}

// The pairs (case j, member m of j's place at risk from j), per gathering.  A workgroup takes TPB neighbouring places at a time
// and skips those without a case (pass one's counts) or without a second member.  A place of up to 64 members is held by one
// wavefront in registers, a lane per member, several such places per workgroup at once: every counted case is broadcast with
// a shuffle and every lane compares its own member.  A longer place is staged by the whole workgroup in LDS, PLACE_TILE
// members at a time, and its cases run against its members from there, tile against tile where it is longer than a tile: its
// list is read once, or once per tile of cases, and not once per case.  No pair (j, j) is counted: a case stops being
// Susceptible at its own exposure, before its first infectious step.  MODE as for k_hh_sar: PAIRTAB_ONE_CELL, PAIRTAB_LDS
// (2 * n_cols^2 counters of dynamic LDS beside the tiles) or PAIRTAB_GLOBAL.
template <int MODE, bool ROOMS>
__global__ __launch_bounds__(TPB) void k_place_sar(Dev d, Setting q, Tree t, Place h, SarWindow s)
{
    extern __shared__ unsigned long long place_pairs[];
    __shared__ PlaceShared sm;
    const uint32_t cells = s.n_cols * s.n_cols, lane = threadIdx.x & 63u, n_list = list_len<place_list(ROOMS)>(d);
    const uint32_t *off = list_off<place_list(ROOMS)>(d), *idx = list_idx<place_list(ROOMS)>(d);
    if (MODE == PAIRTAB_LDS) pairtab_clear(place_pairs, 2u * cells);
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
                g = MODE == PAIRTAB_ONE_CELL ? 0u : (uint32_t)s.grp[m];
                if (g < s.n_cols) {
                    end = hh_susceptible_end(d, q, m);
                    f = sar_counted_f(s, tree_step(q, m), d.exposed_time, q.t_done);
                    uint32_t row = 0u;
                    if (place_secondary<ROOMS>(d, q, t, s, p, m, end, &row)) {
                        if (MODE == PAIRTAB_ONE_CELL) ++n_sec;
                        else pairtab_add<MODE>(place_pairs, s.at_risk, cells + row + g, 1ull);
                    }
                }
            }
            unsigned long long cases = __ballot(f != 0u);
            while (cases) {
                const int cj = __ffsll((long long)cases) - 1;
                cases &= cases - 1ull;
                const uint32_t fj = __shfl(f, cj, 64), gj = __shfl(g, cj, 64);
                if (fj > end) continue;                                   // (end is 0 on a lane without a member)
                if (MODE == PAIRTAB_ONE_CELL) ++n_at;
                else pairtab_add<MODE>(place_pairs, s.at_risk, gj * s.n_cols + g, 1ull);
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
    if (MODE == PAIRTAB_ONE_CELL) {
        pairtab_wave_add(s.at_risk, n_at);
        pairtab_wave_add(s.secondary, n_sec);
    }
    if (MODE == PAIRTAB_LDS) pairtab_flush(place_pairs, s.at_risk, 2u * cells);
}
