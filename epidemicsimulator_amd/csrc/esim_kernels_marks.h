// esim_kernels_marks.h -- the item map of a one-pass chunk: an item per building / room / route that somebody Infected stands in
// during the chunk (k_chunk_marks), and the stretches that did not fit an item's own records summed into its per-step counters
// (k_chunk_fold).
#pragma once
#include "esim_kernels_common.h"
#include "esim_chunk_sets.h"
// ------------------------------------------------------------------------- time-parallel chunk
// Inside a chunk nothing a draw depends on changes: who is Infected and where (known ahead), the mask
// status, the Philox counters.  A citizen's exposure step is therefore simply the EARLIEST step at which any of
// its draws succeeds (later draws would have been skipped by `is_susceptible()`, simulator.rs:337), and within a
// step a building exposure precedes a bus exposure (simulator.rs:268-401).  With the exposure step in the top
// bits of the citizen word and the bus bit right below, that is one atomicMin per successful draw -- so all
// steps of the chunk are drawn in ONE pass.
//   k_chunk_marks  an item per building / room / route that somebody Infected stands in during the chunk, and per item the
//                  stretches of steps in which each of them stands there (generate_exposures)
//   k_chunk_fold   the stretches that did not fit an item's own records, summed into its per-step counters; the prefix sums
//                  that let the draw pass take the items in equal shares
//   k_chunk_draw   the (member, slot of four marked steps) pairs of every item, densely over the lanes (apply_exposures); long
//                  member lists are cut into units
//   k_chunk_units  the units, dealt evenly; routes of more than 64 riders
//   k_chunk_books  exposure counts, records, log entries, clean-up, the next chunk's decisions
//                  (k_chunk_count / k_chunk_scatter: its two wide parts as kernels of their own while many are Infected)
__device__ __forceinline__ uint32_t hash64(unsigned long long k)
{
    k ^= k >> 33; k *= 0xff51afd7ed558ccdull; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull; k ^= k >> 33;
    return (uint32_t)k;
}

// Items live in an open-addressing hash map keyed by (building | n_bld + room | n_bld + n_room + route).  Whoever
// inserts the key claims the item: it takes the next id of its wavefront's own id range (a counter bumped once per claim
// would serialise the pass) and writes the item's record.  Everything the others add to the item -- their interval
// records, the per-step counters of those that found no record free, a route's registered bus steps -- is indexed by the
// hash SLOT, which the probe itself returns: nobody ever waits for anybody.
#define ITEM_UNUSED 0xFFFFFFFFu

// generate_exposures (simulator.rs:181-198) for every step of the chunk: one LANE per citizen that is Infected somewhere in
// the chunk.
__global__ __launch_bounds__(TPB) void k_chunk_marks(Dev d)
{
    Ctrl *ctrl = d.ctrl;
    const uint32_t t0 = ctrl->chunk_t0, n = ctrl->chunk_ok;
    if (!ctrl->chunk_parallel || n == 0u) return;
    // the marks of step t0 - 1 (a sequential or pipelined step's) would have gone in the exposure pass of step t0; this chunk has none
    clear_marks(d, ctrl, (t0 + MARK_SLOTS - 1u) & (MARK_SLOTS - 1u), blockIdx.x * TPB + threadIdx.x, gridDim.x * TPB);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (blockIdx.x * TPB + threadIdx.x) >> 6, n_waves = (gridDim.x * TPB) >> 6;
    const uint32_t i0 = ctrl->chunk_i0, i1 = ctrl->chunk_i1;                 // log slice of the chunk's Infected (k_decide)
    // every wavefront owns a fixed range of item ids (a citizen claims at most four items), so no counter is shared
    uint32_t n_remote = 0u;
    if (d.world > 1u) for (uint32_t r = 0; r < d.world; ++r) if (r != d.rank) n_remote += min(d.xs[(size_t)r * (1u + 3u * d.xs_cap)], d.xs_cap);
    const uint32_t per_wave = 4u * ((i1 - i0 + n_remote + n_waves - 1u) / n_waves + (n_remote ? 1u : 0u));
    if (wave == 0 && lane == 0) { ctrl->items_per_wave = per_wave; ctrl->n_items = per_wave * n_waves; }
    // (cannot fail on one shard: per_wave * n_waves <= 4 * E + 4 * CHUNK_WAVES_MAX <= 4 * E + 65 536 <= items_cap, future_body; E <= pairs)
    if ((unsigned long long)per_wave * n_waves > d.items_cap) { if (lane == 0) ctrl->error = (uint32_t)(-ESIM_ERANGE); return; }
    uint32_t next_id = wave * per_wave;
    // The chunk's schedule as step masks: riders are on a bus in at most CHUNK_BUS_STEPS steps (k_decide: a route item keeps one
    // bit per such step -- "an Infected rider of this route has registered the (route, step) pair").
    const ChunkMasks cm = chunk_masks(d.dec, lane, n);
    const M96 &AW = cm.AW, &BUS = cm.BUS;                                     // (who wears a mask, cm.EV, is the draw pass's business)
    const unsigned long long lt = (1ull << lane) - 1ull;
    const uint32_t pm0 = PROF_NOW();
    WORK_TALLY;
    uint32_t p_entries = 0u;
    uint32_t my_pairs = 0u;                                                   // (route, bus step) pairs this wavefront registered
    uint32_t ps[5] = { 0u, 0u, 0u, 0u, 0u };                                   // diagnostics: time per stage
    // ONE LANE PER INFECTED CITIZEN: the pass is a chain of dependent round trips (log entry -> word and keys -> hash claim ->
    // the item's lists / a record position -> the record), so what it needs is requests in flight, not lanes per citizen.
    // Where a citizen stands in each step follows from its Infected stretch and the schedule masks with a few 96-bit
    // operations.  Entry idx of the chunk's log slice (then of the commuters the other shards sent) belongs to wavefront
    // idx % n_waves -- every wavefront gets the same share, whatever the number of entries, and with it the same share of item
    // ids and of the draw pass's work.
    const uint32_t E = i1 - i0, total = E + n_remote;
    for (uint32_t round = 0; wave + n_waves * (round * 64u) < total; ++round) {
        const uint32_t pa = PROF_NOW();
        const uint32_t idx = wave + n_waves * (round * 64u + lane);
        bool act = idx < total;
        const bool remote = act && idx >= E;
        uint32_t c = 0u, w = 0u, r_bld = 0xFFFFFFFFu, r_room = 0xFFFFFFFFu;
        if (act && !remote) { c = d.log[i0 + idx]; w = d.cit[c]; }
        if (remote) {
            // Sharded: the Infected commuters the other shards sent (k_shared_pack, all-to-all): each stands in a building
            // (and room) that has members here too; it enters the map like a local citizen's work building and room.
            uint32_t e = idx - E;
            const uint32_t *seg = nullptr;
            for (uint32_t r = 0; r < d.world; ++r) {
                if (r == d.rank) continue;
                const uint32_t *sg = d.xs + (size_t)r * (1u + 3u * d.xs_cap);
                const uint32_t cnt = min(sg[0], d.xs_cap);
                if (e < cnt) { seg = sg; break; }
                e -= cnt;
            }
            act = false;
            if (seg) {
                w = seg[1u + 3u * e];
                const uint32_t sb = seg[2u + 3u * e], sr = seg[3u + 3u * e];
                const int32_t lb = d.shared_bld[sb];
                if (lb >= 0) {                                                // (else nobody of that building lives here)
                    act = true;
                    r_bld = (uint32_t)lb;
                    const int32_t lr = sr != 0xFFFFFFFFu ? d.shared_room[sr] : -1;
                    if (lr >= 0) r_room = (uint32_t)lr;                       // (a remote commuter's room may have no member here)
                }
            }
        }
        // the steps of the chunk in which the citizen is Infected and where it stands in each; a lane without a citizen has none
        const Stretch st = infected_stretch(d, w, t0, n, AW, BUS, act);
        // (a commuter from another shard only counts where it works: its home and its route are its own shard's business)
        const bool any_home = !remote && m96_any(st.home), any_work = m96_any(st.work), any_bus = !remote && m96_any(st.bus);
        const bool school = w & FL_WORK_SCHOOL;
        if (any_home || any_work || any_bus) { ++p_entries; WORK_ADD(WK_ENTRIES, 1); }
        // the four keys: home building, work building, room, route
        uint32_t src[4] = { 0u, r_bld, r_room, 0u };
        if (!remote && (any_home || any_work || any_bus)) {
            const uint4 k4 = d.where4[c];                                      // (one request for the four)
            src[0] = k4.x; src[1] = k4.y; src[2] = k4.z; src[3] = k4.w;
        }
        unsigned long long key[4];
        key[0] = any_home ? (unsigned long long)src[0] : HKEY_EMPTY;
        key[1] = any_work ? (unsigned long long)src[1] : HKEY_EMPTY;
        key[2] = (any_work && school && src[2] != 0xFFFFFFFFu) ? (unsigned long long)d.n_bld + src[2] : HKEY_EMPTY;
        key[3] = any_bus ? (unsigned long long)d.n_bld + d.n_room + src[3] : HKEY_EMPTY;
        const uint32_t pb = PROF_NOW() + (uint32_t)(key[0] & 0ull) + (uint32_t)(key[1] & 0ull) + (uint32_t)(key[2] & 0ull) + (uint32_t)(key[3] & 0ull);
        // claim or find the items: the first probes of all four keys go out together
        uint32_t slot[4];
        unsigned long long seen[4];
        // (a look before the CAS: the hundreds of Infected of one school all ask for the same key, and compare-and-swaps on one
        // address are served one after the other, loads are not -- a stale "empty" only costs the CAS it would have cost anyway)
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) {
            slot[k] = hash64(key[k]) & (d.hcap - 1u);
            seen[k] = key[k];
            if (key[k] != HKEY_EMPTY) seen[k] = d.hkey[slot[k]];
        }
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k)
            if (key[k] != HKEY_EMPTY && seen[k] == HKEY_EMPTY) seen[k] = atomicCAS(&d.hkey[slot[k]], HKEY_EMPTY, key[k]);
        bool claimed[4], pending[4];
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) {
            claimed[k] = false; pending[k] = false;
            if (key[k] == HKEY_EMPTY) continue;
            WORK_ADD(WK_KEYS, 1);
            if (seen[k] == HKEY_EMPTY) claimed[k] = true;
            else if (seen[k] == key[k]) pending[k] = true;
            else {
                // somebody else's key in the slot: linear probing
                uint32_t h = slot[k];
                bool found = false;
                for (uint32_t probe = 1; probe < d.hcap && !found; ++probe) {
                    h = (h + 1u) & (d.hcap - 1u);
                    const unsigned long long old = atomicCAS(&d.hkey[h], HKEY_EMPTY, key[k]);
                    if (old == HKEY_EMPTY) { claimed[k] = true; found = true; }
                    else if (old == key[k]) { pending[k] = true; found = true; }
                }
                // (cannot fail: at most 4 keys per entry, <= items_cap = hcap / 4 of them -- load <= 1/4)
                if (!found) { ctrl->error = (uint32_t)(-ESIM_ERANGE); key[k] = HKEY_EMPTY; h = 0u; }
                slot[k] = h;
            }
        }
        const uint32_t pc = PROF_NOW() + (slot[0] & 0u) + (slot[1] & 0u) + (slot[2] & 0u) + (slot[3] & 0u);
        const uint32_t iv_home = stretch_record(st, w);
        const uint32_t iv_work = iv_home | IV_AS_WORK;
        // the claimers take the next ids of this wavefront's range and write what the draw pass needs of the item; the claimer's
        // own stretch travels in it (a school's counts are looked up by slot from its rooms, so even its claimer's stretch goes
        // into a slot record), and a room's record names the slot of its school (the citizen's work building)
        // (ids in citizen order, a citizen's items side by side: the draw pass walks a wavefront's items in id order, and a
        // mix of short and long member lists along the way keeps its load even)
        uint32_t before = 0u, n_claims = 0u;
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) { const unsigned long long cm = __ballot(claimed[k]); before += (uint32_t)__popcll(cm & lt); n_claims += (uint32_t)__popcll(cm); }
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) {
            if (claimed[k]) {
                WORK_ADD(WK_CLAIMS, 1);
                const uint32_t v = next_id + before++;
                d.hitems[v] = slot[k];
                const uint32_t id = (uint32_t)key[k];
                ItemRec rec = { id, 0u, 0u, 0u, 0u, 0u, k == 2u ? slot[1] : 0xFFFFFFFFu,
                                k == 0u ? iv_home : (k == 1u && !school) || k == 2u ? iv_work : 0u };
                if (k == 0u || k == 1u) {
                    const uint4 b4 = *reinterpret_cast<const uint4 *>(&d.bld8[id]);
                    rec.a_lo = b4.x; rec.a_hi = b4.y; rec.b_lo = b4.z; rec.b_hi = b4.w;
                    rec.aux = d.bld8[id].type;
                } else if (k == 2u) {
                    const uint32_t r = id - d.n_bld;
                    rec.a_lo = d.room_off[r]; rec.a_hi = d.room_off[r + 1u];
                    rec.aux = d.room_bld[r];
                }
                d.item_rec[v] = rec;
            }
        }
        next_id += n_claims;
        const uint32_t pd = PROF_NOW();
        // Somebody else's building / room: my stretch goes into one of the slot's ITEM_RECS records; when they are taken,
        // into its per-step counters (`vec`), one atomic per step.  The route: which of my bus steps nobody has registered yet.
        uint32_t mine = 0u;                                                   // bit i: I ride, Infected, in the i-th bus step of the chunk
        if (any_bus) {
            uint32_t i = 0u;
            for (unsigned long long m = BUS.lo; m; m &= m - 1ull, ++i) mine |= (uint32_t)((st.bus.lo >> __builtin_ctzll(m)) & 1ull) << i;
            for (uint32_t m = BUS.hi; m; m &= m - 1u, ++i) mine |= ((st.bus.hi >> __builtin_ctz(m)) & 1u) << i;
        }
        bool add_rec[3];
        uint32_t old[4] = { 0u, 0u, 0u, 0u };
#pragma unroll
        for (uint32_t k = 0; k < 3u; ++k) {
            // (a school's Infected -- hundreds -- do not queue for record positions: they count themselves, see below)
            add_rec[k] = pending[k] && !(k == 1u && school);
            if (add_rec[k]) old[k] = atomicAdd(&d.slot_state[slot[k]], 1u);
        }
        if (claimed[1] && school) d.slot_state[slot[1]] = SLOT_COUNTERS_ONLY;     // (tells item_counts and the clean-up)
        if (any_bus && key[3] != HKEY_EMPTY) old[3] = atomicOr(&d.slot_state[slot[3]], mine);
        // positions beyond ITEM_RECS: the record goes into the building's / room's own stretch of `ovf` (one place per member, so
        // it cannot run out -- except for commuters from other shards, who are no members here: those add themselves to the
        // slot's per-step counters, one atomic per step, which nobody has to wait for; so does everybody in a school
        // building); the first to get there lists the slot for k_chunk_fold
        bool direct[3], first[3];
        uint32_t first_base[3] = { 0u, 0u, 0u }, first_cap[3] = { 0u, 0u, 0u };
        if (school && key[1] != HKEY_EMPTY) {
            // a school building: my stretch goes into the school's difference arrays (two atomics, four for a rider, whatever
            // the number of steps); whoever claimed the building's item lists it for k_chunk_fold
            const int32_t sch = d.sch_of_bld[(uint32_t)key[1]];
            if (sch < 0 || (uint32_t)sch >= d.n_sch) RAISE(ctrl, ESIM_ERANGE, ERR_AT_SCHOOL);
            else {
                uint32_t *dd = d.sch_diff + ((size_t)sch * SD_REPL + (wave & (SD_REPL - 1u))) * 2u * FREE_MAX;
                WORK_ADD(WK_DIRECT, (w & FL_USES_PT) ? 4 : 2);
                atomicAdd(&dd[st.iv_a], 1u);
                if (st.iv_b + 1u < FREE_MAX) atomicAdd(&dd[st.iv_b + 1u], 0xFFFFFFFFu);
                if (w & FL_USES_PT) {
                    atomicAdd(&dd[FREE_MAX + st.iv_a], 1u);
                    if (st.iv_b + 1u < FREE_MAX) atomicAdd(&dd[FREE_MAX + st.iv_b + 1u], 0xFFFFFFFFu);
                }
                if (claimed[1]) { first_base[1] = (uint32_t)sch; first_cap[1] = 0xFFFFFFFFu; }
            }
        }
#pragma unroll
        for (uint32_t k = 0; k < 3u; ++k) {
            direct[k] = false; first[k] = k == 1u && first_cap[1] == 0xFFFFFFFFu;
            if (!add_rec[k]) continue;
            WORK_ADD(WK_RECORDS, 1);
            const uint32_t iv = k == 0u ? iv_home : iv_work;
            if (old[k] < ITEM_RECS) { d.slot_iv[(size_t)slot[k] * SLOT_IV_STRIDE + old[k]] = iv; continue; }
            const uint32_t q = old[k] - ITEM_RECS, id = (uint32_t)key[k];
            uint32_t base, cap;
            if (k < 2u) { base = d.bld8[id].ovf_lo; cap = d.bld8[id].ovf_hi - base; }
            else { const uint32_t r = id - d.n_bld; const uint32_t o = d.room_off[r]; base = d.ovf_room_base + o; cap = d.room_off[r + 1u] - o; }
            if (q < cap) { d.ovf[base + q] = iv; first[k] = q == 0u; first_base[k] = base; first_cap[k] = cap; }
            else direct[k] = true;
        }
        {
            // (one reservation in this wavefront's list for everything the 64 citizens list)
            const unsigned long long f[3] = { __ballot(first[0]), __ballot(first[1]), __ballot(first[2]) };
            const uint32_t n_first = (uint32_t)(__popcll(f[0]) + __popcll(f[1]) + __popcll(f[2]));
            if (n_first) {
                const uint32_t r = wave & (SUBQ - 1u);
                uint32_t at0 = 0u;
                if (lane == 0) at0 = atomicAdd(&d.hot[(HOT_BIG + r) * HOT_STRIDE], n_first);
                at0 = __shfl(at0, 0, 64);
                uint32_t *bl = d.big_list + (size_t)r * d.big_qcap * 3u;
                uint32_t at = at0;
#pragma unroll
                for (uint32_t k = 0; k < 3u; ++k) {
                    const uint32_t pos = at + (uint32_t)__popcll(f[k] & lt);
                    if (first[k] && pos < d.big_qcap) { bl[3u * pos] = slot[k]; bl[3u * pos + 1u] = first_base[k]; bl[3u * pos + 2u] = first_cap[k]; }
                    at += (uint32_t)__popcll(f[k]);
                }
                // (cannot fail: a wavefront lists <= 3 slots per entry, <= 3/4 per_wave; queue r serves n_waves / SUBQ wavefronts (grids are
                // whole groups of 64 wavefronts), so <= 3/4 * items_cap / SUBQ < big_qcap)
                if (at0 + n_first > d.big_qcap && lane == 0) ctrl->error = (uint32_t)(-ESIM_ERANGE);
            }
        }
#pragma unroll
        for (uint32_t k = 0; k < 3u; ++k) {
            const M96 at = k == 0u ? st.home : st.work;
            for (unsigned long long sp = __ballot(direct[k]); sp; sp &= sp - 1ull) {
                const int src_lane = __builtin_ctzll(sp);
                const uint32_t sl = __shfl(slot[k], src_lane, 64), hi = __shfl(at.hi, src_lane, 64);
                const unsigned long long lo = ((unsigned long long)__shfl((uint32_t)(at.lo >> 32), src_lane, 64) << 32) | __shfl((uint32_t)at.lo, src_lane, 64);
                uint32_t *v = d.vec + (size_t)sl * FREE_MAX;
                WORK_ADD(WK_DIRECT, ((lo >> lane) & 1ull) + ((lane < 32u && ((hi >> lane) & 1u)) ? 1 : 0));
                if ((lo >> lane) & 1ull) atomicAdd(&v[lane], 1u);
                if (lane < 32u && ((hi >> lane) & 1u)) atomicAdd(&v[64u + lane], 1u);
            }
        }
        const uint32_t pe = PROF_NOW() + (old[0] & 0u) + (old[1] & 0u) + (old[2] & 0u) + (old[3] & 0u);
        // register the (route, step) pairs that are new: k_chunk_draw ranks the riders of each once
        const uint32_t new_bits = (any_bus && key[3] != HKEY_EMPTY) ? (mine & ~old[3]) : 0u;
        if (__any(new_bits != 0u)) {
            const bool big = w & FL_BIG_ROUTE;
            const uint32_t rt = src[3];                                       // the route itself, not its item: saves the pass a hop
            // routes of few riders: this wavefront's own stretch of the list, no shared counter; the others share one
            const uint32_t K = PAIR_K(per_wave, ctrl->chunk_bus);
            uint32_t *list = d.route_pairs + (size_t)wave * K;
            uint32_t n_big = 0u;
            for (uint32_t i = 0; i < CHUNK_BUS_STEPS; ++i) n_big += (uint32_t)__popcll(__ballot(big && ((new_bits >> i) & 1u)));
            uint32_t big_base = 0u;
            if (n_big) {
                if (lane == 0) big_base = atomicAdd(&d.hot[HOT_BIGPAIRS * HOT_STRIDE], n_big);
                big_base = __shfl(big_base, 0, 64);
                // (cannot fail: big_pairs_cap bounds the distinct (big route, bus step) pairs of any chunk, esim_upload_population)
                if (big_base + n_big > d.big_pairs_cap) { if (lane == 0) ctrl->error = (uint32_t)(-ESIM_ERANGE); n_big = 0u; big_base = 0xFFFFFFFFu; }
            }
            uint32_t i = 0u;
            auto put = [&](uint32_t j) {
                const bool f = (new_bits >> i) & 1u;
                const unsigned long long ms = __ballot(f && !big), mb = __ballot(f && big);
                if (f && !big) {
                    const uint32_t pos = my_pairs + (uint32_t)__popcll(ms & lt);
                    // (cannot fail: <= per_wave / 4 entries x chunk_bus pairs <= K; equal when each entry rides its own route every bus step)
                    if (pos < K) list[pos] = (rt << 7) | j; else ctrl->error = (uint32_t)(-ESIM_ERANGE);
                }
                if (f && big && big_base != 0xFFFFFFFFu) d.route_pairs_big[big_base + (uint32_t)__popcll(mb & lt)] = (rt << 7) | j;
                my_pairs += (uint32_t)__popcll(ms);
                if (big_base != 0xFFFFFFFFu) big_base += (uint32_t)__popcll(mb);
                ++i;
            };
            for (unsigned long long m = BUS.lo; m; m &= m - 1ull) put((uint32_t)__builtin_ctzll(m));
            for (uint32_t m = BUS.hi; m; m &= m - 1u) put(64u + (uint32_t)__builtin_ctz(m));
            my_pairs = min(my_pairs, K);
        }
        { const uint32_t pf = PROF_NOW(); ps[0] += pb - pa; ps[1] += pc - pb; ps[2] += pd - pc; ps[3] += pe - pd; ps[4] += pf - pe; }
    }
    if (lane == 0) { d.pair_cnt[wave] = my_pairs; d.used_cnt[wave] = next_id - wave * per_wave; }
    WORK_FLUSH(d);
    const uint32_t pm1 = PROF_NOW();
    PROF_PUT(d, 8, pm0); PROF_PUT(d, 9, pm1); PROF_PUT(d, 10, p_entries);
    PROF_PUT(d, 11, ps[0]); PROF_PUT(d, 12, ps[1]); PROF_PUT(d, 13, ps[2]); PROF_PUT(d, 14, ps[3]); PROF_PUT(d, 15, ps[4]);
    (void)p_entries; (void)ps;
}

// The interval records k_chunk_marks put into `ovf` (slots with more than ITEM_RECS of them: schools, large work places),
// summed into the slots' per-step counters before the draw pass reads them.  One wavefront per listed slot, 64 records at a
// time; each lane turns its record into the set of steps in which that citizen stands there, one ballot per step counts them.
__global__ __launch_bounds__(TPB) void k_chunk_fold(Dev d)
{
    Ctrl *ctrl = d.ctrl;
    const uint32_t n = ctrl->chunk_ok;
    if (!ctrl->chunk_parallel || n == 0u) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (blockIdx.x * TPB + threadIdx.x) >> 6, n_waves = (gridDim.x * TPB) >> 6;
    const uint32_t per_wave = ld(&ctrl->items_per_wave);
    if ((unsigned long long)per_wave * n_waves > d.items_cap) return;
    if (blockIdx.x == 0) {
        // for k_chunk_draw: used_pref[k] = ids handed out by the wavefronts before k
        __shared__ uint32_t s_pref[CHUNK_WAVES_MAX + 1u];
        __shared__ uint32_t s_wtot[TPB / 64];
        const uint32_t pf0 = PROF_NOW();
        constexpr uint32_t RUN = CHUNK_WAVES_MAX / TPB;
        const uint32_t run = (n_waves + TPB - 1u) / TPB, b = threadIdx.x * run;   // <= RUN
        uint32_t cnt[RUN];
        uint32_t sum = 0u;
#pragma unroll
        for (uint32_t k = 0; k < RUN; ++k) { cnt[k] = (k < run && b + k < n_waves) ? min(d.used_cnt[b + k], per_wave) : 0u; sum += cnt[k]; }
        uint32_t x = sum;
        for (uint32_t o = 1; o < 64u; o <<= 1) { const uint32_t y = __shfl_up(x, o, 64); if (lane >= o) x += y; }
        if (lane == 63u) s_wtot[threadIdx.x >> 6] = x;
        if (threadIdx.x == 0) s_pref[0] = 0u;
        __syncthreads();
        const uint32_t pf1 = PROF_NOW();
        uint32_t acc = x - sum;
        for (uint32_t k = 0; k < (threadIdx.x >> 6); ++k) acc += s_wtot[k];
#pragma unroll
        for (uint32_t k = 0; k < RUN; ++k) if (k < run && b + k < n_waves) { acc += cnt[k]; s_pref[b + k + 1u] = acc; }
        __syncthreads();
        const uint32_t pf2 = PROF_NOW();
        for (uint32_t w = threadIdx.x; w <= n_waves; w += TPB) d.used_pref[w] = s_pref[w];
        BOOKS_PROF(d, 8, pf1 - pf0); BOOKS_PROF(d, 9, pf2 - pf1); BOOKS_PROF(d, 10, PROF_NOW() - pf2);
        (void)pf0; (void)pf1; (void)pf2;
    }
    // list `wave & 63`, every (n_waves / 64)-th entry of it
    const uint32_t qr = wave & (SUBQ - 1u), first = wave >> 6, step = n_waves >> 6;
    const uint32_t n_list = step ? min(ld(&d.hot[(HOT_BIG + qr) * HOT_STRIDE]), d.big_qcap) : 0u;
#ifdef ESIM_PROFILE_FOLD
    const uint32_t pq0 = PROF_NOW();
    uint32_t pq_rec = 0u, pq_n = 0u;
    PROF_PUT(d, 11, 0u); PROF_PUT(d, 12, 0u); PROF_PUT(d, 13, 0u);
#endif
    if (first >= n_list) return;
    WORK_TALLY;
    const uint32_t *bl = d.big_list + (size_t)qr * d.big_qcap * 3u;
    const Decision q0 = lane < n ? d.dec[lane] : Decision{ 0u, 0u, 0u, 0u };   // (chunk_masks, written out: DESIGN.md 3.15)
    const Decision q1 = 64u + lane < n ? d.dec[64u + lane] : Decision{ 0u, 0u, 0u, 0u };
    const M96 AW = { __ballot(lane < n && q0.at_work != 0u), (uint32_t)__ballot(64u + lane < n && q1.at_work != 0u) };
    const M96 BUS = { __ballot(lane < n && q0.bus_dir != 0u), (uint32_t)__ballot(64u + lane < n && q1.bus_dir != 0u) };
    for (uint32_t g = first; g < n_list; g += 64u * step) {
        // 64 of this wavefront's entries at a time, a lane each: the slot, where its records are and how many (those that
        // did not fit counted themselves)
        uint32_t slot_l = 0u, base_l = 0u, n_ov_l = 0u, sch_l = 0xFFFFFFFFu;
        const uint32_t mine = g + lane * step;
        if (mine < n_list) {
            slot_l = bl[3u * mine]; base_l = bl[3u * mine + 1u];
            const uint32_t cap_l = bl[3u * mine + 2u] & 0x7FFFFFFFu, all_ovf = bl[3u * mine + 2u] >> 31;
            if (all_ovf) {
                // a school building (k_chunk_marks: capacity word 0xFFFFFFFF, the school's number where the records would start)
                sch_l = base_l; base_l = 0u;
                if (sch_l >= d.n_sch || slot_l >= d.hcap) { sch_l = 0xFFFFFFFFu; slot_l = 0u; RAISE(ctrl, ESIM_ERANGE, ERR_AT_BIG_LIST); }
            } else
            if (slot_l < d.hcap && base_l <= d.ovf_n && cap_l <= d.ovf_n - base_l) {
                const uint32_t state = d.slot_state[slot_l];
                n_ov_l = min((state > ITEM_RECS && state < SLOT_COUNTERS_ONLY) ? state - ITEM_RECS : 0u, cap_l);
            } else { slot_l = 0u; base_l = 0u; ctrl->error = (uint32_t)(-ESIM_ERANGE); }   // (no list entry k_chunk_marks wrote looks like this)
        }
        const uint32_t m = min(64u, (n_list - g + step - 1u) / step);
        // ... then slot by slot, lanes = records; the first 64 records of eight slots are fetched together
        for (uint32_t i8 = 0; i8 < m; i8 += 8u) {
        uint32_t ivs[8];
#pragma unroll
        for (uint32_t u = 0; u < 8u; ++u) ivs[u] = (i8 + u < m && lane < FX(n_ov_l, min(i8 + u, 63u))) ? d.ovf[FX(base_l, min(i8 + u, 63u)) + lane] : 0u;
#pragma unroll
        for (uint32_t u = 0; u < 8u; ++u) {
            const uint32_t i = i8 + u;
            if (i >= m) break;
            const uint32_t slot = FX(slot_l, i), base = FX(base_l, i), n_ov = FX(n_ov_l, i);
            uint32_t iv = ivs[u];
            uint32_t c0 = 0u, c1 = 0u;
            WORK_ADD(WK_FOLDED, lane == 0 ? n_ov : 0);
            if (FX(sch_l, i) != 0xFFFFFFFFu) {
                // A school building: the prefix sums of its difference arrays are its Infected per step -- all of
                // them, and the riders among them --; they stand there while those with a work place are at work, the riders not
                // while riders are on a bus (what infected_stretch's `work` says per citizen).  The arrays are zeroed for the next chunk.
                uint32_t *dd = d.sch_diff + (size_t)FX(sch_l, i) * SD_REPL * 2u * FREE_MAX;
                uint32_t a0 = 0u, a1 = 0u, p0 = 0u, p1 = 0u;
#pragma unroll
                for (uint32_t r = 0; r < SD_REPL; ++r) {
                    uint32_t *rr = dd + (size_t)r * 2u * FREE_MAX;
                    a0 += rr[lane]; p0 += rr[FREE_MAX + lane];
                    if (lane < FREE_MAX - 64u) { a1 += rr[64u + lane]; p1 += rr[FREE_MAX + 64u + lane]; }
                }
#pragma unroll
                for (uint32_t r = 0; r < SD_REPL; ++r) {
                    uint32_t *rr = dd + (size_t)r * 2u * FREE_MAX;
                    rr[lane] = 0u; rr[FREE_MAX + lane] = 0u;
                    if (lane < FREE_MAX - 64u) { rr[64u + lane] = 0u; rr[FREE_MAX + 64u + lane] = 0u; }
                }
                for (uint32_t o = 1; o < 64u; o <<= 1) {
                    const uint32_t ya = __shfl_up(a0, o, 64), yp = __shfl_up(p0, o, 64), yb = __shfl_up(a1, o, 64), yq = __shfl_up(p1, o, 64);
                    if (lane >= o) { a0 += ya; p0 += yp; a1 += yb; p1 += yq; }
                }
                a1 += __shfl(a0, 63, 64); p1 += __shfl(p0, 63, 64);
                if (lane < n) c0 = ((AW.lo >> lane) & 1ull) ? a0 - (((BUS.lo >> lane) & 1ull) ? p0 : 0u) : 0u;
                if (lane < FREE_MAX - 64u && 64u + lane < n) c1 = ((AW.hi >> lane) & 1u) ? a1 - (((BUS.hi >> lane) & 1u) ? p1 : 0u) : 0u;
            }
#ifdef ESIM_PROFILE_FOLD
            pq_rec += n_ov; ++pq_n;
#endif
            for (uint32_t b = 0; b < n_ov; b += 64u) {
                if (b) iv = b + lane < n_ov ? d.ovf[base + b + lane] : 0u;
                const uint32_t nb = min(64u, n_ov - b);
                if (nb <= 12u) {
                    // few records (a class room): one after the other, its set of steps in scalar registers, lanes = steps
                    for (uint32_t k = 0; k < nb; ++k) {
                        iv_count(FX(iv, k), lane, AW, BUS, c0, c1);
                    }
                    continue;
                }
                // many: lanes = records, one ballot per step
                const M96 at = iv_steps(iv, AW, BUS);
                for (uint32_t j = 0; j < n && j < 64u; ++j) {
                    const uint32_t k = (uint32_t)__popcll(__ballot((at.lo >> j) & 1ull));
                    if (lane == j) c0 += k;
                }
                for (uint32_t j = 64u; j < n; ++j) {
                    const uint32_t k = (uint32_t)__popcll(__ballot((at.hi >> (j - 64u)) & 1u));
                    if (lane == j - 64u) c1 += k;
                }
            }
            uint32_t *v = d.vec + (size_t)slot * FREE_MAX;
            // (added, not stored: commuters from other shards may have counted themselves there; atomics, because nobody has
            // to wait for them)
            if (lane < n && c0) atomicAdd(&v[lane], c0);
            if (64u + lane < n && c1) atomicAdd(&v[64u + lane], c1);
        }
        }
    }
    WORK_FLUSH(d);
#ifdef ESIM_PROFILE_FOLD
    PROF_PUT(d, 11, pq_n); PROF_PUT(d, 12, PROF_NOW() - pq0); PROF_PUT(d, 13, pq_rec);
#endif
}
