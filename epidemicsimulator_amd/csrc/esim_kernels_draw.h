// esim_kernels_draw.h -- the draws of a one-pass chunk: a member list over the marked steps (member_pairs), a (route, bus step)
// pair (route_pair_small, route_pair_big), the items dealt to the wavefronts (k_chunk_draw) and the deferred units of long member
// lists (k_chunk_units).
#pragma once
#include "esim_kernels_common.h"
#include "esim_rank.h"
#include "esim_chunk_sets.h"
#include "esim_kernels_marks.h"
// A successful draw of citizen m in step s (bus: on public transport).
__device__ __forceinline__ void expose_min(const Dev &d, Ctrl *ctrl, uint32_t m, uint32_t w, uint32_t s, uint32_t bus)
{
    const uint32_t cand = CW_MAKE(s + TE_BIAS, bus | (w & CW_KEEP));
    const uint32_t prev = atomicMin(&d.cit[m], cand);
    // exposed on a bus although the chunk's plan vaccinates it later: it leaves the eligible set with this exposure (simulator.rs:447-449),
    // so the plan of the steps from here on is off by this citizen -- noted for the repair (k_chunk_vax<true>)
    if (bus && cand < prev && CW_VAX_REL(w) != CW_VAX_NONE) {
        const uint32_t at = atomicAdd(&d.hot[HOT_LOST * HOT_STRIDE], 1u);
        if (at < LOST_CAP) d.lost_list[at] = m;
    }
    if (cand < prev && CW_TE(prev) == TE_SUSCEPTIBLE) {                       // first exposure in this chunk
        const uint32_t r = m & (SUBQ - 1u);
        d.newexp[(size_t)r * d.newexp_cap + atomicAdd(&d.hot[(HOT_NEWEXP + r) * HOT_STRIDE], 1u)] = m;
    }
}

struct ChunkShared {
    Decision dec[FREE_MAX];
    uint64_t thr[512];
};
// The chunk's decisions and thresholds into the workgroup's LDS, by its n_threads threads (the caller's barrier follows).
__device__ __forceinline__ void stage_chunk(const Dev &d, ChunkShared &sm, uint32_t n, uint32_t n_threads)
{
    for (uint32_t i = threadIdx.x; i < n; i += n_threads) sm.dec[i] = d.dec[i];
    for (uint32_t i = threadIdx.x; i < 512u; i += n_threads) sm.thr[i] = d.thr[i];
}
struct RouteShared {
    uint32_t s_key[CHUNK_ROUTE_MAX];
    uint16_t s_bus[CHUNK_ROUTE_MAX];
    uint8_t s_inf[CHUNK_ROUTE_MAX];
    uint32_t s_cnt[CHUNK_ROUTE_MAX + 1];
    uint32_t s_seen[CHUNK_ROUTE_MAX / 32u];               // ranks handed out (rank_seen)
};
// Per wavefront: the item's / the school's Infected per step; 64 staged members; the item's slots of four time steps
// (item_steps_regs).  A slot's descriptor is eight words: [0] first step of the slot + 3 (bits 0-6; a slot may begin up to three
// steps before the chunk) | its steps that are marked (8-11) | in which of them those with a work place are at work (12-15) | in
// which masks are worn everywhere (16-19); [1] the item's Infected & 255 in the four steps, a byte each (the threshold index,
// `as u8`); [2] the same for the school of a room; [3], [4] the item's Infected in steps 0-1 / 2-3, 16 bits each.
#define SLOT_STEPS 4u
struct WaveScratch { uint32_t rounds; uint32_t cnt[FREE_MAX]; uint32_t sch[FREE_MAX]; uint32_t mem_id[64]; uint32_t mem_w[64]; uint4 desc[2u * (FREE_MAX / SLOT_STEPS + 1u)]; };
// the school's Infected in step `lane` (s0) and 64 + lane (s1) of the chunk into the wavefront's scratch
__device__ __forceinline__ void put_school(WaveScratch &ws, uint32_t lane, uint32_t s0, uint32_t s1) { ws.sch[lane] = s0; if (lane < FREE_MAX - 64u) ws.sch[64u + lane] = s1; }

// One member list of one item over the marked steps of the chunk.  The time steps 4k .. 4k+3 share one Philox block (RNG
// contract: step t takes word t & 3), so the unit of work is a (member, slot of four steps) pair: the pairs [p_lo, p_hi) are
// spread densely over the 64 lanes (the draws are Philox-bound -- 20 quarter-rate multiplies a block -- so idle lanes and
// blocks used for one draw only are what costs).  ws.desc: the item's slots with a marked step, in order, S of them.
// kind 0 residents, 1 workers, 2 room participants.
// pre_m / pre_w: members lo + pre_base + lane of the list and their words when the caller has already fetched them (have_pre).
__device__ __forceinline__ void member_pairs(const Dev &d, Ctrl *ctrl, const ChunkShared &sm, WaveScratch &ws, const uint32_t *idx,
                                             uint32_t lo, uint32_t p_lo, uint32_t p_hi, uint32_t lane, uint32_t kind, uint32_t S, uint32_t t0 WORK_ARG,
                                             bool have_pre = false, uint32_t pre_m = 0u, uint32_t pre_w = 0u, uint32_t pre_base = 0u)
{
    const uint64_t seed = ((uint64_t)d.seed_hi << 32) | d.seed_lo;
    // members touched by the slots [p_lo, p_hi): staged in LDS 64 at a time -- every member recurs once per slot
    const uint32_t m_first = p_lo / S, m_last = (p_hi - 1u) / S;
    for (uint32_t mb = m_first; mb <= m_last; mb += 64u) {
        __builtin_amdgcn_wave_barrier();
        if (mb + lane <= m_last) {
            WORK_ADD(WK_MEMBERS, 1); WORK_ADD(WK_MEMBERS_IDX, idx ? 1 : 0);
            if (have_pre && mb == pre_base) { ws.mem_id[lane] = pre_m; ws.mem_w[lane] = pre_w; }
            else {
                const uint32_t m = idx ? idx[lo + mb + lane] : lo + mb + lane;
                ws.mem_id[lane] = m;
                ws.mem_w[lane] = d.cit[m];
            }
        }
        __builtin_amdgcn_wave_barrier();
        const uint32_t q_lo = max(p_lo, mb * S), q_hi = min(p_hi, (mb + 64u) * S);
#ifdef ESIM_WAVE_PROFILE
        if (lane == 0) ws.rounds += (q_hi - q_lo + 63u) / 64u;
#endif
        for (uint32_t p = q_lo + lane; p < q_hi; p += 64u) {
            const uint32_t um = p / S, si = p - um * S;
            const uint32_t m = ws.mem_id[um - mb], w = ws.mem_w[um - mb];
            const uint32_t te = CW_TE(w);
            WORK_ADD(WK_PAIRS, 1);
            if (te >= TE_RECOVERED && te != TE_SUSCEPTIBLE) continue;
            const uint4 dsc = ws.desc[2u * si];
            const uint32_t cnt23 = ws.desc[2u * si + 1u].x;
            const int jb = (int)(dsc.x & 127u) - 3;                            // first step of the slot (may lie before the chunk)
            const uint32_t mk = (dsc.x >> 8) & 15u, atw = (dsc.x >> 12) & 15u, everywhere = (dsc.x >> 16) & 15u;
            // The steps of the slot in which this member takes a draw, all four at once: marked; Susceptible when this list is
            // walked in that step -- w > (step << 19 | the bits an exposure keeps), i.e. never exposed, or so far only by
            // something that comes later (a later step, or a bus of this step: that exposure may be undercut) --; not Vaccinated
            // by then (k_chunk_vax); standing in the building's area (simulator.rs:324)
            const uint32_t vrel = CW_VAX_REL(w);
            const int js = (int)te + (((w & ~CW_KEEP) & ((1u << CW_TE_SHIFT) - 1u)) ? 1 : 0) - (int)(t0 + TE_BIAS);   // Susceptible in steps j < js
            const int lim = min(js, vrel == CW_VAX_NONE ? (int)FREE_MAX : (int)vrel + 1) - jb;                  // ... of the slot: h < lim
            const uint32_t early = lim <= 0 ? 0u : lim >= (int)SLOT_STEPS ? 15u : (1u << lim) - 1u;
            const bool same = w & FL_SAME_AREA;
            const uint32_t here = kind == 0u ? (((w & FL_HAS_WORK) && !same) ? ~atw : 15u) : (same ? 15u : atw);
            const uint32_t act = mk & early & here;
            if (!act) continue;
            WORK_ADD(WK_PAIRS_ACTIVE, 1);
            const uint32_t nn = kind == 2u ? dsc.z : dsc.y;                    // exposure_count & 255 per step: infected in the building
            const uint32_t row = (w & FL_MASK_COMPLIANT) ? 0u : everywhere;   // steps in which this member's chance is the masked one
            uint64_t thr[SLOT_STEPS];
#pragma unroll
            for (uint32_t h = 0; h < SLOT_STEPS; ++h) thr[h] = sm.thr[(((row >> h) & 1u) << 8) + ((nn >> (8u * h)) & 255u)];
            const uint32_t gid = d.id_base + m;
            const uint32_t s_blk = (uint32_t)((int)t0 + jb) + (uint32_t)__builtin_ctz(act);   // a time step of the slot: names its block
            uint32_t hit = 0u;                                                // bit h: a draw of step h succeeded
            if (kind == 2u) {
                // School::find_exposures: one draw per Infected in the room (building.rs:494-522); the earliest step decides
                const uint32_t cnt[SLOT_STEPS] = { dsc.w & 0xFFFFu, dsc.w >> 16, cnt23 & 0xFFFFu, cnt23 >> 16 };
                uint32_t kmax = 0u;
#pragma unroll
                for (uint32_t h = 0; h < SLOT_STEPS; ++h) if ((act >> h) & 1u) kmax = max(kmax, cnt[h]);
                const uint32_t first_act = act & (0u - act);
#ifdef ESIM_COUNT_WORK
                for (uint32_t h = 0; h < SLOT_STEPS; ++h) if ((act >> h) & 1u) WORK_ADD(WK_DRAWS, cnt[h]);
#endif
                for (uint32_t k = 0; k < kmax && !(hit & first_act); ++k) {
                    WORK_ADD(WK_BLOCKS, 1);
                    const philox_out o = esim_draw_block(seed, gid, s_blk, ESIM_SLOT_ROOM0 + k);
                    const uint32_t wd[SLOT_STEPS] = { o.w0, o.w1, o.w2, o.w3 };
#pragma unroll
                    for (uint32_t h = 0; h < SLOT_STEPS; ++h) if (((act >> h) & 1u) && k < cnt[h] && (uint64_t)wd[h] < thr[h]) hit |= 1u << h;
                }
            } else {
                WORK_ADD(WK_BLOCKS, 1); WORK_ADD(WK_DRAWS, __popc(act));
                const philox_out o = esim_draw_block(seed, gid, s_blk, kind == 0u ? ESIM_SLOT_HOME : ESIM_SLOT_WORK);
                const uint32_t wd[SLOT_STEPS] = { o.w0, o.w1, o.w2, o.w3 };
#pragma unroll
                for (uint32_t h = 0; h < SLOT_STEPS; ++h) if ((uint64_t)wd[h] < thr[h]) hit |= 1u << h;
                hit &= act;
            }
            if (hit) { WORK_ADD(WK_HITS, 1); expose_min(d, ctrl, m, w, (uint32_t)((int)t0 + jb) + (uint32_t)__builtin_ctz(hit), 0u); }   // (the earliest wins anyway)
        }
    }
}

// The marked steps of item v as slots of four time steps (4k .. 4k+3), in order, with what member_pairs needs of each step,
// into this wavefront's scratch (ws.sch holds the school's counts when the item is a room).  Returns S, the number of slots
// with a marked step.
// AW / EV: the steps of the chunk in which those with a work place are at work / masks are worn everywhere.
__device__ __forceinline__ uint32_t item_steps_regs(uint32_t c0, uint32_t c1, uint32_t lane, WaveScratch &ws, uint32_t t0, const M96 &AW, const M96 &EV)
{
    ws.cnt[lane] = c0;
    if (lane < FREE_MAX - 64u) ws.cnt[64u + lane] = c1;
    const M96 MK = { __ballot(c0 != 0u), (uint32_t)__ballot(lane < FREE_MAX - 64u && c1 != 0u) };
    __builtin_amdgcn_wave_barrier();
    // lane L looks at the slot whose first time step is step j0 = 4L - (t0 & 3) of the chunk (negative: before the chunk)
    const int j0 = (int)(SLOT_STEPS * lane) - (int)(t0 & (SLOT_STEPS - 1u));
    const uint32_t mk = lane <= FREE_MAX / SLOT_STEPS ? m96_nibble(MK, j0) : 0u;
    const unsigned long long present = __ballot(mk != 0u);
    if (mk) {
        // the counts of the slot's four steps (the item's, the school's), all eight reads in flight together
        uint32_t c[SLOT_STEPS], sc[SLOT_STEPS];
#pragma unroll
        for (uint32_t h = 0; h < SLOT_STEPS; ++h) {
            const int j = j0 + (int)h;
            const uint32_t jc = (uint32_t)(j < 0 ? 0 : j >= (int)FREE_MAX ? (int)FREE_MAX - 1 : j);
            c[h] = ws.cnt[jc]; sc[h] = ws.sch[jc];
        }
        uint32_t nn = 0u, ns = 0u;
#pragma unroll
        for (uint32_t h = 0; h < SLOT_STEPS; ++h) {
            if (!((mk >> h) & 1u)) c[h] = 0u;
            nn |= (c[h] & 255u) << (8u * h);
            ns |= (sc[h] & 255u) << (8u * h);
        }
        const uint32_t i = (uint32_t)__popcll(present & ((1ull << lane) - 1ull));
        ws.desc[2u * i] = make_uint4((uint32_t)(j0 + 3) | (mk << 8) | (m96_nibble(AW, j0) << 12) | (m96_nibble(EV, j0) << 16), nn, ns,
                                     min(c[0], 0xFFFFu) | (min(c[1], 0xFFFFu) << 16));
        ws.desc[2u * i + 1u] = make_uint4(min(c[2], 0xFFFFu) | (min(c[3], 0xFFFFu) << 16), 0u, 0u, 0u);
    }
    return (uint32_t)__popcll(present);
}

__device__ __forceinline__ void school_counts(const Dev &d, uint32_t s_sch, uint32_t lane, uint32_t n, WaveScratch &ws)
{
    // s_sch: the hash slot of the room's school (k_chunk_marks left it in the room's record): infected in the whole school, per
    // step.  Everybody Infected in a school building counts itself in the slot's per-step counters (k_chunk_marks).
    uint32_t c0 = 0u, c1 = 0u;
    if (s_sch != 0xFFFFFFFFu) {
        if (lane < n) c0 = d.vec[(size_t)s_sch * FREE_MAX + lane];
        if (64u + lane < n) c1 = d.vec[(size_t)s_sch * FREE_MAX + 64u + lane];
    }
    put_school(ws, lane, c0, c1);
}

// Lists with more pairs than this are cut into units that any wavefront can take (k_chunk_units), so that one
// 200-member workplace does not keep a single wavefront busy while the chip idles.
// A deferred unit carries everything its consumer needs, so that it is three dependent loads away from drawing: the
// item's hash slot and its claimer's stretch (the Infected per step), the school's slot for a room, the member list, and
// where in it the unit's first pair falls.
struct UnitSrc { uint32_t slot, link, own; };
__device__ __forceinline__ void list_or_units(const Dev &d, Ctrl *ctrl, const ChunkShared &sm, WaveScratch &ws, const uint32_t *idx,
                                              uint32_t lo, uint32_t hi, const UnitSrc &src, uint32_t lane, uint32_t kind, uint32_t S, uint32_t t0 WORK_ARG,
                                              bool have_pre = false, uint32_t pre_m = 0u, uint32_t pre_w = 0u)
{
    const uint32_t pairs = (hi - lo) * S;
    if (pairs == 0) return;
    if (pairs <= UNIT_INLINE) { member_pairs(d, ctrl, sm, ws, idx, lo, 0u, pairs, lane, kind, S, t0 WORK_PASS, have_pre, pre_m, pre_w); return; }
    const uint32_t n_units = (pairs + UNIT_PAIRS - 1u) / UNIT_PAIRS;
    const uint32_t r = ((blockIdx.x * TPB + threadIdx.x) >> 6) & (SUBQ - 1u);  // this wavefront's queue
    uint32_t start = 0;
    if (lane == 0) start = atomicAdd(&d.hot[(HOT_UNITS + r) * HOT_STRIDE], n_units);
    start = __shfl(start, 0, 64);
    UnitRec *q = d.units + (size_t)r * d.unit_qcap;
    if (start + n_units > d.unit_qcap) {
        // queue full: what was reserved of it becomes no-ops and the list is drawn here
        for (uint32_t i = lane; i < n_units && start + i < d.unit_qcap; i += 64u) q[start + i].code = UNIT_NOOP;
        member_pairs(d, ctrl, sm, ws, idx, lo, 0u, pairs, lane, kind, S, t0 WORK_PASS, have_pre, pre_m, pre_w);
        return;
    }
    for (uint32_t i = lane; i < n_units; i += 64u) {
        const uint32_t p_lo = i * UNIT_PAIRS;
        q[start + i] = UnitRec{ src.slot, kind == 2u ? src.link : 0xFFFFFFFFu, lo, hi - lo, (kind << 30) | p_lo, src.own, p_lo / S, 0u };
    }
}

// What a wavefront needs of item v before it can start on it; depends on v alone, so the fetch of the next item is
// issued before the work on the current one (the pass is bound by chains of dependent loads, not by bandwidth).
// The fetch of an item is one register in two hops: lanes 0..7 its record and lane 17 its hash slot (ITEM_UNUSED: id not
// handed out) by item id; then lanes 8..14 the slot's interval records and lane 16 their number by slot.
struct ItemFetch { uint32_t slot, id, a_lo, a_hi, b_lo, b_hi, aux, link, c0, c1; };
__device__ __forceinline__ uint32_t fetch_item(const Dev &d, uint32_t v, uint32_t lane)
{
    uint32_t x = 0u;
    if (lane < 8u) x = reinterpret_cast<const uint32_t *>(d.item_rec)[(size_t)v * 8u + lane];
    else if (lane == LANE_HSLOT) x = d.hitems[v];
    return x;
}
__device__ __forceinline__ uint32_t fetch_slot(const Dev &d, uint32_t slot, uint32_t lane)
{
    uint32_t x = 0u;
    if (slot < d.hcap) {                                                       // (ITEM_UNUSED, or anything else that is no slot: nothing fetched)
        if (lane >= 8u && lane < 8u + ITEM_RECS) x = d.slot_iv[(size_t)slot * SLOT_IV_STRIDE + (lane - 8u)];
        else if (lane == LANE_STATE) x = d.slot_state[slot];
    }
    return x;
}
__device__ __forceinline__ uint32_t merge_fetch(uint32_t by_id, uint32_t by_slot, uint32_t lane)
{
    return (lane < 8u || lane == LANE_HSLOT) ? by_id : by_slot;
}

// Infected standing in the item in step `lane` (c0) and `64 + lane` (c1) of the chunk: the records of its slot, plus the
// per-step counters of those that found no record free.  (The claimer's own stretch is added by decode_item.)
__device__ __forceinline__ void item_counts(const Dev &d, uint32_t x, uint32_t slot, uint32_t lane, uint32_t n, const M96 &AW,
                                            const M96 &BUS, uint32_t &c0, uint32_t &c1)
{
    const uint32_t state = FX(x, LANE_STATE);
    c0 = 0u; c1 = 0u;
    if (state > ITEM_RECS) {
        // (summed up by k_chunk_fold from the records beyond ITEM_RECS)
        if (lane < n) c0 = d.vec[(size_t)slot * FREE_MAX + lane];
        if (64u + lane < n) c1 = d.vec[(size_t)slot * FREE_MAX + 64u + lane];
    }
    const uint32_t n_rec = state >= SLOT_COUNTERS_ONLY ? 0u : state < ITEM_RECS ? state : ITEM_RECS;
    for (uint32_t k = 0; k < n_rec; ++k) {
        const uint32_t iv = (uint32_t)__builtin_amdgcn_readlane((int)x, (int)(8u + k));
        iv_count(iv, lane, AW, BUS, c0, c1);
    }
}

__device__ __forceinline__ ItemFetch decode_item(const Dev &d, uint32_t x, uint32_t lane, uint32_t n, const M96 &AW, const M96 &BUS)
{
    ItemFetch f;
    f.slot = FX(x, LANE_HSLOT); f.id = FX(x, 0); f.a_lo = FX(x, 1); f.a_hi = FX(x, 2); f.b_lo = FX(x, 3); f.b_hi = FX(x, 4); f.aux = FX(x, 5); f.link = FX(x, 6);
    f.c0 = 0u; f.c1 = 0u;
    if (f.slot < d.hcap) {
        item_counts(d, x, f.slot, lane, n, AW, BUS, f.c0, f.c1);
        iv_count(FX(x, 7), lane, AW, BUS, f.c0, f.c1);
    }
    return f;
}

// What a chunk table says is checked against the capacities before it is used as an index: a table that does not hold what
// k_chunk_marks writes (a diagnostics build that leaves a write out, a defect) ends in ESIM_ERANGE, not in a memory fault.
__device__ __forceinline__ bool item_ok(const Dev &d, const ItemFetch &it)
{
    if (it.slot >= d.hcap) return false;
    if (it.id < d.n_bld) return it.a_lo <= it.a_hi && it.a_hi <= d.n && it.b_lo <= it.b_hi && it.b_hi <= d.n_wrk_idx;
    if (it.id < d.n_bld + d.n_room) return it.a_lo <= it.a_hi && it.a_hi <= d.n_room_idx && (it.link == 0xFFFFFFFFu || it.link < d.hcap);
    return true;
}
#define PAIR_SPREAD 1237u
// apply_exposures (simulator.rs:262-405) for every item and every step of the chunk.
// One (route of <= 64 riders, bus step j) pair with an Infected rider: rank the riders by (Philox key, id) with shuffles, buses
// are runs of bus_capacity ranks, every bus with an Infected rider draws for its Susceptible riders (simulator.rs:362-401).
__device__ __forceinline__ void route_pair_small(const Dev &d, Ctrl *ctrl, const ChunkShared &sm, uint32_t off, uint32_t sz, uint32_t j, uint32_t t0, uint32_t lane WORK_ARG)
{
    const uint64_t seed = ((uint64_t)d.seed_hi << 32) | d.seed_lo;
    const uint32_t s = t0 + j, mask = sm.dec[j].mask;
    uint32_t c = 0, w = 0, key = 0;
    bool inf = false;
    WORK_ADD(WK_ROUTE_PAIRS, lane == 0 ? 1 : 0); WORK_ADD(WK_RIDERS, lane < sz ? 1 : 0);
    bool can = false;                                                          // could take a draw on this bus step at all
    if (lane < sz) {
        c = d.route_riders[off + lane];
        w = d.cit[c];
        inf = status_in_chunk(d, w, t0, j) == ESIM_INFECTED;
        can = rider_can(w, s, j);
    }
    // Nobody Infected aboard, or nobody who could still be exposed: no draw is made, whatever the buses (the order of the riders
    // is only needed to tell who shares a bus with whom).  A route that fills one bus at most needs no order either.
    if (!__any(inf) || !__any(can)) return;
    const uint32_t cap = d.bus_capacity;
    uint32_t rank = 0;
    if (sz > cap) {
        if (lane < sz) key = philox4x32_10(d.id_base + c, s, ESIM_SLOT_BUS_ORDER, 0u, d.seed_lo, d.seed_hi).w0;
        rank = rank_wave64(key, lane, sz);
    }
    // The bus of a rank, and the buses of the route.  At most 64 riders in buses of 16 or more are four buses at most: the bus is
    // the number of b >= 1 with rank >= b * cap, no division (the hardware has no scalar one: a uniform divisor costs the same
    // 14 vector instructions as any).  Smaller buses divide.
    uint32_t bus, n_bus;
    if (cap >= 16u) {
        bus = (rank >= cap ? 1u : 0u) + (rank >= 2u * cap ? 1u : 0u) + (rank >= 3u * cap ? 1u : 0u);
        n_bus = 1u + (sz > cap ? 1u : 0u) + (sz > 2u * cap ? 1u : 0u) + (sz > 3u * cap ? 1u : 0u);
    } else {
        bus = rank / cap;
        n_bus = (sz + cap - 1u) / cap;
    }
    // Infected riders on my bus: one ballot per bus of the route
    const unsigned long long inf_m = __ballot(inf);
    uint32_t k = 0;
    for (uint32_t b = 0; b < n_bus; ++b) {
        const unsigned long long on_b = __ballot(lane < sz && bus == b);
        if (bus == b) k = (uint32_t)__popcll(on_b & inf_m);
    }
    if (lane < sz && k && can) {                                               // not exposed before this bus, not Vaccinated by then
        const uint32_t row = (!(w & FL_MASK_COMPLIANT) && mask == ESIM_MASK_EVERYWHERE) ? 1u : 0u;
        WORK_ADD(WK_BUS_DRAWS, 1);
        if (esim_u32(seed, d.id_base + c, s, ESIM_SLOT_BUS) < sm.thr[row * 256u + (k & 255u)]) { WORK_ADD(WK_HITS, 1); expose_min(d, ctrl, c, w, s, CW_BUS_EXPOSED); }
    }
}
// One (route of more than 64 riders, bus step) pair, by a whole workgroup of NT threads: ranks through LDS (simulator.rs:362-401).
template <uint32_t NT>
__device__ __forceinline__ void route_pair_big(const Dev &d, Ctrl *ctrl, const ChunkShared &sm, RouteShared &rs, uint32_t code, uint32_t t0, uint32_t n WORK_ARG)
{
    const uint64_t seed = ((uint64_t)d.seed_hi << 32) | d.seed_lo;
    const uint32_t r = code >> 7, j = code & 127u;
    if (r >= d.n_routes || j >= n) { if (threadIdx.x == 0) ctrl->error = (uint32_t)(-ESIM_ERANGE); return; }   // (block-uniform)
    const uint32_t off = d.route_off[r], sz = d.route_off[r + 1] - off;
    if (sz > CHUNK_ROUTE_MAX) { if (threadIdx.x == 0) ctrl->error = (uint32_t)(-ESIM_ERANGE); return; }
    const uint32_t s = t0 + j, mask = sm.dec[j].mask;
    WORK_ADD(WK_ROUTE_PAIRS, threadIdx.x == 0 ? 1 : 0);
    int loc_inf = 0, loc_can = 0;
    for (uint32_t i = threadIdx.x; i < sz; i += NT) {
        const uint32_t c = d.route_riders[off + i];
        WORK_ADD(WK_RIDERS, 1);
        const uint32_t w = d.cit[c];
        rs.s_inf[i] = status_in_chunk(d, w, t0, j) == ESIM_INFECTED ? 1 : 0;
        loc_inf |= rs.s_inf[i];
        loc_can |= rider_can(w, s, j) ? 1 : 0;
    }
    // (nobody Infected aboard, or nobody who could still be exposed: no draw is made, whatever the order of the riders)
    const int any_inf = __syncthreads_or(loc_inf), any_can = __syncthreads_or(loc_can);
    if (!any_inf || !any_can) return;
    for (uint32_t i = threadIdx.x; i < sz; i += NT)
        rs.s_key[i] = philox4x32_10(d.id_base + d.route_riders[off + i], s, ESIM_SLOT_BUS_ORDER, 0u, d.seed_lo, d.seed_hi).w0;
    for (uint32_t i = threadIdx.x; i < sz / d.bus_capacity + 1u; i += NT) rs.s_cnt[i] = 0u;
    for (uint32_t i = threadIdx.x; i < (sz + 31u) / 32u; i += NT) rs.s_seen[i] = 0u;
    __syncthreads();
    // ranks by key alone, and a look whether two riders were given the same one (they shared a key: about once in 10^7 pairs)
    int tie = 0;
    for (uint32_t i = threadIdx.x; i < sz; i += NT) {
        const uint32_t rank = rank_block(rs.s_key, rs.s_key[i], sz);
        tie |= rank_seen(rs.s_seen, rank) ? 1 : 0;
        const uint32_t bus = rank / d.bus_capacity;
        rs.s_bus[i] = (uint16_t)bus;
        if (rs.s_inf[i]) atomicAdd(&rs.s_cnt[bus], 1u);
    }
    if (__syncthreads_or(tie)) {
        // ... then once more, by (key, index)
        for (uint32_t i = threadIdx.x; i < sz / d.bus_capacity + 1u; i += NT) rs.s_cnt[i] = 0u;
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < sz; i += NT) {
            const uint32_t bus = rank_block_exact(rs.s_key, rs.s_key[i], i, sz) / d.bus_capacity;
            rs.s_bus[i] = (uint16_t)bus;
            if (rs.s_inf[i]) atomicAdd(&rs.s_cnt[bus], 1u);
        }
        __syncthreads();
    }
    for (uint32_t i = threadIdx.x; i < sz; i += NT) {
        const uint32_t k = rs.s_cnt[rs.s_bus[i]];
        if (!k) continue;
        const uint32_t c = d.route_riders[off + i];
        const uint32_t w = d.cit[c];
        if (!rider_can(w, s, j)) continue;                                     // exposed before this bus, or Vaccinated by then
        const uint32_t row = (!(w & FL_MASK_COMPLIANT) && mask == ESIM_MASK_EVERYWHERE) ? 1u : 0u;
        WORK_ADD(WK_BUS_DRAWS, 1);
        if (esim_u32(seed, d.id_base + c, s, ESIM_SLOT_BUS) < sm.thr[row * 256u + (k & 255u)]) { WORK_ADD(WK_HITS, 1); expose_min(d, ctrl, c, w, s, CW_BUS_EXPOSED); }
    }
    __syncthreads();
}

__global__ __launch_bounds__(TPB) void k_chunk_draw(Dev d, uint32_t n_mw)
{
    __shared__ ChunkShared sm;
    __shared__ WaveScratch wsc[TPB / 64];
    Ctrl *ctrl = d.ctrl;
    const uint32_t t0 = ctrl->chunk_t0, n = ctrl->chunk_ok;
    if (!ctrl->chunk_parallel || n == 0u) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (blockIdx.x * TPB + threadIdx.x) >> 6, n_waves = (gridDim.x * TPB) >> 6;   // <= CHUNK_WAVES_MAX (esim_create)
    const uint32_t pt0 = PROF_NOW();
    WORK_TALLY;
    uint32_t p_items = 0u, p_item_max = 0u;
    // The wavefronts of k_chunk_marks (same grid) each handed out the first used_cnt[w] ids of [w * per_wave, ...): whoever
    // reaches a key first claims its item, so the early wavefronts hold far more items than the late ones.  The pass
    // therefore takes the items in id order as ONE dense sequence and every wavefront draws an equal stretch of it
    // (k_chunk_fold left the prefix sums of used_cnt in used_pref).
    // n_mw = wavefronts of k_chunk_marks (whose id ranges the items sit in); this kernel's own grid is a multiple of that:
    // equal stretches are equal in ITEMS, not in work -- 20 to 40 items per wavefront with member lists of 2 to 200, then the
    // wavefront's share of the routes: in round 2 the slowest of 4096 wavefronts ran 1.4x (items) and 2x (routes) the median,
    // and 2.8 of the 4 wavefronts a SIMD had been given were resident on average.  Taking blocks from shared counters does
    // not help at 20 items per wavefront (measured: +-0); what does is MORE, SHORTER wavefronts than the chip holds at once
    // (ESIM_DRAW_MULT x the marks grid): the dispatcher starts the next workgroup where one has finished.
    const uint32_t per_wave = ld(&ctrl->items_per_wave);
    if ((unsigned long long)per_wave * n_mw > d.items_cap || n_waves % n_mw != 0u) return;   // (k_chunk_marks raised ESIM_ERANGE and left no items)
    const uint32_t G = n_waves / n_mw;
    const uint32_t T = d.used_pref[n_mw];
    const uint32_t coarse = d.used_pref[min(64u * lane, n_mw)];
    const uint32_t Tq = T / n_waves, Tr = T % n_waves;                         // (T * wave / n_waves without 64-bit division)
    const uint32_t d_lo = Tq * wave + (uint32_t)(((unsigned long long)Tr * wave) / n_waves), d_hi = Tq * (wave + 1u) + (uint32_t)(((unsigned long long)Tr * (wave + 1u)) / n_waves);
    // the wavefront of k_chunk_marks that owns dense index i: the last one whose ids start at or before it -- first among
    // every 64th (`coarse`), then among the 64 from there on (`win`: lane l holds where the ids of owner ow_base + l start; a
    // window of 64 owners, moved on when used up)
    uint32_t ow_base = 0u, win = 0u, ow = 0u;
    auto seek = [&](uint32_t i) {
        ow_base = 64u * ((uint32_t)__popcll(__ballot(64u * lane < n_mw && coarse <= i)) - 1u);
        win = d.used_pref[min(ow_base + lane, n_mw)];
        ow = ow_base + (uint32_t)__popcll(__ballot(ow_base + lane < n_mw && win <= i)) - 1u;
    };
    seek(d_lo);
    // item id of dense index i; called with ascending i
    auto id_of = [&](uint32_t i) -> uint32_t {
        for (;;) {
            const uint32_t rel = ow - ow_base;
            if (rel == 63u) { ow_base = ow; win = d.used_pref[min(ow_base + lane, n_mw)]; continue; }
            if (ow + 1u < n_mw && (uint32_t)__builtin_amdgcn_readlane((int)win, (int)(rel + 1u)) <= i) { ++ow; continue; }
            return ow * per_wave + (i - (uint32_t)__builtin_amdgcn_readlane((int)win, (int)rel));
        }
    };
    // three items in flight: the record of the one after next (by id), the slot records of the next (by its slot), this one
    uint32_t id_cur = 0u, id_nxt = 0u, sl_cur = 0u;
    if (d_lo < d_hi) id_cur = fetch_item(d, id_of(d_lo), lane);
    if (d_lo + 1u < d_hi) id_nxt = fetch_item(d, id_of(d_lo + 1u), lane);
    // ... and the first look at the (route, bus step) pairs dealt to this wavefront (phase 2 below), so that they are here
    // when the items are done
    // Wavefront w of k_chunk_marks left pair_cnt[w] pairs in its own stretch of K places.  Its k-th pair goes to the wavefront
    // of this kernel with number ((w + k * PAIR_SPREAD) mod n_mw) + n_mw * (k mod G): lane l of wavefront (base, r) looks at
    // k = l * G + r of the stretch it may have been dealt from.
    const uint32_t K = PAIR_K(per_wave, ld(&ctrl->chunk_bus));                 // pairs a stretch of the list can hold
    const uint32_t w_base = wave % n_mw, w_rep = wave / n_mw;
    uint32_t code_l = 0u, off_l = 0u, sz_l = 0u; bool have = false;
    // this lane's pair of the 64 from place k0 on (have: it exists), then where its route's riders are
    auto deal = [&](uint32_t k0) {
        const uint32_t k = (k0 + lane) * G + w_rep;
        have = false;
        if (k < K) {
            const uint32_t src = (w_base + n_mw - (uint32_t)(((unsigned long long)k * PAIR_SPREAD) % n_mw)) % n_mw;
            code_l = d.route_pairs[(size_t)src * K + k];                      // in bounds whether or not the pair exists
            have = k < d.pair_cnt[src] && (code_l >> 7) < d.n_routes && (code_l & 127u) < n;
        }
    };
    auto deal_riders = [&]() { if (have) { const uint32_t r = code_l >> 7; off_l = d.route_off[r]; sz_l = d.route_off[r + 1] - off_l; } };
    deal(0u);
    stage_chunk(d, sm, n, TPB);
    __syncthreads();
    const uint32_t route_base = d.n_bld + d.n_room;
    WaveScratch &ws = wsc[threadIdx.x >> 6];
    const auto [AW, BUS, EV] = chunk_masks(sm.dec, lane, n);
    if (d_lo < d_hi) sl_cur = fetch_slot(d, FX(id_cur, LANE_HSLOT), lane);
    deal_riders();
#ifdef ESIM_WAVE_PROFILE
    if (lane == 0) ws.rounds = 0u;
#endif
    uint32_t pst[5] = { 0u, 0u, 0u, 0u, 0u };
    const uint32_t pt1 = PROF_NOW();
    // (1) buildings and school rooms: one wavefront per item
    for (uint32_t v = d_lo; v < d_hi; ++v) {
        const uint32_t x = merge_fetch(id_cur, sl_cur, lane);
        id_cur = id_nxt;
        if (v + 2u < d_hi) id_nxt = fetch_item(d, id_of(v + 2u), lane);
        if (v + 1u < d_hi) sl_cur = fetch_slot(d, FX(id_cur, LANE_HSLOT), lane);
        const uint32_t pq0 = PROF_NOW();
        const ItemFetch it = decode_item(d, x, lane, n, AW, BUS);
        if (it.slot == ITEM_UNUSED) continue;
        if (!item_ok(d, it)) { if (lane == 0) RAISE(ctrl, ESIM_ERANGE, ERR_AT_ITEM_CHECK); continue; }
        if (it.id >= route_base) continue;
        const uint32_t pi0 = PROF_NOW();
        pst[0] += pi0 - pq0;
        (void)pi0; ++p_items; WORK_ADD(WK_ITEMS, lane == 0 ? 1 : 0);
        if (it.id < d.n_bld) {
            if (it.aux == ESIM_SCHOOL) continue;                              // School::find_exposures works per room
            // first 64 residents and workers and their words: both lists' loads are in flight together
            const uint32_t n_res = it.a_hi - it.a_lo, n_wrk = it.b_hi - it.b_lo;
            uint32_t rm = 0u, wm = 0u, rw = 0u, ww = 0u;
            if (lane < n_res) rm = d.res_idx ? d.res_idx[it.a_lo + lane] : it.a_lo + lane;
            if (lane < n_wrk) wm = d.wrk_idx[it.b_lo + lane];
            if (lane < n_res) rw = d.cit[rm];
            if (lane < n_wrk) ww = d.cit[wm];
            const uint32_t pq1 = PROF_NOW();
            const uint32_t S = item_steps_regs(it.c0, it.c1, lane, ws, t0, AW, EV);
            __builtin_amdgcn_wave_barrier();
            const uint32_t pq2 = PROF_NOW();
            // Household / Workplace::find_exposures: every registered occupant (building.rs:202-204,278-280)
            const UnitSrc src = { it.slot, it.link, FX(x, 7) };
            list_or_units(d, ctrl, sm, ws, d.res_idx, it.a_lo, it.a_hi, src, lane, 0u, S, t0 WORK_PASS, true, rm, rw);
            const uint32_t pq3 = PROF_NOW();
            list_or_units(d, ctrl, sm, ws, d.wrk_idx, it.b_lo, it.b_hi, src, lane, 1u, S, t0 WORK_PASS, true, wm, ww);
            const uint32_t pq4 = PROF_NOW();
            pst[1] += pq1 - pi0; pst[2] += pq2 - pq1; pst[3] += pq3 - pq2; pst[4] += pq4 - pq3;
        } else {
            const uint32_t n_mem = it.a_hi - it.a_lo;
            uint32_t mm = 0u, mw = 0u;
            if (lane < n_mem) mm = d.room_idx[it.a_lo + lane];
            school_counts(d, it.link, lane, n, ws);
            if (lane < n_mem) mw = d.cit[mm];
            const uint32_t S = item_steps_regs(it.c0, it.c1, lane, ws, t0, AW, EV);
            __builtin_amdgcn_wave_barrier();
            // School::find_exposures: the room once per infected in it (building.rs:494-522)
            const UnitSrc src = { it.slot, it.link, FX(x, 7) };
            list_or_units(d, ctrl, sm, ws, d.room_idx, it.a_lo, it.a_hi, src, lane, 2u, S, t0 WORK_PASS, true, mm, mw);
        }
        __builtin_amdgcn_wave_barrier();
        { const uint32_t dt = PROF_NOW() - pi0; p_item_max = dt > p_item_max ? dt : p_item_max; }
    }
    const uint32_t pt2 = PROF_NOW();
    // (2) routes of <= 64 riders: one wavefront per (route, bus step) with an Infected rider (the pairs dealt to this wavefront --
    // see the first look above --, taken one by one)
    for (uint32_t k0 = 0; k0 * G < K; k0 += 64u) {
        if (k0) { deal(k0); deal_riders(); }                                  // (beyond the 64 looked at up front: many Infected)
        unsigned long long todo = __ballot(have);
        while (todo) {
            const int src_lane = __ffsll((long long)todo) - 1;
            todo &= todo - 1ull;
            const uint32_t code = __shfl(code_l, src_lane, 64), off = __shfl(off_l, src_lane, 64), sz = __shfl(sz_l, src_lane, 64);
            route_pair_small(d, ctrl, sm, off, sz, code & 127u, t0, lane WORK_PASS);
        }
    }
    WORK_FLUSH(d);
    const uint32_t pt3 = PROF_NOW();
#ifndef ESIM_PROFILE_UNITS
    PROF_PUT(d, 0, pt0); PROF_PUT(d, 1, pt1); PROF_PUT(d, 2, pt2); PROF_PUT(d, 3, pt3);   // start, after preamble, after items, end
    PROF_PUT(d, 4, p_items); PROF_PUT(d, 5, p_item_max); PROF_PUT(d, 6, wsc[threadIdx.x >> 6].rounds);
    PROF_PUT(d, 11, pst[0]); PROF_PUT(d, 12, pst[1]); PROF_PUT(d, 13, pst[2]); PROF_PUT(d, 14, pst[3]); PROF_PUT(d, 15, pst[4]);
#endif
    (void)pst;
    (void)pt0; (void)pt1; (void)pt2; (void)pt3; (void)p_items; (void)p_item_max;
}

// The deferred units of long member lists, dealt to the wavefronts round-robin.
// Then the routes of more than 64 riders: one workgroup per (route, bus step), ranks through LDS.
__global__ __launch_bounds__(TPB) void k_chunk_units(Dev d)
{
    __shared__ ChunkShared sm;
    __shared__ WaveScratch wsc[TPB / 64];
    __shared__ RouteShared rs;
    Ctrl *ctrl = d.ctrl;
    const uint32_t t0 = ctrl->chunk_t0, n = ctrl->chunk_ok;
    if (!ctrl->chunk_parallel || n == 0u) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (blockIdx.x * TPB + threadIdx.x) >> 6, n_waves = (gridDim.x * TPB) >> 6;
    const uint32_t pu0 = PROF_NOW();
    WORK_TALLY;
    uint32_t pu_n = 0u, pu_max = 0u, pu_it = 0u;
    // queue `wave & 63`, every (n_waves / 64)-th unit of it
    const uint32_t qr = wave & (SUBQ - 1u), first = wave / SUBQ, step = n_waves / SUBQ;
    const uint32_t n_units = step ? min(ld(&d.hot[(HOT_UNITS + qr) * HOT_STRIDE]), d.unit_qcap) : 0u;
    const uint32_t n_pairs = min(ld(&d.hot[HOT_BIGPAIRS * HOT_STRIDE]), d.big_pairs_cap);
    if (__syncthreads_or(first < n_units) == 0 && n_pairs == 0u) return;
    stage_chunk(d, sm, n, TPB);
    __syncthreads();
    WaveScratch &ws = wsc[threadIdx.x >> 6];
    const uint32_t *q_words = reinterpret_cast<const uint32_t *>(d.units + (size_t)qr * d.unit_qcap);
    const auto [AW, BUS, EV] = chunk_masks(sm.dec, lane, n);
    // Per unit: its record (lanes 0..7 of one register); then, together, the slot's interval records, the school's, and the
    // ids of the first members its pairs touch; then those members' words.  The record of the unit after next and the
    // second stage of the next are in flight while this one draws.
    // (unit records are written by k_chunk_draw from items it has checked (item_ok), into queues that are initialised to
    // no-ops; what a record names as hash slots is checked by fetch_slot, which fetches nothing for a value that is no slot)
    auto unit_words = [&](uint32_t q) -> uint32_t { return lane < 8u ? q_words[(size_t)q * 8u + lane] : 0u; };
    auto member_id = [&](uint32_t u) -> uint32_t {
        const uint32_t code = FX(u, 4), kind = code >> 30, lo = FX(u, 2), n_mem = FX(u, 3), mf = FX(u, 6);
        if (code == UNIT_NOOP || mf + lane >= n_mem) return 0u;
        const uint32_t *idx = kind == 2u ? d.room_idx : kind == 1u ? d.wrk_idx : d.res_idx;
        return idx ? idx[lo + mf + lane] : lo + mf + lane;
    };
    const uint32_t pu1 = PROF_NOW();
    uint32_t u_0 = 0xFFFFFFFFu, u_1 = 0xFFFFFFFFu;                            // this unit, the next (code word UNIT_NOOP: none)
    uint32_t xs_0 = 0u, ys_0 = 0u, mid_0 = 0u;
    if (first < n_units) u_0 = unit_words(first);
    if (first + step < n_units) u_1 = unit_words(first + step);
    if (first < n_units && FX(u_0, 4) != UNIT_NOOP) { xs_0 = fetch_slot(d, FX(u_0, 0), lane); ys_0 = fetch_slot(d, FX(u_0, 1), lane); mid_0 = member_id(u_0); }
    for (uint32_t q = first; q < n_units; q += step) {
        const uint32_t u = u_0, xs = xs_0, ys = ys_0, mid = mid_0;
        u_0 = u_1;
        u_1 = 0xFFFFFFFFu;
        if (q + 2u * step < n_units) u_1 = unit_words(q + 2u * step);
        if (q + step < n_units && FX(u_0, 4) != UNIT_NOOP) { xs_0 = fetch_slot(d, FX(u_0, 0), lane); ys_0 = fetch_slot(d, FX(u_0, 1), lane); mid_0 = member_id(u_0); }
        const uint32_t code = FX(u, 4);
        if (code == UNIT_NOOP) continue;
        const uint32_t pui = PROF_NOW();
        ++pu_n;
        const uint32_t kind = code >> 30, p_lo = code & 0x3FFFFFFFu, slot = FX(u, 0), link = FX(u, 1), lo = FX(u, 2), n_mem = FX(u, 3), own = FX(u, 5), mf = FX(u, 6);
        const uint32_t mw = (mf + lane < n_mem) ? d.cit[mid] : 0u;
        uint32_t c0, c1;
        item_counts(d, xs, slot, lane, n, AW, BUS, c0, c1);
        iv_count(own, lane, AW, BUS, c0, c1);
        if (kind == 2u) {
            uint32_t s0 = 0u, s1 = 0u;
            if (link != 0xFFFFFFFFu) item_counts(d, ys, link, lane, n, AW, BUS, s0, s1);
            put_school(ws, lane, s0, s1);
        }
        const uint32_t *idx = kind == 2u ? d.room_idx : kind == 1u ? d.wrk_idx : d.res_idx;
        const uint32_t S = item_steps_regs(c0, c1, lane, ws, t0, AW, EV);
        __builtin_amdgcn_wave_barrier();
        const uint32_t pairs = n_mem * S;
        WORK_ADD(WK_UNITS, lane == 0 ? 1 : 0);
        member_pairs(d, ctrl, sm, ws, idx, lo, p_lo, min(pairs, p_lo + UNIT_PAIRS), lane, kind, S, t0 WORK_PASS, true, mid, mw, mf);
        __builtin_amdgcn_wave_barrier();
        { const uint32_t dt = PROF_NOW() - pui; pu_max = dt > pu_max ? dt : pu_max; pu_it += (min(pairs, p_lo + UNIT_PAIRS) - p_lo + 63u) / 64u; }
    }
    const uint32_t pu2 = PROF_NOW();
    WORK_FLUSH(d);
#ifdef ESIM_PROFILE_UNITS
    PROF_PUT(d, 0, pu0); PROF_PUT(d, 1, pu1); PROF_PUT(d, 2, pu2); PROF_PUT(d, 4, pu_n); PROF_PUT(d, 5, pu_max); PROF_PUT(d, 7, pu_it);
#endif
    (void)pu0; (void)pu1; (void)pu2; (void)pu_n; (void)pu_max; (void)pu_it;
    for (uint32_t q = blockIdx.x; q < n_pairs; q += gridDim.x) route_pair_big<TPB>(d, ctrl, sm, rs, d.route_pairs_big[q], t0, n WORK_PASS);
    WORK_FLUSH(d);
}
