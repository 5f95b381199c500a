// esim_chunk_sets.h -- what every form of a chunk shares and no kernel owns: sets of steps (M96), the interval record of an Infected
// citizen (IV_*), the chunk's schedule as step masks, a citizen's DiseaseStatus and place in a step and over its Infected stretch.
#pragma once
#include "esim_kernels_common.h"
// An interval record: a citizen that is Infected in steps [a, b] of the chunk, the flags that decide where it stands
// in each of them, and whether the record sits in its work building / room or in its home.
#define IV_VALID   0x80000000u
#define IV_PT      (1u << 14)
#define IV_HW      (1u << 15)
#define IV_AS_WORK (1u << 16)
__device__ __forceinline__ uint32_t iv_present(uint32_t iv, uint32_t j, const Decision &q)
{
    if (!(iv & IV_VALID) || j < (iv & 127u) || j > ((iv >> 7) & 127u)) return 0u;
    if (q.bus_dir && (iv & IV_PT)) return 0u;                                 // on a bus (simulator.rs:181-186)
    const bool at_work = q.at_work && (iv & IV_HW);
    return ((iv & IV_AS_WORK) != 0u) == at_work ? 1u : 0u;
}

// DiseaseStatus of a citizen in step t0 + j of a chunk: a vaccination planned for the end of step f of the chunk
// (k_chunk_vax) makes it Vaccinated from step f + 1 on, whatever it was (simulator.rs:551).
__device__ __forceinline__ uint32_t status_in_chunk(const Dev &d, uint32_t w, uint32_t t0, uint32_t j)
{
    const uint32_t f = CW_VAX_REL(w);
    if (f != CW_VAX_NONE && j > f) return ESIM_VACCINATED;
    return status_of(CW_TE(w), t0 + j, d.exposed_time, d.infected_time);
}

// Where an Infected citizen stands in step t0 + j of the chunk (simulator.rs:181-198): bit 0 in the home building,
// bit 1 in the work building, bit 2 on the bus.  0 when not Infected in that step.
__device__ __forceinline__ uint32_t where_in_step(const Dev &d, uint32_t w, uint32_t t0, uint32_t j, const Decision &q)
{
    if (status_in_chunk(d, w, t0, j) != ESIM_INFECTED) return 0u;
    if (q.bus_dir && (w & FL_USES_PT)) return 4u;
    return (q.at_work && (w & FL_HAS_WORK)) ? 2u : 1u;
}

#define FX(x, i) ((uint32_t)__builtin_amdgcn_readlane((int)(x), (int)(i)))
// A set of steps of a chunk (FREE_MAX = 96 bits).
struct M96 { unsigned long long lo; uint32_t hi; };
__device__ __forceinline__ M96 m96_and(M96 a, M96 b) { return M96{ a.lo & b.lo, a.hi & b.hi }; }
__device__ __forceinline__ M96 m96_andn(M96 a, M96 b) { return M96{ a.lo & ~b.lo, a.hi & ~b.hi }; }
__device__ __forceinline__ bool m96_any(M96 a) { return a.lo != 0ull || a.hi != 0u; }
// steps a..b (a <= b < 96)
__device__ __forceinline__ M96 m96_range(uint32_t a, uint32_t b)
{
    M96 r = { 0ull, 0u };
    if (a < 64u) { const uint32_t e = min(b, 63u); r.lo = (e == 63u ? ~0ull : ((1ull << (e + 1u)) - 1ull)) & (~0ull << a); }
    if (b >= 64u) { const uint32_t s0 = a > 64u ? a - 64u : 0u, e = min(b - 64u, 31u); r.hi = (e == 31u ? ~0u : ((1u << (e + 1u)) - 1u)) & (~0u << s0); }
    return r;
}

// The steps of the chunk in which the citizen of interval record iv stands where the record was left (iv_present as a set):
// AW / BUS = the steps in which those with a work place are at work / riders are on a bus.  With a wavefront-uniform record
// this is scalar arithmetic; a lane then only picks its step's bit.
__device__ __forceinline__ M96 iv_steps(uint32_t iv, const M96 &AW, const M96 &BUS)
{
    if (!(iv & IV_VALID)) return M96{ 0ull, 0u };
    const M96 I = m96_range(iv & 127u, (iv >> 7) & 127u);
    const M96 rest = (iv & IV_PT) ? m96_andn(I, BUS) : I;
    const M96 atw = (iv & IV_HW) ? m96_and(rest, AW) : M96{ 0ull, 0u };
    return (iv & IV_AS_WORK) ? atw : m96_andn(rest, atw);
}
__device__ __forceinline__ void iv_count(uint32_t iv, uint32_t lane, const M96 &AW, const M96 &BUS, uint32_t &c0, uint32_t &c1)
{
    const M96 at = iv_steps(iv, AW, BUS);
    c0 += (uint32_t)(at.lo >> lane) & 1u;
    c1 += lane < 32u ? (at.hi >> lane) & 1u : 0u;
}
// The chunk's schedule as step masks (wavefront-uniform; all 64 lanes call): the steps in which those with a work place are at
// work (AW), riders are on a bus (BUS) and masks are worn everywhere (EV).  dec: the chunk's decisions, n of them.
struct ChunkMasks { M96 AW, BUS, EV; };
__device__ __forceinline__ ChunkMasks chunk_masks(const Decision *dec, uint32_t lane, uint32_t n)
{
    const Decision q0 = lane < n ? dec[lane] : Decision{ 0u, 0u, 0u, 0u };
    const Decision q1 = 64u + lane < n ? dec[64u + lane] : Decision{ 0u, 0u, 0u, 0u };
    return ChunkMasks{ M96{ __ballot(lane < n && q0.at_work != 0u), (uint32_t)__ballot(64u + lane < n && q1.at_work != 0u) },
                       M96{ __ballot(lane < n && q0.bus_dir != 0u), (uint32_t)__ballot(64u + lane < n && q1.bus_dir != 0u) },
                       M96{ __ballot(lane < n && q0.mask == ESIM_MASK_EVERYWHERE), (uint32_t)__ballot(64u + lane < n && q1.mask == ESIM_MASK_EVERYWHERE) } };
}

// (four bits of a set of steps from step p on; p may be up to three steps before the chunk)
__device__ __forceinline__ uint32_t m96_nibble(const M96 &m, int p)
{
    if (p < 0) return (uint32_t)(m.lo << (-p)) & 15u;
    if (p >= 64) return p >= 96 ? 0u : (m.hi >> (p - 64)) & 15u;
    return (uint32_t)((m.lo >> p) | (p > 60 ? (unsigned long long)m.hi << (64 - p) : 0ull)) & 15u;
}

// The stretch rule.  The citizen of word w is Infected in steps [iv_a, iv_b] of the chunk of n steps from t0 (one stretch:
// disease.rs:60-65), Vaccinated after the step its plan names (k_chunk_vax); where it stands in each of them (simulator.rs:181-198)
// follows from its flags and the schedule.  act: Infected in some step (never for a lane without a citizen: !live); else the sets are empty.
struct Stretch { M96 home, work, bus; uint32_t iv_a, iv_b; bool act; };
__device__ __forceinline__ Stretch infected_stretch(const Dev &d, uint32_t w, uint32_t t0, uint32_t n, const M96 &AW, const M96 &BUS, bool live = true)
{
    Stretch s;
    const int a_abs = (int)CW_TE(w) - (int)TE_BIAS + (int)d.exposed_time + 1;
    const int b_rel = a_abs + (int)d.infected_time - (int)t0;
    s.iv_a = a_abs > (int)t0 ? (uint32_t)(a_abs - (int)t0) : 0u;
    s.iv_b = b_rel < 0 ? 0u : min(min((uint32_t)b_rel, n - 1u), CW_VAX_REL(w));   // (CW_VAX_NONE is the largest value)
    s.act = live && !(CW_TE(w) >= TE_RECOVERED || b_rel < 0 || s.iv_a > s.iv_b);
    M96 I = m96_range(s.iv_a, s.iv_b);
    if (!s.act) I = M96{ 0ull, 0u };
    s.bus = (w & FL_USES_PT) ? m96_and(I, BUS) : M96{ 0ull, 0u };
    const M96 rest = m96_andn(I, s.bus);
    s.work = (w & FL_HAS_WORK) ? m96_and(rest, AW) : M96{ 0ull, 0u };
    s.home = m96_andn(rest, s.work);
    return s;
}
// The interval record of the stretch as left in the citizen's home (| IV_AS_WORK: in its work building / room).
__device__ __forceinline__ uint32_t stretch_record(const Stretch &s, uint32_t w)
{
    return IV_VALID | s.iv_a | (s.iv_b << 7) | ((w & FL_USES_PT) ? IV_PT : 0u) | ((w & FL_HAS_WORK) ? IV_HW : 0u);
}

// Can the rider of word w still be exposed on the bus of step s = t0 + j of the chunk: not exposed before this bus, neither
// Recovered nor Vaccinated, and not Vaccinated by then (k_chunk_vax).
__device__ __forceinline__ bool rider_can(uint32_t w, uint32_t s, uint32_t j)
{
    const uint32_t te = CW_TE(w);
    return !(w <= CW_MAKE(s + TE_BIAS, CW_BUS_EXPOSED | (w & CW_KEEP)) || (te >= TE_RECOVERED && te != TE_SUSCEPTIBLE) || j > CW_VAX_REL(w));
}
