"""The step sets of esim_chunk_sets.h on their own (tests/native/sets_probe.hip includes esim_kernels_common.h and that header only),
against numpy written from the rule: a step j is in a set iff the per-step predicate holds for j.  Exact equality, no tolerance.
The shapes are the smallest at which the 64-bit / 32-bit seam of M96, the p < 0 and p > 60 branches of m96_nibble and a chunk of
exactly one or exactly 96 steps can go wrong.  The probe is compiled here, as test_rank_gpu.py compiles its own."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FREE_MAX = 96
# the citizen word (esim_device.h) and the interval record (esim_chunk_sets.h)
TE_SHIFT, TE_BIAS = 19, 512
TE_SUSCEPTIBLE, TE_VACCINATED, TE_RECOVERED = 0x1FFF, 0x1FFE, 0x1FFD
VAX_SHIFT = 11
FL_USES_PT, FL_HAS_WORK = 0x01, 0x10
IV_VALID, IV_PT, IV_HW, IV_AS_WORK = 0x80000000, 1 << 14, 1 << 15, 1 << 16
MASK_EVERYWHERE = 2
N_CHUNK = (1, 63, 64, 65, 96)
T0 = 1000
STRETCH_OUT = 22


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("sets_probe") / "libsets_probe.so")
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
           "-I", os.path.join(ROOT, "epidemicsimulator_amd", "csrc"), "-o", out, os.path.join(ROOT, "tests", "native", "sets_probe.hip")]
    done = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stderr[-2000:]
    lib = ctypes.CDLL(out)
    for name in ("sets_probe_range", "sets_probe_nibble", "sets_probe_iv", "sets_probe_stretch"):
        getattr(lib, name).restype = ctypes.c_int
    return lib


def ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


def bits(words3):
    """three words (bits 0-31, 32-63, 64-95) -> the set as a Python int"""
    return int(words3[0]) | (int(words3[1]) << 32) | (int(words3[2]) << 64)


def set_of(pred):
    """{j < 96 : pred[j]} as a Python int"""
    return sum(1 << j for j in range(FREE_MAX) if pred[j])


def schedules(n):
    """name -> (at_work, bus_dir, mask) per step, zero behind the chunk's n steps"""
    rng = np.random.default_rng(7000 + n)
    j = np.arange(FREE_MAX)
    out = {"zero": (np.zeros(FREE_MAX, np.uint32), np.zeros(FREE_MAX, np.uint32), np.zeros(FREE_MAX, np.uint32)),
           "alternating": ((j & 1).astype(np.uint32), ((j >> 1) & 1).astype(np.uint32) * 2, (j % 3).astype(np.uint32)),
           "random": (rng.integers(0, 2, FREE_MAX).astype(np.uint32), rng.integers(0, 3, FREE_MAX).astype(np.uint32),
                      rng.integers(0, 3, FREE_MAX).astype(np.uint32))}
    for aw, bus, mask in out.values():
        aw[n:] = 0; bus[n:] = 0; mask[n:] = 0
    return out


def decisions(aw, bus, mask):
    """FREE_MAX decisions of four words: lockdown, mask, at_work, bus_dir"""
    dec = np.zeros((FREE_MAX, 4), np.uint32)
    dec[:, 1] = mask; dec[:, 2] = aw; dec[:, 3] = bus
    return np.ascontiguousarray(dec)


def test_m96_range_is_the_steps_a_to_b(probe):
    ab = np.array([(a, b) for a in range(FREE_MAX) for b in range(a, FREE_MAX)], np.uint32)
    assert len(ab) == 4656
    out = np.zeros((len(ab), 3), np.uint32)
    assert probe.sets_probe_range(ptr(ab), len(ab), ptr(out)) == 0
    bad = [(int(a), int(b)) for (a, b), o in zip(ab, out) if bits(o) != ((1 << (int(b) + 1)) - 1) & ~((1 << int(a)) - 1)]
    print("m96_range: %d of %d pairs differ" % (len(bad), len(ab)))
    assert not bad, bad[:8]


def test_m96_nibble_is_four_steps_from_p(probe):
    rng = np.random.default_rng(41)
    sets = [(1 << 96) - 1, 1 << 0, 1 << 63, 1 << 64, 1 << 95] + [int.from_bytes(rng.bytes(12), "little") for _ in range(2)]
    masks = np.array([[m & 0xFFFFFFFF, (m >> 32) & 0xFFFFFFFF, m >> 64] for m in sets], np.uint32)
    p = np.arange(-3, 99, dtype=np.int32)
    out = np.zeros((len(sets), len(p)), np.uint32)
    assert probe.sets_probe_nibble(ptr(masks), len(sets), ptr(p), len(p), ptr(out)) == 0
    bad = []
    for i, m in enumerate(sets):
        for k, pk in enumerate(p.tolist()):
            # bit h: step p + h is in the set (a step before 0 or from 96 on is in no set)
            want = sum(1 << h for h in range(4) if 0 <= pk + h < FREE_MAX and (m >> (pk + h)) & 1)
            if int(out[i, k]) != want:
                bad.append((i, pk, int(out[i, k]), want))
    print("m96_nibble: %d of %d differ" % (len(bad), out.size))
    assert not bad, bad[:8]


def iv_rule(iv, aw, bus):
    """per step j: the citizen of record iv stands where the record was left"""
    a, b = iv & 127, (iv >> 7) & 127
    pred = []
    for j in range(FREE_MAX):
        ok = bool(iv & IV_VALID) and a <= j <= b and not (bus[j] and iv & IV_PT)
        at_work = bool(aw[j]) and bool(iv & IV_HW)
        pred.append(ok and bool(iv & IV_AS_WORK) == at_work)
    return set_of(pred)


@pytest.mark.parametrize("n", N_CHUNK)
def test_iv_steps_is_the_set_of_steps_with_iv_present(probe, n):
    ivs = [IV_VALID | a | (b << 7) | (IV_PT if f & 1 else 0) | (IV_HW if f & 2 else 0) | (IV_AS_WORK if f & 4 else 0)
           for (a, b) in ((0, 0), (0, 95), (63, 64), (60, 67), (95, 95)) for f in range(8)]
    ivs += [60 | (67 << 7) | IV_PT | IV_HW | f * IV_AS_WORK for f in (0, 1)]          # not valid
    ivs = np.array(ivs, np.uint32)
    for name, (aw, bus, mask) in schedules(n).items():
        out = np.zeros((len(ivs), 6), np.uint32)
        masks = np.zeros(9, np.uint32)
        assert probe.sets_probe_iv(ptr(ivs), len(ivs), ptr(decisions(aw, bus, mask)), n, ptr(out), ptr(masks)) == 0
        assert bits(masks[0:3]) == set_of(aw != 0) and bits(masks[3:6]) == set_of(bus != 0) and bits(masks[6:9]) == set_of(mask == MASK_EVERYWHERE), name
        bad = []
        for iv, o in zip(ivs.tolist(), out):
            want = iv_rule(iv, aw, bus)
            if bits(o[0:3]) != want or bits(o[3:6]) != want:
                bad.append((hex(iv), hex(bits(o[0:3])), hex(bits(o[3:6])), hex(want)))
        print("iv_steps n %d %s: %d of %d records differ" % (n, name, len(bad), len(ivs)))
        assert not bad, (name, bad[:4])


def status_of(te, t, et, it):
    if te == TE_SUSCEPTIBLE: return "S"
    if te == TE_VACCINATED: return "V"
    if te == TE_RECOVERED: return "R"
    d = t + TE_BIAS - te
    return "E" if d <= et else "I" if d <= et + 1 + it else "R"


def stretch_rule(w, n, aw, bus, et, it):
    """(home, work, bus) of the word, one step at a time: status of the word at step T0 + j, the vaccination field, the flags and
    the schedule bits"""
    te, vf = w >> TE_SHIFT, (w >> VAX_SHIFT) & 0x7F
    vax_rel = 127 - vf if vf else None
    home, work, onbus = [], [], []
    for j in range(FREE_MAX):
        inf = j < n and not (vax_rel is not None and j > vax_rel) and status_of(te, T0 + j, et, it) == "I"
        b = inf and bool(bus[j]) and bool(w & FL_USES_PT)
        k = inf and not b and bool(aw[j]) and bool(w & FL_HAS_WORK)
        onbus.append(b); work.append(k); home.append(inf and not b and not k)
    return set_of(home), set_of(work), set_of(onbus)


def stretch_words(n, et, it):
    """Exposure steps that put the first / the last Infected step before, on and behind every edge of the chunk and of the 64-bit
    seam; Recovered, Vaccinated, Susceptible; a vaccination absent, at step 0 and at n - 1; the flags"""
    first = [T0 + a - et - 1 for a in (-10, 0, 5, 63, 64, n - 1, n)]                     # first Infected step T0 + a
    last = [T0 + b - et - 1 - it for b in (-1, 0, 63, 64, n - 1, n + 5)]                  # last Infected step T0 + b
    tes = sorted({e + TE_BIAS for e in first + last}) + [TE_RECOVERED, TE_VACCINATED, TE_SUSCEPTIBLE]
    assert min(tes) > 0
    words = [(te << TE_SHIFT) | ((127 - f) << VAX_SHIFT if f is not None else 0) | fl
             for te, f, fl in itertools.product(tes, (None, 0, n - 1), (0, FL_USES_PT, FL_HAS_WORK, FL_USES_PT | FL_HAS_WORK))]
    return np.array(words, np.uint32)


@pytest.mark.parametrize("et_it", ((96, 336), (1, 1)))
@pytest.mark.parametrize("n", N_CHUNK)
def test_infected_stretch_is_where_in_step_as_sets(probe, n, et_it):
    et, it = et_it
    words = stretch_words(n, et, it)
    active = 0
    for name, (aw, bus, mask) in schedules(n).items():
        out = np.zeros((len(words), STRETCH_OUT), np.uint32)
        assert probe.sets_probe_stretch(ptr(words), len(words), ptr(decisions(aw, bus, mask)), T0, n, et, it, ptr(out)) == 0
        bad = []
        for w, o in zip(words.tolist(), out):
            want = stretch_rule(w, n, aw, bus, et, it)
            got = (bits(o[0:3]), bits(o[3:6]), bits(o[6:9]))
            by_step = (bits(o[13:16]), bits(o[16:19]), bits(o[19:22]))
            ok = got == want and by_step == want and int(o[11]) == (1 if any(want) else 0)
            if any(want):
                active += 1
                both = want[0] | want[1] | want[2]
                rec = int(o[12])
                # the record: first and last Infected step, the flags; its steps at home / at work are the stretch's
                ok = ok and int(o[9]) == (both & -both).bit_length() - 1 and int(o[10]) == both.bit_length() - 1
                ok = ok and rec == (IV_VALID | int(o[9]) | (int(o[10]) << 7) | (IV_PT if w & FL_USES_PT else 0) | (IV_HW if w & FL_HAS_WORK else 0))
                ok = ok and iv_rule(rec, aw, bus) == want[0] and iv_rule(rec | IV_AS_WORK, aw, bus) == want[1]
            if not ok:
                bad.append((hex(w), [hex(x) for x in got], [hex(x) for x in want], o[9:13].tolist()))
        print("infected_stretch n %d et %d it %d %s: %d of %d words differ" % (n, et, it, name, len(bad), len(words)))
        assert not bad, (name, bad[:4])
    assert active > 0
