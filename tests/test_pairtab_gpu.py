"""The layer that the household, place and contact outputs share (esim_kernels_pairtab.h) on its own, against numpy, no tolerance:
the three counting modes of a group-by-group table of 64-bit counters against numpy.add.at, and the reduction over the runs of a
member list against numpy.add.at and numpy.minimum.at.  tests/native/pairtab_probe.hip is compiled here, as test_pairs_gpu.py
compiles its probe, and loaded with ctypes."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from epidemicsimulator_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE_CELL, LDS, GLOBAL = 0, 1, 2
BY_ALL, BY_GROUP = _lib.BY_ALL, _lib.BY_GROUP
NEVER = _lib.NEVER
N_TRIPLES = 1000                               # no multiple of 64 or of 256: the last wavefront and the last workgroup are partial


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("pairtab_probe") / "libpairtab_probe.so")
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
           "-I", os.path.join(ROOT, "epidemicsimulator_amd", "csrc"), "-o", out, os.path.join(ROOT, "tests", "native", "pairtab_probe.hip")]
    done = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stderr[-2000:]
    lib = ctypes.CDLL(out)
    lib.pairtab_probe_mode.restype = ctypes.c_int
    lib.pairtab_probe_mode.argtypes = [ctypes.c_int, ctypes.c_uint32]
    lib.pairtab_probe_pairs.restype = ctypes.c_int
    lib.pairtab_probe_pairs.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p]
    lib.pairtab_probe_runs.restype = ctypes.c_int
    lib.pairtab_probe_runs.argtypes = [ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32,
                                       ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    assert int(ctypes.c_uint32.in_dll(lib, "pairtab_lds_bytes").value) == 32768
    return lib


def test_the_switch_between_the_modes(probe):
    """One cell without groups; with groups the workgroup's table up to 45 groups (2 * 45 * 45 * 8 B <= 32 KB), the global one from 46."""
    assert probe.pairtab_probe_mode(BY_ALL, 1) == ONE_CELL
    assert [probe.pairtab_probe_mode(BY_GROUP, n) for n in (1, 2, 45, 46)] == [LDS, LDS, LDS, GLOBAL]


def triples(n_cols):
    """1000 (row group, column group, count): about a tenth of the labels on either side lie outside the groups, the counts reach
    2^32 - 1, and the first cell gets enough of those to pass 2^32."""
    rng = np.random.default_rng(1000 + n_cols)
    row = rng.integers(0, n_cols, N_TRIPLES, dtype=np.uint32)
    col = rng.integers(0, n_cols, N_TRIPLES, dtype=np.uint32)
    row[rng.random(N_TRIPLES) < 0.1] = n_cols
    col[rng.random(N_TRIPLES) < 0.1] = 0xFFFF
    cnt = rng.integers(0, 1 << 32, N_TRIPLES, dtype=np.uint64).astype(np.uint32)
    cnt[:8] = 0xFFFFFFFF
    row[:8] = col[:8] = 0
    cnt[8] = 0
    return row, col, cnt


def expected(row, col, cnt, n_cols):
    """The two tables: the triples at even positions go to the first, those at odd positions to the second."""
    cells = n_cols * n_cols
    want = np.zeros(2 * cells, np.uint64)
    keep = (row < n_cols) & (col < n_cols)
    which = (np.arange(row.size) & 1).astype(np.uint64)
    np.add.at(want, (which * np.uint64(cells) + row.astype(np.uint64) * np.uint64(n_cols) + col.astype(np.uint64))[keep].astype(np.int64), cnt[keep].astype(np.uint64))
    return want


@pytest.mark.parametrize("grid", (1, 3))
@pytest.mark.parametrize("n_cols", (1, 2, 45, 46))
def test_the_three_modes_give_the_table_of_numpy(probe, n_cols, grid):
    row, col, cnt = triples(n_cols)
    want = expected(row, col, cnt, n_cols)
    assert int(want[0]) > 1 << 32 and (~((row < n_cols) & (col < n_cols))).sum() >= 50
    # (one cell is the form without groups; the workgroup's table is run at 46 groups too, where the library has left it)
    for mode in (ONE_CELL, LDS, GLOBAL) if n_cols == 1 else (LDS, GLOBAL):
        got = np.full(2 * n_cols * n_cols, 0xDEADBEEF, np.uint64)
        rc = probe.pairtab_probe_pairs(mode, grid, row.ctypes.data, col.ctypes.data, cnt.ctypes.data, N_TRIPLES, n_cols, got.ctypes.data)
        assert rc == 0, (mode, rc)
        bad = np.flatnonzero(got != want)
        print("n_cols %d, grid %d, mode %d: %d cells, %d non-zero, %d differ" % (n_cols, grid, mode, got.size, int((want != 0).sum()), bad.size))
        assert bad.size == 0, (mode, bad[:8].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist())


def runs():
    """A key per run, runs of 63, 1, 2, 64, 65, 129 and 300 entries and a few entries without a key between and behind them: the
    run of 64 crosses a wavefront boundary (entry 128), the run of 129 a workgroup boundary (256), the run of 300 the next (512)."""
    rng = np.random.default_rng(77)
    lengths = (63, 1, 2, 64, 65, 129, 300)
    key = np.concatenate([np.full(n, k, np.uint32) for k, n in enumerate(lengths)] + [np.full(5, NEVER, np.uint32)])
    key[200] = key[400] = NEVER                                     # (an entry of no place inside a run: the run goes on behind it)
    n = key.size
    is_case = rng.random(n) < 0.4
    is_intro = is_case & (rng.random(n) < 0.5)
    step = np.where(is_case, rng.integers(0, 5000, n), NEVER).astype(np.uint32)
    is_case[:63] = False; is_intro[:63] = False; step[:63] = NEVER    # a run without a case: nothing is added, its first step stays
    is_case[key == NEVER] = False; is_intro[key == NEVER] = False; step[key == NEVER] = NEVER
    return key, is_case, is_intro, step, len(lengths)


@pytest.mark.parametrize("grid", (1, 3))
def test_the_run_reduction_gives_the_counts_and_the_first_step_per_key(probe, grid):
    key, is_case, is_intro, step, n_keys = runs()
    assert key.size > 2 * 256 and key[127] == key[128] and key[255] == key[256] and key[511] == key[512]
    live = key != NEVER
    want_cases, want_intro, want_first = np.zeros(n_keys, np.uint32), np.zeros(n_keys, np.uint32), np.full(n_keys, NEVER, np.uint32)
    np.add.at(want_cases, key[live], is_case[live].astype(np.uint32))
    np.add.at(want_intro, key[live], is_intro[live].astype(np.uint32))
    np.minimum.at(want_first, key[live], step[live])
    assert want_cases[0] == 0 and want_first[0] == NEVER and (want_cases[3:] > 0).all() and (want_first[3:] != NEVER).all()
    flags = (is_case.astype(np.uint8) | (is_intro.astype(np.uint8) << 1)).astype(np.uint8)
    cases, intro, first = (np.full(n_keys, 0xDEADBEEF, np.uint32) for _ in range(3))
    rc = probe.pairtab_probe_runs(grid, key.ctypes.data, flags.ctypes.data, step.ctypes.data, key.size, n_keys, cases.ctypes.data, intro.ctypes.data, first.ctypes.data)
    assert rc == 0, rc
    print("grid %d: cases %s, introductions %s, first step %s" % (grid, cases.tolist(), intro.tolist(), first.tolist()))
    assert (cases == want_cases).all(), (cases.tolist(), want_cases.tolist())
    assert (intro == want_intro).all(), (intro.tolist(), want_intro.tolist())
    assert (first == want_first).all(), (first.tolist(), want_first.tolist())
