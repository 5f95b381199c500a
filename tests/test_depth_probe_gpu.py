"""The kernels of esim_depth.h on their own, against numpy (tests/_depth_ref.py): every value, no tolerance.
tests/native/depth_probe.hip is compiled here as test_members_probe_gpu.py compiles its probe, and loaded with ctypes.  The member
counts are that file's -- every padded size, one past each, both sides of the seam between the register and the LDS kernels --
and so are the planes, with their eight kinds of cell.  The shapes put one column under all 64 lanes of a wavefront, a few
columns under some of them, exactly a wavefront of columns, and tails behind 64 and 256; a grid bound of 1 and of 3 workgroups
makes the loops take several trips."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import _depth_ref as ref
from _members_ref import NEVER
from test_members_probe_gpu import KINDS, MEMBERS, make_planes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((1, 1), (7, 1), (200, 1), (5, 3), (3, 64), (2, 65), (4, 257), (1, 1000))      # (rows, cols)
GRIDS = (1, 3)
u32p, u64p = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)
u32 = ctypes.c_uint32


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("depth_probe") / "libdepth_probe.so")
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
           "-I", os.path.join(ROOT, "epidemicsimulator_amd", "csrc"), "-o", out, os.path.join(ROOT, "tests", "native", "depth_probe.hip")]
    done = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert done.returncode == 0, done.stderr[-2000:]
    lib = ctypes.CDLL(out)
    lib.depth_probe_depth.restype = ctypes.c_int
    lib.depth_probe_depth.argtypes = [u32p, u32, u32, u32, u32, u32, u64p, u32, u32p, u32, u32p, u64p]
    lib.depth_probe_band.restype = ctypes.c_int
    lib.depth_probe_band.argtypes = [u32p, u32, u32, u32, u32, u32, u64p, u32, u32p, u32, ctypes.c_int, u32, u32p, u32p, u32p, u32p, u32p]
    assert int(u32.in_dll(lib, "depth_members_max").value) == 256
    return lib


def tables(x):
    """(zero, never) as the accumulators hold them per cell of planes [m, cells]: the sum, and the members that reached it."""
    return np.ascontiguousarray(x.astype(np.uint64).sum(axis=0)), np.ascontiguousarray((x != NEVER).sum(axis=0).astype(np.uint32))


def skip_args(skip):
    zero, never = skip if skip is not None else (None, None)
    return (None if zero is None else zero.ctypes.data_as(u64p), 0, None if never is None else never.ctypes.data_as(u32p))


def depth(probe, x, first_row, n_rows, n_cols, grid, skip=None):
    m, stride = x.shape
    d, t = np.full((m, n_cols), 0xA5A5A5A5, np.uint32), np.zeros(m, np.uint64)
    rc = probe.depth_probe_depth(x.ctypes.data_as(u32p), m, stride, first_row, n_rows, n_cols, *skip_args(skip), grid, d.ctypes.data_as(u32p), t.ctypes.data_as(u64p))
    assert rc == 0, rc
    return d, t


def band(probe, x, first_row, n_rows, n_cols, need, pooled, grid, skip=None):
    m, stride = x.shape
    planes = [np.zeros((n_rows, n_cols), np.uint32) for _ in range(3)]
    cols = [np.zeros(n_cols, np.uint32) for _ in range(2)]
    rc = probe.depth_probe_band(x.ctypes.data_as(u32p), m, stride, first_row, n_rows, n_cols, *skip_args(skip), need, int(pooled), grid,
                                *(a.ctypes.data_as(u32p) for a in planes + cols))
    assert rc == 0, rc                                              # (-2: a word behind a plane of the output was written)
    return dict(zip(("lo", "hi", "median", "deepest", "n_in"), planes + cols))


def check(probe, x, first_row, n_rows, n_cols, what):
    """The window of planes [m, cells] against numpy: depth, totals and the band at three sizes, pooled and not; with and without
    the skip tables; under both grid bounds."""
    m = x.shape[0]
    stack = x.reshape(m, -1, n_cols)[:, first_row:first_row + n_rows]
    want_d = ref.depth(stack)
    assert int(want_d.max()) <= n_rows * ref.pairs(m) < 1 << 32
    want_b = {(need, pooled): ref.band(stack, need, pooled) for need in sorted({1, -(-m // 2), m}) for pooled in (False, True)}
    for grid in GRIDS:
        for skip in (None, tables(x)):
            note = (what, "grid %d" % grid, "skip" if skip else "no skip")
            d, t = depth(probe, x, first_row, n_rows, n_cols, grid, skip)
            assert (d == want_d).all(), (note, "depth", np.argwhere(d != want_d)[:8].tolist())
            assert (t == want_d.sum(axis=1, dtype=np.uint64)).all(), (note, "total")
            for (need, pooled), want in want_b.items():
                got = band(probe, x, first_row, n_rows, n_cols, need, pooled, grid, skip)
                for k in got:
                    assert (got[k] == want[k]).all(), (note, "need %d" % need, "pooled" if pooled else "per column", k, np.argwhere(got[k] != want[k])[:8].tolist())
    return want_d, want_b


@pytest.mark.parametrize("m", MEMBERS)
def test_every_value_equals_numpy(probe, m):
    for rows, cols in SHAPES:
        cells = rows * cols
        x, kind = make_planes(m, cells, 100 * m + cells)
        if cells >= KINDS:
            assert set(kind.tolist()) == set(range(KINDS))
            zero, never = tables(x)
            assert (zero == 0).any() and (never == 0).any()         # cells the skip tables settle, of both kinds
        if cells == 1000:                                           # trips of the loops: 256 cells a workgroup up to 64 members, 64 beyond
            assert all(-(-cells // (grid * 256)) >= (3 if grid == 1 else 2) for grid in GRIDS)
        want_d, want_b = check(probe, x, 0, rows, cols, "m = %d, %d x %d" % (m, rows, cols))
        if m >= 7 and cells >= 64:                                  # the input is not trivial: depths differ, ties at the threshold occur
            assert (want_d.min(axis=0) < want_d.max(axis=0)).any()
            half = want_b[(-(-m // 2), False)]
            assert (half["lo"] < half["hi"]).any() and (half["n_in"] >= -(-m // 2)).all()


def test_a_window_of_rows_inside_taller_planes(probe):
    """Rows [first_row, first_row + n_rows) of planes with more rows, as the library addresses the store: the depths are those of
    the window alone, and nothing behind the window's planes is written (the probe checks its guard words)."""
    for m, rows, cols, first_row, n_rows in ((9, 12, 5, 2, 7), (33, 9, 70, 3, 4), (70, 6, 131, 1, 3), (6, 40, 1, 13, 20)):
        x, _ = make_planes(m, rows * cols, 7 * m + cols)
        check(probe, x, first_row, n_rows, cols, "m = %d, rows %d..%d of %d x %d" % (m, first_row, first_row + n_rows, rows, cols))
    x, _ = make_planes(9, 60, 1)
    d, t = depth(probe, x, 4, 0, 5, 1)                              # a window without rows: every depth is 0
    assert not d.any() and not t.any()


def test_ties_at_the_threshold_are_all_in_and_the_first_deepest_member_is_taken(probe):
    x = np.array([[0, 5], [3, 5], [3, 5], [9, 5]], np.uint32)       # column 0: members 1 and 2 tie for the deepest; column 1: all equal
    got = band(probe, x, 0, 1, 2, 1, False, 1)
    assert got["deepest"].tolist() == [1, 0] and got["n_in"].tolist() == [2, 4]
    assert got["lo"].tolist() == [[3, 5]] and got["hi"].tolist() == [[3, 5]] and got["median"].tolist() == [[3, 5]]
    want = ref.band(x.reshape(4, 1, 2), 1, False)
    assert all((got[k] == want[k]).all() for k in got)


def test_the_probe_refuses_what_the_library_refuses(probe):
    x = np.zeros((4, 8), np.uint32)
    planes = [np.zeros(8, np.uint32) for _ in range(5)]
    args = lambda need, pooled=0, n_rows=2, m=4: (x.ctypes.data_as(u32p), m, 8, 0, n_rows, 4, None, 0, None, need, pooled, 1, *(a.ctypes.data_as(u32p) for a in planes))
    assert probe.depth_probe_band(*args(0)) == -1 and probe.depth_probe_band(*args(5)) == -1      # need outside 1..members
    assert probe.depth_probe_band(*args(1, n_rows=3)) == -1                                       # rows outside the planes
    assert probe.depth_probe_band(*args(4)) == 0
