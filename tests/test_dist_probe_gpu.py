"""The kernels of esim_dist.h on their own, against numpy (tests/_dist_ref.py): every value, no tolerance.
tests/native/dist_probe.hip is compiled here as test_depth_probe_gpu.py compiles its probe, and loaded with ctypes; the probe
keeps guard words behind the matrix and behind the kernel's counts.  The member counts and the planes are those of
test_members_probe_gpu.py -- every padded size, one past each, both sides of 64; 65 to 256 members take several member tiles and
a padded last one -- and the shapes those of test_depth_probe_gpu.py.  A grid bound of 1 and of 3 workgroups makes the loops
over tile pairs and trips take several turns."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import _dist_ref as ref
from _members_ref import NEVER, to_key
from test_members_probe_gpu import KINDS, MEMBERS, make_planes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((1, 1), (7, 1), (200, 1), (5, 3), (3, 64), (2, 65), (4, 257), (1, 1000))      # (rows, cols)
GRIDS = (1, 3)
NEVER_AS = (0xFFFFFFFF, 0, 12345)
METRICS = (("l1", 0), ("differ", 1))
u32p, u64p = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)
u32 = ctypes.c_uint32
TILE, TRIP, NARROW = 64, 256, 1 << 26          # the cells of a tile and of a trip; a tile whose key range is below NARROW sums in 32 bits


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("dist_probe") / "libdist_probe.so")
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
           "-I", os.path.join(ROOT, "epidemicsimulator_amd", "csrc"), "-o", out, os.path.join(ROOT, "tests", "native", "dist_probe.hip")]
    done = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert done.returncode == 0, done.stderr[-2000:]
    lib = ctypes.CDLL(out)
    lib.dist_probe.restype = ctypes.c_int
    lib.dist_probe.argtypes = [u32p, u32, u32, u32, u32, u32, u64p, u32, u32p, ctypes.c_int, u32, u32, u64p, u64p]
    const = lambda name: int(u32.in_dll(lib, name).value)
    assert const("dist_members_max") == 256 and const("dist_tile_cells") == TILE and const("dist_trip_cells") == TRIP and const("dist_narrow_range") == NARROW
    return lib


def tables(x):
    """(zero, never) as the accumulators hold them per cell of planes [m, cells]: the sum, and the members that reached it."""
    return np.ascontiguousarray(x.astype(np.uint64).sum(axis=0)), np.ascontiguousarray((x != NEVER).sum(axis=0).astype(np.uint32))


def dist(probe, x, first_row, n_rows, n_cols, metric, never_as, grid, skip=None):
    """(matrix uint64 [m, m], {"live", "tiles", "narrow", "partial"})."""
    m, stride = x.shape
    zero, never = skip if skip is not None else (None, None)
    out, stats = np.full((m, m), 0x5A5A5A5A, np.uint64), np.zeros(4, np.uint64)
    rc = probe.dist_probe(x.ctypes.data_as(u32p), m, stride, first_row, n_rows, n_cols, None if zero is None else zero.ctypes.data_as(u64p), 0,
                          None if never is None else never.ctypes.data_as(u32p), metric, never_as, grid, out.ctypes.data_as(u64p), stats.ctypes.data_as(u64p))
    assert rc == 0, rc                                              # (-2: a word behind an output was written)
    return out, dict(zip(("live", "tiles", "narrow", "partial"), (int(v) for v in stats)))


def tile_pairs(m):
    t = -(-m // (16 if m <= 16 else 32 if m <= 32 else 64))
    return t * (t + 1) // 2


def check(probe, x, first_row, n_rows, n_cols, what, never_as=NEVER_AS, skips=True):
    """The window of planes [m, cells] against numpy: both metrics, every never_as, with and without the skip tables, under both
    grid bounds.  Returns the counts of the L1 call with the first never_as, without skip tables, under a grid of 1."""
    m = x.shape[0]
    first, n = first_row * n_cols, n_rows * n_cols
    window = x[:, first:first + n]
    kept = None
    for name, code in METRICS:
        for na in never_as:
            want = ref.distances(window, name, na)
            assert (want == want.T).all() and not np.diagonal(want).any()
            for grid in GRIDS:
                for skip in ((None, tables(x)) if skips else (None,)):
                    note = (what, name, "never_as %#x" % na, "grid %d" % grid, "skip" if skip else "no skip")
                    got, stats = dist(probe, x, first_row, n_rows, n_cols, code, na, grid, skip)
                    assert (got == want).all(), (note, np.argwhere(got != want)[:8].tolist())
                    assert (got == got.T).all() and not np.diagonal(got).any(), note
                    live = ref.live_cells(*(skip or (None, None)), first, n) if m > 1 else 0
                    assert stats["live"] == live, (note, stats)
                    assert stats["narrow"] <= stats["tiles"] and stats["partial"] <= stats["tiles"], (note, stats)
                    if code == 1:
                        assert stats["narrow"] == stats["tiles"], (note, stats)
                    if grid == 1 and m > 1:                         # one workgroup: every tile pair packs the live cells into ceil(live / TILE) tiles
                        assert stats["tiles"] == tile_pairs(m) * -(-live // TILE) and stats["partial"] == tile_pairs(m) * (1 if live % TILE else 0), (note, stats)
                    if grid == 1 and skip is None and code == 0 and na == never_as[0]:
                        kept = stats
    return kept


@pytest.mark.parametrize("m", MEMBERS)
def test_every_value_equals_numpy(probe, m):
    for rows, cols in SHAPES:
        cells = rows * cols
        x, kind = make_planes(m, cells, 100 * m + cells)
        if cells >= KINDS:
            assert set(kind.tolist()) == set(range(KINDS))
            zero, never = tables(x)
            assert (zero == 0).any() and (never == 0).any()         # cells the skip tables settle, of both kinds
        stats = check(probe, x, 0, rows, cols, "m = %d, %d x %d" % (m, rows, cols))
        if cells == 1000 and m > 1:
            # the loops make at least two trips under either grid bound, the packed tile is flushed more than once and once partially
            assert all(-(-cells // (grid * TRIP)) >= 2 for grid in GRIDS) and tile_pairs(m) >= (1 if m <= 64 else 3)
            assert stats["tiles"] == 16 * tile_pairs(m) and stats["partial"] == tile_pairs(m), stats


def seam_planes(m, cells, lo, span, seed):
    """Keys in [lo, lo + span] with both ends in every cell among the first two members of every member tile of 64, so that every
    tile of every tile pair has exactly that range."""
    rng = np.random.default_rng(seed)
    x = (lo + rng.integers(0, span + 1, size=(m, cells), dtype=np.uint64)).astype(np.uint32)
    for t in range(0, m - 1, 64):
        x[t], x[t + 1] = lo, lo + span
        x[t:t + 2] = np.where(rng.integers(0, 2, size=cells).astype(bool), x[t:t + 2], x[t:t + 2][::-1])
    return np.ascontiguousarray(x)


def test_the_seam_between_32_and_64_bit_accumulation(probe):
    """A tile sums in 32 bits while (max - min) * 64 < 2^32: a range of 2^26 - 1 is the last that does, 2^26 sits exactly at the
    bound and 2^26 + 1 past it.  The counts say which path ran; the sums are exact on both."""
    for m, cells in ((3, 64), (5, 200), (70, 130)):                      # (70: three tile pairs, members 64 and 65 hold the ends too)
        for lo in (0, 12345, 0xFFFFFFFE - (NARROW + 1)):
            for span, narrow in ((NARROW - 1, True), (NARROW, False), (NARROW + 1, False)):
                x = seam_planes(m, cells, lo, span, m + span % 7)
                assert int(x.max()) - int(x.min()) == span
                what = "m = %d, cells = %d, keys %#x + %#x" % (m, cells, lo, span)
                check(probe, x, 0, 1, cells, what, never_as=(NEVER,), skips=False)
                _, stats = dist(probe, x, 0, 1, cells, 0, NEVER, 1)
                assert stats["narrow"] == (stats["tiles"] if narrow else 0), (what, stats)
    # every cell {0, 0xFFFFFFFE}: two cells overflow 32 bits
    for m, cells in ((2, 2), (2, 64), (9, 300), (66, 70)):
        rng = np.random.default_rng(cells)
        x = np.ascontiguousarray(np.where(rng.integers(0, 2, size=(m, cells)).astype(bool), np.uint32(0xFFFFFFFE), np.uint32(0)))
        for t in range(0, m - 1, 64):
            x[t], x[t + 1] = 0, 0xFFFFFFFE
        want = ref.distances(x, "l1")
        assert int(want[0, 1]) == cells * 0xFFFFFFFE and (cells < 2 or int(want[0, 1]) >= 1 << 32)
        check(probe, x, 0, 1, cells, "0 and 0xFFFFFFFE, m = %d, cells = %d" % (m, cells), skips=False)
        _, stats = dist(probe, x, 0, 1, cells, 0, NEVER, 1)
        assert stats["narrow"] == 0, stats
    # a signed store: keys around 0x80000000 differ as the values do, and a small range stays in 32 bits
    rng = np.random.default_rng(5)
    v = rng.integers(-5, 6, size=(7, 333)).astype(np.int32)
    x = np.ascontiguousarray(to_key(v))
    assert (x < 0x80000000).any() and (x >= 0x80000000).any()
    want = ref.distances(x, "l1")
    assert (want == ref.distances(v, "l1")).all() and int(want[0, 1]) == int(np.abs(v[0].astype(np.int64) - v[1]).sum())
    check(probe, x, 0, 1, 333, "signed keys", skips=False)
    _, stats = dist(probe, x, 0, 1, 333, 0, NEVER, 1)
    assert stats["narrow"] == stats["tiles"] == 6, stats


def test_live_cells_are_packed_and_settled_cells_are_not_read(probe):
    """Live cells between settled ones; a run of settled cells longer than a tile and longer than a trip; a single live cell at
    the end of the window.  live_cells is the count from the tables, and the matrix is the one without them."""
    rng = np.random.default_rng(11)
    for m in (6, 40, 130):
        cells = 1500
        x = rng.integers(0, 1 << 20, size=(m, cells), dtype=np.uint64).astype(np.uint32)
        x[:, 1:600:2] = 0                                           # alternating: settled by the sums
        x[:, 2:600:4] = NEVER                                       # and by the members that reached the cell
        x[:, 600:1499] = 0                                          # a run of 899 settled cells
        x[:, 700:900] = NEVER
        x = np.ascontiguousarray(x)
        zero, never = tables(x)
        live = int(((zero != 0) & (never != 0)).sum())
        assert live == 151 and zero[1499] != 0 and never[1499] != 0 and zero[1498] == 0
        for name, code in METRICS:
            for na in NEVER_AS:
                want = ref.distances(x, name, na)
                for grid in GRIDS:
                    plain, s0 = dist(probe, x, 0, 1, cells, code, na, grid)
                    got, s1 = dist(probe, x, 0, 1, cells, code, na, grid, (zero, never))
                    assert (plain == want).all() and (got == want).all(), (m, name, na, grid)
                    assert s0["live"] == cells and s1["live"] == live, (s0, s1)
                    if grid == 1:                                   # 151 live cells: two full tiles and a partial one per tile pair
                        assert s1["tiles"] == 3 * tile_pairs(m) and s1["partial"] == tile_pairs(m), s1
        # the window [1400, 1500): one live cell, the last
        got, s1 = dist(probe, x, 14, 1, 100, 0, NEVER, 1, (zero, never))
        assert (got == ref.distances(x[:, 1499:], "l1")).all() and s1["live"] == 1 and s1["tiles"] == s1["partial"] == tile_pairs(m)
        # only one of the two tables
        for skip in ((zero, None), (None, never)):
            got, s1 = dist(probe, x, 0, 1, cells, 0, 0, 3, skip)
            assert (got == ref.distances(x, "l1", 0)).all() and s1["live"] == ref.live_cells(*skip, 0, cells)


def test_a_window_of_rows_inside_taller_planes(probe):
    """Rows [first_row, first_row + n_rows) of planes with more rows, as the library addresses the store; a window without rows
    and a single member give zeros; the matrix is symmetric with a zero diagonal."""
    for m, rows, cols, first_row, n_rows in ((9, 12, 5, 2, 7), (33, 9, 70, 3, 4), (70, 6, 131, 1, 3), (6, 40, 1, 13, 20)):
        x, _ = make_planes(m, rows * cols, 7 * m + cols)
        check(probe, x, first_row, n_rows, cols, "m = %d, rows %d..%d of %d x %d" % (m, first_row, first_row + n_rows, rows, cols))
    x, _ = make_planes(9, 60, 1)
    for code in (0, 1):
        got, stats = dist(probe, x, 4, 0, 5, code, NEVER, 1)        # a window without rows
        assert not got.any() and not any(stats.values())
        got, stats = dist(probe, x[:1], 0, 12, 5, code, NEVER, 3)   # one member
        assert got.shape == (1, 1) and not got.any()
    x, _ = make_planes(12, 500, 3)
    got, _ = dist(probe, x, 0, 5, 100, 0, NEVER, 3)
    assert all(int(got[i, i]) == 0 for i in range(12))
    assert all(int(got[i, j]) == int(got[j, i]) for i in range(12) for j in range(i))
    assert (got[np.triu_indices(12, 1)] > 0).all()


def test_the_probe_refuses_what_the_library_refuses(probe):
    x = np.zeros((4, 8), np.uint32)
    out, stats = np.zeros(16, np.uint64), np.zeros(4, np.uint64)
    args = lambda metric, n_rows=2: (x.ctypes.data_as(u32p), 4, 8, 0, n_rows, 4, None, 0, None, metric, NEVER, 1, out.ctypes.data_as(u64p), stats.ctypes.data_as(u64p))
    assert probe.dist_probe(*args(2)) == -1 and probe.dist_probe(*args(-1)) == -1                 # an unknown metric
    assert probe.dist_probe(*args(0, n_rows=3)) == -1                                             # rows outside the planes
    assert probe.dist_probe(*args(0)) == 0 and probe.dist_probe(*args(1)) == 0
