"""The kernels of esim_arms.h on their own, against numpy (tests/_arms_ref.py): every value, no tolerance.
tests/native/arms_probe.hip is compiled here as test_dist_probe_gpu.py compiles its probe, and loaded with ctypes; the probe
keeps guard words behind each of its six outputs.  The planes are those of test_members_probe_gpu.py and the shapes those of
test_dist_probe_gpu.py.  The (arms, replicates) cover every padded width of the arms (2, 4, 8, 16), one past each, and both sides
of 64 and of 256 members; a grid bound of 1 and of 3 workgroups makes the loop over the cells take several trips."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import _arms_ref as ref
from test_members_probe_gpu import KINDS, make_planes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEVER = ref.NEVER
SHAPES = ((1, 1), (7, 1), (200, 1), (5, 3), (3, 64), (2, 65), (4, 257), (1, 1000))      # (rows, cols)
GRIDS = (1, 3)
NEVER_AS = (0xFFFFFFFF, 0, 12345)
GRID = ((1, (1, 7)), (2, (1, 2, 32, 33, 128)), (3, (1, 5, 21, 22, 85)), (4, (16, 17, 64)), (5, (3, 51)), (8, (8, 9, 32)), (9, (7,)), (15, (17,)), (16, (1, 4, 5, 16)))
CASES = [(a, s) for a, reps in GRID for s in reps]
TRIP = 256                                                          # the cells of a workgroup's trip
u32p, u64p = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)
u32 = ctypes.c_uint32


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("arms_probe") / "libarms_probe.so")
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
           "-I", os.path.join(ROOT, "epidemicsimulator_amd", "csrc"), "-o", out, os.path.join(ROOT, "tests", "native", "arms_probe.hip")]
    done = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert done.returncode == 0, done.stderr[-2000:]
    lib = ctypes.CDLL(out)
    lib.arms_probe.restype = ctypes.c_int
    lib.arms_probe.argtypes = [u32p, u32, u32, u32, u32, u32, u64p, u32, u32p, u32, ctypes.c_int, u32, u32, u32p, u32p, u64p, u64p, u64p, u64p]
    const = lambda name: int(u32.in_dll(lib, name).value)
    assert const("arms_members_max") == 256 and const("arms_max") == 16 and const("arms_trip_cells") == TRIP
    return lib


def tables(x):
    """(zero, never) as the accumulators hold them per cell of planes [m, cells]: the sum, and the members that reached it."""
    return np.ascontiguousarray(x.astype(np.uint64).sum(axis=0)), np.ascontiguousarray((x != NEVER).sum(axis=0).astype(np.uint32))


def arms(probe, x, first_row, n_rows, n_cols, n_arms, maximize, never_as, grid, skip=None):
    """({"best", "sole", "regret", "sum": [n_arms, n_rows * n_cols], "totals": [S, n_arms]}, {"live", "common"})."""
    m, stride = x.shape
    zero, never = skip if skip is not None else (None, None)
    cells = n_rows * n_cols
    out = {"best": np.full((n_arms, cells), 0x5A5A5A5A, np.uint32), "sole": np.full((n_arms, cells), 0x5A5A5A5A, np.uint32),
           "regret": np.full((n_arms, cells), 0x5A5A5A5A, np.uint64), "sum": np.full((n_arms, cells), 0x5A5A5A5A, np.uint64),
           "totals": np.full((m // n_arms, n_arms), 0x5A5A5A5A, np.uint64)}
    stats = np.zeros(2, np.uint64)
    rc = probe.arms_probe(x.ctypes.data_as(u32p), m, stride, first_row, n_rows, n_cols, None if zero is None else zero.ctypes.data_as(u64p), 0,
                          None if never is None else never.ctypes.data_as(u32p), n_arms, int(maximize), never_as, grid, out["best"].ctypes.data_as(u32p),
                          out["sole"].ctypes.data_as(u32p), out["regret"].ctypes.data_as(u64p), out["sum"].ctypes.data_as(u64p), out["totals"].ctypes.data_as(u64p),
                          stats.ctypes.data_as(u64p))
    assert rc == 0, rc                                              # (-2: a word behind an output was written)
    return out, {"live": int(stats[0]), "common": int(stats[1])}


def same(got, want, note):
    for k in ref.KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (note, k, got[k].shape, want[k].shape)
        assert (got[k] == want[k]).all(), (note, k, np.argwhere(got[k] != want[k])[:8].tolist())


def check(probe, x, n_arms, first_row, n_rows, n_cols, what, never_as=NEVER_AS, skips=True, grids=GRIDS):
    """The window of planes [m, cells] against numpy: both senses, every never_as, with and without the skip tables, under both
    grid bounds."""
    first, n = first_row * n_cols, n_rows * n_cols
    window = x[:, first:first + n]
    s = x.shape[0] // n_arms
    both = tables(x)
    for maximize in (False, True):
        for na in never_as:
            want = ref.arms(window, n_arms, maximize, na)
            assert (want["sole"] <= want["best"]).all() and (want["sole"].sum(axis=0) <= s).all() and (want["best"].sum(axis=0) >= s).all()
            for grid in grids:
                for skip in ((None, both) if skips else (None,)):
                    note = (what, "%d arms" % n_arms, "max" if maximize else "min", "never_as %#x" % na, "grid %d" % grid, "skip" if skip else "no skip")
                    got, stats = arms(probe, x, first_row, n_rows, n_cols, n_arms, maximize, na, grid, skip)
                    same(got, want, note)
                    assert stats["live"] == ref.live_cells(*(skip or (None, None)), first, n), (note, stats)


@pytest.mark.parametrize("n_arms,reps", CASES)
def test_every_value_equals_numpy(probe, n_arms, reps):
    m = n_arms * reps
    for rows, cols in SHAPES:
        cells = rows * cols
        x, kind = make_planes(m, cells, 100 * m + cells + n_arms)
        if cells >= KINDS:
            assert set(kind.tolist()) == set(range(KINDS))
            zero, never = tables(x)
            assert (zero == 0).any() and (never == 0).any()         # cells the skip tables settle, of both kinds
        check(probe, x, n_arms, 0, rows, cols, "%d x %d, %d x %d" % (n_arms, reps, rows, cols))
    assert all(-(-1000 // (grid * TRIP)) >= 2 for grid in GRIDS)    # the loop makes at least two trips under either bound


@pytest.mark.parametrize("n_arms", (3, 5))
def test_padding_arms_neither_win_nor_tie_nor_break_a_sole_win(probe, n_arms):
    """A replicate whose real arms all sit at the padding key: 0xFFFFFFFF when minimising with ESIM_NEVER left as it is, 0 when
    maximising.  All real arms tie, nobody wins alone, nobody regrets -- and a single arm off the padding key wins alone."""
    for reps, cells in ((1, 1), (4, 70), (9, 300)):
        m = n_arms * reps
        for key, maximize in ((NEVER, False), (0, True)):
            x = np.full((m, cells), key, np.uint32)
            for grid in GRIDS:
                got, stats = arms(probe, x, 0, 1, cells, n_arms, maximize, NEVER, grid)
                note = (n_arms, reps, cells, key, grid)
                assert (got["best"] == reps).all() and not got["sole"].any() and not got["regret"].any(), note
                assert (got["sum"] == reps * key).all() and (got["totals"] == cells * key).all() and stats["live"] == cells, note
                same(got, ref.arms(x, n_arms, maximize, NEVER), note)
            # the last real arm of every replicate one step off the padding key, towards the better side: it alone is best
            y = x.copy()
            y[n_arms - 1::n_arms] = key - 1 if key else 1
            got, _ = arms(probe, y, 0, 1, cells, n_arms, maximize, NEVER, 3)
            same(got, ref.arms(y, n_arms, maximize, NEVER), (n_arms, reps, cells, key, "one arm off"))
            assert (got["sole"][n_arms - 1] == reps).all() and (got["best"][:n_arms - 1] == 0).all() and (got["regret"][:n_arms - 1] == reps).all()
        # both senses on both fills, with the tables that settle every cell: nothing is read
        for key in (NEVER, 0):
            x = np.full((m, cells), key, np.uint32)
            for maximize in (False, True):
                got, stats = arms(probe, x, 0, 1, cells, n_arms, maximize, NEVER, 1, tables(x))
                assert (got["best"] == reps).all() and not got["sole"].any() and not got["regret"].any() and stats["live"] == 0
                same(got, ref.arms(x, n_arms, maximize, NEVER), (n_arms, key, maximize, "settled"))


def test_regret_sums_and_totals_beyond_32_bits(probe):
    """Keys 0 and 0xFFFFFFFE over 300 cells: a cell's regret and sum pass 2^32 with two replicates, a member's total with two
    cells."""
    for n_arms, reps in ((2, 2), (3, 5), (7, 9), (16, 16)):
        rng = np.random.default_rng(n_arms)
        x = np.ascontiguousarray(np.where(rng.integers(0, 2, size=(n_arms * reps, 300)).astype(bool), np.uint32(0xFFFFFFFE), np.uint32(0)))
        x[0], x[1] = 0, 0xFFFFFFFE
        want = ref.arms(x, n_arms)
        assert int(want["regret"].max()) >= 1 << 32 and int(want["sum"].max()) >= 1 << 32 and int(want["totals"].min(initial=1 << 63, where=want["totals"] > 0)) >= 1 << 32
        assert int(want["totals"][0, 1]) == 300 * 0xFFFFFFFE and int(want["regret"][1, 0]) >= 0xFFFFFFFE
        check(probe, x, n_arms, 0, 1, 300, "0 and 0xFFFFFFFE", never_as=(NEVER,))


def test_settled_cells_are_not_read_and_change_nothing(probe):
    """Live cells between settled ones; a run of settled cells longer than a trip, of either kind; a single live cell at the end
    of the window.  live_cells is the count from the tables, and every output is the one without them."""
    rng = np.random.default_rng(11)
    for n_arms, reps in ((2, 3), (3, 14), (8, 17)):
        m, cells = n_arms * reps, 1500
        x = rng.integers(0, 1 << 20, size=(m, cells), dtype=np.uint64).astype(np.uint32)
        x[:, 1:600:2] = 0                                           # alternating: settled by the sums
        x[:, 2:600:4] = NEVER                                       # and by the members that reached the cell
        x[:, 600:1499] = 0                                          # a run of 899 settled cells
        x[:, 700:900] = NEVER
        x = np.ascontiguousarray(x)
        zero, never = tables(x)
        live = int(((zero != 0) & (never != 0)).sum())
        assert live == 151 and zero[1499] != 0 and never[1499] != 0 and zero[1498] == 0
        for maximize in (False, True):
            for na in NEVER_AS:
                want = ref.arms(x, n_arms, maximize, na)
                for grid in GRIDS:
                    plain, s0 = arms(probe, x, 0, 1, cells, n_arms, maximize, na, grid)
                    got, s1 = arms(probe, x, 0, 1, cells, n_arms, maximize, na, grid, (zero, never))
                    note = (n_arms, reps, maximize, na, grid)
                    same(plain, want, note)
                    same(got, want, note)
                    assert s0["live"] == cells and s0["common"] == 0 and s1["live"] == live, (note, s0, s1)
                    assert s1["common"] == 350 * na, (note, s1)      # the settled cells' keys: 150 + 200 cells at ESIM_NEVER, the others hold 0
        # the window [1400, 1500): one live cell, the last
        got, s1 = arms(probe, x, 14, 1, 100, n_arms, False, NEVER, 1, (zero, never))
        same(got, ref.arms(x[:, 1400:], n_arms), "the last cell")
        assert s1["live"] == 1
        # only one of the two tables
        for skip in ((zero, None), (None, never)):
            got, s1 = arms(probe, x, 0, 1, cells, n_arms, True, 0, 3, skip)
            same(got, ref.arms(x, n_arms, True, 0), "one table")
            assert s1["live"] == ref.live_cells(*skip, 0, cells)


def test_a_window_of_rows_inside_taller_planes(probe):
    """Rows [first_row, first_row + n_rows) of planes with more rows, as the library addresses the store; a window without rows
    gives zero totals and reads nothing."""
    for n_arms, reps, rows, cols, first_row, n_rows in ((3, 3, 12, 5, 2, 7), (2, 17, 9, 70, 3, 4), (5, 14, 6, 131, 1, 3), (6, 1, 40, 1, 13, 20), (16, 2, 5, 300, 4, 1)):
        x, _ = make_planes(n_arms * reps, rows * cols, 7 * n_arms + cols)
        check(probe, x, n_arms, first_row, n_rows, cols, "rows %d..%d of %d x %d" % (first_row, first_row + n_rows, rows, cols), never_as=(NEVER, 12345))
    x, _ = make_planes(12, 60, 1)
    for maximize in (False, True):
        got, stats = arms(probe, x, 4, 0, 5, 3, maximize, NEVER, 1)
        assert got["best"].shape == (3, 0) and not got["totals"].any() and not any(stats.values())


def test_the_probe_refuses_what_the_library_refuses(probe):
    x = np.zeros((12, 8), np.uint32)
    o32, o64, stats = np.zeros(2 * 16 * 8, np.uint32), np.zeros(3 * 16 * 8, np.uint64), np.zeros(2, np.uint64)
    p32, p64 = o32.ctypes.data_as(u32p), o64.ctypes.data_as(u64p)
    args = lambda n_arms, maximize=0, n_rows=2: (x.ctypes.data_as(u32p), 12, 8, 0, n_rows, 4, None, 0, None, n_arms, maximize, NEVER, 1, p32, p32, p64, p64, p64,
                                                  stats.ctypes.data_as(u64p))
    assert probe.arms_probe(*args(0)) == -1 and probe.arms_probe(*args(17)) == -1                 # no arms, too many
    assert probe.arms_probe(*args(5)) == -1 and probe.arms_probe(*args(8)) == -1                  # 12 members are no replicates of 5 or 8 arms
    assert probe.arms_probe(*args(3, maximize=2)) == -1 and probe.arms_probe(*args(3, n_rows=3)) == -1
    assert all(probe.arms_probe(*args(a)) == 0 for a in (1, 2, 3, 4, 6, 12))
