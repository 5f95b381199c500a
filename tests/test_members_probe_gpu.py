"""The selection and the exceedance kernels of esim_members.h on their own, against numpy: every value, no tolerance.
tests/native/members_probe.hip is compiled here, as test_curves_probe_gpu.py compiles its probe, and loaded with ctypes.  The
member counts are every padded size of the sorting network, one past each, and both sides of the seam between the register
kernels (up to 64 members) and the LDS kernels; the cell counts leave tails behind the 64-cell tiles of a wavefront and the
256-cell trips of a workgroup; a grid bound of 1 and of 3 workgroups makes 1000 cells take three trips or more."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import _members_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEMBERS = (1, 2, 7, 8, 9, 16, 17, 32, 33, 63, 64, 65, 128, 129, 255, 256)
CELLS = (1, 3, 4, 63, 64, 65, 257, 1000)
GRIDS = (1, 3)
KINDS = 8                                      # of cells the generator makes
u32p, u64p, i64p = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_int64)


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("members_probe") / "libmembers_probe.so")
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
           "-I", os.path.join(ROOT, "epidemicsimulator_amd", "csrc"), "-o", out, os.path.join(ROOT, "tests", "native", "members_probe.hip")]
    done = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert done.returncode == 0, done.stderr[-2000:]
    lib = ctypes.CDLL(out)
    lib.members_probe_select.restype = ctypes.c_int
    lib.members_probe_select.argtypes = [u32p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, u64p, ctypes.c_uint32, u32p, u32p, ctypes.c_uint32,
                                         ctypes.c_uint32, u32p]
    lib.members_probe_exceed.restype = ctypes.c_int
    lib.members_probe_exceed.argtypes = [u32p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, u64p, ctypes.c_uint32, u32p, i64p, ctypes.c_uint32,
                                         ctypes.c_int, ctypes.c_int, ctypes.c_uint32, u32p]
    assert int(ctypes.c_uint32.in_dll(lib, "members_max").value) == 256 and int(ctypes.c_uint32.in_dll(lib, "members_ranks_max").value) == 16
    return lib


def make_planes(m, cells, seed):
    """uint32 [m, cells] and the kind of every cell: 0 all zero, 1 one non-zero member, 2 all equal, 3 duplicates from a few
    values, 4 anything with 0xFFFFFFFF among it, 5 the signed-flipped range around 0x80000000, 6 all 0xFFFFFFFF, 7 anything."""
    rng = np.random.default_rng(seed)
    kind = np.arange(cells) % KINDS if cells >= KINDS else rng.integers(0, KINDS, size=cells)
    kind = rng.permutation(kind)
    x = np.zeros((m, cells), np.uint32)
    for c in range(cells):
        k = kind[c]
        if k == 1:
            x[rng.integers(0, m), c] = rng.integers(1, 500)
        elif k == 2:
            x[:, c] = rng.integers(0, 1 << 32, dtype=np.uint64)
        elif k == 3:
            x[:, c] = rng.choice(np.array([0, 1, 1, 2, 7, 400], np.uint32), size=m)
        elif k == 4:
            x[:, c] = rng.integers(0, 1 << 32, size=m, dtype=np.uint64)
            x[rng.integers(0, m), c] = ref.NEVER
        elif k == 5:
            x[:, c] = ref.to_key(rng.integers(-5, 6, size=m).astype(np.int32))
        elif k == 6:
            x[:, c] = ref.NEVER
        elif k == 7:
            x[:, c] = rng.integers(0, 1 << 32, size=m, dtype=np.uint64)
    return np.ascontiguousarray(x), kind


def rank_lists(m):
    """{0, M - 1, M // 2} with a repeated and an unsorted rank, and 16 ranks at once."""
    rng = np.random.default_rng(m)
    return [np.array([m - 1, 0, m // 2, 0], np.uint32), rng.integers(0, m, size=16).astype(np.uint32)]


def select(probe, x, first, n, ranks, grid, zero=None, never=None):
    m, stride = x.shape
    out = np.zeros((ranks.size, n), np.uint32)
    rc = probe.members_probe_select(x.ctypes.data_as(u32p), m, stride, first, n, None if zero is None else zero.ctypes.data_as(u64p), 0,
                                    None if never is None else never.ctypes.data_as(u32p), ranks.ctypes.data_as(u32p), ranks.size, grid, out.ctypes.data_as(u32p))
    assert rc == 0, rc
    return out


def exceed(probe, x, first, n, thresholds, grid, signed=False, has_never=False, zero=None, never=None):
    m, stride = x.shape
    thr = np.ascontiguousarray(thresholds, np.int64)
    out = np.zeros((thr.size, n), np.uint32)
    rc = probe.members_probe_exceed(x.ctypes.data_as(u32p), m, stride, first, n, None if zero is None else zero.ctypes.data_as(u64p), 0,
                                    None if never is None else never.ctypes.data_as(u32p), thr.ctypes.data_as(i64p), thr.size, int(signed), int(has_never), grid,
                                    out.ctypes.data_as(u32p))
    assert rc == 0, rc
    return out


@pytest.mark.parametrize("m", MEMBERS)
def test_every_value_equals_numpy(probe, m):
    for cells in CELLS:
        x, kind = make_planes(m, cells, 100 * m + cells)
        if cells >= KINDS:
            assert set(kind.tolist()) == set(range(KINDS))
        zero = np.ascontiguousarray(x.astype(np.uint64).sum(axis=0))                       # as the accumulators hold them: the sum,
        never = np.ascontiguousarray((x != ref.NEVER).sum(axis=0).astype(np.uint32))       # and the members that reached the cell
        if cells >= KINDS:
            assert (zero == 0).any() and (never == 0).any() and ((x != 0).sum(axis=0) == 1).any()
        mid = int(np.sort(x.reshape(-1))[x.size // 2])
        thresholds = [0, 1, mid, ref.NEVER, 1 << 40, -3]
        for grid in GRIDS:
            what = "m = %d, cells = %d, grid = %d" % (m, cells, grid)
            if cells == 1000:
                assert -(-cells // (grid * 256)) >= (3 if grid == 1 else 2) and -(-cells // (grid * 64)) >= 3   # trips of the workgroups' loops
            for ranks in rank_lists(m):
                want = ref.order_statistics(x, ranks)
                got = select(probe, x, 0, cells, ranks, grid)
                assert (got == want).all(), (what, "select", np.argwhere(got != want)[:8].tolist())
                got = select(probe, x, 0, cells, ranks, grid, zero=zero, never=never)
                assert (got == want).all(), (what, "select with the zero-skip", np.argwhere(got != want)[:8].tolist())
            for has_never in (False, True):
                want = ref.exceedance(x, thresholds, never=has_never)
                got = exceed(probe, x, 0, cells, thresholds, grid, has_never=has_never)
                assert (got == want).all(), (what, "exceed", has_never, np.argwhere(got != want)[:8].tolist())
                got = exceed(probe, x, 0, cells, thresholds, grid, has_never=has_never, zero=zero, never=never)
                assert (got == want).all(), (what, "exceed with the zero-skip", has_never, np.argwhere(got != want)[:8].tolist())
            signed_thr = [-(1 << 40), -(1 << 31), -3, 0, 2, (1 << 31) - 1, 1 << 31]
            want = ref.exceedance(ref.from_key(x), signed_thr)
            got = exceed(probe, x, 0, cells, signed_thr, grid, signed=True)
            assert (got == want).all(), (what, "signed exceed", np.argwhere(got != want)[:8].tolist())


def test_a_window_of_cells_and_sixteen_thresholds(probe):
    """Cells [first, first + n) of wider planes, as a range of rows of the store is addressed; nothing outside is written."""
    m, stride, first, n = 70, 1000, 129, 333
    x, _ = make_planes(m, stride, 7)
    zero = np.ascontiguousarray(x.astype(np.uint64).sum(axis=0))
    ranks = np.arange(16, dtype=np.uint32)[::-1].copy() * 4
    want = ref.order_statistics(x[:, first:first + n], ranks)
    for grid in GRIDS:
        assert (select(probe, x, first, n, ranks, grid) == want).all()
        assert (select(probe, x, first, n, ranks, grid, zero=zero) == want).all()
    thr = np.array([0, 1, 2, 3, 7, 8, 399, 400, 401, 1 << 31, (1 << 31) + 5, ref.NEVER - 1, ref.NEVER, 1 << 32, 1 << 33, -1], np.int64)
    for has_never in (False, True):
        assert (exceed(probe, x, first, n, thr, 3, has_never=has_never, zero=zero) == ref.exceedance(x[:, first:first + n], thr, never=has_never)).all()


def test_the_probe_refuses_what_the_library_refuses(probe):
    x = np.zeros((4, 8), np.uint32)
    out = np.zeros(8, np.uint32)
    bad = np.array([4], np.uint32)
    args = lambda ranks, n: (x.ctypes.data_as(u32p), 4, 8, 0, 8, None, 0, None, ranks.ctypes.data_as(u32p), n, 1, out.ctypes.data_as(u32p))
    assert probe.members_probe_select(*args(bad, 1)) == -1                       # a rank that is not below the members
    assert probe.members_probe_select(*args(np.zeros(17, np.uint32), 17)) == -1   # more ranks than a call takes
    assert probe.members_probe_select(*args(bad, 0)) == -1
