"""k_ensemble_fold_ratio on its own, on synthetic planes against numpy: every counter and every sum of every cell, no tolerance.
tests/native/ratio_probe.hip is compiled here, as test_events_probe_gpu.py compiles its probe, and loaded with ctypes.  The cell
counts walk the tail behind the last whole four and the second workgroup, a grid of one workgroup walks the stride loop, and the
planes hold the edges of the ratio test and of the 64-bit sums."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import _ens_transmission_ref as ens_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ens_ref.REPRODUCTION_KEYS
SUMS = KEYS[2:]
FULL = 0xFFFFFFFF


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("ratio_probe") / "libratio_probe.so")
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-I", os.path.join(ROOT, "epidemicsimulator_amd", "csrc"),
           "-I", os.path.join(ROOT, "include"), "-o", out, os.path.join(ROOT, "tests", "native", "ratio_probe.hip")]
    done = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stderr[-2000:]
    lib = ctypes.CDLL(out)
    lib.ratio_probe.restype = ctypes.c_int
    lib.ratio_probe.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64] + [ctypes.c_uint32] * 5 + [ctypes.c_void_p] * 5
    return lib


def fold(probe, planes, min_cohort=1, r=(1, 1), grid=0, start=None):
    """The accumulators after the planes [(cases, offspring), ...] were folded one after another, from `start` (None: zero)."""
    c = np.ascontiguousarray([p[0] for p in planes], np.uint32)
    o = np.ascontiguousarray([p[1] for p in planes], np.uint32)
    cells = c.shape[1]
    members = np.array([0 if start is None else start["members"]], np.uint32)
    words = {k: np.zeros(cells, np.uint32) if start is None else np.ascontiguousarray(start[k], np.uint32).copy() for k in KEYS[:2]}
    sums = np.zeros((5, cells), np.uint64) if start is None else np.ascontiguousarray([start[k] for k in SUMS], np.uint64)
    rc = probe.ratio_probe(c.ctypes.data, o.ctypes.data, cells, len(planes), grid, min_cohort, r[0], r[1], members.ctypes.data, words["defined"].ctypes.data,
                           words["hit"].ctypes.data, sums.ctypes.data, None)
    assert rc == 0, rc
    return dict(words, members=int(members[0]), **{k: sums[i] for i, k in enumerate(SUMS)})


def planes_of(cells, n, seed, zero_share=0.5):
    """n members of synthetic cohort rows: about zero_share of the cells empty, offspring without cases among the others (the
    kernel must not rely on offspring > 0 implying cases > 0), runs of empty cells so that whole groups of four are skipped."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        c = rng.integers(0, 40, size=cells, dtype=np.uint32)
        o = rng.integers(0, 90, size=cells, dtype=np.uint32)
        empty = rng.random(cells) < zero_share
        empty |= np.repeat(rng.random((cells + 7) // 8) < 0.3, 8)[:cells]
        c[empty] = 0
        o[empty] = 0
        c[rng.random(cells) < 0.05] = 0
        out.append((c, o))
    return out


def exact(probe, planes, min_cohort, r, grid=0, what=""):
    got = fold(probe, planes, min_cohort, r, grid)
    ens_ref.same_fold(got, ens_ref.fold_reproduction(planes, min_cohort, r), KEYS, what)
    return got


@pytest.mark.parametrize("cells", (1, 3, 4, 5, 255, 1027))
def test_cell_counts_around_the_tail_and_the_second_workgroup(probe, cells):
    for min_cohort in (1, 5):
        for r in ((1, 1), (0, 1), (3, 2)):
            planes = planes_of(cells, 3, 1000 + cells)                 # three folds in a row
            got = exact(probe, planes, min_cohort, r, what="%d cells, min_cohort %d, r %s" % (cells, min_cohort, r))
            assert got["members"] == 3
            if r == (0, 1):
                assert (got["hit"] == got["defined"]).all()
    some = np.stack([p[0] for p in planes])
    assert cells < 255 or (((np.stack([p[1] for p in planes]) > 0) & (some == 0)).any() and (some == 0).any() and (some >= 5).any())


def test_a_grid_of_one_workgroup_strides_over_5000_cells(probe):
    planes = planes_of(5000, 3, 7)
    one = exact(probe, planes, 5, (3, 2), grid=1, what="grid of one workgroup")
    wide = exact(probe, planes, 5, (3, 2), what="the library's grid")
    ens_ref.same_fold(one, wide, KEYS, "one workgroup against five")
    assert one["hit"].any() and (one["defined"] > one["hit"]).any() and (one["defined"] < 3).any()


def test_all_zero_planes_leave_the_accumulators_as_they_are(probe):
    for cells in (3, 1027):
        zero = [(np.zeros(cells, np.uint32), np.zeros(cells, np.uint32))] * 2
        got = fold(probe, zero, 1, (0, 1))
        assert got["members"] == 2 and all(not got[k].any() for k in KEYS)                # from a zero start: nothing but the member counter
        # ... and from accumulators that three members filled: every cell as it was
        before = ens_ref.fold_reproduction(planes_of(cells, 3, 50 + cells), 1, (1, 1))
        after = fold(probe, zero, 1, (1, 1), start=before)
        ens_ref.same_fold(after, dict(before, members=5), KEYS, "two empty members on top of three")


def test_the_ratio_at_its_threshold_and_one_either_side(probe):
    # o * r_den == c * r_num exactly, one offspring less, one more; with large factors too (the products need 64 bits)
    c = np.array([2, 2, 2, 4, 4, 4, 200000, 200000, 200000, 6, 0, 0, 1], np.uint32)
    o = np.array([3, 2, 4, 6, 5, 7, 300000, 299999, 300001, 0, 3, 0, 0], np.uint32)
    got = exact(probe, [(c, o)], 1, (3, 2), what="r = 3/2")
    assert got["hit"].tolist() == [1, 0, 1, 1, 0, 1, 1, 0, 1, 0, 0, 0, 0] and got["defined"].tolist() == [1] * 10 + [0, 0, 1]
    got = exact(probe, [(c, o)], 1, (3000000000, 2000000000), what="r = 3e9/2e9")
    assert got["hit"].tolist() == [1, 0, 1, 1, 0, 1, 1, 0, 1, 0, 0, 0, 0]
    got = exact(probe, [(c, o)], 5, (1, 1), what="min_cohort 5")
    assert got["defined"].tolist() == [0] * 6 + [1, 1, 1, 1, 0, 0, 0] and got["hit"].tolist() == [0] * 6 + [1, 1, 1, 0, 0, 0, 0]
    assert got["sum_offspring"][10] == 3 and got["sum_cases"][10] == 0 and got["sumsq_offspring"][10] == 9     # offspring without cases still sums


def test_the_largest_counts_fit_the_64_bit_sums(probe):
    for cells, at in ((5, 4), (8, 2), (1, 0)):                          # in the tail, in a whole four, alone
        c, o = np.zeros(cells, np.uint32), np.zeros(cells, np.uint32)
        c[at] = o[at] = FULL
        small = planes_of(cells, 2, 90 + cells, zero_share=0.0)
        small[0][0][at] = small[0][1][at] = small[1][0][at] = small[1][1][at] = 0     # the cell is folded once
        got = exact(probe, [small[0], (c, o), small[1]], 1, (1, 1), what="0xFFFFFFFF in cell %d of %d" % (at, cells))
        assert int(got["sumsq_cases"][at]) == FULL * FULL and int(got["sum_cross"][at]) == FULL * FULL and int(got["sum_offspring"][at]) == FULL
        assert got["hit"][at] == 1 and got["defined"][at] == 1
        # r_num and r_den at their largest: both products are (2^32 - 1)^2
        assert exact(probe, [(c, o)], FULL, (FULL, FULL), what="largest factors")["hit"][at] == 1
