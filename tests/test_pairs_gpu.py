"""The pair engine of esim_pairs.h (hash-table insert, compaction, bitonic sort of 64-bit keys with their counts) on its own,
against numpy.unique: every key and every count, no tolerance.  tests/native/pairs_probe.hip is compiled here, as
test_rank_gpu.py compiles its probe, and loaded with ctypes.  The sizes walk the edges of the sort: one pair, one wavefront, one
tile of PAIR_SORT_TILE pairs in LDS, and several tiles, where the global steps and the tail in LDS run."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOP = 0xFFFFFFFEFFFFFFFE                       # the largest key the library can form: both words one below their sentinel


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("pairs_probe") / "libpairs_probe.so")
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
           "-I", os.path.join(ROOT, "epidemicsimulator_amd", "csrc"), "-o", out, os.path.join(ROOT, "tests", "native", "pairs_probe.hip")]
    done = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stderr[-2000:]
    lib = ctypes.CDLL(out)
    lib.pairs_probe.restype = ctypes.c_int
    lib.pairs_probe.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p,
                                ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]
    lib.tile = int(ctypes.c_uint32.in_dll(lib, "pairs_sort_tile").value)
    assert lib.tile >= 64 and lib.tile & (lib.tile - 1) == 0
    return lib


def log2_for(distinct):
    """The capacity the library would choose: the smallest power of two >= twice the keys, at least 64."""
    return max(6, int(2 * max(1, distinct) - 1).bit_length())


def run(probe, keys, log2_cap):
    keys = np.ascontiguousarray(keys, np.uint64)
    cap = 1 << log2_cap
    out_keys, out_counts = np.full(cap, 0xDEADBEEF, np.uint64), np.full(cap, 0xDEADBEEF, np.uint32)
    n_out, overflow = ctypes.c_uint32(7), ctypes.c_uint32(7)
    rc = probe.pairs_probe(keys.ctypes.data if keys.size else None, keys.size, log2_cap, out_keys.ctypes.data, out_counts.ctypes.data,
                           ctypes.byref(n_out), ctypes.byref(overflow))
    assert rc == 0, rc
    assert n_out.value <= cap
    return out_keys[:n_out.value], out_counts[:n_out.value], overflow.value


def exact(probe, keys, log2_cap=None, what=""):
    keys = np.asarray(keys, np.uint64)
    want_keys, want_counts = np.unique(keys, return_counts=True)
    got_keys, got_counts, overflow = run(probe, keys, log2_for(want_keys.size) if log2_cap is None else log2_cap)
    print("%s: %d keys, %d distinct, %d delivered, overflow %d" % (what, keys.size, want_keys.size, got_keys.size, overflow))
    assert overflow == 0, what
    assert got_keys.size == want_keys.size, (what, got_keys.size, want_keys.size)
    assert (got_keys == want_keys).all(), (what, np.flatnonzero(got_keys != want_keys)[:8].tolist())
    assert (got_counts == want_counts).all(), (what, np.flatnonzero(got_counts != want_counts)[:8].tolist())


def random_keys(distinct, copies, seed):
    """`distinct` different keys with both words in use, each between 1 and `copies` times, shuffled."""
    rng = np.random.default_rng(seed)
    keys = np.unique(rng.integers(0, 1 << 62, size=distinct + 64, dtype=np.uint64))[:distinct]
    assert keys.size == distinct
    keys = np.repeat(keys, rng.integers(1, copies + 1, size=distinct))
    return rng.permutation(keys)


@pytest.mark.parametrize("n", (0, 1, 63, 64, 65))
def test_a_few_keys(probe, n):
    exact(probe, random_keys(n, 1, 100 + n), what="n = %d" % n)
    if n:
        exact(probe, random_keys(max(1, n // 3), 5, 200 + n)[:n], what="n = %d with repeats" % n)


@pytest.mark.parametrize("tiles, more", ((1, -1), (1, 0), (1, 1), (2, 1), (3, 5), (4, 0)))
def test_around_the_sort_tile(probe, tiles, more):
    distinct = tiles * probe.tile + more
    exact(probe, random_keys(distinct, 3, 300 + distinct), what="%d T %+d distinct" % (tiles, more))


def test_one_key_five_thousand_times(probe):
    exact(probe, np.full(5000, 0x0000012300000456, np.uint64), what="5000 copies")


def test_keys_that_differ_in_one_word_only(probe):
    lo = np.arange(3000, dtype=np.uint64)
    exact(probe, np.concatenate([(lo << np.uint64(32)) | np.uint64(77), (lo[::2] << np.uint64(32)) | np.uint64(77)]), what="high word only")
    exact(probe, np.concatenate([(np.uint64(77) << np.uint64(32)) | lo, (np.uint64(77) << np.uint64(32)) | lo[::3]]), what="low word only")


def test_the_smallest_and_the_largest_key(probe):
    exact(probe, np.array([TOP, 0, TOP, 5, 0, TOP], np.uint64), what="0 and 0xFFFFFFFEFFFFFFFE")


@pytest.mark.parametrize("log2_cap", (6, 12))
def test_a_table_exactly_full(probe, log2_cap):
    cap = 1 << log2_cap
    exact(probe, random_keys(cap, 2, 400 + log2_cap), log2_cap=log2_cap, what="distinct = cap = %d" % cap)


@pytest.mark.parametrize("log2_cap", (6, 12))
def test_one_key_too_many_is_a_bounded_error(probe, log2_cap):
    cap = 1 << log2_cap
    keys = random_keys(cap + 1, 1, 500 + log2_cap)
    got_keys, got_counts, overflow = run(probe, keys, log2_cap)
    print("distinct = cap + 1 = %d: %d delivered, overflow %d" % (cap + 1, got_keys.size, overflow))
    assert overflow >= 1 and got_keys.size == cap and overflow + int(got_counts.sum()) == keys.size
    assert (got_keys[1:] > got_keys[:-1]).all() and np.isin(got_keys, keys).all() and (got_counts == 1).all()
