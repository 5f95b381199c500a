"""The ranking routines of esim_rank.h (riders of a bus route by (Philox key, id)) on their own, against numpy.lexsort: every
rank, no tolerance.  tests/native/rank_probe.hip is compiled here, as test_kernel_resources.py compiles, and loaded with ctypes.
Both forms count `key_i < key` only and take an exact loop when they find that two riders were given one rank; the probe says
whether that loop ran, and the cases with equal keys must have taken it -- in the library a tie comes about once in 10^7 pairs,
so nothing else would ever walk that path."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WAVE, BLOCK = 0, 1
TOP = 0xFFFFFFFF


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("rank_probe") / "librank_probe.so")
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
           "-I", os.path.join(ROOT, "epidemicsimulator_amd", "csrc"), "-o", out, os.path.join(ROOT, "tests", "native", "rank_probe.hip")]
    done = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stderr[-2000:]
    lib = ctypes.CDLL(out)
    lib.rank_probe.restype = ctypes.c_int
    lib.rank_probe.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    return lib


def expected_ranks(keys):
    ids = np.arange(keys.size)
    order = np.lexsort((ids, keys))            # by key, then by id
    ranks = np.empty(keys.size, np.uint32)
    ranks[order] = np.arange(keys.size, dtype=np.uint32)
    return ranks


def key_sets(sz):
    """name -> (keys, whether two of them are equal; None: look)"""
    rng = np.random.default_rng(1000 + sz)
    distinct = rng.permutation(np.arange(1, 40 * sz + 1, 40, dtype=np.uint64)).astype(np.uint32) * np.uint32(1000003)
    assert np.unique(distinct).size == sz
    sets = {"distinct": (distinct, False), "all_equal": (np.full(sz, 12345, np.uint32), sz > 1),
            "all_top": (np.full(sz, TOP, np.uint32), sz > 1)}
    sets["edges_mixed"] = (rng.choice(np.array([0, 1, TOP - 1, TOP], np.uint32), sz), None)
    if sz > 20:
        # exactly two equal keys, at ranks 19 and 20 (the last of one bus of 20 and the first of the next): ascending keys at
        # shuffled places, the 19th and 20th smallest made equal
        asc = np.arange(sz, dtype=np.uint32) * np.uint32(7919) + np.uint32(11)
        asc[20] = asc[19]
        two = np.empty(sz, np.uint32)
        two[rng.permutation(sz)] = asc
        assert np.unique(two).size == sz - 1 and sorted(expected_ranks(two)[two == asc[19]].tolist()) == [19, 20]
        sets["two_equal_19_20"] = (two, True)
    return sets


def check(probe, form, sz):
    for name, (keys, tie) in key_sets(sz).items():
        keys = np.ascontiguousarray(keys, np.uint32)
        ranks = np.full(sz, 0xDEADBEEF, np.uint32)
        exact = ctypes.c_uint32(7)
        rc = probe.rank_probe(keys.ctypes.data, sz, form, ranks.ctypes.data, ctypes.byref(exact))
        assert rc == 0, (name, sz, rc)
        want = expected_ranks(keys)
        print("form %d sz %d %s: %d ranks differ, exact path %d" % (form, sz, name, int((ranks != want).sum()), exact.value))
        assert (ranks == want).all(), (name, sz, np.flatnonzero(ranks != want)[:8].tolist())
        if tie is None:
            tie = np.unique(keys).size < sz
        assert exact.value == (1 if tie else 0), (name, sz, exact.value)


@pytest.mark.timeout(120)
@pytest.mark.parametrize("sz", (1, 2, 20, 21, 40, 41, 63, 64))
def test_wavefront_form_ranks_by_key_then_id(probe, sz):
    check(probe, WAVE, sz)


@pytest.mark.timeout(120)
@pytest.mark.parametrize("sz", (65, 200))
def test_workgroup_form_ranks_by_key_then_id(probe, sz):
    check(probe, BLOCK, sz)
