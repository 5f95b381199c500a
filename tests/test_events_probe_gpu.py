"""The parts of the event engine that need nothing but a pair table (the compaction with a threshold of esim_pairs.h, the size
table and the order by size of esim_kernels_events.h) on their own, on synthetic keys against numpy: every key, every count and
every bin, no tolerance.  tests/native/events_probe.hip is compiled here, as test_pairs_gpu.py compiles its probe, and loaded
with ctypes.  The sizes walk the edges of the sort, the counts the clamp of the last bin."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
u32p = ctypes.POINTER(ctypes.c_uint32)


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("events_probe") / "libevents_probe.so")
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-I", os.path.join(ROOT, "epidemicsimulator_amd", "csrc"),
           "-I", os.path.join(ROOT, "include"), "-o", out, os.path.join(ROOT, "tests", "native", "events_probe.hip")]
    done = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stderr[-2000:]
    lib = ctypes.CDLL(out)
    lib.events_probe.restype = ctypes.c_int
    lib.events_probe.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                 u32p, u32p, ctypes.c_void_p, u32p]
    lib.tile = int(ctypes.c_uint32.in_dll(lib, "events_sort_tile").value)
    lib.bins = int(ctypes.c_uint32.in_dll(lib, "events_bins").value)
    assert lib.tile >= 64 and lib.tile & (lib.tile - 1) == 0 and lib.bins == 256
    return lib


def run(probe, keys, min_count=1, plain=False, by_size=False):
    """(keys, counts, size table, kernels launched behind the compaction) from a table never more than half full."""
    keys = np.ascontiguousarray(keys, np.uint64)
    log2_cap = max(6, int(2 * max(1, np.unique(keys).size) - 1).bit_length())
    cap = 1 << log2_cap
    out_keys, out_counts = np.full(cap, 0xDEADBEEF, np.uint64), np.full(cap, 0xDEADBEEF, np.uint32)
    sizes = np.full(4 * probe.bins, 0xDEADBEEF, np.uint32)
    n_out, overflow, launches = ctypes.c_uint32(7), ctypes.c_uint32(7), ctypes.c_uint32(7)
    rc = probe.events_probe(keys.ctypes.data if keys.size else None, keys.size, log2_cap, min_count, int(plain), int(by_size), out_keys.ctypes.data,
                            out_counts.ctypes.data, ctypes.byref(n_out), ctypes.byref(overflow), sizes.ctypes.data, ctypes.byref(launches))
    assert rc == 0 and overflow.value == 0 and n_out.value <= cap, (rc, overflow.value, n_out.value)
    assert (out_keys[n_out.value:] == 0xDEADBEEF).all() and (out_counts[n_out.value:] == 0xDEADBEEF).all()
    return out_keys[:n_out.value], out_counts[:n_out.value], sizes.reshape(4, probe.bins), launches.value


def expected(keys, min_count=1, by_size=False, bins=256):
    keys = np.asarray(keys, np.uint64)
    k, c = np.unique(keys, return_counts=True)
    table = np.bincount(((k >> np.uint64(32)) & np.uint64(3)).astype(np.int64) * bins + np.minimum(c, bins - 1), minlength=4 * bins).reshape(4, bins)
    keep = c >= min_count
    k, c = k[keep], c[keep]
    if by_size:
        order = np.lexsort((k, -c.astype(np.int64)))
        k, c = k[order], c[order]
    return k, c, table


def exact(probe, keys, min_count=1, plain=False, by_size=False, what=""):
    got_k, got_c, got_t, launches = run(probe, keys, min_count, plain, by_size)
    want_k, want_c, want_t = expected(keys, min_count, by_size, probe.bins)
    print("%s: %d keys, min_count %d, %d events expected, %d delivered, %d launches" % (what, np.asarray(keys).size, min_count, want_k.size, got_k.size, launches))
    assert got_k.size == want_k.size, (what, got_k.size, want_k.size)
    assert (got_k == want_k).all(), (what, np.flatnonzero(got_k != want_k)[:8].tolist())
    assert (got_c == want_c).all(), (what, np.flatnonzero(got_c != want_c)[:8].tolist())
    assert (got_t == want_t).all(), (what, np.argwhere(got_t != want_t)[:8].tolist())
    assert (launches == 0) == (want_k.size == 0), (what, launches)
    return got_k, got_c


def event_keys(distinct, copies, seed):
    """`distinct` different keys shaped as the library forms them (step << 34 | setting << 32 | place), each between 1 and
    `copies` times, shuffled."""
    rng = np.random.default_rng(seed)
    keys = np.unique((rng.integers(1, 1 << 20, size=distinct + 64, dtype=np.uint64) << np.uint64(34)) | (rng.integers(0, 4, size=distinct + 64, dtype=np.uint64) << np.uint64(32))
                     | rng.integers(0, 1 << 24, size=distinct + 64, dtype=np.uint64))
    keys = rng.permutation(keys)[:distinct]
    assert keys.size == distinct
    return rng.permutation(np.repeat(keys, rng.integers(1, copies + 1, size=distinct)))


def sizes_around(tile):
    return (0, 1, 63, 64, 65, tile - 1, tile, tile + 1, 2 * tile + 1)


@pytest.mark.parametrize("which", range(9))
def test_events_at_the_edges_of_the_sort(probe, which):
    n = sizes_around(probe.tile)[which]
    keys = event_keys(n, 4, 100 + which)
    for by_size in (False, True):
        exact(probe, keys, by_size=by_size, what="n = %d, by_size %s" % (n, by_size))
    # with a threshold of 2 about five in eight remain: the list is the filtered one, the table still counts every event
    exact(probe, keys, min_count=2, what="n = %d, min_count 2" % n)
    exact(probe, keys, min_count=3, by_size=True, what="n = %d, min_count 3 by size" % n)


@pytest.mark.parametrize("which", range(9))
def test_all_counts_equal_so_that_the_order_is_by_key(probe, which):
    n = sizes_around(probe.tile)[which]
    keys = np.repeat(event_keys(n, 1, 200 + which), 3)
    by_key = exact(probe, keys, what="n = %d, three copies each" % n)
    by_size = exact(probe, keys, by_size=True, what="n = %d, three copies each, by size" % n)
    assert (by_key[0] == by_size[0]).all() and (by_size[1] == 3).all()


def test_the_last_bin_is_open_ended(probe):
    base = event_keys(4, 1, 300)
    keys = np.concatenate([np.repeat(base[i], c) for i, c in enumerate((254, 255, 256, 300))] + [event_keys(70, 3, 301)])
    _, _, table, _ = run(probe, keys)
    want = expected(keys, bins=probe.bins)[2]
    assert (table == want).all() and int(table[:, 254].sum()) == 1 and int(table[:, 255].sum()) == 3 and int(table[:, 0].sum()) == 0
    got = exact(probe, keys, by_size=True, what="254, 255, 256 and 300 copies")
    assert got[1][:4].tolist() == [300, 256, 255, 254]                 # the list carries the true sizes
    exact(probe, keys, min_count=255, what="min_count 255")
    exact(probe, keys, min_count=256, by_size=True, what="min_count 256 by size")


def test_min_count_one_is_the_plain_compaction(probe):
    for n in (0, 1, 65, probe.tile + 1):
        keys = event_keys(n, 5, 400 + n)
        plain, mine = run(probe, keys, plain=True), run(probe, keys, min_count=1)
        assert (plain[0] == mine[0]).all() and (plain[1] == mine[1]).all() and (plain[2] == mine[2]).all()
        exact(probe, keys, plain=True, what="k_pairs_compact, n = %d" % n)


def test_a_threshold_above_every_count_delivers_nothing_and_sorts_nothing(probe):
    keys = event_keys(probe.tile + 5, 4, 500)
    for by_size in (False, True):
        got_k, got_c, table, launches = run(probe, keys, min_count=5, by_size=by_size)
        assert got_k.size == 0 and launches == 0 and (table == expected(keys, bins=probe.bins)[2]).all() and int(table.sum()) == probe.tile + 5


def test_keys_that_differ_in_the_setting_bits_only(probe):
    place = np.arange(700, dtype=np.uint64) * np.uint64(3)
    step = np.uint64(123) << np.uint64(34)
    keys = np.concatenate([step | (np.uint64(s) << np.uint64(32)) | place[::s + 1] for s in range(4)] + [step | (np.uint64(2) << np.uint64(32)) | place[:100]])
    got = exact(probe, keys, what="four settings at one step")
    assert (np.diff(((got[0] >> np.uint64(32)) & np.uint64(3)).astype(np.int64)) >= 0).all()    # at one step the settings ascend
    exact(probe, keys, min_count=2, by_size=True, what="four settings at one step, min_count 2 by size")
    table = run(probe, keys)[2]
    assert table.sum(axis=1).tolist() == [700, 350, 234 + 100 - 34, 175] and int(table[2, 2]) == 34
