"""The paired policy comparison on the device: esim_baseline_keep / _info / _drop, esim_compare, esim_compare_series, the paired
kind of the ensemble accumulators and Ensemble.compare.  Every comparison of device output is exact integer equality against
tests/_compare_ref.py -- two CPU-oracle runs reduced to an exposure step per citizen, and numpy on those --, on the worlds and
pairs that tests/test_policy_compare.py shows not to be vacuous.  tests/native/compare_probe.hip runs the kernels on their own,
on synthetic planes: the populations of 1 to 257 citizens (the four-per-lane tail, the wavefront edges) and a build whose LDS
window of areas is two areas wide, so that the direct path to the global table carries nearly every area."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _compare_ref as cr
import _oracle
import _setting_ref as ref_mod
from epidemicsimulator_amd import Ensemble, Population, Simulator, _lib
from epidemicsimulator_amd.ensemble import paired_summary

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ESTATE, ERANGE = -1, -4, -5
NEVER = _lib.NEVER
ALL, HOME, GROUP = _lib.BY_ALL, _lib.AREA_HOME, _lib.BY_GROUP
B, AV, AD, E, L = _lib.CMP_BOTH, _lib.CMP_AVERTED, _lib.CMP_ADDED, _lib.CMP_EARLIER, _lib.CMP_LATER
u8p, u32p, u64p, i64p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_int64)
KEYS = cr.PAIRED_KEYS


def run_arm(sim, ep, over, n):
    """The simulator at the end of n steps under the world's parameters changed by `over`."""
    sim.restart(ref_mod.copy_params(ep), **over)
    return sim.run(n)


def both_arms(world, pair, level=None):
    pop, ep, n, over_b, over_c, b, rec_b, c, rec_c = cr.cached(world, pair)
    sim = Simulator(pop, ref_mod.copy_params(ep))
    if level is not None:
        sim.set_pipeline(level)
    got_b = run_arm(sim, ep, over_b, n)
    sim.keep_baseline()
    got_c = run_arm(sim, ep, over_c, n)
    return sim, pop, n, b, c, (got_b, rec_b), (got_c, rec_c)


def same_compare(got, want, what, cls=True):
    assert np.array_equal(got["counts"], want["counts"]), (what, got["counts"][:4], want["counts"][:4])
    assert np.array_equal(got["delay"], want["delay"]), (what, got["delay"][:4], want["delay"][:4])
    assert got["first_divergence"] == want["first_divergence"], (what, got["first_divergence"], want["first_divergence"])
    if cls:
        bad = np.flatnonzero(got["cls"] != want["cls"])
        assert bad.size == 0, (what, bad[:5], got["cls"][bad[:5]], want["cls"][bad[:5]])


def groups_of(pop, g):
    return (np.arange(pop.n_citizens) % g).astype(np.uint16), g


# ---- 1. the worlds against the reference ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", (0, None), ids=("level0", "default"))
@pytest.mark.parametrize("world,pair", cr.WORLD_PAIRS)
def test_worlds_against_the_reference(world, pair, level):
    sim, pop, n, b, c, arm_b, arm_c = both_arms(world, pair, level)
    check_world(sim, pop, n, b, c, arm_b, arm_c, world, pair)
    sim.close()


def check_world(sim, pop, n, b, c, arm_b, arm_c, world, pair):
    """Every comparison of a world with both arms run and the baseline kept (both_arms) against the reference."""
    for got, want in (arm_b, arm_c):                                  # (the runs themselves are the oracle's)
        assert len(got) == n and all((got[f] == want[f]).all() for f in ("susceptible", "exposures_building", "exposures_bus", "vaccinated"))
    info = sim.baseline_info()
    assert info["steps"] == n and info["n_cases"] == int((b != NEVER).sum()) and info["params"].seed == sim.params.seed - (1 if pair == "seed" else 0)
    windows = ((0, n), (1, n), (n // 3, 2 * n // 3))
    by_all = {}
    for where, g in (("all", 0), ("home", 0), ("group", 1), ("group", 7), ("group", 1024)):
        labels, n_groups = groups_of(pop, g) if g else (None, 0)
        if g:
            sim.set_groups(labels, n_groups)
        col, n_cols = cr.columns(pop, where, labels, n_groups)
        for first, last in windows:
            want = cr.compare(b, c, col, n_cols, first, last)
            got = sim.compare(where, first, last, citizens=True)
            same_compare(got, want, (world, pair, where, g, first, last))
            # the columns add up to the by-all row
            if where == "all":
                by_all[(first, last)] = got
            else:
                assert (got["counts"].sum(0) == by_all[(first, last)]["counts"][0]).all() and got["delay"].sum() == by_all[(first, last)]["delay"][0]
        # the event rows of both runs
        if g in (1, 1024):
            continue
        for stride in (1, 24, 7):
            for first in (0, 5):
                for cumulative in (False, True):
                    n_rows = (n - first) // stride + 1
                    want_b, want_c = cr.series(b, c, col, n_cols, first, n_rows, stride, cumulative)
                    got_b, got_c = sim.compare_series(where, first, None, stride, cumulative)
                    assert got_b.shape == want_b.shape and np.array_equal(got_b, want_b) and np.array_equal(got_c, want_c), (world, pair, where, g, stride, first, cumulative)
    # identities: the window of the whole run holds every log entry of either run; the rows are the records' exposures; the last
    # cumulative row is the window's counts
    whole = by_all[(0, n)]["counts"][0]
    events = sim.exposure_events()
    assert whole[B] + whole[AV] == info["n_cases"] and whole[B] + whole[AD] == len(events[0]) + len(sim.seeds())
    rows_b, rows_c = sim.compare_series("all", 1, n, 1)
    for rows, (rec, _) in ((rows_b, arm_b), (rows_c, arm_c)):
        assert (rows[:, 0] == rec["exposures_building"].astype(np.int64) + rec["exposures_bus"]).all()
    cum_b, cum_c = sim.compare_series("home", 0, None, 24, True)
    t = sim.compare("home", 0, n)["counts"]
    assert (cum_b[-1] == t[:, B] + t[:, AV]).all() and (cum_c[-1] == t[:, B] + t[:, AD]).all()


def test_each_output_alone_and_none():
    sim, pop, n, b, c, _, _ = both_arms("situations", "lockdown")
    lib, ctx = sim.lib, sim._ctx
    col, n_cols = cr.columns(pop, "home")
    first, last = 100, 400
    want = cr.compare(b, c, col, n_cols, first, last)
    counts, delay, div, cls = np.full((n_cols, 5), 7, np.uint64), np.full(n_cols, 7, np.int64), C.c_uint32(7), np.full(pop.n_citizens, 7, np.uint8)
    ptrs = (counts.ctypes.data_as(u64p), delay.ctypes.data_as(i64p), C.byref(div), cls.ctypes.data_as(u8p))
    for i in range(4):
        args = [None] * 4
        args[i] = ptrs[i]
        assert lib.esim_compare(ctx, HOME, first, last, *args) == 0, i
    assert np.array_equal(counts, want["counts"]) and np.array_equal(delay, want["delay"]) and div.value == want["first_divergence"] and np.array_equal(cls, want["cls"])
    assert lib.esim_compare(ctx, HOME, first, last, None, None, None, None) == 0
    want_b, want_c = cr.series(b, c, col, n_cols, 5, 3, 100)
    rows = np.full((3, n_cols), 7, np.uint32)
    assert lib.esim_compare_series(ctx, HOME, 5, 3, 100, 0, rows.ctypes.data_as(u32p), None) == 0 and np.array_equal(rows, want_b)
    assert lib.esim_compare_series(ctx, HOME, 5, 3, 100, 0, None, rows.ctypes.data_as(u32p)) == 0 and np.array_equal(rows, want_c)
    assert lib.esim_compare_series(ctx, HOME, 5, 3, 100, 0, None, None) == 0
    sim.close()


# ---- 2. the kernels on their own: small populations, a shrunken LDS window -----------------------------------------------------
@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("compare_probe") / "libcompare_probe.so")
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-DCOMPARE_AREA_WINDOW=2", "-I", os.path.join(ROOT, "epidemicsimulator_amd", "csrc"),
           "-I", os.path.join(ROOT, "include"), "-o", out, os.path.join(ROOT, "tests", "native", "compare_probe.hip")]
    done = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stderr[-2000:]
    lib = C.CDLL(out)
    lib.compare_probe.restype = C.c_int
    lib.compare_probe.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_int] + [C.c_uint32] * 4 + [C.c_void_p] * 4
    lib.compare_rows_probe.restype = C.c_int
    lib.compare_rows_probe.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_int] + [C.c_uint32] * 4 + [C.c_int, C.c_uint32, C.c_void_p, C.c_void_p]
    lib.compare_probe_window.restype = C.c_uint32
    assert lib.compare_probe_window() == 2
    return lib


def probe_compare(probe, b, c, home, bld_area, where, n_cols, first, last, labels=None, per_block=1024):
    n = len(b)
    b, c, home, bld_area = (np.ascontiguousarray(a, np.uint32) for a in (b, c, home, bld_area))
    grp = None if labels is None else np.ascontiguousarray(labels, np.uint16)
    counts, delay, div, cls = np.zeros((n_cols, 5), np.uint32), np.zeros(n_cols, np.int64), np.zeros(1, np.uint32), np.zeros(n, np.uint8)
    rc = probe.compare_probe(b.ctypes.data, c.ctypes.data, n, home.ctypes.data, bld_area.ctypes.data, len(bld_area), None if grp is None else grp.ctypes.data,
                             {"all": ALL, "home": HOME, "group": GROUP}[where], n_cols, first, last, per_block, counts.ctypes.data, delay.ctypes.data, div.ctypes.data,
                             cls.ctypes.data)
    assert rc == 0, rc
    return {"counts": counts.astype(np.uint64), "delay": delay, "first_divergence": None if div[0] == NEVER else int(div[0]), "cls": cls}


def probe_rows(probe, b, c, home, bld_area, where, n_cols, first, n_rows, stride, cumulative, labels=None, grid=0):
    n = len(b)
    b, c, home, bld_area = (np.ascontiguousarray(a, np.uint32) for a in (b, c, home, bld_area))
    grp = None if labels is None else np.ascontiguousarray(labels, np.uint16)
    rows_b, rows_c = np.zeros((n_rows, n_cols), np.uint32), np.zeros((n_rows, n_cols), np.uint32)
    rc = probe.compare_rows_probe(b.ctypes.data, c.ctypes.data, n, home.ctypes.data, bld_area.ctypes.data, len(bld_area), None if grp is None else grp.ctypes.data,
                                  {"all": ALL, "home": HOME, "group": GROUP}[where], n_cols, first, n_rows, stride, int(cumulative), grid, rows_b.ctypes.data, rows_c.ctypes.data)
    assert rc == 0, rc
    return rows_b, rows_c


def made_up_planes(n, seed, steps=60, share=0.6):
    """Two planes of a made-up pair of runs over n citizens: most of them cases of at least one run, a few index cases, every class
    and both signs of the delay present where n allows."""
    rng = np.random.default_rng(seed)
    b = rng.integers(1, steps + 1, size=n).astype(np.uint32)
    c = np.where(rng.random(n) < 0.5, b, rng.integers(1, steps + 1, size=n)).astype(np.uint32)
    b[rng.random(n) > share] = NEVER
    c[rng.random(n) > share] = NEVER
    seeds = rng.random(n) < 0.1
    b[seeds] = 0
    c[seeds] = 0
    return b, c


@pytest.mark.parametrize("n", (1, 3, 5, 63, 64, 65, 257))
def test_small_populations_around_the_tail_and_the_wavefront_edges(probe, n):
    """Hand-built populations: households of three, an area per four households."""
    home = np.arange(n) // 3
    bld_area = np.arange(home.max() + 1) // 4
    n_areas = int(bld_area.max()) + 1
    labels = (np.arange(n) % 5).astype(np.uint16)
    seen = np.zeros(5, np.int64)
    for seed in range(4):
        b, c = made_up_planes(n, 10 * n + seed)
        for where, lab, g in (("all", None, 0), ("home", None, 0), ("group", labels, 5)):
            col, n_cols = (home_col(home, bld_area), n_areas) if where == "home" else cr.columns(FakePop(n), where, lab, g)
            for first, last in ((0, 60), (1, 60), (20, 40), (60, 60)):
                want = cr.compare(b, c, col, n_cols, first, last)
                same_compare(probe_compare(probe, b, c, home, bld_area, where, n_cols, first, last, lab), want, (n, seed, where, first, last))
                seen += want["counts"].sum(0).astype(np.int64)
            for first, stride, cumulative in ((0, 1, False), (0, 7, True), (5, 24, False), (5, 3, True)):
                n_rows = (60 - first) // stride + 1
                want_b, want_c = cr.series(b, c, col, n_cols, first, n_rows, stride, cumulative)
                got_b, got_c = probe_rows(probe, b, c, home, bld_area, where, n_cols, first, n_rows, stride, cumulative, lab)
                assert np.array_equal(got_b, want_b) and np.array_equal(got_c, want_c), (n, seed, where, first, stride, cumulative)
    assert n < 63 or seen.all()                                      # every class occurred


class FakePop:
    def __init__(self, n):
        self.n_citizens = n


def home_col(home, bld_area):
    return np.asarray(bld_area)[np.asarray(home)].astype(np.int64)


def test_identical_and_disjoint_planes(probe):
    n = 1027
    home, bld_area = np.arange(n) // 3, np.arange(n // 3 + 1) // 4
    b, _ = made_up_planes(n, 1)
    col = np.zeros(n, np.int64)
    got = probe_compare(probe, b, b, home, bld_area, "all", 1, 0, 60)
    same_compare(got, cr.compare(b, b, col, 1, 0, 60), "identical")
    assert got["first_divergence"] is None and not got["counts"][0, 1:].any() and got["delay"][0] == 0
    never = np.full(n, NEVER, np.uint32)
    for x, y, k in ((b, never, AV), (never, b, AD)):
        got = probe_compare(probe, x, y, home, bld_area, "all", 1, 0, 60)
        same_compare(got, cr.compare(x, y, col, 1, 0, 60), "disjoint")
        assert got["counts"][0, k] == (b != NEVER).sum() and got["counts"][0].sum() == got["counts"][0, k] and got["first_divergence"] == 0
    got = probe_compare(probe, never, never, home, bld_area, "all", 1, 0, 60)
    assert not got["counts"].any() and got["first_divergence"] is None and not got["cls"].any()


@pytest.mark.parametrize("world,pair", (("permuted", "masks"), ("situations", "lockdown"), ("fixture_a", "masks")))
def test_a_window_of_two_areas_sends_the_others_down_the_direct_path(probe, world, pair):
    pop, ep, n, _, _, b, _, c, _ = cr.cached(world, pair)
    col, n_cols = cr.columns(pop, "home")
    assert n_cols > 2 * 4 and probe.compare_probe_window() == 2      # more areas than any workgroup's window holds
    for per_block in (1024, 4096, 1 << 20):                          # several stretches, and one workgroup striding over everybody
        for first, last in ((0, n), (n // 3, 2 * n // 3)):
            want = cr.compare(b, c, col, n_cols, first, last)
            got = probe_compare(probe, b, c, pop.home_building, pop.building_area, "home", n_cols, first, last, per_block=per_block)
            same_compare(got, want, (world, pair, per_block, first, last))
    assert (want["counts"][:, B] > 0).sum() > 2
    # by group with the LDS table full: 1024 columns
    labels = (np.arange(pop.n_citizens) % 1024).astype(np.uint16)
    colg, _ = cr.columns(pop, "group", labels, 1024)
    same_compare(probe_compare(probe, b, c, pop.home_building, pop.building_area, "group", 1024, 0, n, labels, per_block=4096), cr.compare(b, c, colg, 1024, 0, n), "1024 groups")
    # the rows kernel under a grid of one workgroup strides over everybody
    want_b, want_c = cr.series(b, c, col, n_cols, 0, 5, 97, True)
    got_b, got_c = probe_rows(probe, b, c, pop.home_building, pop.building_area, "home", n_cols, 0, 5, 97, True, grid=1)
    assert np.array_equal(got_b, want_b) and np.array_equal(got_c, want_c)


# ---- 3. identities and lifetime ------------------------------------------------------------------------------------------------
def state_of(sim, tmp_path, name):
    path = str(tmp_path / name)
    sim.save_checkpoint(path)
    with open(path, "rb") as f:
        ckpt = f.read()
    return (_oracle.state_digest(sim.download_state()), sim.records_so_far().tobytes(), tuple(a.tobytes() for a in sim.exposure_events()),
            sim.area_census("home").tobytes(), ckpt)


def test_keep_and_compare_leave_everything_as_it_is_and_right_after_keep_nothing_differs(tmp_path):
    pop, ep, n, over_b, _, b, _, _, _ = cr.cached("situations", "lockdown")
    sim = Simulator(pop, ref_mod.copy_params(ep))
    sim.set_groups(*groups_of(pop, 7))
    run_arm(sim, ep, over_b, n)
    before = state_of(sim, tmp_path, "before")
    sim.keep_baseline()
    for where in ("all", "home", "group"):
        got = sim.compare(where, 0, n, citizens=True)
        assert not got["counts"][:, 1:].any() and got["counts"][:, B].sum() == (b != NEVER).sum() and not got["delay"].any() and got["first_divergence"] is None
        assert (got["cls"] == (b != NEVER)).all()
        rows_b, rows_c = sim.compare_series(where, 0, None, 24, True)
        assert np.array_equal(rows_b, rows_c) and rows_b[-1].sum() == (b != NEVER).sum()
    assert state_of(sim, tmp_path, "after") == before
    sim.close()


def test_the_baseline_survives_what_the_snapshot_survives_and_goes_with_an_upload_and_a_drop(tmp_path):
    pop, ep, n, over_b, over_c, b, _, c, _ = cr.cached("situations", "masks")
    sim = Simulator(pop, ref_mod.copy_params(ep))
    lib, ctx = sim.lib, sim._ctx
    col, n_cols = cr.columns(pop, "all")
    run_arm(sim, ep, over_b, n)
    sim.keep_baseline()
    kept = sim.baseline_info()
    sim.reset()                                                      # esim_reset
    assert sim.baseline_info()["steps"] == n
    n_seeds = len(np.unique(pop.seeds))
    got = sim.compare("all", 0, 0)                                   # the index cases are the same: nothing but BOTH at step 0
    assert got["counts"][0].tolist() == [n_seeds, 0, 0, 0, 0] and got["first_divergence"] == int(b[b > 0].min())
    sim.restart(ref_mod.copy_params(ep), seeds=pop.seeds[:5], **over_c)    # esim_restart_seeded: the other index cases are averted
    assert sim.compare("all", 0, 0)["counts"][0].tolist() == [5, n_seeds - 5, 0, 0, 0] and len(np.unique(pop.seeds[:5])) == 5
    run_arm(sim, ep, over_c, 30)                                     # esim_restart
    assert sim.baseline_info()["steps"] == n
    sim.restart(ref_mod.copy_params(ep), seeds=pop.seeds, **over_c)  # the population's own index cases again
    sim.run(200)
    sim.snapshot()                                                   # esim_snapshot
    path = str(tmp_path / "ckpt")
    sim.save_checkpoint(path)
    sim.run(n - 200)
    want = cr.compare(b, c, col, n_cols, 0, n)
    same_compare(sim.compare("all", 0, n, citizens=True), want, "after reset, restarts and a snapshot")
    sim.rollback()                                                   # esim_rollback
    assert sim.baseline_info()["n_cases"] == kept["n_cases"]
    sim.run(n - 200)
    same_compare(sim.compare("all", 0, n, citizens=True), want, "after a rollback")
    sim.restart(ref_mod.copy_params(ep), **over_c)
    sim.load_checkpoint(path)                                        # esim_checkpoint_restore
    sim.run(n - 200)
    same_compare(sim.compare("all", 0, n, citizens=True), want, "after a checkpoint restore")
    # a later keep replaces it; a drop forgets it; a new upload drops it
    sim.keep_baseline()
    assert sim.baseline_info()["n_cases"] == int((c != NEVER).sum()) and sim.compare("all", 0, n)["first_divergence"] is None
    sim.drop_baseline()
    assert lib.esim_baseline_info(ctx, None, None, None) == ESTATE and lib.esim_baseline_drop(ctx) == ESTATE and lib.esim_compare(ctx, ALL, 0, n, None, None, None, None) == ESTATE
    sim.keep_baseline()
    ps = pop.as_struct()
    _lib.check(lib.esim_upload_population(ctx, C.byref(ps)), ctx)
    assert lib.esim_baseline_info(ctx, None, None, None) == ESTATE and lib.esim_compare(ctx, ALL, 0, 0, None, None, None, None) == ESTATE
    sim.close()


def test_in_a_branch_the_histories_diverge_behind_the_snapshot():
    pop, ep, n, t, over, b, c = cr.forecast()
    sim = Simulator(pop, ref_mod.copy_params(ep))
    sim.run(t)
    sim.snapshot()
    sim.run(n - t)
    sim.keep_baseline()
    sim.rollback(**over)
    sim.run(n - t)
    for where in ("all", "home"):
        col, n_cols = cr.columns(pop, where)
        got = sim.compare(where, 0, n, citizens=True)
        same_compare(got, cr.compare(b, c, col, n_cols, 0, n), ("forecast", where))
        assert got["first_divergence"] > t
    got = sim.compare("all", 0, t)                                   # the shared history: nothing differs in it
    assert not got["counts"][0, 1:].any() and got["delay"][0] == 0
    sim.close()


# ---- 4. the error table --------------------------------------------------------------------------------------------------------
def test_the_error_table():
    pop, ep, n, over_b, _, _, _, _, _ = cr.cached("situations", "lockdown")
    lib = _lib.load()
    ctx = C.c_void_p()
    _lib.check(lib.esim_create(C.byref(_lib.default_params()), C.byref(ctx)))
    assert lib.esim_baseline_keep(ctx) == ESTATE and lib.esim_baseline_info(ctx, None, None, None) == ESTATE and lib.esim_baseline_drop(ctx) == ESTATE    # before an upload
    assert lib.esim_compare(ctx, ALL, 0, 0, None, None, None, None) == ESTATE and lib.esim_compare_series(ctx, ALL, 0, 1, 1, 0, None, None) == ESTATE
    assert lib.esim_ensemble_begin_paired(ctx, ALL, 0, 1, 1, 0, 1, 1) == ESTATE and lib.esim_ensemble_read_paired(ctx, 0, 0, *([None] * 8)) == ESTATE
    lib.esim_destroy(ctx)
    for fn, args in ((lib.esim_baseline_keep, ()), (lib.esim_baseline_drop, ()), (lib.esim_baseline_info, (None, None, None)), (lib.esim_compare, (ALL, 0, 0, None, None, None, None)),
                     (lib.esim_compare_series, (ALL, 0, 1, 1, 0, None, None)), (lib.esim_ensemble_begin_paired, (ALL, 0, 1, 1, 0, 1, 1)),
                     (lib.esim_ensemble_read_paired, (0, 0) + (None,) * 8)):
        assert fn(None, *args) == EINVAL                             # a null context
    sim = Simulator(pop, ref_mod.copy_params(ep))
    lib, ctx = sim.lib, sim._ctx
    n_areas = pop.n_areas
    counts, delay, div, cls = np.full((n_areas, 5), 7, np.uint64), np.full(n_areas, 7, np.int64), C.c_uint32(7), np.full(pop.n_citizens, 7, np.uint8)
    rows_b, rows_c = np.full((4, n_areas), 7, np.uint32), np.full((4, n_areas), 7, np.uint32)
    outs = (counts.ctypes.data_as(u64p), delay.ctypes.data_as(i64p), C.byref(div), cls.ctypes.data_as(u8p))
    rows = (rows_b.ctypes.data_as(u32p), rows_c.ctypes.data_as(u32p))
    compare = lambda where, first, last: lib.esim_compare(ctx, where, first, last, *outs)
    series = lambda where, first, n_rows, stride: lib.esim_compare_series(ctx, where, first, n_rows, stride, 0, *rows)
    sim.run(50)
    # without a baseline
    assert compare(HOME, 0, 10) == ESTATE and series(HOME, 0, 4, 10) == ESTATE and b"esim_baseline_keep" in lib.esim_last_error(ctx)
    assert lib.esim_baseline_info(ctx, None, None, None) == ESTATE and lib.esim_baseline_drop(ctx) == ESTATE
    sim.keep_baseline()                                              # a baseline of 50 steps
    sim.run(30)                                                      # against a run of 80
    for where in (_lib.AREA_CURRENT, _lib.BY_SETTING, 7, -1):
        assert compare(where, 0, 10) == EINVAL and series(where, 0, 4, 10) == EINVAL and lib.esim_ensemble_begin_paired(ctx, where, 0, 4, 10, 0, 1, 1) == EINVAL, where
    assert series(HOME, 0, 4, 0) == EINVAL and series(HOME, 0, 0, 10) == EINVAL
    for bad in ((0, 4, 0, 0, 1, 1), (0, 0, 10, 0, 1, 1), (0, 4, 10, 0, 1, 0)):
        assert lib.esim_ensemble_begin_paired(ctx, HOME, *bad) == EINVAL, bad
    assert compare(GROUP, 0, 10) == ESTATE and series(GROUP, 0, 4, 10) == ESTATE and lib.esim_ensemble_begin_paired(ctx, GROUP, 0, 4, 10, 0, 1, 1) == ESTATE    # no labels
    assert compare(HOME, 11, 10) == ERANGE and compare(HOME, 0, 51) == ERANGE and compare(HOME, 0, 50) == 0        # the shorter run bounds the window
    counts[:], delay[:], div.value, cls[:] = 7, 7, 7, 7
    assert series(HOME, 0, 4, 17) == ERANGE and series(HOME, 51, 1, 1) == ERANGE and series(HOME, 0, 4, 16) == 0 and series(HOME, 50, 1, 1) == 0
    rows_b[:], rows_c[:] = 7, 7
    sim.restart(ref_mod.copy_params(ep))
    sim.run(20)                                                      # the current run is the shorter one now
    assert compare(HOME, 0, 21) == ERANGE and series(HOME, 21, 1, 1) == ERANGE
    # a refusal touches no output
    assert (counts == 7).all() and (delay == 7).all() and div.value == 7 and (cls == 7).all() and (rows_b == 7).all() and (rows_c == 7).all()
    assert compare(HOME, 0, 20) == 0 and (cls <= 3).all()
    # a paired fold: no rows behind either run, and none without a baseline
    assert lib.esim_ensemble_begin_paired(ctx, HOME, 0, 3, 10, 0, 1, 1) == 0
    assert lib.esim_ensemble_fold(ctx) == 0 and lib.esim_ensemble_fold(ctx) == 0
    assert lib.esim_ensemble_begin_paired(ctx, HOME, 0, 4, 7, 0, 1, 1) == 0
    assert lib.esim_ensemble_fold(ctx) == ERANGE and b"rows outside" in lib.esim_last_error(ctx)
    sim._ens_rows, sim._ens_n = 4, n_areas
    assert sim.ensemble_read_paired()["members"] == 0
    assert lib.esim_ensemble_read_paired(ctx, 3, 2, *([None] * 8)) == ERANGE and lib.esim_ensemble_read_paired(ctx, 3, 1, *([None] * 8)) == 0
    assert lib.esim_ensemble_read(ctx, None, None, None, None) == ESTATE and lib.esim_ensemble_read_series(ctx, 0, 0, None, None, None, None) == ESTATE
    assert lib.esim_ensemble_read_reproduction(ctx, 0, 0, *([None] * 8)) == ESTATE
    sim.drop_baseline()
    assert lib.esim_ensemble_fold(ctx) == ESTATE and b"esim_baseline_keep" in lib.esim_last_error(ctx)
    assert sim.ensemble_read_paired()["members"] == 0
    # a sticky device-side error is reported as the series calls report it
    sim.keep_baseline()
    assert lib.esim_ensemble_begin_paired(ctx, HOME, 0, 3, 10, 0, 1, 1) == 0
    _lib.check(lib.esim_debug_inject_error(ctx, ERANGE), ctx)
    want = lib.esim_area_status_series(ctx, HOME, _lib.AREA_SERIES_INCIDENCE, 1, 4, 1, rows_b.ctypes.data_as(u32p))
    assert want != 0
    assert lib.esim_baseline_keep(ctx) == want and compare(HOME, 0, 20) == want and series(HOME, 0, 1, 1) == want and lib.esim_ensemble_fold(ctx) == want
    sim.close()


def test_a_shard_and_a_communicator_of_two_ranks_are_refused():
    whole = Population.synthetic("york", n_citizens=20000, n_areas=64, citizens_per_school=2500)
    cuts = whole.even_cuts(2)
    s0, s1 = whole.shard(cuts, 0), whole.shard(cuts, 1)
    sim = Simulator(s0, _lib.default_params())
    lib, ctx = sim.lib, sim._ctx
    assert lib.esim_baseline_keep(ctx) == ESTATE and b"shard" in lib.esim_last_error(ctx)             # a shard without a communicator
    assert lib.esim_compare(ctx, ALL, 0, 0, None, None, None, None) == ESTATE and lib.esim_compare_series(ctx, ALL, 0, 1, 1, 0, None, None) == ESTATE
    assert lib.esim_ensemble_begin_paired(ctx, HOME, 0, 2, 1, 0, 1, 1) == 0 and lib.esim_ensemble_fold(ctx) == ESTATE

    def allreduce(user, which, host_ptr, n_u32):
        if which == 8:                                   # the set-up's layout check: rank 1's row, as its process would add it
            a = (C.c_uint32 * n_u32).from_address(host_ptr)
            a[5:10] = [s0.n_citizens, s1.n_citizens, whole.n_citizens, s1.n_shared_buildings, s1.n_shared_rooms]
        return 0

    cb = _lib.ALLREDUCE_FN(allreduce)
    _lib.check(lib.esim_comm_init_callback(ctx, cb, None, 0, 2), ctx)
    assert lib.esim_baseline_keep(ctx) == ESTATE and lib.esim_compare(ctx, ALL, 0, 0, None, None, None, None) == ESTATE
    assert lib.esim_compare_series(ctx, ALL, 0, 1, 1, 0, None, None) == ESTATE and lib.esim_ensemble_begin_paired(ctx, HOME, 0, 2, 1, 0, 1, 1) == ESTATE
    assert lib.esim_ensemble_fold(ctx) == ESTATE
    sim.close()


# ---- 5. the paired accumulators and Ensemble.compare ---------------------------------------------------------------------------
MEMBER_SEEDS = (123, 1001, 1002)
POLICY = {"mask_effectiveness": 1.0}


def member_planes():
    """Per member the planes of its two arms on `situations`, from the oracle: the world's parameters against perfect masks."""
    pop, ep, n = cr.world("situations")
    out = []
    for seed in MEMBER_SEEDS:
        out.append(tuple(cr.steps_of_run(pop, ref_mod.copy_params(ep, seed=seed, **over), n)[0] for over in ({}, POLICY)))
    return pop, ep, n, out


@pytest.fixture(scope="module")
def members():
    return member_planes()


def test_three_members_folded_against_members_compared_singly(members):
    pop, ep, n, planes = members
    sim = Simulator(pop, ref_mod.copy_params(ep))
    labels, n_groups = groups_of(pop, 7)
    sim.set_groups(labels, n_groups)
    window = dict(first_step=0, n_rows=7, stride=64, cumulative=True)
    for where, min_baseline, min_averted in (("home", 20, 3), ("all", 100, 100), ("group", 100, 10)):
        col, n_cols = cr.columns(pop, where, labels, n_groups)
        sim.ensemble_begin_paired(where, min_baseline=min_baseline, min_averted=min_averted, **window)
        singly = []
        for seed in MEMBER_SEEDS:
            run_arm(sim, ep, dict(seed=seed), n)
            sim.keep_baseline()
            run_arm(sim, ep, dict(POLICY, seed=seed), n)
            singly.append(sim.compare_series(where, **window))
            sim.ensemble_fold()
        got = sim.ensemble_read_paired()
        assert got["members"] == 3 and got["hit"].shape == (7, n_cols)
        want = cr.fold_paired(singly, min_baseline, min_averted)
        for k in KEYS:
            assert np.array_equal(got[k], want[k]), (where, k)
        ref = cr.fold_paired([cr.series(b, c, col, n_cols, 0, 7, 64, True) for b, c in planes], min_baseline, min_averted)
        for k in KEYS:
            assert np.array_equal(got[k], ref[k]), (where, k, "reference")
        assert want["hit"].any() and (want["defined"] > want["hit"]).any() and (want["defined"] < 3).any(), where
        # every pointer alone, and a part of the rows
        for i, k in enumerate(("members",) + KEYS):
            out = np.full(1 if k == "members" else want["hit"].size, 7, np.uint32 if i < 3 else np.uint64)
            args = [None] * 8
            args[i] = out.ctypes.data_as(u32p if i < 3 else u64p)
            assert sim.lib.esim_ensemble_read_paired(sim._ctx, 0, 7, *args) == 0, k
            assert (out == (3 if k == "members" else want[k].ravel())).all(), k
        part = sim.ensemble_read_paired(first_row=2, n_rows=3)
        assert all(np.array_equal(part[k], want[k][2:5]) for k in KEYS)
    # a begin of the same shape zeroes; another shape replaces; the other kinds take over and give way again
    sim.ensemble_begin_paired("group", min_baseline=1, min_averted=1, **window)
    zero = sim.ensemble_read_paired()
    assert zero["members"] == 0 and all(not zero[k].any() for k in KEYS)
    sim.ensemble_fold()
    one = cr.fold_paired(singly[-1:], 1, 1)
    assert all(np.array_equal(sim.ensemble_read_paired()[k], one[k]) for k in KEYS)
    sim.ensemble_begin_paired("group", first_step=5, n_rows=3, stride=100, cumulative=False)
    sim.ensemble_fold()
    other = cr.fold_paired([sim.compare_series("group", 5, 3, 100)], 1, 1)
    got = sim.ensemble_read_paired()
    assert got["hit"].shape == (3, 7) and all(np.array_equal(got[k], other[k]) for k in KEYS)
    x = sim.reproduction_series("home", 0, 3, 100)
    sim.ensemble_begin_reproduction("home", first_step=0, n_rows=3, stride=100)
    assert sim.lib.esim_ensemble_read_paired(sim._ctx, 0, 0, *([None] * 8)) == ESTATE
    sim.ensemble_fold()
    r = sim.ensemble_read_reproduction()
    assert r["members"] == 1 and np.array_equal(r["sum_cases"], x[0]) and np.array_equal(r["sum_offspring"], x[1])
    y = sim.setting_series("home", None, 1, 3, 100)
    sim.ensemble_begin_settings("home", first_step=1, n_rows=3, stride=100)
    sim.ensemble_fold()
    assert np.array_equal(sim.ensemble_read_series()["sum"], y)
    sim.ensemble_begin_paired("all", **window)
    assert sim.lib.esim_ensemble_read_reproduction(sim._ctx, 0, 0, *([None] * 8)) == ESTATE and sim.ensemble_read_paired()["members"] == 0
    # replaced labels invalidate accumulators begun by group
    sim.ensemble_begin_paired("group", **window)
    sim.set_groups(labels, n_groups)
    assert sim.lib.esim_ensemble_fold(sim._ctx) == ESTATE and sim.lib.esim_ensemble_read_paired(sim._ctx, 0, 0, *([None] * 8)) == ESTATE
    sim.close()


def test_ensemble_compare_with_and_without_a_shared_history(members, tmp_path):
    pop, ep, n, planes = members
    codes = ["E%05d" % i for i in range(pop.n_areas)]
    ens = Ensemble(pop, ref_mod.copy_params(ep), area_codes=codes)
    overrides = [{"seed": s} for s in MEMBER_SEEDS]
    rows = dict(first_step=0, n_rows=19, stride=24, cumulative=False, min_baseline=5, min_averted=2)
    res = ens.compare({}, POLICY, overrides, n, where="home", rows=rows)
    col, n_cols = cr.columns(pop, "home")
    want = [cr.compare(b, c, col, n_cols, 0, n) for b, c in planes]
    assert res.counts.shape == (3, n_cols, 5) and res.area_codes == codes and res.members == overrides
    assert np.array_equal(res.counts, np.stack([w["counts"] for w in want])) and np.array_equal(res.delay, np.stack([w["delay"] for w in want]))
    assert res.first_divergence.tolist() == [-1 if w["first_divergence"] is None else w["first_divergence"] for w in want] and (res.averted().sum(1) > 0).all()
    member_rows = [cr.series(b, c, col, n_cols, 0, 19, 24) for b, c in planes]
    acc = cr.fold_paired(member_rows, 5, 2)
    got = ens.simulator.ensemble_read_paired()
    assert all(np.array_equal(got[k], acc[k]) for k in KEYS)
    summary = paired_summary(acc, 0, 24)
    for k in ("defined", "hit", "mean_baseline", "mean_policy", "mean_averted", "p_averted", "se_paired", "se_unpaired", "steps"):
        assert np.array_equal(res.summary[k], summary[k], equal_nan=True), k
    for arm, i in ((res.records_baseline, 0), (res.records_policy, 1)):
        assert arm.shape == (3, n)
        for m in range(3):
            steps = planes[m][i]
            per_step = np.bincount(steps[(steps != NEVER) & (steps > 0)], minlength=n + 1)[1:]
            assert (arm[m]["exposures_building"].astype(np.int64) + arm[m]["exposures_bus"] == per_step).all()
    res.dump(str(tmp_path))
    z = np.load(tmp_path / "ensemble_compare.npz")
    assert np.array_equal(z["counts"], res.counts) and z["codes"].tolist() == codes and np.array_equal(z["summary_se_paired"], summary["se_paired"], equal_nan=True)
    # both arms as branches from a shared history of 200 steps under the world's parameters
    t = 200
    res = ens.compare({}, POLICY, overrides[:2], n, history_steps=t, where="all")
    assert res.summary is None and res.counts.shape == (2, 1, 5) and (res.first_divergence > t).all()
    sim = ens.simulator
    by_hand = []
    for over in overrides[:2]:
        sim.restart(ref_mod.copy_params(ep))
        sim.run(t)
        sim.snapshot()
        sim.rollback(**over)
        sim.run(n - t)
        sim.keep_baseline()
        sim.rollback(**dict(POLICY, **over))
        sim.run(n - t)
        by_hand.append(sim.compare("all", 0, n))
    assert np.array_equal(res.counts, np.stack([w["counts"] for w in by_hand])) and np.array_equal(res.delay, np.stack([w["delay"] for w in by_hand]))
    assert res.first_divergence.tolist() == [w["first_divergence"] for w in by_hand]
    # the member under the world's own seed is the reference's forecast
    pop_f, ep_f, n_f, t_f, over_f, b, c = cr.forecast()
    col, n_cols = cr.columns(pop, "all")
    assert t_f == t and np.array_equal(res.counts[0], cr.compare(b, c, col, n_cols, 0, n)["counts"])
    ens.close()
