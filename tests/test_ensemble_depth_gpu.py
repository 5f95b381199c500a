"""Curve-based ensemble statistics through the library: esim_ensemble_depth and esim_ensemble_band over the store of
esim_ensemble_keep_members, and the Python Ensemble on top.  Every comparison is exact integer equality.  The member stack comes
from the existing per-member calls, as in test_ensemble_members_gpu.py, whose worlds and helpers these tests use; the depths and
the central region from numpy over that stack (tests/_depth_ref.py) -- never from the code under test."""
import ctypes as C
import os

import numpy as np
import pytest

import _depth_ref as ref
from epidemicsimulator_amd import Ensemble, Population, Simulator, _lib
from test_ensemble_gpu import area_world
from test_ensemble_members_gpu import (AGE_EDGES, AREA_WINDOW, KINDS, PAIRED_WINDOW, SERIES_AREA, TINY_WINDOWS, E, I, R, census_x, dumped, fold_all, frozen_clock,  # noqa: F401
                                       series_of, tiny, world)

pytestmark = pytest.mark.gpu

EINVAL, ESTATE, ERANGE = -1, -4, -5
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "epidemicsimulator_amd", "csrc")
u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
PLANES = ("lo", "hi", "median", "deepest", "n_in")


def half(m):
    return -(-m // 2)


def check_curves(sim, stack, what, first_row=0, n_rows=None):
    """The depth call and the band call at need 1, ceil(M / 2) and M, pooled and not, over rows [first_row, first_row + n_rows)
    of the store against numpy over the stack [members, rows, cols]: (the depths, {(need, pooled): the band})."""
    m = stack.shape[0]
    win = stack[:, first_row:] if n_rows is None else stack[:, first_row:first_row + n_rows]
    want = ref.depth(win)
    got = sim.ensemble_depth(first_row, n_rows)
    assert got["depth"].dtype == np.uint32 and got["depth"].shape == want.shape and (got["depth"] == want).all(), (what, "depth", np.argwhere(got["depth"] != want)[:8].tolist())
    assert got["total"].dtype == np.uint64 and (got["total"] == ref.total(win)).all(), (what, "total")
    assert got["pairs"] == ref.pairs(m) and got["rows"] == win.shape[1]
    if m > 1 and win.shape[1]:
        assert np.array_equal(got["mbd"], want / float(win.shape[1] * ref.pairs(m))) and got["mbd"].max() <= 1.0
    else:
        assert np.isnan(got["mbd"]).all() and not want.any()
    bands = {}
    for need in sorted({1, half(m), m}):
        for pooled in (False, True):
            b = bands[(need, pooled)] = ref.band(win, need, pooled)
            g = sim.ensemble_band(need=need, pooled=pooled, first_row=first_row, n_rows=n_rows)
            assert g["need"] == need and g["lo"].dtype == stack.dtype
            for k in PLANES:
                assert g[k].shape == b[k].shape and (g[k] == b[k]).all(), (what, "need %d" % need, "pooled" if pooled else "per column", k, np.argwhere(g[k] != b[k])[:8].tolist())
    return want, bands


def assert_not_trivial(stack, depths, bands, what):
    """Depths differ between members in some column, the central half is a band with lo < hi somewhere, and it lies strictly
    inside the envelope of all members somewhere -- per column and pooled."""
    m = stack.shape[0]
    assert (depths.min(axis=0) < depths.max(axis=0)).any(), what
    for pooled in (False, True):
        b = bands[(half(m), pooled)]
        assert (b["lo"] < b["hi"]).any(), (what, pooled)
        assert ((b["lo"] > stack.min(axis=0)) | (b["hi"] < stack.max(axis=0))).any(), (what, pooled)
        assert (b["n_in"] >= half(m)).all() and (b["n_in"] < m).any(), (what, pooled)
    whole = bands[(m, False)]
    assert (whole["lo"] == stack.min(axis=0)).all() and (whole["hi"] == stack.max(axis=0)).all() and (whole["n_in"] == m).all()


def arrival_at_the_median_step(sim, members, steps, ep):
    """(begin, the member's x) of the arrival kind with the horizon at the median of the arrival steps of these members.  Under
    the horizon of the members test (120) most areas are reached by no member or at step 0 by all, and the central half of six
    members is a single value in every column: here half of the arrivals count and the other half are ESIM_NEVER."""
    raw = []
    for m in members:
        sim.restart(ep, **m)
        sim.run(steps)
        raw.append(sim.area_arrival("home"))
    raw = np.asarray(raw)
    horizon = int(np.median(raw[(raw > 0) & (raw <= steps)]))
    assert 0 < horizon < steps
    return (lambda s: s.ensemble_begin_arrival("home", horizon)), (lambda s: np.where(s.area_arrival("home") <= horizon, s.area_arrival("home"), _lib.NEVER).astype(np.uint32)[None, :])


# ---- 1. four kinds, six members: unsigned with many all-zero cells, one row with NEVER, signed, the step of the peak ------------------
@pytest.mark.parametrize("kind", ("series-incidence", "arrival", "paired-cumulative", "peaks-step"))
def test_four_kinds_over_six_members(world, kind):
    sim, policy, members, steps, ep = world
    begin, x_of, what, _, _ = KINDS[kind]
    mem = policy if kind.startswith("paired") else members
    if kind == "arrival":
        begin, x_of = arrival_at_the_median_step(sim, mem, steps, ep)
    stack = fold_all(sim, mem, steps, begin, x_of, keep=len(mem), what=what, params=ep)
    assert stack.shape[0] == 6 and stack.dtype == (np.int32 if kind.startswith("paired") else np.uint32)
    depths, bands = check_curves(sim, stack, kind)
    assert_not_trivial(stack, depths, bands, kind)
    if kind in ("arrival", "peaks-step"):
        assert (stack == _lib.NEVER).any() and (bands[(6, False)]["hi"] == _lib.NEVER).any()
    if stack.shape[1] > 2:                      # windows of rows: the second and third, the two where the members differ most, none
        check_curves(sim, stack, kind + ", rows 1..2", first_row=1, n_rows=2)
        spread = (stack.max(axis=0).astype(np.int64) - stack.min(axis=0)).sum(axis=1)
        first = int(np.argmax(spread[:-1] + spread[1:]))
        d, b = check_curves(sim, stack, kind + ", rows %d..%d" % (first, first + 1), first_row=first, n_rows=2)
        assert_not_trivial(stack[:, first:first + 2], d, b, kind + ", rows %d..%d" % (first, first + 1))
        check_curves(sim, stack, kind + ", no rows", first_row=stack.shape[1], n_rows=0)


# ---- 2. a few columns, and one ----------------------------------------------------------------------------------------------------------
def test_by_group_over_five_age_bands(world):
    sim, _, members, steps, ep = world
    sim.set_groups(np.digitize(sim.population.age, AGE_EDGES).astype(np.uint16), 5)
    try:
        begin = lambda s: s.ensemble_begin_series("group", "exposures", min_cases=1, **AREA_WINDOW)
        stack = fold_all(sim, members, steps, begin, lambda s: s.group_series("exposures", **AREA_WINDOW), keep=6, params=ep)
        assert stack.shape == (6, AREA_WINDOW["n_rows"], 5)
        depths, bands = check_curves(sim, stack, "group")
        assert_not_trivial(stack, depths, bands, "group")
        # new labels invalidate a store begun by group
        sim.set_groups(np.zeros(sim.population.n_citizens, np.uint16), 1)
        for call in (sim.ensemble_depth, sim.ensemble_band):
            with pytest.raises(_lib.EsimError) as err:
                call()
            assert err.value.code == ESTATE
    finally:
        sim.set_groups(None)


def test_a_paired_begin_by_all_has_one_column(world):
    sim, policy, _, steps, ep = world
    begin = lambda s: s.ensemble_begin_paired("all", cumulative=True, min_baseline=0, min_averted=1, **PAIRED_WINDOW)

    def x_of(s):
        b, c = s.compare_series("all", cumulative=True, **PAIRED_WINDOW)
        return (b.astype(np.int64) - c.astype(np.int64)).astype(np.int32)
    stack = fold_all(sim, policy, steps, begin, x_of, keep=6, params=ep)
    assert stack.shape == (6, PAIRED_WINDOW["n_rows"], 1) and stack.dtype == np.int32
    depths, bands = check_curves(sim, stack, "paired by all")
    assert_not_trivial(stack, depths, bands, "paired by all")
    one = bands[(1, True)]                      # one column: pooled and per column are the same ranking
    assert all((one[k] == bands[(1, False)][k]).all() for k in PLANES) and (one["median"][:, 0] == stack[one["deepest"][0], :, 0]).all()


# ---- 3. member counts through the library: one member, two, the pad to 16, the LDS path -------------------------------------------------
@pytest.mark.parametrize("n_members", (1, 2, 9, 65))
def test_member_counts(tiny, n_members):
    members = Ensemble.seeds(n_members, first=3)
    stack = fold_all(tiny, members, 200, lambda s: s.ensemble_begin("home", E | I | R, 1), census_x, keep=n_members)
    assert stack.shape == (n_members, 1, 3)
    depths, bands = check_curves(tiny, stack, "census, %d members" % n_members)
    if n_members == 1:
        assert not depths.any() and (bands[(1, False)]["lo"] == stack[0]).all()
    elif n_members == 2:
        assert (depths == 1).all()              # the one pair holds both of its members
    else:
        assert_not_trivial(stack, depths, bands, "census, %d members" % n_members)


@pytest.mark.parametrize("window", TINY_WINDOWS, ids=["21cells", "3cells"])
def test_cell_counts_that_are_no_multiple_of_four(tiny, window):
    begin = lambda s: s.ensemble_begin_series("home", "infected", min_cases=1, **window)
    stack = fold_all(tiny, Ensemble.seeds(6, first=3), 540, begin, lambda s: series_of(s, "home", "infected", **window), keep=6)
    assert stack.shape[1] * stack.shape[2] in (21, 3) and stack.any()
    depths, bands = check_curves(tiny, stack, "series, %d cells" % (stack.shape[1] * stack.shape[2]))
    assert_not_trivial(stack, depths, bands, "series, %d cells" % (stack.shape[1] * stack.shape[2]))


# ---- 4. under ESIM_GRID_CAP -----------------------------------------------------------------------------------------------------------
def wide_world_outputs():
    """The 800-area world of the members test, three members of the incidence rows: the stack and every output of both calls."""
    pop = Population.synthetic("york", n_citizens=8000, n_areas=800, citizens_per_school=4000, n_seeds=12, p_public_transport=0.4)
    sim = Simulator(pop, _lib.default_params(exposure_chance=0.004))  # (the knob is read at the upload)
    try:
        begin, x_of, what, _, _ = KINDS["series-incidence"]
        stack = fold_all(sim, Ensemble.seeds(3, first=11), 250, begin, x_of, keep=3, what=what)
        out = {"depth": sim.ensemble_depth(), "window": sim.ensemble_depth(first_row=20, n_rows=9)}
        for need in (1, 2, 3):
            for pooled in (False, True):
                out[(need, pooled)] = sim.ensemble_band(need=need, pooled=pooled)
        return stack, out, {k: v for k, v in sim.debug_launches().items() if "esim_host_depth.h" in k}
    finally:
        sim.close()


@pytest.fixture(scope="module")
def uncapped():
    knob = os.environ.pop("ESIM_GRID_CAP", None)
    try:
        stack, out, sites = wide_world_outputs()
    finally:
        if knob is not None:
            os.environ["ESIM_GRID_CAP"] = knob
    assert stack.shape == (3, 35, 800) and stack.any() and not sites
    assert (out["depth"]["depth"] == ref.depth(stack)).all() and (out["window"]["depth"] == ref.depth(stack[:, 20:29])).all()
    for need in (1, 2, 3):
        for pooled in (False, True):
            want = ref.band(stack, need, pooled)
            assert all((out[(need, pooled)][k] == want[k]).all() for k in PLANES), (need, pooled)
    assert (out["depth"]["depth"].min(axis=0) < out["depth"]["depth"].max(axis=0)).any() and (out[(2, False)]["lo"] < out[(2, False)]["hi"]).any()
    return stack, out


@pytest.mark.parametrize("cap", (1, 3))
def test_capped_grids_give_identical_outputs_and_clip_every_launch_site(uncapped, cap, monkeypatch):
    monkeypatch.setenv("ESIM_GRID_CAP", str(cap))
    stack, out, sites = wide_world_outputs()
    assert (stack == uncapped[0]).all()
    for key, want in uncapped[1].items():
        assert sorted(out[key]) == sorted(want), key
        for k in want:
            assert np.array_equal(out[key][k], want[k], equal_nan=True), (cap, key, k)
    text = open(os.path.join(CSRC, "esim_host_depth.h")).read().splitlines()
    lines = sorted(i + 1 for i, line in enumerate(text) if "grid_capped(" in line)
    assert len(lines) == 5 and sorted(int(k.rsplit(":", 1)[1]) for k in sites) == lines, (sites, lines)
    for k, v in sites.items():
        assert v["launches"] >= 1 and v["clipped"] >= 1, (k, v)
    if cap == 1:
        assert all(v["max_trips"] >= 3 for v in sites.values()), sites


# ---- 5. errors and lifetime -----------------------------------------------------------------------------------------------------------
def test_errors_and_lifetime(tiny):
    sim, lib, ctx = tiny, tiny.lib, tiny._ctx
    planes = [np.zeros(64, np.uint32) for _ in range(5)]
    table, totals = np.zeros(64, np.uint32), np.zeros(8, np.uint64)
    p = [a.ctypes.data_as(u32p) for a in planes]
    depth = lambda first_row=0, n_rows=1, d=table.ctypes.data_as(u32p), t=totals.ctypes.data_as(u64p), c=ctx, l=lib: l.esim_ensemble_depth(c, first_row, n_rows, d, t)
    band = lambda first_row=0, n_rows=1, need=1, pooled=0, out=p, c=ctx, l=lib: l.esim_ensemble_band(c, first_row, n_rows, need, pooled, *out)
    fresh = Simulator(sim.population, sim.params)
    assert depth(c=fresh._ctx, l=fresh.lib) == ESTATE and band(c=fresh._ctx, l=fresh.lib) == ESTATE      # before a begin
    fresh.close()
    sim.restart(seed=5)
    sim.run(120)
    sim.ensemble_begin("home", E | I | R, 1)
    assert depth() == ESTATE and band() == ESTATE                                             # no store
    sim.ensemble_keep_members(3)
    assert depth() == ESTATE and band() == ESTATE and b"no member has been folded" in lib.esim_last_error(ctx)   # before a fold
    xs = []
    for seed in (5, 6, 7):
        sim.restart(seed=seed)
        sim.run(120)
        xs.append(census_x(sim))
        sim.ensemble_fold()
    stack = np.stack(xs)
    before = sim.ensemble_read()
    assert depth() == 0 and (table[:9].reshape(3, 3) == ref.depth(stack)).all() and (totals[:3] == ref.total(stack)).all()
    assert band(need=2) == 0 and (planes[0][:3] == ref.band(stack, 2, False)["lo"][0]).all() and (planes[4][:3] == ref.band(stack, 2, False)["n_in"]).all()
    # rows outside the store, need outside 1..kept, pooled that is neither 0 nor 1
    assert depth(first_row=1) == ERANGE and depth(n_rows=2) == ERANGE and band(first_row=1) == ERANGE and band(n_rows=2) == ERANGE
    assert depth(first_row=1, n_rows=0) == 0 and band(first_row=1, n_rows=0) == 0             # no rows, inside
    assert band(need=0) == ERANGE and band(need=4) == ERANGE and band(need=3) == 0 and b"need" in (lib.esim_last_error(ctx) if band(need=4) else b"")
    assert band(pooled=2) == EINVAL and band(pooled=-1) == EINVAL and band(pooled=1) == 0
    # every output NULL: the call still validates
    nothing = [None] * 5
    assert depth(d=None, t=None) == 0 and band(out=nothing) == 0 and band(out=nothing, pooled=1) == 0
    assert band(out=nothing, need=4) == ERANGE and band(out=nothing, n_rows=2) == ERANGE and depth(d=None, t=None, n_rows=2) == ERANGE
    assert band(out=[None, p[1], None, None, p[4]], need=3) == 0 and (planes[1][:3] == stack.max(axis=0)[0]).all() and (planes[4][:3] == 3).all()
    # nothing of it touched the store or the accumulators
    assert (sim.ensemble_members() == stack).all()
    got = sim.ensemble_read()
    assert all(np.array_equal(got[k], before[k]) for k in before)
    # a new begin ends the store
    sim.ensemble_begin("home", E | I | R, 1)
    assert depth() == ESTATE and band() == ESTATE and depth(d=None, t=None) == ESTATE


# ---- 6. the Python Ensemble -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ensemble():
    pop, base, members, steps = area_world()
    ens = Ensemble(pop, _lib.default_params(**base))
    yield ens, members, steps
    ens.close()


BAND_KEYS = ("band_lo", "band_hi", "band_median", "band_deepest", "band_n_in")


def assert_band_summary(area, stack, pooled, what):
    want = ref.band(stack, 3, pooled)                                # band=0.5 of six members
    for k in BAND_KEYS:
        assert (area[k] == want[k[5:]]).all() and area[k].shape == want[k[5:]].shape, (what, k)
    assert area["band_need"] == 3 and area["band_coverage"] == 0.5 and area["band_pooled"] is pooled
    assert np.array_equal(area["depth"], ref.depth(stack) / float(stack.shape[1] * 15)), what
    assert (area["band_lo"] < area["band_hi"]).any() and ((area["band_lo"] > stack.min(axis=0)) | (area["band_hi"] < stack.max(axis=0))).any(), what
    assert "quantiles" not in area and "probs" not in area


def test_ensemble_run_and_forecast_bands_equal_numpy_over_the_members_rows(ensemble, frozen_clock, tmp_path):
    ens, members, steps = ensemble
    sim = ens.simulator
    res = ens.run(members, steps, area=dict(SERIES_AREA, band=0.5))
    pooled = ens.run(members, steps, area=dict(SERIES_AREA, band=0.5, band_pooled=True))
    plain = ens.run(members, steps, area=SERIES_AREA)
    xs = []
    for m in members:
        sim.restart(ens.base, **m)
        sim.run(steps)
        xs.append(series_of(sim, "home", "incidence", **AREA_WINDOW))
    stack = np.asarray(xs)
    assert_band_summary(res.area, stack, False, "run")
    assert_band_summary(pooled.area, stack, True, "run, pooled")
    assert (pooled.area["band_median"] == stack[pooled.area["band_deepest"][0]]).all()          # one real member for the whole map
    assert not (res.area["band_deepest"] == res.area["band_deepest"][0]).all()
    assert not any(k.startswith("band_") or k == "depth" for k in plain.area)
    for k in plain.area:
        assert np.array_equal(res.area[k], plain.area[k], equal_nan=True) if isinstance(plain.area[k], np.ndarray) else res.area[k] == plain.area[k], k
    # the dump differs from the dump without the keys by the band's file only
    a, b = dumped(res, tmp_path / "with"), dumped(plain, tmp_path / "without")
    assert sorted(a) == sorted(list(b) + ["ensemble_area_band.npz"])
    for name in b:
        assert a[name] == b[name], name
    got = np.load(os.path.join(str(tmp_path / "with"), "ensemble_area_band.npz"))
    assert all((got[k] == res.area[k]).all() for k in BAND_KEYS + ("depth", "steps")) and int(got["band_need"]) == 3
    # beside the quantile maps: both files
    both = ens.run(members, steps, area=dict(SERIES_AREA, band=0.5, quantiles=(0.5,)))
    assert (both.area["band_lo"] == res.area["band_lo"]).all() and both.area["quantiles"].shape == (1,) + stack.shape[1:]
    assert sorted(dumped(both, tmp_path / "both")) == sorted(list(b) + ["ensemble_area_band.npz", "ensemble_area_quantiles.npz"])
    # a kind without rows: [n_cols]
    census = ens.run(members, steps, area=dict(kind="census", where="home", status_mask=E | I | R, min_cases=1, band=0.5)).area
    want = []
    for m in members:
        sim.restart(ens.base, **m)
        sim.run(steps)
        want.append(census_x(sim))
    want = ref.band(np.asarray(want), 3, False)
    assert census["band_lo"].shape == (sim.population.n_areas,) and all((census["band_" + k] == (want[k][0] if want[k].ndim == 2 else want[k])).all() for k in PLANES)
    # the forecast: every member a branch from a shared history
    history = 100
    fc = ens.forecast(history, members, steps, area=dict(SERIES_AREA, band=0.5))
    fcp = ens.forecast(history, members, steps, area=dict(SERIES_AREA, band=0.5, band_pooled=True))
    sim.restart(ens.base)
    sim.run(history)
    sim.snapshot()
    xs = []
    for m in members:
        sim.rollback(**m)
        sim.run(steps - history)
        xs.append(series_of(sim, "home", "incidence", **AREA_WINDOW))
    assert_band_summary(fc.area, np.asarray(xs), False, "forecast")
    assert_band_summary(fcp.area, np.asarray(xs), True, "forecast, pooled")
    with pytest.raises(ValueError):
        ens.run(members, steps, area=dict(kind="reproduction", where="home", band=0.5))
