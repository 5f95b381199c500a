"""Ensemble quantile maps through the library: esim_ensemble_keep_members and the store beside the accumulators of every kind,
esim_ensemble_read_members, esim_ensemble_quantiles, esim_ensemble_exceedance, and the Python Ensemble on top.  Every comparison
is exact integer equality.  The member stack comes from the existing per-member calls (area_census, area_arrival, the series
calls, setting_series, compare_series, curve_summary: their own tests pin these to the oracle), the order statistics and the
counts from numpy over that stack (tests/_members_ref.py) -- never from the code under test."""
import ctypes as C
import os

import numpy as np
import pytest

import _members_ref as ref
from epidemicsimulator_amd import Ensemble, Population, Simulator, _lib
from test_ensemble_gpu import area_world
from test_ensemble_series_gpu import AGE_EDGES, AREA_WINDOW, series_of

pytestmark = pytest.mark.gpu

EINVAL, ENOMEM, ESTATE, ERANGE = -1, -3, -4, -5
NEVER = _lib.NEVER
E, I, R = 1 << _lib.EXPOSED, 1 << _lib.INFECTED, 1 << _lib.RECOVERED
u32p, i64p = C.POINTER(C.c_uint32), C.POINTER(C.c_int64)
HORIZON = 120                                  # of the arrival kind: some areas are reached later in some members, some never
PAIRED_WINDOW = dict(first_step=0, n_rows=10, stride=25)
PEAKS = dict(where="home", status="infected", first_step=1, last_step=250, threshold=2)
TINY_WINDOWS = (dict(first_step=10, stride=80, n_rows=7), dict(first_step=300, stride=1, n_rows=1))    # 21 cells, 3 cells


def census_x(sim):
    return sim.area_census("home")[:, [_lib.EXPOSED, _lib.INFECTED, _lib.RECOVERED]].sum(axis=1, dtype=np.uint32)[None, :]


def arrival_x(sim):
    a = sim.area_arrival("home")
    return np.where(a <= HORIZON, a, NEVER).astype(np.uint32)[None, :]


def paired_x(cumulative):
    def x(sim):
        b, c = sim.compare_series("home", cumulative=cumulative, **PAIRED_WINDOW)
        return (b.astype(np.int64) - c.astype(np.int64)).astype(np.int32)
    return x


def peaks_x(key):
    return lambda sim: sim.curve_summary(**PEAKS)[key][None, :]


# kind -> (begin, the member's x by the existing call, what, the read call, (the accumulator that is the sum of x, min for hit))
KINDS = {
    "census": (lambda s: s.ensemble_begin("home", E | I | R, 2), census_x, "value", "ensemble_read", ("sum", 2)),
    "arrival": (lambda s: s.ensemble_begin_arrival("home", HORIZON), arrival_x, "value", "ensemble_read", (None, None)),
    "series-incidence": (lambda s: s.ensemble_begin_series("home", "incidence", min_cases=1, **AREA_WINDOW), lambda s: series_of(s, "home", "incidence", **AREA_WINDOW),
                         "value", "ensemble_read_series", ("sum", 1)),
    "series-infected-stood": (lambda s: s.ensemble_begin_series("current", "infected", min_cases=2, **AREA_WINDOW), lambda s: series_of(s, "current", "infected", **AREA_WINDOW),
                              "value", "ensemble_read_series", ("sum", 2)),
    "settings": (lambda s: s.ensemble_begin_settings("setting", min_cases=3, **AREA_WINDOW), lambda s: s.setting_series("setting", **AREA_WINDOW),
                 "value", "ensemble_read_series", ("sum", 3)),
    "paired": (lambda s: s.ensemble_begin_paired("home", min_baseline=0, min_averted=1, **PAIRED_WINDOW), paired_x(False), "value", "ensemble_read_paired", (None, 1)),
    "paired-cumulative": (lambda s: s.ensemble_begin_paired("home", cumulative=True, min_baseline=0, min_averted=2, **PAIRED_WINDOW), paired_x(True), "value",
                          "ensemble_read_paired", (None, 2)),
    "peaks-value": (lambda s: s.ensemble_begin_peaks(min_peak=3, **PEAKS), peaks_x("peak"), "value", "ensemble_read_peaks", ("sum_peak", 3)),
    "peaks-step": (lambda s: s.ensemble_begin_peaks(min_peak=3, **PEAKS), peaks_x("peak_step"), "peak_step", "ensemble_read_peaks", (None, None)),
    "peaks-duration": (lambda s: s.ensemble_begin_peaks(min_peak=3, **PEAKS), peaks_x("steps_at_least"), "duration", "ensemble_read_peaks", ("sum_duration", None)),
}


def fold_all(sim, members, steps, begin, x_of=None, keep=None, what="value", params=None):
    """begin, keep (unless None), then per member: restart (from `params`, the same for every kind), run, the member's x by the
    existing call, fold."""
    begin(sim)
    if keep is not None:
        sim.ensemble_keep_members(keep, what)
    xs = []
    for m in members:
        sim.restart(params, **m)
        sim.run(steps)
        if x_of is not None:
            xs.append(x_of(sim))
        sim.ensemble_fold()
    return np.asarray(xs)


def same_dicts(got, want, what):
    assert sorted(got) == sorted(want), what
    for k in got:
        assert np.array_equal(got[k], want[k]), (what, k)


def thresholds_for(stack):
    mid = int(np.sort(stack.reshape(-1))[stack.size // 2])
    return [0, 1, 2, mid, 5, NEVER, -1] if stack.dtype == np.uint32 else [-(1 << 31), -2, -1, 0, 1, 2, mid, 1 << 31]


def check_store(sim, stack, kind, never):
    """members, quantiles and exceedance of the store against the stack [members, rows, cols] and numpy over it."""
    m = stack.shape[0]
    info = sim.ensemble_members_info()
    assert info["kept"] == m and info["signed"] == (stack.dtype == np.int32), (kind, info)
    got = sim.ensemble_members()
    assert got.dtype == stack.dtype and got.shape == stack.shape and (got == stack).all(), (kind, "members")
    ranks = [0, 2, m - 1] if m > 2 else [0, m - 1]
    q = sim.ensemble_quantiles(ranks=ranks)
    assert q.dtype == stack.dtype and (q == ref.order_statistics(stack, ranks)).all(), (kind, "quantiles")
    thr = thresholds_for(stack)
    assert (sim.ensemble_exceedance(thr) == ref.exceedance(stack, thr, never=never)).all(), (kind, "exceedance")
    if stack.shape[1] > 2:                      # a range of rows, and of members
        assert (sim.ensemble_quantiles(ranks=[m - 1, 0], first_row=1, n_rows=2) == ref.order_statistics(stack[:, 1:3], [m - 1, 0])).all(), (kind, "rows 1..2")
        assert (sim.ensemble_members(first_member=1, n_members=m - 1, first_row=2, n_rows=1) == stack[1:, 2:3]).all(), (kind, "members 1.., row 2")
    return q


# ---- 1. every kind, six members ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def world():
    pop, base, members, steps = area_world()
    ep = _lib.default_params(**base)
    sim = Simulator(pop, ep)
    sim.run(steps)
    sim.keep_baseline()                         # of the paired kinds: the run under the base parameters
    yield sim, [dict(m, exposure_chance=0.0012) for m in members], members, steps, ep
    sim.close()


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_every_kind_over_six_members(world, kind):
    sim, policy, members, steps, ep = world
    begin, x_of, what, read, (sum_key, min_hit) = KINDS[kind]
    mem = policy if kind.startswith("paired") else members
    stack = fold_all(sim, mem, steps, begin, x_of, keep=len(mem), what=what, params=ep)
    assert stack.shape[0] == 6 and stack.dtype == (np.int32 if kind.startswith("paired") else np.uint32)
    never = kind in ("arrival", "peaks-step")
    q = check_store(sim, stack, kind, never)
    # the input is not trivial
    assert (q[0] < q[2]).any(), kind
    if kind.startswith("paired"):
        assert (stack != 0).any() and (stack == 0).all(axis=0).any()
    elif never:
        assert (stack == NEVER).all(axis=0).any() and (stack == NEVER).any(axis=0).sum() > (stack == NEVER).all(axis=0).sum() and (stack != NEVER).any()
    else:
        assert (stack == 0).all(axis=0).any() and (stack != 0).any()
    # the store is consistent with the moments
    acc = getattr(sim, read)()
    shape = stack.shape[1:] if read in ("ensemble_read_series", "ensemble_read_paired") else stack.shape[2:]
    if sum_key:
        assert (acc[sum_key].reshape(shape) == stack.astype(np.uint64).sum(axis=0).reshape(shape)).all(), kind
    if min_hit is not None:
        assert (acc["hit"].reshape(shape) == sim.ensemble_exceedance([min_hit])[0].reshape(shape)).all(), kind
    if kind == "arrival":
        assert (acc["hit"] == 6 - sim.ensemble_exceedance([NEVER])[0, 0]).all()
    # ... and the accumulators are what the same folds give without keeping
    fold_all(sim, mem, steps, begin, params=ep)
    with pytest.raises(_lib.EsimError) as err:
        sim.ensemble_members_info()
    assert err.value.code == ESTATE
    same_dicts(getattr(sim, read)(), acc, kind)


# ---- 2. by group ---------------------------------------------------------------------------------------------------------------
def test_by_group_over_five_age_bands(world):
    sim, _, members, steps, ep = world
    sim.set_groups(np.digitize(sim.population.age, AGE_EDGES).astype(np.uint16), 5)
    try:
        begin = lambda s: s.ensemble_begin_series("group", "exposures", min_cases=1, **AREA_WINDOW)
        stack = fold_all(sim, members, steps, begin, lambda s: s.group_series("exposures", **AREA_WINDOW), keep=6, params=ep)
        assert stack.shape == (6, AREA_WINDOW["n_rows"], 5)
        q = check_store(sim, stack, "group", False)
        assert (q[0] < q[2]).any()
        acc = sim.ensemble_read_series()
        assert (acc["sum"] == stack.astype(np.uint64).sum(axis=0)).all() and (acc["hit"] == sim.ensemble_exceedance([1])[0]).all()
        # new labels invalidate a store begun by group
        sim.set_groups(np.zeros(sim.population.n_citizens, np.uint16), 1)
        for call in (sim.ensemble_members_info, sim.ensemble_members, lambda: sim.ensemble_quantiles(ranks=[0]), lambda: sim.ensemble_exceedance([1])):
            with pytest.raises(_lib.EsimError) as err:
                call()
            assert err.value.code == ESTATE
    finally:
        sim.set_groups(None)


# ---- 3. member counts through the library: one member, the pad to 16, the LDS path ----------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    pop = Population.synthetic("york", n_citizens=600, n_areas=3, citizens_per_school=600, n_seeds=5)
    sim = Simulator(pop, _lib.default_params(exposure_chance=0.01, vaccination_threshold=0.011, vaccination_rate=25))
    yield sim
    sim.close()


@pytest.mark.parametrize("n_members", (1, 9, 65))
def test_member_counts(tiny, n_members):
    members = Ensemble.seeds(n_members, first=3)
    stack = fold_all(tiny, members, 200, lambda s: s.ensemble_begin("home", E | I | R, 1), census_x, keep=n_members)
    assert stack.shape == (n_members, 1, 3)
    check_store(tiny, stack, "census, %d members" % n_members, False)
    ranks = sorted({0, n_members // 2, n_members - 1})
    assert (tiny.ensemble_quantiles(ranks=ranks) == ref.order_statistics(stack, ranks)).all()
    if n_members > 1:
        assert (stack.min(axis=0) < stack.max(axis=0)).any()
        probs = (0.0, 0.05, 0.5, 0.95, 1.0)
        want = ref.order_statistics(stack, [ref.nearest_rank(p, n_members) for p in ("0", "1/20", "1/2", "19/20", "1")])
        assert (tiny.ensemble_quantiles(probs) == want).all()
        lin = tiny.ensemble_quantiles(probs, method="linear")
        assert np.allclose(lin, np.stack([ref.linear_quantile(stack, p) for p in probs]), rtol=1e-12, atol=0)


@pytest.mark.parametrize("window", TINY_WINDOWS, ids=["21cells", "3cells"])
def test_cell_counts_that_are_no_multiple_of_four(tiny, window):
    begin = lambda s: s.ensemble_begin_series("home", "infected", min_cases=1, **window)
    stack = fold_all(tiny, Ensemble.seeds(6, first=3), 540, begin, lambda s: series_of(s, "home", "infected", **window), keep=6)
    assert stack.shape[1] * stack.shape[2] in (21, 3) and stack.any()
    check_store(tiny, stack, "series, %d cells" % (stack.shape[1] * stack.shape[2]), False)


# ---- 4. under ESIM_GRID_CAP ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", (1, 3))
def test_capped_grids_give_identical_outputs_and_clip_every_new_launch_site(cap, monkeypatch):
    monkeypatch.setenv("ESIM_GRID_CAP", str(cap))
    # 800 areas: the kernels with a lane per column make four trips under a cap of one workgroup
    pop = Population.synthetic("york", n_citizens=8000, n_areas=800, citizens_per_school=4000, n_seeds=12, p_public_transport=0.4)
    members, steps = Ensemble.seeds(3, first=11), 250
    sim = Simulator(pop, _lib.default_params(exposure_chance=0.004))  # (the knob is read at the upload)
    try:
        stacks = {}
        sim.run(steps)
        sim.keep_baseline()
        for kind in ("series-incidence", "census", "arrival", "paired", "peaks-step"):
            begin, x_of, what, _, _ = KINDS[kind]
            stacks[kind] = fold_all(sim, members, steps, begin, x_of, keep=3, what=what)
            check_store(sim, stacks[kind], kind, kind in ("arrival", "peaks-step"))
        assert stacks["series-incidence"].shape == (3, 35, 800) and stacks["series-incidence"].any() and stacks["paired"].any()
        sites = {k: v for k, v in sim.debug_launches().items() if "esim_host_members.h" in k}
    finally:
        sim.close()
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "epidemicsimulator_amd", "csrc", "esim_host_members.h")).read().splitlines()
    lines = sorted(i + 1 for i, line in enumerate(text) if "grid_capped(" in line)
    assert len(lines) >= 5 and sorted(int(k.rsplit(":", 1)[1]) for k in sites) == lines, (sites, lines)
    for k, v in sites.items():
        assert v["launches"] >= 1 and v["clipped"] >= 1, (k, v)
    if cap == 1:
        assert all(v["max_trips"] >= 3 for v in sites.values()), sites


# ---- 5. errors and lifetime ----------------------------------------------------------------------------------------------------
def test_errors_and_lifetime(tiny):
    sim, lib, ctx = tiny, tiny.lib, tiny._ctx
    keep, fold = lib.esim_ensemble_keep_members, lib.esim_ensemble_fold
    out = np.zeros(4096, np.uint32)
    po = out.ctypes.data_as(u32p)
    ranks = (C.c_uint32 * 17)(*([0] * 17))
    thr = (C.c_int64 * 17)(*([1] * 17))
    quant = lambda first_row=0, n_rows=1, n=1, o=po, r=ranks: lib.esim_ensemble_quantiles(ctx, first_row, n_rows, r, n, o)
    exceed = lambda first_row=0, n_rows=1, n=1, o=po, t=thr: lib.esim_ensemble_exceedance(ctx, first_row, n_rows, t, n, o)
    members = lambda first=0, n=1, first_row=0, n_rows=1, o=po: lib.esim_ensemble_read_members(ctx, first, n, first_row, n_rows, o)
    fresh = Simulator(sim.population, sim.params)
    assert fresh.lib.esim_ensemble_keep_members(fresh._ctx, 4, 0) == ESTATE                   # before a begin
    assert fresh.lib.esim_ensemble_members_info(fresh._ctx, None, None, None, None) == ESTATE
    fresh.close()
    sim.restart(seed=5)
    sim.run(120)
    sim.ensemble_begin("home", E | I | R, 1)
    for bad in ((0, 0), (257, 0), (4, 3), (4, -1)):
        assert keep(ctx, *bad) == EINVAL, bad
    assert keep(ctx, 4, _lib.KEEP_PEAK_STEP) == EINVAL                                        # only the peaks kind has one
    assert quant() == ESTATE and exceed() == ESTATE and members() == ESTATE                   # no store
    assert keep(ctx, 2, 0) == 0
    assert keep(ctx, 3, 0) == 0                                                               # again, in front of the first fold: replaced
    assert sim.ensemble_members_info() == {"capacity": 3, "kept": 0, "what": "value", "signed": False}
    assert quant() == ESTATE and exceed() == ESTATE and members() == ESTATE                   # nothing kept yet
    sim.ensemble_fold()
    assert keep(ctx, 4, 0) == ESTATE                                                          # after a fold
    assert sim.ensemble_members_info()["kept"] == 1
    # the store survives restart, snapshot and rollback
    x0 = census_x(sim)
    sim.restart(seed=6)
    sim.run(60)
    sim.snapshot()
    sim.run(60)
    sim.ensemble_fold()
    x1 = census_x(sim)
    sim.rollback()
    sim.run(60)
    assert (census_x(sim) == x1).all()
    sim.ensemble_fold()
    stack = np.stack([x0, x1, x1])
    assert (sim.ensemble_members() == stack).all()
    records, state = sim.records_so_far(), sim.download_state()
    # the store is full: the fold is refused and nothing changes
    before = sim.ensemble_read()
    assert fold(ctx) == ERANGE and b"full" in lib.esim_last_error(ctx)
    same_dicts(sim.ensemble_read(), before, "a refused fold")
    assert before["members"] == 3 and sim.ensemble_members_info()["kept"] == 3 and (sim.ensemble_members() == stack).all()
    # ranks, rows, members and counts out of range; null pointers
    assert quant(r=(C.c_uint32 * 1)(3)) == ERANGE and quant(r=(C.c_uint32 * 1)(2)) == 0
    assert quant(first_row=1) == ERANGE and quant(n_rows=2) == ERANGE and exceed(first_row=1) == ERANGE and members(first_row=0, n_rows=2) == ERANGE
    assert members(first=3, n=1) == ERANGE and members(first=0, n=4) == ERANGE and members(first=2, n=1) == 0
    assert quant(n=0) == EINVAL and quant(n=17) == EINVAL and quant(n=16) == 0 and exceed(n=0) == EINVAL and exceed(n=17) == EINVAL and exceed(n=16) == 0
    assert quant(o=None) == EINVAL and exceed(o=None) == EINVAL and members(o=None) == EINVAL and quant(r=None) == EINVAL and exceed(t=None) == EINVAL
    assert (sim.ensemble_members() == stack).all()
    same_dicts(sim.ensemble_read(), before, "refused reads")
    # the reproduction kind keeps nothing; a second begin ends keeping and the fold works as before
    sim.ensemble_begin_reproduction("home", first_step=0, n_rows=2, stride=24)
    assert keep(ctx, 4, 0) == ESTATE and b"reproduction" in lib.esim_last_error(ctx)
    sim.ensemble_begin("home", E | I | R, 1)
    assert quant() == ESTATE and lib.esim_ensemble_members_info(ctx, None, None, None, None) == ESTATE
    for _ in range(4):
        sim.ensemble_fold()
    assert sim.ensemble_read()["members"] == 4 and (sim.ensemble_read()["sum"] == 4 * x1[0].astype(np.uint64)).all()
    # a store that cannot fit leaves the accumulators readable (nothing is asserted where the device takes it, or has no room
    # for the accumulators of so many rows themselves)
    try:
        sim.ensemble_begin_series("home", "infected", first_step=1, n_rows=1 << 27, stride=1)  # 403 M cells: 11 GB of accumulators, 1.6 GB a member
        big = True
    except _lib.EsimError as e:
        assert e.code == ENOMEM
        big = False
    if big:
        rc = keep(ctx, 256, 0)                                                               # 412 GB
        assert rc in (0, ENOMEM)
        if rc == ENOMEM:
            assert lib.esim_ensemble_members_info(ctx, None, None, None, None) == ESTATE
            assert sim.ensemble_read_series(first_row=0, n_rows=2)["members"] == 0
    sim.ensemble_begin_series("home", "infected", first_step=1, n_rows=1, stride=1)           # (the large accumulators go)
    # after all of it the simulation state and the records are what they were
    assert (sim.records_so_far() == records).all()
    again = sim.download_state()
    for k in state:
        assert (again[k] == state[k]).all(), k


# ---- 6. the Python Ensemble ----------------------------------------------------------------------------------------------------
SERIES_AREA = dict(kind="series", where="home", what="incidence", min_cases=1, **AREA_WINDOW)
PROBS, EXACT = (0.05, 0.5, 0.95), ("1/20", "1/2", "19/20")


@pytest.fixture(scope="module")
def ensemble():
    pop, base, members, steps = area_world()
    ens = Ensemble(pop, _lib.default_params(**base))
    yield ens, members, steps
    ens.close()


@pytest.fixture
def frozen_clock(monkeypatch):
    """np.savez stamps every entry of the archive with the time of day: two dumps compare byte for byte under one clock."""
    import time
    at = time.localtime(1700000000)
    monkeypatch.setattr(time, "localtime", lambda *a: at)


def dumped(result, directory):
    result.dump(str(directory))
    return {name: open(os.path.join(str(directory), name), "rb").read() for name in sorted(os.listdir(str(directory)))}


def assert_dumps_differ_by_the_quantile_file_only(with_keys, without, tmp_path):
    a, b = dumped(with_keys, tmp_path / "with"), dumped(without, tmp_path / "without")
    assert sorted(a) == sorted(list(b) + ["ensemble_area_quantiles.npz"])
    for name in b:
        assert a[name] == b[name], name
    return np.load(os.path.join(str(tmp_path / "with"), "ensemble_area_quantiles.npz"))


def test_ensemble_run_and_forecast_quantiles_equal_numpy_over_the_members_rows(ensemble, frozen_clock, tmp_path):
    ens, members, steps = ensemble
    sim = ens.simulator
    ranks = [ref.nearest_rank(p, len(members)) for p in EXACT]
    res = ens.run(members, steps, area=dict(SERIES_AREA, quantiles=PROBS, exceed=(1, 5)))
    plain = ens.run(members, steps, area=SERIES_AREA)
    xs = []
    for m in members:
        sim.restart(ens.base, **m)
        sim.run(steps)
        xs.append(series_of(sim, "home", "incidence", **AREA_WINDOW))
    stack = np.asarray(xs)
    assert res.area["quantiles"].shape == (3,) + stack.shape[1:] and (res.area["quantiles"] == ref.order_statistics(stack, ranks)).all()
    assert (res.area["quantiles"][0] < res.area["quantiles"][2]).any()
    assert (res.area["exceed"] == ref.exceedance(stack, (1, 5))).all() and res.area["probs"].tolist() == list(PROBS) and res.area["thresholds"].tolist() == [1, 5]
    assert "quantiles" not in plain.area
    for k in plain.area:
        assert np.array_equal(res.area[k], plain.area[k], equal_nan=True) if isinstance(plain.area[k], np.ndarray) else res.area[k] == plain.area[k], k
    lin = ens.run(members, steps, area=dict(SERIES_AREA, quantiles=PROBS, quantile_method="linear")).area["quantiles"]
    assert np.allclose(lin, np.stack([ref.linear_quantile(stack, p) for p in PROBS]), rtol=1e-12, atol=0)
    got = assert_dumps_differ_by_the_quantile_file_only(res, plain, tmp_path)
    assert (got["quantiles"] == res.area["quantiles"]).all() and (got["exceed"] == res.area["exceed"]).all() and got["probs"].tolist() == list(PROBS)
    # a kind without rows: [n_q, n_cols]
    census = ens.run(members, steps, area=dict(kind="census", where="home", status_mask=E | I | R, min_cases=1, quantiles=PROBS)).area
    want = []
    for m in members:
        sim.restart(ens.base, **m)
        sim.run(steps)
        want.append(census_x(sim)[0])
    assert census["quantiles"].shape == (3, sim.population.n_areas) and (census["quantiles"] == ref.order_statistics(np.asarray(want), ranks)).all()
    # the forecast: every member a branch from a shared history
    history = 100
    fc = ens.forecast(history, members, steps, area=dict(SERIES_AREA, quantiles=PROBS, exceed=(1, 5)))
    sim.restart(ens.base)
    sim.run(history)
    sim.snapshot()
    xs = []
    for m in members:
        sim.rollback(**m)
        sim.run(steps - history)
        xs.append(series_of(sim, "home", "incidence", **AREA_WINDOW))
    stack = np.asarray(xs)
    assert (fc.area["quantiles"] == ref.order_statistics(stack, ranks)).all() and (fc.area["exceed"] == ref.exceedance(stack, (1, 5))).all()
    assert (fc.area["quantiles"][0] < fc.area["quantiles"][2]).any()


def test_ensemble_compare_quantiles_of_the_cases_averted(ensemble, frozen_clock, tmp_path):
    ens, members, steps = ensemble
    sim = ens.simulator
    policy = {"exposure_chance": 0.0012}
    res = ens.compare({}, policy, members, steps, where="home", rows=dict(PAIRED_WINDOW), quantiles=PROBS)
    plain = ens.compare({}, policy, members, steps, where="home", rows=dict(PAIRED_WINDOW))
    xs = []
    for m in members:
        sim.restart(ens.base, **m)
        sim.run(steps)
        sim.keep_baseline()
        sim.restart(ens.base, **dict(policy, **m))
        sim.run(steps)
        xs.append(paired_x(False)(sim))
    stack = np.asarray(xs)
    ranks = [ref.nearest_rank(p, len(members)) for p in EXACT]
    assert res.averted_quantiles.dtype == np.int32 and (res.averted_quantiles == ref.order_statistics(stack, ranks)).all()
    assert (res.averted_quantiles[0] < res.averted_quantiles[2]).any() and plain.averted_quantiles is None
    got = assert_dumps_differ_by_the_quantile_file_only(res, plain, tmp_path)
    assert (got["quantiles"] == res.averted_quantiles).all()
    with pytest.raises(ValueError):
        ens.compare({}, policy, members, steps, where="home", quantiles=PROBS)                 # no rows to take them of
