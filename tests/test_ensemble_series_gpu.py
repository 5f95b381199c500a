"""Space-time ensembles: esim_ensemble_begin_series / esim_ensemble_fold / esim_ensemble_read_series and Ensemble(kind="series").
Every comparison is exact integer equality.  The references are two: the rows the existing series calls return for every member,
folded in numpy, and -- for every key -- the numpy tables of tests/_area_status_ref.py, tests/_area_ref.py and tests/_group_ref.py
over the CPU oracle's members, so that the engine is not only compared with itself."""
import ctypes as C
import functools

import numpy as np
import pytest

import _area_ref
import _area_status_ref
import _group_ref
import _oracle
from epidemicsimulator_amd import Ensemble, Population, Simulator, _lib
from test_ensemble_gpu import area_world
from test_parity_gpu import AGGRESSIVE

pytestmark = pytest.mark.gpu

EINVAL, ESTATE, ERANGE = -1, -4, -5
EVENTS = (5, "incidence", "exposures")


def series_of(sim, where, what, **window):
    """The rows of the existing series call that (where, what) names (the table of include/esim.h)."""
    if where == "group":
        return sim.group_series("exposures" if what in EVENTS else what, **window)
    if where == "current" and what in EVENTS:
        return sim.area_series("exposures", **window)
    return sim.area_status_series("incidence" if what in EVENTS else what, where, **window)


def numpy_fold(xs, min_cases):
    x = np.asarray(xs).astype(np.uint64)                       # [members, rows, cols]
    return {"members": x.shape[0], "hit": (x >= min_cases).sum(0).astype(np.uint32), "sum": x.sum(0), "sumsq": (x * x).sum(0)}


def assert_same_fold(got, want, what=""):
    assert got["members"] == want["members"], what
    for k in ("hit", "sum", "sumsq"):
        assert got[k].shape == want[k].shape and (got[k] == want[k]).all(), (what, k)


def fold_members(sim, members, steps, where, what, min_cases, window):
    """begin, then per member: restart, run, the member's rows by the existing call, fold.  Returns (read_series(), the rows)."""
    sim.ensemble_begin_series(where, what, min_cases=min_cases, **window)
    xs = []
    for m in members:
        sim.restart(**m)
        sim.run(steps)
        xs.append(series_of(sim, where, what, **window))
        sim.ensemble_fold()
    return sim.ensemble_read_series(), xs


@functools.lru_cache(maxsize=None)
def _oracle_tables(world, seed, n_steps):
    """The oracle's tables of one member of a world, computed once per session: the status and incidence tables of
    _area_status_ref, and the building exposures by the area stood in of _area_ref."""
    pop, base = world()
    ep = _lib.default_params(**dict(base, seed=seed))
    ref = _area_status_ref.reference_tables(pop, ep, n_steps)
    orc = _oracle.Oracle(pop, _oracle.params_from_esim(ep))
    orc.run(n_steps)
    step, area = orc.exposures()
    orc.close()
    ref["exposures"] = _area_ref.exposure_rows(pop, step, area, n_steps)
    return ref


def oracle_rows(world, seed, n_steps, where, what, window):
    """x of one member from the oracle."""
    ref = _oracle_tables(world, seed, n_steps)
    if where == "current" and what in EVENTS:
        return _area_status_ref.expected({"incidence": ref["exposures"]}, "home", "incidence", n_steps, **window)
    return _area_status_ref.expected(ref, where, "incidence" if what in EVENTS else what, n_steps, **window)


# ---- 1. areas, six members ---------------------------------------------------------------------------------------------------
AREA_WINDOW = dict(first_step=3, stride=7, n_rows=35)          # 35 x 64 = 2240 cells, the last row is step 241 of 250
# The first four are the configurations the feature was specified with.  Nobody recovers in this world before step 337 (the
# index cases are Infected for infected_time + 1 steps), so the Recovered rows are zero in every cell of every member: that
# configuration checks the pass that touches nothing, the non-triviality is asserted for the others, and the Exposed rows are
# added so that a status by household area is folded with counts in it.
AREA_CONFIGS = (("home", "recovered", 1), ("current", "infected", 2), ("home", "incidence", 1), ("current", 5, 0), ("home", "exposed", 1))


def area_base():
    pop, base, _, _ = area_world()
    return pop, base


@pytest.mark.parametrize("where,what,min_cases", AREA_CONFIGS)
def test_area_rows_over_six_members_equal_numpy_over_the_series_calls_and_over_the_oracle(where, what, min_cases):
    pop, base, members, steps = area_world()
    assert pop.n_areas == 64 and len(members) == 6 and steps == 250
    sim = Simulator(pop, _lib.default_params(**base))
    got, xs = fold_members(sim, members, steps, where, what, min_cases, AREA_WINDOW)
    sim.close()
    x = np.asarray(xs)
    assert x.shape == (6, 35, 64)
    if what == "recovered":
        assert not x.any()
    else:
        # the input is not trivial: a cell hit in some members only, a cell with x == 0 in a member
        hits = (x >= max(1, min_cases)).sum(0)
        assert ((hits > 0) & (hits < len(members))).any() and (x == 0).any()
    assert_same_fold(got, numpy_fold(xs, min_cases), "series calls")
    if min_cases == 0:
        assert (got["hit"] == got["members"]).all()            # (a zero-skip applied to hit would miss the zero cells)
    want = [oracle_rows(area_base, m["seed"], steps, where, what, AREA_WINDOW) for m in members]
    assert_same_fold(got, numpy_fold(want, min_cases), "oracle")


# ---- 2. the tail and alignment -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where,what", (("home", "infected"), ("current", "recovered"), ("home", "incidence")))
def test_cell_counts_that_are_no_multiple_of_four(where, what):
    pop = Population.synthetic("york", n_citizens=600, n_areas=3, citizens_per_school=600, n_seeds=5)
    base = dict(exposure_chance=0.01, vaccination_threshold=0.011, vaccination_rate=25)
    members, steps = Ensemble.seeds(3, first=3), 540
    sim = Simulator(pop, _lib.default_params(**base))
    for window in (dict(first_step=10, stride=80, n_rows=7), dict(first_step=300, stride=1, n_rows=1)):     # 21 cells, 3 cells
        got, xs = fold_members(sim, members, steps, where, what, 1, window)
        assert (window["n_rows"] * pop.n_areas) % 4 and len(sim.exposure_events()[0]) + len(pop.seeds) < 64
        want = numpy_fold(xs, 1)
        assert_same_fold(got, want, window)
        if window["n_rows"] == 7:
            assert want["sum"].any()
            part = sim.ensemble_read_series(first_row=2, n_rows=3)
            assert_same_fold(part, {k: v if k == "members" else v[2:5] for k, v in want.items()}, "rows 2..4")
            assert sim.ensemble_read_series(first_row=7)["hit"].shape == (0, 3)
    sim.close()


# ---- 3. under a vaccination programme ------------------------------------------------------------------------------------------
VAX_WINDOW = dict(first_step=150, stride=5, n_rows=30)          # steps 150 .. 295 of 300
VAX_MEMBERS = [{"seed": 77}, {"seed": 78}, {"seed": 79}]
AGE_EDGES = (16, 35, 50, 65)                                   # five age bands


def vax_base():
    return vax_world()[0], dict(AGGRESSIVE)


@functools.lru_cache(maxsize=None)
def vax_world():
    pop = Population.synthetic("york", n_citizens=6000, n_areas=20, citizens_per_school=3000, n_seeds=12, p_public_transport=0.4)
    labels, n_groups = pop.age_bands(AGE_EDGES)
    assert n_groups == 5
    return pop, labels, n_groups


@pytest.mark.parametrize("where,what", (("home", "vaccinated"), ("current", "susceptible"), ("group", "infected")))
def test_rows_under_a_vaccination_programme(where, what):
    pop, labels, n_groups = vax_world()
    steps = 300
    sim = Simulator(pop, _lib.default_params(**AGGRESSIVE))
    sim.set_groups(labels, n_groups)
    sim.ensemble_begin_series(where, what, min_cases=1, **VAX_WINDOW)
    xs = []
    for m in VAX_MEMBERS:
        sim.restart(**m)
        rec = sim.run(steps)
        start = int(np.argmax(rec["vaccination_active"])) + 1
        assert rec["vaccination_active"].any() and VAX_WINDOW["first_step"] < start < 295 and rec["vaccinated"][-1] > 0   # starts inside the window
        xs.append(series_of(sim, where, what, **VAX_WINDOW))
        sim.ensemble_fold()
    got = sim.ensemble_read_series()
    sim.close()
    assert_same_fold(got, numpy_fold(xs, 1), "series calls")
    want = []
    for m in VAX_MEMBERS:
        if where == "group":
            ep = _lib.default_params(**dict(AGGRESSIVE, **m))
            rows = _group_ref.reference_tables(pop, ep, labels, n_groups, steps)["status_rows"]
            want.append(rows[VAX_WINDOW["first_step"] - 1:steps:VAX_WINDOW["stride"], :, _lib.INFECTED][:VAX_WINDOW["n_rows"]])
        else:
            want.append(oracle_rows(vax_base, m["seed"], steps, where, what, VAX_WINDOW))
    assert_same_fold(got, numpy_fold(want, 1), "oracle")


# ---- 4. groups at the cap ------------------------------------------------------------------------------------------------------
def test_exposure_rows_of_1024_groups():
    pop, base, members, steps = area_world()
    labels = ((np.arange(pop.n_citizens, dtype=np.uint64) * 2654435761 >> 7) % 1024).astype(np.uint16)
    assert len(np.unique(labels)) == 1024
    window = dict(first_step=1, stride=50, n_rows=5)
    sim = Simulator(pop, _lib.default_params(**base))
    sim.set_groups(labels, 1024)
    got, xs = fold_members(sim, members[:2], steps, "group", 5, 1, window)
    sim.close()
    assert got["hit"].shape == (5, 1024) and np.asarray(xs).any()
    assert_same_fold(got, numpy_fold(xs, 1), "series calls")
    want = []
    for m in members[:2]:
        orc = _oracle.Oracle(pop, _oracle.params_from_esim(_lib.default_params(**dict(base, **m))))
        orc.run(steps)
        step, _ = orc.exposures()
        orc.close()
        ref = {"incidence": _group_ref.exposure_rows(labels, 1024, step, steps)}
        want.append(_area_status_ref.expected(ref, "home", "incidence", steps, **window))
    assert_same_fold(got, numpy_fold(want, 1), "oracle")


# ---- 5. forecast ---------------------------------------------------------------------------------------------------------------
def test_forecast_folds_a_window_that_straddles_the_snapshot():
    pop, _, _ = vax_world()
    policies = [{"seed": 5, "vaccination_rate": 10}, {"seed": 6, "vaccination_rate": 40}, {"seed": 7, "vaccination_rate": 120}]
    window = dict(first_step=100, n_rows=30, stride=5)             # steps 100 .. 245: the snapshot's step 120 lies inside
    ens = Ensemble(pop, _lib.default_params(**AGGRESSIVE))
    res = ens.forecast(history_steps=120, members=policies, n_steps=250, area=dict(kind="series", where="home", what="infected", **window))
    assert res.n_done.tolist() == [250] * 3
    sim = ens.simulator
    xs = []
    for m in policies:                                             # the snapshot is still held: every branch once more, by hand
        sim.rollback(**m)
        sim.run(130)
        xs.append(sim.area_status_series("infected", "home", **window))
    assert any(r["vaccinated"][-1] > 0 for r in res.records) and (xs[0] != xs[1]).any() and (xs[0][:4] == xs[1][:4]).all()
    want = numpy_fold(xs, 1)
    a = res.area
    assert a["members"] == 3 and (a["hit"] == want["hit"]).all() and a["steps"].tolist() == list(range(100, 250, 5))
    raw = sim.ensemble_read_series()                                # (rollback and run left the accumulators alone)
    assert_same_fold(raw, want, "forecast")
    x = np.asarray(xs, np.float64)
    assert np.allclose(a["mean"], x.mean(0), rtol=1e-12, atol=0) and np.allclose(a["var"], x.var(0), rtol=1e-9, atol=1e-9)
    ens.close()


# ---- 6. errors and lifetime ----------------------------------------------------------------------------------------------------
def read_codes(sim, first_row=0, n=0):
    return sim.lib.esim_ensemble_read_series(sim._ctx, first_row, n, None, None, None, None)


def test_errors_and_lifetime():
    pop, labels, n_groups = vax_world()
    lib = _lib.load()
    ctx = C.c_void_p()
    _lib.check(lib.esim_create(C.byref(_lib.default_params()), C.byref(ctx)))
    assert lib.esim_ensemble_begin_series(ctx, _lib.AREA_HOME, _lib.INFECTED, 1, 4, 1, 1) == ESTATE      # before an upload
    assert lib.esim_ensemble_read_series(ctx, 0, 0, None, None, None, None) == ESTATE
    lib.esim_destroy(ctx)
    sim = Simulator(pop, _lib.default_params(**AGGRESSIVE))
    begin = lambda *a: sim.lib.esim_ensemble_begin_series(sim._ctx, *a)
    assert sim.lib.esim_ensemble_fold(sim._ctx) == ESTATE and read_codes(sim) == ESTATE                     # before begin
    for bad in ((7, 2, 1, 4, 1, 1), (_lib.AREA_HOME, 6, 1, 4, 1, 1), (_lib.AREA_HOME, -1, 1, 4, 1, 1), (_lib.AREA_HOME, 2, 1, 4, 0, 1), (_lib.AREA_HOME, 2, 1, 0, 1, 1)):
        assert begin(*bad) == EINVAL, bad
    assert begin(_lib.AREA_HOME, 2, 0, 4, 1, 1) == ERANGE
    assert begin(_lib.BY_GROUP, 2, 1, 4, 1, 1) == ESTATE                                                    # by group without labels
    assert sim.lib.esim_ensemble_fold(sim._ctx) == ESTATE                                                   # (none of these began anything)
    window = dict(first_step=3, stride=7, n_rows=10)                                                        # the last row is step 66
    sim.ensemble_begin_series("home", "infected", **window)
    sim.run(70)
    x1 = sim.area_status_series("infected", "home", **window)
    state, rec, census = sim.download_state(), sim.records_so_far(), sim.area_census("home")
    sim.ensemble_fold()
    after = sim.download_state()
    assert all((after[k] == state[k]).all() for k in state) and (sim.records_so_far() == rec).all() and (sim.area_census("home") == census).all()
    one = numpy_fold([x1], 1)
    assert_same_fold(sim.ensemble_read_series(), one, "one member")
    # the other read, and rows outside
    assert sim.lib.esim_ensemble_read(sim._ctx, None, None, None, None) == ESTATE
    assert b"esim_ensemble_read_series" in sim.lib.esim_last_error(sim._ctx)
    assert read_codes(sim, 8, 3) == ERANGE and read_codes(sim, 11, 0) == ERANGE and read_codes(sim, 8, 2) == 0
    # a member that has not run to the last row: refused, nothing folded
    sim.restart(seed=5)
    sim.run(50)
    assert sim.lib.esim_ensemble_fold(sim._ctx) == ERANGE
    assert_same_fold(sim.ensemble_read_series(), one, "after the refused fold")
    # kept through snapshot, rollback, reset and restart
    sim.run(30)
    sim.snapshot()
    sim.run(10)
    sim.rollback()
    assert_same_fold(sim.ensemble_read_series(), one, "after rollback")
    x2 = sim.area_status_series("infected", "home", **window)
    sim.ensemble_fold()
    sim.reset()
    sim.restart(seed=9)
    assert_same_fold(sim.ensemble_read_series(), numpy_fold([x1, x2], 1), "after reset and restart")
    # a census kind replaces the series kind, and the other way round
    sim.ensemble_begin("home")
    assert read_codes(sim) == ESTATE and sim.lib.esim_ensemble_fold(sim._ctx) == 0
    assert sim.ensemble_read()["members"] == 1
    # by group: set_groups invalidates
    sim.set_groups(labels, n_groups)
    sim.ensemble_begin_series("group", "exposed", first_step=1, n_rows=3, stride=1)
    sim.run(5)
    sim.ensemble_fold()
    assert sim.ensemble_read_series()["hit"].shape == (3, n_groups)
    sim.set_groups(labels, n_groups)
    assert sim.lib.esim_ensemble_fold(sim._ctx) == ESTATE and read_codes(sim) == ESTATE
    # a new upload drops them
    sim.ensemble_begin_series("home", "infected", **window)
    ps = pop.as_struct()
    _lib.check(sim.lib.esim_upload_population(sim._ctx, C.byref(ps)), sim._ctx)
    assert sim.lib.esim_ensemble_fold(sim._ctx) == ESTATE and read_codes(sim) == ESTATE
    sim.close()


def test_a_context_with_a_communicator_of_two_ranks_is_refused():
    whole = Population.synthetic("york", n_citizens=20000, n_areas=64, citizens_per_school=2500)
    cuts = whole.even_cuts(2)
    s0, s1 = whole.shard(cuts, 0), whole.shard(cuts, 1)
    sim = Simulator(s0, _lib.default_params())

    def allreduce(user, which, host_ptr, n_u32):
        if which == 8:                                   # the set-up's layout check: rank 1's row, as its process would add it
            a = (C.c_uint32 * n_u32).from_address(host_ptr)
            a[5:10] = [s0.n_citizens, s1.n_citizens, whole.n_citizens, s1.n_shared_buildings, s1.n_shared_rooms]
        return 0

    cb = _lib.ALLREDUCE_FN(allreduce)
    _lib.check(sim.lib.esim_comm_init_callback(sim._ctx, cb, None, 0, 2), sim._ctx)
    assert sim.lib.esim_ensemble_begin_series(sim._ctx, _lib.AREA_HOME, _lib.INFECTED, 1, 4, 1, 1) == ESTATE
    assert sim.lib.esim_ensemble_fold(sim._ctx) == ESTATE
    sim.close()
