"""esim_area_status_series against tables computed with numpy from the CPU oracle (tests/_area_status_ref.py), and against the
library's other read-backs.  Every comparison is exact equality of integer arrays, every table is compared in full."""
import ctypes as C

import numpy as np
import pytest

import _area_ref
import _area_status_ref as ref_mod
import _group_ref
from epidemicsimulator_amd import Population, Simulator, _lib

pytestmark = pytest.mark.gpu

FIELDS = [f for f in _lib.RECORD_FIELDS if f != "reserved"]
N_STEPS = _area_ref.FIXTURE_A_STEPS
STOPS = (1, 96, 300, 700)
STATUS, TABLES = ref_mod.STATUS, ref_mod.TABLES
S, E, I, R, V = range(5)
EINVAL, ESTATE, ERANGE = -1, -4, -5
u32p = C.POINTER(C.c_uint32)


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, "%s: shape %s, expected %s" % (what, got.shape, want.shape)
    if not (got == want).all():
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d entries differ, first at %s: got %d, expected %d"
                             % (what, len(bad), bad[0].tolist(), int(got[tuple(bad[0])]), int(want[tuple(bad[0])])))


def check_all(sim, ref, t_done, note="", **window):
    """All eleven tables of the window (default: every step run, stride 1) against the reference."""
    for where, what in TABLES:
        got = sim.area_status_series(what, where, **window)
        assert got.dtype == np.uint32
        same(got, ref_mod.expected(ref, where, what, t_done, **window), "%s by %s, %d steps run, %s %s" % (what, where, t_done, window, note))


def check_records(sim, ref):
    got = sim.records_so_far()
    for f in FIELDS:
        same(got[f], ref["records"][f][:len(got)], "record field %s" % f)


def params_dict(ep):
    return {n: getattr(ep, n) for n, _ in _lib.Params._fields_}


def with_seeds(pop, seeds):
    kw = {n: getattr(pop, n) for n in ("home_building", "work_building", "room", "flags", "age", "occupation", "building_area",
                                       "building_type", "room_building")}
    return Population(seeds=np.asarray(seeds, np.uint32), n_areas=pop.n_areas, **kw)


@pytest.fixture(scope="module")
def world():
    return ref_mod.fixture_a_tables()


# ---- 1. every table at every stop, in both step forms; the calls leave the run alone -----------------------------------------
@pytest.mark.parametrize("pipeline", [None, 0], ids=["default", "sequential"])
def test_all_tables_follow_the_oracle_and_the_calls_leave_the_run_alone(world, pipeline):
    pop, ep, ref = world
    sim = Simulator(pop, ep)
    if pipeline is not None:
        sim.set_pipeline(pipeline)
    done = 0
    for s in STOPS:
        sim.run(s - done)
        done = s
        check_all(sim, ref, s)
    check_records(sim, ref)
    state = sim.download_state()
    for k in ("status", "timer", "current_building", "on_bus", "eligible"):
        same(state[k], ref["final_state"][k], "final state %s" % k)
    sim.close()


@pytest.fixture(scope="module")
def finished_run(world):
    pop, ep, ref = world
    sim = Simulator(pop, ep)
    sim.run(N_STEPS)
    yield sim
    sim.close()


# ---- 2. strides and windows ------------------------------------------------------------------------------------------------------
def test_strides_and_windows(world, finished_run):
    pop, ep, ref = world
    sim, rec = finished_run, ref["records"]
    locked = int(np.argmax(rec["lockdown"])) + 3                       # a first step inside the lockdown
    assert rec["lockdown"][locked - 1] and rec["lockdown"][locked + 48]
    inside = int(np.argmax(rec["vaccination_active"])) + 3            # ... and one behind the programme's trigger step
    assert rec["vaccination_active"][inside - 1] and rec["vaccinated_now"][inside - 1] > 0
    for first in (5, locked, inside):
        for stride in (7, 24):
            check_all(sim, ref, N_STEPS, first_step=first, stride=stride)
            check_all(sim, ref, N_STEPS, first_step=first, n_rows=3, stride=stride)
    check_all(sim, ref, N_STEPS, first_step=inside, n_rows=1, stride=1)
    check_all(sim, ref, N_STEPS, first_step=N_STEPS, n_rows=1, stride=50)
    check_all(sim, ref, N_STEPS, first_step=N_STEPS - 99, n_rows=100, stride=1)          # a last row at exactly step 700
    check_all(sim, ref, N_STEPS, first_step=N_STEPS - 10 * 7, n_rows=11, stride=7)
    # a window behind the start of intervals that are still open: by step 600 most of the Recovered and Vaccinated have been so
    # for long, and so has everybody no longer Susceptible
    assert ref["home"][598, :, R].sum() > 0 and ref["home"][598, :, V].sum() > 0
    check_all(sim, ref, N_STEPS, first_step=600, stride=1)
    check_all(sim, ref, N_STEPS, first_step=600, n_rows=9, stride=11)


# ---- 3. consistency on the device alone --------------------------------------------------------------------------------------
def test_consistency_with_the_other_read_backs(world, finished_run):
    pop, ep, ref = world
    sim = finished_run
    same(sim.area_status_series("infected", "current"), sim.area_series("infected"), "(CURRENT, INFECTED) vs esim_area_series")
    same(sim.area_status_series(_lib.INFECTED, _lib.AREA_CURRENT, first_step=5, stride=7), sim.area_series("infected", first_step=5, stride=7),
         "(CURRENT, INFECTED) vs esim_area_series, stride 7")
    sim.set_groups(ref_mod.home_area_labels(pop), pop.n_areas)
    try:
        for name in STATUS:
            same(sim.area_status_series(name, "home"), sim.group_series(name), "%s by home area vs by group" % name)
            same(sim.area_status_series(name, "home", first_step=3, stride=24), sim.group_series(name, first_step=3, stride=24), "%s, stride 24" % name)
        same(sim.area_status_series("incidence"), sim.group_series("exposures"), "incidence vs the groups' exposure rows")
        same(sim.area_status_series(_lib.AREA_SERIES_INCIDENCE, first_step=3, stride=24), sim.group_series("exposures", first_step=3, stride=24), "incidence, stride 24")
    finally:
        sim.set_groups(None)
    for where in ("home", "current"):
        census = sim.area_census(where)
        for k, name in enumerate(STATUS):
            same(sim.area_status_series(name, where)[-1], census[:, k], "last %s row by %s vs the census" % (name, where))
            same(sim.area_status_series(name, where, first_step=N_STEPS, n_rows=1)[0], census[:, k], "the one row of step 700")


# ---- 4. citizens that are not home-sorted ---------------------------------------------------------------------------------------
def test_population_that_is_not_home_sorted(world):
    pop, ep, _ = world
    per = _area_ref.permuted(pop)
    ref = ref_mod.reference_tables(per, ep, 400)
    sim = Simulator(per, ep)
    sim.run(400)
    check_records(sim, ref)
    check_all(sim, ref, 400)
    sim.close()


# ---- 5. high prevalence ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def high_prevalence():
    pop, _ = _area_ref.fixture_a()
    ep = _lib.default_params(**_group_ref.HIGH_PREVALENCE)
    return pop, ep, ref_mod.reference_tables(pop, ep, _group_ref.HIGH_PREVALENCE_STEPS)


@pytest.mark.parametrize("pipeline", [None, 0], ids=["default", "sequential"])
def test_high_prevalence(high_prevalence, pipeline):
    """Most of the population leaves Susceptible, and Exposed, Infected and Recovered citizens are among the vaccinated."""
    pop, ep, ref = high_prevalence
    n = _group_ref.HIGH_PREVALENCE_STEPS
    assert ref["records"]["infected"].max() > 0.3 * pop.n_citizens and ref["records"]["vaccination_active"].any()
    sim = Simulator(pop, ep)
    if pipeline is not None:
        sim.set_pipeline(pipeline)
    sim.run(n)
    check_records(sim, ref)
    check_all(sim, ref, n)
    check_all(sim, ref, n, first_step=4, stride=24)
    sim.close()


# ---- 6. small worlds -------------------------------------------------------------------------------------------------------------
def commuting_world():
    """Two Output Areas: the school and every work place in area 0, three households in four in area 1, so that most of those
    who work cross the boundary twice a day."""
    base = Population.synthetic("york", n_citizens=9000, n_areas=2, citizens_per_school=9000, n_seeds=40, p_public_transport=0.5)
    area = np.zeros(base.n_buildings, np.uint32)
    households = np.flatnonzero(base.building_type == _lib.HOUSEHOLD)
    area[households[len(households) // 4:]] = 1
    names = ("home_building", "work_building", "room", "flags", "age", "occupation", "building_type", "room_building", "seeds")
    pop = Population(building_area=area, n_areas=2, **{n: getattr(base, n) for n in names})
    works = pop.home_building != pop.work_building
    crossing = pop.building_area[pop.home_building] != pop.building_area[pop.work_building]
    assert crossing[works].mean() > 0.5
    return pop


@pytest.fixture(scope="module")
def small_worlds():
    """(pop, ep, reference tables, building-exposure rows by the area stood in) of the two worlds, computed once."""
    out = []
    for pop, ep, n in (
            # three areas, 500 citizens
            (Population.synthetic("york", n_citizens=500, n_areas=3, citizens_per_school=500, n_seeds=5),
             _lib.default_params(exposure_chance=0.003, vaccination_threshold=0.02, vaccination_rate=2, lockdown_threshold=0.05, seed=3), 400),
            # two areas, most workers commuting across the boundary: the two planes differ for most citizens
            (commuting_world(),
             _lib.default_params(exposure_chance=0.01, vaccination_threshold=0.1, vaccination_rate=20, lockdown_threshold=0.2, seed=5), 500)):
        out.append((pop, ep, ref_mod.reference_tables(pop, ep, n), _area_ref.reference_tables(pop, ep, n)["exposure_rows"]))
    return out


def check_other_entry_points(sim, pop, ref, exposure_rows, t_done, note):
    """esim_area_series and, with the home area as the label, esim_group_series against the numpy reference itself: after the
    fold all three entry points run one engine, so comparing them with each other would compare a code path with itself."""
    same(sim.area_series("infected"), ref_mod.expected(ref, "current", "infected", t_done), "area_series infected, %s" % note)
    assert exposure_rows[:t_done].any()
    same(sim.area_series("exposures"), exposure_rows[:t_done], "area_series exposures, %s" % note)
    sim.set_groups(ref_mod.home_area_labels(pop), pop.n_areas)
    try:
        # every step run; and the one row of the last step run: every interval that reaches it has nothing behind it
        for window in (dict(first_step=1, stride=1), dict(first_step=t_done, n_rows=1)):
            for name in STATUS:
                want = ref_mod.expected(ref, "home", name, t_done, **window)
                same(sim.group_series(name, **window), want, "group_series %s by home-area label, %s %s" % (name, window, note))
            want = ref_mod.expected(ref, "home", "incidence", t_done, **window)
            same(sim.group_series("exposures", **window), want, "group_series exposures by home-area label, %s %s" % (window, note))
    finally:
        sim.set_groups(None)


@pytest.mark.parametrize("pipeline", [None, 0], ids=["default", "sequential"])
def test_small_worlds(small_worlds, pipeline):
    # three areas, 500 citizens: asked while the exposure log is shorter than one wavefront, and again at the end
    pop, ep, ref, exposure_rows = small_worlds[0]
    rec = ref["records"]
    entries = len(np.unique(pop.seeds)) + np.cumsum(rec["exposures_building"].astype(np.int64) + rec["exposures_bus"])
    early = int(np.flatnonzero(entries < 64)[-1]) + 1
    assert early >= 100 and entries[early - 1] > len(np.unique(pop.seeds)) and rec["vaccination_active"].any() and rec["lockdown"].any()
    sim = Simulator(pop, ep)
    if pipeline is not None:
        sim.set_pipeline(pipeline)
    sim.run(early)
    check_all(sim, ref, early, "three areas, a log below 64 entries")
    check_other_entry_points(sim, pop, ref, exposure_rows, early, "three areas, a log below 64 entries")
    sim.run(400 - early)
    check_records(sim, ref)
    check_all(sim, ref, 400, "three areas")
    check_other_entry_points(sim, pop, ref, exposure_rows, 400, "three areas")
    for name in STATUS:                                               # (the reference tables of this world are not empty)
        assert ref["home"][:, :, STATUS.index(name)].any() and ref["current"][:, :, STATUS.index(name)].any()
    sim.close()
    # two areas, most workers commuting across the boundary: the two planes differ for most citizens
    pop, ep, ref, exposure_rows = small_worlds[1]
    assert ref["records"]["vaccination_active"].any() and ref["records"]["lockdown"].any() and ref["records"]["exposures_bus"].sum() > 0
    assert (ref["current"] != ref["home"]).any()
    assert (exposure_rows != ref["incidence"]).any()                  # (by the area stood in and without the buses: another table)
    sim = Simulator(pop, ep)
    if pipeline is not None:
        sim.set_pipeline(pipeline)
    sim.run(500)
    check_records(sim, ref)
    check_all(sim, ref, 500, "two areas")
    check_all(sim, ref, 500, "two areas", first_step=2, stride=5)
    check_other_entry_points(sim, pop, ref, exposure_rows, 500, "two areas")
    sim.close()


# ---- 7. members on one context ---------------------------------------------------------------------------------------------------
def test_members_on_one_context(world):
    pop, ep, ref = world
    base = params_dict(ep)
    sim = Simulator(pop, ep)
    sim.run(300)
    check_all(sim, ref, 300, "the first member", first_step=2, stride=9)
    over = dict(seed=77, exposure_chance=0.008, vaccination_threshold=0.03, exposed_time=60, infected_time=150)
    other = ref_mod.reference_tables(pop, _lib.default_params(**dict(base, **over)), 260)
    assert other["records"]["vaccination_active"].any()
    sim.restart(**over)
    sim.run(260)
    check_records(sim, other)
    check_all(sim, other, 260, "after esim_restart")
    seeds = np.random.default_rng(5).permutation(pop.n_citizens)[:33]
    ep3 = _lib.default_params(**dict(base, seed=9))
    third = ref_mod.reference_tables(with_seeds(pop, seeds), ep3, 240)
    sim.restart(ep3, seeds=seeds)
    sim.run(240)
    check_records(sim, third)
    check_all(sim, third, 240, "after esim_restart_seeded")
    sim.close()


# ---- 8. the york preset, 5000 steps, no oracle ----------------------------------------------------------------------------------
def test_york_self_consistency():
    pop = Population.synthetic("york")
    sim = Simulator(pop, _lib.default_params())
    rec = sim.run(5000)
    assert len(rec) == 5000
    state = sim.download_state()
    home_area = pop.building_area[pop.home_building]
    residents = np.bincount(home_area, minlength=pop.n_areas)
    total = {w: np.zeros((100, pop.n_areas), np.int64) for w in ("home", "current")}
    for where in ("home", "current"):
        census = sim.area_census(where)
        same(census, _area_ref.census_table(pop, state, where), "census by %s vs download_state" % where)
        for k, name in enumerate(STATUS):
            rows = sim.area_status_series(name, where, first_step=50, stride=50)
            assert rows.shape == (100, pop.n_areas)
            same(rows[-1], census[:, k], "last %s row by %s vs the census" % (name, where))
            total[where] += rows
    same(total["home"], np.broadcast_to(residents, total["home"].shape), "rows by home area summed over the statuses vs the residents")
    same(total["current"].sum(axis=1), np.full(100, pop.n_citizens), "rows by the area stood in, summed")
    same(sim.area_status_series("infected", "current", first_step=50, stride=50), sim.area_series("infected", first_step=50, stride=50),
         "(CURRENT, INFECTED) vs esim_area_series")
    cit, step, _ = sim.exposure_events()
    want = np.bincount(home_area[cit[step >= 1]], minlength=pop.n_areas)
    full = sim.area_status_series("incidence")
    assert full.shape == (5000, pop.n_areas)
    same(full.sum(axis=0, dtype=np.int64), want, "incidence rows summed over time vs the exposure log by home area")
    same(full.sum(axis=1, dtype=np.int64), rec["exposures_building"].astype(np.int64) + rec["exposures_bus"], "incidence rows summed over the areas vs the records")
    same(sim.area_status_series("incidence", stride=5000)[0], want, "one incidence row for the whole run")
    sim.close()


# ---- 9. errors -------------------------------------------------------------------------------------------------------------------
def test_error_table(world):
    pop, ep, ref = world
    lib = _lib.load()
    rows = np.zeros((4, pop.n_areas), np.uint32)
    pr = rows.ctypes.data_as(u32p)
    fn = lib.esim_area_status_series
    HOME, CUR, INC = _lib.AREA_HOME, _lib.AREA_CURRENT, _lib.AREA_SERIES_INCIDENCE
    bare = C.c_void_p()
    _lib.check(lib.esim_create(C.byref(ep), C.byref(bare)))
    assert fn(bare, HOME, I, 1, 4, 1, pr) == ESTATE                                           # before an upload
    assert fn(bare, HOME, INC, 1, 4, 1, pr) == ESTATE
    lib.esim_destroy(bare)
    assert fn(None, HOME, I, 1, 4, 1, pr) == EINVAL                                           # null context
    sim = Simulator(pop, ep)
    sim.run(10)
    ctx = sim._ctx
    assert fn(ctx, HOME, I, 1, 4, 1, None) == EINVAL                                          # null output
    assert fn(ctx, 3, I, 1, 4, 1, pr) == EINVAL and fn(ctx, -1, I, 1, 4, 1, pr) == EINVAL     # unknown where
    assert fn(ctx, _lib.BY_GROUP, I, 1, 4, 1, pr) == EINVAL                                   # by group: not here
    assert fn(ctx, _lib.BY_GROUP, INC, 1, 4, 1, pr) == EINVAL
    assert fn(ctx, HOME, 6, 1, 4, 1, pr) == EINVAL and fn(ctx, CUR, -1, 1, 4, 1, pr) == EINVAL  # unknown what
    assert fn(ctx, CUR, INC, 1, 4, 1, pr) == EINVAL                                           # incidence by the area stood in
    assert fn(ctx, HOME, I, 1, 4, 0, pr) == EINVAL and fn(ctx, HOME, INC, 1, 4, 0, pr) == EINVAL   # stride 0
    assert fn(ctx, CUR, R, 1, 0, 1, pr) == EINVAL                                             # no rows
    assert fn(ctx, HOME, I, 0, 4, 1, pr) == ERANGE                                            # first_step = 0
    assert fn(ctx, CUR, S, 8, 4, 1, pr) == ERANGE                                             # last row = step 11 of 10
    assert fn(ctx, HOME, INC, 2, 4, 3, pr) == ERANGE
    assert fn(ctx, HOME, V, 11, 1, 1, pr) == ERANGE
    assert fn(ctx, CUR, S, 7, 4, 1, pr) == 0                                                  # last row = step 10: fine
    same(rows, ref["current"][6:10, :, S], "Susceptible rows 7..10 after the refusals")
    assert fn(ctx, HOME, INC, 1, 4, 3, pr) == 0
    same(rows, ref_mod.expected(ref, "home", "incidence", 10, first_step=1, n_rows=4, stride=3), "incidence rows after the refusals")
    with pytest.raises(_lib.EsimError):
        sim.area_status_series("infected", first_step=11)
    with pytest.raises(_lib.EsimError):
        sim.area_status_series("incidence", "current")
    sim.run(90)                                                                               # the context is usable afterwards
    check_all(sim, ref, 100)
    # a sticky device error comes back as the other read-backs report it
    probe = _lib.StepResult()
    _lib.check(lib.esim_debug_inject_error(ctx, ERANGE), ctx)
    want = lib.esim_read_records(ctx, 1, 1, C.byref(probe))
    assert want != 0
    assert lib.esim_area_series(ctx, _lib.SERIES_INFECTED, 1, 4, 1, pr) == want
    assert fn(ctx, HOME, I, 1, 4, 1, pr) == want and fn(ctx, CUR, V, 1, 4, 1, pr) == want and fn(ctx, HOME, INC, 1, 4, 1, pr) == want
    sim.close()



def test_a_context_with_a_communicator_of_two_ranks_describes_its_own_citizens():
    """Rank 0 of two, stepped on its own: the transport leaves the other rank's contribution at zero.  Its incidence rows are
    its own exposure log by household area, before and after a vaccination programme has run; its status rows answer (and end
    in its own census) until a programme has run, and are ESIM_ESTATE from then on."""
    whole = Population.synthetic("york", n_citizens=20000, n_areas=64, citizens_per_school=2500, n_seeds=20)
    cuts = whole.even_cuts(2)
    s0, s1 = whole.shard(cuts, 0), whole.shard(cuts, 1)
    sim = Simulator(s0, _lib.default_params(exposure_chance=0.004, vaccination_threshold=0.003, lockdown_threshold=0.02, seed=123))

    def allreduce(user, which, host_ptr, n_u32):
        if which == 8:                                   # the set-up's layout check: rank 1's row, as its process would add it
            a = (C.c_uint32 * n_u32).from_address(host_ptr)
            a[5:10] = [s0.n_citizens, s1.n_citizens, whole.n_citizens, s1.n_shared_buildings, s1.n_shared_rooms]
        return 0

    cb = _lib.ALLREDUCE_FN(allreduce)
    _lib.check(sim.lib.esim_comm_init_callback(sim._ctx, cb, None, 0, 2), sim._ctx)
    fn, home_area = sim.lib.esim_area_status_series, s0.building_area[s0.home_building]
    out = np.zeros((4, s0.n_areas), np.uint32)

    def check_incidence():
        cit, step, _ = sim.exposure_events()
        keep = step >= 1
        want = np.zeros((sim._steps, s0.n_areas), np.uint32)
        np.add.at(want, (step[keep].astype(np.int64) - 1, home_area[cit[keep]].astype(np.int64)), 1)
        assert want.sum() > 0
        same(sim.area_status_series("incidence"), want, "incidence rows vs the rank's own exposure log, %d steps run" % sim._steps)
        same(sim.area_status_series("incidence", first_step=3, stride=24), np.add.reduceat(want[2:], np.arange(0, sim._steps - 2, 24), axis=0),
             "incidence rows, stride 24, %d steps run" % sim._steps)

    n_done, before, after = C.c_uint32(0), False, False
    for _ in range(12):
        _lib.check(sim.lib.esim_run_sharded(sim._ctx, 50, C.byref(n_done)), sim._ctx)
        assert n_done.value == 50
        sim._steps += 50
        if sim.records_so_far()["vaccination_active"].any():
            after = True
            break
        if not before:                                   # no programme yet: the status rows are this rank's own citizens
            before = True
            for where in ("home", "current"):
                census = sim.area_census(where)
                for k, name in enumerate(STATUS):
                    rows = sim.area_status_series(name, where)
                    same(rows[-1], census[:, k], "a rank's last %s row by %s vs its census" % (name, where))
            same(sum(sim.area_status_series(name, "home").astype(np.int64) for name in STATUS),
                 np.broadcast_to(np.bincount(home_area, minlength=s0.n_areas), (sim._steps, s0.n_areas)), "rows summed over the statuses vs the rank's residents")
            check_incidence()
    assert before and after
    check_incidence()
    for where in (_lib.AREA_HOME, _lib.AREA_CURRENT):
        for what in range(5):
            assert fn(sim._ctx, where, what, 1, 4, 1, out.ctypes.data_as(u32p)) == ESTATE, (where, what)
    assert fn(sim._ctx, _lib.AREA_HOME, _lib.AREA_SERIES_INCIDENCE, 1, 4, 1, out.ctypes.data_as(u32p)) == 0
    check_incidence()                                    # the refusals left the context usable
    sim.close()
