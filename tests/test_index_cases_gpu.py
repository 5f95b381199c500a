"""Ensembles over the index cases: esim_restart_seeded / esim_get_seeds (step 0 under other initially infected citizens),
esim_area_arrival (the step of the first exposure per Output Area or group) and the arrival accumulators of an ensemble.
Every expectation comes from a FRESH CPU oracle on the population with its seeds replaced (the oracle cannot change them in
place), through tests/_arrival_ref.py, or from a fresh context -- never from the code under test."""
import ctypes as C
import json

import numpy as np
import pytest

import _area_ref
import _arrival_ref
import _group_ref
import _oracle
from epidemicsimulator_amd import Ensemble, Population, Simulator, _lib
from test_ensemble_gpu import FORMS, checkpoint_bytes, oracle_for, oracle_x, parity_world
from test_parity_gpu import AGGRESSIVE, assert_same_records, random_population, set_form

pytestmark = pytest.mark.gpu

NEVER = _lib.NEVER
EINVAL, ESTATE, ERANGE = -1, -4, -5
E, I, R = 1 << _lib.EXPOSED, 1 << _lib.INFECTED, 1 << _lib.RECOVERED
u32p = C.POINTER(C.c_uint32)
STATE_KEYS = ("status", "timer", "current_building", "on_bus", "eligible")


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, "%s: shape %s, expected %s" % (what, got.shape, want.shape)
    if not (got == want).all():
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d entries differ, first at %s: got %d, expected %d"
                             % (what, len(bad), bad[0].tolist(), int(got[tuple(bad[0])]), int(want[tuple(bad[0])])))


def with_seeds(pop, seeds):
    """The same world with other initially infected citizens, as a population of its own (what a fresh oracle runs)."""
    kw = {n: getattr(pop, n) for n in ("home_building", "work_building", "room", "flags", "age", "occupation", "building_area",
                                       "building_type", "room_building")}
    return Population(seeds=np.asarray(seeds, np.uint32), n_areas=pop.n_areas, **kw)


def distinct(seeds):
    """First occurrences, in order."""
    return list(dict.fromkeys(int(s) for s in seeds))


def p32(a):
    return a.ctypes.data_as(u32p)


# ---- 1. every member is the run of a fresh oracle on the population that carries its seeds ---------------------------------
def seeded_members():
    """(seed list, overrides, steps) on parity_world(): the uploaded list; one citizen; 65 distinct citizens, one more than the
    one-launch chunk holds; an unsorted list with duplicates; 300 citizens, more than were uploaded (the device list grows);
    nobody.  Philox seed and exposure_chance change along the way; the predecessors stop at steps that are no chunk boundary."""
    pop, base, _ = parity_world()
    rng = np.random.default_rng(2027)
    l65 = rng.permutation(pop.n_citizens)[:65]
    l300 = rng.permutation(pop.n_citizens)[:300]
    ldup = [400, 3, 699, 3, 250, 400, 17, 0, 699, 5]
    return pop, base, [(pop.seeds.tolist(), {}, 500), ([123], {"seed": 99}, 437), (l65.tolist(), {"exposure_chance": 0.02}, 230),
                       (ldup, {"seed": 7}, 410), (l300.tolist(), {"exposure_chance": 0.004, "seed": 3}, 333), ([], {}, 150)]


@pytest.fixture(scope="module")
def seeded_world():
    pop, base, members = seeded_members()
    want = []
    for seeds, overrides, steps in members:
        orc = oracle_for(with_seeds(pop, seeds), base, overrides)        # (the oracle takes a population without seeds, too)
        want.append((orc.run(steps), orc.state()))
        orc.close()
    return pop, base, members, want


def test_the_reference_members_are_not_trivial(seeded_world):
    pop, base, members, want = seeded_world
    assert [len(distinct(m[0])) for m in members] == [8, 1, 65, 7, 300, 0] and len(members[3][0]) == 10
    assert members[3][0] != sorted(members[3][0]) and len(pop.seeds) == 9
    assert any(rec["lockdown"].sum() > 0 and rec["vaccinated"][-1] > 0 for rec, _ in want)
    assert any(steps % 97 and steps % 96 for _, _, steps in members[:-1])
    # nobody infected: everybody stays Susceptible
    rec, state = want[-1]
    assert (rec["susceptible"] == pop.n_citizens).all() and (state["status"] == _lib.SUSCEPTIBLE).all()


@pytest.mark.parametrize("form", FORMS, ids=[str(f) for f in FORMS])
def test_every_seeded_member_is_the_run_of_a_fresh_oracle(seeded_world, form):
    pop, base, members, want = seeded_world
    sim = Simulator(pop, _lib.default_params(**base))
    set_form(sim, form)
    try:
        for (seeds, overrides, steps), (rec, state) in zip(members, want):
            sim.restart(_lib.default_params(**base), seeds=seeds, **overrides)
            same(sim.seeds(), distinct(seeds), "seeds in force")
            assert_same_records(sim.run(steps), rec)
            g = sim.download_state()
            for k in STATE_KEYS:
                assert (g[k] == state[k]).all(), (k, len(seeds), overrides)
    finally:
        sim.close()


# ---- 2. esim_reset and a plain esim_restart go back to the seeds in force --------------------------------------------------
def test_reset_and_plain_restart_keep_the_seeds_in_force(seeded_world):
    pop, base, members, want = seeded_world
    seeds, overrides, steps = members[3]
    rec, state = want[3]
    sim = Simulator(pop, _lib.default_params(**base))
    sim.run(61)
    sim.restart(seeds=seeds, **overrides)
    assert_same_records(sim.run(steps), rec)
    same(sim.seeds(), [400, 3, 699, 250, 17, 0, 5], "first occurrences, in order")
    sim.reset()
    assert_same_records(sim.run(steps), rec)
    sim.restart(**overrides)
    same(sim.seeds(), [400, 3, 699, 250, 17, 0, 5], "after a plain restart")
    assert_same_records(sim.run(steps), rec)
    g = sim.download_state()
    for k in STATE_KEYS:
        assert (g[k] == state[k]).all(), k
    # esim_get_seeds with too little room: the size needed comes back
    n, buf = C.c_uint32(0), np.zeros(3, np.uint32)
    assert sim.lib.esim_get_seeds(sim._ctx, p32(buf), 3, C.byref(n)) == ERANGE and n.value == 7
    # ... and a plain restart under other parameters still starts from them
    other = oracle_for(with_seeds(pop, seeds), base, {"seed": 11, "exposure_chance": 0.02})
    sim.restart(seed=11, exposure_chance=0.02)
    assert_same_records(sim.run(200), other.run(200))
    sim.close()


# ---- 3. checkpoints ---------------------------------------------------------------------------------------------------------
def test_checkpoint_after_a_seeded_restart_belongs_to_the_seeds_in_force(tmp_path):
    pop = Population.synthetic("york", n_citizens=6000, n_areas=20, citizens_per_school=3000, n_seeds=12)
    ep = _lib.default_params(**AGGRESSIVE)
    new = [5000, 17, 2500, 17, 3, 5999, 2500] + list(range(100, 130))
    carried = with_seeds(pop, new)
    want = _oracle.Oracle(carried, _oracle.params_from_esim(ep)).run(450)
    fresh = Simulator(carried, ep)
    fresh.reset()
    at_zero = checkpoint_bytes(fresh, tmp_path / "fresh.bin")
    sim = Simulator(pop, ep)
    sim.run(123)
    sim.restart(seeds=new)
    got = checkpoint_bytes(sim, tmp_path / "seeded.bin")
    assert got.size == at_zero.size and (got == at_zero).all()
    first = sim.run(200)
    path = str(tmp_path / "seeded200.bin")
    sim.save_checkpoint(path)
    # it restores into the context that was uploaded with those seeds and continues bit for bit
    fresh.load_checkpoint(path)
    assert fresh._steps == 200
    assert_same_records(np.concatenate([first, fresh.run(250)]), want)
    fresh.close()
    # a context whose seeds in force differ refuses it and is usable afterwards
    plain = Simulator(pop, ep)
    with pytest.raises(_lib.EsimError, match="another population"):
        plain.load_checkpoint(path)
    same(plain.seeds(), distinct(pop.seeds), "seeds of the refusing context")
    assert_same_records(plain.run(150), _oracle.Oracle(pop, _oracle.params_from_esim(ep)).run(150))
    # ... the same distinct citizens given as another list are another list
    plain.restart(seeds=distinct(new))
    with pytest.raises(_lib.EsimError, match="another population"):
        plain.load_checkpoint(path)
    # ... and it goes in once that context has been restarted to the list
    plain.restart(seeds=new)
    plain.load_checkpoint(path)
    assert_same_records(np.concatenate([first, plain.run(250)]), want)
    plain.close()
    # the uploaded list given again is the uploaded population's hash: the checkpoint at step 0 is the one of a reset
    again = Simulator(pop, ep)
    again.reset()
    zero = checkpoint_bytes(again, tmp_path / "zero.bin")
    sim.restart(seeds=pop.seeds)
    back = checkpoint_bytes(sim, tmp_path / "back.bin")
    assert back.size == zero.size and (back == zero).all()
    again.close()
    sim.close()


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------
def test_refused_seeded_restarts_leave_the_context_as_it_was():
    pop = Population.synthetic("york", n_citizens=6000, n_areas=20, citizens_per_school=3000, n_seeds=12)
    base = dict(max_steps=400, **AGGRESSIVE)
    in_force = [4000, 9, 4000, 77, 1234]
    orc = oracle_for(with_seeds(pop, in_force), base, {})
    want = orc.run(200)
    orc.close()
    sim = Simulator(pop, _lib.default_params(**base))
    lib, ctx = sim.lib, sim._ctx
    sim.restart(seeds=in_force)
    good = _lib.default_params(**base)
    n = pop.n_citizens
    at_n = np.array([5, n, 6], np.uint32)
    three = np.array([1, 2, 3], np.uint32)
    too_many = np.zeros(n + 1, np.uint32)
    refused = [("an index == n_citizens", good, p32(at_n), 3, EINVAL), ("NULL with n_seeds 3", good, None, 3, EINVAL),
               ("n_seeds = n_citizens + 1", good, p32(too_many), n + 1, ERANGE),
               ("bus_capacity 0", _lib.default_params(**dict(base, bus_capacity=0)), p32(three), 3, EINVAL),
               ("exposed + infected time beyond the encoding", _lib.default_params(**dict(base, exposed_time=400, infected_time=200)), p32(three), 3, ERANGE),
               ("max_steps above the context's", _lib.default_params(**dict(base, max_steps=401)), p32(three), 3, ERANGE),
               ("another device", _lib.default_params(**dict(base, device=1)), p32(three), 3, EINVAL)]
    for what, p, seeds, n_seeds, code in refused:
        assert lib.esim_restart_seeded(ctx, C.byref(p), seeds, n_seeds) == code, what
        same(sim.seeds(), distinct(in_force), "seeds after: " + what)
        assert_same_records(sim.run(200), want)
        sim.reset()
    assert lib.esim_restart_seeded(ctx, None, p32(three), 3) == EINVAL
    with pytest.raises(_lib.EsimError):
        sim.restart(seeds=[n])
    with pytest.raises(ValueError):
        sim.restart(seeds=[-1])
    with pytest.raises(ValueError):
        sim.restart(seeds=[[1, 2]])
    # a refusal in the middle of a run: the run goes on from where it stood
    sim.run(50)
    assert lib.esim_restart_seeded(ctx, C.byref(good), p32(at_n), 3) == EINVAL
    assert_same_records(sim.run(150), want[50:])
    sim.close()
    # before the upload
    bare, cnt, buf = C.c_void_p(), C.c_uint32(99), np.zeros(8, np.uint32)
    _lib.check(lib.esim_create(C.byref(good), C.byref(bare)))
    assert lib.esim_get_seeds(bare, p32(buf), 8, C.byref(cnt)) == ESTATE
    assert lib.esim_restart_seeded(bare, C.byref(good), p32(three), 3) == ESTATE
    assert lib.esim_get_seeds(bare, p32(buf), 8, C.byref(cnt)) == ESTATE
    lib.esim_destroy(bare)


def test_seeded_restart_of_a_context_with_a_communicator_of_two_ranks_is_refused():
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
    before = sim.seeds()
    same(before, distinct(s0.seeds), "the shard's seeds")
    three = np.array([1, 2, 3], np.uint32)
    p = _lib.default_params(seed=5)
    assert sim.lib.esim_restart_seeded(sim._ctx, C.byref(p), p32(three), 3) == ESTATE
    same(sim.seeds(), before, "seeds after the refusal")
    sim.close()


# ---- 5. arrival -------------------------------------------------------------------------------------------------------------
ARRIVAL_STOPS = (0, 50, 300, 700)


@pytest.fixture(scope="module")
def world():
    pop, ep, labels, n_groups = _group_ref.fixture_a_groups()
    rec, step, _ = _arrival_ref.oracle_run(pop, ep, _area_ref.FIXTURE_A_STEPS)
    return pop, ep, labels, n_groups, rec, step


def tables(pop, labels, n_groups, step, seeds, upto=None):
    return (_arrival_ref.arrival(_arrival_ref.home_area(pop), pop.n_areas, step, seeds, upto),
            _arrival_ref.arrival(labels, n_groups, step, seeds, upto))


@pytest.mark.parametrize("pipeline", [None, 0], ids=["default", "sequential"])
def test_arrival_follows_the_oracle_and_leaves_the_run_alone(world, pipeline):
    pop, ep, labels, n_groups, rec, step = world
    assert rec["lockdown"].any() and rec["vaccination_active"].any() and pop.n_areas == 64 and n_groups == 8
    home50, _ = tables(pop, labels, n_groups, step, pop.seeds, 50)
    assert (home50 == NEVER).any() and (home50 == 0).any() and ((home50 >= 1) & (home50 <= 50)).any()
    sim = Simulator(pop, ep)
    if pipeline is not None:
        sim.set_pipeline(pipeline)
    sim.set_groups(labels, n_groups)
    done = 0
    for s in ARRIVAL_STOPS:
        if s > done:
            sim.run(s - done)
            done = s
        home, group = tables(pop, labels, n_groups, step, pop.seeds, s)
        got = sim.area_arrival("home")
        assert got.dtype == np.uint32
        same(got, home, "arrival by home area after step %d" % s)
        same(sim.area_arrival("group"), group, "arrival by group after step %d" % s)
    assert_same_records(sim.records_so_far(), rec)
    sim.close()


@pytest.fixture(scope="module")
def finished_run(world):
    pop, ep, labels, n_groups, rec, step = world
    sim = Simulator(pop, ep)
    sim.run(_area_ref.FIXTURE_A_STEPS)
    yield sim
    sim.close()


def test_arrival_with_one_group_and_with_1024(world, finished_run):
    pop, ep, labels, n_groups, rec, step = world
    sim = finished_run
    try:
        sim.set_groups(np.zeros(pop.n_citizens, np.uint16), 1)
        same(sim.area_arrival("group"), [0], "one group")
        many = (np.arange(pop.n_citizens) % 1024).astype(np.uint16)
        want = _arrival_ref.arrival(many, 1024, step, pop.seeds)
        assert (want == NEVER).any() and (want == 0).sum() == len(np.unique(pop.seeds)) and ((want != 0) & (want != NEVER)).sum() > 300
        sim.set_groups(many, 1024)
        same(sim.area_arrival("group"), want, "1024 groups")
        same(sim.area_arrival("home"), _arrival_ref.arrival(_arrival_ref.home_area(pop), pop.n_areas, step, pop.seeds), "by home area in between")
    finally:
        sim.set_groups(None)


def test_arrival_on_a_population_that_is_not_home_sorted(world):
    pop, ep, labels, n_groups, _, _ = world
    perm = _area_ref.permuted(pop)
    assert (np.diff(perm.home_building.astype(np.int64)) < 0).any()
    plabels, _ = perm.age_bands(_group_ref.AGE_EDGES)
    rec, step, _ = _arrival_ref.oracle_run(perm, ep, 300)
    sim = Simulator(perm, ep)
    sim.set_groups(plabels, n_groups)
    assert_same_records(sim.run(300), rec)
    home, group = tables(perm, plabels, n_groups, step, perm.seeds)
    assert ((home != 0) & (home != NEVER)).any()
    same(sim.area_arrival("home"), home, "by home area, permuted citizens")
    same(sim.area_arrival("group"), group, "by group, permuted citizens")
    sim.close()


def test_arrival_in_a_world_of_three_areas_and_on_a_short_log():
    # test_random_populations_all_paths' kind of world on three areas (people work in any area), two index cases in area 1
    world3 = random_population(5, n_areas=3)
    home = _arrival_ref.home_area(world3)
    pop = with_seeds(world3, np.flatnonzero(home == 1)[:2])
    ep = _lib.default_params(**parity_world()[1])
    n = 400
    rec, step, _ = _arrival_ref.oracle_run(pop, ep, n)
    assert pop.n_areas == 3 and (np.bincount(home, minlength=3) > 0).all()
    sim = Simulator(pop, ep)
    same(sim.area_arrival("home"), [NEVER, 0, NEVER], "before step 1")
    # a log of fewer than 64 entries: less than one wavefront of the kernel; one area is still to be reached at the first stop
    entries = lambda s: int(((step >= 1) & (step <= s)).sum()) + 2
    short = next(s for s in range(n, 0, -1) if entries(s) < 64)
    early = short // 2
    assert 2 < entries(early) < entries(short) and (_arrival_ref.arrival(home, 3, step, pop.seeds, early) == NEVER).any()
    done = 0
    for s in (early, short):
        sim.run(s - done)
        done = s
        assert sim.debug_counters()["log_len"] == entries(s) < 64
        same(sim.area_arrival("home"), _arrival_ref.arrival(home, 3, step, pop.seeds, s), "after step %d" % s)
    sim.run(n - short)
    want = _arrival_ref.arrival(home, 3, step, pop.seeds)
    assert (want != NEVER).all() and (want > 0).sum() == 2 and sim.debug_counters()["log_len"] > 64
    same(sim.area_arrival("home"), want, "after step %d" % n)
    assert_same_records(sim.records_so_far(), rec)
    sim.close()


def test_arrival_at_high_prevalence_reaches_every_area(world):
    pop, _, labels, n_groups, _, _ = world
    ep = _lib.default_params(**_group_ref.HIGH_PREVALENCE)
    n = _group_ref.HIGH_PREVALENCE_STEPS
    rec, step, _ = _arrival_ref.oracle_run(pop, ep, n)
    home, group = tables(pop, labels, n_groups, step, pop.seeds)
    populated = np.bincount(_arrival_ref.home_area(pop), minlength=pop.n_areas) > 0         # (three areas have no households)
    assert (home[populated] != NEVER).all() and (home[~populated] == NEVER).all() and (step >= 1).sum() > pop.n_citizens // 2
    sim = Simulator(pop, ep)
    sim.set_groups(labels, n_groups)
    assert_same_records(sim.run(n), rec)
    same(sim.area_arrival("home"), home, "by home area")
    same(sim.area_arrival("group"), group, "by group")
    sim.close()


def test_arrival_after_a_seeded_restart_starts_from_the_new_seeds(world, finished_run):
    pop, ep, labels, n_groups, _, _ = world
    sim = finished_run
    home = _arrival_ref.home_area(pop)
    new = [int(np.flatnonzero(home == 40)[3]), int(np.flatnonzero(home == 10)[0]), int(np.flatnonzero(home == 40)[5])]
    assert not np.isin([10, 40], home[pop.seeds]).any()
    sim.restart(seeds=new, seed=5)
    want = np.full(pop.n_areas, NEVER, np.uint32)
    want[[10, 40]] = 0
    same(sim.area_arrival("home"), want, "at step 0: only the new seeds' areas")
    carried = with_seeds(pop, new)
    rec, step, _ = _arrival_ref.oracle_run(carried, _lib.default_params(**dict({n: getattr(ep, n) for n, _ in _lib.Params._fields_}, seed=5)), 300)
    assert_same_records(sim.run(300), rec)
    full = _arrival_ref.arrival(home, pop.n_areas, step, new)
    assert sorted(np.flatnonzero(full == 0).tolist()) == [10, 40]
    same(sim.area_arrival("home"), full, "after 300 steps from the new seeds")
    sim.restart(ep, seeds=pop.seeds)                            # (the module's run, for whoever comes next)
    sim.run(_area_ref.FIXTURE_A_STEPS)


def test_arrival_on_york_equals_numpy_over_the_downloaded_log():
    pop = Population.synthetic("york")
    sim = Simulator(pop, _lib.default_params(exposure_chance=0.001))
    sim.run(900)
    cit, step, _ = sim.exposure_events()
    assert cit.size > 1000
    home = _arrival_ref.home_area(pop)
    want = np.full(pop.n_areas, NEVER, np.uint32)
    np.minimum.at(want, home[cit], step)
    want[home[sim.seeds()]] = 0
    assert (want == NEVER).any() and ((want != 0) & (want != NEVER)).sum() > 50
    same(sim.area_arrival("home"), want, "york, by home area")
    labels, n_groups = pop.occupation_groups()
    sim.set_groups(labels, n_groups)
    wg = np.full(n_groups, NEVER, np.uint32)
    np.minimum.at(wg, labels[cit], step)
    wg[labels[sim.seeds()]] = 0
    same(sim.area_arrival("group"), wg, "york, by occupation")
    sim.close()


# ---- 6. error table ---------------------------------------------------------------------------------------------------------
def test_arrival_error_table(world):
    pop, ep, labels, n_groups, _, _ = world
    lib = _lib.load()
    out = np.zeros(1024, np.uint32)
    bare = C.c_void_p()
    _lib.check(lib.esim_create(C.byref(ep), C.byref(bare)))
    assert lib.esim_area_arrival(bare, _lib.AREA_HOME, p32(out)) == ESTATE              # before an upload
    assert lib.esim_ensemble_begin_arrival(bare, _lib.AREA_HOME, NEVER) == ESTATE
    assert lib.esim_area_arrival(bare, _lib.AREA_CURRENT, p32(out)) == EINVAL
    lib.esim_destroy(bare)
    sim = Simulator(pop, ep)
    sim.run(10)
    ctx = sim._ctx
    for call in (lambda w: lib.esim_area_arrival(ctx, w, p32(out)), lambda w: lib.esim_ensemble_begin_arrival(ctx, w, 100)):
        assert call(_lib.AREA_CURRENT) == EINVAL                                          # not built
        assert call(7) == EINVAL and call(-1) == EINVAL
        assert call(_lib.BY_GROUP) == ESTATE                                              # no labels
    assert lib.esim_area_arrival(ctx, _lib.AREA_HOME, None) == EINVAL
    assert lib.esim_ensemble_fold(ctx) == ESTATE                                          # no begin yet
    with pytest.raises(_lib.EsimError):
        sim.area_arrival("current")
    assert lib.esim_area_arrival(ctx, _lib.AREA_HOME, p32(out)) == 0
    sim.set_groups(labels, n_groups)
    assert lib.esim_area_arrival(ctx, _lib.BY_GROUP, p32(out)) == 0
    assert lib.esim_ensemble_begin_arrival(ctx, _lib.BY_GROUP, 0) == 0
    sim.set_groups(None)
    assert lib.esim_area_arrival(ctx, _lib.BY_GROUP, p32(out)) == ESTATE
    assert lib.esim_ensemble_fold(ctx) == ESTATE and lib.esim_ensemble_begin_arrival(ctx, _lib.BY_GROUP, 0) == ESTATE
    sim.close()


# ---- 7. arrival accumulators over an ensemble ---------------------------------------------------------------------------------
ENS_STEPS = 400
HORIZONS = (NEVER, 200, 0)


@pytest.fixture(scope="module")
def arrival_ensemble(world):
    pop, ep, labels, n_groups, _, _ = world
    base = {n: getattr(ep, n) for n, _ in _lib.Params._fields_}
    ens = Ensemble(pop, ep, group=(labels, n_groups))
    members = ens.index_cases(6, n=10, first=40)
    home = _arrival_ref.home_area(pop)
    by_home, by_group, states, records = [], [], [], []
    for m in members:
        orc = oracle_for(with_seeds(pop, m["index_cases"]), base, {"seed": m["seed"]})
        orc.set_threads(16)
        records.append(orc.run(ENS_STEPS))
        step, _ = orc.exposures()
        states.append(orc.state())
        orc.close()
        by_home.append(_arrival_ref.arrival(home, pop.n_areas, step, m["index_cases"]))
        by_group.append(_arrival_ref.arrival(labels, n_groups, step, m["index_cases"]))
    yield ens, members, np.array(by_home), np.array(by_group), states, records
    ens.close()


def expected(x, horizon):
    x = x.astype(np.uint64)
    reached = (x != NEVER) & (x <= horizon)
    xr = np.where(reached, x, 0)
    return reached.sum(0), xr.sum(0), (xr * xr).sum(0)


def test_index_case_members_differ_in_place_and_seed(world, arrival_ensemble):
    pop = world[0]
    ens, members, by_home, by_group, states, records = arrival_ensemble
    assert [m["seed"] for m in members] == list(range(40, 46))
    assert all(m["index_cases"] == pop.draw_index_cases(10, m["seed"]).tolist() for m in members)
    assert len({tuple(m["index_cases"]) for m in members}) == 6
    # the input is not trivial: an area reached in some members only, reached by step 200 in fewer, a seed area in some
    hit = expected(by_home, NEVER)[0]
    assert ((hit > 0) & (hit < 6)).any() and (expected(by_home, 200)[0] < hit).any()
    zero = expected(by_home, 0)[0]
    assert ((zero > 0) & (zero < 6)).any() and (by_home == NEVER).any()


@pytest.mark.parametrize("where", ["home", "group"])
def test_arrival_accumulators_equal_numpy_over_the_oracle_members(world, arrival_ensemble, where):
    pop = world[0]
    ens, members, by_home, by_group, states, records = arrival_ensemble
    sim, x = ens.simulator, by_home if where == "home" else by_group
    for horizon in HORIZONS:
        sim.ensemble_begin_arrival(where, None if horizon == NEVER else horizon)
        for k, m in enumerate(members):
            sim.restart(ens.base, seeds=m["index_cases"], seed=m["seed"])
            rec = sim.run(ENS_STEPS)
            if horizon == NEVER:
                assert_same_records(rec, records[k])
            before = sim.area_arrival(where)
            sim.ensemble_fold()
            if k % 2:                                                  # the table is shared with esim_area_arrival: nothing leaks
                same(sim.area_arrival(where), before, "arrival around a fold")
                same(before, x[k], "member %d" % k)
        sim.reset()                                                    # (the accumulators survive)
        got = sim.ensemble_read()
        hit, total, sq = expected(x, horizon)
        assert got["members"] == 6 and got["hit"].shape == (x.shape[1],)
        same(got["hit"], hit, "hit, horizon %d" % horizon)
        same(got["sum"], total, "sum, horizon %d" % horizon)
        same(got["sumsq"], sq, "sumsq, horizon %d" % horizon)


def test_set_groups_invalidates_the_group_kind_only_and_a_risk_map_follows(world, arrival_ensemble):
    pop, ep, labels, n_groups, _, _ = world
    ens, members, by_home, by_group, states, records = arrival_ensemble
    sim = ens.simulator
    sim.ensemble_begin_arrival("group", 200)
    sim.set_groups(labels, n_groups)
    assert sim.lib.esim_ensemble_fold(sim._ctx) == ESTATE and sim.lib.esim_ensemble_read(sim._ctx, None, None, None, None) == ESTATE
    sim.ensemble_begin_arrival("home", 200)
    sim.set_groups(labels, n_groups)
    sim.ensemble_fold()
    assert sim.ensemble_read()["members"] == 1
    # accumulators begun with esim_ensemble_begin afterwards, on the same context: the risk map of these members
    x = np.array([oracle_x(pop, st, "home", E | I | R) for st in states])
    sim.ensemble_begin("home", E | I | R, 1)
    for m in members:
        sim.restart(ens.base, seeds=m["index_cases"], seed=m["seed"])
        sim.run(ENS_STEPS)
        sim.ensemble_fold()
    got = sim.ensemble_read()
    assert got["members"] == 6
    same(got["hit"], (x >= 1).sum(0), "risk map hit")
    same(got["sum"], x.sum(0), "risk map sum")
    same(got["sumsq"], (x * x).sum(0), "risk map sumsq")


def test_ensemble_run_with_index_cases_and_an_arrival_summary(world, arrival_ensemble, tmp_path):
    pop = world[0]
    ens, members, by_home, by_group, states, records = arrival_ensemble
    res = ens.run(members, ENS_STEPS, area=dict(kind="arrival", where="home", horizon=200))
    assert res.members == members and res.n_done.tolist() == [ENS_STEPS] * 6
    for k, r in enumerate(records):
        assert_same_records(res.records[k], r)
    hit, total, sq = expected(by_home, 200)
    assert res.area["members"] == 6
    same(res.area["hit"], hit, "Ensemble hit")
    some, none = hit > 0, hit == 0
    assert some.any() and none.any()
    x = np.where((by_home != NEVER) & (by_home <= 200), by_home.astype(np.float64), np.nan)
    with np.errstate(all="ignore"):
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            mean, var = np.nanmean(x, axis=0), np.nanvar(x, axis=0)
    assert np.isnan(res.area["mean"][none]).all() and np.isnan(res.area["var"][none]).all()
    assert np.allclose(res.area["mean"][some], mean[some], rtol=1e-12, atol=0)
    assert np.allclose(res.area["var"][some], var[some], rtol=1e-9, atol=1e-6)
    out = str(tmp_path / "ens")
    res.dump(out)
    doc = json.load(open(out + "/ensemble_areas.json"))
    stats = json.load(open(out + "/ensemble_stats.json"))
    assert stats["members"] == members and doc["members"] == 6 and sorted(doc["areas"], key=int) == [str(a) for a in range(pop.n_areas)]
    for a in range(pop.n_areas):
        entry = doc["areas"][str(a)]
        assert entry["hit"] == int(hit[a])
        if hit[a]:
            assert entry["mean"] == float(res.area["mean"][a]) and entry["var"] == float(res.area["var"][a])
        else:
            assert entry["mean"] is None and entry["var"] is None
    # a member without index cases, after members with them, starts from the population's own seeds; by group, no horizon
    res = ens.run([members[0], {"seed": 123}], ENS_STEPS, area=dict(kind="arrival", where="group"))
    base = {n: getattr(ens.base, n) for n, _ in _lib.Params._fields_}
    orc = oracle_for(pop, base, {"seed": 123})
    assert_same_records(res.records[1], orc.run(ENS_STEPS))
    step, _ = orc.exposures()
    orc.close()
    own = _arrival_ref.arrival(world[2], world[3], step, pop.seeds)
    hit, total, sq = expected(np.array([by_group[0], own]), NEVER)
    same(res.area["hit"], hit, "Ensemble hit by group")
    assert res.area_codes is None and np.allclose(res.area["mean"][hit > 0], (total / np.maximum(hit, 1))[hit > 0], rtol=1e-12, atol=0)
    with pytest.raises(ValueError):
        ens.run(members[:1], 5, area=dict(kind="census-by-arrival", where="home"))
