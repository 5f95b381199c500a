"""esim_set_groups / esim_group_census / esim_group_series / ensembles by group against tables computed with numpy from the CPU
oracle (tests/_group_ref.py).  Every comparison is exact equality of integer arrays."""
import ctypes as C

import numpy as np
import pytest

import _area_ref
import _group_ref
import _oracle
from epidemicsimulator_amd import Ensemble, Population, Simulator, _lib

pytestmark = pytest.mark.gpu

FIELDS = [f for f in _lib.RECORD_FIELDS if f != "reserved"]
N_STEPS = _area_ref.FIXTURE_A_STEPS
STOPS = (1, 96, 300, 700)
S, E, I, R, V = range(5)
STATUS = ("susceptible", "exposed", "infected", "recovered", "vaccinated")
EINVAL, ESTATE, ERANGE = -1, -4, -5
u16p, u32p = C.POINTER(C.c_uint16), C.POINTER(C.c_uint32)


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, "%s: shape %s, expected %s" % (what, got.shape, want.shape)
    if not (got == want).all():
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d entries differ, first at %s: got %d, expected %d"
                             % (what, len(bad), bad[0].tolist(), int(got[tuple(bad[0])]), int(want[tuple(bad[0])])))


@pytest.fixture(scope="module")
def world():
    pop, ep, labels, n_groups = _group_ref.fixture_a_groups()
    return pop, ep, labels, n_groups, _group_ref.reference_tables(pop, ep, labels, n_groups, N_STEPS)


@pytest.mark.parametrize("pipeline", [None, 0], ids=["default", "sequential"])
def test_census_follows_the_oracle_and_the_calls_leave_the_run_alone(world, pipeline):
    pop, ep, labels, n_groups, ref = world
    sim = Simulator(pop, ep)
    if pipeline is not None:
        sim.set_pipeline(pipeline)
    sim.set_groups(labels, n_groups)
    same(sim.group_census(), ref["initial"], "census before step 1")
    done = 0
    for s in STOPS:
        sim.run(s - done)
        done = s
        got = sim.group_census()
        assert got.dtype == np.uint32 and got.shape == (n_groups, 5)
        same(got, ref["status_rows"][s - 1], "census after step %d" % s)
        same(got.sum(axis=0), sim.area_census("home").sum(axis=0), "census by group vs by area, summed, after step %d" % s)
        for k, name in enumerate(STATUS):
            same(sim.group_series(name), ref["status_rows"][:s, :, k], "%s rows 1..%d" % (name, s))
        same(sim.group_series("exposures"), ref["exposure_rows"][:s], "exposure rows 1..%d" % s)
    got = sim.records_so_far()
    for f in FIELDS:
        same(got[f], ref["records"][f], "record field %s" % f)
    state = sim.download_state()
    for k in ("status", "timer", "current_building", "on_bus", "eligible"):
        same(state[k], ref["final_state"][k], "final state %s" % k)
    sim.reset()
    same(sim.group_census(), ref["initial"], "census after reset")
    sim.close()


@pytest.fixture(scope="module")
def finished_run(world):
    pop, ep, labels, n_groups, ref = world
    sim = Simulator(pop, ep)
    sim.run(N_STEPS)
    sim.set_groups(labels, n_groups)           # (labels set after the run: the series are derived after the fact)
    yield sim
    sim.close()


def test_series_all_kinds_rows_strides_and_windows(world, finished_run):
    pop, ep, labels, n_groups, ref = world
    sim = finished_run
    rec = ref["records"]
    inside = int(np.argmax(rec["vaccination_active"])) + 3            # a first step inside the programme
    assert rec["vaccination_active"][inside - 1] and rec["vaccinated_now"][inside - 1] > 0
    census = sim.group_census()
    for k, name in enumerate(STATUS):
        full = sim.group_series(k, first_step=1, n_rows=N_STEPS, stride=1)
        assert full.dtype == np.uint32
        same(full, ref["status_rows"][:, :, k], "%s rows 1..700" % name)
        for stride in (7, 24):
            same(sim.group_series(name, first_step=inside, stride=stride), full[inside - 1::stride], "%s rows from %d, stride %d" % (name, inside, stride))
            same(sim.group_series(name, first_step=inside, n_rows=3, stride=stride), full[inside - 1::stride][:3], "%s, three rows, stride %d" % (name, stride))
        same(sim.group_series(name, first_step=N_STEPS - 99, n_rows=100), full[-100:], "%s, the window that ends at the last step" % name)
        same(full[-1], census[:, k], "last %s row vs the census" % name)
    full = sim.group_series("exposures")
    same(full, ref["exposure_rows"], "exposure rows 1..700")
    assert int(full.sum()) == 799 + 11                                  # buildings and public transport
    for stride in (7, 24):
        want = np.add.reduceat(full[inside - 1:], np.arange(0, N_STEPS - inside + 1, stride), axis=0)
        same(sim.group_series(_lib.GROUP_SERIES_EXPOSURES, first_step=inside, stride=stride), want, "exposure rows from %d, stride %d" % (inside, stride))
    same(sim.group_series("exposures", first_step=N_STEPS - 99, n_rows=100), full[-100:], "exposure rows, the window that ends at the last step")


def test_label_edge_cases(world, finished_run):
    pop, ep, labels, n_groups, ref = world
    sim = finished_run
    rows = ref["status_rows"]
    try:
        # one group: the rows are the after-step census of the whole population
        sim.set_groups(np.zeros(pop.n_citizens, np.uint16), 1)
        same(sim.group_census(), rows[-1].sum(axis=0)[None, :], "census, one group")
        for k, name in enumerate(STATUS):
            same(sim.group_series(name), rows[:, :, k].sum(axis=1)[:, None], "%s rows, one group" % name)
        same(sim.group_series("exposures")[:, 0], ref["records"]["exposures_building"] + ref["records"]["exposures_bus"], "exposure rows, one group")
        # 1024 groups, every one of them in use: the LDS table is full
        many = (np.arange(pop.n_citizens) % 1024).astype(np.uint16)
        final = ref["final_state"]["status"]
        sim.set_groups(many, 1024)
        same(sim.group_census(), _group_ref.census_table(many, 1024, final), "census, 1024 groups")
        same(sim.group_series("infected")[-1], _group_ref.census_table(many, 1024, final)[:, I], "last Infected row, 1024 groups")
        same(sim.group_series("vaccinated", stride=50).sum(axis=1), rows[::50, :, V].sum(axis=1), "Vaccinated rows, 1024 groups, summed")
        # an all-but-empty group: one citizen in group 1, nobody in group 2
        lone = np.zeros(pop.n_citizens, np.uint16)
        lone[pop.n_citizens - 1] = 1
        sim.set_groups(lone, 3)
        got = sim.group_census()
        same(got, _group_ref.census_table(lone, 3, final), "census, an all-but-empty group")
        assert int(got[1].sum()) == 1 and int(got[2].sum()) == 0
        same(sim.group_series("susceptible", stride=100).sum(axis=1), rows[::100, :, S].sum(axis=1), "Susceptible rows, an all-but-empty group")
    finally:
        sim.set_groups(labels, n_groups)


def test_population_that_is_not_home_sorted(world):
    """The citizens permuted, their labels with them: the same world, so the same tables as the oracle run on it gives --
    and, group by group, the same sizes as before."""
    pop, ep, labels, n_groups, _ = world
    per = _area_ref.permuted(pop)
    plab, png = per.age_bands(_group_ref.AGE_EDGES)
    assert png == n_groups and (np.bincount(plab, minlength=png) == np.bincount(labels, minlength=n_groups)).all()
    ref = _group_ref.reference_tables(per, ep, plab, png, 400)
    sim = Simulator(per, ep)
    sim.set_groups(plab, png)
    got = sim.run(400)
    for f in FIELDS:
        same(got[f], ref["records"][f], "record field %s" % f)
    same(sim.group_census(), ref["status_rows"][-1], "census")
    for k, name in enumerate(STATUS):
        same(sim.group_series(name), ref["status_rows"][:, :, k], "%s rows" % name)
    same(sim.group_series("exposures"), ref["exposure_rows"], "exposure rows")
    sim.close()


@pytest.mark.parametrize("pipeline", [None, 0], ids=["default", "sequential"])
def test_high_prevalence(pipeline):
    """Most of the population leaves Susceptible (tests/test_groups.py pins the regime): the non-Susceptible path of the census
    is the common one, and Exposed, Infected and Recovered citizens are among the vaccinated."""
    pop, _, labels, n_groups = _group_ref.fixture_a_groups()
    ep = _lib.default_params(**_group_ref.HIGH_PREVALENCE)
    n = _group_ref.HIGH_PREVALENCE_STEPS
    ref = _group_ref.reference_tables(pop, ep, labels, n_groups, n)
    sim = Simulator(pop, ep)
    if pipeline is not None:
        sim.set_pipeline(pipeline)
    sim.set_groups(labels, n_groups)
    done = 0
    for s in (250, 400, n):
        got = sim.run(s - done)
        done = s
        same(sim.group_census(), ref["status_rows"][s - 1], "census after step %d" % s)
    got = sim.records_so_far()
    for f in FIELDS:
        same(got[f], ref["records"][f], "record field %s" % f)
    for k, name in enumerate(STATUS):
        same(sim.group_series(name), ref["status_rows"][:, :, k], "%s rows" % name)
    same(sim.group_series("exposures"), ref["exposure_rows"], "exposure rows")
    sim.close()


def test_ensembles_by_group_and_area_accumulators_afterwards(world):
    pop, ep, labels, n_groups, _ = world
    base = {n: getattr(ep, n) for n, _ in _lib.Params._fields_}
    members, steps = [{"seed": 500 + k} for k in range(3)], 250
    mask = (1 << E) | (1 << I) | (1 << R)
    states = []
    for m in members:
        orc = _oracle.Oracle(pop, _oracle.params_from_esim(_lib.default_params(**dict(base, **m))))
        orc.run(steps)
        states.append(orc.state())
        orc.close()
    sel = [((1 << st["status"].astype(np.uint32)) & mask) != 0 for st in states]
    x = np.array([np.bincount(labels[s], minlength=n_groups) for s in sel]).astype(np.uint64)
    assert len({tuple(r) for r in x.tolist()}) == 3                       # the members differ
    min_cases = int(np.median(x))
    assert ((x >= min_cases).sum(0) > 0).any() and ((x >= min_cases).sum(0) < 3).any()
    sim = Simulator(pop, ep)
    assert sim.lib.esim_ensemble_begin(sim._ctx, _lib.BY_GROUP, mask, 1) == ESTATE      # no labels yet
    assert sim.lib.esim_ensemble_begin(sim._ctx, 7, mask, 1) == EINVAL
    sim.set_groups(labels, n_groups)
    sim.ensemble_begin("group", mask, min_cases)
    for m in members:
        sim.restart(**m)
        sim.run(steps)
        before = sim.group_census()
        sim.ensemble_fold()
        same(sim.group_census(), before, "census around a fold")
    sim.reset()                                                             # (the accumulators survive)
    got = sim.ensemble_read()
    assert got["members"] == 3 and got["hit"].shape == (n_groups,)
    same(got["hit"], (x >= min_cases).sum(0), "hit")
    same(got["sum"], x.sum(0), "sum")
    same(got["sumsq"], (x * x).sum(0), "sumsq")
    # area-mode accumulators begun afterwards on the same context
    home_area = pop.building_area[pop.home_building]
    xa = np.array([np.bincount(home_area[s], minlength=pop.n_areas) for s in sel]).astype(np.uint64)
    sim.ensemble_begin("home", mask, 1)
    for m in members:
        sim.restart(**m)
        sim.run(steps)
        sim.ensemble_fold()
    got = sim.ensemble_read()
    assert got["members"] == 3 and got["hit"].shape == (pop.n_areas,)
    same(got["hit"], (xa >= 1).sum(0), "hit by home area")
    same(got["sum"], xa.sum(0), "sum by home area")
    same(got["sumsq"], (xa * xa).sum(0), "sumsq by home area")
    sim.close()
    # the Python Ensemble, by group
    ens = Ensemble(pop, ep, group=(labels, n_groups))
    res = ens.run(members, steps, area=dict(where="group", status_mask=mask, min_cases=min_cases))
    assert res.area["members"] == 3
    same(res.area["hit"], (x >= min_cases).sum(0), "Ensemble hit")
    assert np.allclose(res.area["mean"], x.astype(np.float64).mean(0), rtol=1e-12, atol=0)
    ens.close()


def test_lifetime_of_the_labels(world, tmp_path):
    pop, ep, labels, n_groups, ref = world
    mask = 1 << I
    a = Simulator(pop, ep)
    a.set_groups(labels, n_groups)
    a.run(300)
    path = str(tmp_path / "step300.ckpt")
    a.save_checkpoint(path)
    same(a.group_census(), ref["status_rows"][299], "census at step 300")
    a.run(50)
    a.load_checkpoint(path)                                                 # labels survive a checkpoint restore
    same(a.group_census(), ref["status_rows"][299], "census after load_checkpoint")
    same(a.group_series("infected"), ref["status_rows"][:300, :, I], "Infected rows after load_checkpoint")
    a.restart()                                                             # ... a restart
    same(a.group_census(), ref["initial"], "census after restart")
    a.run(96)
    same(a.group_census(), ref["status_rows"][95], "census at step 96 after restart")
    a.reset()                                                               # ... and a reset
    same(a.group_census(), ref["initial"], "census after reset")
    # set_groups again invalidates accumulators begun by group, and only those
    a.ensemble_begin("group", mask, 1)
    a.ensemble_fold()
    a.set_groups(labels, n_groups)
    assert a.lib.esim_ensemble_fold(a._ctx) == ESTATE
    assert a.lib.esim_ensemble_read(a._ctx, None, None, None, None) == ESTATE
    a.ensemble_begin("group", mask, 1)
    a.ensemble_fold()
    assert a.ensemble_read()["members"] == 1
    a.ensemble_begin("home", mask, 1)
    a.set_groups(labels, n_groups)
    a.ensemble_fold()
    assert a.ensemble_read()["members"] == 1
    # a second upload drops the labels
    ps = pop.as_struct()
    _lib.check(a.lib.esim_upload_population(a._ctx, C.byref(ps)), a._ctx)
    out = np.zeros((n_groups, 5), np.uint32)
    assert a.lib.esim_group_census(a._ctx, out.ctypes.data_as(u32p)) == ESTATE
    assert a.lib.esim_group_series(a._ctx, I, 1, 1, 1, out.ctypes.data_as(u32p)) == ESTATE
    assert a.lib.esim_ensemble_begin(a._ctx, _lib.BY_GROUP, mask, 1) == ESTATE
    a.close()


def test_error_table(world):
    pop, ep, labels, n_groups, ref = world
    lib = _lib.load()
    census = np.zeros((1024, 5), np.uint32)
    rows = np.zeros((4, 1024), np.uint32)
    pc, pr = census.ctypes.data_as(u32p), rows.ctypes.data_as(u32p)
    lab = np.ascontiguousarray(labels, np.uint16)
    pl = lab.ctypes.data_as(u16p)
    bare = C.c_void_p()
    _lib.check(lib.esim_create(C.byref(ep), C.byref(bare)))
    assert lib.esim_set_groups(bare, pl, n_groups) == ESTATE                                  # before an upload
    assert lib.esim_group_census(bare, pc) == ESTATE
    assert lib.esim_ensemble_begin(bare, _lib.BY_GROUP, 1 << I, 1) == ESTATE
    lib.esim_destroy(bare)
    assert lib.esim_set_groups(None, pl, n_groups) == EINVAL and lib.esim_group_census(None, pc) == EINVAL
    sim = Simulator(pop, ep)
    sim.run(10)
    ctx = sim._ctx
    assert lib.esim_group_census(ctx, pc) == ESTATE                                           # no labels yet
    assert lib.esim_group_series(ctx, I, 1, 4, 1, pr) == ESTATE
    assert lib.esim_set_groups(ctx, pl, 0) == EINVAL                                          # n_groups 0 or 1025
    assert lib.esim_set_groups(ctx, pl, 1025) == EINVAL
    assert lib.esim_group_census(ctx, pc) == ESTATE
    sim.set_groups(labels, n_groups)
    want = sim.group_census()
    same(want, ref["status_rows"][9], "census at step 10")
    bad = lab.copy()
    bad[-1] = n_groups                                                                        # a label out of range ...
    assert lib.esim_set_groups(ctx, bad.ctypes.data_as(u16p), n_groups) == EINVAL
    same(sim.group_census(), want, "the previous labels still answer")                        # ... leaves the context as it was
    assert lib.esim_set_groups(ctx, pl, n_groups - 1) == EINVAL
    same(sim.group_census(), want, "the previous labels still answer")
    assert lib.esim_group_census(ctx, None) == EINVAL
    assert lib.esim_group_series(ctx, I, 1, 4, 1, None) == EINVAL
    assert lib.esim_group_series(ctx, 6, 1, 4, 1, pr) == EINVAL                               # what = 6
    assert lib.esim_group_series(ctx, -1, 1, 4, 1, pr) == EINVAL
    assert lib.esim_group_series(ctx, I, 1, 4, 0, pr) == EINVAL                               # stride 0, no rows
    assert lib.esim_group_series(ctx, I, 1, 0, 1, pr) == EINVAL
    assert lib.esim_group_series(ctx, I, 0, 4, 1, pr) == ERANGE                               # first_step = 0
    assert lib.esim_group_series(ctx, I, 8, 4, 1, pr) == ERANGE                               # last row = step 11 of 10
    assert lib.esim_group_series(ctx, _lib.GROUP_SERIES_EXPOSURES, 2, 4, 3, pr) == ERANGE
    assert lib.esim_group_series(ctx, I, 7, 4, 1, pr) == 0                                    # last row = step 10: fine
    assert lib.esim_group_series(ctx, _lib.GROUP_SERIES_EXPOSURES, 1, 4, 3, pr) == 0
    with pytest.raises(_lib.EsimError):
        sim.group_series("infected", first_step=11)
    assert lib.esim_ensemble_begin(ctx, 7, 1 << I, 1) == EINVAL                               # where = 7 still EINVAL
    assert lib.esim_ensemble_begin(ctx, _lib.BY_GROUP, 0, 1) == EINVAL
    assert lib.esim_ensemble_begin(ctx, _lib.BY_GROUP, 1 << I, 1) == 0
    assert lib.esim_set_groups(ctx, None, 0) == 0                                             # NULL labels, then census
    assert lib.esim_group_census(ctx, pc) == ESTATE
    assert lib.esim_ensemble_fold(ctx) == ESTATE
    assert lib.esim_ensemble_begin(ctx, _lib.BY_GROUP, 1 << I, 1) == ESTATE
    sim.close()


def test_a_context_with_a_communicator_of_two_ranks_refuses_labels():
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
    lab = np.zeros(s0.n_citizens, np.uint16)
    assert sim.lib.esim_set_groups(sim._ctx, lab.ctypes.data_as(u16p), 1) == ESTATE
    sim.close()


def test_full_size_self_consistency():
    """uk64m, default parameters, 5000 steps, 19 five-year age bands; no oracle run at that size."""
    pop = Population.synthetic("uk64m")
    labels, n_groups = pop.age_bands(np.arange(5, 95, 5))
    assert n_groups == 19
    sizes = np.bincount(labels, minlength=n_groups)
    sim = Simulator(pop, _lib.default_params())
    sim.set_groups(labels, n_groups)
    rec = sim.run(5000)
    assert len(rec) == 5000
    census = sim.group_census()
    same(census.sum(axis=1), sizes, "group sizes")
    same(census.sum(axis=0), sim.area_census("home").sum(axis=0, dtype=np.uint32), "census by group vs by home area, per status")
    status = sim.download_state()["status"]
    same(census, np.bincount(labels.astype(np.int64) * 5 + status, minlength=n_groups * 5).reshape(n_groups, 5), "census vs download_state")
    del status
    total = np.zeros((50, n_groups), np.int64)
    for k, name in enumerate(STATUS):
        rows = sim.group_series(name, first_step=100, stride=100)
        assert rows.shape == (50, n_groups)
        same(rows[-1], census[:, k], "last %s row vs the census" % name)
        total += rows
    same(total, np.broadcast_to(sizes, total.shape), "rows summed over the statuses vs the group sizes")
    exp = sim.group_series("exposures")
    same(exp.sum(axis=1, dtype=np.int64), rec["exposures_building"].astype(np.int64) + rec["exposures_bus"], "exposure rows summed over the groups vs the records")
    sim.close()
