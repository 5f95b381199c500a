"""esim_curve_summary and the peaks kind of the ensemble accumulators against tests/_curve_ref.py: numpy over the status rows the
CPU oracle gives, by all, by home area and by age band.  Every comparison is exact equality of whole integer arrays."""
import ctypes as C

import numpy as np
import pytest

import _area_ref
import _area_status_ref
import _curve_ref as ref_mod
import _group_ref
import _oracle
from epidemicsimulator_amd import Ensemble, Population, Simulator, _lib
from epidemicsimulator_amd.ensemble import PEAKS_ARRAYS, peaks_summary

pytestmark = pytest.mark.gpu

FIELDS = [f for f in _lib.RECORD_FIELDS if f != "reserved"]
N_STEPS = _area_ref.FIXTURE_A_STEPS
STOPS = (1, 96, 300, 700)
WHERES = ("all", "home", "group")
STATUS, KEYS, NEVER = ref_mod.STATUS, ref_mod.KEYS, ref_mod.NEVER
EINVAL, ESTATE, ERANGE = -1, -4, -5
MASK = {"exposed": 1 << _lib.EXPOSED, "infected": 1 << _lib.INFECTED, "active": (1 << _lib.EXPOSED) | (1 << _lib.INFECTED)}
u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, "%s: %s %s, expected %s %s" % (what, got.dtype, got.shape, want.dtype, want.shape)
    if not (got == want).all():
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d entries differ, first at %s: got %d, expected %d"
                             % (what, len(bad), bad[0].tolist(), int(got[tuple(bad[0])]), int(want[tuple(bad[0])])))


def same_summary(got, want, what):
    assert sorted(got) == sorted(KEYS), what
    for k in KEYS:
        same(got[k], want[k], "%s: %s" % (what, k))


def check(sim, tables, where, status, note="", **window):
    """One curve_summary call against the reference tables of `where` (which cover at least the steps run)."""
    first, last, threshold = window.get("first_step", 1), window.get("last_step"), window.get("threshold", 1)
    want = ref_mod.summarize(ref_mod.curves(tables[where]["status_rows"], status), first, sim._steps if last is None else last, threshold)
    same_summary(sim.curve_summary(where, status, **window), want, "%s by %s, %d steps run, %s %s" % (status, where, sim._steps, window, note))
    return want


def check_records(sim, records):
    got = sim.records_so_far()
    for f in FIELDS:
        same(got[f], records[f][:len(got)], "record field %s" % f)


def from_rows(sim, where, status, first_step, last_step, threshold):
    """The summary from the library's own stride-1 rows, reduced with numpy."""
    def rows(what):
        if where == "group":
            return sim.group_series(what, first_step=first_step, n_rows=last_step - first_step + 1)
        return sim.area_status_series(what, "home", first_step=first_step, n_rows=last_step - first_step + 1)
    x = sum(rows(what).astype(np.int64) for what in (("exposed", "infected") if status == "active" else (status,)))
    if where == "all":
        x = x.sum(axis=1, keepdims=True)
    got = ref_mod.summarize(x, 1, x.shape[0], threshold)
    for k in ("peak_step", "first_at_least", "last_at_least"):                   # (rows count from first_step)
        got[k] = np.where(got[k] != NEVER, got[k].astype(np.int64) + first_step - 1, NEVER).astype(np.uint32)
    return got


def vaccinated_while_active(pop, ep, n_steps):
    """{"exposed": k, "infected": k}: the citizens whose status is Exposed / Infected after some step and Vaccinated after the
    next one, from the CPU oracle stepped one step at a time."""
    orc = _oracle.Oracle(pop, _oracle.params_from_esim(ep))
    before, out = orc.state()["status"].copy(), {"exposed": 0, "infected": 0}
    for _ in range(n_steps):
        orc.step()
        after = orc.state()["status"]
        now = after == _lib.VACCINATED
        out["exposed"] += int((now & (before == _lib.EXPOSED)).sum())
        out["infected"] += int((now & (before == _lib.INFECTED)).sum())
        before = after.copy()
    orc.close()
    return out


@pytest.fixture(scope="module")
def world():
    return ref_mod.fixture_a_rows()


@pytest.fixture(scope="module")
def finished_run(world):
    pop, ep, labels, n_groups, _ = world
    sim = Simulator(pop, ep)
    sim.set_groups(labels, n_groups)
    sim.run(N_STEPS)
    yield sim
    sim.close()


# ---- a, g. all three masks by all three kinds of column at every stop; the calls leave the run alone ------------------------------
def test_every_mask_and_column_at_every_stop_and_the_calls_leave_the_run_alone(world):
    pop, ep, labels, n_groups, tables = world
    sim = Simulator(pop, ep)
    sim.set_groups(labels, n_groups)
    done = 0
    for s in STOPS:
        sim.run(s - done)
        done = s
        for where in WHERES:
            for status in STATUS:
                check(sim, tables, where, status)
    check_records(sim, tables["home"]["records"])
    state = sim.download_state()
    for k in ("status", "timer", "current_building", "on_bus", "eligible"):
        same(state[k], tables["home"]["final_state"][k], "final state %s" % k)
    sim.close()


# ---- b. windows and thresholds on the finished run --------------------------------------------------------------------------------
def test_windows_and_thresholds(world, finished_run):
    pop, ep, labels, n_groups, tables = world
    sim = finished_run
    home = tables["home"]["status_rows"]
    whole = ref_mod.summarize(ref_mod.curves(home, "infected"))
    assert (whole["peak"] >= 2).sum() * 2 >= pop.n_areas                          # at least half of the areas have a peak of 2 or more
    mid = int(np.argmax(tables["home"]["records"]["infected"])) + 1               # the step of the national peak: intervals begun earlier are clipped
    assert 100 < mid < N_STEPS - 100 and ref_mod.curves(home, "active")[mid - 2].sum() > 100
    late = ref_mod.summarize(ref_mod.curves(home, "infected"), mid, N_STEPS)
    assert (late["peak"] == 0).any() and (late["peak"] > 0).any()                 # a column without a case in the window
    # the cut at the vaccinating step is exercised: citizens Exposed or Infected after one step and Vaccinated after the next,
    # counted from the oracle's state after every step
    cut = vaccinated_while_active(pop, ep, N_STEPS)
    assert cut["exposed"] + cut["infected"] > 0, cut                              # (fixture A: 99 while Exposed, none while Infected)
    # ... which shows in the curves: nothing but a vaccination ends an Exposed interval early (it lasts exposed_time + 1 steps, or
    # to the end of the run), so the Exposed person-steps fall short of that many per exposure
    exposures = tables["group"]["exposure_rows"].sum(axis=1).astype(np.int64)
    uncut = sum(int(exposures[s - 1]) * min(ep.exposed_time + 1, N_STEPS - s + 1) for s in range(1, N_STEPS + 1))
    assert 0 < int(ref_mod.curves(tables["all"]["status_rows"], "exposed").sum()) < uncut
    above = int(max(ref_mod.curves(tables[w]["status_rows"], "active").max() for w in WHERES)) + 1
    windows = (dict(first_step=mid), dict(first_step=mid, last_step=mid), dict(last_step=500), dict(first_step=250, last_step=600),
               dict(first_step=N_STEPS, last_step=N_STEPS), dict(first_step=1, last_step=1))
    for where in WHERES:
        for status in STATUS:
            for window in windows:
                for threshold in (1, 5, above):
                    want = check(sim, tables, where, status, threshold=threshold, **window)
                    if threshold == above:
                        assert not want["steps_at_least"].any() and (want["first_at_least"] == NEVER).all() and (want["last_at_least"] == NEVER).all()
    assert check(sim, tables, "home", "infected", threshold=5)["steps_at_least"].any()


# ---- c. against the library's own rows --------------------------------------------------------------------------------------------
def test_against_the_series_of_the_library(finished_run):
    sim = finished_run
    for where in WHERES:
        for status in STATUS:
            for first, last, threshold in ((1, N_STEPS, 1), (300, 650, 3)):
                same_summary(sim.curve_summary(where, status, first, last, threshold), from_rows(sim, where, status, first, last, threshold),
                             "%s by %s, steps %d..%d, threshold %d vs the stride-1 rows" % (status, where, first, last, threshold))


# ---- d. three areas, most citizens become cases -----------------------------------------------------------------------------------
def test_three_areas_in_which_most_citizens_become_cases():
    pop = Population.synthetic("york", n_citizens=500, n_areas=3, citizens_per_school=500, n_seeds=5)
    ep = _lib.default_params(**_group_ref.HIGH_PREVALENCE)
    n = _group_ref.HIGH_PREVALENCE_STEPS
    home = ref_mod.reference_rows(pop, ep, n, "home")
    tables = {"home": home, "all": {"status_rows": home["status_rows"].sum(axis=1, keepdims=True)}}
    assert int(home["exposure_rows"].sum()) + len(np.unique(pop.seeds)) > pop.n_citizens // 2 and home["records"]["vaccination_active"].any()
    sim = Simulator(pop, ep)
    sim.run(n)
    check_records(sim, home["records"])
    for where in ("all", "home"):
        for status in STATUS:
            check(sim, tables, where, status, "three areas")
            check(sim, tables, where, status, "three areas", first_step=200, last_step=400, threshold=50)
    sim.close()


# ---- e. citizens that are not home-sorted -----------------------------------------------------------------------------------------
def test_population_that_is_not_home_sorted(world):
    pop, ep = world[0], world[1]
    per = _area_ref.permuted(pop)
    labels, n_groups = per.age_bands(_group_ref.AGE_EDGES)
    home, group = ref_mod.reference_rows(per, ep, 400, "home"), ref_mod.reference_rows(per, ep, 400, "group", (labels, n_groups))
    tables = {"home": home, "group": group, "all": {"status_rows": group["status_rows"].sum(axis=1, keepdims=True)}}
    assert (np.diff(_area_status_ref.home_area_labels(per).astype(np.int64)) < 0).any()
    sim = Simulator(per, ep)
    sim.set_groups(labels, n_groups)
    sim.run(400)
    check_records(sim, home["records"])
    for where in WHERES:
        for status in STATUS:
            check(sim, tables, where, status, "permuted")
            check(sim, tables, where, status, "permuted", first_step=230, threshold=2)
    sim.close()


# ---- f. a branch after snapshot / rollback under another seed and vaccination rate ------------------------------------------------
def test_branch_after_rollback_under_another_seed_and_rate(world):
    pop, ep, labels, n_groups, tables = world
    trigger = int(np.argmax(tables["home"]["records"]["vaccination_active"])) + 1
    assert trigger + 20 < 300                                                     # the snapshot lies inside the programme: a seam the replay must honour
    sim = Simulator(pop, ep)
    sim.set_groups(labels, n_groups)
    sim.run(300)
    sim.snapshot()
    sim.run(100)
    sim.rollback(seed=99, vaccination_rate=300)
    sim.run(300)
    rec = sim.records_so_far()
    assert len(rec) == 600 and (rec["vaccinated"][300:] != tables["home"]["records"]["vaccinated"][300:600]).any()
    for where in WHERES:
        for status in STATUS:
            for first, last, threshold in ((1, 600, 1), (280, 420, 2)):
                same_summary(sim.curve_summary(where, status, first, last, threshold), from_rows(sim, where, status, first, last, threshold),
                             "branch: %s by %s, steps %d..%d" % (status, where, first, last))
    sim.close()


# ---- h. errors ----------------------------------------------------------------------------------------------------------------------
def test_error_table(world):
    pop, ep, labels, n_groups, tables = world
    lib = _lib.load()
    fn = lib.esim_curve_summary
    HOME, ALL, GROUP, CUR, I = _lib.AREA_HOME, _lib.BY_ALL, _lib.BY_GROUP, _lib.AREA_CURRENT, MASK["infected"]
    out = {k: np.full(pop.n_areas, 12345, np.uint64 if k == "person_steps" else np.uint32) for k in KEYS}
    ptrs = [out[k].ctypes.data_as(u64p if k == "person_steps" else u32p) for k in KEYS]
    none = [None] * 6
    bare = C.c_void_p()
    _lib.check(lib.esim_create(C.byref(ep), C.byref(bare)))
    assert fn(bare, HOME, I, 1, 1, 1, *ptrs) == ESTATE                                        # before an upload
    assert lib.esim_ensemble_begin_peaks(bare, HOME, I, 1, 1, 1, 1) == ESTATE
    lib.esim_destroy(bare)
    assert fn(None, HOME, I, 1, 1, 1, *ptrs) == EINVAL                                        # null context
    sim = Simulator(pop, ep)
    sim.run(10)
    ctx = sim._ctx
    for where in (CUR, _lib.BY_SETTING, 5, -1):
        assert fn(ctx, where, I, 1, 10, 1, *ptrs) == EINVAL, where                            # by the area stood in, and anything else
    for mask in (0, 1 << _lib.SUSCEPTIBLE, 1 << _lib.RECOVERED, 1 << _lib.VACCINATED, I | (1 << _lib.RECOVERED), 0x1F, 1 << 5):
        assert fn(ctx, HOME, mask, 1, 10, 1, *ptrs) == EINVAL, mask                           # the monotone statuses, mixtures, none
    assert fn(ctx, HOME, I, 1, 10, 0, *ptrs) == EINVAL                                        # threshold 0
    assert fn(ctx, GROUP, I, 1, 10, 1, *ptrs) == ESTATE                                       # by group without labels
    assert fn(ctx, HOME, I, 0, 10, 1, *ptrs) == ERANGE                                        # first_step 0
    assert fn(ctx, HOME, I, 5, 4, 1, *ptrs) == ERANGE                                         # last_step < first_step
    assert fn(ctx, HOME, I, 1, 11, 1, *ptrs) == ERANGE and fn(ctx, ALL, I, 11, 11, 1, *ptrs) == ERANGE   # beyond the steps run
    for k in KEYS:
        assert (out[k] == 12345).all(), k                                                     # the refusals left the outputs untouched
    assert fn(ctx, HOME, I, 1, 10, 1, *none) == 0                                             # every output NULL: the call still runs
    assert fn(ctx, HOME, I, 10, 10, 1, *ptrs) == 0
    want = ref_mod.summarize(ref_mod.curves(tables["home"]["status_rows"], "infected"), 10, 10, 1)
    same_summary(out, want, "step 10 alone after the refusals")
    for k in KEYS:                                                                            # any single output alone
        one = [p if j == KEYS.index(k) else None for j, p in enumerate(ptrs)]
        out[k][:] = 777
        assert fn(ctx, HOME, MASK["active"], 1, 10, 1, *one) == 0
        same(out[k], ref_mod.summarize(ref_mod.curves(tables["home"]["status_rows"], "active"), 1, 10, 1)[k], "%s alone" % k)
    with pytest.raises(_lib.EsimError):
        sim.curve_summary("current")
    with pytest.raises(_lib.EsimError):
        sim.curve_summary("home", last_step=11)
    begin = lib.esim_ensemble_begin_peaks
    assert begin(ctx, HOME, I, 1, 10, 1, 0) == EINVAL and begin(ctx, HOME, I, 1, 10, 0, 1) == EINVAL    # min_peak 0, threshold 0
    assert begin(ctx, CUR, I, 1, 10, 1, 1) == EINVAL and begin(ctx, HOME, 1 << _lib.RECOVERED, 1, 10, 1, 1) == EINVAL
    assert begin(ctx, GROUP, I, 1, 10, 1, 1) == ESTATE and begin(ctx, HOME, I, 0, 10, 1, 1) == ERANGE and begin(ctx, HOME, I, 7, 6, 1, 1) == ERANGE
    assert lib.esim_ensemble_read_peaks(ctx, *([None] * 9)) == ESTATE                         # nothing begun
    sim.run(90)                                                                               # the context is usable afterwards
    sim.set_groups(labels, n_groups)
    for where in WHERES:
        check(sim, tables, where, "active", "after the refusals")
    # a sticky device error comes back as the series calls report it
    probe = _lib.StepResult()
    _lib.check(lib.esim_debug_inject_error(ctx, ERANGE), ctx)
    want_rc = lib.esim_read_records(ctx, 1, 1, C.byref(probe))
    rows = np.zeros((4, pop.n_areas), np.uint32)
    assert want_rc != 0 and lib.esim_area_status_series(ctx, HOME, _lib.INFECTED, 1, 4, 1, rows.ctypes.data_as(u32p)) == want_rc
    assert fn(ctx, HOME, I, 1, 10, 1, *ptrs) == want_rc and fn(ctx, ALL, MASK["active"], 1, 10, 1, *none) == want_rc
    sim.close()


def test_a_shard_and_a_communicator_of_two_ranks_are_refused():
    """ESIM_ESTATE from esim_curve_summary, esim_ensemble_begin_peaks and the fold, with the outputs untouched: on a shard without
    a communicator, on a shard with a communicator of two ranks, and on a whole population whose context got a communicator of two
    ranks after the begin (rank 1 holding nobody), which is how a fold can meet one."""
    lib = _lib.load()
    HOME, ALL, I = _lib.AREA_HOME, _lib.BY_ALL, MASK["infected"]
    whole = Population.synthetic("york", n_citizens=20000, n_areas=64, citizens_per_school=2500, n_seeds=20)
    cuts = whole.even_cuts(2)
    s0, s1 = whole.shard(cuts, 0), whole.shard(cuts, 1)
    out = {k: np.full(whole.n_areas, 4242, np.uint64 if k == "person_steps" else np.uint32) for k in KEYS}
    ptrs = [out[k].ctypes.data_as(u64p if k == "person_steps" else u32p) for k in KEYS]
    ep = _lib.default_params(exposure_chance=0.004, seed=123)

    def refused(ctx, word):
        for where in (HOME, ALL):
            assert lib.esim_curve_summary(ctx, where, I, 1, 1, 1, *ptrs) == ESTATE and word in lib.esim_last_error(ctx)
            assert lib.esim_curve_summary(ctx, where, MASK["active"], 1, 1, 1, *([None] * 6)) == ESTATE
        assert lib.esim_ensemble_begin_peaks(ctx, HOME, I, 1, 1, 1, 1) == ESTATE and word in lib.esim_last_error(ctx)
        for k in KEYS:
            assert (out[k] == 4242).all(), k

    def communicator(sim, rank_1_row):
        def allreduce(user, which, host_ptr, n_u32):
            if which == 8:                               # the set-up's layout check: rank 1's row, as its process would add it
                a = (C.c_uint32 * n_u32).from_address(host_ptr)
                a[5:10] = rank_1_row
            return 0
        cb = _lib.ALLREDUCE_FN(allreduce)
        _lib.check(lib.esim_comm_init_callback(sim._ctx, cb, None, 0, 2), sim._ctx)
        return cb                                        # (kept alive by the caller)

    sim = Simulator(s0, ep)
    refused(sim._ctx, b"shard")                                                               # a shard without a communicator
    assert lib.esim_ensemble_fold(sim._ctx) == ESTATE                                         # (nothing could be begun)
    keep = communicator(sim, [s0.n_citizens, s1.n_citizens, whole.n_citizens, s1.n_shared_buildings, s1.n_shared_rooms])
    refused(sim._ctx, b"ranks")                                                               # ... and with one of two ranks
    assert lib.esim_ensemble_fold(sim._ctx) == ESTATE
    sim.close()
    sim = Simulator(whole, ep)
    sim.run(120)
    sim.ensemble_begin_peaks("home", "infected", 1, 120, 1, 1)
    sim.ensemble_fold()
    before = sim.ensemble_read_peaks()
    assert before["members"] == 1 and before["defined"].any()
    assert lib.esim_curve_summary(sim._ctx, HOME, I, 1, 120, 1, *ptrs) == 0 and (out["peak"] != 4242).all()
    for k in KEYS:
        out[k][:] = 4242
    keep = communicator(sim, [whole.n_citizens, 0, whole.n_citizens, 0, 0])                   # rank 1 holds nobody
    refused(sim._ctx, b"ranks")
    assert lib.esim_ensemble_fold(sim._ctx) == ESTATE and b"ranks" in lib.esim_last_error(sim._ctx)   # the fold's own refusal: the kind is still in force
    after = sim.ensemble_read_peaks()
    assert after["members"] == 1
    for k in ref_mod.PEAKS_KEYS:
        same(after[k], before[k], "accumulator %s after the refused fold" % k)
    del keep
    sim.close()


# ---- i. the ensemble kind -----------------------------------------------------------------------------------------------------------
def test_peaks_ensemble_kind(world):
    pop, ep, labels, n_groups, tables = world
    spec = dict(where="home", status="infected", first_step=50, last_step=300, threshold=2)
    sim = Simulator(pop, ep)
    sim.ensemble_begin_peaks(min_peak=3, **spec)
    singles = []
    for k, seed in enumerate((123, 7, 2024)):
        sim.restart(seed=seed)
        sim.run(300 + 20 * k)                                     # (a member may have run on beyond the window)
        sim.ensemble_fold()
        singles.append(sim.curve_summary(**spec))
    same_summary(singles[0], ref_mod.summarize(ref_mod.curves(tables["home"]["status_rows"], "infected"), 50, 300, 2), "the first member is fixture A")
    assert any((a["peak"] != b["peak"]).any() for a, b in zip(singles, singles[1:]))
    want = ref_mod.fold(singles, 3)
    got = sim.ensemble_read_peaks()
    assert got["members"] == 3 and want["hit"].any() and (want["defined"] > want["hit"]).any() and (want["defined"] < 3).any()
    for k in ref_mod.PEAKS_KEYS:
        same(got[k], want[k], "accumulator %s" % k)
    # a member that stopped before the window's end is refused, with nothing folded
    sim.restart(seed=5)
    sim.run(200)
    assert sim.lib.esim_ensemble_fold(sim._ctx) == ERANGE
    again = sim.ensemble_read_peaks()
    assert again["members"] == 3
    for k in ref_mod.PEAKS_KEYS:
        same(again[k], want[k], "accumulator %s after the refused fold" % k)
    # the other reads are refused while this kind is in force, and this one once another kind is
    lib, ctx = sim.lib, sim._ctx
    assert lib.esim_ensemble_read(ctx, None, None, None, None) == ESTATE and lib.esim_ensemble_read_series(ctx, 0, 1, None, None, None, None) == ESTATE
    assert lib.esim_ensemble_read_reproduction(ctx, 0, 1, *([None] * 8)) == ESTATE and lib.esim_ensemble_read_paired(ctx, 0, 1, *([None] * 8)) == ESTATE
    sim.ensemble_begin_reproduction("home", n_rows=2)
    assert lib.esim_ensemble_read_peaks(ctx, *([None] * 9)) == ESTATE
    # by group: new labels invalidate the accumulators
    sim.set_groups(labels, n_groups)
    sim.ensemble_begin_peaks("group", "active", 1, 200, 1, 1)
    sim.ensemble_fold()
    by_group = sim.ensemble_read_peaks()
    assert by_group["members"] == 1 and by_group["defined"].shape == (n_groups,)
    same(by_group["sum_peak"], sim.curve_summary("group", "active", 1, 200)["peak"].astype(np.uint64), "one member by group")
    sim.set_groups(labels, n_groups)
    assert lib.esim_ensemble_read_peaks(ctx, *([None] * 9)) == ESTATE and lib.esim_ensemble_fold(ctx) == ESTATE
    sim.close()


def test_ensemble_run_with_the_peaks_kind(world, tmp_path):
    pop, ep, labels, n_groups, tables = world
    ens = Ensemble(pop, ep)
    area = dict(kind="peaks", where="home", status="active", threshold=3, min_peak=5)
    res = ens.run([dict(seed=123), dict(seed=8)], 250, area=area)
    first = ref_mod.summarize(ref_mod.curves(tables["home"]["status_rows"], "active"), 1, 250, 3)
    a = res.area
    assert res.area_kind == "peaks" and a["members"] == 2 and a["defined"].shape == (pop.n_areas,)
    assert (a["defined"] >= (first["peak"] >= 1)).all() and (a["hit"] >= (first["peak"] >= 5)).all() and (a["peak_mean"] * 2 >= first["peak"]).all()
    same(a["p_peak"], a["hit"] / 2.0, "p_peak")
    assert np.isnan(a["peak_step_mean"][a["defined"] == 0]).all() and not np.isnan(a["peak_step_mean"][a["defined"] > 0]).any()
    with pytest.raises(ValueError):
        ens.run([dict(seed=1)], 50, stop_when_done=True, area=area)
    # forecast: two branches from step 100 of the base run, against the same branches made by hand and folded in numpy
    over = [dict(seed=5), dict(seed=6, vaccination_rate=400)]
    fc = ens.forecast(100, over, 250, area=area)
    sim = Simulator(pop, ep)
    sim.run(100)
    sim.snapshot()
    singles = []
    for m in over:
        sim.rollback(**m)
        sim.run(150)
        singles.append(sim.curve_summary("home", "active", 1, 250, 3))
    sim.close()
    want = peaks_summary(ref_mod.fold(singles, 5))
    assert fc.area_kind == "peaks" and fc.area["members"] == 2 and (singles[0]["peak"] != singles[1]["peak"]).any()
    for k in PEAKS_ARRAYS:
        assert np.array_equal(fc.area[k], want[k], equal_nan=True), k
    res.dump(str(tmp_path))
    saved = np.load(str(tmp_path / "ensemble_area_peaks.npz"))
    assert int(saved["members"]) == 2 and (saved["peak_mean"] == a["peak_mean"]).all() and (saved["duration_var"] == a["duration_var"]).all()
    ens.simulator.close()
