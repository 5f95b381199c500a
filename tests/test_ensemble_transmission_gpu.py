"""Ensemble maps of transmission on the device: esim_ensemble_begin_settings, esim_ensemble_begin_reproduction,
esim_ensemble_read_reproduction and esim_ensemble_fold with one of them in force, and Ensemble(kind="settings" / "reproduction").
Every comparison of device output is exact integer equality.  The references are two: the rows esim_setting_series and
esim_reproduction_series return for every member, folded in numpy, and the numpy rows of tests/_setting_ref.py and
tests/_tree_ref.py over the CPU oracle's members, so that the replay is not only compared with itself.  The worlds, members and
windows are those of tests/_ens_transmission_ref.py, which tests/test_ensemble_transmission.py shows not to be vacuous."""
import ctypes as C

import numpy as np
import pytest

import _ens_transmission_ref as ens_ref
import _setting_ref as ref_mod
import _tree_ref as tree
from epidemicsimulator_amd import Ensemble, Population, Simulator, _lib
from epidemicsimulator_amd.ensemble import reproduction_summary, series_summary

pytestmark = pytest.mark.gpu

EINVAL, ESTATE, ERANGE = -1, -4, -5
KEYS = ens_ref.REPRODUCTION_KEYS
SERIES_KEYS = ("hit", "sum", "sumsq")
u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
W = ens_ref.W


def started(world):
    pop, ep, n, mem = ens_ref.members(world)
    sim = Simulator(pop, ref_mod.copy_params(ep))
    sim.set_groups(*ens_ref.labels_of(pop))
    return sim, pop, n, mem


def each_member(sim, world, n, mem):
    """Brings the simulator to the end of every member's run in turn: restarts of a plain world, branches of the rollback world."""
    if world == "rollback":
        t = ref_mod.rollback_world()[2]
        sim.run(t)
        sim.snapshot()
        for over, ref in mem:
            sim.rollback(**over)
            sim.run(n - t)
            yield over, ref
    else:
        for over, ref in mem:
            sim.restart(**over)
            sim.run(n)
            yield over, ref


def names(settings):
    return None if settings is None else tuple(_lib.SETTING_NAMES[s] for s in settings)


# ---- 1. exact comparisons ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(ens_ref.REPRODUCTION_CASES)))
def test_reproduction_accumulators_equal_numpy_over_the_series_calls_and_over_the_reference(case):
    world, where, window, r, min_cohort = ens_ref.REPRODUCTION_CASES[case]
    sim, pop, n, mem = started(world)
    sim.ensemble_begin_reproduction(where, min_cohort=min_cohort, r=r, **window)
    xs = []
    for _ in each_member(sim, world, n, mem):
        xs.append(sim.reproduction_series(where, **window))
        sim.ensemble_fold()
    got = sim.ensemble_read_reproduction()
    sim.close()
    assert got["members"] == 3 and got["hit"].shape == xs[0][0].shape
    ens_ref.same_fold(got, ens_ref.fold_reproduction(xs, min_cohort, r), KEYS, "series calls")
    ens_ref.same_fold(got, ens_ref.fold_reproduction(ens_ref.reproduction_of(world, where, window), min_cohort, r), KEYS, "reference")
    if r == (0, 1):
        assert (got["hit"] == got["defined"]).all()


@pytest.mark.parametrize("case", range(len(ens_ref.SETTINGS_CASES)))
def test_settings_accumulators_equal_numpy_over_the_series_calls_and_over_the_reference(case):
    world, where, settings, window, min_cases = ens_ref.SETTINGS_CASES[case]
    sim, pop, n, mem = started(world)
    sim.ensemble_begin_settings(where, names(settings), min_cases=min_cases, **window)
    xs = []
    for _ in each_member(sim, world, n, mem):
        xs.append(sim.setting_series(where, names(settings), **window))
        sim.ensemble_fold()
    got = sim.ensemble_read_series()
    sim.close()
    assert got["members"] == 3 and got["hit"].shape == xs[0].shape
    ens_ref.same_fold(got, ens_ref.fold_settings(xs, min_cases), SERIES_KEYS, "series calls")
    ens_ref.same_fold(got, ens_ref.fold_settings(ens_ref.settings_of(world, where, settings, window), min_cases), SERIES_KEYS, "reference")


# ---- 2. begin, read and kind switching -----------------------------------------------------------------------------------------
def read_codes(sim):
    """(esim_ensemble_read, esim_ensemble_read_series, esim_ensemble_read_reproduction) with every pointer NULL."""
    lib, ctx = sim.lib, sim._ctx
    return (lib.esim_ensemble_read(ctx, None, None, None, None), lib.esim_ensemble_read_series(ctx, 0, 0, None, None, None, None),
            lib.esim_ensemble_read_reproduction(ctx, 0, 0, *([None] * 8)))


def test_begin_read_and_switching_between_the_kinds():
    world = "situations"
    sim, pop, n, mem = started(world)
    window = W(0, 7, 48)
    sim.restart(**mem[0][0])
    sim.run(n)
    x = sim.reproduction_series("home", **window)
    sim.ensemble_begin_reproduction("home", min_cohort=2, r=(3, 2), **window)
    assert read_codes(sim) == (ESTATE, ESTATE, 0)
    assert b"esim_ensemble_read_reproduction" in sim.lib.esim_last_error(sim._ctx)
    sim.ensemble_fold()
    sim.ensemble_fold()
    two = ens_ref.fold_reproduction([x, x], 2, (3, 2))
    full = sim.ensemble_read_reproduction()
    ens_ref.same_fold(full, two, KEYS, "the same member twice")
    # every pointer alone, and a part of the rows
    cells = two["hit"].size
    for i, k in enumerate(("members",) + KEYS):
        out = np.full(1 if k == "members" else cells, 7, np.uint32 if i < 3 else np.uint64)
        args = [None] * 8
        args[i] = out.ctypes.data_as(u32p if i < 3 else u64p)
        assert sim.lib.esim_ensemble_read_reproduction(sim._ctx, 0, window["n_rows"], *args) == 0, k
        assert (out == (2 if k == "members" else two[k].ravel())).all(), k
    part = sim.ensemble_read_reproduction(first_row=2, n_rows=3)
    ens_ref.same_fold(part, {k: v if k == "members" else v[2:5] for k, v in two.items()}, KEYS, "rows 2..4")
    assert sim.ensemble_read_reproduction(first_row=7)["hit"].shape == (0, pop.n_areas)
    lib, ctx = sim.lib, sim._ctx
    assert lib.esim_ensemble_read_reproduction(ctx, 5, 3, *([None] * 8)) == ERANGE and lib.esim_ensemble_read_reproduction(ctx, 8, 0, *([None] * 8)) == ERANGE
    assert lib.esim_ensemble_read_reproduction(ctx, 5, 2, *([None] * 8)) == 0
    # a begin of the same kind and shape zeroes, under other parameters
    sim.ensemble_begin_reproduction("home", min_cohort=1, r=(1, 1), **window)
    zero = sim.ensemble_read_reproduction()
    assert zero["members"] == 0 and all(not zero[k].any() for k in KEYS)
    sim.ensemble_fold()
    ens_ref.same_fold(sim.ensemble_read_reproduction(), ens_ref.fold_reproduction([x], 1, (1, 1)), KEYS, "after the second begin")
    # the settings kind replaces it: esim_ensemble_read_series serves it
    s_window = W(100, 7, 50)
    y = sim.setting_series("home", ("household",), **s_window)
    sim.ensemble_begin_settings("home", ("household",), min_cases=1, **s_window)
    assert read_codes(sim) == (ESTATE, 0, ESTATE)
    sim.ensemble_fold()
    ens_ref.same_fold(sim.ensemble_read_series(), ens_ref.fold_settings([y], 1), SERIES_KEYS, "settings after reproduction")
    sim.ensemble_begin_settings("home", ("household",), min_cases=3, **s_window)               # the same shape: zeroed
    again = sim.ensemble_read_series()
    assert again["members"] == 0 and all(not again[k].any() for k in SERIES_KEYS)
    sim.ensemble_fold()
    ens_ref.same_fold(sim.ensemble_read_series(), ens_ref.fold_settings([y], 3), SERIES_KEYS, "settings, min_cases 3")
    # the series kind in the settings kind's shape: its own buffers, its own rows
    z = sim.area_status_series("infected", "home", **s_window)
    sim.ensemble_begin_series("home", "infected", **s_window)
    assert read_codes(sim) == (ESTATE, 0, ESTATE)
    sim.ensemble_fold()
    ens_ref.same_fold(sim.ensemble_read_series(), ens_ref.fold_settings([z], 1), SERIES_KEYS, "series after settings")
    # back to reproduction in another shape, then the census kind
    sim.ensemble_begin_reproduction("group", first_step=1, n_rows=3, stride=100)
    sim.ensemble_fold()
    ens_ref.same_fold(sim.ensemble_read_reproduction(), ens_ref.fold_reproduction([sim.reproduction_series("group", 1, 3, 100)], 1, (1, 1)), KEYS, "by group")
    sim.ensemble_begin("home")
    assert read_codes(sim) == (0, ESTATE, ESTATE)
    sim.ensemble_fold()
    assert sim.ensemble_read()["members"] == 1
    sim.ensemble_begin_arrival("home")
    assert read_codes(sim) == (0, ESTATE, ESTATE)
    sim.ensemble_begin_reproduction("all", first_step=0, n_rows=2, stride=200)
    assert read_codes(sim) == (ESTATE, ESTATE, 0)
    sim.close()


# ---- 3. what a fold does and refuses -------------------------------------------------------------------------------------------
def test_a_fold_leaves_state_records_log_and_tree_as_they_are_and_reports_nothing_for_a_member_that_stopped_early():
    world = "situations"
    sim, pop, n, mem = started(world)
    window, s_window = W(0, 5, 60), W(1, 5, 60)                      # the last row starts at step 240 / 241
    sim.restart(**mem[0][0])
    sim.run(n)
    before = (sim.download_state(), sim.records_so_far(), sim.exposure_events(), sim.transmission_tree(), sim.area_census("home"))
    x = sim.reproduction_series("group", **window)
    sim.ensemble_begin_reproduction("group", **window)
    sim.ensemble_fold()
    y = sim.setting_series("group", **s_window)
    after = (sim.download_state(), sim.records_so_far(), sim.exposure_events(), sim.transmission_tree(), sim.area_census("home"))
    assert all((after[0][k] == before[0][k]).all() for k in before[0]) and (after[1] == before[1]).all() and (after[4] == before[4]).all()
    assert all((a == b).all() for a, b in zip(after[2], before[2])) and all((a == b).all() for a, b in zip(after[3], before[3]))
    one = ens_ref.fold_reproduction([x], 1, (1, 1))
    ens_ref.same_fold(sim.ensemble_read_reproduction(), one, KEYS, "one member")
    # a member that has not run to the last row: ESIM_ERANGE, nothing folded, members as it was
    sim.restart(seed=5)
    sim.run(239)
    assert sim.lib.esim_ensemble_fold(sim._ctx) == ERANGE and b"rows outside" in sim.lib.esim_last_error(sim._ctx)
    ens_ref.same_fold(sim.ensemble_read_reproduction(), one, KEYS, "after the refused fold")
    sim.run(1)                                                       # step 240 has run: the last row's first step
    x2 = sim.reproduction_series("group", **window)
    sim.ensemble_fold()
    ens_ref.same_fold(sim.ensemble_read_reproduction(), ens_ref.fold_reproduction([x, x2], 1, (1, 1)), KEYS, "the member at step 240")
    # the same for the settings kind, whose rows are 1-based: step 241 is missing
    sim.ensemble_begin_settings("group", **s_window)
    assert sim.lib.esim_ensemble_fold(sim._ctx) == ERANGE
    assert sim.ensemble_read_series()["members"] == 0
    sim.run(1)
    sim.ensemble_fold()
    ens_ref.same_fold(sim.ensemble_read_series(), ens_ref.fold_settings([sim.setting_series("group", **s_window)], 1), SERIES_KEYS, "the member at step 241")
    assert y.shape == (5, 5)
    sim.close()


def test_after_restart_seeded_and_through_reset():
    world = "fixture_a"
    sim, pop, n, mem = started(world)
    window = W(0, 7, 100)
    sim.ensemble_begin_reproduction("home", **window)
    sim.restart(seeds=pop.seeds, **mem[1][0])                        # esim_restart_seeded with the population's own index cases
    sim.run(n)
    x = sim.reproduction_series("home", **window)
    sim.ensemble_fold()
    sim.reset()                                                      # the accumulators are kept through esim_reset and esim_restart
    sim.restart(**mem[2][0])
    got = sim.ensemble_read_reproduction()
    ens_ref.same_fold(got, ens_ref.fold_reproduction([x], 1, (1, 1)), KEYS, "series call")
    ens_ref.same_fold(got, ens_ref.fold_reproduction(ens_ref.reproduction_of(world, "home", window)[1:2], 1, (1, 1)), KEYS, "reference")
    sim.close()


def test_a_forecast_folds_a_window_that_straddles_the_snapshot():
    pop, a, t, b, n = ref_mod.rollback_world()
    mem = ens_ref.members("rollback")[3]
    window = W(50, 4, 50)                                            # cohorts of steps 50 .. 249: the snapshot's step 200 lies inside
    ens = Ensemble(pop, ref_mod.copy_params(a), group=ens_ref.labels_of(pop))
    res = ens.forecast(history_steps=t, members=[o for o, _ in mem], n_steps=n, area=dict(kind="reproduction", where="group", r=(1, 2), **window))
    assert res.n_done.tolist() == [n] * 3 and res.area_kind == "reproduction" and res.area_codes is None
    want_rows = [tree.reproduction_rows(ref, pop, "group", 50, 4, 50, *ens_ref.labels_of(pop)) for _, ref in mem]
    want = ens_ref.fold_reproduction(want_rows, 1, (1, 2))
    assert any((p[0] != q[0]).any() for p, q in zip(want_rows, want_rows[1:])) and any((p[1] != q[1]).any() for p, q in zip(want_rows, want_rows[1:]))
    assert want["sum_cases"][0].all() and want["hit"].any() and (want["defined"] > want["hit"]).any()
    ens_ref.same_fold(ens.simulator.ensemble_read_reproduction(), want, KEYS, "forecast")
    summary = reproduction_summary(want, 50, 50)
    for k in ("defined", "hit", "r", "p_r", "r_se", "cases_mean", "offspring_mean", "steps"):
        assert np.array_equal(res.area[k], summary[k], equal_nan=k not in ("defined", "hit", "steps")), k
    # the settings kind over the same branches, the snapshot still held
    s_window = W(150, 3, 50)
    res = ens.forecast(history_steps=t, members=[o for o, _ in mem], n_steps=n, area=dict(kind="settings", where="setting", min_cases=30, **s_window))
    want = ens_ref.fold_settings(ens_ref.settings_of("rollback", "setting", None, s_window), 30)
    ens_ref.same_fold(ens.simulator.ensemble_read_series(), want, SERIES_KEYS, "forecast, settings")
    assert (res.area["hit"] == want["hit"]).all() and res.area["steps"].tolist() == [150, 200, 250] and want["sum"].any()
    ens.close()


def test_a_rollback_under_another_bus_capacity_is_refused_by_the_reproduction_kind_only():
    pop, a, t, b, n = ref_mod.rollback_world()
    sim = Simulator(pop, ref_mod.copy_params(a))
    window = W(1, 3, 50)
    sim.run(t)
    sim.snapshot()
    sim.ensemble_begin_reproduction("home", **window)
    sim.ensemble_fold()
    one = sim.ensemble_read_reproduction()
    assert one["members"] == 1 and one["sum_cases"].any()
    sim.rollback(bus_capacity=int(a.bus_capacity) + 5)
    sim.run(10)
    assert sim.lib.esim_ensemble_fold(sim._ctx) == ESTATE and b"two capacities" in sim.lib.esim_last_error(sim._ctx)
    ens_ref.same_fold(sim.ensemble_read_reproduction(), one, KEYS, "after the refused fold")
    # the settings replay no bus: their kind folds the same history
    sim.ensemble_begin_settings("home", **window)
    sim.ensemble_fold()
    ens_ref.same_fold(sim.ensemble_read_series(), ens_ref.fold_settings([sim.setting_series("home", **window)], 1), SERIES_KEYS, "settings under two capacities")
    # a history mixed twice is refused by both
    sim.restart(ref_mod.copy_params(a))
    sim.run(t)
    sim.snapshot()
    sim.rollback(exposure_chance=b.exposure_chance)
    sim.run(20)
    sim.snapshot()
    sim.rollback(exposure_chance=0.005)
    sim.run(5)
    assert sim.lib.esim_ensemble_fold(sim._ctx) == ESTATE and sim.ensemble_read_series()["members"] == 1
    sim.ensemble_begin_reproduction("home", **window)
    assert sim.lib.esim_ensemble_fold(sim._ctx) == ESTATE and sim.ensemble_read_reproduction()["members"] == 0
    sim.close()


def test_a_sharded_context_and_a_communicator_of_two_ranks_are_refused():
    whole = Population.synthetic("york", n_citizens=20000, n_areas=64, citizens_per_school=2500)
    cuts = whole.even_cuts(2)
    s0, s1 = whole.shard(cuts, 0), whole.shard(cuts, 1)
    sim = Simulator(s0, _lib.default_params())
    lib, ctx = sim.lib, sim._ctx
    # a shard without a communicator: the begin has nothing to object to, the fold's replay has
    sim.ensemble_begin_settings("home", first_step=1, n_rows=2, stride=1)
    assert lib.esim_ensemble_fold(ctx) == ESTATE and b"shard" in lib.esim_last_error(ctx)
    sim.ensemble_begin_reproduction("home", first_step=0, n_rows=2, stride=1)
    assert lib.esim_ensemble_fold(ctx) == ESTATE and b"shard" in lib.esim_last_error(ctx)
    assert sim.ensemble_read_reproduction()["members"] == 0

    def allreduce(user, which, host_ptr, n_u32):
        if which == 8:                                   # the set-up's layout check: rank 1's row, as its process would add it
            a = (C.c_uint32 * n_u32).from_address(host_ptr)
            a[5:10] = [s0.n_citizens, s1.n_citizens, whole.n_citizens, s1.n_shared_buildings, s1.n_shared_rooms]
        return 0

    cb = _lib.ALLREDUCE_FN(allreduce)
    _lib.check(lib.esim_comm_init_callback(ctx, cb, None, 0, 2), ctx)
    assert lib.esim_ensemble_begin_settings(ctx, _lib.AREA_HOME, 0xF, 1, 4, 1, 1) == ESTATE
    assert lib.esim_ensemble_begin_reproduction(ctx, _lib.AREA_HOME, 0, 4, 24, 1, 1, 1) == ESTATE
    assert lib.esim_ensemble_fold(ctx) == ESTATE
    sim.close()


def test_replaced_labels_invalidate_accumulators_begun_by_group_and_an_upload_drops_them():
    sim, pop, n, mem = started("situations")
    labels, n_groups = ens_ref.labels_of(pop)
    sim.run(30)
    lib, ctx = sim.lib, sim._ctx
    for begin, read in ((lambda: sim.ensemble_begin_reproduction("group", first_step=0, n_rows=3, stride=10), lambda: lib.esim_ensemble_read_reproduction(ctx, 0, 0, *([None] * 8))),
                        (lambda: sim.ensemble_begin_settings("group", first_step=1, n_rows=3, stride=10), lambda: lib.esim_ensemble_read_series(ctx, 0, 0, None, None, None, None))):
        begin()
        sim.ensemble_fold()
        assert read() == 0
        sim.set_groups(labels, n_groups)
        assert lib.esim_ensemble_fold(ctx) == ESTATE and read() == ESTATE
        begin()
        sim.ensemble_fold()
        assert read() == 0
    # by area: replaced labels leave them alone; a new upload drops them
    sim.ensemble_begin_reproduction("home", first_step=0, n_rows=3, stride=10)
    sim.set_groups(labels, n_groups)
    sim.ensemble_fold()
    assert sim.ensemble_read_reproduction()["members"] == 1
    ps = pop.as_struct()
    _lib.check(lib.esim_upload_population(ctx, C.byref(ps)), ctx)
    assert lib.esim_ensemble_fold(ctx) == ESTATE and lib.esim_ensemble_read_reproduction(ctx, 0, 0, *([None] * 8)) == ESTATE
    sim.close()


# ---- 4. errors, and end to end -------------------------------------------------------------------------------------------------
def test_the_error_table():
    pop = ens_ref.members("situations")[0]
    lib = _lib.load()
    ctx = C.c_void_p()
    _lib.check(lib.esim_create(C.byref(_lib.default_params()), C.byref(ctx)))
    assert lib.esim_ensemble_begin_settings(ctx, _lib.AREA_HOME, 0xF, 1, 4, 1, 1) == ESTATE            # before an upload
    assert lib.esim_ensemble_begin_reproduction(ctx, _lib.AREA_HOME, 0, 4, 24, 1, 1, 1) == ESTATE
    assert lib.esim_ensemble_read_reproduction(ctx, 0, 0, *([None] * 8)) == ESTATE
    lib.esim_destroy(ctx)
    sim = Simulator(pop, _lib.default_params())
    settings = lambda *a: sim.lib.esim_ensemble_begin_settings(sim._ctx, *a)
    reproduction = lambda *a: sim.lib.esim_ensemble_begin_reproduction(sim._ctx, *a)
    assert sim.lib.esim_ensemble_fold(sim._ctx) == ESTATE and sim.lib.esim_ensemble_read_reproduction(sim._ctx, 0, 0, *([None] * 8)) == ESTATE    # before begin
    # (where, mask, first_step, n_rows, stride, min_cases)
    for bad in ((_lib.AREA_CURRENT, 0xF, 1, 4, 1, 1), (_lib.BY_ALL, 0xF, 1, 4, 1, 1), (7, 0xF, 1, 4, 1, 1), (-1, 0xF, 1, 4, 1, 1), (_lib.AREA_HOME, 0, 1, 4, 1, 1),
                (_lib.AREA_HOME, 0x10, 1, 4, 1, 1), (_lib.AREA_HOME, 0xF, 1, 4, 0, 1), (_lib.AREA_HOME, 0xF, 1, 0, 1, 1)):
        assert settings(*bad) == EINVAL, bad
    assert settings(_lib.AREA_HOME, 0xF, 0, 4, 1, 1) == ERANGE
    assert settings(_lib.BY_GROUP, 0xF, 1, 4, 1, 1) == ESTATE                                           # by group without labels
    assert settings(_lib.BY_SETTING, 0x1, 1, 4, 1, 0) == 0
    # (where, first_step, n_rows, stride, min_cohort, r_num, r_den)
    for bad in ((_lib.AREA_CURRENT, 0, 4, 24, 1, 1, 1), (_lib.BY_SETTING, 0, 4, 24, 1, 1, 1), (7, 0, 4, 24, 1, 1, 1), (_lib.AREA_HOME, 0, 4, 0, 1, 1, 1),
                (_lib.AREA_HOME, 0, 0, 24, 1, 1, 1), (_lib.AREA_HOME, 0, 4, 24, 0, 1, 1), (_lib.AREA_HOME, 0, 4, 24, 1, 1, 0)):
        assert reproduction(*bad) == EINVAL, bad
    assert reproduction(_lib.BY_GROUP, 0, 4, 24, 1, 1, 1) == ESTATE                                     # by group without labels
    assert sim.lib.esim_ensemble_read_series(sim._ctx, 0, 4, None, None, None, None) == 0               # (none of these replaced the settings kind)
    assert reproduction(_lib.BY_ALL, 0, 4, 24, 1, 0, 1) == 0                                            # first_step 0 and r_num 0 are allowed
    assert sim.lib.esim_ensemble_fold(sim._ctx) == ERANGE                                               # nothing has run
    sim._ens_rows, sim._ens_n = 4, 1
    assert sim.ensemble_read_reproduction()["members"] == 0
    sim.close()


def test_ensemble_run_end_to_end(tmp_path):
    world = "situations"
    pop, ep, n, mem = ens_ref.members(world)
    codes = ["E%05d" % i for i in range(pop.n_areas)]
    ens = Ensemble(pop, ref_mod.copy_params(ep), area_codes=codes, group=ens_ref.labels_of(pop))
    overrides = [o for o, _ in mem]
    done = n - int(ep.exposed_time) - 1 - int(ep.infected_time)       # the last complete cohort step: 17 of 450
    assert done == 17
    with pytest.raises(ValueError, match="no complete cohort row"):
        ens.run(overrides, n, area=dict(kind="reproduction", where="home", stride=24))
    res = ens.run(overrides, n, area=dict(kind="reproduction", where="home", stride=6, r=(2, 1)))
    assert res.n_done.tolist() == [n] * 3 and res.area_codes == codes
    window = W(0, 3, 6)                                              # rows end at steps 5, 11 and 17
    rows = ens_ref.reproduction_of(world, "home", window)
    acc = ens_ref.fold_reproduction(rows, 1, (2, 1))
    ens_ref.same_fold(ens.simulator.ensemble_read_reproduction(), acc, KEYS, "Ensemble.run")
    a, want = res.area, ens_ref.direct_summary(rows, 1, (2, 1))
    assert a["members"] == 3 and a["steps"].tolist() == [0, 6, 12] and (a["hit"] == acc["hit"]).all() and (a["defined"] == acc["defined"]).all()
    assert acc["hit"].any() and (acc["defined"] > acc["hit"]).any() and np.isfinite(a["r_se"]).any()
    for k in ("r", "p_r", "cases_mean", "offspring_mean"):
        assert np.allclose(a[k], want[k], rtol=1e-12, atol=0, equal_nan=True), k
    err, bound = np.abs(a["r_se"] - want["r_se"]), 1e-12 * np.abs(want["r_se"]) + ens_ref.se_atol(3, want["r"])
    assert (np.isnan(a["r_se"]) == np.isnan(want["r_se"])).all() and (np.isnan(err) | (err <= bound)).all()
    res.dump(str(tmp_path))
    z = np.load(tmp_path / "ensemble_area_reproduction.npz")
    assert np.array_equal(z["r"], a["r"], equal_nan=True) and z["codes"].tolist() == codes
    # household-acquired cases in the week after the lockdown began (step 136), by group
    s_window = W(137, 1, 168)
    res = ens.run(overrides, n, area=dict(kind="settings", where="group", settings=("household",), min_cases=5, **s_window))
    want = ens_ref.fold_settings(ens_ref.settings_of(world, "group", (tree.H,), s_window), 5)
    ens_ref.same_fold(ens.simulator.ensemble_read_series(), want, SERIES_KEYS, "Ensemble.run, settings")
    summary = series_summary(3, want["hit"], want["sum"], want["sumsq"], 137, 168)
    assert res.area_codes is None and all(np.array_equal(res.area[k], summary[k]) for k in ("hit", "mean", "var", "steps")) and want["sum"].all()
    ens.close()
