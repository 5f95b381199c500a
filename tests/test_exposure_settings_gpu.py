"""Exposures by setting on the device (esim_exposure_settings, esim_setting_series, esim_building_exposures) against the numpy
reference of tests/_setting_ref.py, which replays both sides of every building exposure of the CPU oracle.  Every comparison
is exact."""
import ctypes as C

import numpy as np
import pytest

import _setting_ref as ref_mod
from epidemicsimulator_amd import Population, Simulator, _lib
from epidemicsimulator_amd.ensemble import Ensemble
from test_exposure_settings import situation

pytestmark = pytest.mark.gpu

EINVAL, ESTATE, ERANGE, ESIM = -1, -4, -5, -6
u32p, u8p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)
H, W, S, T = _lib.SETTING_HOUSEHOLD, _lib.SETTING_WORKPLACE, _lib.SETTING_SCHOOL, _lib.SETTING_TRANSPORT


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, "%s: shape %s, expected %s" % (what, got.shape, want.shape)
    bad = np.flatnonzero(got.ravel() != want.ravel())
    assert bad.size == 0, "%s: %d of %d differ, first at %d: got %s, expected %s" % (what, bad.size, got.size, bad[0], got.ravel()[bad[0]], want.ravel()[bad[0]])


def labels_of(pop):
    return pop.age_bands([18, 40, 65])


def started(name, level=None, steps=None):
    pop, ep, n, ref = ref_mod.cached(name)
    sim = Simulator(pop, ref_mod.copy_params(ep))
    if level is not None:
        sim.set_pipeline(level)
    sim.set_groups(*labels_of(pop))
    sim.run(n if steps is None else steps)
    return sim, pop, n, ref


def check_citizens(sim, ref, what):
    setting, building = sim.exposure_settings()
    same(setting, ref["setting"], what + ": setting per citizen")
    same(building, ref["building"], what + ": building per citizen")


def check_all(sim, pop, ref, n, what, windows=()):
    check_citizens(sim, ref, what)
    lab, n_groups = labels_of(pop)
    for where in ("setting", "home", "group"):
        for kw in (dict(), dict(first_step=3, stride=24), dict(settings=("household", "school"), first_step=2, stride=7)) + tuple(windows):
            got = sim.setting_series(where, **kw)
            mask = Simulator._setting_mask(kw.get("settings"))
            want = ref_mod.rows(ref, pop, where, mask, kw.get("first_step", 1), kw.get("n_rows"), kw.get("stride", 1), lab, n_groups)
            same(got, want, "%s: rows by %s, %s" % (what, where, kw))
    for first, last in ((1, n), (n // 3, n // 2), (n, n)):
        same(sim.building_exposures(first, last), ref_mod.building_counts(ref, pop, first, last), "%s: buildings of steps %d..%d" % (what, first, last))


def at_work_bits(sim, rec):
    bits, cur = np.zeros(len(rec) + 1, bool), False
    for s in range(1, len(rec) + 1):
        if s == 1 or not rec["lockdown"][s - 2]:
            cur = True if s % 24 == sim.params.start_hour else False if s % 24 == sim.params.end_hour else cur
        bits[s] = cur
    return bits


def identities(sim, pop, rec, what):
    """What must hold without any reference: nothing unexplained (the calls return ESIM_OK), and the rows agree with the records
    and with the other read-backs."""
    n = len(rec)
    setting, building = sim.exposure_settings()
    rows = sim.setting_series("setting")
    total = rec["exposures_building"].astype(np.int64) + rec["exposures_bus"]
    same(rows.sum(axis=1, dtype=np.int64), total, what + ": the four columns summed vs the records")
    same(rows[:, T], rec["exposures_bus"], what + ": the transport column vs exposures_bus")
    same(rows[:, :T].sum(axis=1, dtype=np.int64), rec["exposures_building"], what + ": the building columns vs exposures_building")
    same(sim.setting_series("home"), sim.area_status_series("incidence"), what + ": full mask by home vs the incidence rows")
    same(sim.setting_series("home", first_step=5, stride=24), sim.area_status_series("incidence", first_step=5, stride=24), what + ": the same at stride 24")
    same(sim.setting_series("group"), sim.group_series("exposures"), what + ": full mask by group vs the group rows")
    first, last = n // 4, n // 2
    by_area = np.bincount(pop.building_area, weights=sim.building_exposures(first, last), minlength=pop.n_areas).astype(np.int64)
    same(by_area, sim.area_series("exposures", first_step=first, n_rows=last - first + 1).sum(axis=0, dtype=np.int64), what + ": buildings by area vs the exposure rows")
    same(np.bincount(building[building != _lib.NO_ROOM], minlength=pop.n_buildings), sim.building_exposures(1, n), what + ": buildings per citizen vs the tally")
    # a commuter with a work place in another area: the at-work bit of its exposure step alone decides
    cit, step, bus = sim.exposure_events()
    area = pop.building_area
    commuter = (pop.work_building != pop.home_building) & (area[pop.work_building] != area[pop.home_building])
    keep = (step >= 1) & (bus == 0) & commuter[cit]
    assert keep.sum() > 0, what
    at_work = at_work_bits(sim, rec)[step[keep]]
    assert at_work.any() and (~at_work).any(), what
    same(setting[cit[keep]] == H, ~at_work, what + ": commuters exposed at home iff not at work")
    same(np.where(at_work, pop.work_building[cit[keep]], pop.home_building[cit[keep]]), building[cit[keep]], what + ": their buildings")


# ---- 1. fixture A: lockdown and programme run, two execution forms, restarts, a permuted population -------------------------
@pytest.mark.parametrize("level", [0, None])
def test_fixture_a(level):
    situation("fixture_a")
    sim, pop, n, ref = started("fixture_a", level)
    rec = sim.records_so_far()
    same(rec["exposures_building"], ref["records"]["exposures_building"], "the run itself vs the oracle")
    lock = int(np.argmax(rec["lockdown"])) + 1
    assert rec["lockdown"][lock - 1 + 20] and lock + 20 + 150 <= n
    before = (sim.download_state(), sim.records_so_far(), sim.exposure_events(), sim.area_census("home"))
    check_all(sim, pop, ref, n, "fixture A, level %s" % level, windows=(dict(first_step=lock + 20, n_rows=150), dict(first_step=lock + 20, n_rows=6, stride=24)))
    after = (sim.download_state(), sim.records_so_far(), sim.exposure_events(), sim.area_census("home"))
    for k in before[0]:
        same(after[0][k], before[0][k], "state untouched: " + k)
    assert (after[1] == before[1]).all()
    for a, b in zip(after[2], before[2]):
        same(a, b, "exposure log untouched")
    same(after[3], before[3], "census untouched")
    identities(sim, pop, rec, "fixture A")
    if level is None:
        sim.restart()
        sim.run(n)
        check_all(sim, pop, ref, n, "fixture A after esim_restart")
        sim.restart(seeds=pop.seeds)
        sim.run(n)
        check_all(sim, pop, ref, n, "fixture A after esim_restart_seeded")
    sim.close()


def test_permuted_population():
    sim, pop, n, ref = started("permuted")
    assert (np.diff(pop.home_building.astype(np.int64)) < 0).any()          # (not home-sorted: the residents go through res_idx)
    check_all(sim, pop, ref, n, "permuted fixture A")
    sim.close()


# ---- 2. identities, also without an oracle ----------------------------------------------------------------------------------
def test_york_5000_steps_identities():
    pop = Population.synthetic("york")
    sim = Simulator(pop, _lib.default_params())
    sim.set_groups(*labels_of(pop))
    rec = sim.run(5000)
    assert len(rec) == 5000
    identities(sim, pop, rec, "york")
    sim.close()


# ---- 3 .. 6. worlds built for one situation each -------------------------------------------------------------------------------
def test_ties_go_to_the_household():
    situation("ties")
    sim, pop, n, ref = started("ties")
    check_all(sim, pop, ref, n, "ties")
    ties = ref["home_ok"] & ref["work_ok"]
    setting, building = sim.exposure_settings()
    assert ties.sum() >= 10 and (setting[ties] == H).all() and (building[ties] == pop.home_building[ties]).all()
    sim.close()


def test_256_infected_at_home_expose_nobody_there():
    situation("as_u8")
    sim, pop, n, ref = started("as_u8")
    check_all(sim, pop, ref, n, "as u8")
    setting, building = sim.exposure_settings()
    at_256 = (ref["step"] > 0) & (ref["n_home"] == 256)
    assert at_256.any() and (setting[at_256] == W).all() and (building[at_256] == 1).all()
    assert (setting[ref["n_home"] > 256] == H).any()
    sim.close()


def test_school_against_household():
    situation("school")
    sim, pop, n, ref = started("school")
    check_all(sim, pop, ref, n, "school world")
    identities(sim, pop, sim.records_so_far(), "school world")
    sim.close()


def test_frozen_bus_hour_and_vaccinated_housemate():
    situation("situations")
    sim, pop, n, ref = started("situations")
    check_all(sim, pop, ref, n, "situations")
    sim.close()


# ---- 7. the draw seam of a rollback ------------------------------------------------------------------------------------------
def checkpoint_codes(sim):
    size = C.c_size_t(0)
    rc = sim.lib.esim_checkpoint_size(sim._ctx, C.byref(size))
    if rc:
        buf = np.zeros(64, np.uint8)
        return rc, sim.lib.esim_checkpoint_save(sim._ctx, buf.ctypes.data_as(C.c_void_p), buf.size)
    buf = np.zeros(size.value, np.uint8)
    return rc, sim.lib.esim_checkpoint_save(sim._ctx, buf.ctypes.data_as(C.c_void_p), buf.size)


def test_rollback_under_another_seed_and_exposure_chance():
    situation("rollback")
    pop, a, t, b, n = ref_mod.rollback_world()
    ref_b, ref_c, ref_a = (ref_mod.cached(k)[3] for k in ("rollback", "rollback_chance", "rollback_straight"))
    sim = Simulator(pop, ref_mod.copy_params(a))
    sim.set_groups(*labels_of(pop))
    sim.run(t)
    sim.snapshot()
    sim.run(60)                                                      # a future that the rollback abandons
    sim.rollback(seed=int(b.seed), exposure_chance=b.exposure_chance)
    sim.run(n - t)
    same(sim.records_so_far()["exposures_building"], ref_b["records"]["exposures_building"], "the branch itself vs the piecewise oracle")
    check_all(sim, pop, ref_b, n, "branch under another seed and chance")
    assert checkpoint_codes(sim) == (ESTATE, ESTATE)                 # (the seam of the vaccination replay: as before)
    # another chance alone: a draw seam, but none that the checkpoint calls know of
    sim.rollback(exposure_chance=b.exposure_chance)
    sim.run(n - t)
    check_all(sim, pop, ref_c, n, "branch under another chance")
    assert checkpoint_codes(sim) == (0, 0)
    # back to the snapshot's own values: one history, no seam
    sim.rollback()
    sim.run(n - t)
    check_all(sim, pop, ref_a, n, "branch under the snapshot's own values")
    assert checkpoint_codes(sim) == (0, 0)
    # the draw seam outlives the snapshot
    sim.rollback(seed=int(b.seed), exposure_chance=b.exposure_chance)
    sim.run(n - t)
    _lib.check(sim.lib.esim_snapshot_drop(sim._ctx), sim._ctx)
    assert sim.snapshot_step() == 0
    check_all(sim, pop, ref_b, n, "the same branch after esim_snapshot_drop")
    assert checkpoint_codes(sim) == (ESTATE, ESTATE)
    # a snapshot on a branch with a draw seam, rolled back under yet other values: three parameter sets are not followed
    sim.restart(ref_mod.copy_params(a))
    sim.run(t)
    sim.snapshot()
    sim.rollback(exposure_chance=b.exposure_chance)
    sim.run(20)
    sim.snapshot()
    sim.rollback()
    sim.run(n - t - 20)
    check_all(sim, pop, ref_c, n, "a second snapshot on the branch, rolled back to under its own values")
    sim.rollback(exposure_chance=0.005)
    sim.run(5)
    assert sim.lib.esim_exposure_settings(sim._ctx, None, None) == ESTATE
    sim.close()


# ---- 8. errors ---------------------------------------------------------------------------------------------------------------
def test_error_table():
    pop, ep, n, ref = ref_mod.cached("school")
    lib = _lib.load()
    rows = np.zeros((4, 4), np.uint32)
    pr = rows.ctypes.data_as(u32p)
    counts = np.zeros(pop.n_buildings, np.uint32)
    pc = counts.ctypes.data_as(u32p)
    series, buildings, per_citizen = lib.esim_setting_series, lib.esim_building_exposures, lib.esim_exposure_settings
    BY = _lib.BY_SETTING
    bare = C.c_void_p()
    _lib.check(lib.esim_create(C.byref(ep), C.byref(bare)))
    assert series(bare, BY, 0xF, 1, 4, 1, pr) == ESTATE and buildings(bare, 1, 1, pc) == ESTATE and per_citizen(bare, None, None) == ESTATE
    lib.esim_destroy(bare)
    assert series(None, BY, 0xF, 1, 4, 1, pr) == EINVAL and buildings(None, 1, 1, pc) == EINVAL and per_citizen(None, None, None) == EINVAL
    sim = Simulator(pop, ref_mod.copy_params(ep))
    sim.run(10)
    ctx = sim._ctx
    assert series(ctx, BY, 0xF, 1, 4, 1, None) == EINVAL and buildings(ctx, 1, 1, None) == EINVAL          # null output
    assert series(ctx, _lib.AREA_CURRENT, 0xF, 1, 4, 1, pr) == EINVAL                                          # a bus has no area
    assert series(ctx, 4, 0xF, 1, 4, 1, pr) == EINVAL and series(ctx, -1, 0xF, 1, 4, 1, pr) == EINVAL
    assert series(ctx, BY, 0, 1, 4, 1, pr) == EINVAL and series(ctx, BY, 0x10, 1, 4, 1, pr) == EINVAL and series(ctx, BY, 0x1F, 1, 4, 1, pr) == EINVAL
    assert series(ctx, BY, 0xF, 1, 4, 0, pr) == EINVAL and series(ctx, BY, 0xF, 1, 0, 1, pr) == EINVAL      # stride 0, no rows
    assert series(ctx, _lib.BY_GROUP, 0xF, 1, 4, 1, pr) == ESTATE                                              # no labels
    assert series(ctx, BY, 0xF, 0, 4, 1, pr) == ERANGE and series(ctx, BY, 0xF, 8, 4, 1, pr) == ERANGE and series(ctx, BY, 0xF, 2, 4, 3, pr) == ERANGE
    assert buildings(ctx, 0, 5, pc) == ERANGE and buildings(ctx, 5, 4, pc) == ERANGE and buildings(ctx, 5, 11, pc) == ERANGE
    assert series(ctx, BY, 0xF, 7, 4, 1, pr) == 0
    same(rows, ref_mod.rows(ref, pop, "setting")[6:10], "rows 7..10 after the refusals")
    assert buildings(ctx, 10, 10, pc) == 0 and per_citizen(ctx, None, None) == 0
    with pytest.raises(_lib.EsimError):
        sim.setting_series("current")
    with pytest.raises(_lib.EsimError):
        sim.building_exposures(1, 11)
    sim.run(n - 10)                                                                                             # the context is usable afterwards
    check_citizens(sim, ref, "after the refusals")
    # a sticky device-side error comes back as the series calls report it
    _lib.check(lib.esim_debug_inject_error(ctx, ERANGE), ctx)
    want = lib.esim_area_status_series(ctx, _lib.AREA_HOME, _lib.AREA_SERIES_INCIDENCE, 1, 4, 1, np.zeros((4, pop.n_areas), np.uint32).ctypes.data_as(u32p))
    assert want != 0
    assert series(ctx, BY, 0xF, 1, 4, 1, pr) == want and buildings(ctx, 1, 4, pc) == want and per_citizen(ctx, None, None) == want
    sim.close()


def test_a_context_with_a_communicator_of_two_ranks_is_refused():
    whole = Population.synthetic("york", n_citizens=20000, n_areas=64, citizens_per_school=2500, n_seeds=20)
    cuts = whole.even_cuts(2)
    s0, s1 = whole.shard(cuts, 0), whole.shard(cuts, 1)
    sim = Simulator(s0, _lib.default_params(exposure_chance=0.004, seed=123))

    def allreduce(user, which, host_ptr, n_u32):
        if which == 8:                                   # the set-up's layout check: rank 1's row, as its process would add it
            a = (C.c_uint32 * n_u32).from_address(host_ptr)
            a[5:10] = [s0.n_citizens, s1.n_citizens, whole.n_citizens, s1.n_shared_buildings, s1.n_shared_rooms]
        return 0

    cb = _lib.ALLREDUCE_FN(allreduce)
    _lib.check(sim.lib.esim_comm_init_callback(sim._ctx, cb, None, 0, 2), sim._ctx)
    n_done = C.c_uint32(0)
    _lib.check(sim.lib.esim_run_sharded(sim._ctx, 30, C.byref(n_done)), sim._ctx)
    rows, counts = np.zeros((4, 4), np.uint32), np.zeros(s0.n_buildings, np.uint32)
    assert sim.lib.esim_setting_series(sim._ctx, _lib.BY_SETTING, 0xF, 1, 4, 1, rows.ctypes.data_as(u32p)) == ESTATE
    assert sim.lib.esim_building_exposures(sim._ctx, 1, 4, counts.ctypes.data_as(u32p)) == ESTATE
    assert sim.lib.esim_exposure_settings(sim._ctx, None, None) == ESTATE
    sim.close()


# ---- 9. ensembles ------------------------------------------------------------------------------------------------------------
def test_ensemble_gathers_the_members_settings(tmp_path):
    pop, ep, n, ref = ref_mod.cached("school")
    spec = dict(first_step=5, stride=24)
    ens = Ensemble(pop, ref_mod.copy_params(ep))
    members = [{"seed": int(ep.seed)}, {"seed": 8}, {"seed": 9, "exposure_chance": 0.02}]
    res = ens.run(members, 200, settings=spec)
    assert res.settings.shape == (3, (200 - 5) // 24 + 1, 4) and res.settings.dtype == np.uint32
    ref200 = ref_mod.reference(pop, ep, 200)
    same(res.settings[0], ref_mod.rows(ref200, pop, "setting", first_step=5, stride=24), "member 0 vs the reference")
    for i, m in enumerate(members):
        one = Simulator(pop, ref_mod.copy_params(ep, **m))
        one.run(200)
        same(res.settings[i], one.setting_series("setting", **spec), "member %d vs the same run made singly" % i)
        one.close()
    assert ens.run(members[:1], 200).settings is None
    fc = ens.forecast(100, [{"seed": 5}, {}], 200, settings=dict(n_rows=150))
    assert fc.settings.shape == (2, 150, 4)
    same(fc.settings[1], ref_mod.rows(ref200, pop, "setting", n_rows=150), "the branch under the base parameters vs the reference")
    same(fc.settings[0][:100], fc.settings[1][:100], "the shared history of two branches")
    fc.dump(str(tmp_path))
    same(np.load(tmp_path / "ensemble_settings.npz")["settings"], fc.settings, "ensemble_settings.npz")
    ens.close()
