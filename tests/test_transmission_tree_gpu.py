"""Who infected whom on the device (esim_transmission_tree, esim_offspring, esim_reproduction_series, esim_mixing_matrix) against
the numpy reference of tests/_tree_ref.py, which finds the Infected present at every exposure of the CPU oracle and replays the
bus order and the pick.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import _setting_ref as ref_mod
import _tree_ref as tree
from epidemicsimulator_amd import Population, Simulator, _lib
from epidemicsimulator_amd.ensemble import Ensemble
from test_transmission_tree import situation

pytestmark = pytest.mark.gpu

EINVAL, ESTATE, ERANGE = -1, -4, -5
u32p = C.POINTER(C.c_uint32)


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, "%s: shape %s, expected %s" % (what, got.shape, want.shape)
    bad = np.flatnonzero(got.ravel() != want.ravel())
    assert bad.size == 0, "%s: %d of %d differ, first at %d: got %s, expected %s" % (what, bad.size, got.size, bad[0], got.ravel()[bad[0]], want.ravel()[bad[0]])


def labels_of(pop):
    return pop.age_bands([18, 40, 65])


def started(name, level=None):
    pop, ep, n, ref = tree.cached(name)
    sim = Simulator(pop, ref_mod.copy_params(ep))
    if level is not None:
        sim.set_pipeline(level)
    sim.set_groups(*labels_of(pop))
    sim.run(n)
    return sim, pop, n, ref


def check_all(sim, pop, ref, n, what):
    infector, k, gen = sim.transmission_tree()
    same(k, ref["n_candidates"], what + ": candidates per citizen")
    same(infector, ref["infector"], what + ": infector per citizen")
    same(gen, ref["generation"], what + ": generation per citizen")
    for first, last in ((1, n), (n // 3, n // 2), (n, n)):
        same(sim.offspring(first, last), tree.offspring(ref, pop, first, last), "%s: offspring of steps %d..%d" % (what, first, last))
    lab, n_groups = labels_of(pop)
    for where in ("all", "home", "group"):
        for first in (0, 5):
            for stride in (1, 24, 7):
                cases, off = sim.reproduction_series(where, first_step=first, stride=stride)
                want = tree.reproduction_rows(ref, pop, where, first, None, stride, lab, n_groups)
                same(cases, want[0], "%s: cases by %s from %d, stride %d" % (what, where, first, stride))
                same(off, want[1], "%s: offspring by %s from %d, stride %d" % (what, where, first, stride))
    same(sim.mixing_matrix(), tree.mixing_matrix(ref, pop, lab, n_groups), what + ": matrix, all settings")
    same(sim.mixing_matrix("household", 2, n - 1), tree.mixing_matrix(ref, pop, lab, n_groups, 1, 2, n - 1), what + ": matrix, households, steps 2..n-1")


# ---- 1. every world against the reference ----------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [0, None])
def test_fixture_a(level):
    situation("fixture_a")
    sim, pop, n, ref = started("fixture_a", level)
    before = (sim.download_state(), sim.records_so_far(), sim.exposure_events(), sim.area_census("home"))
    check_all(sim, pop, ref, n, "fixture A, level %s" % level)
    after = (sim.download_state(), sim.records_so_far(), sim.exposure_events(), sim.area_census("home"))
    for key in before[0]:
        same(after[0][key], before[0][key], "state untouched: " + key)
    assert (after[1] == before[1]).all()
    for a, b in zip(after[2], before[2]):
        same(a, b, "exposure log untouched")
    same(after[3], before[3], "census untouched")
    if level is None:
        sim.restart()
        sim.run(n)
        check_all(sim, pop, ref, n, "fixture A after esim_restart")
        sim.restart(seeds=pop.seeds)
        sim.run(n)
        check_all(sim, pop, ref, n, "fixture A after esim_restart_seeded")
    sim.close()


@pytest.mark.parametrize("name", ["permuted", "ties", "as_u8", "school", "situations", "bus"])
def test_world(name):
    if name != "permuted":
        situation(name)
    sim, pop, n, ref = started(name)
    check_all(sim, pop, ref, n, name)
    sim.close()


def test_rollback_under_another_seed_and_exposure_chance():
    pop, a, t, b, n = ref_mod.rollback_world()
    ref_b, ref_c, ref_a = (tree.cached(k)[3] for k in ("rollback", "rollback_chance", "rollback_straight"))
    assert ((ref_b["setting"] == tree.T) & (ref_b["step"] <= t) & (ref_b["n_buses"] >= 2)).any()      # bus keys under the old seed
    assert ((ref_b["setting"] == tree.T) & (ref_b["step"] > t) & (ref_b["n_buses"] >= 2)).any()       # ... and under the new one
    sim = Simulator(pop, ref_mod.copy_params(a))
    sim.set_groups(*labels_of(pop))
    sim.run(t)
    sim.snapshot()
    sim.run(60)                                                      # a future that the rollback abandons
    sim.rollback(seed=int(b.seed), exposure_chance=b.exposure_chance)
    sim.run(n - t)
    check_all(sim, pop, ref_b, n, "branch under another seed and chance")
    sim.rollback(exposure_chance=b.exposure_chance)
    sim.run(n - t)
    check_all(sim, pop, ref_c, n, "branch under another chance")
    sim.rollback()
    sim.run(n - t)
    check_all(sim, pop, ref_a, n, "branch under the snapshot's own values")
    # a rollback under another bus_capacity: two capacities in one history are not replayed; the settings still are
    sim.rollback(bus_capacity=int(a.bus_capacity) + 5)
    sim.run(10)
    lib, ctx = sim.lib, sim._ctx
    one = np.zeros(max(pop.n_citizens, 16), np.uint32)
    p = one.ctypes.data_as(u32p)
    assert lib.esim_transmission_tree(ctx, None, None, None) == ESTATE and lib.esim_offspring(ctx, 1, 1, p) == ESTATE
    assert lib.esim_reproduction_series(ctx, _lib.BY_ALL, 0, 1, 1, p, None) == ESTATE and lib.esim_mixing_matrix(ctx, 0xF, 1, 1, p) == ESTATE
    assert b"two capacities" in lib.esim_last_error(ctx)
    assert lib.esim_exposure_settings(ctx, None, None) == 0
    sim.rollback()                                                   # (back under the snapshot's capacity: one history again)
    sim.run(n - t)
    check_all(sim, pop, ref_a, n, "after the branch under another capacity was abandoned")
    sim.rollback(bus_capacity=int(a.bus_capacity) + 5)
    sim.restart(ref_mod.copy_params(a))
    sim.run(t)
    assert lib.esim_transmission_tree(ctx, None, None, None) == 0
    # a history mixed twice
    sim.snapshot()
    sim.rollback(exposure_chance=b.exposure_chance)
    sim.run(20)
    sim.snapshot()
    sim.rollback(exposure_chance=0.005)
    sim.run(5)
    assert lib.esim_transmission_tree(ctx, None, None, None) == ESTATE
    sim.close()


# ---- 2. identities without an oracle ---------------------------------------------------------------------------------------
def test_york_5000_steps_identities():
    pop = Population.synthetic("york")
    ep = _lib.default_params(max_steps=5600)
    sim = Simulator(pop, ep)
    sim.set_groups(*labels_of(pop))
    n = 5000
    rec = sim.run(n)
    assert len(rec) == n
    total = int(rec["exposures_building"].sum()) + int(rec["exposures_bus"].sum())
    infector, k, gen = sim.transmission_tree()                       # (ESIM_OK: nothing unexplained, nobody without a candidate)
    cit, step, bus = sim.exposure_events()
    te = np.full(pop.n_citizens, -1, np.int64)
    te[cit] = step
    seeds = np.unique(pop.seeds)
    te[seeds] = -(int(ep.exposed_time) + 1)                          # Infected from step 1
    exposed = np.zeros(pop.n_citizens, bool)
    exposed[cit[step >= 1]] = True
    print("york: %d exposures, deepest generation %d, most candidates %d, most offspring %d" % (total, gen[exposed].max(), k.max(), sim.offspring(1, n).max()))
    assert total >= 1000 and gen[exposed].max() >= 5                # (York's epidemic is contained by its interventions, but it is one)
    assert exposed.sum() == total and (infector[exposed] < pop.n_citizens).all() and (k[exposed] >= 1).all()
    assert (infector[~exposed] == _lib.NO_INFECTOR).all() and (gen[seeds] == 0).all()
    same(gen[exposed], gen[infector[exposed]] + 1, "generation = the infector's + 1")
    assert (te[infector[exposed]] + int(ep.exposed_time) + 1 <= te[exposed]).all()
    assert (te[exposed] <= te[infector[exposed]] + int(ep.exposed_time) + 1 + int(ep.infected_time)).all()
    assert int(sim.offspring(1, n).sum()) == total and int(sim.mixing_matrix().sum()) == total
    same(sim.offspring(1, n), np.bincount(infector[exposed], minlength=pop.n_citizens), "offspring vs the tree")
    same(sim.reproduction_series("home", first_step=1, stride=1)[0], sim.area_status_series("incidence"), "cases by home vs the incidence rows")
    same(sim.reproduction_series("group", first_step=1, stride=24)[0], sim.group_series("exposures", stride=24), "cases by group vs the group rows")
    cases, off = sim.reproduction_series("all")
    assert int(cases.sum()) == total + len(seeds) and int(off.sum()) == total
    # a row is complete once the last Infected step of a citizen exposed in its last step has run
    complete = np.arange(len(cases)) * 24 + 23 + int(ep.exposed_time) + 1 + int(ep.infected_time) <= n
    assert complete.sum() >= 100
    sim.run(500)
    cases2, off2 = sim.reproduction_series("all")
    same(cases2[:len(cases)][complete], cases[complete], "complete rows: cases after 500 more steps")
    same(off2[:len(off)][complete], off[complete], "complete rows: offspring after 500 more steps")
    sim.close()


# ---- 3. errors -------------------------------------------------------------------------------------------------------------
def test_error_table():
    pop, ep, n, ref = tree.cached("school")
    lib = _lib.load()
    lab, n_groups = labels_of(pop)
    buf = np.zeros(max(pop.n_citizens, 4 * pop.n_areas, n_groups * n_groups), np.uint32)
    p = buf.ctypes.data_as(u32p)
    tr, offs, series, matrix = lib.esim_transmission_tree, lib.esim_offspring, lib.esim_reproduction_series, lib.esim_mixing_matrix
    ALL = _lib.BY_ALL
    bare = C.c_void_p()
    _lib.check(lib.esim_create(C.byref(ep), C.byref(bare)))
    assert tr(bare, None, None, None) == ESTATE and offs(bare, 1, 1, p) == ESTATE and series(bare, ALL, 0, 1, 1, p, p) == ESTATE and matrix(bare, 0xF, 1, 1, p) == ESTATE
    lib.esim_destroy(bare)
    assert tr(None, None, None, None) == EINVAL and offs(None, 1, 1, p) == EINVAL and series(None, ALL, 0, 1, 1, p, p) == EINVAL and matrix(None, 0xF, 1, 1, p) == EINVAL
    sim = Simulator(pop, ref_mod.copy_params(ep))
    sim.run(10)
    ctx = sim._ctx
    assert offs(ctx, 1, 1, None) == EINVAL and matrix(ctx, 0xF, 1, 1, None) == EINVAL and series(ctx, ALL, 0, 4, 1, None, None) == EINVAL      # null output
    assert series(ctx, _lib.AREA_CURRENT, 0, 4, 1, p, p) == EINVAL                                             # a bus has no area
    assert series(ctx, _lib.BY_SETTING, 0, 4, 1, p, p) == EINVAL and series(ctx, 5, 0, 4, 1, p, p) == EINVAL and series(ctx, -1, 0, 4, 1, p, p) == EINVAL
    assert series(ctx, ALL, 0, 4, 0, p, p) == EINVAL and series(ctx, ALL, 0, 0, 1, p, p) == EINVAL             # stride 0, no rows
    assert matrix(ctx, 0, 1, 1, p) == EINVAL and matrix(ctx, 0x10, 1, 1, p) == EINVAL and matrix(ctx, 0x1F, 1, 1, p) == EINVAL
    assert series(ctx, _lib.BY_GROUP, 0, 4, 1, p, p) == ESTATE and matrix(ctx, 0xF, 1, 1, p) == ESTATE          # no labels
    assert series(ctx, ALL, 8, 4, 1, p, p) == ERANGE and series(ctx, ALL, 2, 4, 3, p, p) == ERANGE and series(ctx, ALL, 11, 1, 1, p, p) == ERANGE
    assert offs(ctx, 0, 5, p) == ERANGE and offs(ctx, 5, 4, p) == ERANGE and offs(ctx, 5, 11, p) == ERANGE
    sim.set_groups(lab, n_groups)
    assert matrix(ctx, 0xF, 0, 5, p) == ERANGE and matrix(ctx, 0xF, 5, 4, p) == ERANGE and matrix(ctx, 0xF, 5, 11, p) == ERANGE
    # after the refusals: rows 7..10, then either output alone, then first_step 0 with the last row on the last step
    cases, off = sim.reproduction_series("all", first_step=7, n_rows=4, stride=1)
    want = tree.reproduction_rows(ref, pop, "all", 0, stride=1)
    same(cases, want[0][7:11], "cases of steps 7..10")
    one = np.zeros(4, np.uint32)
    assert series(ctx, ALL, 7, 4, 1, one.ctypes.data_as(u32p), None) == 0
    same(one, want[0][7:11, 0], "cases alone")
    assert series(ctx, ALL, 0, 11, 1, None, p) == 0 and offs(ctx, 10, 10, p) == 0 and tr(ctx, None, None, None) == 0
    with pytest.raises(_lib.EsimError):
        sim.reproduction_series("current")
    with pytest.raises(_lib.EsimError):
        sim.offspring(1, 11)
    sim.run(n - 10)                                                                                             # the context is usable afterwards
    same(sim.transmission_tree()[0], ref["infector"], "after the refusals")
    # a sticky device-side error comes back as the series calls report it
    _lib.check(lib.esim_debug_inject_error(ctx, ERANGE), ctx)
    want = lib.esim_area_status_series(ctx, _lib.AREA_HOME, _lib.AREA_SERIES_INCIDENCE, 1, 4, 1, np.zeros((4, pop.n_areas), np.uint32).ctypes.data_as(u32p))
    assert want != 0
    assert tr(ctx, None, None, None) == want and offs(ctx, 1, 4, p) == want and series(ctx, ALL, 0, 4, 1, p, p) == want and matrix(ctx, 0xF, 1, 4, p) == want
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
    buf = np.zeros(s0.n_citizens, np.uint32)
    p = buf.ctypes.data_as(u32p)
    assert sim.lib.esim_transmission_tree(sim._ctx, p, None, None) == ESTATE and sim.lib.esim_offspring(sim._ctx, 1, 4, p) == ESTATE
    assert sim.lib.esim_reproduction_series(sim._ctx, _lib.BY_ALL, 0, 4, 1, p, p) == ESTATE
    sim.close()


def test_ensemble_gathers_the_members_reproduction_rows(tmp_path):
    pop, ep, n, ref = tree.cached("school")
    spec = dict(first_step=0, stride=24)
    ens = Ensemble(pop, ref_mod.copy_params(ep))
    members = [{"seed": int(ep.seed)}, {"seed": 8}, {"seed": 9, "exposure_chance": 0.02}]
    res = ens.run(members, 200, reproduction=spec)
    assert res.reproduction.shape == (3, 200 // 24 + 1, 2) and res.reproduction.dtype == np.uint32 and res.settings is None
    for i, m in enumerate(members):
        one = Simulator(pop, ref_mod.copy_params(ep, **m))
        one.run(200)
        cases, off = one.reproduction_series("all", **spec)
        same(res.reproduction[i, :, 0], cases[:, 0], "member %d vs the same run made singly: cases" % i)
        same(res.reproduction[i, :, 1], off[:, 0], "member %d vs the same run made singly: offspring" % i)
        one.close()
    assert ens.run(members[:1], 200).reproduction is None
    with pytest.raises(ValueError):
        ens.run(members[:1], 200, stop_when_done=True, reproduction=spec)
    fc = ens.forecast(100, [{"seed": 5}, {}], 200, reproduction=dict(n_rows=6))
    assert fc.reproduction.shape == (2, 6, 2)
    same(fc.reproduction[1, :, 0], res.reproduction[0, :6, 0], "the branch under the base parameters vs the straight run")
    same(fc.reproduction[0, :4, 0], fc.reproduction[1, :4, 0], "cohorts of the shared history")
    fc.dump(str(tmp_path))
    same(np.load(tmp_path / "ensemble_reproduction.npz")["reproduction"], fc.reproduction, "ensemble_reproduction.npz")
    ens.close()
