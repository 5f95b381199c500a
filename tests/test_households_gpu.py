"""Household outbreaks on the device (esim_household_outbreaks, esim_household_final_sizes, esim_household_sar) against the numpy
reference of tests/_household_ref.py, which reads who was still Susceptible from the states of the CPU oracle and the infectors
from the tree of tests/_tree_ref.py.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import _chain_ref as chain
import _household_ref as hh
import _setting_ref as ref_mod
import _tree_ref as tree
from epidemicsimulator_amd import Population, Simulator, _lib
from epidemicsimulator_amd.ensemble import Ensemble
from test_households import situation, table_identities

pytestmark = pytest.mark.gpu

EINVAL, ESTATE, ERANGE = -1, -4, -5
u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
PER_HOUSEHOLD = ("cases", "introductions", "first_step")
LDS_GROUPS = 45                      # the largest n_groups whose two pair tables fit k_hh_sar's LDS: 2 * 45 * 45 * 8 B <= 32 KB
GROUPS = (1, 5, LDS_GROUPS, LDS_GROUPS + 1)


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, "%s: shape %s, expected %s" % (what, got.shape, want.shape)
    bad = np.flatnonzero(got.ravel() != want.ravel())
    assert bad.size == 0, "%s: %d of %d differ, first at %d: got %s, expected %s" % (what, bad.size, got.size, bad[0], got.ravel()[bad[0]], want.ravel()[bad[0]])


def check_all(sim, pop, n, ref, house, pairs_of, what):
    """pairs_of(first_step, last_step, n_groups) -> the reference's (at_risk, secondary, ...); n_groups 0: one cell."""
    got = sim.household_outbreaks()
    for k in PER_HOUSEHOLD:
        same(got[k], house[k], "%s: %s per household" % (what, k))
    final_size, intro_size = sim.household_final_sizes()
    want = hh.final_sizes(house)
    same(final_size, want[0], what + ": final sizes")
    same(intro_size, want[1], what + ": introductions by household size")
    table_identities(dict(got, size=house["size"]), final_size, intro_size)
    busy = int(np.bincount(ref["step"][ref["step"] > 0]).argmax())                     # the cohort step with the most cases
    windows = ((0, n), (max(1, n // 3), n // 2), (busy, busy))
    for first, last in windows:
        at, sec = sim.household_sar("all", first, last, complete=False)
        w = pairs_of(first, last, 0)
        same(at, w[0], "%s: at risk, cohorts %d..%d" % (what, first, last))
        same(sec, w[1], "%s: secondary, cohorts %d..%d" % (what, first, last))
        assert (sec <= at).all()
    for g in GROUPS:
        sim.set_groups(hh.labels(pop, g), g)
        for first, last in windows if g == 5 else windows[:1]:
            at, sec = sim.household_sar("group", first, last, complete=False)
            w = pairs_of(first, last, g)
            assert at.shape == (g, g) and at.dtype == np.uint64
            same(at, w[0], "%s: at risk by %d groups, cohorts %d..%d" % (what, g, first, last))
            same(sec, w[1], "%s: secondary by %d groups, cohorts %d..%d" % (what, g, first, last))
    sim.set_groups(None)
    # each output alone, and none
    lib, ctx = sim.lib, sim._ctx
    one = np.zeros(pop.n_buildings, np.uint32)
    for i, k in enumerate(PER_HOUSEHOLD):
        args = [None, None, None]
        args[i] = one.ctypes.data_as(u32p)
        assert lib.esim_household_outbreaks(ctx, *args) == 0
        same(one, house[k], "%s: %s alone" % (what, k))
    assert lib.esim_household_outbreaks(ctx, None, None, None) == 0
    tab = np.zeros((hh.BINS, hh.BINS), np.uint32)
    assert lib.esim_household_final_sizes(ctx, tab.ctypes.data_as(u32p), None) == 0
    same(tab, want[0], what + ": final sizes alone")
    assert lib.esim_household_final_sizes(ctx, None, tab.ctypes.data_as(u32p)) == 0
    same(tab, want[1], what + ": introductions alone")
    assert lib.esim_household_final_sizes(ctx, None, None) == 0
    cell, w = np.zeros(1, np.uint64), pairs_of(0, n, 0)
    assert lib.esim_household_sar(ctx, _lib.BY_ALL, 0, n, cell.ctypes.data_as(u64p), None) == 0
    same(cell, w[0].ravel(), what + ": at risk alone")
    assert lib.esim_household_sar(ctx, _lib.BY_ALL, 0, n, None, cell.ctypes.data_as(u64p)) == 0
    same(cell, w[1].ravel(), what + ": secondary alone")


def cached_pairs_of(name):
    return lambda first, last, g: hh.cached_pairs(name, first, last, g)


def started(name, level=None):
    pop, ep, n, ref, sus, house = hh.cached(name)
    sim = Simulator(pop, ref_mod.copy_params(ep))
    if level is not None:
        sim.set_pipeline(level)
    sim.run(n)
    return sim, pop, ep, n, ref, house


# ---- 1. every world against the reference ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["permuted", "ties", "as_u8", "school", "situations", "bus", "deep"])
def test_world(name):
    situation(name)
    sim, pop, ep, n, ref, house = started(name)
    check_all(sim, pop, n, ref, house, cached_pairs_of(name), name)
    sim.close()


@pytest.mark.parametrize("level", [0, None])
def test_fixture_a(level):
    situation("fixture_a")
    sim, pop, ep, n, ref, house = started("fixture_a", level)
    before = (sim.download_state(), sim.records_so_far(), sim.exposure_events(), sim.area_census("home"))
    check_all(sim, pop, n, ref, house, cached_pairs_of("fixture_a"), "fixture A, level %s" % level)
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
        check_all(sim, pop, n, ref, house, cached_pairs_of("fixture_a"), "fixture A after esim_restart")
        # other index cases, from a list with a duplicate: three seeds in force
        s = pop.seeds
        seeds = (int(s[3]), int(s[0]), int(s[3]), int(s[7]))
        pop2, ep2, _, ref2, sus2, house2 = hh.reseeded("fixture_a", seeds, n)
        assert int((house2["first_step"] == 0).sum()) == 3 and int(house2["cases"].sum()) >= 100
        sim.restart(seeds=np.asarray(seeds, np.uint32))
        sim.run(n)

        def pairs_of(first, last, g):
            return hh.pairs(ref2, pop2, ep2, sus2, first, last, hh.labels(pop2, g) if g else None, max(1, g), jm=house2["jm"])
        check_all(sim, pop2, n, ref2, house2, pairs_of, "fixture A after esim_restart_seeded with a duplicate in the list")
    sim.close()


def test_rollback_under_another_seed_and_exposure_chance():
    pop, a, t, b, n = ref_mod.rollback_world()
    sim = Simulator(pop, ref_mod.copy_params(a))
    sim.run(t)
    sim.snapshot()
    sim.run(60)                                                      # a future that the rollback abandons
    for name, over, what in (("rollback", dict(seed=int(b.seed), exposure_chance=b.exposure_chance), "branch under another seed and chance"),
                             ("rollback_chance", dict(exposure_chance=b.exposure_chance), "branch under another chance"),
                             ("rollback_straight", {}, "branch under the snapshot's own values")):
        _, _, _, ref, _, house = hh.cached(name)
        sim.rollback(**over)
        sim.run(n - t)
        check_all(sim, pop, n, ref, house, cached_pairs_of(name), what)
    # a rollback under another bus_capacity: the households need no bus replay, the pairs need the tree
    sim.rollback(bus_capacity=int(a.bus_capacity) + 5)
    sim.run(10)
    lib, ctx = sim.lib, sim._ctx
    cell = np.zeros(1, np.uint64)
    assert lib.esim_household_sar(ctx, _lib.BY_ALL, 0, 5, cell.ctypes.data_as(u64p), None) == ESTATE
    assert b"two capacities" in lib.esim_last_error(ctx)
    assert lib.esim_household_outbreaks(ctx, None, None, None) == 0 and lib.esim_household_final_sizes(ctx, None, None) == 0
    # a history mixed twice
    sim.rollback()
    sim.run(20)
    sim.snapshot()
    sim.rollback(exposure_chance=b.exposure_chance)
    sim.run(20)
    sim.snapshot()
    sim.rollback(exposure_chance=0.005)
    sim.run(5)
    assert lib.esim_household_sar(ctx, _lib.BY_ALL, 0, 5, cell.ctypes.data_as(u64p), None) == ESTATE
    assert lib.esim_household_outbreaks(ctx, None, None, None) == ESTATE and lib.esim_household_final_sizes(ctx, None, None) == ESTATE
    sim.close()


# ---- 2. errors -------------------------------------------------------------------------------------------------------------
def test_error_table():
    pop, ep, n, ref, sus, house = hh.cached("school")
    lib = _lib.load()
    buf32, buf64 = np.zeros(max(pop.n_buildings, 2 * 64 * 64), np.uint32), np.zeros(64, np.uint64)
    p, q = buf32.ctypes.data_as(u32p), buf64.ctypes.data_as(u64p)
    outbreaks, sizes, sar = lib.esim_household_outbreaks, lib.esim_household_final_sizes, lib.esim_household_sar
    ALL, GROUP = _lib.BY_ALL, _lib.BY_GROUP
    bare = C.c_void_p()
    _lib.check(lib.esim_create(C.byref(ep), C.byref(bare)))
    assert outbreaks(bare, p, p, p) == ESTATE and sizes(bare, p, p) == ESTATE and sar(bare, ALL, 0, 0, q, q) == ESTATE     # before an upload
    assert sar(bare, ALL, 0, 0, None, None) == EINVAL and sar(bare, _lib.AREA_HOME, 0, 0, q, q) == EINVAL
    lib.esim_destroy(bare)
    assert outbreaks(None, p, p, p) == EINVAL and sizes(None, p, p) == EINVAL and sar(None, ALL, 0, 0, q, q) == EINVAL
    sim = Simulator(pop, ref_mod.copy_params(ep))
    sim.run(10)
    ctx = sim._ctx
    assert sar(ctx, ALL, 0, 5, None, None) == EINVAL                                                             # both outputs NULL
    for where in (_lib.AREA_CURRENT, _lib.AREA_HOME, _lib.BY_SETTING, 7, -1):
        assert sar(ctx, where, 0, 5, q, q) == EINVAL                                                             # unknown `where`
    assert sar(ctx, GROUP, 0, 5, q, q) == ESTATE                                                                 # by group without labels
    assert sar(ctx, ALL, 5, 4, q, q) == ERANGE and sar(ctx, ALL, 0, 11, q, q) == ERANGE and sar(ctx, ALL, 11, 11, q, q) == ERANGE
    assert sar(ctx, ALL, 0, 0, q, q) == 0 and sar(ctx, ALL, 10, 10, q, q) == 0 and sar(ctx, ALL, 0, 10, q, None) == 0
    with pytest.raises(_lib.EsimError):
        sim.household_sar(last_step=11, complete=False)
    with pytest.raises(ValueError):
        sim.household_sar()                                          # no cohort is complete after 10 steps
    sim.run(n - 10)                                                  # the context is usable afterwards
    done = n - int(ep.exposed_time) - 1 - int(ep.infected_time)
    assert 1 <= done < n
    w = hh.cached_pairs("school", 0, done)
    at, sec = sim.household_sar()                                    # clipped to the last complete cohort
    same(at, w[0], "complete cohorts: at risk")
    same(sec, w[1], "complete cohorts: secondary")
    at, sec = sim.household_sar(first_step=5, last_step=n)
    same(sec, hh.cached_pairs("school", 5, done)[1], "complete cohorts from step 5 on: secondary")
    with pytest.raises(ValueError):
        sim.household_sar(first_step=done + 1)
    same(sim.household_outbreaks()["cases"], house["cases"], "after the refusals")
    # a sticky device-side error comes back as the calls underneath report it
    _lib.check(lib.esim_debug_inject_error(ctx, ERANGE), ctx)
    want = lib.esim_transmission_tree(ctx, None, None, None)
    assert want != 0
    assert outbreaks(ctx, p, p, p) == want and sizes(ctx, p, p) == want and sar(ctx, ALL, 0, 4, q, q) == want
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
    cell = np.zeros(1, np.uint64)
    assert sim.lib.esim_household_outbreaks(sim._ctx, None, None, None) == ESTATE and sim.lib.esim_household_final_sizes(sim._ctx, None, None) == ESTATE
    assert sim.lib.esim_household_sar(sim._ctx, _lib.BY_ALL, 0, 4, cell.ctypes.data_as(u64p), None) == ESTATE
    sim.close()


# ---- 3. the ensemble -------------------------------------------------------------------------------------------------------
def test_ensemble_gathers_the_members_households(tmp_path):
    pop, ep, _ = ref_mod.ties_world()
    n_steps, g = 120, 5
    done = n_steps - int(ep.exposed_time) - 1 - int(ep.infected_time)                  # the last complete cohort
    assert done >= 40
    lab = hh.labels(pop, g)
    ens = Ensemble(pop, ref_mod.copy_params(ep), group=(lab, g))
    members = ens.seeds(3, first=31)
    res = ens.households(members, n_steps)
    by_group = ens.households(members, n_steps, where="group", first_step=1, last_step=30)
    assert res.final_size.shape == res.introductions.shape == (3, 64, 64) and res.at_risk.shape == res.secondary.shape == (3, 1, 1)
    assert by_group.at_risk.shape == (3, g, g) and by_group.at_risk.dtype == np.uint64
    for i, m in enumerate(members):
        ep_i = ref_mod.copy_params(ep, seed=m["seed"])
        ref = tree.reference(pop, ep_i, n_steps, ref_mod.reference(pop, ep_i, n_steps))
        sus, house = hh.sus_until(pop, ep_i, n_steps), hh.households(ref, pop)
        want = hh.final_sizes(house)
        same(res.final_size[i], want[0], "member %d: final sizes" % i)
        same(res.introductions[i], want[1], "member %d: introductions" % i)
        at, sec, _ = hh.pairs(ref, pop, ep_i, sus, 0, done)
        same(res.at_risk[i], at, "member %d: at risk" % i)
        same(res.secondary[i], sec, "member %d: secondary" % i)
        at, sec, _ = hh.pairs(ref, pop, ep_i, sus, 1, 30, lab, g)
        same(by_group.at_risk[i], at, "member %d: at risk by group" % i)
        same(by_group.secondary[i], sec, "member %d: secondary by group" % i)
    assert int(res.secondary.sum()) >= 100
    sar = res.sar()
    assert sar.shape == (1, 1) and sar[0, 0] == float(res.secondary.sum()) / float(res.at_risk.sum())
    res.dump(str(tmp_path))
    same(np.load(tmp_path / "ensemble_households.npz")["at_risk"], res.at_risk, "ensemble_households.npz")
    ens.close()
