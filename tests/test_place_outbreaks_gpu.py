"""Work place and school outbreaks on the device (esim_place_outbreaks, esim_place_sizes, esim_place_sar) against the numpy
reference of tests/_place_ref.py, which reads who was still Susceptible from the states of the CPU oracle and the infectors from
the tree of tests/_tree_ref.py.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import _household_ref as hh
import _place_ref as pl
import _setting_ref as ref_mod
import _tree_ref as tree
from epidemicsimulator_amd import Population, Simulator, _lib
from epidemicsimulator_amd.ensemble import Ensemble
from test_place_outbreaks import situation, table_identities

pytestmark = pytest.mark.gpu

EINVAL, ESTATE, ERANGE = -1, -4, -5
u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
PER_PLACE = ("members", "cases", "introductions", "first_step")
KIND = {"work": _lib.PLACE_WORK, "room": _lib.PLACE_ROOM, "school": _lib.PLACE_SCHOOL}
LDS_GROUPS = 45                      # the largest n_groups whose two pair tables fit k_place_sar's LDS: 2 * 45 * 45 * 8 B <= 32 KB
GROUPS = (1, 5, LDS_GROUPS, LDS_GROUPS + 1)


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, "%s: shape %s, expected %s" % (what, got.shape, want.shape)
    bad = np.flatnonzero(got.ravel() != want.ravel())
    assert bad.size == 0, "%s: %d of %d differ, first at %d: got %s, expected %s" % (what, bad.size, got.size, bad[0], got.ravel()[bad[0]], want.ravel()[bad[0]])


def check_kind(sim, pop, n, kind, ob, pairs_of, windows, what):
    """ob: the reference's per-place arrays; pairs_of(first_step, last_step, n_groups) -> its (at_risk, secondary); n_groups 0:
    one cell."""
    what = "%s, %s" % (what, kind)
    got = sim.place_outbreaks(kind)
    for k in PER_PLACE:
        same(got[k], ob[k], "%s: %s per place" % (what, k))
    final_size, introduced = sim.place_sizes(kind)
    want = pl.sizes(ob)
    same(final_size, want[0], what + ": final sizes")
    same(introduced, want[1], what + ": introductions by size")
    table_identities(got, final_size, introduced)
    lib, ctx = sim.lib, sim._ctx
    # each output alone, and none
    one = np.zeros(len(ob["members"]), np.uint32)
    for i, k in enumerate(PER_PLACE):
        args = [None] * 4
        args[i] = one.ctypes.data_as(u32p)
        assert lib.esim_place_outbreaks(ctx, KIND[kind], *args) == 0
        same(one, ob[k], "%s: %s alone" % (what, k))
    assert lib.esim_place_outbreaks(ctx, KIND[kind], None, None, None, None) == 0
    tab = np.zeros((pl.BINS, pl.BINS), np.uint32)
    assert lib.esim_place_sizes(ctx, KIND[kind], tab.ctypes.data_as(u32p), None) == 0
    same(tab, want[0], what + ": final sizes alone")
    assert lib.esim_place_sizes(ctx, KIND[kind], None, tab.ctypes.data_as(u32p)) == 0
    same(tab, want[1], what + ": introductions alone")
    assert lib.esim_place_sizes(ctx, KIND[kind], None, None) == 0
    cell = np.zeros(1, np.uint64)
    if kind == "school":
        assert lib.esim_place_sar(ctx, KIND[kind], _lib.BY_ALL, 0, n, cell.ctypes.data_as(u64p), None) == EINVAL
        return
    for first, last in windows:
        at, sec = sim.place_sar(kind, "all", first, last, complete=False)
        w = pairs_of(first, last, 0)
        same(at, w[0], "%s: at risk, cohorts %d..%d" % (what, first, last))
        same(sec, w[1], "%s: secondary, cohorts %d..%d" % (what, first, last))
        assert (sec <= at).all()
    for g in GROUPS:
        sim.set_groups(hh.labels(pop, g), g)
        for first, last in windows if g == 5 else windows[:1]:
            at, sec = sim.place_sar(kind, "group", first, last, complete=False)
            w = pairs_of(first, last, g)
            assert at.shape == (g, g) and at.dtype == np.uint64
            same(at, w[0], "%s: at risk by %d groups, cohorts %d..%d" % (what, g, first, last))
            same(sec, w[1], "%s: secondary by %d groups, cohorts %d..%d" % (what, g, first, last))
    sim.set_groups(None)
    w = pairs_of(0, n, 0)
    assert lib.esim_place_sar(ctx, KIND[kind], _lib.BY_ALL, 0, n, cell.ctypes.data_as(u64p), None) == 0
    same(cell, w[0].ravel(), what + ": at risk alone")
    assert lib.esim_place_sar(ctx, KIND[kind], _lib.BY_ALL, 0, n, None, cell.ctypes.data_as(u64p)) == 0
    same(cell, w[1].ravel(), what + ": secondary alone")


def check_cached(sim, name, kind, what):
    pop, ep, n, ref, sus, _ = pl.cached(name)
    check_kind(sim, pop, n, kind, pl.cached_outbreaks(name, kind), lambda first, last, g: pl.cached_pairs(name, kind, first, last, g), pl.windows(name), what)


def started(name, level=None):
    pop, ep, n, ref, sus, _ = pl.cached(name)
    sim = Simulator(pop, ref_mod.copy_params(ep))
    if level is not None:
        sim.set_pipeline(level)
    sim.run(n)
    return sim


# ---- 1. every world against the reference ----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", pl.KINDS)
@pytest.mark.parametrize("name", ["edge", "school", "ties", "situations", "bus", "deep"])
def test_world(name, kind):
    situation(name)
    sim = started(name)
    check_cached(sim, name, kind, name)
    sim.close()


@pytest.mark.parametrize("level", [0, None])
def test_fixture_a(level):
    situation("fixture_a")
    pop, ep, n, ref, sus, _ = pl.cached("fixture_a")
    sim = started("fixture_a", level)
    before = (sim.download_state(), sim.records_so_far(), sim.exposure_events(), sim.area_census("home"))
    for kind in pl.KINDS:
        check_cached(sim, "fixture_a", kind, "fixture A, level %s" % level)
    after = (sim.download_state(), sim.records_so_far(), sim.exposure_events(), sim.area_census("home"))
    for key in before[0]:
        same(after[0][key], before[0][key], "state untouched: " + key)
    assert (after[1] == before[1]).all()
    for a, b in zip(after[2], before[2]):
        same(a, b, "exposure log untouched")
    same(after[3], before[3], "census untouched")
    sim.close()


def test_after_a_restart_and_other_index_cases():
    pop, ep, n, ref, sus, _ = pl.cached("fixture_a")
    sim = started("fixture_a")
    sim.restart()
    sim.run(n)
    check_cached(sim, "fixture_a", "work", "fixture A after esim_restart")
    # other index cases, from a list with a duplicate: three seeds in force
    s = pop.seeds
    seeds = (int(s[3]), int(s[0]), int(s[3]), int(s[7]))
    pop2, ep2, _, ref2, sus2, _ = hh.reseeded("fixture_a", seeds, n)
    world = (pop2, ep2, n, ref2, sus2)
    sim.restart(seeds=np.asarray(seeds, np.uint32))
    sim.run(n)
    busy = int(np.bincount(ref2["step"][ref2["step"] > 0]).argmax())
    windows = ((0, n), (max(1, n // 3), n // 2), (busy, busy))
    for kind in pl.KINDS:
        ob = pl.outbreaks(ref2, pop2, kind)
        assert int((ob["first_step"] == 0).sum()) <= 3 and int(ob["cases"].sum()) >= 50
        check_kind(sim, pop2, n, kind, ob, lambda first, last, g, kind=kind: pl.pairs_counting(world, kind, first, last, g), windows,
                   "fixture A after esim_restart_seeded with a duplicate in the list")
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
        sim.rollback(**over)
        sim.run(n - t)
        for kind in pl.KINDS:
            check_cached(sim, name, kind, what)
    # a rollback under another bus_capacity: the places need no bus replay, the pairs need the tree
    sim.rollback(bus_capacity=int(a.bus_capacity) + 5)
    sim.run(10)
    lib, ctx = sim.lib, sim._ctx
    cell = np.zeros(1, np.uint64)
    for kind in (_lib.PLACE_WORK, _lib.PLACE_ROOM):
        assert lib.esim_place_sar(ctx, kind, _lib.BY_ALL, 0, 5, cell.ctypes.data_as(u64p), None) == ESTATE
        assert b"two capacities" in lib.esim_last_error(ctx)
    for kind in KIND.values():
        assert lib.esim_place_outbreaks(ctx, kind, None, None, None, None) == 0 and lib.esim_place_sizes(ctx, kind, None, None) == 0
    # a history mixed twice
    sim.rollback()
    sim.run(20)
    sim.snapshot()
    sim.rollback(exposure_chance=b.exposure_chance)
    sim.run(20)
    sim.snapshot()
    sim.rollback(exposure_chance=0.005)
    sim.run(5)
    assert lib.esim_place_sar(ctx, _lib.PLACE_WORK, _lib.BY_ALL, 0, 5, cell.ctypes.data_as(u64p), None) == ESTATE
    assert lib.esim_place_outbreaks(ctx, _lib.PLACE_WORK, None, None, None, None) == ESTATE and lib.esim_place_sizes(ctx, _lib.PLACE_ROOM, None, None) == ESTATE
    sim.close()


# ---- 2. errors -------------------------------------------------------------------------------------------------------------
def test_error_table():
    pop, ep, n, ref, sus, _ = pl.cached("school")
    lib = _lib.load()
    buf32, buf64 = np.zeros(max(pop.n_buildings, pop.n_rooms, 2 * 32 * 32), np.uint32), np.zeros(64, np.uint64)
    p, q = buf32.ctypes.data_as(u32p), buf64.ctypes.data_as(u64p)
    outbreaks, sizes, sar = lib.esim_place_outbreaks, lib.esim_place_sizes, lib.esim_place_sar
    ALL, GROUP, WORK, ROOM, SCHOOL = _lib.BY_ALL, _lib.BY_GROUP, _lib.PLACE_WORK, _lib.PLACE_ROOM, _lib.PLACE_SCHOOL
    bare = C.c_void_p()
    _lib.check(lib.esim_create(C.byref(ep), C.byref(bare)))
    assert outbreaks(bare, WORK, p, p, p, p) == ESTATE and sizes(bare, ROOM, p, p) == ESTATE and sar(bare, WORK, ALL, 0, 0, q, q) == ESTATE     # before an upload
    assert sar(bare, WORK, ALL, 0, 0, None, None) == EINVAL and sar(bare, WORK, _lib.AREA_HOME, 0, 0, q, q) == EINVAL and sar(bare, SCHOOL, ALL, 0, 0, q, q) == EINVAL
    assert outbreaks(bare, 3, p, p, p, p) == EINVAL and sizes(bare, -1, p, p) == EINVAL
    lib.esim_destroy(bare)
    assert outbreaks(None, WORK, p, p, p, p) == EINVAL and sizes(None, WORK, p, p) == EINVAL and sar(None, WORK, ALL, 0, 0, q, q) == EINVAL
    sim = Simulator(pop, ref_mod.copy_params(ep))
    sim.run(10)
    ctx = sim._ctx
    assert sar(ctx, WORK, ALL, 0, 5, None, None) == EINVAL                                                       # both outputs NULL
    for where in (_lib.AREA_CURRENT, _lib.AREA_HOME, _lib.BY_SETTING, 7, -1):
        assert sar(ctx, ROOM, where, 0, 5, q, q) == EINVAL                                                       # unknown `where`
    for kind in (SCHOOL, 3, -1):
        assert sar(ctx, kind, ALL, 0, 5, q, q) == EINVAL                                                         # no pairs per school, unknown `kind`
    for kind in (3, 7, -1):
        assert outbreaks(ctx, kind, p, p, p, p) == EINVAL and sizes(ctx, kind, p, p) == EINVAL
    assert sar(ctx, WORK, GROUP, 0, 5, q, q) == ESTATE                                                           # by group without labels
    for kind in (WORK, ROOM):
        assert sar(ctx, kind, ALL, 5, 4, q, q) == ERANGE and sar(ctx, kind, ALL, 0, 11, q, q) == ERANGE and sar(ctx, kind, ALL, 11, 11, q, q) == ERANGE
        assert sar(ctx, kind, ALL, 0, 0, q, q) == 0 and sar(ctx, kind, ALL, 10, 10, q, q) == 0 and sar(ctx, kind, ALL, 0, 10, q, None) == 0
    with pytest.raises(_lib.EsimError):
        sim.place_sar(last_step=11, complete=False)
    with pytest.raises(ValueError):
        sim.place_sar()                                              # no cohort is complete after 10 steps
    sim.run(n - 10)                                                  # the context is usable afterwards
    done = n - int(ep.exposed_time) - 1 - int(ep.infected_time)
    assert 1 <= done < n
    for kind in ("work", "room"):
        w = pl.cached_pairs("school", kind, 0, done)
        at, sec = sim.place_sar(kind)                                # clipped to the last complete cohort
        same(at, w[0], kind + ", complete cohorts: at risk")
        same(sec, w[1], kind + ", complete cohorts: secondary")
        at, sec = sim.place_sar(kind, first_step=5, last_step=n)
        same(sec, pl.cached_pairs("school", kind, 5, done)[1], kind + ", complete cohorts from step 5 on: secondary")
    with pytest.raises(ValueError):
        sim.place_sar(first_step=done + 1)
    same(sim.place_outbreaks("room")["cases"], pl.cached_outbreaks("school", "room")["cases"], "after the refusals")
    # a sticky device-side error comes back as the calls underneath report it
    _lib.check(lib.esim_debug_inject_error(ctx, ERANGE), ctx)
    want = lib.esim_transmission_tree(ctx, None, None, None)
    assert want != 0
    assert outbreaks(ctx, WORK, p, p, p, p) == want and sizes(ctx, SCHOOL, p, p) == want and sar(ctx, ROOM, ALL, 0, 4, q, q) == want
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
    for kind in KIND.values():
        assert sim.lib.esim_place_outbreaks(sim._ctx, kind, None, None, None, None) == ESTATE and sim.lib.esim_place_sizes(sim._ctx, kind, None, None) == ESTATE
    assert sim.lib.esim_place_sar(sim._ctx, _lib.PLACE_WORK, _lib.BY_ALL, 0, 4, cell.ctypes.data_as(u64p), None) == ESTATE
    sim.close()


# ---- 3. the ensemble -------------------------------------------------------------------------------------------------------
def test_ensemble_gathers_the_members_places(tmp_path):
    pop, ep, _ = ref_mod.ties_world()
    n_steps, g = 120, 5
    done = n_steps - int(ep.exposed_time) - 1 - int(ep.infected_time)                  # the last complete cohort
    assert done >= 40
    lab = hh.labels(pop, g)
    ens = Ensemble(pop, ref_mod.copy_params(ep), group=(lab, g))
    members = ens.seeds(3, first=31)
    res = ens.places(members, n_steps)
    by_group = ens.places(members, n_steps, where="group", first_step=1, last_step=30)
    schools = ens.places(members, n_steps, kind="school")
    assert res.final_size.shape == res.introduced.shape == (3, 32, 32) and res.at_risk.shape == res.secondary.shape == (3, 1, 1)
    assert by_group.at_risk.shape == (3, g, g) and by_group.at_risk.dtype == np.uint64
    assert int(schools.final_size.sum()) == 0 and int(schools.at_risk.sum()) == 0      # (this world has no school)
    for i, m in enumerate(members):
        ep_i = ref_mod.copy_params(ep, seed=m["seed"])
        ref = tree.reference(pop, ep_i, n_steps, ref_mod.reference(pop, ep_i, n_steps))
        world = (pop, ep_i, n_steps, ref, hh.sus_until(pop, ep_i, n_steps))
        want = pl.sizes(pl.outbreaks(ref, pop, "work"))
        same(res.final_size[i], want[0], "member %d: final sizes" % i)
        same(res.introduced[i], want[1], "member %d: introductions" % i)
        at, sec = pl.pairs_counting(world, "work", 0, done)
        same(res.at_risk[i], at, "member %d: at risk" % i)
        same(res.secondary[i], sec, "member %d: secondary" % i)
        at, sec = pl.pairs_counting(world, "work", 1, 30, g)
        same(by_group.at_risk[i], at, "member %d: at risk by group" % i)
        same(by_group.secondary[i], sec, "member %d: secondary by group" % i)
    assert int(res.secondary.sum()) >= 30
    sar = res.sar()
    assert sar.shape == (1, 1) and sar[0, 0] == float(res.secondary.sum()) / float(res.at_risk.sum())
    assert res.attack_rate_by_size().shape == (32,)
    res.dump(str(tmp_path))
    same(np.load(tmp_path / "ensemble_places.npz")["at_risk"], res.at_risk, "ensemble_places.npz")
    ens.close()
