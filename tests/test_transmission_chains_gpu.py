"""Transmission chains on the device (esim_transmission_chains, esim_outbreaks, esim_transmission_ages) against the numpy
reference of tests/_chain_ref.py, which walks the tree of tests/_tree_ref.py built on the CPU oracle.  Every comparison is
exact."""
import ctypes as C

import numpy as np
import pytest

import _chain_ref as chain
import _setting_ref as ref_mod
import _tree_ref as tree
from epidemicsimulator_amd import Population, Simulator, _lib
from epidemicsimulator_amd.ensemble import Ensemble
from test_transmission_chains import identities, situation

pytestmark = pytest.mark.gpu

EINVAL, ESTATE, ERANGE = -1, -4, -5
u32p = C.POINTER(C.c_uint32)
TABLE = ("size", "depth", "last_step")


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, "%s: shape %s, expected %s" % (what, got.shape, want.shape)
    bad = np.flatnonzero(got.ravel() != want.ravel())
    assert bad.size == 0, "%s: %d of %d differ, first at %d: got %s, expected %s" % (what, bad.size, got.size, bad[0], got.ravel()[bad[0]], want.ravel()[bad[0]])


def check_all(sim, pop, ep, ref, ch, n, what):
    lineage, desc = sim.transmission_chains()
    same(lineage, ch["lineage"], what + ": lineage per citizen")
    same(desc, ch["descendants"], what + ": descendants per citizen")
    table = sim.outbreaks()
    same(table["seeds"], ch["seeds"], what + ": the index cases in force")
    for k in TABLE:
        same(table[k], ch[k], "%s: %s per index case" % (what, k))
    same(sim.transmission_ages(), chain.ages(ref, pop, ep), what + ": ages over the whole run")
    busy = int(np.bincount(ref["step"][ref["step"] > 0]).argmax())                     # the step with the most exposures
    for first, last in ((max(1, n // 3), n // 2), (busy, busy)):
        same(sim.transmission_ages(first, last), chain.ages(ref, pop, ep, first, last), "%s: ages of steps %d..%d" % (what, first, last))
    # either output alone, and none
    lib, ctx = sim.lib, sim._ctx
    one = np.zeros(pop.n_citizens, np.uint32)
    assert lib.esim_transmission_chains(ctx, None, one.ctypes.data_as(u32p)) == 0
    same(one, ch["descendants"], what + ": descendants alone")
    assert lib.esim_transmission_chains(ctx, one.ctypes.data_as(u32p), None) == 0
    same(one, ch["lineage"], what + ": lineage alone")
    assert lib.esim_transmission_chains(ctx, None, None) == 0


def started(name, level=None):
    pop, ep, n, ref, ch = chain.cached(name)
    sim = Simulator(pop, ref_mod.copy_params(ep))
    if level is not None:
        sim.set_pipeline(level)
    sim.run(n)
    return sim, pop, ep, n, ref, ch


# ---- 1. every world against the reference ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["permuted", "ties", "as_u8", "school", "situations", "bus", "deep"])
def test_world(name):
    situation(name)
    sim, pop, ep, n, ref, ch = started(name)
    check_all(sim, pop, ep, ref, ch, n, name)
    sim.close()


@pytest.mark.parametrize("level", [0, None])
def test_fixture_a(level):
    situation("fixture_a")
    sim, pop, ep, n, ref, ch = started("fixture_a", level)
    before = (sim.download_state(), sim.records_so_far(), sim.exposure_events(), sim.area_census("home"))
    check_all(sim, pop, ep, ref, ch, n, "fixture A, level %s" % level)
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
        check_all(sim, pop, ep, ref, ch, n, "fixture A after esim_restart")
        # other index cases: a list with a duplicate (three seeds in force, the ordinals those of the first occurrences), a list of one
        s = pop.seeds
        for seeds in ((int(s[3]), int(s[0]), int(s[3]), int(s[7])), (int(s[5]),)):
            pop2, _, _, ref2, ch2 = chain.reseeded("fixture_a", seeds, n)
            assert len(ch2["seeds"]) == len(set(seeds)) and int(ch2["size"].sum()) >= 100
            sim.restart(seeds=np.asarray(seeds, np.uint32))
            sim.run(n)
            check_all(sim, pop2, ep, ref2, ch2, n, "fixture A after esim_restart_seeded with %d index cases" % len(seeds))
        sim.restart(seeds=pop.seeds)
        sim.run(n)
        check_all(sim, pop, ep, ref, ch, n, "fixture A after esim_restart_seeded with its own index cases")
    sim.close()


def test_rollback_under_another_seed_and_exposure_chance():
    pop, a, t, b, n = ref_mod.rollback_world()
    (ref_b, ch_b), (ref_c, ch_c), (ref_a, ch_a) = (chain.cached(k)[3:] for k in ("rollback", "rollback_chance", "rollback_straight"))
    sim = Simulator(pop, ref_mod.copy_params(a))
    sim.run(t)
    sim.snapshot()
    sim.run(60)                                                      # a future that the rollback abandons
    sim.rollback(seed=int(b.seed), exposure_chance=b.exposure_chance)
    sim.run(n - t)
    check_all(sim, pop, a, ref_b, ch_b, n, "branch under another seed and chance")
    sim.rollback(exposure_chance=b.exposure_chance)
    sim.run(n - t)
    check_all(sim, pop, a, ref_c, ch_c, n, "branch under another chance")
    sim.rollback()
    sim.run(n - t)
    check_all(sim, pop, a, ref_a, ch_a, n, "branch under the snapshot's own values")
    # a rollback under another bus_capacity: two capacities in one history are not replayed
    sim.rollback(bus_capacity=int(a.bus_capacity) + 5)
    sim.run(10)
    lib, ctx = sim.lib, sim._ctx
    buf = np.zeros(max(pop.n_citizens, 4 * 512), np.uint32)
    p, n_out = buf.ctypes.data_as(u32p), C.c_uint32(0)
    assert lib.esim_transmission_chains(ctx, None, None) == ESTATE and lib.esim_transmission_ages(ctx, 1, 1, p) == ESTATE
    assert lib.esim_outbreaks(ctx, p, None, None, 64, C.byref(n_out)) == ESTATE
    assert b"two capacities" in lib.esim_last_error(ctx)
    sim.rollback()                                                   # (back under the snapshot's capacity: one history again)
    sim.run(n - t)
    check_all(sim, pop, a, ref_a, ch_a, n, "after the branch under another capacity was abandoned")
    # a history mixed twice
    sim.snapshot()
    sim.rollback(exposure_chance=b.exposure_chance)
    sim.run(20)
    sim.snapshot()
    sim.rollback(exposure_chance=0.005)
    sim.run(5)
    assert lib.esim_transmission_chains(ctx, None, None) == ESTATE and lib.esim_transmission_ages(ctx, 1, 1, p) == ESTATE
    assert lib.esim_outbreaks(ctx, p, None, None, 64, C.byref(n_out)) == ESTATE
    sim.close()


# ---- 2. identities without an oracle ---------------------------------------------------------------------------------------
def test_york_5000_steps_identities():
    pop = Population.synthetic("york")
    ep = _lib.default_params(max_steps=5600)
    sim = Simulator(pop, ep)
    n = 5000
    rec = sim.run(n)
    assert len(rec) == n
    total = int(rec["exposures_building"].sum()) + int(rec["exposures_bus"].sum())
    infector, k, gen = sim.transmission_tree()
    cit, step, bus = sim.exposure_events()
    te = np.zeros(pop.n_citizens, np.uint32)
    te[cit[step >= 1]] = step[step >= 1]
    lineage, desc = sim.transmission_chains()
    table = sim.outbreaks()
    ages = sim.transmission_ages()
    print("york: %d exposures from %d index cases, sizes %s, depths %s, last steps %s, ages %d..%d" %
          (total, len(table["seeds"]), table["size"].tolist(), table["depth"].tolist(), table["last_step"].tolist(),
           np.flatnonzero(ages.sum(axis=0)).min(), np.flatnonzero(ages.sum(axis=0)).max()))
    assert total >= 1000
    identities(pop, ep, n, infector, gen, te, total, dict(table, lineage=lineage, descendants=desc), ages, sim.setting_series("setting", stride=n, n_rows=1)[0])
    # an outbreak is over once the last Infected step of its last case has run: its size does not change afterwards
    over = table["last_step"].astype(np.int64) + int(ep.exposed_time) + 1 + int(ep.infected_time) < n
    assert over.any()
    sim.run(500)
    later = sim.outbreaks()
    same(later["seeds"], table["seeds"], "the index cases after 500 more steps")
    same(later["size"][over], table["size"][over], "finished outbreaks: size after 500 more steps")
    assert (later["size"] >= table["size"]).all()
    sim.close()


# ---- 3. errors -------------------------------------------------------------------------------------------------------------
def test_error_table():
    pop, ep, n, ref, ch = chain.cached("school")
    lib = _lib.load()
    buf = np.zeros(max(pop.n_citizens, 4 * 512), np.uint32)
    p, n_out = buf.ctypes.data_as(u32p), C.c_uint32(0)
    chains, outbreaks, ages = lib.esim_transmission_chains, lib.esim_outbreaks, lib.esim_transmission_ages
    bare = C.c_void_p()
    _lib.check(lib.esim_create(C.byref(ep), C.byref(bare)))
    assert chains(bare, p, p) == ESTATE and outbreaks(bare, p, p, p, 64, C.byref(n_out)) == ESTATE and ages(bare, 1, 1, p) == ESTATE   # before an upload
    assert outbreaks(bare, p, p, p, 64, None) == EINVAL and ages(bare, 1, 1, None) == EINVAL
    lib.esim_destroy(bare)
    assert chains(None, p, p) == EINVAL and outbreaks(None, p, p, p, 64, C.byref(n_out)) == EINVAL and ages(None, 1, 1, p) == EINVAL
    sim = Simulator(pop, ref_mod.copy_params(ep))
    sim.run(10)
    ctx = sim._ctx
    n_seeds = len(ch["seeds"])
    assert ages(ctx, 1, 1, None) == EINVAL and outbreaks(ctx, p, p, p, 64, None) == EINVAL                      # null pointers
    n_out.value = 0
    assert outbreaks(ctx, p, p, p, n_seeds - 1, C.byref(n_out)) == ERANGE and n_out.value == n_seeds            # cap too small, *n_out set
    n_out.value = 0
    assert outbreaks(ctx, None, None, None, 0, C.byref(n_out)) == ERANGE and n_out.value == n_seeds
    assert ages(ctx, 0, 5, p) == ERANGE and ages(ctx, 5, 4, p) == ERANGE and ages(ctx, 5, 11, p) == ERANGE and ages(ctx, 11, 11, p) == ERANGE
    # after the refusals: any output of the table may be NULL, the audits alone run
    n_out.value = 0
    assert outbreaks(ctx, None, None, None, n_seeds, C.byref(n_out)) == 0 and n_out.value == n_seeds
    assert outbreaks(ctx, None, p, None, n_seeds, C.byref(n_out)) == 0 and ages(ctx, 10, 10, p) == 0 and chains(ctx, None, None) == 0
    with pytest.raises(_lib.EsimError):
        sim.transmission_ages(1, 11)
    with pytest.raises(_lib.EsimError):
        sim.transmission_ages(0)
    sim.run(n - 10)                                                                                             # the context is usable afterwards
    same(sim.transmission_chains()[0], ch["lineage"], "after the refusals")
    same(sim.outbreaks()["size"], ch["size"], "after the refusals")
    # a sticky device-side error comes back as the tree calls report it
    _lib.check(lib.esim_debug_inject_error(ctx, ERANGE), ctx)
    want = lib.esim_transmission_tree(ctx, None, None, None)
    assert want != 0
    assert chains(ctx, p, None) == want and outbreaks(ctx, p, p, p, 64, C.byref(n_out)) == want and ages(ctx, 1, 4, p) == want
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
    buf = np.zeros(max(s0.n_citizens, 4 * 512), np.uint32)
    p, n_out = buf.ctypes.data_as(u32p), C.c_uint32(0)
    assert sim.lib.esim_transmission_chains(sim._ctx, p, None) == ESTATE and sim.lib.esim_transmission_ages(sim._ctx, 1, 4, p) == ESTATE
    assert sim.lib.esim_outbreaks(sim._ctx, p, None, None, 64, C.byref(n_out)) == ESTATE
    sim.close()


# ---- 4. the ensemble -------------------------------------------------------------------------------------------------------
def test_ensemble_gathers_the_members_outbreaks(tmp_path):
    pop, ep, n, ref, ch = chain.cached("school")
    ens = Ensemble(pop, ref_mod.copy_params(ep))
    members = ens.index_cases(3, n=4)
    n_steps = 200
    res = ens.outbreaks(members, n_steps, ages=True)
    width = max(len(s) for s in res.seeds)
    assert res.size.shape == res.depth.shape == res.last_step.shape == (3, width) and res.size.dtype == np.int64
    assert res.ages.shape == (3, _lib.N_SETTINGS, _lib.AGE_BINS) and res.ages.dtype == np.uint32
    for i, m in enumerate(members):
        one = Simulator(pop, ref_mod.copy_params(ep, seed=m["seed"]))
        one.restart(seeds=np.asarray(m["index_cases"], np.uint32))
        one.run(n_steps)
        table = one.outbreaks()
        k = len(table["seeds"])
        assert k == len(set(m["index_cases"]))
        same(res.seeds[i], table["seeds"], "member %d vs the same run made singly: seeds" % i)
        for key in TABLE:
            same(getattr(res, key)[i, :k], table[key].astype(np.int64), "member %d vs the same run made singly: %s" % (i, key))
            assert (getattr(res, key)[i, k:] == -1).all()
        same(res.ages[i], one.transmission_ages(), "member %d vs the same run made singly: ages" % i)
        one.close()
    assert int(res.size.clip(min=0).sum()) >= 100 and res.extinct().shape == res.size.shape
    assert ens.outbreaks(members[:1], n_steps).ages is None
    # run() starts its members as before: the population's own index cases are back in force for a member without any
    back = ens.run([{"seed": int(ep.seed)}], n)
    assert int(back.records["exposures_building"][0].sum()) + int(back.records["exposures_bus"][0].sum()) == int((ref["step"] > 0).sum())
    res.dump(str(tmp_path))
    same(np.load(tmp_path / "ensemble_outbreaks.npz")["size"], res.size, "ensemble_outbreaks.npz")
    ens.close()
