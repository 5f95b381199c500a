"""Contact-hours at risk on the device (esim_contact_hours) against the rule of tests/_contact_ref.py, which tests/test_contact_hours.py
checks against what the CPU oracle's states show.  Every comparison is exact."""
import ctypes as C
import functools

import numpy as np
import pytest

import _contact_ref as ref
import _household_ref as hh
import _setting_ref as ref_mod
from epidemicsimulator_amd import Population, Simulator, _lib
from epidemicsimulator_amd.ensemble import Ensemble

pytestmark = pytest.mark.gpu

EINVAL, ESTATE, ERANGE = -1, -4, -5
u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
LDS_GROUPS = 32                      # the largest n_groups whose four planes fit the kernels' LDS: 4 * 32 * 32 * 8 B <= 32 KB
MASKS = (0xF, 1, 2, 4, 8, 0b1001)


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, "%s: shape %s, expected %s" % (what, got.shape, want.shape)
    bad = np.flatnonzero(got.ravel() != want.ravel())
    assert bad.size == 0, "%s: %d of %d differ, first at %d: got %s, expected %s" % (what, bad.size, got.size, bad[0], got.ravel()[bad[0]], want.ravel()[bad[0]])


def settings_of(mask):
    return [s for s in range(4) if (mask >> s) & 1]


def check_all(sim, pop, n, tr, rule_of, what, groups=(1, 5)):
    """rule_of(g) -> the rule's Tables by g groups (labels: _contact_ref.labels_of)."""
    busy = int(np.bincount(tr["step"][tr["step"] > 0]).argmax())                     # the step with the most exposures
    windows = ((1, n), (max(1, n // 3), n // 2), (busy, busy))
    for g in groups:
        tab, lab = rule_of(g), ref.labels_of(pop, g)
        where = "all" if g == 1 else "group"
        if g > 1:
            sim.set_groups(lab, g)
        for first, last in windows:
            for mask in MASKS if g <= 5 else MASKS[:1]:
                got = sim.contact_hours(where, settings_of(mask), first, last)
                label = "%s: by %d, steps %d..%d, mask %x" % (what, g, first, last, mask)
                assert got["hours"].shape == (4, g, g) and got["hours"].dtype == np.uint64
                same(got["hours"], tab.window(first, last, mask), label + ": hours")
                same(got["transmissions"], ref.transmissions(tr, lab, g, first, last, mask), label + ": transmissions")
                assert (got["transmissions"] <= got["hours"]).all()
            if g > 5:
                break
    sim.set_groups(None)
    # per case, and each output alone, and none
    one = rule_of(1)
    first, last = windows[1]
    same(sim.contact_hours(per_case=True)["per_case"], one.per_case(), what + ": per case")
    same(sim.contact_hours("all", (0, 3), first, last, per_case=True)["per_case"], one.per_case(first, last, 0b1001), what + ": per case, households and transport, a middle window")
    lib, ctx = sim.lib, sim._ctx
    cell, cases = np.zeros(4, np.uint64), np.zeros(pop.n_citizens, np.uint32)
    assert lib.esim_contact_hours(ctx, _lib.BY_ALL, 0xF, 1, n, cell.ctypes.data_as(u64p), None, None) == 0
    same(cell, one.window().ravel(), what + ": hours alone")
    assert lib.esim_contact_hours(ctx, _lib.BY_ALL, 0xF, 1, n, None, cell.ctypes.data_as(u64p), None) == 0
    same(cell, ref.transmissions(tr, ref.labels_of(pop, 1), 1).ravel(), what + ": transmissions alone")
    assert lib.esim_contact_hours(ctx, _lib.BY_ALL, 0xF, 1, n, None, None, cases.ctypes.data_as(u32p)) == 0
    same(cases, one.per_case(), what + ": per case alone")
    assert lib.esim_contact_hours(ctx, _lib.BY_ALL, 0xF, 1, n, None, None, None) == 0


def cached_rule_of(name):
    return lambda g: ref.cached_rule(name, g)


def started(name, level=None):
    pop, ep, n, tr = ref.base(name)
    sim = Simulator(pop, ref_mod.copy_params(ep))
    if level is not None:
        sim.set_pipeline(level)
    sim.run(n)
    return sim, pop, ep, n, tr


# ---- 1. every world against the rule ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["permuted", "ties", "as_u8", "school", "situations", "bus", "deep", "edge"])
def test_world(name):
    sim, pop, ep, n, tr = started(name)
    # (school and bus: also the largest group count that takes the LDS form, and the first that does not)
    check_all(sim, pop, n, tr, cached_rule_of(name), name, (1, 5, LDS_GROUPS, LDS_GROUPS + 1) if name in ("school", "bus") else (1, 5))
    sim.close()


@functools.lru_cache(maxsize=None)
def reseeded(seeds, n):
    pop, ep, _, tr, _ = __import__("_chain_ref").reseeded("fixture_a", seeds, n)
    return pop, ep, tr, {g: ref.member_rule(pop, ep, n, g)[0] for g in (1, 5)}


@pytest.mark.parametrize("level", [0, None])
def test_fixture_a(level):
    sim, pop, ep, n, tr = started("fixture_a", level)
    before = (sim.download_state(), sim.records_so_far(), sim.exposure_events(), sim.area_census("home"))
    check_all(sim, pop, n, tr, cached_rule_of("fixture_a"), "fixture A, level %s" % level)
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
        check_all(sim, pop, n, tr, cached_rule_of("fixture_a"), "fixture A after esim_restart")
        # other index cases, from a list with a duplicate: three seeds in force
        s = pop.seeds
        seeds = (int(s[3]), int(s[0]), int(s[3]), int(s[7]))
        pop2, ep2, tr2, rules = reseeded(seeds, n)
        sim.restart(seeds=np.asarray(seeds, np.uint32))
        sim.run(n)
        check_all(sim, pop2, n, tr2, lambda g: rules[g], "fixture A after esim_restart_seeded with a duplicate in the list")
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
        tr = ref.base(name)[3]
        sim.rollback(**over)
        sim.run(n - t)
        check_all(sim, pop, n, tr, cached_rule_of(name), what)
    # a rollback under another bus_capacity: a bus replay under two capacities is not built
    sim.rollback(bus_capacity=int(a.bus_capacity) + 5)
    sim.run(10)
    lib, ctx = sim.lib, sim._ctx
    cell = np.zeros(4, np.uint64)
    assert lib.esim_contact_hours(ctx, _lib.BY_ALL, 0xF, 1, 5, cell.ctypes.data_as(u64p), None, None) == ESTATE
    assert b"two capacities" in lib.esim_last_error(ctx)
    # a history mixed twice
    sim.rollback()
    sim.run(20)
    sim.snapshot()
    sim.rollback(exposure_chance=b.exposure_chance)
    sim.run(20)
    sim.snapshot()
    sim.rollback(exposure_chance=0.005)
    sim.run(5)
    assert lib.esim_contact_hours(ctx, _lib.BY_ALL, 0xF, 1, 5, cell.ctypes.data_as(u64p), None, None) == ESTATE
    assert lib.esim_contact_hours(ctx, _lib.BY_ALL, 0xF, 1, 5, None, None, None) == ESTATE
    sim.close()


# ---- 2. errors -------------------------------------------------------------------------------------------------------------
def test_error_table():
    pop, ep, n, tr = ref.base("school")
    lib = _lib.load()
    buf64, buf32 = np.zeros(4 * 64, np.uint64), np.zeros(pop.n_citizens, np.uint32)
    q, p = buf64.ctypes.data_as(u64p), buf32.ctypes.data_as(u32p)
    call = lib.esim_contact_hours
    ALL, GROUP = _lib.BY_ALL, _lib.BY_GROUP
    bare = C.c_void_p()
    _lib.check(lib.esim_create(C.byref(ep), C.byref(bare)))
    assert call(bare, ALL, 0xF, 1, 1, q, q, p) == ESTATE and call(bare, ALL, 0xF, 1, 1, None, None, None) == ESTATE     # before an upload
    assert call(bare, _lib.AREA_HOME, 0xF, 1, 1, q, q, p) == EINVAL and call(bare, ALL, 0, 1, 1, q, q, p) == EINVAL
    lib.esim_destroy(bare)
    assert call(None, ALL, 0xF, 1, 1, q, q, p) == EINVAL
    sim = Simulator(pop, ref_mod.copy_params(ep))
    sim.run(10)
    ctx = sim._ctx
    for where in (_lib.AREA_CURRENT, _lib.AREA_HOME, _lib.BY_SETTING, 7, -1):
        assert call(ctx, where, 0xF, 1, 5, q, q, p) == EINVAL                                                     # unknown `where`
    assert call(ctx, ALL, 0, 1, 5, q, q, p) == EINVAL and call(ctx, ALL, 0x10, 1, 5, q, q, p) == EINVAL           # empty mask, a bit beyond transport
    assert call(ctx, ALL, 0x1F, 1, 5, q, q, p) == EINVAL
    assert call(ctx, GROUP, 0xF, 1, 5, q, q, p) == ESTATE                                                        # by group without labels
    assert call(ctx, ALL, 0xF, 0, 5, q, q, p) == ERANGE and call(ctx, ALL, 0xF, 5, 4, q, q, p) == ERANGE
    assert call(ctx, ALL, 0xF, 1, 11, q, q, p) == ERANGE and call(ctx, ALL, 0xF, 11, 11, q, q, p) == ERANGE
    assert call(ctx, ALL, 0xF, 1, 1, q, q, p) == 0 and call(ctx, ALL, 0xF, 10, 10, q, q, p) == 0 and call(ctx, ALL, 8, 1, 10, q, None, None) == 0
    with pytest.raises(_lib.EsimError):
        sim.contact_hours(last_step=11)
    with pytest.raises(ValueError):
        sim.contact_hours(settings="nowhere")
    sim.run(n - 10)                                                  # the context is usable afterwards
    rule = ref.cached_rule("school", 1)
    same(sim.contact_hours()["hours"], rule.window(), "after the refusals")
    rates = sim.contact_rates(first_step=n // 2)
    got = sim.contact_hours(first_step=n // 2)
    assert rates.shape == (4, 1, 1) and np.array_equal(rates, Simulator._rate(got["transmissions"], got["hours"]), equal_nan=True)
    # a sticky device-side error comes back as esim_transmission_tree reports it
    _lib.check(lib.esim_debug_inject_error(ctx, ERANGE), ctx)
    want = lib.esim_transmission_tree(ctx, None, None, None)
    assert want != 0
    assert call(ctx, ALL, 0xF, 1, 4, q, q, p) == want and call(ctx, ALL, 0xF, 1, 4, None, None, None) == want
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
    cell = np.zeros(4, np.uint64)
    assert sim.lib.esim_contact_hours(sim._ctx, _lib.BY_ALL, 0xF, 1, 4, cell.ctypes.data_as(u64p), None, None) == ESTATE
    sim.close()


# ---- 3. the ensemble -------------------------------------------------------------------------------------------------------
def test_ensemble_gathers_the_members_contacts(tmp_path):
    pop, ep, _ = ref_mod.ties_world()
    n_steps, g = 120, 5
    lab = hh.labels(pop, g)
    ens = Ensemble(pop, ref_mod.copy_params(ep), group=(lab, g))
    members = ens.seeds(3, first=31)
    res = ens.contacts(members, n_steps)
    by_group = ens.contacts(members, n_steps, where="group", settings=("household",), first_step=10, last_step=60)
    assert res.hours.shape == res.transmissions.shape == (3, 4, 1, 1) and by_group.hours.shape == (3, 4, g, g) and by_group.hours.dtype == np.uint64
    for i, m in enumerate(members):
        ep_i = ref_mod.copy_params(ep, seed=m["seed"])
        rule, tr, _ = ref.member_rule(pop, ep_i, n_steps, g)
        same(res.hours[i, :, 0, 0], rule.window().sum(axis=(1, 2)), "member %d: hours" % i)
        same(res.transmissions[i], ref.transmissions(tr, np.zeros(pop.n_citizens, np.uint16), 1), "member %d: transmissions" % i)
        same(by_group.hours[i], rule.window(10, 60, 1), "member %d: hours by group" % i)
        same(by_group.transmissions[i], ref.transmissions(tr, lab, g, 10, 60, 1), "member %d: transmissions by group" % i)
    assert int(res.transmissions.sum()) >= 100
    rate = res.rate()
    assert rate.shape == (4, 1, 1) and rate[0, 0, 0] == float(res.transmissions[:, 0].sum()) / float(res.hours[:, 0].sum()) and np.isnan(rate[2]).all()
    res.dump(str(tmp_path))
    same(np.load(tmp_path / "ensemble_contacts.npz")["hours"], res.hours, "ensemble_contacts.npz")
    ens.close()
