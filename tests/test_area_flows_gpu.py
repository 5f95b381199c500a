"""Area flows, imports, the invasion tree and the (lineage, area) pairs on the device (esim_area_flows, esim_area_imports,
esim_area_invasion, esim_lineage_areas) against the numpy reference of tests/_flow_ref.py, which takes the infectors from the
tree of tests/_tree_ref.py and the lineages from tests/_chain_ref.py.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import _chain_ref as chain
import _flow_ref as flow
import _setting_ref as ref_mod
import _tree_ref as tree
from epidemicsimulator_amd import Population, Simulator, _lib
from epidemicsimulator_amd.ensemble import Ensemble
from test_area_flows import MASKS, flow_identities, situation, windows

pytestmark = pytest.mark.gpu

EINVAL, ENOMEM, ESTATE, ERANGE = -1, -3, -4, -5
u32p, u8p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)
IMPORTS = ("local", "imported", "exported")
INVASION = ("first_case", "step", "source_area", "setting")
NAMES = ("household", "workplace", "school", "transport")


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, "%s: shape %s, expected %s" % (what, got.shape, want.shape)
    bad = np.flatnonzero(got.ravel() != want.ravel())
    assert bad.size == 0, "%s: %d of %d differ, first at %d: got %s, expected %s" % (what, bad.size, got.size, bad[0], got.ravel()[bad[0]], want.ravel()[bad[0]])


def settings_of(mask):
    return None if mask == flow.ALL else [NAMES[s] for s in range(4) if (mask >> s) & 1]


def ptr(a):
    return a.ctypes.data_as(u8p if a.dtype == np.uint8 else u32p)


def check_all(sim, pop, n, ref, ch, what):
    na = pop.n_areas
    for mask in MASKS:
        for first, last in windows(ref, n):
            tag = "%s, mask %x, steps %d..%d" % (what, mask, first, last)
            got = sim.area_flows(settings_of(mask), first, last)
            for g, w, k in zip(got, flow.flows(ref, pop, mask, first, last), ("src", "dst", "count")):
                same(g, w, "%s: flows %s" % (tag, k))
            imp = sim.area_imports(settings_of(mask), first, last)
            want = flow.imports(ref, pop, mask, first, last)
            for k in IMPORTS:
                same(imp[k], want[k], "%s: %s" % (tag, k))
            flow_identities(got[0], got[1], got[2], imp, na)
    inv, want = sim.area_invasion(), flow.invasion(ref, pop)
    for k in INVASION:
        same(inv[k], want[k], "%s: invasion %s" % (what, k))
    same(inv["step"], sim.area_arrival("home"), what + ": the steps of the invasion tree are the arrival times")
    has = np.flatnonzero(inv["source_area"] != _lib.NO_AREA)
    assert (inv["step"][inv["source_area"][has]] < inv["step"][has]).all() and (inv["source_area"][has] != has).all()
    lin, w_lin = sim.lineage_areas(), flow.lineage_areas(ch, pop)
    for g, w, k in zip(lin, w_lin, ("lineage", "area", "count")):
        same(g, w, "%s: lineage areas %s" % (what, k))
    # each output alone, and none; a buffer too small by one
    lib, ctx = sim.lib, sim._ctx
    w_flows, w_imp = flow.flows(ref, pop), flow.imports(ref, pop)
    n_out = C.c_uint32(0)
    for i in range(3):
        for call, head, full in ((lib.esim_area_flows, (flow.ALL, 1, n), w_flows), (lib.esim_lineage_areas, (), w_lin)):
            one, args = np.zeros(full[i].size, np.uint32), [None, None, None]
            args[i] = ptr(one)
            assert call(ctx, *head, *args, one.size, C.byref(n_out)) == 0 and n_out.value == one.size
            same(one, full[i], "%s: output %d alone" % (what, i))
        one, args = np.zeros(na, np.uint32), [None, None, None]
        args[i] = ptr(one)
        assert lib.esim_area_imports(ctx, flow.ALL, 1, n, *args) == 0
        same(one, w_imp[IMPORTS[i]], "%s: %s alone" % (what, IMPORTS[i]))
    for i, k in enumerate(INVASION):
        one, args = np.zeros(na, np.uint8 if k == "setting" else np.uint32), [None, None, None, None]
        args[i] = ptr(one)
        assert lib.esim_area_invasion(ctx, *args) == 0
        same(one, flow.invasion(ref, pop)[k], "%s: invasion %s alone" % (what, k))
    assert lib.esim_area_imports(ctx, flow.ALL, 1, n, None, None, None) == 0 and lib.esim_area_invasion(ctx, None, None, None, None) == 0
    for call, head, full in ((lib.esim_area_flows, (flow.ALL, 1, n), w_flows), (lib.esim_lineage_areas, (), w_lin)):
        size = full[0].size
        assert call(ctx, *head, None, None, None, size, C.byref(n_out)) == 0 and n_out.value == size
        buf = np.full(size, 0xDEADBEEF, np.uint32)
        n_out.value = 0
        assert call(ctx, *head, ptr(buf), ptr(buf), ptr(buf), size - 1, C.byref(n_out)) == ERANGE and n_out.value == size
        assert (buf == 0xDEADBEEF).all()
    same(sim.area_flows()[2], w_flows[2], what + ": usable after ESIM_ERANGE")


def started(name, level=None):
    pop, ep, n, ref, ch = flow.cached(name)
    sim = Simulator(pop, ref_mod.copy_params(ep))
    if level is not None:
        sim.set_pipeline(level)
    sim.run(n)
    return sim, pop, ep, n, ref, ch


# ---- 1. every world against the reference ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["permuted", "ties", "as_u8", "school", "situations", "bus", "deep", "spread"])
def test_world(name):
    if name == "spread":
        situation()
    sim, pop, ep, n, ref, ch = started(name)
    check_all(sim, pop, n, ref, ch, name)
    if name == "spread":
        stats = sim.pair_stats()                                     # of check_all's last call: the flows of the whole run
        assert stats["dropped"] == 0 and stats["capacity"] >= 2 * stats["distinct"] and stats["distinct"] == flow.flows(ref, pop)[0].size
    sim.close()


@pytest.mark.parametrize("level", [0, None])
def test_fixture_a(level):
    sim, pop, ep, n, ref, ch = started("fixture_a", level)
    before = (sim.download_state(), sim.records_so_far(), sim.exposure_events(), sim.area_census("home"))
    check_all(sim, pop, n, ref, ch, "fixture A, level %s" % level)
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
        check_all(sim, pop, n, ref, ch, "fixture A after esim_restart")
        # other index cases, from a list with a duplicate: three seeds in force
        s = pop.seeds
        seeds = (int(s[3]), int(s[0]), int(s[3]), int(s[7]))
        pop2, ep2, _, ref2, ch2 = flow.reseeded("fixture_a", seeds, n)
        assert len(ch2["seeds"]) == 3 and int(np.unique(flow.lineage_areas(ch2, pop2)[0]).size) == 3
        sim.restart(seeds=np.asarray(seeds, np.uint32))
        sim.run(n)
        check_all(sim, pop2, n, ref2, ch2, "fixture A after esim_restart_seeded with a duplicate in the list")
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
        _, _, _, ref, ch = flow.cached(name)
        sim.rollback(**over)
        sim.run(n - t)
        check_all(sim, pop, n, ref, ch, what)
    lib, ctx = sim.lib, sim._ctx
    n_out = C.c_uint32(0)

    def all_four():
        return (lib.esim_area_flows(ctx, flow.ALL, 1, 5, None, None, None, 0, C.byref(n_out)), lib.esim_area_imports(ctx, flow.ALL, 1, 5, None, None, None),
                lib.esim_area_invasion(ctx, None, None, None, None), lib.esim_lineage_areas(ctx, None, None, None, 0, C.byref(n_out)))
    # a rollback under another bus_capacity: all four need the tree
    sim.rollback(bus_capacity=int(a.bus_capacity) + 5)
    sim.run(10)
    assert all_four() == (ESTATE,) * 4
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
    assert all_four() == (ESTATE,) * 4
    sim.close()


# ---- 2. errors -------------------------------------------------------------------------------------------------------------
def test_error_table():
    pop, ep, n, ref, ch = flow.cached("school")
    lib = _lib.load()
    buf, n_out = np.zeros(max(pop.n_areas, 4096), np.uint32), C.c_uint32(0)
    p, q, cap = buf.ctypes.data_as(u32p), buf.ctypes.data_as(u8p), buf.size
    flows, imports, invasion, lineages = lib.esim_area_flows, lib.esim_area_imports, lib.esim_area_invasion, lib.esim_lineage_areas
    A = flow.ALL
    bare = C.c_void_p()
    _lib.check(lib.esim_create(C.byref(ep), C.byref(bare)))
    assert flows(bare, A, 1, 1, p, p, p, cap, C.byref(n_out)) == ESTATE and imports(bare, A, 1, 1, p, p, p) == ESTATE                # before an upload
    assert invasion(bare, p, p, p, q) == ESTATE and lineages(bare, p, p, p, cap, C.byref(n_out)) == ESTATE
    assert flows(bare, A, 1, 1, p, p, p, cap, None) == EINVAL and lineages(bare, p, p, p, cap, None) == EINVAL and flows(bare, 0, 1, 1, p, p, p, cap, C.byref(n_out)) == EINVAL
    lib.esim_destroy(bare)
    assert flows(None, A, 1, 1, p, p, p, cap, C.byref(n_out)) == EINVAL and imports(None, A, 1, 1, p, p, p) == EINVAL
    assert invasion(None, p, p, p, q) == EINVAL and lineages(None, p, p, p, cap, C.byref(n_out)) == EINVAL
    sim = Simulator(pop, ref_mod.copy_params(ep))
    sim.run(10)
    ctx = sim._ctx
    assert flows(ctx, A, 1, 5, p, p, p, cap, None) == EINVAL and lineages(ctx, p, p, p, cap, None) == EINVAL                         # null n_out
    for mask in (0, 16, 0x1F, 0xFFFFFFFF):
        assert flows(ctx, mask, 1, 5, p, p, p, cap, C.byref(n_out)) == EINVAL and imports(ctx, mask, 1, 5, p, p, p) == EINVAL       # the mask
    for first, last in ((0, 5), (5, 4), (1, 11), (11, 11)):
        assert flows(ctx, A, first, last, p, p, p, cap, C.byref(n_out)) == ERANGE and imports(ctx, A, first, last, p, p, p) == ERANGE   # the steps
    assert flows(ctx, A, 1, 1, p, p, p, cap, C.byref(n_out)) == 0 and flows(ctx, A, 10, 10, p, p, p, cap, C.byref(n_out)) == 0 and imports(ctx, A, 1, 10, p, None, None) == 0
    with pytest.raises(_lib.EsimError):
        sim.area_flows(last_step=11)
    with pytest.raises(_lib.EsimError):
        sim.area_imports(first_step=0)
    with pytest.raises(ValueError):
        sim.area_flows(settings="pub")
    sim.run(n - 10)                                                  # the context is usable afterwards
    same(sim.area_flows()[2], flow.flows(ref, pop)[2], "after the refusals")
    # a sticky device-side error comes back as the calls underneath report it
    _lib.check(lib.esim_debug_inject_error(ctx, ERANGE), ctx)
    want = lib.esim_transmission_tree(ctx, None, None, None)
    assert want != 0
    assert flows(ctx, A, 1, 5, p, p, p, cap, C.byref(n_out)) == want and imports(ctx, A, 1, 5, p, p, p) == want
    assert invasion(ctx, p, p, p, q) == want and lineages(ctx, p, p, p, cap, C.byref(n_out)) == want
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
    n_done, n_out = C.c_uint32(0), C.c_uint32(0)
    _lib.check(sim.lib.esim_run_sharded(sim._ctx, 30, C.byref(n_done)), sim._ctx)
    lib, ctx = sim.lib, sim._ctx
    assert lib.esim_area_flows(ctx, flow.ALL, 1, 4, None, None, None, 0, C.byref(n_out)) == ESTATE and lib.esim_area_imports(ctx, flow.ALL, 1, 4, None, None, None) == ESTATE
    assert lib.esim_area_invasion(ctx, None, None, None, None) == ESTATE and lib.esim_lineage_areas(ctx, None, None, None, 0, C.byref(n_out)) == ESTATE
    sim.close()


# ---- 3. the capacity knob --------------------------------------------------------------------------------------------------
def test_pair_table_exactly_large_enough_and_too_small(monkeypatch):
    pop, ep, n, ref, ch = flow.cached("permuted")
    want = flow.flows(ref, pop)
    assert 64 < want[0].size == 125 <= 128
    monkeypatch.setenv("ESIM_PAIR_LOG2", "7")                        # 125 pairs in 128 slots
    sim = Simulator(pop, ref_mod.copy_params(ep))
    sim.run(n)
    for g, w, k in zip(sim.area_flows(), want, ("src", "dst", "count")):
        same(g, w, "ESIM_PAIR_LOG2=7: " + k)
    stats = sim.pair_stats()
    assert (stats["distinct"], stats["capacity"], stats["dropped"]) == (125, 128, 0)
    sim.close()
    monkeypatch.setenv("ESIM_PAIR_LOG2", "6")                        # ... and in 64
    sim = Simulator(pop, ref_mod.copy_params(ep))
    sim.run(n)
    n_out = C.c_uint32(0)
    assert sim.lib.esim_area_flows(sim._ctx, flow.ALL, 1, n, None, None, None, 0, C.byref(n_out)) == ENOMEM
    text = sim.lib.esim_last_error(sim._ctx).decode()
    assert "ESIM_PAIR_LOG2" in text and "keys were dropped" in text and int(text.split(": ")[-1].split()[0]) >= 125 - 64
    with pytest.raises(_lib.EsimError):
        sim.area_flows()
    same(sim.area_imports()["local"], flow.imports(ref, pop)["local"], "the context is usable after ESIM_ENOMEM")
    sim.close()
    monkeypatch.delenv("ESIM_PAIR_LOG2")
    sim = Simulator(pop, ref_mod.copy_params(ep))
    sim.run(n)
    for g, w, k in zip(sim.area_flows(), want, ("src", "dst", "count")):
        same(g, w, "without the knob again: " + k)
    sim.close()


# ---- 4. the ensemble -------------------------------------------------------------------------------------------------------
def test_ensemble_gathers_the_members_flows(tmp_path):
    pop, ep, n_steps = ref_mod.situations_world()
    n_steps = min(n_steps, 200)
    ens = Ensemble(pop, ref_mod.copy_params(ep))
    members = ens.seeds(3, first=31)
    res = ens.flows(members, n_steps)
    school = ens.flows(members, n_steps, settings="school", first_step=10, last_step=n_steps - 10)
    assert res.local.shape == res.step.shape == school.exported.shape == (3, pop.n_areas)
    for i, m in enumerate(members):
        ep_i = ref_mod.copy_params(ep, seed=m["seed"])
        ref = tree.reference(pop, ep_i, n_steps, ref_mod.reference(pop, ep_i, n_steps))
        imp, inv, imp_s = flow.imports(ref, pop), flow.invasion(ref, pop), flow.imports(ref, pop, 1 << _lib.SETTING_SCHOOL, 10, n_steps - 10)
        for k in IMPORTS:
            same(getattr(res, k)[i], imp[k], "member %d: %s" % (i, k))
            same(getattr(school, k)[i], imp_s[k], "member %d: %s at school" % (i, k))
        same(res.step[i], inv["step"], "member %d: step" % i)
        same(res.source_area[i], inv["source_area"], "member %d: source area" % i)
    share = res.imported_share()
    tot = res.imported.sum(axis=0).astype(np.float64) + res.local.sum(axis=0)
    assert share.shape == (pop.n_areas,) and (np.isnan(share) == (tot == 0)).all() and int(res.imported.sum()) >= 1
    res.dump(str(tmp_path))
    same(np.load(tmp_path / "ensemble_flows.npz")["imported"], res.imported, "ensemble_flows.npz")
    ens.close()
