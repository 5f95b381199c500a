"""Ensembles on one uploaded population: esim_restart (back to step 0 under other parameters, rebuilt on the device), the
per-Output-Area accumulators over the members (esim_ensemble_*) and the Python Ensemble.  Every expectation comes from the CPU
oracle created fresh with a member's parameters, or from esim_reset on a fresh context -- never from the code under test."""
import ctypes as C
import json

import numpy as np
import pytest

import _oracle
from epidemicsimulator_amd import Ensemble, Population, Simulator, _lib
from test_parity_gpu import AGGRESSIVE, assert_same_records, assert_same_state, random_population, set_form

pytestmark = pytest.mark.gpu

E, I, R = 1 << _lib.EXPOSED, 1 << _lib.INFECTED, 1 << _lib.RECOVERED
FORMS = ("vax", "wide", "tinymax", "pipe", None)


def oracle_for(pop, base, overrides):
    return _oracle.Oracle(pop, _oracle.params_from_esim(_lib.default_params(**dict(base, **overrides))))


def checkpoint_bytes(sim, path):
    sim.save_checkpoint(str(path))
    return np.fromfile(str(path), np.uint8)


# ---- 1. a restart equals a reset, to the byte ------------------------------------------------------------------------------
def test_restart_with_the_same_parameters_equals_a_reset_to_the_byte(tmp_path):
    pop = Population.synthetic("york")
    ep = _lib.default_params()
    fresh = Simulator(pop, ep)
    fresh.reset()
    want = checkpoint_bytes(fresh, tmp_path / "fresh.bin")
    fresh.close()
    sim = Simulator(pop, ep)
    sim.run(300)
    sim.restart()
    got = checkpoint_bytes(sim, tmp_path / "restarted.bin")
    assert got.size == want.size and (got == want).all()
    sim.close()
    # ... and after a run that ended under a vaccination programme: plan fields, plan_skip and bus_exposed bits are set in the words
    small = Population.synthetic("york", n_citizens=6000, n_areas=20, citizens_per_school=3000, n_seeds=12, p_public_transport=0.4)
    ep = _lib.default_params(**AGGRESSIVE)
    fresh = Simulator(small, ep)
    fresh.reset()
    want = checkpoint_bytes(fresh, tmp_path / "fresh2.bin")
    fresh.close()
    sim = Simulator(small, ep)
    rec = sim.run(433)
    assert rec["vaccination_active"][-1] == 1 and rec["vaccinated"][-1] > 0 and rec["exposures_bus"].sum() > 0
    sim.restart()
    got = checkpoint_bytes(sim, tmp_path / "restarted2.bin")
    assert got.size == want.size and (got == want).all()
    # the restarted context runs what the fresh one runs
    assert_same_records(sim.run(433), rec)
    sim.close()


# ---- 2. every member is the run a fresh context would have made --------------------------------------------------------------
def parity_world():
    # test_random_populations_all_paths, seed 5: reaches a lockdown and a vaccination programme within 500 steps
    pop = random_population(5)
    base = dict(exposure_chance=0.01, seed=1023163785973, vaccination_rate=3, vaccination_threshold=0.08, lockdown_threshold=0.05,
                mask_pt_threshold=0.02, mask_everywhere_threshold=0.04, bus_capacity=20, exposed_time=96, infected_time=336,
                start_hour=9, end_hour=20)
    members = [({}, 500), ({"seed": 99}, 137), ({"exposure_chance": 0.02}, 500),
               ({"vaccination_rate": 25, "vaccination_threshold": 0.03, "lockdown_threshold": 0.1, "mask_pt_threshold": 0.01,
                 "mask_everywhere_threshold": 0.03}, 500),
               ({"exposed_time": 30, "infected_time": 100, "seed": 7}, 410)]
    return pop, base, members


def york_world():
    # York with the v1.7.1 parameters (85 vaccinations a step, threshold 0.003), 1200 steps
    pop = Population.synthetic("york")
    base = dict(vaccination_rate=85, vaccination_threshold=0.003)
    members = [({}, 1200), ({"seed": 20260101}, 683), ({"exposure_chance": 0.0008}, 1200),
               ({"vaccination_rate": 400, "vaccination_threshold": 0.002, "lockdown_threshold": 0.002, "mask_pt_threshold": 0.0005,
                 "mask_everywhere_threshold": 0.001}, 1200),
               ({"exposed_time": 48, "infected_time": 200}, 1200)]
    return pop, base, members


@pytest.mark.parametrize("world", (parity_world, york_world))
def test_every_member_is_the_run_of_a_fresh_context(world):
    pop, base, members = world()
    want = []
    for overrides, steps in members:
        orc = oracle_for(pop, base, overrides)
        orc.set_threads(16)
        want.append((orc.run(steps), orc.state()))
        orc.close()
    if world is parity_world:
        assert want[0][0]["lockdown"].sum() > 0 and want[0][0]["vaccinated"][-1] > 0
    # a predecessor stops at a step that is no chunk boundary (chunks are exposed_time + 1 = 97 steps long at most)
    assert any(steps % 97 and steps % 96 for _, steps in members[:-1])
    for form in FORMS:
        sim = Simulator(pop, _lib.default_params(**base))
        set_form(sim, form)
        try:
            for (overrides, steps), (rec, state) in zip(members, want):
                sim.restart(_lib.default_params(**base), **overrides)
                assert_same_records(sim.run(steps), rec)
                g = sim.download_state()
                for k in ("status", "timer", "current_building", "on_bus", "eligible"):
                    assert (g[k] == state[k]).all(), (k, overrides)
        except AssertionError as e:
            raise AssertionError("execution form %r: %s" % (form, e)) from e
        finally:
            sim.close()


# ---- 3. refusals -------------------------------------------------------------------------------------------------------------
def test_refused_restarts_leave_the_context_as_it_was():
    pop = Population.synthetic("york", n_citizens=6000, n_areas=20, citizens_per_school=3000, n_seeds=12)
    base = dict(max_steps=400, **AGGRESSIVE)
    sim = Simulator(pop, _lib.default_params(**base))
    sim.run(50)
    # the cases of test_create_rejects_out_of_range_params, with the codes esim_create returns for them
    for bad, code in ((dict(exposed_time=400, infected_time=200), -5), (dict(max_steps=9000), -5), (dict(bus_capacity=0), -1),
                      (dict(max_steps=401), -5), (dict(device=1), -1)):
        p = _lib.default_params(**dict(base, **bad))
        ctx = C.c_void_p()
        if "device" not in bad and bad.get("max_steps") != 401:
            assert sim.lib.esim_create(C.byref(p), C.byref(ctx)) == code
        assert sim.lib.esim_restart(sim._ctx, C.byref(p)) == code, bad
        with pytest.raises(_lib.EsimError):
            sim.restart(**bad)
    # the run that follows still is the old parameters' run, from where it stood
    orc = oracle_for(pop, base, {})
    want = orc.run(300)
    assert_same_records(sim.run(250), want[50:])
    assert_same_state(sim, orc)
    sim.close()


def test_restart_of_a_context_with_a_communicator_of_two_ranks_is_refused():
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
    p = _lib.default_params(seed=5)
    assert sim.lib.esim_restart(sim._ctx, C.byref(p)) == -4          # ESIM_ESTATE
    sim.close()


# ---- 4. checkpoint after a restart --------------------------------------------------------------------------------------------
def test_checkpoint_after_a_restart_belongs_to_the_new_parameters(tmp_path):
    pop = Population.synthetic("york", n_citizens=6000, n_areas=20, citizens_per_school=3000, n_seeds=12)
    a_par = dict(AGGRESSIVE)
    b_over = dict(seed=4242, exposure_chance=0.006, vaccination_rate=60, exposed_time=60, infected_time=200)
    want = oracle_for(pop, a_par, b_over).run(450)
    sim = Simulator(pop, _lib.default_params(**a_par))
    sim.run(123)
    sim.restart(**b_over)
    first = sim.run(200)
    path = str(tmp_path / "b200.bin")
    sim.save_checkpoint(path)
    sim.close()
    direct = Simulator(pop, _lib.default_params(**dict(a_par, **b_over)))
    direct.load_checkpoint(path)
    assert direct._steps == 200
    assert_same_records(np.concatenate([first, direct.run(250)]), want)
    direct.close()
    still_a = Simulator(pop, _lib.default_params(**a_par))
    with pytest.raises(_lib.EsimError, match="another population"):
        still_a.load_checkpoint(path)
    # ... and goes in once that context has been restarted to B's parameters
    still_a.restart(**b_over)
    still_a.load_checkpoint(path)
    assert_same_records(np.concatenate([first, still_a.run(250)]), want)
    still_a.close()


# ---- 5. accumulators -----------------------------------------------------------------------------------------------------------
def area_world():
    pop = Population.synthetic("york", n_citizens=20000, n_areas=64, citizens_per_school=5000, n_seeds=6)
    return pop, dict(exposure_chance=0.002), [{"seed": 100 + s} for s in range(6)], 250      # step 250: hour 10, commuters at work


def oracle_x(pop, state, where, mask):
    if where == "home":
        area = pop.building_area[pop.home_building]
    else:
        area = pop.building_area[state["current_building"]]      # (the oracle's at-work bit, through _oracle.Oracle.state)
    sel = ((1 << state["status"].astype(np.uint32)) & mask) != 0
    return np.bincount(area[sel], minlength=pop.n_areas).astype(np.uint64)


def test_area_accumulators_equal_numpy_over_the_oracle_members():
    pop, base, members, steps = area_world()
    assert pop.n_areas >= 50 and len(members) >= 6
    states = []
    for m in members:
        orc = oracle_for(pop, base, m)
        orc.run(steps)
        states.append(orc.state())
        orc.close()
    configs = (("home", E | I | R, 1), ("current", I, 2))
    xs = {c: np.array([oracle_x(pop, st, c[0], c[1]) for st in states]) for c in configs}
    # the input is not trivial: an area reached in some members only; an area with two different counts >= 2
    hit0 = (xs[configs[0]] >= 1).sum(0)
    assert ((hit0 > 0) & (hit0 < len(members))).any()
    x1 = xs[configs[1]]
    assert any(len(set(int(v) for v in x1[:, a] if v >= 2)) >= 2 for a in range(pop.n_areas))
    assert any((st["current_building"] != pop.home_building).any() for st in states)
    sim = Simulator(pop, _lib.default_params(**base))
    assert sim.lib.esim_ensemble_fold(sim._ctx) == -4 and sim.lib.esim_ensemble_read(sim._ctx, None, None, None, None) == -4   # before begin
    assert sim.lib.esim_ensemble_begin(sim._ctx, _lib.AREA_HOME, 0, 1) == -1 and sim.lib.esim_ensemble_begin(sim._ctx, 7, I, 1) == -1
    for where, mask, min_cases in configs:
        x = xs[(where, mask, min_cases)]
        sim.ensemble_begin(where, mask, min_cases)
        for k, m in enumerate(members):
            sim.restart(**m)
            sim.run(steps)
            before = sim.area_census(where)
            sim.ensemble_fold()
            if k % 2:                                         # the count table is shared with esim_area_census: no state leaks
                assert (sim.area_census(where) == before).all()
                assert (sim.area_census("home" if where == "current" else "current") ==
                        np.stack([oracle_x(pop, states[k], "home" if where == "current" else "current", 1 << s) for s in range(5)], 1)).all()
        if where == "home":
            sim.reset()                                       # esim_reset and esim_restart keep the accumulators
        else:
            sim.restart(seed=1)
        got = sim.ensemble_read()
        assert got["members"] == len(members)
        assert (got["hit"] == (x >= min_cases).sum(0)).all()
        assert (got["sum"] == x.sum(0)).all()
        assert (got["sumsq"] == (x * x).sum(0)).all()
    # a new upload drops them
    ps = pop.as_struct()
    _lib.check(sim.lib.esim_upload_population(sim._ctx, C.byref(ps)), sim._ctx)
    assert sim.lib.esim_ensemble_fold(sim._ctx) == -4
    sim.close()
    # before any upload
    ctx = C.c_void_p()
    lib = _lib.load()
    _lib.check(lib.esim_create(C.byref(_lib.default_params()), C.byref(ctx)))
    assert lib.esim_ensemble_begin(ctx, _lib.AREA_HOME, I, 1) == -4
    lib.esim_destroy(ctx)


# ---- 6. Ensemble ---------------------------------------------------------------------------------------------------------------
def test_ensemble_records_quantiles_and_dump(tmp_path):
    pop, base, members, steps = area_world()
    codes = ["E%08d" % (7 * a) for a in range(pop.n_areas)]
    recs, states = [], []
    for m in members:
        orc = oracle_for(pop, base, m)
        recs.append(orc.run(steps))
        states.append(orc.state())
        orc.close()
    ens = Ensemble(pop, _lib.default_params(**base), area_codes=codes)
    assert Ensemble.seeds(6, first=100) == members
    res = ens.run(members, steps, area=dict(where="home", status_mask=E | I | R, min_cases=1))
    assert res.records.shape == (len(members), steps) and res.n_done.tolist() == [steps] * len(members) and res.members == members
    for k, r in enumerate(recs):
        assert_same_records(res.records[k], r)
    inf = np.array([r["infected"] for r in recs], np.float64)
    assert (res.quantiles("infected", [0.5]) == np.quantile(inf, [0.5], axis=0)).all()
    assert res.quantiles("infected", [0.05, 0.95]).shape == (2, steps)
    assert (res.mean("infected") == inf.mean(0)).all()
    x = np.array([oracle_x(pop, st, "home", E | I | R) for st in states], np.float64)
    assert res.area["members"] == len(members) and (res.area["hit"] == (x >= 1).sum(0)).all()
    assert np.allclose(res.area["mean"], x.mean(0), rtol=1e-12, atol=0) and np.allclose(res.area["var"], x.var(0), rtol=1e-9, atol=1e-9)
    out = str(tmp_path / "ens")
    res.dump(out)
    stats = json.load(open(out + "/ensemble_stats.json"))
    areas = json.load(open(out + "/ensemble_areas.json"))
    assert stats["fields"]["infected"]["q50"] == np.quantile(inf, 0.5, axis=0).tolist() and stats["fields"]["infected"]["mean"] == inf.mean(0).tolist()
    assert stats["n_done"] == [steps] * len(members) and stats["members"] == members
    assert sorted(areas["areas"]) == sorted(codes) and areas["members"] == len(members)
    for a in (0, 7, 36, 63):
        assert areas["areas"][codes[a]] == {"hit": int((x[:, a] >= 1).sum()), "mean": float(res.area["mean"][a]), "var": float(res.area["var"][a])}
    ens.close()


def test_ensemble_pads_members_whose_epidemic_died_out():
    # 600 citizens, 25 vaccinations a step from early on: everybody left Susceptible is vaccinated, the last case recovers --
    # around step 520-545, depending on the seed
    pop = Population.synthetic("york", n_citizens=600, n_areas=3, citizens_per_school=600, n_seeds=5)
    base = dict(exposure_chance=0.01, vaccination_threshold=0.011, vaccination_rate=25)
    members, steps = Ensemble.seeds(6, first=3), 540
    recs = [oracle_for(pop, base, m).run(steps, stop_when_done=True) for m in members]
    lens = [len(r) for r in recs]
    assert min(lens) < steps and max(lens) == steps and all(r["disease_exists"][-1] == 0 for r in recs if len(r) < steps)
    ens = Ensemble(pop, _lib.default_params(**base))
    res = ens.run(members, steps, stop_when_done=True)
    assert res.area is None and res.records.shape == (len(members), steps)
    assert res.n_done.tolist() == lens
    for k, r in enumerate(recs):
        n = len(r)
        assert_same_records(res.records[k][:n], r)
        pad = res.records[k][n:]
        assert pad["time_step"].tolist() == list(range(n + 1, steps + 1))
        for f in ("susceptible", "exposed", "infected", "recovered", "vaccinated", "lockdown", "vaccination_active", "mask_status"):
            assert (pad[f] == r[f][-1]).all(), f
        for f in ("exposures_building", "exposures_bus", "vaccinated_now", "disease_exists"):
            assert (pad[f] == 0).all(), f
    ens.close()
