"""Forecast ensembles on the device: esim_snapshot keeps the state of step T, esim_rollback branches from it.  Expectations come
from the CPU oracle run uninterrupted (same future; a branch whose overrides cannot act before T), from a second, independently
pinned execution form (branches the oracle cannot follow), and from numpy over per-step state downloads (the seam)."""
import ctypes as C

import numpy as np
import pytest

import _snapshot_ref as ref
from epidemicsimulator_amd import Ensemble, Simulator, _lib
from test_ensemble_gpu import FORMS, oracle_x
from test_parity_gpu import assert_same_records, set_form

pytestmark = pytest.mark.gpu

N = ref.N_STEPS
STATE_KEYS = ("status", "timer", "current_building", "on_bus", "eligible")
STATUS = ("susceptible", "exposed", "infected", "recovered", "vaccinated")
EINVAL, ESTATE, ERANGE = -1, -4, -5
WORLDS = ("parity", "york")
# The words of the control block (Ctrl, esim_device.h) that a rollback zeroes, as esim_checkpoint_restore does: the marks' lengths,
# counts, n_riders, future_t0, small_done, chunk_ok; items_per_wave, chunk_parallel; n_items .. chunk_done; prev_n_items,
# prev_per_wave; peer_error.  They describe the last chunk or launch of their kind and are written again only by the next one,
# which need not come (one kernel per step has no chunks once a programme runs): a checkpoint comparison leaves them out.
CTRL_NORMALISED = list(range(17, 42)) + [45, 46] + list(range(48, 54)) + [55, 56, 70]


def new_sim(name, form="vax", **over):
    pop, base = ref.world(name)
    sim = Simulator(pop, _lib.default_params(**dict(base, **over)))
    set_form(sim, form)
    return sim


def assert_state(sim, want, note=""):
    got = sim.download_state()
    for k in STATE_KEYS:
        assert (got[k] == want[k]).all(), "%s %s" % (k, note)


def same_log(a, b, note=""):
    assert a.shape == b.shape and (a == b).all(), "exposure logs differ as sets per step %s" % note


def oracle_log(name, branch=False):
    return ref.straight(name, branch)[2]


# ---- 1. same future ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS, ids=[str(f) for f in FORMS])
@pytest.mark.parametrize("name", WORLDS)
def test_a_rollback_to_the_snapshots_own_parameters_gives_the_same_future(name, form, tmp_path):
    """For T in 61, 137, 300 (300 lies inside the vaccination programme; none is a multiple of 96 or 97): run T, snapshot, run
    to 500, rollback(NULL), run to 500 again -- both passes equal the oracle's uninterrupted 500 steps in records, state and
    exposure log.  The checkpoint afterwards equals, byte for byte (log entries sorted inside a step: their order there is
    unspecified; the control block's per-chunk fields that the rollback's normalisation zeroes left out), that of a context that
    made the same two calls without a snapshot, and, the control block apart (it holds the last chunk's diagnostics, which follow the calls'
    boundaries), that of a context that ran the 500 steps in one call."""
    pop, _ = ref.world(name)
    want_rec, want_state, _ = ref.straight(name)
    want_log = oracle_log(name)
    one = new_sim(name, form)
    one.run(N)
    one.save_checkpoint(str(tmp_path / "one.bin"))
    one.close()
    one_call = ref.checkpoint_parts(tmp_path / "one.bin", pop.n_citizens)
    for t in (61, 137, 300):
        sim = new_sim(name, form)
        head = sim.run(t)
        sim.snapshot()
        assert sim.snapshot_step() == t
        for attempt in (0, 1):
            if attempt:
                _lib.check(sim.lib.esim_rollback(sim._ctx, None), sim._ctx)
                sim._steps = t
            tail = sim.run(N - t)
            note = "(T = %d, pass %d)" % (t, attempt)
            assert_same_records(np.concatenate([head, tail]), want_rec)
            assert_same_records(sim.records_so_far(), want_rec)
            assert_state(sim, want_state, note)
            same_log(ref.log_sets(sim), want_log, note)
        sim.save_checkpoint(str(tmp_path / "branch.bin"))
        sim.close()
        plain = new_sim(name, form)
        plain.run(t); plain.run(N - t)
        plain.save_checkpoint(str(tmp_path / "plain.bin"))
        plain.close()
        got, two_calls = ref.checkpoint_parts(tmp_path / "branch.bin", pop.n_citizens), ref.checkpoint_parts(tmp_path / "plain.bin", pop.n_citizens)
        for parts in (got, two_calls):
            words = parts["ctrl"].copy().view(np.uint32)
            assert words.size == 76
            words[CTRL_NORMALISED] = 0
            parts["ctrl"] = words.view(np.uint8)
        for key in got:
            assert got[key].size == two_calls[key].size, key
            bad = np.flatnonzero(got[key] != two_calls[key])
            assert bad.size == 0, "checkpoint section %s, T = %d: %d bytes differ, first at byte %d" % (key, t, bad.size, bad[0])
            if key != "ctrl":
                assert got[key].size == one_call[key].size and (got[key] == one_call[key]).all(), "checkpoint section %s against one call, T = %d" % (key, t)


# ---- 2. a branch under other parameters, against the oracle -----------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS, ids=[str(f) for f in FORMS])
@pytest.mark.parametrize("name", WORLDS)
def test_a_branch_whose_overrides_cannot_act_before_t_is_the_oracles_run_under_them(name, form):
    t, same_state, _ = ref.branch_step(name)
    assert t >= 100 and same_state                       # (tests/test_snapshot.py checks the precondition without a device)
    want_rec, want_state, _ = ref.straight(name, True)
    sim = new_sim(name, form)
    head = sim.run(t)
    sim.snapshot()
    sim.run(40)                                          # the branch does not leave from where the snapshot was taken
    sim.rollback(**ref.BRANCH_B[name])
    assert sim._steps == t
    tail = sim.run(N - t)
    assert_same_records(np.concatenate([head, tail]), want_rec)
    assert_same_records(sim.records_so_far(), want_rec)
    assert_state(sim, want_state)
    same_log(ref.log_sets(sim), oracle_log(name, True))
    sim.close()


# ---- 3. branches the oracle cannot follow ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", WORLDS)
def test_branches_under_a_new_seed_or_exposure_chance(name):
    pop, _ = ref.world(name)
    t = 137
    base_rec = ref.straight(name)[0]
    results = {}
    for over in (dict(seed=4242), dict(exposure_chance=0.02), dict(seed=99991)):
        key = tuple(sorted(over.items()))
        for form in ("vax", None):                       # the default and sequential steps, pinned independently of each other
            sim = new_sim(name, form)
            sim.run(t); sim.snapshot(); sim.run(60)
            runs = []
            for again in (0, 1):                         # the same branch taken twice
                sim.rollback(**over)
                sim.run(N - t)
                runs.append((sim.records_so_far(), sim.download_state(), ref.log_sets(sim)))
            sim.close()
            for rec, state, log in runs:
                results.setdefault(key, []).append((rec, state, log))
        first = results[key][0]
        for rec, state, log in results[key][1:]:
            assert_same_records(rec, first[0])
            for k in STATE_KEYS:
                assert (state[k] == first[1][k]).all(), (k, over)
            same_log(log, first[2], str(over))
        rec = first[0]
        assert len(rec) == N
        assert_same_records(rec[:t], base_rec[:t])                                      # records up to T are untouched
        total = sum(rec[f].astype(np.int64) for f in STATUS)
        assert (total == pop.n_citizens).all()
        assert any((rec[f][t:] != base_rec[f][t:]).any() for f in ref.FIELDS)          # ... and the future is another one
        base_log = oracle_log(name)
        same_log(first[2][first[2][:, 0] <= t], base_log[base_log[:, 0] <= t], "up to T")
    a, b = results[(("seed", 4242),)][0][0], results[(("seed", 99991),)][0][0]
    assert any((a[f][t:] != b[f][t:]).any() for f in ref.FIELDS)                        # a different seed, different records behind T


# ---- 4. the seam ---------------------------------------------------------------------------------------------------------------------
def tables_from_states(pop, states):
    """[steps, n_areas, 5] by home area and by the area stood in, from one per-citizen state per step."""
    home_area = pop.building_area[pop.home_building]
    out = {"home": np.zeros((len(states), pop.n_areas, 5), np.uint32), "current": np.zeros((len(states), pop.n_areas, 5), np.uint32)}
    for i, st in enumerate(states):
        cur_area = pop.building_area[st["current_building"]]
        for s in range(5):
            sel = st["status"] == s
            out["home"][i, :, s] = np.bincount(home_area[sel], minlength=pop.n_areas)
            out["current"][i, :, s] = np.bincount(cur_area[sel], minlength=pop.n_areas)
    return out


def all_tables(sim, pop):
    out = {(w, k): sim.area_status_series(name, w) for w in ("home", "current") for k, name in enumerate(STATUS)}
    sim.set_groups(pop.building_area[pop.home_building], pop.n_areas)
    for k, name in enumerate(STATUS):
        out[("group", k)] = sim.group_series(name)
    out["group_census"] = sim.group_census()
    sim.set_groups(None)
    return out


def test_the_series_across_a_seam():
    """Snapshot inside a running programme, rollback under another seed AND vaccination rate, run on: the steps up to T drew their
    vaccinations under the old pair, the later ones under the new.  The reference is numpy over the per-citizen state downloaded
    after every single step of the same branch made step by step."""
    name, t, over = "york", 300, dict(seed=4242, vaccination_rate=15)
    pop, base = ref.world(name)
    assert ref.straight(name)[0]["vaccinated_now"][t - 1] > 0 and base["vaccination_rate"] != 15
    slow = new_sim(name)
    states = []
    for s in range(1, N + 1):
        if s == t + 1:
            slow.snapshot(); slow.rollback(**over)
        slow.run(1)
        states.append(slow.download_state())
    slow_rec = slow.records_so_far()
    slow.close()
    want = tables_from_states(pop, states)
    sim = new_sim(name)
    sim.run(t); sim.snapshot(); sim.run(77); sim.rollback(**over); sim.run(N - t)
    rec = sim.records_so_far()
    assert_same_records(rec, slow_rec)
    assert (rec["vaccinated_now"][t:t + 50] > 0).all() and rec["vaccinated_now"][t:].max() <= 15 < rec["vaccinated_now"][t - 1]   # the rate changed at the seam
    got = all_tables(sim, pop)
    V, I = _lib.VACCINATED, _lib.INFECTED
    for where in ("home", "current", "group"):
        census = got["group_census"] if where == "group" else sim.area_census(where)
        for k, status in enumerate(STATUS):
            tab = got[(where, k)]
            assert tab.shape == (N, pop.n_areas)
            assert (tab[-1] == census[:, k]).all(), "last %s row by %s against the census" % (status, where)
            w = want["home" if where == "group" else where][:, :, k]
            bad = np.argwhere(tab != w)
            assert len(bad) == 0, "%s rows by %s: %d entries differ, first at step %d" % (status, where, len(bad), bad[0][0] + 1)
        v = got[(where, V)].sum(1).astype(np.int64)
        assert (v[:-1] == rec["vaccinated"][1:]).all() and v[t - 1] > 0 and v[-1] > v[t - 1], where     # both sides of T
        # a record holds the census before its step's vaccinations, the rows the state after them: every status loses what the step
        # vaccinated of it, and together they lose what the Vaccinated gain
        lost = {k: rec[STATUS[k]].astype(np.int64) - got[(where, k)].sum(1) for k in range(4)}
        gained = v - rec["vaccinated"]
        assert all((lost[k] >= 0).all() for k in lost) and (sum(lost.values()) == gained).all(), where
        assert (lost[I][rec["vaccinated_now"] == 0] == 0).all() and lost[I].sum() > 0, where
    # checkpoints name one parameter set: refused while the seam is in force, and so is a snapshot of the mixed history
    size = C.c_size_t(0)
    buf = np.zeros(1 << 20, np.uint8)
    assert sim.lib.esim_checkpoint_size(sim._ctx, C.byref(size)) == ESTATE
    assert sim.lib.esim_checkpoint_save(sim._ctx, buf.ctypes.data_as(C.c_void_p), buf.size) == ESTATE
    assert sim.lib.esim_snapshot(sim._ctx) == ESTATE and sim.snapshot_step() == t
    # back under the snapshot's own parameters the tables are those of the uninterrupted run, exactly
    sim.rollback()
    sim.run(N - t)
    assert sim.lib.esim_checkpoint_size(sim._ctx, C.byref(size)) == 0            # (no seam any more)
    again = all_tables(sim, pop)
    plain = new_sim(name)
    plain.run(N)
    straight = all_tables(plain, pop)
    for key in straight:
        assert (again[key] == straight[key]).all(), key
    assert_same_records(sim.records_so_far(), ref.straight(name)[0])
    plain.close(); sim.close()


# ---- 5. ensemble accumulators and arrival ------------------------------------------------------------------------------------------------
def test_forecast_accumulators_equal_numpy_over_the_members_and_forecast_equals_run():
    name = "york"
    pop, base = ref.world(name)
    t = ref.branch_step(name)[0]
    E_, I_, R_ = 1 << _lib.EXPOSED, 1 << _lib.INFECTED, 1 << _lib.RECOVERED
    members = [{"seed": 11}, {"seed": 12, "exposure_chance": 0.006}, {"lockdown_threshold": 0.01}, {}]
    # the members' own states and arrival maps, one branch at a time
    labels, n_groups = np.arange(pop.n_citizens) // 25, (pop.n_citizens + 24) // 25
    sim = new_sim(name)
    sim.set_groups(labels, n_groups)
    sim.run(t); sim.snapshot()
    states, arrivals, recs = [], [], []
    for m in members:
        sim.rollback(**m)
        sim.run(N - t)
        states.append(sim.download_state()); arrivals.append(sim.area_arrival("group")); recs.append(sim.records_so_far())
    sim.close()
    ens = Ensemble(pop, _lib.default_params(**base), group=(labels, n_groups))
    res = ens.forecast(t, members, N, area=dict(kind="census", where="home", status_mask=E_ | I_ | R_, min_cases=2))
    x = np.array([oracle_x(pop, st, "home", E_ | I_ | R_) for st in states])
    assert res.records.shape == (len(members), N) and res.n_done.tolist() == [N] * len(members)
    for k in range(len(members)):
        assert_same_records(res.records[k], recs[k])
        assert_same_records(res.records[k][:t], ref.straight(name)[0][:t])
    assert len({x[:, a].tobytes() for a in range(pop.n_areas)}) > 1 and (x.std(0) > 0).any()
    assert res.area["members"] == len(members) and (res.area["hit"] == (x >= 2).sum(0)).all()
    assert np.allclose(res.area["mean"], x.mean(0), rtol=1e-12, atol=0) and np.allclose(res.area["var"], x.var(0), rtol=1e-9, atol=1e-9)
    raw = ens.simulator.ensemble_read()
    assert (raw["sum"] == x.sum(0)).all() and (raw["sumsq"] == (x * x).sum(0)).all()
    horizon = t + 100
    res = ens.forecast(t, members, N, area=dict(kind="arrival", where="group", horizon=horizon))
    raw = ens.simulator.ensemble_read()
    a = np.array(arrivals).astype(np.uint64)
    reached = (np.array(arrivals) != _lib.NEVER) & (a <= horizon)
    assert (reached.sum(0) % len(members) != 0).any()                 # a group reached in some members only
    assert raw["members"] == len(members) and (raw["hit"] == reached.sum(0)).all()
    assert (raw["sum"] == np.where(reached, a, 0).sum(0)).all() and (raw["sumsq"] == np.where(reached, a * a, 0).sum(0)).all()
    assert res.quantiles("infected", [0.5]).shape == (1, N) and res.mean("infected").shape == (N,)
    # a forecast from T under overrides that cannot act before T is Ensemble.run of the same members from step 0
    pair = [dict(ref.BRANCH_B[name]), {}]
    fore, full = ens.forecast(t, pair, N), ens.run(pair, N)
    assert fore.records.shape == full.records.shape == (2, N)
    for k in range(2):
        assert_same_records(fore.records[k], full.records[k])
    assert_same_records(fore.records[0], ref.straight(name, True)[0])
    ens.close()


# ---- 6. the error table ----------------------------------------------------------------------------------------------------------------
def untouched(sim, rec, state, step):
    """A refused call left the records, the state and the snapshot as they were."""
    assert_same_records(sim.records_so_far(), rec)
    assert_state(sim, state)
    assert sim.snapshot_step() == step


def test_refusals_leave_records_state_and_snapshot_unchanged():
    name = "york"
    pop, base = ref.world(name)
    want_rec, want_state, _ = ref.straight(name)
    lib = _lib.load()
    sim = new_sim(name, max_steps=600)
    P = lambda **over: C.byref(_lib.default_params(**dict(base, max_steps=600, **over)))
    rec = sim.run(120)
    state = sim.download_state()
    # without a snapshot, and after a drop
    assert lib.esim_rollback(sim._ctx, None) == ESTATE and lib.esim_rollback(sim._ctx, P()) == ESTATE
    untouched(sim, rec, state, 0)
    sim.snapshot()
    info, step = _lib.Params(), C.c_uint32(0)
    assert lib.esim_snapshot_info(sim._ctx, C.byref(step), C.byref(info)) == 0 and step.value == 120
    assert (info.seed, info.vaccination_rate, info.max_steps) == (base["seed"], base["vaccination_rate"], 600)
    assert lib.esim_snapshot_drop(sim._ctx) == 0 and lib.esim_snapshot_drop(sim._ctx) == 0
    assert lib.esim_rollback(sim._ctx, None) == ESTATE
    untouched(sim, rec, state, 0)
    # parameters a rollback refuses
    sim.snapshot()
    more = sim.run(30)
    rec, state = np.concatenate([rec, more]), sim.download_state()
    for bad, code in ((dict(exposed_time=95), EINVAL), (dict(infected_time=300), EINVAL), (dict(start_hour=8), EINVAL), (dict(end_hour=18), EINVAL),
                      (dict(device=1), EINVAL), (dict(max_steps=601), ERANGE), (dict(max_steps=100), ERANGE), (dict(exposure_chance=float("nan")), EINVAL),
                      (dict(exposure_chance=-0.25), EINVAL), (dict(exposure_chance=1.5), EINVAL), (dict(bus_capacity=0), EINVAL),
                      (dict(vaccination_rate=9000), ERANGE)):
        p = _lib.default_params(**dict(dict(base, max_steps=600), **bad))
        assert lib.esim_rollback(sim._ctx, C.byref(p)) == code, bad
        untouched(sim, rec, state, 120)
    # a snapshot on a branch with a seam, and checkpoints there
    sim.rollback(seed=5)
    sim.run(10)
    size = C.c_size_t(0)
    assert lib.esim_snapshot(sim._ctx) == ESTATE and lib.esim_checkpoint_size(sim._ctx, C.byref(size)) == ESTATE
    assert sim.snapshot_step() == 120
    # a sticky error before a snapshot (the existing diagnostics call)
    sim.rollback()
    sim.run(17)
    _lib.check(lib.esim_debug_inject_error(sim._ctx, -6), sim._ctx)
    assert lib.esim_snapshot(sim._ctx) == ESTATE and sim.snapshot_step() == 120
    # ... a rollback clears it with the rest of the control block; the future is the oracle's
    sim.rollback()
    assert_same_records(np.concatenate([rec[:120], sim.run(N - 120)]), want_rec)
    assert_state(sim, want_state)
    # the snapshot survives esim_reset and esim_restart
    sim.reset()
    assert sim.snapshot_step() == 120
    sim.run(33)
    sim.rollback()
    assert_same_records(np.concatenate([rec[:120], sim.run(N - 120)]), want_rec)
    assert_same_records(sim.records_so_far(), want_rec)
    sim.restart(seed=31337, exposed_time=40)
    sim.run(50)
    sim.rollback()
    assert sim.params.seed == base["seed"] and sim.params.exposed_time == 96
    sim.run(N - 120)
    assert_same_records(sim.records_so_far(), want_rec)
    assert_state(sim, want_state)
    same_log(ref.log_sets(sim), oracle_log(name))
    sim.reset()                                          # (a reset afterwards starts under the times the rollback put back in force)
    assert_same_records(sim.run(150), want_rec[:150])
    # a second snapshot replaces the first
    sim.rollback(); sim.run(80); sim.snapshot()
    assert sim.snapshot_step() == 200
    sim.run(100); sim.rollback()
    assert sim._steps == 200
    sim.run(N - 200)
    assert_same_records(sim.records_so_far(), want_rec)
    assert_state(sim, want_state)
    # esim_restart_seeded and a new upload drop it; at step 0 there is nothing to keep
    sim.restart(seeds=pop.seeds)
    assert sim.snapshot_step() == 0 and lib.esim_rollback(sim._ctx, None) == ESTATE and lib.esim_snapshot(sim._ctx) == ESTATE
    sim.run(20); sim.snapshot()
    ps = pop.as_struct()
    _lib.check(lib.esim_upload_population(sim._ctx, C.byref(ps)), sim._ctx)
    assert sim.snapshot_step() == 0 and lib.esim_rollback(sim._ctx, None) == ESTATE
    sim._steps = 0
    assert_same_records(sim.run(150), want_rec[:150])
    sim.close()
    # before an upload
    ctx = C.c_void_p()
    _lib.check(lib.esim_create(C.byref(_lib.default_params()), C.byref(ctx)))
    assert lib.esim_snapshot(ctx) == ESTATE and lib.esim_rollback(ctx, None) == ESTATE and lib.esim_snapshot_drop(ctx) == 0
    step = C.c_uint32(9)
    assert lib.esim_snapshot_info(ctx, C.byref(step), None) == 0 and step.value == 0
    lib.esim_destroy(ctx)


def test_a_context_with_a_communicator_of_two_ranks_refuses_snapshot_and_rollback():
    from epidemicsimulator_amd import Population
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
    assert sim.lib.esim_snapshot(sim._ctx) == ESTATE and b"communicator" in sim.lib.esim_last_error(sim._ctx)
    assert sim.lib.esim_rollback(sim._ctx, None) == ESTATE and b"communicator" in sim.lib.esim_last_error(sim._ctx)
    assert sim.snapshot_step() == 0
    sim.close()
