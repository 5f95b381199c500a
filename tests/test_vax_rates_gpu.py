"""The vaccination walk at rates of thousands, up to the limit of 8192 a step (tests/_vax_rates.py; tests/test_vax_rates.py checks
on the CPU that every case reaches its regime: several batches of candidates per step, a hash set more than half full, the cut at
the rate in a second or later batch).  Every comparison is exact integer equality against the CPU oracle, or numpy over it.
  a. all eight execution forms in every case: every record field, the full state at the end of every block of 67 steps
  b. the forms that plan chunks under a programme once more with kernel timing on: planned steps where the plan condition
     holds, none where it fails; plans cut or repaired at 1024 a step, and the same records with the repair forced and off
  c. one context restarted from rate to rate, a predecessor stopped inside a planned chunk
  d. the consumers of the replayed walk (k_area_vax_replay) against their reference modules, once more with the grids capped
  e. a rollback's seam across the two arms of the choice: 8192 to 25 a step, 25 to 8192, the whole set to the walk and back
  f. two ranks: coupled steps where one batch of exchanged liveness cannot reach the rate, sharded plans where it can"""
import functools

import numpy as np
import pytest

import _area_status_ref as asr
import _burden_ref as burden
import _contact_ref as contact
import _curve_ref as curve
import _group_ref
import _household_ref as hh
import _setting_ref as setting
import _tree_ref as tree
import _vax_rates as vr
from epidemicsimulator_amd import Simulator, _lib
from test_burden_gpu import check_world as check_burden
from test_burden_gpu import same
from test_parity_gpu import SMALL_LIMITS, OracleRun, assert_same_records, run_forms
from test_sharded_gpu import launch
from test_snapshot_gpu import tables_from_states

pytestmark = pytest.mark.gpu

STATE_KEYS = ("status", "timer", "current_building", "on_bus", "eligible")
N_GROUPS = 5


@functools.lru_cache(maxsize=None)
def run_of(name):
    return vr.Run(name)


def under_the_programme(name):
    case = vr.CASES[name]
    return case.steps - case.trigger + 1


# ---- a. every execution form ----------------------------------------------------------------------------------------------------
FORM_IDS = {"vax": "vax", "wide": "wide", "tinymax": "tinymax", "tp": "tp", "pipe": "pipe", None: "sequential", 0: "multi_workgroup", 1 << 30: "persistent"}


@pytest.mark.parametrize("form", SMALL_LIMITS, ids=[FORM_IDS[f] for f in SMALL_LIMITS])
@pytest.mark.parametrize("name", list(vr.CASES))
def test_every_form_matches_the_oracle(name, form):
    run = run_of(name)
    assert run.steps == vr.CASES[name].steps and len(run.states) == len(run.asked)
    run_forms(run, (form,))


# ---- b. what was run is what was meant --------------------------------------------------------------------------------------------
def timed_stats(name):
    """Forms vax and wide once more with kernel timing on (the counters of the planned chunks count only then): the stats after
    the last block, per form."""
    run, seen = run_of(name), {}

    def observe(form, sim, i):
        if i < 0:
            sim.enable_kernel_timing(1)
        elif i == len(run.asked) - 1:
            seen[form] = dict(sim.vax_chunk_stats(), chunks=sim.chunk_timing()["steps"])

    run_forms(run, ("vax", "wide"), observe)
    return seen


@pytest.mark.parametrize("name", list(vr.CASES))
def test_the_plan_runs_where_its_condition_holds_and_nowhere_else(name):
    case = vr.CASES[name]
    for form, got in timed_stats(name).items():
        print("%s form %s: %d steps under the programme; %s" % (name, form, under_the_programme(name), got))
        assert got["chunks"] > 0, (form, got)                              # (steps run as one-pass chunks, planned or not)
        if case.plans:
            assert got["steps"] > 0 and got["chunks"] >= got["steps"], (form, got)
        else:
            assert got["steps"] == 0 and got["chunks"] < case.trigger, (form, got)     # chunks before the programme only
        if name == "rate_1024":
            assert got["repairs"] + got["cuts"] >= 1, (form, got)


@pytest.mark.parametrize("repair", (2, 0), ids=("repair_always", "cut_only"))
def test_plans_of_1024_a_step_repaired_from_the_start_or_only_cut(repair, monkeypatch):
    monkeypatch.setenv("ESIM_VAX_REPAIR", str(repair))
    for form, got in timed_stats("rate_1024").items():
        print("ESIM_VAX_REPAIR=%d form %s: %s" % (repair, form, got))
        assert got["steps"] > 0, (form, got)
        assert got["repairs"] >= 1 if repair else got["repairs"] == 0 and got["cuts"] >= 1, (form, got)


# ---- c. one context from rate to rate ---------------------------------------------------------------------------------------------
def test_one_context_restarted_from_rate_to_rate():
    """rate_8192_early stopped 40 steps into the programme -- inside a planned chunk, with rows of 8192 citizens in vax_ev and
    the census adjustments of the plan pending --, then a programme of 0 a step, rate_4096 stopped inside a chunk again, and
    rate_1024 to its end: every member equals a fresh oracle run."""
    pop = vr.world("W40")
    first = vr.CASES["rate_8192_early"]
    sim = Simulator(pop, vr.params_of("rate_8192_early"))
    members = (("rate_8192_early", None, first.trigger + 40), ("rate 0", dict(first.params, vaccination_rate=0), first.trigger + 60),
               ("rate_4096", None, vr.CASES["rate_4096"].trigger + 50), ("rate_1024", None, vr.CASES["rate_1024"].steps))
    for i, (name, params, steps) in enumerate(members):
        if i:
            sim.restart(params=_lib.default_params(**params) if params else vr.params_of(name))
        got = sim.run(steps)
        state = sim.download_state()
        try:
            if params:
                want = OracleRun(pop, steps, steps, threads=4, **params)
                assert_same_records(got, want.records[0])
                assert want.records[0]["vaccination_active"][-1] == 1 and not want.records[0]["vaccinated_now"].any()
                for k in STATE_KEYS:
                    assert (state[k] == want.states[0][k]).all(), k
            else:
                tr = vr.trace(name)
                assert_same_records(got, tr["records"][:steps])
                assert_same_records(sim.records_so_far(), tr["records"][:steps])
                assert (state["status"] == tr["status"][steps - tr["first"]]).all(), "status"
                assert ((state["eligible"] != 0) == tr["eligible"][steps - tr["first"]]).all(), "eligible"
                if steps == vr.CASES[name].steps:
                    for k in STATE_KEYS:
                        assert (state[k] == tr["states"][-1][k]).all(), k
        except AssertionError as e:
            raise AssertionError("member %d (%s): %s" % (i, name, e)) from e
    sim.close()


# ---- d. the consumers of the replayed walk ------------------------------------------------------------------------------------------
BURDEN_TABLES = dict(burden.table_set_t(), admit_thr=burden.percent((5, 10, 20, 40, 70)), death_thr=burden.percent((0, 2, 5, 15, 40)))


@functools.lru_cache(maxsize=None)
def references(name):
    case = vr.CASES[name]
    pop, ep, n = case.pop, vr.params_of(name), case.steps
    lab = hh.labels(pop, N_GROUPS)
    sref = setting.reference(pop, ep, n)
    tref = tree.reference(pop, ep, n, sref)
    sus = hh.sus_until(pop, ep, n)
    jm = hh.all_pairs(tref, pop)
    _, seen = contact.walk(pop, ep, n, tref, lab, N_GROUPS)
    one = contact.labels_of(pop, 1)
    return dict(pop=pop, ep=ep, n=n, labels=lab, tables=asr.reference_tables(pop, ep, n), groups=_group_ref.reference_tables(pop, ep, lab, N_GROUPS, n),
                sref=sref, tref=tref, sus=sus, jm=jm, one=one,
                rule=contact.rule(pop, ep, n, tref, lab, N_GROUPS, seen["vax"], seen["buses"], seen["world"]),
                rule_all=contact.rule(pop, ep, n, tref, one, 1, seen["vax"], seen["buses"], seen["world"]),
                burden=burden.build(pop, ep, lab, N_GROUPS, n, tables=BURDEN_TABLES))


def check_consumers(name, what):
    case, w = vr.CASES[name], references(name)
    pop, n, lab = w["pop"], w["n"], w["labels"]
    assert_same_records(w["tables"]["records"], vr.trace(name)["records"])
    sim = Simulator(pop, setting.copy_params(w["ep"]))
    sim.set_groups(lab, N_GROUPS)
    sim.set_burden(BURDEN_TABLES)
    assert_same_records(sim.run(n), w["tables"]["records"])
    inside = case.trigger + 5                                              # a strided window that starts inside the programme
    for where, status in asr.TABLES:
        same(sim.area_status_series(status, where), asr.expected(w["tables"], where, status, n), "%s: %s by %s" % (what, status, where))
        want = asr.expected(w["tables"], where, status, n, first_step=inside, stride=7)
        assert len(want) >= 10
        same(sim.area_status_series(status, where, first_step=inside, stride=7), want, "%s: %s by %s, stride 7 from step %d" % (what, status, where, inside))
    for k, status in enumerate(asr.STATUS):
        same(sim.group_series(status), w["groups"]["status_rows"][:, :, k], "%s: %s rows by group" % (what, status))
    same(sim.group_series("exposures"), w["groups"]["exposure_rows"], what + ": exposure rows by group")
    for status in curve.STATUS:                                            # (every status the call knows)
        for kw in (dict(), dict(first_step=inside, last_step=n - 3, threshold=3)):
            got = sim.curve_summary("home", status, **kw)
            want = curve.summarize(curve.curves(w["tables"]["home"], status), kw.get("first_step", 1), kw.get("last_step", n), kw.get("threshold", 1))
            for key in curve.KEYS:
                same(got[key], want[key], "%s: curve summary of %s, %s, %s" % (what, status, key, kw))
    got_setting, got_building = sim.exposure_settings()
    same(got_setting, w["sref"]["setting"], what + ": setting per citizen")
    same(got_building, w["sref"]["building"], what + ": building per citizen")
    infector, k, gen = sim.transmission_tree()
    same(k, w["tref"]["n_candidates"], what + ": candidates per citizen")
    same(infector, w["tref"]["infector"], what + ": infector per citizen")
    same(gen, w["tref"]["generation"], what + ": generation per citizen")
    # (cohorts whose infectious period straddles the programme's start: their housemates leave the risk set by vaccination)
    for first, last in ((0, n), (case.trigger - 150, case.trigger - 60)):
        for where, g in (("all", 0), ("group", N_GROUPS)):
            at, sec = sim.household_sar(where, first, last, complete=False)
            want = hh.pairs(w["tref"], pop, w["ep"], w["sus"], first, last, lab, g, jm=w["jm"]) if g else hh.pairs(w["tref"], pop, w["ep"], w["sus"], first, last, jm=w["jm"])
            same(at, want[0], "%s: household pairs at risk by %s, cohorts %d..%d" % (what, where, first, last))
            same(sec, want[1], "%s: secondary cases by %s, cohorts %d..%d" % (what, where, first, last))
    for first, last in ((1, n), (case.trigger - 20, case.trigger + 40)):
        for where, rule, labels, g in (("all", w["rule_all"], w["one"], 1), ("group", w["rule"], lab, N_GROUPS)):
            got = sim.contact_hours(where, None, first, last, per_case=where == "all")
            tag = "%s: contact-hours by %s, steps %d..%d" % (what, where, first, last)
            same(got["hours"], rule.window(first, last), tag + ": hours")
            same(got["transmissions"], contact.transmissions(w["tref"], labels, g, first, last), tag + ": transmissions")
            if where == "all":
                same(got["per_case"], rule.per_case(first, last), tag + ": per case")
    check_burden(sim, w["burden"]["cols"], burden.at_stop(w["burden"]["full"], n), n, what)
    state = sim.download_state()
    for key in STATE_KEYS:
        same(state[key], w["tables"]["final_state"][key], "%s: state untouched: %s" % (what, key))
    return sim


@pytest.mark.parametrize("name", vr.REPLAYED)
def test_the_consumers_of_the_replayed_walk(name):
    w = references(name)
    run = w["burden"]["run"]
    if name == "rate_1024":
        assert int(run["vax_exposed"].sum()) >= 1000 and int(run["vax_infected"].sum()) >= 50 and int(w["sref"]["housemate_vaccinated"].sum()) >= 10
    check_consumers(name, name).close()


@pytest.mark.parametrize("name", vr.REPLAYED)
def test_the_consumers_with_grids_capped_to_one_workgroup(name, monkeypatch):
    monkeypatch.setenv("ESIM_GRID_CAP", "1")
    sim = check_consumers(name, name + ", ESIM_GRID_CAP=1")
    clipped = {site: r for site, r in sim.debug_launches().items() if r["clipped"]}
    sim.close()
    assert len(clipped) >= 10 and max(r["max_trips"] for r in clipped.values()) >= vr.CASES[name].pop.n_citizens // 256, clipped


# ---- e. a seam across the two arms ------------------------------------------------------------------------------------------------
TOWN_TRIGGER, TOWN_ELIGIBLE = vr.TOWN_TRIGGER, vr.TOWN_ELIGIBLE            # (tests/test_vax_rates.py checks them over the oracle)
TOWN_BASE = dict(vr.BASE, vaccination_threshold=vr.TOWN_THRESHOLD)
EARLY = vr.CASES["rate_8192_early"]
SEAMS = {
    # name: (world, parameters up to the seam, the seam's step, what the rollback changes, steps in all, which arm runs before and behind)
    "8192_to_25": ("W40", EARLY.params, EARLY.trigger + 30, dict(vaccination_rate=25, seed=4242), EARLY.trigger + 90, ("walk", "walk")),
    "25_to_8192": ("W40", dict(EARLY.params, vaccination_rate=25), EARLY.trigger + 30, dict(vaccination_rate=8192, seed=4242), EARLY.trigger + 90, ("walk", "walk")),
    # the whole set at the trigger because eligible_count == rate exactly, the seam right behind that step: the replay has to
    # decide that step under the old rate (under the new one it would be walked) and walk the later ones under the new
    "whole_set_to_walk": ("town", dict(TOWN_BASE, vaccination_rate=TOWN_ELIGIBLE), TOWN_TRIGGER,
                          dict(vaccination_rate=4097, seed=4242), TOWN_TRIGGER + 40, ("whole", "walk")),
    "walk_to_whole_set": ("town", dict(TOWN_BASE, vaccination_rate=25), TOWN_TRIGGER + 20,
                          dict(vaccination_rate=8192, seed=4242), TOWN_TRIGGER + 60, ("walk", "whole")),
}


def seam_world(which):
    return vr.town() if which == "town" else vr.world(which)


@pytest.mark.parametrize("name", list(SEAMS))
def test_the_status_tables_across_a_seam_between_the_arms(name):
    """Snapshot, rollback under another rate and seed, run on.  The reference is numpy over the per-citizen state downloaded
    after every single step of the same branch, made by sequential steps of one step a call."""
    which, params, t, over, n, arms = SEAMS[name]
    pop, ep = seam_world(which), _lib.default_params(**params)
    slow = Simulator(pop, setting.copy_params(ep))
    slow.set_pipeline(0)
    states = []
    for s in range(1, n + 1):
        if s == t + 1:
            slow.snapshot(); slow.rollback(**over)
        slow.run(1)
        states.append(slow.download_state())
    slow_rec = slow.records_so_far()
    slow.close()
    # the arms the seam is about, by the records of the sequential branch
    now, elig = slow_rec["vaccinated_now"].astype(np.int64), slow_rec["eligible_count"].astype(np.int64)
    for arm, steps, rate in ((arms[0], slice(t - 1, t), params["vaccination_rate"]), (arms[1], slice(t, n), over["vaccination_rate"])):
        assert now[steps].all() and ((elig[steps] <= rate).all() if arm == "whole" else (elig[steps] > rate).all() and (now[steps] == rate).all()), (arm, rate)
    want = tables_from_states(pop, states)
    sim = Simulator(pop, setting.copy_params(ep))
    sim.run(t); sim.snapshot(); sim.run(min(50, n - t)); sim.rollback(**over); sim.run(n - t)
    assert_same_records(sim.records_so_far(), slow_rec)
    state = sim.download_state()
    for k in STATE_KEYS:
        assert (state[k] == states[-1][k]).all(), k
    for where in ("home", "current"):
        census = sim.area_census(where)
        for k, status in enumerate(asr.STATUS):
            tab = sim.area_status_series(status, where)
            same(tab, want[where][:, :, k], "%s rows by %s" % (status, where))
            assert (tab[-1] == census[:, k]).all()
        same(sim.area_status_series("vaccinated", where, first_step=t - 3, stride=5), want[where][t - 4::5, :, 4], "vaccinated rows by %s, stride 5 across the seam" % where)
    sim.close()


# ---- f. two ranks -------------------------------------------------------------------------------------------------------------------
def sharded(name, steps, **more):
    case = vr.CASES[name]
    return dict(backend="gloo", cuts="even", spec=vr.WORLDS[case.world], params=dict(case.params, max_steps=700), steps=steps, chunk=BLOCK_SHARDED,
                expect=dict(vaccinated=case.rate), **more)


BLOCK_SHARDED = 120
# One batch of PLAN_W = 4096 exchanged liveness bits can never hold 4096 or 8192 distinct eligible candidates (tests/test_vax_rates.py):
# every sharded plan fails, and every step under the programme runs coupled over the VACC_WINDOW bits -- all but two of them at
# the least, the worker asserts (and that chunks ran: those before the trigger).  Steps behind the trigger are cut to keep the
# two oracle runs of the two ranks short.
COUPLED = {name: sharded(name, vr.CASES[name].trigger + 60, expect_coupled=61 - 2) for name in ("rate_8192_early", "rate_4096")}
# 1024 a step fit one batch: sharded plans run (fewer coupled steps than steps under the programme would not show it, so the
# worker's line is read: chunks beyond the steps before the trigger)
PLANNED = sharded("rate_1024", vr.CASES["rate_1024"].trigger + 100)


@pytest.mark.parametrize("name", list(COUPLED))
def test_two_ranks_run_coupled_where_one_batch_cannot_reach_the_rate(name):
    outs = launch(2, COUPLED[name])
    assert all("ok" in o for o in outs), outs


def test_two_ranks_plan_chunks_at_1024_a_step():
    outs = launch(2, PLANNED)
    assert all("ok" in o for o in outs), outs
    for o in outs:
        line = [l for l in o.splitlines() if " ok: " in l][-1]
        in_chunks = int(line.split("(")[1].split(" in chunks")[0])
        assert in_chunks > vr.CASES["rate_1024"].trigger + 8, line          # chunks under the programme too
