"""The replayed outputs at the edges of esim_params (tests/_replay_edges.py; tests/test_replay_edges.py checks on the CPU that
no case is inert): every replay family of the device -- a. exposures by setting, b. the transmission tree, c. chains and the
infectious-age profile, d. household outbreaks, e. area flows and the invasion tree, f. transmission events, g. contact-hours,
h. place outbreaks, i. curve summaries -- against its numpy reference over the CPU oracle, and j. the identities that need no
reference, in all 27 cases.  Every comparison is exact integer equality; the attack rates and contact rates are compared
through the tallies they are quotients of.  Six cases run again at pipeline level 0 on a permuted population and once more with
the output grids capped to one workgroup.  One more test pins the documented limit of the replays: a household that is
somebody's work place."""
import numpy as np
import pytest

import _chain_ref as chain
import _contact_ref as contact
import _curve_ref as curve
import _event_ref as event
import _flow_ref as flow
import _household_ref as hh
import _oracle
import _param_edges as pe
import _place_ref as place
import _replay_edges as edges
import _setting_ref as setting
import _tree_ref as tree
from epidemicsimulator_amd import Simulator, _lib
from test_exposure_settings_gpu import at_work_bits, same

pytestmark = pytest.mark.gpu

ESTATE = -4
H, W, S, T = edges.H, edges.W, edges.S, edges.T
PARTIAL = ("household", "transport")             # the partial setting mask of the flows, and its bits
PARTIAL_MASK = (1 << H) | (1 << T)
LIMIT_WORDS = b"household that is the work place"


def started(w, level=None):
    sim = Simulator(w.pop, setting.copy_params(w.ep))
    if level is not None:
        sim.set_pipeline(level)
    sim.set_groups(w.labels, w.n_groups)
    rec = sim.run(w.n)
    same(rec["exposures_building"], w.sref["records"]["exposures_building"], "the run itself vs the oracle: building exposures")
    same(rec["exposures_bus"], w.sref["records"]["exposures_bus"], "the run itself vs the oracle: bus exposures")
    return sim, rec


def windows(w):
    return (1, w.n), edges.inner_window(w)


# ---- a. exposures by setting ----------------------------------------------------------------------------------------------------
def check_settings(sim, w, what):
    pop, ref, n = w.pop, w.sref, w.n
    got_setting, got_building = sim.exposure_settings()
    same(got_setting, ref["setting"], what + " a: setting per citizen")
    same(got_building, ref["building"], what + " a: building per citizen")
    for where in ("setting", "home", "group"):
        for kw in (dict(), dict(first_step=3, stride=24)):
            want = setting.rows(ref, pop, where, 0xF, kw.get("first_step", 1), None, kw.get("stride", 1), w.labels, w.n_groups)
            same(sim.setting_series(where, **kw), want, "%s a: rows by %s, %s" % (what, where, kw))
    for first, last in windows(w):
        same(sim.building_exposures(first, last), setting.building_counts(ref, pop, first, last), "%s a: buildings of steps %d..%d" % (what, first, last))


# ---- b. who infected whom -------------------------------------------------------------------------------------------------------
def check_tree(sim, w, what):
    pop, ref = w.pop, w.tref
    infector, k, gen = sim.transmission_tree()
    same(k, ref["n_candidates"], what + " b: candidates per citizen")
    same(infector, ref["infector"], what + " b: infector per citizen")
    same(gen, ref["generation"], what + " b: generation per citizen")
    for where in ("all", "home", "group"):
        cases, off = sim.reproduction_series(where)
        want = tree.reproduction_rows(ref, pop, where, 0, None, 24, w.labels, w.n_groups)
        same(cases, want[0], "%s b: cohort sizes by %s" % (what, where))
        same(off, want[1], "%s b: offspring by %s" % (what, where))
    same(sim.mixing_matrix(), tree.mixing_matrix(ref, pop, w.labels, w.n_groups), what + " b: mixing matrix")


# ---- c. chains and the infectious-age profile -------------------------------------------------------------------------------------
def check_chains(sim, w, what):
    lineage, desc = sim.transmission_chains()
    same(lineage, w.chains["lineage"], what + " c: lineage per citizen")
    same(desc, w.chains["descendants"], what + " c: descendants per citizen")
    table = sim.outbreaks()
    for k in ("seeds", "size", "depth", "last_step"):
        same(table[k], w.chains[k], "%s c: %s per index case" % (what, k))
    for first, last in windows(w):
        same(sim.transmission_ages(first, last), chain.ages(w.tref, w.pop, w.ep, first, last), "%s c: infectious ages of steps %d..%d" % (what, first, last))


# ---- d. household outbreaks -----------------------------------------------------------------------------------------------------
def check_households(sim, w, what):
    got = sim.household_outbreaks()
    for k in ("cases", "introductions", "first_step"):
        same(got[k], w.households[k], "%s d: %s per household" % (what, k))
    final_size, intro_size = sim.household_final_sizes()
    want = hh.final_sizes(w.households)
    same(final_size, want[0], what + " d: final sizes")
    same(intro_size, want[1], what + " d: introductions by household size")
    for first, last in ((0, w.n), edges.cohort_window(w)):
        for where, g in (("all", 0), ("group", w.n_groups)):
            at, sec = sim.household_sar(where, first, last, complete=False)
            want = w.pairs(first, last, g)
            same(at, want[0], "%s d: at risk by %s, cohorts %d..%d" % (what, where, first, last))
            same(sec, want[1], "%s d: secondary by %s, cohorts %d..%d" % (what, where, first, last))


# ---- e. area flows, imports, the invasion tree ----------------------------------------------------------------------------------
def check_flows(sim, w, what):
    pop, ref = w.pop, w.tref
    first, last = edges.inner_window(w)
    partial = flow.flows(ref, pop, PARTIAL_MASK, first, last), flow.imports(ref, pop, PARTIAL_MASK, first, last)
    for settings, mask, a, b, (want_flows, want_imports) in ((None, flow.ALL, 1, w.n, (w.flows, w.imports)), (PARTIAL, PARTIAL_MASK, first, last, partial)):
        tag = "%s e: mask %x, steps %d..%d" % (what, mask, a, b)
        for g, want, k in zip(sim.area_flows(settings, a, b), want_flows, ("src", "dst", "count")):
            same(g, want, "%s: flows %s" % (tag, k))
        got = sim.area_imports(settings, a, b)
        for k in ("local", "imported", "exported"):
            same(got[k], want_imports[k], "%s: %s" % (tag, k))
    got, want = sim.area_invasion(), w.invasion
    for k in ("first_case", "step", "source_area", "setting"):
        same(got[k], want[k], "%s e: invasion %s" % (what, k))


# ---- f. transmission events -----------------------------------------------------------------------------------------------------
def check_events(sim, w, what):
    for min_size in (1, 2):
        got, want = sim.transmission_events(min_size=min_size), event.events(w.event_world, min_size=min_size)
        for k in event.KEYS:
            same(got[k], want[k], "%s f: events of at least %d: %s" % (what, min_size, k))
    same(sim.event_sizes(), event.sizes(w.event_world), what + " f: event sizes")


# ---- g. contact-hours -----------------------------------------------------------------------------------------------------------
def check_contacts(sim, w, what):
    one = contact.labels_of(w.pop, 1)
    for i, (first, last) in enumerate(windows(w)):
        for where, rule, lab, g in (("all", w.contact_rule_all, one, 1), ("group", w.contact_rule, w.labels, w.n_groups)):
            per_case = (where == "all") == (i == 0)          # per case: the whole run by all, the window by group
            got = sim.contact_hours(where, None, first, last, per_case=per_case)
            tag = "%s g: by %s, steps %d..%d" % (what, where, first, last)
            same(got["hours"], rule.window(first, last), tag + ": hours")
            same(got["transmissions"], contact.transmissions(w.tref, lab, g, first, last), tag + ": transmissions")
            assert (got["transmissions"] <= got["hours"]).all(), tag
            if per_case:
                same(got["per_case"], rule.per_case(first, last), tag + ": per case")


# ---- h. place outbreaks ---------------------------------------------------------------------------------------------------------
def check_places(sim, w, what):
    for kind in ("work", "school"):
        got, want = sim.place_outbreaks(kind), w.place_outbreaks[kind]
        for k in ("members", "cases", "introductions", "first_step"):
            same(got[k], want[k], "%s h: %s per place, %s" % (what, k, kind))
        for g, t, k in zip(sim.place_sizes(kind), place.sizes(want), ("final sizes", "introductions by size")):
            same(g, t, "%s h: %s, %s" % (what, k, kind))
    # the attack rate of the schools is that of their rooms (esim_place_sar counts class-mates, not school-mates)
    for kind in ("work", "room"):
        for first, last in ((0, w.n), edges.cohort_window(w)):
            for where, g in (("all", 0), ("group", w.n_groups)):
                at, sec = sim.place_sar(kind, where, first, last, complete=False)
                want = w.place_pairs(kind, first, last, g)
                same(at, want[0], "%s h: %s at risk by %s, cohorts %d..%d" % (what, kind, where, first, last))
                same(sec, want[1], "%s h: %s secondary by %s, cohorts %d..%d" % (what, kind, where, first, last))


# ---- i. curve summaries ---------------------------------------------------------------------------------------------------------
def check_curves(sim, w, what):
    x = curve.curves(w.status_rows, "infected")
    first, last = edges.inner_window(w)
    for kw in (dict(), dict(first_step=first, last_step=last, threshold=3)):
        got = sim.curve_summary("home", "infected", **kw)
        want = curve.summarize(x, kw.get("first_step", 1), kw.get("last_step", w.n), kw.get("threshold", 1))
        for k in curve.KEYS:
            same(got[k], want[k], "%s i: %s by home, %s" % (what, k, kw))


# ---- j. what holds without a reference --------------------------------------------------------------------------------------------
def check_identities(sim, w, rec, what):
    """Those of test_exposure_settings_gpu.identities, without its demand that commuters were exposed both at work and at home:
    tests/test_replay_edges.py asks that of every case that can meet it."""
    pop = w.pop
    got_setting, got_building = sim.exposure_settings()
    rows = sim.setting_series("setting")
    same(rows.sum(axis=1, dtype=np.int64), rec["exposures_building"].astype(np.int64) + rec["exposures_bus"], what + " j: the four columns summed vs the records")
    same(rows[:, T], rec["exposures_bus"], what + " j: the transport column vs exposures_bus")
    same(rows[:, :T].sum(axis=1, dtype=np.int64), rec["exposures_building"], what + " j: the building columns vs exposures_building")
    same(sim.setting_series("home"), sim.area_status_series("incidence"), what + " j: full mask by home vs the incidence rows")
    same(sim.setting_series("group"), sim.group_series("exposures"), what + " j: full mask by group vs the group rows")
    cit, step, bus = sim.exposure_events()
    area = pop.building_area
    commuter = (pop.work_building != pop.home_building) & (area[pop.work_building] != area[pop.home_building])
    keep = (step >= 1) & (bus == 0) & commuter[cit]
    at_work = at_work_bits(sim, rec)[step[keep]]
    same(got_setting[cit[keep]] == H, ~at_work, what + " j: commuters exposed at home iff not at work")
    same(np.where(at_work, pop.work_building[cit[keep]], pop.home_building[cit[keep]]), got_building[cit[keep]], what + " j: their buildings")
    return int(at_work.sum()), int((~at_work).sum())


def check_empty(sim, w, what):
    """A run without one exposure: every table of transmissions is empty, and no call complained."""
    n = w.pop.n_citizens
    got_setting, got_building = sim.exposure_settings()
    assert (got_setting == _lib.SETTING_NONE).all() and (got_building == _lib.NO_ROOM).all(), what
    infector, k, gen = sim.transmission_tree()
    assert (infector == _lib.NO_INFECTOR).all() and not k.any() and int((gen == 0).sum()) == edges.n_index_cases() and int((gen == _lib.NEVER).sum()) == n - edges.n_index_cases(), what
    assert not sim.setting_series("setting").any() and not sim.building_exposures().any() and not sim.mixing_matrix().any(), what
    assert not sim.outbreaks()["size"].any() and not sim.transmission_ages().any(), what
    assert all(a.size == 0 for a in sim.area_flows()) and not any(v.any() for v in sim.area_imports().values()), what
    assert all(v.size == 0 for v in sim.transmission_events().values()) and not sim.event_sizes().any(), what
    assert not sim.household_sar("all", 0, w.n, complete=False)[1].any() and not sim.contact_hours()["transmissions"].any(), what
    hho = sim.household_outbreaks()
    assert int(hho["cases"].sum()) == edges.n_index_cases() and (hho["cases"] == hho["introductions"]).all(), what


def snapshot_of(sim):
    return sim.download_state(), sim.records_so_far(), sim.exposure_events(), sim.area_census("home")


def check_case(sim, w, rec, what):
    before = snapshot_of(sim)
    check_settings(sim, w, what)
    check_tree(sim, w, what)
    check_chains(sim, w, what)
    check_households(sim, w, what)
    check_flows(sim, w, what)
    check_events(sim, w, what)
    check_contacts(sim, w, what)
    check_places(sim, w, what)
    check_curves(sim, w, what)
    commuters = check_identities(sim, w, rec, what)
    if w.name in edges.NO_EXPOSURES:
        check_empty(sim, w, what)
    after = snapshot_of(sim)
    for k in before[0]:
        same(after[0][k], before[0][k], what + ": state untouched: " + k)
    assert (after[1] == before[1]).all(), what + ": records untouched"
    for a, b in zip(after[2], before[2]):
        same(a, b, what + ": exposure log untouched")
    same(after[3], before[3], what + ": census untouched")
    return commuters


# ---- the 27 cases ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(pe.CASES))
def test_every_replay_matches_its_reference(name):
    w = edges.cached(name)
    sim, rec = started(w)
    at_work, at_home = check_case(sim, w, rec, name)
    f = edges.facts(w)
    assert (at_work, at_home) == (f["commuters_at_work"], f["commuters_at_home"])
    sim.close()


@pytest.mark.parametrize("name", edges.SECOND_FORM)
def test_sequential_steps_on_the_permuted_world(name):
    w = edges.cached(name, True)
    sim, rec = started(w, level=0)
    check_case(sim, w, rec, name + ", permuted, level 0")
    sim.close()


@pytest.mark.parametrize("name", edges.SECOND_FORM)
def test_grids_capped_to_one_workgroup(name, monkeypatch):
    monkeypatch.setenv("ESIM_GRID_CAP", "1")
    w = edges.cached(name)
    sim, rec = started(w)
    check_case(sim, w, rec, name + ", ESIM_GRID_CAP=1")
    launches = sim.debug_launches()
    sim.close()
    clipped = {site: r for site, r in launches.items() if r["clipped"]}
    # 3 000 citizens are twelve trips of one workgroup of 256: the strides of the per-citizen kernels were walked
    assert len(clipped) >= 10 and max(r["max_trips"] for r in clipped.values()) >= 3000 // 256, launches


# ---- the documented limit: a household that is somebody's work place ------------------------------------------------------------
def replay_calls(sim, n):
    """One call of every replay family that derives the setting of an exposure, by name."""
    return {"esim_exposure_settings": lambda: sim.exposure_settings(), "esim_setting_series": lambda: sim.setting_series("setting"),
            "esim_building_exposures": lambda: sim.building_exposures(), "esim_transmission_tree": lambda: sim.transmission_tree(),
            "esim_offspring": lambda: sim.offspring(), "esim_reproduction_series": lambda: sim.reproduction_series("all"),
            "esim_mixing_matrix": lambda: sim.mixing_matrix(), "esim_transmission_chains": lambda: sim.transmission_chains(),
            "esim_outbreaks": lambda: sim.outbreaks(), "esim_transmission_ages": lambda: sim.transmission_ages(),
            "esim_household_outbreaks": lambda: sim.household_outbreaks(), "esim_household_final_sizes": lambda: sim.household_final_sizes(),
            "esim_household_sar": lambda: sim.household_sar("all", 0, n, complete=False), "esim_area_flows": lambda: sim.area_flows(),
            "esim_area_imports": lambda: sim.area_imports(), "esim_area_invasion": lambda: sim.area_invasion(),
            "esim_lineage_areas": lambda: sim.lineage_areas(), "esim_transmission_events": lambda: sim.transmission_events(),
            "esim_contact_hours": lambda: sim.contact_hours(), "esim_place_outbreaks": lambda: sim.place_outbreaks("work"),
            "esim_place_sizes": lambda: sim.place_sizes("work"), "esim_place_sar": lambda: sim.place_sar("work", "all", 0, n, complete=False)}


def test_a_household_that_is_a_work_place_is_refused_by_the_replays_and_by_nothing_else():
    """_param_edges.world(): people work in somebody's household.  The replays count residents only into the Infected of a
    household (DESIGN 16 "Limits"), so on this world they would credit exposures to the wrong setting; every one of them
    refuses with ESIM_ESTATE and names the limit.  The step path and the outputs that replay no draw take the world as before."""
    pop, n = pe.world(), pe.N_STEPS
    away = pop.work_building != pop.home_building
    assert (pop.building_type[pop.work_building[away]] == _lib.HOUSEHOLD).any()
    ep = _lib.default_params(**pe.BASE)
    ref = setting.reference(pop, ep, n)
    sim = Simulator(pop, setting.copy_params(ep))
    sim.set_groups(*edges.labels_of(pop))
    rec = sim.run(n)
    for k in ("exposures_building", "exposures_bus", "infected", "vaccinated", "lockdown"):
        same(rec[k], ref["records"][k], "the step path on the world of the parameter edges: " + k)
    for who, call in replay_calls(sim, n).items():
        with pytest.raises(_lib.EsimError) as e:
            call()
        assert e.value.code == ESTATE, (who, str(e.value))
        assert LIMIT_WORDS in sim.lib.esim_last_error(sim._ctx), (who, str(e.value))
    # what replays no household draw answers as before
    orc = _oracle.Oracle(pop, _oracle.params_from_esim(ep))
    orc.set_threads(4)
    orc.run(n)
    step, where = orc.exposures()
    orc.close()
    cit, got_step, bus = sim.exposure_events()
    c = np.flatnonzero(step > 0)
    order = np.lexsort((c, step[c]))
    same(cit, c[order], "exposure log: citizens")
    same(got_step, step[c][order], "exposure log: steps")
    same(bus != 0, where[c][order] == setting.BUS_AREA, "exposure log: bus flags")
    status_rows = curve.reference_rows(pop, ep, n, "home")["status_rows"]
    got, want = sim.curve_summary("home", "infected"), curve.summarize(curve.curves(status_rows, "infected"))
    for k in curve.KEYS:
        same(got[k], want[k], "curve summary by home: " + k)
    same(sim.area_status_series("infected"), status_rows[:, :, _lib.INFECTED], "status rows by home")
    sim.close()
