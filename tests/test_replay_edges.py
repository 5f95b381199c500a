"""CPU side of the replay edges (tests/_replay_edges.py): on the builder-shaped world every case of tests/_param_edges.py still
does what it is meant to, reaches every setting it can reach with enough exposures for a wrong replay to show, and is explained
completely by the references -- so that the GPU cases (tests/test_replay_edges_gpu.py) cannot pass vacuously.  A fixture that
stops reaching its edge fails here."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import _contact_ref as contact
import _param_edges as pe
import _replay_edges as edges
import _setting_ref as setting
from epidemicsimulator_amd import _lib
from test_exposure_settings_gpu import at_work_bits

CASES = list(pe.CASES)


def test_importing_the_module_needs_no_library():
    # the import and the tables in a fresh interpreter to which libesim.so does not exist (world() calls the library's builder)
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, ESIM_LIB=os.path.join(here, "no-such-library.so"), PYTHONPATH=os.pathsep.join([os.path.dirname(here), here]))
    code = ("import os; import _replay_edges as e; from epidemicsimulator_amd import _lib; assert not os.path.exists(_lib.LIB_PATH); "
            "print(len(e.pe.CASES), len(e.SECOND_FORM), sorted(e.OVERRIDES), e.params_dict('hours_22_6')['start_hour'])")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.split("\n")[0] == "27 6 ['hours_1_23'] 22"


def test_the_world_is_one_the_replays_accept():
    pop = edges.world()
    assert (pop.n_citizens, pop.n_areas, pop.n_buildings, pop.n_rooms) == (3000, 8, 459, 61)
    assert (np.diff(pop.home_building.astype(np.int64)) >= 0).all()                      # home-sorted
    # no household is the work place of a citizen that does not live in it (DESIGN 16 "Limits") -- _param_edges.world() has such
    away = pop.work_building != pop.home_building
    assert not (pop.building_type[pop.work_building[away]] == _lib.HOUSEHOLD).any()
    other = pe.world()
    away = other.work_building != other.home_building
    assert (other.building_type[other.work_building[away]] == _lib.HOUSEHOLD).any()
    pt, compliant = (pop.flags & _lib.FLAG_USES_PUBLIC_TRANSPORT) != 0, (pop.flags & _lib.FLAG_MASK_COMPLIANT) != 0
    assert pt.any() and not pt.all() and compliant.any() and not compliant.all()
    area = pop.building_area
    assert ((area[pop.work_building] != area[pop.home_building]) & pt).sum() > 100       # routes between areas
    assert len(np.unique(pop.room[pop.room != _lib.NO_ROOM])) == pop.n_rooms
    assert edges.n_index_cases() == 10
    perm = edges.permuted_world()
    assert (np.diff(perm.home_building.astype(np.int64)) < 0).any()                      # the residents go through res_idx
    assert sorted(perm.home_building.tolist()) == sorted(pop.home_building.tolist())


def test_the_table_is_that_of_the_parameter_edges():
    assert len(CASES) == 27 and set(edges.SECOND_FORM) <= set(CASES) and len(edges.SECOND_FORM) == 6
    assert set(edges.OVERRIDES) | set(edges.GUARDS) | set(edges.WITHOUT) | set(edges.DEPTH_AT_MOST) <= set(CASES)
    for name in CASES:
        # an override never touches what the case is about
        assert not set(edges.OVERRIDES.get(name, {})) & set(pe.CASES[name].over), name
        assert edges.params_dict(name) == dict(pe.CASES[name].params, **edges.OVERRIDES.get(name, {}))
    assert [edges.depth_asked(n) for n in ("exposed_time_97", "exposed_time_200", "thresholds_0", "seed_0")] == [3, 2, 2, 3]


@pytest.mark.parametrize("name", CASES)
def test_the_case_reaches_its_edge(name):
    w = edges.cached(name)
    case, r = pe.CASES[name], w.sref["records"]
    assert len(r) == edges.N
    # the guards of the parameter edges, over the oracle's records on this world
    guards = edges.guards_of(name)
    assert len(guards) >= 3
    for g in guards:
        assert g(r), "%s: guard %s does not hold on this world (%s)" % (name, getattr(g, "__name__", "?"), case.why)
    # the guards of the replays
    f = edges.facts(w)
    print(name, f)
    allowed = edges.allowed_settings(name)
    for k in range(4):
        if k in allowed:
            assert f["per_setting"][k] >= edges.MIN_PER_SETTING, "%s: %d exposures in setting %s" % (name, f["per_setting"][k], edges.NAMES[k])
        else:
            assert f["per_setting"][k] == 0, "%s: setting %s was waived and has exposures" % (name, edges.NAMES[k])
    if name in edges.NO_EXPOSURES:
        assert f["exposures"] == 0 and not allowed
    else:
        assert f["depth"] >= edges.depth_asked(name), "%s: generation depth %d" % (name, f["depth"])
        # the commuters of the identities: exposed in a building with the at-work bit on and with it off (under a lockdown
        # from the second record on nobody is ever at work)
        assert f["commuters_at_home"] > 0
        assert f["commuters_at_work"] > 0 or name == "thresholds_0"
    # the references explain everything
    assert w.sref["unexplained"] == 0 and w.tref["empty"] == 0 and w.tref["not_infected"] == 0
    # the two contact references agree cell for cell, and the rule's bus bit is what the oracle's states show
    assert (w.contact_rule.hours == w.contact_obs.hours).all()
    aw, bus = contact.bits(w.ep, r, edges.N)
    assert (bus == w.contact_seen["bus_seen"]).all()
    # the third derivation of the at-work bit, that of the GPU identities, agrees with the rule's
    assert (at_work_bits(types.SimpleNamespace(params=w.ep), r) == aw).all()
    # ... and alone decides where the reference credits a commuter's building exposure
    pop, s = w.pop, w.sref
    area = pop.building_area
    commuter = (pop.work_building != pop.home_building) & (area[pop.work_building] != area[pop.home_building])
    who = np.flatnonzero(commuter & (s["step"] > 0) & (s["setting"] != edges.T))
    assert ((s["setting"][who] == edges.H) == ~aw[s["step"][who]]).all()
    # the per-step totals of the settings are the records'
    rows = setting.rows(w.sref, w.pop, "setting").astype(np.int64)
    assert (rows[:, :edges.T].sum(axis=1) == r["exposures_building"]).all() and (rows[:, edges.T] == r["exposures_bus"]).all()


def test_the_lockdown_of_the_longest_day_comes_and_goes():
    # the per-world override of hours_1_23: the lockdown starts and ends inside the run
    lock = edges.cached("hours_1_23").sref["records"]["lockdown"] != 0
    on = np.flatnonzero(lock)
    assert on.size and on[0] > 0 and on[-1] < edges.N - 1 and lock[on[0]:on[-1] + 1].all()


def test_every_situation_occurs_in_some_case():
    f = {name: edges.facts(edges.cached(name)) for name in CASES}
    for what in ("ties", "bus_frozen", "housemate_vaccinated"):
        assert any(v[what] > 0 for v in f.values()), what
    # where the issue saw them: ties at exposure_chance 1, frozen buses at exposed_time 95 and under the day that wraps midnight
    assert f["exposure_chance_1"]["ties"] >= 10 and f["infected_time_1"]["ties"] >= 10
    assert f["exposed_time_95"]["bus_frozen"] >= 10 and f["hours_23_2"]["bus_frozen"] >= 10
    assert sum(v["housemate_vaccinated"] > 0 for v in f.values()) >= 14


@pytest.mark.parametrize("name", edges.SECOND_FORM)
def test_the_permuted_copy_reaches_the_edge_too(name):
    # (another epidemic: the draws are keyed by the citizen's number)
    b = edges.cached(name, True)
    f = edges.facts(b)
    for k in edges.allowed_settings(name):
        assert f["per_setting"][k] >= edges.MIN_PER_SETTING, (name, edges.NAMES[k], f)
    assert f["depth"] >= edges.depth_asked(name) and f["commuters_at_home"] > 0 and f["commuters_at_work"] > 0
    assert b.sref["unexplained"] == 0 and b.tref["empty"] == 0 and b.tref["not_infected"] == 0
    assert (b.contact_rule.hours == b.contact_obs.hours).all()
