"""Outputs by citizen group: the ABI surface, the label builders of Population, and the numpy reference of
tests/_group_ref.py checked against the oracle's own records before the GPU tests trust it.  No GPU needed."""
import ctypes as C
import os
import re

import numpy as np

import _area_ref
import _group_ref
import _oracle
from epidemicsimulator_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARITY = {"esim_set_groups": 3, "esim_group_census": 2, "esim_group_series": 6}
STATUS = ("susceptible", "exposed", "infected", "recovered", "vaccinated")


def test_header_library_and_binding_have_the_three_entry_points():
    header = open(os.path.join(ROOT, "include", "esim.h")).read()
    bare = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = C.CDLL(_lib.LIB_PATH)
    bound = _lib.load()
    for name, arity in ARITY.items():
        proto = re.search(r"\bint\s+%s\s*\((.*?)\);" % name, bare, re.S)
        assert proto, "%s is not declared in include/esim.h" % name
        assert len([a for a in proto.group(1).split(",") if a.strip()]) == arity, name
        assert hasattr(lib, name), "%s is not exported by libesim.so" % name
        assert name in _lib.SYMBOLS
        assert len(getattr(bound, name).argtypes) == arity, name
    assert re.search(r"#define\s+ESIM_MAX_GROUPS\s+1024\b", header)
    assert re.search(r"\bESIM_BY_GROUP\s*=\s*2\b", header) and re.search(r"\bESIM_GROUP_SERIES_EXPOSURES\s*=\s*5\b", header)
    assert (_lib.BY_GROUP, _lib.MAX_GROUPS, _lib.GROUP_SERIES_EXPOSURES) == (2, 1024, 5)


def test_age_bands_and_occupation_groups_on_fixture_a():
    pop, _ = _area_ref.fixture_a()
    labels, n_groups = pop.age_bands(_group_ref.AGE_EDGES)
    assert labels.dtype == np.uint16 and labels.shape == (pop.n_citizens,) and n_groups == len(_group_ref.AGE_EDGES) + 1 == 8
    assert (labels == np.digitize(pop.age, _group_ref.AGE_EDGES)).all()
    # a boundary lands where np.digitize puts it: age == edge opens the next band
    for k, edge in enumerate(_group_ref.AGE_EDGES):
        assert (pop.age == edge).any() and (pop.age == edge - 1).any()
        assert (labels[pop.age == edge] == k + 1).all() and (labels[pop.age == edge - 1] == k).all()
    assert int(labels.max()) < n_groups
    sizes = np.bincount(labels, minlength=n_groups)
    assert int(sizes.sum()) == pop.n_citizens and (sizes > 0).all()
    occ, n_occ = pop.occupation_groups()
    assert occ.dtype == np.uint16 and (occ == pop.occupation).all() and n_occ == int(pop.occupation.max()) + 1
    assert int(occ.max()) < n_occ and int(np.bincount(occ, minlength=n_occ).sum()) == pop.n_citizens


def check_tables(ref, pop, n_steps):
    rec, rows = ref["records"], ref["status_rows"]
    # every row sums over the statuses to the group sizes, at every step
    assert (rows.sum(axis=2) == ref["sizes"][None, :]).all()
    assert int(ref["sizes"].sum()) == pop.n_citizens
    # the exposure rows sum over the groups to the record's two kinds
    assert (ref["exposure_rows"].sum(axis=1) == rec["exposures_building"] + rec["exposures_bus"]).all()
    # Infected and Recovered over the groups against the records wherever the step vaccinated nobody (a record holds the
    # census before its step's vaccinations, the rows the state after them)
    quiet = rec["vaccinated_now"] == 0
    for k, name in enumerate(STATUS):
        assert (rows[:, :, k].sum(axis=1)[quiet] == rec[name][quiet]).all(), name
    assert (rows[:, :, 4].sum(axis=1)[:-1] == rec["vaccinated"][1:]).all()
    seeds = np.unique(pop.seeds)
    assert int(ref["initial"][:, 2].sum()) == len(seeds) and int(ref["initial"][:, 0].sum()) == pop.n_citizens - len(seeds)


def test_reference_tables_agree_with_the_oracles_own_records():
    pop, ep, labels, n_groups = _group_ref.fixture_a_groups()
    n = _area_ref.FIXTURE_A_STEPS
    ref = _group_ref.reference_tables(pop, ep, labels, n_groups, n)
    check_tables(ref, pop, n)
    rec = ref["records"]
    # the fixture of tests/test_area_outputs.py: both exposure kinds, a lockdown, a vaccination programme inside the run
    assert int(rec["exposures_building"].sum()) == 799 and int(rec["exposures_bus"].sum()) == 11
    assert rec["lockdown"].any() and rec["vaccination_active"].any() and not rec["vaccination_active"][0]
    assert ref["status_rows"][-1].sum(axis=0).tolist() == [0, 0, 0, 722, 19278]
    # every group takes part in the epidemic
    assert (ref["exposure_rows"].sum(axis=0) > 0).all()


def test_high_prevalence_parameters_take_most_of_the_population_out_of_susceptible():
    pop, _, labels, n_groups = _group_ref.fixture_a_groups()
    ep = _lib.default_params(**_group_ref.HIGH_PREVALENCE)
    n = _group_ref.HIGH_PREVALENCE_STEPS
    ref = _group_ref.reference_tables(pop, ep, labels, n_groups, n)
    check_tables(ref, pop, n)
    rec = ref["records"]
    share = rec["infected"].max() / pop.n_citizens
    print("high prevalence: peak Infected share %.3f at step %d, Susceptible left %d" % (share, int(np.argmax(rec["infected"])) + 1, int(rec["susceptible"][-1])))
    assert share > 0.30
    assert rec["susceptible"][-1] < pop.n_citizens // 20
    # the programme starts inside the wave: somebody who had been exposed is among the vaccinated
    assert rec["vaccination_active"].any() and rec["exposures_bus"].sum() > 0
    exposed_ever = (ref["exposure_rows"].sum(dtype=np.int64) + len(np.unique(pop.seeds)))
    assert exposed_ever + int(ref["status_rows"][-1][:, 4].sum()) > pop.n_citizens - int(ref["status_rows"][-1][:, 0].sum())
