"""Ensembles over the index cases: the ABI surface, Population.draw_index_cases, and the numpy arrival reference of
tests/_arrival_ref.py checked against the oracle's own records before the GPU tests trust it.  No GPU needed."""
import ctypes as C
import os
import re

import numpy as np

import _area_ref
import _arrival_ref
import _oracle
from epidemicsimulator_amd import Population, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARITY = {"esim_restart_seeded": 4, "esim_get_seeds": 4, "esim_area_arrival": 3, "esim_ensemble_begin_arrival": 3}
EINVAL = -1


def test_header_library_and_binding_have_the_new_entry_points():
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
    assert re.search(r"#define\s+ESIM_NEVER\s+0xFFFFFFFFu", header) and _lib.NEVER == 0xFFFFFFFF == _arrival_ref.NEVER
    # a NULL context is an argument error, before anything touches a device
    p, n, buf = _lib.default_params(), C.c_uint32(7), (C.c_uint32 * 4)()
    assert bound.esim_restart_seeded(None, C.byref(p), buf, 4) == EINVAL
    assert bound.esim_get_seeds(None, buf, 4, C.byref(n)) == EINVAL
    assert bound.esim_area_arrival(None, _lib.AREA_HOME, buf) == EINVAL
    assert bound.esim_ensemble_begin_arrival(None, _lib.AREA_HOME, _lib.NEVER) == EINVAL


def hand_built(residents_per_area, n_areas=None):
    """One household building per populated area, residents_per_area[a] citizens in area a, nobody works."""
    per = np.asarray(residents_per_area)
    populated = np.flatnonzero(per)
    home = np.repeat(np.arange(populated.size), per[populated]).astype(np.uint32)
    return Population(home_building=home, work_building=home, flags=np.zeros(home.size, np.uint8),
                      building_area=populated.astype(np.uint32), building_type=np.zeros(populated.size, np.uint8),
                      n_areas=len(per) if n_areas is None else n_areas)


def test_draws_are_deterministic_and_name_residents():
    pop, _ = _area_ref.fixture_a()
    a = pop.draw_index_cases(10, 42)
    assert a.dtype == np.uint32 and a.ndim == 1 and 1 <= a.size <= 10
    assert (a == pop.draw_index_cases(10, 42)).all()
    assert not np.array_equal(pop.draw_index_cases(10, 43), a)
    big = pop.draw_index_cases(5000, 7)
    assert big.size and int(big.max()) < pop.n_citizens
    per_area = np.bincount(_arrival_ref.home_area(pop), minlength=pop.n_areas)
    assert (per_area[_arrival_ref.home_area(pop)[big]] > 0).all()
    # the residents-by-area index is built once per Population
    assert pop.residents_by_area() is pop.residents_by_area()
    order, off = pop.residents_by_area()
    assert sorted(order.tolist()) == list(range(pop.n_citizens)) and off[-1] == pop.n_citizens
    for area in (0, 17, 63):
        assert (_arrival_ref.home_area(pop)[order[off[area]:off[area + 1]]] == area).all()
    assert pop.draw_index_cases(0, 1).size == 0


def test_an_area_without_residents_yields_no_index_case():
    # the reference's `continue` (simulator_builder.rs:1125-1137): only 1 of 5 areas has residents
    pop = hand_built([0, 0, 300, 0, 0])
    assert pop.n_areas == 5
    n, p = 1000, 1 / 5
    got = pop.draw_index_cases(n, 11)
    sigma = (n * p * (1 - p)) ** 0.5
    print("populated 1 of 5 areas: %d of %d draws came back (expected %.0f +- %.1f)" % (got.size, n, n * p, 5 * sigma))
    assert abs(got.size - n * p) <= 5 * sigma
    assert got.size < n and int(got.max()) < 300
    assert hand_built([0, 0, 0]).draw_index_cases(50, 1).size == 0


def test_the_area_is_drawn_first_and_uniformly_not_the_citizen():
    pop = hand_built([10, 1000])
    got = pop.draw_index_cases(4000, 5)
    assert got.size == 4000
    small = int((got < 10).sum())
    print("two areas of 10 and 1000 residents: %d of 4000 draws from the small one" % small)
    assert 1840 <= small <= 2160                       # 2000 +- 5 sqrt(1000); a citizen-uniform rule gives about 40
    # inside an area every resident is as likely: all ten of the small area turn up
    assert np.unique(got[got < 10]).size == 10


def test_arrival_reference_agrees_with_the_oracles_own_records():
    """The issue asks that every area with a non-zero column in exposure_rows up to s has arrival <= s.  exposure_rows credits a
    building exposure to the area the citizen STANDS in (statistics.rs:186-190), the arrival map is by household: on fixture A
    2-3 areas have their only early exposures among pupils and teachers who live elsewhere.  The property that holds, and is
    checked here for every exposure, is: the HOME area of a citizen exposed at step s has arrival <= s; and the stated one
    for every exposure whose citizen stood in its home area."""
    pop, ep = _area_ref.fixture_a()
    n = _area_ref.FIXTURE_A_STEPS
    rec, step, _ = _arrival_ref.oracle_run(pop, ep, n)
    orc = _oracle.Oracle(pop, _oracle.params_from_esim(ep))
    orc.run(n)
    step2, area = orc.exposures()
    orc.close()
    assert (step2 == step).all()
    assert rec["lockdown"].any() and rec["vaccination_active"].any()
    home = _arrival_ref.home_area(pop)
    seed_areas = np.unique(home[pop.seeds])
    rows_at_home = _area_ref.exposure_rows(pop, np.where(area == home, step, 0), area, n)
    per_step = rec["exposures_building"].astype(np.int64) + rec["exposures_bus"]
    before = 0
    for s in (0, 1, 49, 50, 96, 300, 699, 700):
        a = _arrival_ref.arrival(home, pop.n_areas, step, pop.seeds, upto=s)
        assert a.dtype == np.uint32 and a.shape == (pop.n_areas,)
        assert sorted(np.flatnonzero(a == 0).tolist()) == seed_areas.tolist()
        later = (a >= 1) & (a != _arrival_ref.NEVER)
        assert (a[later] <= s).all()
        assert int(later.sum()) >= before               # entries with arrival in 1..s never decrease in s
        before = int(later.sum())
        exposed = (step >= 1) & (step <= s)
        assert int(exposed.sum()) == int(per_step[:s].sum())
        assert (a[home[exposed]] <= step[exposed]).all()
        assert (a[np.flatnonzero(rows_at_home[:s].any(axis=0))] <= s).all()
        # the first step with an exposure outside the seeds' areas is the smallest arrival behind 0
        outside = exposed & ~np.isin(home, seed_areas)
        assert (int(a[later].min()) if later.any() else None) == (int(step[outside].min()) if outside.any() else None)
    assert before > 0 and (_arrival_ref.arrival(home, pop.n_areas, step, pop.seeds, upto=50) == _arrival_ref.NEVER).any()
    full = _arrival_ref.arrival(home, pop.n_areas, step, pop.seeds)
    assert (full == _arrival_ref.arrival(home, pop.n_areas, step, pop.seeds, upto=n)).all()
