"""esim_area_status_series without a GPU: the entry point exists and refuses a null context, and the numpy reference that the
GPU tests compare against (tests/_area_status_ref.py) is pinned against the oracle's own records on fixture A."""
import ctypes as C

import numpy as np

import _area_ref
import _area_status_ref
from epidemicsimulator_amd import _lib

S, E, I, R, V = range(5)


def test_the_library_exports_the_entry_point_and_refuses_a_null_context():
    lib = _lib.load()
    assert "esim_area_status_series" in _lib.SYMBOLS and hasattr(lib, "esim_area_status_series")
    fn = lib.esim_area_status_series
    assert fn.restype is C.c_int and len(fn.argtypes) == 7
    assert _lib.AREA_SERIES_INCIDENCE == 5
    out = np.zeros(4, np.uint32)
    assert fn(None, _lib.AREA_HOME, _lib.INFECTED, 1, 1, 1, out.ctypes.data_as(C.POINTER(C.c_uint32))) == -1      # ESIM_EINVAL


def test_the_reference_tables_agree_with_the_oracles_records():
    pop, ep, ref = _area_status_ref.fixture_a_tables()
    rec, n = ref["records"], _area_ref.FIXTURE_A_STEPS
    assert rec["lockdown"].any() and rec["vaccination_active"].any() and pop.n_areas == 64
    residents = np.bincount(pop.building_area[pop.home_building], minlength=pop.n_areas)
    assert ref["home"].shape == ref["current"].shape == (n, pop.n_areas, 5) and ref["incidence"].shape == (n, pop.n_areas)
    assert (ref["home"].sum(axis=2) == residents[None, :]).all()
    assert (ref["current"].sum(axis=(1, 2)) == pop.n_citizens).all()
    assert (ref["current"].sum(axis=2) != residents[None, :]).any()                     # somebody stands elsewhere at some step
    # A record holds the census taken BEFORE the step's vaccinations, the rows the state after them: the Vaccinated of step s
    # are what the NEXT record reports.  `vaccinated_now` counts the draws of the step, and a draw can name a citizen twice
    # (fixture A: 1530 draws, 1405 citizens), so vaccinated + vaccinated_now is an upper bound, met by the programme's first step.
    bound = rec["vaccinated"].astype(np.int64) + rec["vaccinated_now"]
    first = int(np.argmax(rec["vaccination_active"]))
    for where in ("home", "current"):
        v = ref[where][:, :, V].sum(axis=1).astype(np.int64)
        assert (v[:-1] == rec["vaccinated"][1:]).all() and (v <= bound).all() and v[first] == bound[first] > 0, where
        assert (ref[where].sum(axis=1) == ref["home"].sum(axis=1)).all(), where             # per status, over the areas
    assert (ref["incidence"].sum(axis=1) == rec["exposures_building"].astype(np.int64) + rec["exposures_bus"]).all()
    assert int(ref["incidence"].sum()) == 799 + 11
    area = _area_ref.reference_tables(pop, ep, n)
    assert (ref["current"][:, :, I] == area["infected_rows"]).all()
    # expected() cuts windows as the library addresses its rows
    inc = _area_status_ref.expected(ref, "home", "incidence", n, first_step=5, stride=24)
    assert inc.shape == ((n - 5) // 24 + 1, pop.n_areas) and int(inc.sum()) == int(ref["incidence"][4:].sum())
    assert (_area_status_ref.expected(ref, "current", "recovered", n, first_step=5, n_rows=3, stride=7) == ref["current"][[4, 11, 18], :, R]).all()
