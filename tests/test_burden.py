"""The parts of the hospital-burden feature that need no GPU: _lib.burden_tables against hand-computed integers, the ABI's new
exports bound in _lib.py, every kernel launch of esim_host_burden.h clamped by ESIM_GRID_CAP or listed as an exact cover, and the
reference module's counts of its two worlds (tests/_burden_ref.py asserts them as it builds a world)."""
import os
import re

import numpy as np
import pytest

import _burden_ref as ref
from epidemicsimulator_amd import _lib
from test_launch_sites import CSRC, ROOT, is_clamped, launches

NEW_EXPORTS = ("esim_burden_set", "esim_burden_drop", "esim_burden_get", "esim_burden_outcomes", "esim_burden_series", "esim_burden_summary",
               "esim_ensemble_begin_burden_peaks")
# (kernel) -> why its grid is not clamped: launches whose grid covers the items exactly.
EXACT_COVER = {"k_series_prefix": "a lane per column, no loop (grid_for without a cap)"}


def test_burden_tables_against_hand_computed_integers():
    t = _lib.burden_tables([0.5, 0.25, 0.0, 1.0], [0.125, 0.0, 1.0, 0.75], [0.5, 0.25], [0.25, 0.25, 0.25], delay_unit=12, stay_unit=48)
    assert t["admit_thr"].dtype == np.uint32 and t["admit_thr"].tolist() == [0x80000000, 0x40000000, 0, 0xFFFFFFFF]
    assert t["death_thr"].tolist() == [0x20000000, 0, 0xFFFFFFFF, 0xC0000000]
    assert t["delay_cdf"].tolist() == [0x80000000, 0xC0000000] and t["stay_cdf"].tolist() == [0x40000000, 0x80000000, 0xC0000000]
    assert (t["delay_unit"], t["stay_unit"]) == (12, 48)
    assert (_lib.burden_tables([0.1], [0.2], [], [])["delay_unit"], _lib.burden_tables([0.1], [0.2], [], [])["stay_unit"]) == (24, 24)
    # a probability that is no binary fraction: the floor of p * 2^32
    assert _lib.burden_tables([0.02], [0.3], [0.05], [0.1])["admit_thr"].tolist() == [int(0.02 * 2 ** 32)] == [85899345]
    assert _lib.burden_tables([0.02], [0.3], [0.05], [0.1])["death_thr"].tolist() == [1288490188]
    # a pmf given in full: the last CDF entry is clamped, and only the largest draw reaches it
    assert _lib.burden_tables([1.0], [1.0], [0.5, 0.5], [0.5, 0.25, 0.25])["delay_cdf"].tolist() == [0x80000000, 0xFFFFFFFF]
    # integer tables are taken as they are
    own = ref.table_set_t()
    got = _lib.burden_tables(own["admit_thr"], own["death_thr"], own["delay_cdf"], own["stay_cdf"])
    for k in ("admit_thr", "death_thr", "delay_cdf", "stay_cdf"):
        assert got[k].dtype == np.uint32 and (got[k] == own[k]).all(), k
    assert own["admit_thr"].tolist()[:3] == [85899345, 85899345, 171798691] and own["delay_cdf"].tolist()[0] == (5 << 32) // 100 == 214748364
    assert own["delay_cdf"].size == 6 and own["stay_cdf"].size == 13 and own["stay_cdf"].tolist()[-1] == (99 << 32) // 100
    for bad in (dict(p_admit=[1.5]), dict(p_death=[-0.1]), dict(p_admit=[0.1, 0.2]), dict(p_admit=[[0.1]])):
        with pytest.raises(ValueError):
            _lib.burden_tables(**dict(dict(p_admit=[0.1], p_death=[0.1], delay_pmf=[0.5], stay_pmf=[0.5]), **bad))


def test_the_new_exports_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "esim.h")).read()
    source = open(os.path.join(os.path.dirname(_lib.__file__), "_lib.py")).read()
    for name in NEW_EXPORTS:
        assert re.search(r"^int\s+%s\(" % name, header, re.M), name
        assert name in _lib.SYMBOLS and '"%s": (C.c_int' % name in source, name
    assert "#define ESIM_BURDEN_BINS 64" in header and _lib.BURDEN_BINS == 64
    assert re.search(r"ESIM_BURDEN_ADMISSIONS = 0, ESIM_BURDEN_OCCUPANCY = 1, ESIM_BURDEN_DEATHS = 2", header)
    assert (_lib.BURDEN_ADMISSIONS, _lib.BURDEN_OCCUPANCY, _lib.BURDEN_DEATHS) == (0, 1, 2)
    philox = open(os.path.join(CSRC, "philox.h")).read()
    assert re.search(r"ESIM_SLOT_BURDEN = 6\b", philox) and "(7 .. 15: free)" in philox and ref.SLOT_BURDEN == 6
    fields = [n for n, _ in _lib.BurdenParams._fields_]
    assert fields == ["n_groups", "admit_thr", "death_thr", "delay_unit", "n_delay", "delay_cdf", "stay_unit", "n_stay", "stay_cdf"]
    body = header[header.index("typedef struct esim_burden_params"):header.index("} esim_burden_params;")]
    declared = re.findall(r"(\w+)\s*(?:,|;)", re.sub(r"/\*.*?\*/", "", body.split("{", 1)[1]))
    assert declared == fields                      # the ctypes structure lays the fields out in the header's order


def test_every_launch_of_the_burden_host_file_is_clamped_or_an_exact_cover():
    seen, used, kernels = [], set(), []
    for kernel, grid, before in launches("esim_host_burden.h"):
        kernels.append(kernel)
        if is_clamped(grid, before):
            assert kernel not in EXACT_COVER, kernel
        elif kernel in EXACT_COVER:
            used.add(kernel)
        else:
            seen.append("%s with grid `%s`" % (kernel, grid))
    assert not seen, "launches that neither go through grid_capped / grid_clamp nor are listed as exact covers:\n" + "\n".join(seen)
    assert sorted(used) == sorted(EXACT_COVER)
    assert sorted(kernels) == ["k_burden_events", "k_burden_outcomes", "k_burden_rows", "k_series_prefix"]
    # the family's kernels are launched from this file alone
    for name in sorted(os.listdir(CSRC)):
        if name.startswith("esim_host_") and name != "esim_host_burden.h":
            assert not [k for k, _, _ in launches(name) if k.startswith("k_burden_")], name


def test_the_reference_counts_of_both_worlds():
    """The module asserts the issue's counts as it builds a world; here the properties the GPU tests rely on."""
    a, w = ref.fixture_a(), ref.world_w2()
    ca, cw = ref.counts(a), ref.counts(w)
    assert ca["cases"] == 722 and ca["admitted"] == 152 and ca["by_band"].count(0) == 2 and ca["deaths"] == 42 and ca["in_bed_at_end"] == 3
    assert (ca["peak"], ca["peak_step"], ca["steps_at_least_10"]) == (87, 396, 431) and (ca["vax_exposed"], ca["vax_infected"]) == (99, 0)
    assert cw["cases"] == 1835 and cw["admitted"] == 475 and cw["deaths"] == 130 and (cw["peak"], cw["peak_step"]) == (236, 402)
    assert (cw["vax_exposed"], cw["vax_infected"], cw["vax_infected_admitted"]) == (85, 275, 64)
    # at the early stops of fixture A ends lie beyond the run (at 96 the four admitted index cases, admitted by step 96), and
    # at 300 admissions too
    for stop in (96, 300):
        o = ref.at_stop(a["full"], stop)
        assert o["admitted"].any() and (o["end_step"][o["admitted"]] > stop).any(), stop
        assert stop == 96 or (o["admit_step"][o["admitted"]] > stop).any(), stop
    # an implementation that forgets that a citizen vaccinated while Exposed is no case would admit some of them
    forgot = np.flatnonzero(w["run"]["vax_exposed"])
    late = ref.outcomes(np.full(len(forgot), 500), w["labels"][forgot], ref.table_set_t(), lambda s: int(w["ep"].seed))
    assert not w["full"]["case"][forgot].any() and late["admitted"].sum() >= 10
    # the summary of the reference agrees with its own rows
    cols, n_cols = a["cols"]["group"]
    o = ref.at_stop(a["full"], 700)
    s = ref.summary(o, cols, n_cols, 700, 1, 700, 10)
    rows = ref.series(o, "occupancy", cols, n_cols, 700)
    assert (s["peak"] == rows.max(axis=0)).all() and (s["bed_steps"] == rows.sum(axis=0)).all() and (s["steps_at_least"] == (rows >= 10).sum(axis=0)).all()
    assert int(s["admissions"].sum()) == int(ref.series(o, "admissions", cols, n_cols, 700).sum()) <= 152
    assert ref.series(o, "deaths", cols, n_cols, 700, 5, 10, 24).shape == (10, n_cols)
