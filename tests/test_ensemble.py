"""Ensembles, the parts that need no device: the new symbols and their prototypes, Ensemble.seeds, and the padding / quantile /
area arithmetic of EnsembleResult on hand-made record arrays."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from epidemicsimulator_amd import Ensemble, EnsembleResult, Population, Simulator, RECORD_DTYPE, _lib
from epidemicsimulator_amd.ensemble import area_summary, pad_records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("esim_restart", "esim_ensemble_begin", "esim_ensemble_fold", "esim_ensemble_read")


def test_new_symbols_are_exported_with_the_header_arity():
    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "esim.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)            # declarations only
    for name in NEW:
        assert hasattr(lib, name) and name in _lib.SYMBOLS
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, text)
        assert m, name
        assert len(getattr(lib, name).argtypes) == len(m.group(1).split(",")), name
        assert getattr(lib, name).restype is C.c_int


def test_seeds():
    assert Ensemble.seeds(3) == [{"seed": 1}, {"seed": 2}, {"seed": 3}]
    assert Ensemble.seeds(2, first=40) == [{"seed": 40}, {"seed": 41}]
    assert Ensemble.seeds(0) == []


def records(n, **cols):
    r = np.zeros(n, RECORD_DTYPE)
    r["time_step"] = np.arange(1, n + 1)
    r["disease_exists"] = 1
    for k, v in cols.items():
        r[k] = v
    return r


def test_padding_carries_the_census_forward():
    r = records(3, susceptible=[5, 4, 0], exposed=[1, 1, 0], infected=[2, 3, 0], recovered=[0, 0, 6], vaccinated=[0, 0, 2],
                exposures_building=[1, 0, 2], exposures_bus=[0, 1, 1], vaccinated_now=[0, 0, 2], lockdown=[0, 1, 1],
                vaccination_active=[0, 0, 1], mask_status=[0, 1, 2], n_riders=[3, 3, 3], disease_exists=[1, 1, 0])
    p = pad_records(r, 6)
    assert p.shape == (6,) and (p[:3] == r).all()
    assert p["time_step"].tolist() == [1, 2, 3, 4, 5, 6]
    for f, v in (("susceptible", 0), ("exposed", 0), ("infected", 0), ("recovered", 6), ("vaccinated", 2), ("lockdown", 1),
                 ("vaccination_active", 1), ("mask_status", 2)):
        assert p[f][3:].tolist() == [v] * 3, f
    for f in ("exposures_building", "exposures_bus", "vaccinated_now", "disease_exists"):
        assert p[f][3:].tolist() == [0, 0, 0], f
    assert (pad_records(r, 3) == r).all()                          # nothing to pad
    z = pad_records(r[:0], 2)                                      # a member without a record
    assert z["time_step"].tolist() == [1, 2] and z["infected"].tolist() == [0, 0] and z["disease_exists"].tolist() == [0, 0]


def test_quantiles_mean_area_and_dump(tmp_path):
    rows = np.stack([records(4, infected=[1, 2, 3, 4]), records(4, infected=[3, 2, 1, 0]), records(4, infected=[5, 8, 5, 8])])
    area = area_summary(3, [3, 1, 0], [12, 5, 0], [56, 25, 0])     # x = (2, 4, 6), (0, 5, 0), (0, 0, 0)
    res = EnsembleResult(rows, [4, 4, 4], [{"seed": s} for s in (1, 2, 3)], area, area_codes=["E1", "E2", "E3"])
    assert res.quantiles("infected", [0.5]).tolist() == [[3.0, 2.0, 3.0, 4.0]]
    assert res.quantiles("infected", [0.0, 0.25, 1.0]).tolist() == [[1.0, 2.0, 1.0, 0.0], [2.0, 2.0, 2.0, 2.0], [5.0, 8.0, 5.0, 8.0]]
    assert res.mean("infected").tolist() == [3.0, 4.0, 3.0, 4.0]
    assert area["members"] == 3 and area["mean"].tolist() == [4.0, 5.0 / 3.0, 0.0]
    assert np.allclose(area["var"], [np.var([2, 4, 6]), np.var([0, 5, 0]), 0.0], rtol=1e-12, atol=1e-12)
    out = str(tmp_path / "e")
    res.dump(out)
    stats = json.load(open(os.path.join(out, "ensemble_stats.json")))
    assert stats["fields"]["infected"]["q50"] == [3.0, 2.0, 3.0, 4.0] and stats["fields"]["infected"]["mean"] == [3.0, 4.0, 3.0, 4.0]
    assert set(stats["fields"]["infected"]) == {"mean", "q05", "q25", "q50", "q75", "q95"}
    areas = json.load(open(os.path.join(out, "ensemble_areas.json")))
    assert areas["members"] == 3 and areas["areas"]["E2"] == {"hit": 1, "mean": 5.0 / 3.0, "var": float(area["var"][1])}
    # without codes the areas are keyed by index; without accumulators the file says so
    EnsembleResult(rows, [4, 4, 4], [], area).dump(out)
    assert sorted(json.load(open(os.path.join(out, "ensemble_areas.json")))["areas"]) == ["0", "1", "2"]
    EnsembleResult(rows, [4, 4, 4], []).dump(out)
    assert json.load(open(os.path.join(out, "ensemble_areas.json"))) is None


def test_restart_fails_loudly_without_a_device():
    assert hasattr(Simulator, "restart")
    pop = Population.synthetic("york", n_citizens=500, n_areas=3, citizens_per_school=500, n_seeds=5)
    lib = _lib.load()
    p = _lib.default_params()
    assert lib.esim_restart(None, C.byref(p)) == -1 and lib.esim_ensemble_fold(None) == -1     # ESIM_EINVAL: no context
    ctx = C.c_void_p()
    if lib.esim_create(C.byref(p), C.byref(ctx)) == 0:             # a device is there: the same calls work
        lib.esim_destroy(ctx)
        sim = Simulator(pop)
        sim.restart(seed=7)
        assert sim.params.seed == 7 and sim._steps == 0
        sim.close()
        return
    with pytest.raises(_lib.EsimError) as e:
        Simulator(pop).restart(seed=7)                             # no device: no context to restart, ESIM_ENODEVICE like the rest
    assert e.value.code == -2
    with pytest.raises(_lib.EsimError) as e:
        Ensemble(pop)
    assert e.value.code == -2
