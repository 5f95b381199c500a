"""Space-time ensembles, the parts that need no GPU: series_summary, the refusal of stop_when_done before anything runs, and the
two calls' answer to a null context."""
import numpy as np
import pytest

from epidemicsimulator_amd import Ensemble, EnsembleResult, _lib
from epidemicsimulator_amd.ensemble import series_summary
from epidemicsimulator_amd.simulator import RECORD_DTYPE


def hand_made():
    x = np.array([[[0, 3], [2, 2], [7, 0]], [[4, 3], [0, 2], [1, 0]], [[2, 0], [1, 2], [1, 0]], [[2, 6], [1, 2], [3, 0]]], np.uint64)   # [members, rows, cols]
    return x, (x >= 2).sum(0).astype(np.uint32), x.sum(0), (x * x).sum(0)


def test_series_summary_on_hand_made_arrays():
    x, hit, total, sumsq = hand_made()
    s = series_summary(4, hit, total, sumsq, first_step=100, stride=5)
    assert s["members"] == 4 and s["hit"].dtype == np.uint32 and (s["hit"] == hit).all()
    assert s["hit"].tolist() == [[3, 3], [1, 4], [2, 0]]
    assert s["mean"].tolist() == [[2.0, 3.0], [1.0, 2.0], [3.0, 0.0]]
    assert s["var"].tolist() == [[2.0, 4.5], [0.5, 0.0], [6.0, 0.0]]                   # the population variance
    assert (s["var"] == x.astype(np.float64).var(0)).all()
    assert s["steps"].tolist() == [100, 105, 110]
    assert series_summary(4, hit, total, sumsq)["steps"].tolist() == [1, 2, 3]
    empty = series_summary(0, np.zeros((2, 3), np.uint32), np.zeros((2, 3), np.uint64), np.zeros((2, 3), np.uint64), 4, 2)
    assert empty["members"] == 0 and not empty["mean"].any() and not empty["var"].any() and empty["steps"].tolist() == [4, 6]


def test_series_with_stop_when_done_is_refused_before_anything_runs():
    ens = Ensemble.__new__(Ensemble)                       # no simulator, no context: the refusal needs neither
    area = dict(kind="series", where="home", what="infected", first_step=1, n_rows=4)
    with pytest.raises(ValueError, match="stop_when_done"):
        ens.run([{"seed": 1}], 10, stop_when_done=True, area=area)
    with pytest.raises(ValueError, match="'census', 'arrival' or 'series'"):
        ens.run([{"seed": 1}], 10, area=dict(kind="rows"))
    with pytest.raises(ValueError, match="'census', 'arrival' or 'series'"):
        ens.forecast(5, [{"seed": 1}], 10, area=dict(kind="rows"))
    assert area["kind"] == "series"                        # (the caller's dict is left alone)


def test_dump_of_a_series_summary(tmp_path):
    import json
    _, hit, total, sumsq = hand_made()
    summary = series_summary(4, hit, total, sumsq, first_step=100, stride=5)
    for codes in (None, ["E01", "E02"]):
        out = tmp_path / ("with" if codes else "without")
        EnsembleResult(np.zeros((4, 6), RECORD_DTYPE), [6] * 4, [{}] * 4, summary, codes).dump(str(out))
        assert json.load(open(out / "ensemble_areas.json")) is None
        z = np.load(out / "ensemble_area_series.npz")
        assert sorted(z.files) == sorted(["steps", "hit", "mean", "var"] + (["codes"] if codes else []))
        assert z["steps"].tolist() == [100, 105, 110] and (z["hit"] == hit).all() and (z["mean"] == summary["mean"]).all() and (z["var"] == summary["var"]).all()
        if codes:
            assert z["codes"].tolist() == codes


def test_both_calls_refuse_a_null_context():
    lib = _lib.load()
    assert lib.esim_ensemble_begin_series(None, _lib.AREA_HOME, _lib.INFECTED, 1, 4, 1, 1) == -1          # ESIM_EINVAL
    assert lib.esim_ensemble_read_series(None, 0, 0, None, None, None, None) == -1
