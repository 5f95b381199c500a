"""Forecast ensembles, the parts that need no device: the four symbols and their prototypes, null arguments, the Python wrappers
without a device, Ensemble.forecast on a stubbed simulator, and the oracle-side precondition of the branch that the GPU tests
compare with the oracle (tests/_snapshot_ref.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _snapshot_ref as ref
from epidemicsimulator_amd import Ensemble, Population, RECORD_DTYPE, Simulator, _lib
from epidemicsimulator_amd.ensemble import pad_records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"esim_snapshot": 1, "esim_rollback": 2, "esim_snapshot_info": 3, "esim_snapshot_drop": 1}


def test_the_four_symbols_exist_with_the_bound_signatures():
    lib = _lib.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "esim.h")).read(), flags=re.S)     # declarations only
    for name, arity in NEW.items():
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, text)
        assert m, name
        fn = getattr(lib, name)
        assert len(m.group(1).split(",")) == arity == len(fn.argtypes) and fn.restype is C.c_int, name
    assert lib.esim_rollback.argtypes[1] == C.POINTER(_lib.Params)
    assert lib.esim_snapshot_info.argtypes[1:] == [C.POINTER(C.c_uint32), C.POINTER(_lib.Params)]
    for name in ("snapshot", "rollback", "snapshot_step"):
        assert callable(getattr(Simulator, name))
    assert callable(Ensemble.forecast)


def test_null_arguments_are_einval():
    lib = _lib.load()
    p, step = _lib.default_params(), C.c_uint32(7)
    assert lib.esim_snapshot(None) == -1 and lib.esim_snapshot_drop(None) == -1
    assert lib.esim_rollback(None, C.byref(p)) == -1 and lib.esim_rollback(None, None) == -1
    assert lib.esim_snapshot_info(None, C.byref(step), C.byref(p)) == -1 and lib.esim_snapshot_info(None, None, None) == -1
    assert step.value == 7                                           # a refused call writes nothing


def test_the_wrappers_fail_loudly_without_a_device():
    pop = Population.synthetic("york", n_citizens=500, n_areas=3, citizens_per_school=500, n_seeds=5)
    lib, p, ctx = _lib.load(), _lib.default_params(), C.c_void_p()
    if lib.esim_create(C.byref(p), C.byref(ctx)) == 0:               # a device is there: the same calls work
        lib.esim_destroy(ctx)
        sim = Simulator(pop)
        assert sim.snapshot_step() == 0
        with pytest.raises(_lib.EsimError) as e:
            sim.rollback()
        assert e.value.code == -4
        sim.run(3); sim.snapshot(); sim.run(2); sim.rollback(seed=7)
        assert sim.snapshot_step() == 3 and sim._steps == 3 and sim.params.seed == 7 and len(sim.statistics_recorder.global_stats) == 3
        sim.close()
        return
    with pytest.raises(_lib.EsimError) as e:
        Simulator(pop).snapshot()                                    # no device: no context to snapshot, ESIM_ENODEVICE like the rest
    assert e.value.code == -2
    with pytest.raises(_lib.EsimError) as e:
        Ensemble(pop).forecast(2, [{}], 4)
    assert e.value.code == -2


def records(first, n, **cols):
    r = np.zeros(n, RECORD_DTYPE)
    r["time_step"] = np.arange(first, first + n)
    r["disease_exists"] = 1
    for k, v in cols.items():
        r[k] = v
    return r


class StubSimulator:
    """Answers what Ensemble.forecast asks of a Simulator, from a script: the history, then one future per member."""

    def __init__(self, history, futures):
        self.history, self.futures, self.calls, self.branch = history, list(futures), [], -1
        self.population = type("P", (), {"seeds": np.array([1, 2], np.uint32)})()

    def restart(self, params, seeds=None, **over):
        self.calls.append(("restart", None if seeds is None else list(seeds), over)); self.branch = -1

    def run(self, n, stop_when_done=False):
        self.calls.append(("run", n))
        out = self.history if self.branch < 0 else self.futures[self.branch]
        assert len(out) <= n
        return out

    def snapshot(self):
        self.calls.append(("snapshot",))

    def rollback(self, params=None, **over):
        self.calls.append(("rollback", over)); self.branch += 1

    def ensemble_begin(self, **kw):
        self.calls.append(("begin", kw))

    def ensemble_fold(self):
        self.calls.append(("fold",))

    def ensemble_read(self):
        return {"members": 2, "hit": np.array([2, 1, 0], np.uint32), "sum": np.array([6, 5, 0], np.uint64), "sumsq": np.array([20, 25, 0], np.uint64)}


def test_forecast_assembles_the_records_with_the_history_repeated_and_padded():
    history = records(1, 3, infected=[1, 2, 3], susceptible=[9, 8, 7])
    full = records(4, 4, infected=[4, 5, 6, 7], susceptible=[6, 5, 4, 3], exposures_building=[1, 1, 1, 1])
    short = records(4, 2, infected=[2, 0], susceptible=[7, 7], exposures_building=[0, 1], disease_exists=[1, 0])   # (a member that ended early)
    ens = Ensemble.__new__(Ensemble)
    ens.simulator, ens.area_codes, ens.base, ens._own_seeds = StubSimulator(history, [full, short]), ["A", "B", "C"], _lib.default_params(), False
    members = [{"seed": 5}, {"lockdown_threshold": 0.01}]
    res = ens.forecast(3, members, 7, area=dict(where="home", status_mask=4, min_cases=1))
    sim = ens.simulator
    assert sim.calls == [("begin", dict(where="home", status_mask=4, min_cases=1)), ("restart", [1, 2], {}), ("run", 3), ("snapshot",),
                         ("rollback", {"seed": 5}), ("run", 4), ("fold",), ("rollback", {"lockdown_threshold": 0.01}), ("run", 4), ("fold",)]
    assert ens._own_seeds and res.members == members and res.n_done.tolist() == [7, 5] and res.records.shape == (2, 7)
    for k, fut in enumerate((full, short)):
        assert (res.records[k][:3] == history).all()                                     # the shared history, in every row
        assert (res.records[k] == pad_records(np.concatenate([history, fut]), 7)).all()
    pad = res.records[1][5:]
    assert pad["time_step"].tolist() == [6, 7] and pad["susceptible"].tolist() == [7, 7] and pad["exposures_building"].tolist() == [0, 0]
    assert pad["disease_exists"].tolist() == [0, 0]
    assert res.area["members"] == 2 and res.area["hit"].tolist() == [2, 1, 0] and res.area["mean"].tolist() == [3.0, 2.5, 0.0] and res.area_codes == ["A", "B", "C"]
    assert res.quantiles("infected", [0.5]).shape == (1, 7) and res.mean("infected")[:3].tolist() == [1.0, 2.0, 3.0]
    # no accumulators asked for, a history as long as the run, and what a branch cannot change
    ens.simulator = StubSimulator(history, [records(4, 0)])
    res = ens.forecast(3, [{}], 3)
    assert res.area is None and (res.records[0] == history).all() and ("fold",) not in ens.simulator.calls and ens.simulator.calls[-1] == ("rollback", {})
    for bad in (lambda: ens.forecast(0, [{}], 3), lambda: ens.forecast(4, [{}], 3), lambda: ens.forecast(2, [{"index_cases": [1]}], 3),
                lambda: ens.forecast(2, [{}], 3, area=dict(kind="median"))):
        with pytest.raises(ValueError):
            bad()


@pytest.mark.parametrize("name", ("parity", "york"))
def test_the_branch_the_gpu_tests_compare_with_the_oracle_cannot_act_before_its_step(name):
    """The oracle cannot change parameters mid-run, so the overrides B of that branch must not act before T; T comes from the
    oracle itself (the last step up to which its records under A and under B agree in every field, minus 5)."""
    t, same_state, ever_differ = ref.branch_step(name)
    assert ever_differ, "A and B never differ: the branch shows nothing"
    assert t >= 100 and same_state, (t, same_state)
    assert t % 96 and t % 97 and t < ref.N_STEPS - 100
    rec = ref.straight(name)[0]
    # the steps the same-future tests snapshot at: one inside the vaccination programme, none on a chunk boundary
    assert rec["vaccination_active"][300 - 1] == 1 and rec["vaccinated_now"][300 - 1] > 0 and rec["vaccination_active"][61 - 1] == 0
    assert all(s % 96 and s % 97 for s in (61, 137, 300))
