"""Ensemble maps of transmission, the parts that need no GPU: the three entries are declared and bound; what the reproduction
accumulators must satisfy on every reference world; that the cases the device test compares are not vacuous; the host summary
(r, p_r, r_se) against a direct numpy computation from the stacked member rows; and Ensemble.run's `complete` rule on a stubbed
simulator."""
import os
import re

import numpy as np
import pytest

import _ens_transmission_ref as ens_ref
import _tree_ref as tree
from epidemicsimulator_amd import Ensemble, EnsembleResult, _lib
from epidemicsimulator_amd.ensemble import reproduction_summary
from epidemicsimulator_amd.simulator import RECORD_DTYPE, Simulator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("esim_ensemble_begin_settings", "esim_ensemble_begin_reproduction", "esim_ensemble_read_reproduction")


def test_the_header_declares_the_three_entries_and_the_binding_has_them():
    text = open(os.path.join(ROOT, "include", "esim.h")).read()
    lib = _lib.load()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(esim_ctx \*ctx" % name, text), name
        assert name in _lib.SYMBOLS and getattr(lib, name).restype is not None and len(getattr(lib, name).argtypes) >= 7
    assert len(lib.esim_ensemble_read_reproduction.argtypes) == 11 and len(lib.esim_ensemble_begin_reproduction.argtypes) == 8
    # a null context is ESIM_EINVAL before anything else is looked at
    assert lib.esim_ensemble_begin_settings(None, _lib.AREA_HOME, 0xF, 1, 4, 1, 1) == -1
    assert lib.esim_ensemble_begin_reproduction(None, _lib.AREA_HOME, 0, 4, 24, 1, 1, 1) == -1
    assert lib.esim_ensemble_read_reproduction(None, 0, 0, *([None] * 8)) == -1
    for name in ("ensemble_begin_settings", "ensemble_begin_reproduction", "ensemble_read_reproduction"):
        assert callable(getattr(Simulator, name))


@pytest.mark.parametrize("world", tree.ALL_WORLDS)
def test_reproduction_accumulators_of_every_reference_world(world):
    pop, ep, n, ref = tree.cached(world)
    lab, n_groups = ens_ref.labels_of(pop)
    for where in ("all", "home", "group"):
        for first, stride in ((0, 24), (1, 7), (0, n + 1)):
            cases, off = tree.reproduction_rows(ref, pop, where, first, None, stride, lab, n_groups)
            assert not ((off > 0) & (cases == 0)).any(), (world, where, first, stride)          # what the fold kernel must not rely on
            assert int(cases.sum()) > 0
            for r in ((1, 1), (0, 1), (3, 2)):
                for min_cohort in (1, 5):
                    acc = ens_ref.fold_reproduction([(cases, off), (cases, off // 2), (cases // 2, off // 3)], min_cohort, r)
                    assert (acc["hit"] <= acc["defined"]).all() and (acc["defined"] <= acc["members"]).all() and acc["members"] == 3
                    if r == (0, 1):
                        assert (acc["hit"] == acc["defined"]).all()
                    c64, o64 = cases.astype(np.uint64), off.astype(np.uint64)
                    assert (acc["sum_cases"] == c64 + c64 + c64 // 2).all() and (acc["sum_offspring"] == o64 + o64 // 2 + o64 // 3).all()
                    assert (acc["sum_cross"] == c64 * o64 + c64 * (o64 // 2) + (c64 // 2) * (o64 // 3)).all()
                    assert (acc["sumsq_cases"] == 2 * c64 * c64 + (c64 // 2) ** 2).all() and (acc["sumsq_offspring"] == o64 * o64 + (o64 // 2) ** 2 + (o64 // 3) ** 2).all()


@pytest.mark.parametrize("case", range(len(ens_ref.REPRODUCTION_CASES)))
def test_the_reproduction_cases_of_the_device_test_are_not_vacuous(case):
    world, where, window, r, min_cohort = ens_ref.REPRODUCTION_CASES[case]
    rows = ens_ref.reproduction_of(world, where, window)
    n = ens_ref.members(world)[2]
    assert len(rows) == 3 and window["first_step"] + (window["n_rows"] - 1) * window["stride"] <= n
    assert any((a[0] != b[0]).any() or (a[1] != b[1]).any() for a, b in zip(rows, rows[1:]))      # the members differ
    acc = ens_ref.fold_reproduction(rows, min_cohort, r)
    assert (acc["hit"] > 0).any(), "no cell is hit"
    assert (acc["defined"] < acc["members"]).any(), "no cell below min_cohort in any member"
    if r[0] == 0:
        # every defined cell is hit whatever its offspring: "a defined cell that is not hit" cannot exist, the equality is the check
        assert (acc["hit"] == acc["defined"]).all() and (acc["defined"] > 0).any()
    else:
        assert (acc["defined"] > acc["hit"]).any(), "no defined cell that is not hit"
    for c, o in rows:
        assert not ((o > 0) & (c == 0)).any()
    # sums over members equal the sum of the rows
    assert (acc["sum_cases"] == sum(c.astype(np.uint64) for c, _ in rows)).all() and (acc["sum_offspring"] == sum(o.astype(np.uint64) for _, o in rows)).all()


def test_the_cell_counts_of_the_device_cases_cover_every_tail():
    cells = []
    for world, where, window, _, _ in ens_ref.REPRODUCTION_CASES:
        pop = ens_ref.members(world)[0]
        cells.append(window["n_rows"] * {"all": 1, "home": pop.n_areas, "group": ens_ref.labels_of(pop)[1]}[where])
    assert {c % 4 for c in cells} == {0, 1, 2, 3}, cells
    assert {tuple(r) for _, _, _, r, _ in ens_ref.REPRODUCTION_CASES} == {(1, 1), (0, 1), (3, 2)}
    assert {w for _, w, _, _, _ in ens_ref.REPRODUCTION_CASES} == {"all", "home", "group"}
    assert {w for _, w, _, _, _ in ens_ref.SETTINGS_CASES} == {"setting", "home", "group"}


@pytest.mark.parametrize("case", range(len(ens_ref.SETTINGS_CASES)))
def test_the_settings_cases_of_the_device_test_are_not_vacuous(case):
    world, where, settings, window, min_cases = ens_ref.SETTINGS_CASES[case]
    rows = ens_ref.settings_of(world, where, settings, window)
    acc = ens_ref.fold_settings(rows, min_cases)
    assert ((acc["hit"] > 0) & (acc["hit"] < acc["members"])).any(), "no cell hit in some members only"
    assert (acc["sum"] == sum(x.astype(np.uint64) for x in rows)).all() and acc["sum"].any()


@pytest.mark.parametrize("case", range(len(ens_ref.REPRODUCTION_CASES)))
def test_the_host_summary_against_a_direct_computation(case):
    world, where, window, r, min_cohort = ens_ref.REPRODUCTION_CASES[case]
    rows = ens_ref.reproduction_of(world, where, window)
    got = reproduction_summary(ens_ref.fold_reproduction(rows, min_cohort, r), window["first_step"], window["stride"])
    want = ens_ref.direct_summary(rows, min_cohort, r)
    assert got["members"] == 3 and got["steps"].tolist() == [window["first_step"] + i * window["stride"] for i in range(window["n_rows"])]
    for k in ("r", "p_r", "cases_mean", "offspring_mean"):
        assert (np.isnan(got[k]) == np.isnan(want[k])).all(), k
        np.testing.assert_allclose(got[k], want[k], rtol=1e-12, atol=0, err_msg=k)
    assert (np.isnan(got["r"]) == (ens_ref.fold_reproduction(rows, min_cohort, r)["sum_cases"] == 0)).all()
    assert (np.isnan(got["r_se"]) == np.isnan(want["r_se"])).all() and np.isfinite(got["r_se"]).any()
    # both sides are float64 on the host: rtol 1e-12, beside the absolute rounding error of the direct computation's residuals
    # (_ens_transmission_ref.direct_summary: at most 4 EPS * r * members / sqrt(members - 1) per cell, about 1e-15 * r here)
    err = np.abs(got["r_se"] - want["r_se"])
    bound = 1e-12 * np.abs(want["r_se"]) + ens_ref.se_atol(3, want["r"])
    ok = np.isnan(want["r_se"]) | (err <= bound)
    assert ok.all(), (np.nanmax(err - bound), np.flatnonzero(~ok.ravel())[:8].tolist())
    # the covariance form of the same quantity, whose terms cancel: agreement to about sqrt(EPS) * r, the identity checked
    fin = np.isfinite(want["r_se"])
    assert (np.abs(got["r_se"] - want["r_se_cov"])[fin] <= 1e-6 * np.maximum(1.0, want["r"][fin])).all()


def test_the_host_summary_on_hand_made_members():
    c = [np.array([[4, 0, 2, 1]], np.uint32), np.array([[2, 0, 4, 0]], np.uint32), np.array([[6, 0, 6, 0]], np.uint32)]
    o = [np.array([[8, 0, 1, 3]], np.uint32), np.array([[4, 0, 6, 0]], np.uint32), np.array([[12, 0, 2, 0]], np.uint32)]
    rows = list(zip(c, o))
    s = reproduction_summary(ens_ref.fold_reproduction(rows, 2, (3, 2)), 10, 5)
    assert s["members"] == 3 and s["defined"].tolist() == [[3, 0, 3, 0]] and s["hit"].tolist() == [[3, 0, 1, 0]] and s["steps"].tolist() == [10]
    assert s["r"][0, 0] == 2.0 and np.isnan(s["r"][0, 1]) and s["r"][0, 2] == 0.75 and s["r"][0, 3] == 3.0
    assert s["p_r"][0, 0] == 1.0 and np.isnan(s["p_r"][0, 1]) and s["p_r"][0, 2] == 1 / 3 and np.isnan(s["p_r"][0, 3])
    assert s["r_se"][0, 0] == 0.0 and np.isnan(s["r_se"][0, 1]) and s["r_se"][0, 3] == 0.0      # offspring proportional to cases: no spread
    e = np.array([1 - 0.75 * 2, 6 - 0.75 * 4, 2 - 0.75 * 6])
    assert abs(s["r_se"][0, 2] - np.sqrt((e * e).sum() / 2 / 3) / 4.0) < 1e-15
    assert s["cases_mean"].tolist() == [[4.0, 0.0, 4.0, 1 / 3]]
    one = reproduction_summary(ens_ref.fold_reproduction(rows[:1], 1, (1, 1)))
    assert one["members"] == 1 and np.isnan(one["r_se"]).all() and one["r"][0, 0] == 2.0         # fewer than two members: no standard error
    # sums too large for int64 products take the exact integer path and give the same answer as the scaled-down members
    big = [(a.astype(np.uint64) << np.uint64(20), b.astype(np.uint64) << np.uint64(20)) for a, b in rows]
    t = reproduction_summary(ens_ref.fold_reproduction(big, 2, (3, 2)))
    assert (np.isnan(t["r_se"]) == np.isnan(s["r_se"])).all() and np.allclose(np.nan_to_num(t["r_se"]), np.nan_to_num(s["r_se"]), rtol=1e-14, atol=0)


class StubSimulator:
    """What Ensemble.run touches of a Simulator, recorded instead of run."""

    def __init__(self):
        self.calls = []

    def restart(self, params, seeds=None, **over):
        self.calls.append(("restart", over))

    def run(self, n_steps, stop_when_done=False):
        rec = np.zeros(n_steps, RECORD_DTYPE)
        rec["time_step"] = np.arange(1, n_steps + 1)
        return rec

    def ensemble_begin_reproduction(self, **kw):
        self.calls.append(("begin_reproduction", kw))
        self.rows = kw["n_rows"]

    def ensemble_begin_settings(self, **kw):
        self.calls.append(("begin_settings", kw))
        self.rows = kw["n_rows"]

    def ensemble_fold(self):
        self.calls.append(("fold", None))

    def ensemble_read_reproduction(self):
        z = lambda t: np.zeros((self.rows, 2), t)
        return dict(members=2, defined=z(np.uint32), hit=z(np.uint32), sum_cases=z(np.uint64), sum_offspring=z(np.uint64), sumsq_cases=z(np.uint64),
                    sumsq_offspring=z(np.uint64), sum_cross=z(np.uint64))

    def ensemble_read_series(self):
        z = lambda t: np.zeros((self.rows, 2), t)
        return dict(members=2, hit=z(np.uint32), sum=z(np.uint64), sumsq=z(np.uint64))


def stubbed(exposed_time=4, infected_time=10):
    ens = Ensemble.__new__(Ensemble)
    ens.simulator, ens.area_codes, ens._own_seeds = StubSimulator(), ["E1", "E2"], True
    ens.base = _lib.default_params(exposed_time=exposed_time, infected_time=infected_time)
    return ens


def test_run_takes_only_complete_cohort_rows_by_default(tmp_path):
    # a cohort exposed in step s is complete once s + 4 + 1 + 10 steps have run: after 100 steps the last complete step is 85
    ens = stubbed()
    res = ens.run(Ensemble.seeds(2), 100, area=dict(kind="reproduction", where="home", first_step=0, stride=24, min_cohort=3, r=(3, 2)))
    begin = [c for c in ens.simulator.calls if c[0] == "begin_reproduction"]
    assert len(begin) == 1 and begin[0][1] == dict(where="home", first_step=0, stride=24, min_cohort=3, r=(3, 2), n_rows=3)   # rows end at steps 23, 47, 71; 95 > 85
    assert [c[0] for c in ens.simulator.calls].count("fold") == 2
    assert res.area["members"] == 2 and res.area["steps"].tolist() == [0, 24, 48] and res.area_codes == ["E1", "E2"] and np.isnan(res.area["r"]).all()
    # the edge: a row whose last step is exactly the last complete one is taken, one step later it is not
    for first, stride, rows in ((0, 43, 2), (1, 43, 1), (0, 86, 1), (0, 87, None), (80, 6, 1), (81, 6, None), (86, 1, None), (85, 1, 1)):
        ens = stubbed()
        area = dict(kind="reproduction", first_step=first, stride=stride)
        if rows is None:
            with pytest.raises(ValueError, match="no complete cohort row"):
                ens.run(Ensemble.seeds(1), 100, area=area)
            assert ens.simulator.calls == []                                                     # refused before anything ran
        else:
            ens.run(Ensemble.seeds(1), 100, area=area)
            assert ens.simulator.calls[0][1]["n_rows"] == rows, (first, stride)
    # complete=False takes the open rows too, an explicit n_rows is the caller's
    ens = stubbed()
    ens.run(Ensemble.seeds(1), 100, area=dict(kind="reproduction", stride=24, complete=False))
    assert ens.simulator.calls[0][1] == dict(stride=24, n_rows=5)
    ens = stubbed()
    ens.run(Ensemble.seeds(1), 100, area=dict(kind="reproduction", stride=24, n_rows=4))
    assert ens.simulator.calls[0][1] == dict(stride=24, n_rows=4)
    ens = stubbed()
    with pytest.raises(ValueError, match="stop_when_done"):
        ens.run(Ensemble.seeds(1), 100, stop_when_done=True, area=dict(kind="reproduction"))
    with pytest.raises(ValueError, match="stop_when_done"):
        ens.run(Ensemble.seeds(1), 100, stop_when_done=True, area=dict(kind="settings"))
    # the settings kind: rows up to the last step of the run, the summary a series summary, both dumped under their own names
    ens = stubbed()
    res2 = ens.run(Ensemble.seeds(1), 100, area=dict(kind="settings", where="group", settings=("household",), first_step=3, stride=7, min_cases=2))
    assert ens.simulator.calls[0] == ("begin_settings", dict(where="group", settings=("household",), first_step=3, stride=7, min_cases=2, n_rows=14))
    assert res2.area["steps"].tolist() == list(range(3, 100, 7)) and res2.area_codes is None and "mean" in res2.area
    res.dump(str(tmp_path / "r"))
    res2.dump(str(tmp_path / "s"))
    z = np.load(tmp_path / "r" / "ensemble_area_reproduction.npz")
    assert sorted(z.files) == sorted(["steps", "members", "defined", "hit", "cases_mean", "offspring_mean", "r", "p_r", "r_se", "codes"]) and int(z["members"]) == 2
    z = np.load(tmp_path / "s" / "ensemble_area_settings.npz")
    assert sorted(z.files) == ["hit", "mean", "steps", "var"] and not os.path.exists(tmp_path / "s" / "ensemble_area_series.npz")
    assert isinstance(res, EnsembleResult) and res.area_kind == "reproduction" and res2.area_kind == "settings"
