"""The paired policy comparison, what needs no GPU: the Python argument checks (made before the library is touched), the host
summary paired_summary and CompareResult against plain numpy on made-up integer tables, and the reference of
tests/_compare_ref.py on the pairs the GPU tests use -- asserted as inequalities that say the pairs are not vacuous, not as
pinned numbers."""
import numpy as np
import pytest

import _compare_ref as cr
from epidemicsimulator_amd import Ensemble, Simulator, _lib
from epidemicsimulator_amd.ensemble import CompareResult, paired_summary

B, AV, AD, E, L = _lib.CMP_BOTH, _lib.CMP_AVERTED, _lib.CMP_ADDED, _lib.CMP_EARLIER, _lib.CMP_LATER


# ---- 1. the argument checks ----------------------------------------------------------------------------------------------------
class Untouchable:
    """Stands where the library would: any use fails the test."""

    def __getattr__(self, name):
        raise AssertionError("the library was touched (%s) before the arguments were checked" % name)


class FakePopulation:
    n_citizens, n_areas = 10, 3


def bare_simulator():
    sim = object.__new__(Simulator)
    sim.lib, sim._ctx, sim._steps, sim.population = Untouchable(), None, 100, FakePopulation()
    sim.params = _lib.default_params()
    return sim


def test_an_unknown_where_raises_before_the_library_is_touched():
    sim = bare_simulator()
    for where in ("current", "setting", "areas", "", None, _lib.AREA_CURRENT, _lib.BY_SETTING, 7, -1, 1.0, True):
        for call in (lambda: sim.compare(where), lambda: sim.compare_series(where), lambda: sim.ensemble_begin_paired(where)):
            with pytest.raises(ValueError, match="where must be"):
                call()
    for where, code in (("all", _lib.BY_ALL), ("home", _lib.AREA_HOME), ("group", _lib.BY_GROUP), (_lib.BY_ALL, _lib.BY_ALL), (np.int64(_lib.AREA_HOME), _lib.AREA_HOME)):
        assert Simulator._compare_place("x", where) == code
    sim._n_groups = 7
    assert [sim._compare_cols(c) for c in (_lib.BY_ALL, _lib.AREA_HOME, _lib.BY_GROUP)] == [1, 3, 7]


def test_windows_and_rows_are_checked_before_the_library_is_touched():
    sim = bare_simulator()
    with pytest.raises(ValueError, match="no window"):
        sim.compare("all", 5, 4)
    with pytest.raises(ValueError, match="no window"):
        sim.compare("all", -1, 4)
    for bad in (dict(first_step=-1, n_rows=2), dict(stride=0, n_rows=2), dict(n_rows=0), dict(n_rows=-3)):
        with pytest.raises(ValueError, match="first_step must be|no rows"):
            sim.compare_series("all", **bad)
        with pytest.raises(ValueError, match="first_step must be|no rows"):
            sim.ensemble_begin_paired("all", **bad)
    for bad in (dict(min_averted=0), dict(min_averted=-1), dict(min_baseline=-1)):
        with pytest.raises(ValueError, match="min_averted"):
            sim.ensemble_begin_paired("all", n_rows=2, **bad)
    # the rows up to a last step: first_step 0 is a row of its own
    assert Simulator._compare_rows("x", 0, None, 24, 450) == (0, 19, 24) and Simulator._compare_rows("x", 5, None, 7, 40) == (5, 6, 7)
    assert Simulator._compare_rows("x", 450, None, 24, 450) == (450, 1, 24)
    with pytest.raises(ValueError, match="no rows"):
        Simulator._compare_rows("x", 451, None, 24, 450)


def bare_ensemble():
    ens = object.__new__(Ensemble)
    ens.simulator, ens.area_codes, ens._own_seeds = bare_simulator(), None, True
    return ens


def test_ensemble_compare_checks_its_arguments_before_anything_runs():
    ens = bare_ensemble()
    seeds = Ensemble.seeds(2)
    with pytest.raises(ValueError, match="where must be"):
        ens.compare({}, {"mask_effectiveness": 1.0}, seeds, 100, where="current")
    with pytest.raises(ValueError, match="index cases belong to the member"):
        ens.compare({"index_cases": [1]}, {}, seeds, 100)
    with pytest.raises(ValueError, match="history_steps must be"):
        ens.compare({}, {}, seeds, 100, history_steps=101)
    with pytest.raises(ValueError, match="history_steps must be"):
        ens.compare({}, {}, seeds, 100, history_steps=0)
    with pytest.raises(ValueError, match="index cases of the shared history"):
        ens.compare({}, {}, [{"seed": 1, "index_cases": [3]}], 100, history_steps=50)
    for arm in ({"exposed_time": 5}, {"infected_time": 5}, {"start_hour": 8}, {"end_hour": 18}):
        with pytest.raises(ValueError, match="cannot change behind a shared history"):
            ens.compare(arm, {}, seeds, 100, history_steps=50)
        with pytest.raises(ValueError, match="cannot change behind a shared history"):
            ens.compare({}, arm, seeds, 100, history_steps=50)
    with pytest.raises(ValueError, match="rows takes"):
        ens.compare({}, {}, seeds, 100, rows=dict(first_step=0, what="infected"))
    with pytest.raises(ValueError, match="no rows"):
        ens.compare({}, {}, seeds, 100, rows=dict(first_step=101))


# ---- 2. the host summaries against plain numpy ---------------------------------------------------------------------------------
def made_up_rows(members, shape, seed, top=60):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(members):
        b = rng.integers(0, top, size=shape, dtype=np.uint32)
        c = (b * rng.uniform(0.5, 1.1, size=shape)).astype(np.uint32)      # correlated with b, as two paired arms are
        b[rng.random(shape) < 0.2] = 0
        out.append((b, c))
    return out


@pytest.mark.parametrize("members", (2, 3, 9))
def test_paired_summary_equals_numpy_on_made_up_tables(members):
    rows = made_up_rows(members, (5, 7), 100 + members)
    acc = cr.fold_paired(rows, min_baseline=10, min_averted=3)
    got, want = paired_summary(acc, first_step=5, stride=12), cr.direct_summary(rows, 10, 3)
    assert got["members"] == members and got["steps"].tolist() == [5, 17, 29, 41, 53]
    assert (got["defined"] == acc["defined"]).all() and (got["hit"] == acc["hit"]).all() and acc["hit"].any() and (acc["defined"] > acc["hit"]).any()
    for k in ("mean_baseline", "mean_policy", "mean_averted"):
        assert np.allclose(got[k], want[k], rtol=1e-15, atol=0), k
    assert np.array_equal(got["p_averted"], want["p_averted"], equal_nan=True)
    # sums of squares of integers below 2^12 over at most 9 members are exact in float64 on both sides: what is left is the
    # rounding of a handful of divisions and one square root
    for k in ("se_paired", "se_unpaired"):
        assert np.allclose(got[k], want[k], rtol=1e-13, atol=1e-13), k
    assert (got["mean_averted"] < 0).any() and (got["mean_averted"] > 0).any()
    # the pairing: two arms that move together have a smaller standard error of their difference
    assert (got["se_paired"] < got["se_unpaired"]).mean() > 0.8


def test_paired_summary_of_identical_arms_of_one_member_and_of_none():
    rows = made_up_rows(4, (2, 3), 5)
    same = [(b, b) for b, _ in rows]
    got = paired_summary(cr.fold_paired(same))
    assert not got["mean_averted"].any() and not got["se_paired"].any() and got["se_unpaired"].any() and not got["hit"].any()
    one = paired_summary(cr.fold_paired(rows[:1]))
    assert one["members"] == 1 and np.isnan(one["se_paired"]).all() and np.isnan(one["se_unpaired"]).all()
    assert np.array_equal(one["mean_averted"], rows[0][0].astype(np.float64) - rows[0][1])
    none = paired_summary({k: np.zeros((2, 3), np.uint64) for k in cr.PAIRED_KEYS} | {"members": 0})
    assert none["members"] == 0 and not none["mean_averted"].any() and np.isnan(none["p_averted"]).all() and np.isnan(none["se_paired"]).all()


def test_paired_summary_stays_exact_where_the_sums_leave_int64():
    # two members with counts near 2^31 (their squares still add up inside 64 bits, as on the device) that differ by 3 and 1: the
    # spread of the difference is (3 - 1)^2 / 2 = 2, whatever the size
    big = 0x7FFFFFF0
    rows = [(np.array([[big]], np.uint32), np.array([[big - 3]], np.uint32)), (np.array([[big - 7]], np.uint32), np.array([[big - 8]], np.uint32))]
    got = paired_summary(cr.fold_paired(rows))
    assert got["mean_averted"][0, 0] == 2.0 and got["se_paired"][0, 0] == 1.0
    assert np.isclose(got["se_unpaired"][0, 0], np.sqrt((24.5 + 12.5) / 2), rtol=1e-12)


def test_compare_result_against_numpy(tmp_path):
    rng = np.random.default_rng(3)
    tables = [{"counts": rng.integers(0, 50, size=(4, 5)).astype(np.uint64), "delay": rng.integers(-90, 90, size=4), "first_divergence": d} for d in (17, None, 0)]
    members = Ensemble.seeds(3)
    rows = made_up_rows(3, (2, 4), 8)
    summary = paired_summary(cr.fold_paired(rows), 0, 24)
    res = CompareResult.gathered(members, tables, [], [], 4, 10, summary, "home", ["a", "b", "c", "d"])
    assert res.counts.shape == (3, 4, 5) and res.delay.shape == (3, 4) and res.first_divergence.tolist() == [17, -1, 0]
    want = np.stack([t["counts"][:, AV].astype(np.int64) - t["counts"][:, AD].astype(np.int64) for t in tables])
    assert (res.averted() == want).all() and (want < 0).any() and res.averted().dtype == np.int64
    assert res.records_baseline.shape == (0, 10) and res.members == members
    res.dump(str(tmp_path))
    z = np.load(tmp_path / "ensemble_compare.npz")
    assert (z["counts"] == res.counts).all() and (z["averted"] == want).all() and z["names"].tolist() == list(_lib.CMP_NAMES) and z["codes"].tolist() == ["a", "b", "c", "d"]
    assert np.array_equal(z["summary_se_paired"], summary["se_paired"]) and int(z["summary_members"]) == 3
    empty = CompareResult.gathered([], [], [], [], 4, 10)
    assert empty.counts.shape == (0, 4, 5) and empty.averted().shape == (0, 4) and empty.summary is None


# ---- 3. the reference is not vacuous on the pairs the GPU tests use ------------------------------------------------------------
def by_all(world, pair):
    pop, ep, n, _, _, b, _, c, _ = cr.cached(world, pair)
    col, n_cols = cr.columns(pop, "all")
    return cr.compare(b, c, col, n_cols, 0, n)


def test_a_lockdown_that_never_comes_moves_cases_both_ways():
    got = by_all("situations", "lockdown")
    assert all(got["counts"][0, k] > 0 for k in (AV, AD, E, L))
    pop, ep, n, _, _, b, _, c, _ = cr.cached("situations", "lockdown")
    col, n_cols = cr.columns(pop, "home")
    t = cr.compare(b, c, col, n_cols, 0, n)["counts"].astype(np.int64)
    cases_b, cases_c = t[:, B] + t[:, AV], t[:, B] + t[:, AD]
    assert (cases_c > cases_b).any() and (cases_c < cases_b).any()
    assert (t.sum(0) == got["counts"][0].astype(np.int64)).all()


def test_perfect_masks_avert_far_more_than_they_add_and_diverge_late():
    got = by_all("situations", "masks")
    assert got["counts"][0, AV] > 10 * got["counts"][0, AD] and got["first_divergence"] > 100


def test_the_same_parameters_differ_in_nothing():
    got = by_all("situations", "same")
    assert not got["counts"][0, 1:].any() and got["counts"][0, B] > 1000 and got["delay"][0] == 0 and got["first_divergence"] is None and (got["cls"] <= 1).all()


def test_another_seed_has_a_negative_total_delay():
    got = by_all("situations", "seed")
    assert got["delay"][0] < 0 and got["counts"][0, AV] > 100 and got["counts"][0, AD] > 100


def test_a_lower_exposure_chance_in_the_school_world_delays_more_than_a_thousand():
    assert by_all("school", "chance")["counts"][0, L] > 1000


def test_every_pair_of_the_gpu_tests_has_cases_in_both_arms_and_the_forecast_diverges_behind_the_snapshot():
    for world, pair in cr.WORLD_PAIRS:
        got = by_all(world, pair)
        assert got["counts"][0, B] > 0, (world, pair)
        assert pair == "same" or got["first_divergence"] is not None, (world, pair)
    pop, ep, n, t, over, b, c = cr.forecast()
    col, n_cols = cr.columns(pop, "all")
    got = cr.compare(b, c, col, n_cols, 0, n)
    assert got["first_divergence"] > t and got["counts"][0, AV] > got["counts"][0, AD] > 0
    # the rows add up to the window's counts
    rows_b, rows_c = cr.series(b, c, col, n_cols, 0, 19, 24)
    assert rows_b.sum() == got["counts"][0, B] + got["counts"][0, AV] and rows_c.sum() == got["counts"][0, B] + got["counts"][0, AD]
    cum_b, _ = cr.series(b, c, col, n_cols, 0, 19, 24, cumulative=True)
    assert (cum_b[-1] == rows_b.sum(0)).all()
