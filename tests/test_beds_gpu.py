"""A run's admitted cases as a list on the device -- the kept burden baseline, esim_burden_compare, esim_burden_compare_series and the
burden-series and burden-paired kinds of the ensemble accumulators -- against tests/_beds_ref.py: numpy over the outcomes of
tests/_burden_ref.py for both arms of a pair.  Every comparison is exact equality of whole integer arrays."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _area_ref
import _beds_ref as beds
import _burden_ref as ref
import test_burden_gpu as bg
from epidemicsimulator_amd import Ensemble, Population, Simulator, _lib

pytestmark = pytest.mark.gpu

NEVER, WHERES, WHATS = ref.NEVER, ref.WHERES, ref.WHATS
EINVAL, ESTATE, ERANGE = -1, -4, -5
T = ref.table_set_t()
u32p, u64p, u8p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint8)
same, check_untouched = bg.same, bg.check_untouched
POLICY = dict(fixture_a=dict(mask_effectiveness=1.0), w2=dict(vaccination_rate=3), w2_seed=dict(seed=322))
CASE_KEYS = ("citizen", "admit_step", "end_step", "died")
ARMS = (("baseline", "_baseline"), ("current", "_current"))


def new_sim(world, tables=T):
    sim = Simulator(world["pop"], world["ep"])
    sim.set_groups(world["labels"], world["n_groups"])
    sim.set_burden(tables)
    return sim


def same_cases(sim, o, note):
    got, want = sim.burden_baseline_cases(), beds.cases(o)
    assert sorted(got) == sorted(CASE_KEYS)
    for k in CASE_KEYS:
        same(got[k], want[k], "%s: the kept cases, %s" % (note, k))
    info = sim.burden_baseline_info()
    assert (info["n_admitted"], info["n_died"]) == (len(want["citizen"]), int(want["died"].sum())), note


def same_totals(got, want, suffix, note):
    for k in beds.TOTALS:
        same(got[k + suffix], want[k], "%s: %s%s" % (note, k, suffix))


def series_windows(t):
    """(first_step, n_rows, stride): every step, every day, and from inside the run."""
    return ((1, None, 1), (1, None, 24), (t // 3, None, 24))


def check_compare(sim, cols, o_base, t_base, o_cur, t_cur, note, kept_summary=None, spans=None, series=None):
    """Everything the comparison calls give against the outcomes of both arms; the _c side also against the library's own
    burden_summary and burden_series of the run as it stands, the _b side against the summaries taken at the keep.  spans: the
    (first_step, last_step) of the totals instead of the three below; series: the (first_step, n_rows, stride) instead of
    series_windows(t)."""
    t = min(t_base, t_cur)
    for where in WHERES:
        lab, n_cols = cols[where]
        for first, last in (((1, t), (min(200, t), min(500, t)), (t, t)) if spans is None else spans):
            got = sim.burden_compare(where, first, last)
            what = "%s: by %s, steps %d..%d" % (note, where, first, last)
            same_totals(got, beds.totals(o_base, lab, n_cols, t_base, first, last), "_baseline", what)
            same_totals(got, beds.totals(o_cur, lab, n_cols, t_cur, first, last), "_current", what)
            same_totals(got, sim.burden_summary(where, first, last), "_current", what + " vs burden_summary now")
            if kept_summary is not None:
                same_totals(got, kept_summary[where, first, last], "_baseline", what + " vs burden_summary at the keep")
            for k in beds.TOTALS:
                same(got[k + "_averted"], got[k + "_baseline"].astype(np.int64) - got[k + "_current"].astype(np.int64), what + ": averted " + k)
        for what in WHATS:
            for first, n_rows, stride in (series_windows(t) if series is None else series):
                for cumulative in ((False,) if what == "occupancy" else (False, True)):
                    b, c = sim.burden_compare_series(what, where, first, n_rows, stride, cumulative)
                    k = (t - first) // stride + 1 if n_rows is None else n_rows
                    tag = "%s: %s by %s from step %d, stride %d%s" % (note, what, where, first, stride, ", cumulative" if cumulative else "")
                    same(b, beds.rows(o_base, what, lab, n_cols, t_base, first, k, stride, cumulative), tag + ", baseline")
                    same(c, beds.rows(o_cur, what, lab, n_cols, t_cur, first, k, stride, cumulative), tag + ", current")
                    if not cumulative:
                        same(c, sim.burden_series(what, where, first, k, stride), tag + " vs burden_series")


def check_pair(base, policy, over, note):
    n = base["n_steps"]
    o_b, o_p = ref.at_stop(base["full"], n), ref.at_stop(policy["full"], n)
    sim = new_sim(base)
    sim.run(n)
    kept = {(where, first, last): sim.burden_summary(where, first, last) for where in WHERES for first, last in ((1, n), (200, 500), (n, n))}
    sim.keep_burden_baseline()
    same_cases(sim, o_b, note)
    info = sim.burden_baseline_info()
    assert info["steps"] == n and info["params"].seed == base["ep"].seed
    # the run against itself averts nothing
    got = sim.burden_compare("group")
    assert not any(got[k + "_averted"].any() for k in beds.TOTALS) and got["bed_steps_baseline"].any()
    b, c = sim.burden_compare_series("occupancy", "home", stride=1)
    same(b, c, note + ": the run against itself")
    sim.restart(**over)
    sim.run(n)
    check_compare(sim, base["cols"], o_b, n, o_p, n, note, kept)
    same_cases(sim, o_b, note + ", after the policy run")
    check_untouched(sim, policy)
    return sim


# ---- the three pairs --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(beds.PAIRS))
def test_the_pairs_of_the_reference_by_all_by_home_area_and_by_group(name):
    base, policy = beds.PAIRS[name]()
    sim = check_pair(base, policy, POLICY[name], name)
    got = sim.burden_compare("all")
    if name == "fixture_a":
        assert (int(got["bed_steps_averted"][0]), int(got["admissions_averted"][0]), int(got["deaths_averted"][0])) == (19790 - 17294, 152 - 137, 42 - 38)
    if name == "w2_seed":
        assert int(got["admissions_averted"][0]) == 0 and int(got["deaths_averted"][0]) == 130 - 146 and int(got["bed_steps_averted"][0]) == 57336 - 56424
    sim.close()


# ---- edges --------------------------------------------------------------------------------------------------------------------------
def test_all_thresholds_zero_an_empty_list():
    world = ref.world_w2()
    sim = new_sim(world, dict(T, admit_thr=np.zeros(8, np.uint32), death_thr=np.zeros(8, np.uint32)))
    sim.run(300)
    sim.keep_burden_baseline()
    got = sim.burden_baseline_cases()
    assert all(got[k].shape == (0,) for k in CASE_KEYS) and sim.burden_baseline_info()["n_admitted"] == 0
    sim.restart(seed=5)
    sim.run(300)
    for where in WHERES:
        got = sim.burden_compare(where)
        assert not any(v.any() for v in got.values()), where
        for what in WHATS:
            assert not any(x.any() for x in sim.burden_compare_series(what, where)), (what, where)
    sim.close()


@pytest.mark.parametrize("stop", (96, 120))
def test_a_baseline_shorter_than_the_run_keeps_what_lies_beyond_it_and_refuses_windows_beyond_it(stop):
    """Kept at step 96 the list holds the four admitted index cases, three of them with an end beyond the run; at step 120 ten
    cases, some admitted beyond it.  They are in the list and in no row; the current run, which goes on, has them in its rows."""
    world = ref.fixture_a()
    o_b, o_c = ref.at_stop(world["full"], stop), ref.at_stop(world["full"], 700)
    assert (o_b["end_step"][o_b["admitted"]] > stop).any() and (stop == 96 or (o_b["admit_step"][o_b["admitted"]] > stop).any())
    sim = new_sim(world)
    sim.run(stop)
    sim.keep_burden_baseline()
    same_cases(sim, o_b, "kept at %d" % stop)
    sim.run(700 - stop)
    check_compare(sim, world["cols"], o_b, stop, o_c, 700, "kept at %d, 700 run" % stop)
    # rows whose stride reaches beyond the baseline: its events stop at its own last step, the run's go on
    for what in ("admissions", "deaths"):
        b, c = sim.burden_compare_series(what, "all", stop - 50, 1, 200)
        same(b, beds.rows(o_b, what, *world["cols"]["all"], stop, stop - 50, 1, 200), what + ": a row across the baseline's end, baseline")
        same(c, beds.rows(o_c, what, *world["cols"]["all"], 700, stop - 50, 1, 200), what + ": a row across the baseline's end, current")
    assert int(c.sum()) > int(b.sum())
    out = np.full(1, 777, np.uint64)
    lib, ctx = sim.lib, sim._ctx
    assert lib.esim_burden_compare(ctx, _lib.BY_ALL, 1, stop + 1, out.ctypes.data_as(u64p), None, None, None, None, None) == ERANGE and out[0] == 777
    assert lib.esim_burden_compare_series(ctx, _lib.BY_ALL, 1, stop, 2, 1, 0, None, None) == ERANGE
    assert lib.esim_burden_compare_series(ctx, _lib.BY_ALL, 1, stop, 1, 1, 0, None, None) == 0
    sim.close()


def test_population_that_is_not_home_sorted():
    pop, ep = _area_ref.fixture_a()
    per = _area_ref.permuted(pop)
    labels, n_groups = per.age_bands(ref._group_ref.AGE_EDGES)
    base = ref.build(per, ep, labels, n_groups, 500)
    policy = beds.arm(base, mask_effectiveness=1.0)
    assert int(ref.at_stop(base["full"], 500)["admitted"].sum()) > int(ref.at_stop(policy["full"], 500)["admitted"].sum()) >= 20
    check_pair(base, policy, dict(mask_effectiveness=1.0), "permuted").close()


def areas100_pair():
    if "pair" not in _cache:
        base = bg.areas100()
        _cache["pair"] = (base, beds.arm(base, vaccination_rate=6))
    return _cache["pair"]


_cache = {}


def test_more_columns_than_an_lds_table_holds():
    base, policy = areas100_pair()
    assert base["pop"].n_areas > 64 and (ref.at_stop(base["full"], 600)["admitted"] != ref.at_stop(policy["full"], 600)["admitted"]).any()
    check_pair(base, policy, dict(vaccination_rate=6), "100 areas").close()


def test_the_baseline_survives_restart_reset_snapshot_and_rollback_and_what_drops_it():
    world = ref.world_w2()
    n = 402
    o = ref.at_stop(world["full"], n)
    sim = new_sim(world)
    sim.run(n)
    sim.keep_burden_baseline()
    sim.keep_baseline()                                                           # the two baselines are independent
    sim.restart(seed=7)
    sim.run(50)
    sim.reset()
    sim.run(60)
    sim.snapshot()
    sim.run(40)
    sim.rollback()
    sim.drop_baseline()
    same_cases(sim, o, "after restart, reset, snapshot and rollback")
    assert sim.burden_baseline_info()["steps"] == n
    sim.restart(seed=int(world["ep"].seed))
    sim.run(n)
    check_compare(sim, world["cols"], o, n, o, n, "the same run again")
    assert not sim.burden_compare("home")["bed_steps_averted"].any()
    sim.set_groups(world["labels"], world["n_groups"])                            # the same group count: tables and baseline stay
    same_cases(sim, o, "after set_groups with the same count")
    # a later keep replaces it, with a longer list (the allocation grows)
    sim.run(900 - n)
    sim.keep_burden_baseline()
    same_cases(sim, ref.at_stop(world["full"], 900), "a later keep")
    for drop in (lambda: sim.set_burden(T), sim.drop_burden, sim.drop_burden_baseline, lambda: sim.set_groups(world["labels"] % 4, 4)):
        drop()
        for call in (sim.burden_baseline_info, sim.burden_baseline_cases, sim.drop_burden_baseline):
            with pytest.raises(_lib.EsimError) as e:
                call()
            assert e.value.code == ESTATE
        sim.set_groups(world["labels"], world["n_groups"])
        sim.set_burden(T)
        sim.keep_burden_baseline()
        assert sim.burden_baseline_info()["n_admitted"] == 475
    ps = world["pop"].as_struct()
    _lib.check(sim.lib.esim_upload_population(sim._ctx, C.byref(ps)), sim._ctx)    # an upload drops it with everything else
    assert sim.lib.esim_burden_baseline_info(sim._ctx, None, None, None, None) == ESTATE
    sim.close()


def test_both_arms_as_branches_from_one_snapshot_under_another_seed():
    """No vaccination programme, so that the onsets follow from the exposure log alone.  Both arms share 250 steps under seed 321
    and go on under seed 99: the baseline's list honours the seam (onsets up to step 250 drew under the old seed)."""
    pop, _, labels, n_groups = ref.w2()
    ep = _lib.default_params(exposure_chance=0.02, lockdown_threshold=2.0, mask_pt_threshold=2.0, mask_everywhere_threshold=2.0,
                             vaccination_threshold=2.0, seed=321, max_steps=600)
    cols = {where: ref._curve_ref.labels_for(pop, where, (labels, n_groups)) for where in WHERES}
    sim = Simulator(pop, ep)
    sim.set_groups(labels, n_groups)
    sim.set_burden(T)
    sim.run(250)
    sim.snapshot()
    arms = []
    for over in (dict(seed=99), dict(seed=99, exposure_chance=0.01)):
        sim.rollback(**over)
        sim.run(350)
        cit, step, _ = sim.exposure_events()
        onset = np.full(pop.n_citizens, NEVER, np.int64)
        onset[cit] = step.astype(np.int64) + int(ep.exposed_time) + 1
        onset[np.unique(pop.seeds)] = 0
        onset[onset > 600] = NEVER
        full = ref.outcomes(onset, labels, T, lambda s: 321 if s <= 250 else 99, pop.citizen_id_base)
        arms.append(full)
        if len(arms) == 1:
            sim.keep_burden_baseline()
            same_cases(sim, full, "the baseline branch")
            assert (ref.outcomes(onset, labels, T, lambda s: 99)["admitted"] != full["admitted"]).any()
    assert (arms[0]["admitted"] != arms[1]["admitted"]).any()
    check_compare(sim, cols, arms[0], 600, arms[1], 600, "two branches")
    sim.close()


# ---- ensembles ----------------------------------------------------------------------------------------------------------------------
def a_of_seed(seed):
    key = ("a", seed)
    if key not in _cache:
        _cache[key] = beds.arm(ref.fixture_a(), seed=seed) if seed != int(ref.fixture_a()["ep"].seed) else ref.fixture_a()
    return _cache[key]


def w2_of(seed, rate):
    key = ("w2", seed, rate)
    if key not in _cache:
        base = ref.world_w2()
        _cache[key] = base if (seed, rate) == (int(base["ep"].seed), 1) else beds.arm(base, seed=seed, vaccination_rate=rate)
    return _cache[key]


def test_burden_series_kind_over_four_seeds_and_the_flag_hazard():
    seeds = (int(ref.fixture_a()["ep"].seed), 5, 6, 7)
    worlds = [a_of_seed(s) for s in seeds]
    lab, n_cols = worlds[0]["cols"]["group"]
    window = dict(first_step=1, n_rows=29, stride=24)
    sim = new_sim(worlds[0])
    for what, min_count in (("occupancy", 10), ("admissions", 2), ("deaths", 1)):
        planes = [ref.series(ref.at_stop(w["full"], 700), what, lab, n_cols, 700, 1, 29, 24) for w in worlds]
        sim.ensemble_begin_burden_series("group", what, min_count=min_count, **window)
        sim.ensemble_keep_members(4, "value")
        for seed, plane in zip(seeds, planes):
            sim.restart(seed=seed)
            sim.run(700)
            sim.ensemble_fold()
            same(sim.burden_series(what, "group", 1, 29, 24), plane, "%s: member of seed %d" % (what, seed))
        got, want = sim.ensemble_read_series(), beds.fold_rows(planes, min_count)
        assert got["members"] == 4 and want["hit"].any() and (want["hit"] < 4).any(), what
        for k in ("hit", "sum", "sumsq"):
            same(got[k], want[k], "%s: accumulator %s" % (what, k))
        ordered = np.sort(np.stack(planes), axis=0)
        same(sim.ensemble_quantiles((0.5,))[0], ordered[1], what + ": the median (inverted CDF: the second smallest of four)")
        same(sim.ensemble_exceedance((min_count,))[0], (ordered >= min_count).sum(axis=0).astype(np.uint32), what + ": members at the capacity or above")
    # a fold beyond the member's steps folds nothing (a begin of its own: the store above is full, which is ESIM_ERANGE too)
    sim.ensemble_begin_burden_series("group", "deaths", **window)
    sim.restart(seed=5)
    sim.run(600)
    assert sim.lib.esim_ensemble_fold(sim._ctx) == ERANGE and b"rows outside" in sim.lib.esim_last_error(sim._ctx) and sim.ensemble_read_series()["members"] == 0
    sim.run(100)
    # the flag hazard: a settings begin of the same shape (29 rows by 8 groups) reuses the accumulators and must fold settings rows
    sim.ensemble_begin_settings("group", None, **window)
    sim.ensemble_fold()
    got = sim.ensemble_read_series()
    same(got["sum"], sim.setting_series("group", None, 1, 29, 24).astype(np.uint64), "a settings begin of the same shape after the burden kind")
    assert got["members"] == 1 and (got["sum"] != sim.burden_series("deaths", "group", 1, 29, 24)).any()
    # and back: the burden kind after the settings kind folds beds again
    sim.ensemble_begin_burden_series("group", "occupancy", **window)
    sim.ensemble_fold()
    same(sim.ensemble_read_series()["sum"], sim.burden_series("occupancy", "group", 1, 29, 24).astype(np.uint64), "the burden kind after the settings kind")
    sim.drop_burden()
    assert sim.lib.esim_ensemble_fold(sim._ctx) == ESTATE and sim.ensemble_read_series()["members"] == 1
    sim.close()


def test_burden_paired_kind_over_four_seeds_and_the_flag_hazard():
    seeds = (321, 5, 6, 7)
    pairs = [(w2_of(s, 1), w2_of(s, 3)) for s in seeds]
    lab, n_cols = pairs[0][0]["cols"]["group"]
    window = dict(first_step=1, n_rows=38, stride=24)
    sim = new_sim(pairs[0][0])
    for what, cumulative, min_b, min_a in (("occupancy", False, 5, 3), ("admissions", True, 1, 2), ("deaths", False, 1, 1)):
        planes = [tuple(beds.rows(ref.at_stop(w["full"], 900), what, lab, n_cols, 900, 1, 38, 24, cumulative) for w in pair) for pair in pairs]
        sim.ensemble_begin_burden_paired("group", what, cumulative=cumulative, min_baseline=min_b, min_averted=min_a, **window)
        sim.ensemble_keep_members(4, "value")
        for seed, plane in zip(seeds, planes):
            sim.restart(seed=seed, vaccination_rate=1)
            sim.run(900)
            sim.keep_burden_baseline()
            sim.restart(seed=seed, vaccination_rate=3)
            sim.run(900)
            sim.ensemble_fold()
        got, want = sim.ensemble_read_paired(), beds.fold_paired(planes, min_b, min_a)
        assert got["members"] == 4 and want["hit"].any() and (want["hit"] < want["defined"]).any(), what
        for k in sim.PAIRED_KEYS:
            same(got[k], want[k], "%s: accumulator %s" % (what, k))
        diff = np.stack([p[0].astype(np.int64) - p[1].astype(np.int64) for p in planes])
        assert (diff > 0).any() and (cumulative or (diff < 0).any())
        assert sim.ensemble_members_info()["signed"]
        same(sim.ensemble_members().astype(np.int64), diff, what + ": the kept members, baseline - current with their sign")
        same(sim.ensemble_quantiles((0.5,))[0].astype(np.int64), np.sort(diff, axis=0)[1], what + ": the median averted")
    # without a burden baseline the fold is refused and folds nothing (a begin of its own: the store above is full)
    sim.ensemble_begin_burden_paired("group", "deaths", **window)
    sim.drop_burden_baseline()
    assert sim.lib.esim_ensemble_fold(sim._ctx) == ESTATE and b"burden baseline" in sim.lib.esim_last_error(sim._ctx)
    assert sim.ensemble_read_paired()["members"] == 0
    # the flag hazard: an ordinary paired begin of the same shape folds cases, not beds
    sim.keep_baseline()
    sim.ensemble_begin_paired("group", **window)
    sim.ensemble_fold()
    b, c = sim.compare_series("group", 1, 38, 24)
    got = sim.ensemble_read_paired()
    same(got["sum_baseline"], b.astype(np.uint64), "an ordinary paired begin of the same shape after the burden kind")
    same(got["sum_current"], c.astype(np.uint64), "... its current side")
    assert got["sum_baseline"].sum() == got["sum_current"].sum() > 1000
    sim.close()


def test_ensemble_run_with_the_burden_series_kind_and_its_dump(tmp_path):
    seeds = (int(ref.fixture_a()["ep"].seed), 5, 6)
    worlds = [a_of_seed(s) for s in seeds]
    lab, n_cols = worlds[0]["cols"]["group"]
    ens = Ensemble(worlds[0]["pop"], worlds[0]["ep"], group=(worlds[0]["labels"], worlds[0]["n_groups"]), burden=T)
    area = dict(kind="burden_series", what="occupancy", where="group", first_step=1, stride=24, min_count=10, quantiles=(0.5,), exceed=(10,))
    res = ens.run([dict(seed=s) for s in seeds], 700, area=area)
    planes = [ref.series(ref.at_stop(w["full"], 700), "occupancy", lab, n_cols, 700, 1, 30, 24) for w in worlds]
    want = beds.fold_rows(planes, 10)
    a = res.area
    assert res.area_kind == "burden_series" and a["members"] == 3 and a["hit"].shape == (30, n_cols) and a["steps"].tolist() == list(range(1, 700, 24))
    same(a["hit"], want["hit"], "hit: members with ten beds or more")
    assert np.array_equal(a["mean"], want["sum"].astype(np.float64) / 3) and a["var"].shape == a["mean"].shape and want["hit"].any()
    same(a["quantiles"][0], np.sort(np.stack(planes), axis=0)[1], "the median of three")
    same(a["exceed"][0], want["hit"], "exceedance at the capacity")
    with pytest.raises(ValueError):
        ens.run([dict(seed=1)], 50, stop_when_done=True, area=area)
    res.dump(str(tmp_path))
    saved = np.load(str(tmp_path / "ensemble_area_burden_series.npz"))
    assert (saved["hit"] == a["hit"]).all() and (saved["mean"] == a["mean"]).all() and (saved["steps"] == a["steps"]).all() and "var" in saved
    assert not os.path.exists(str(tmp_path / "ensemble_area_series.npz")) and os.path.exists(str(tmp_path / "ensemble_area_quantiles.npz"))
    ens.close()


def test_ensemble_compare_burden_and_its_dump(tmp_path):
    seeds = (321, 5, 6)
    pairs = [(w2_of(s, 1), w2_of(s, 3)) for s in seeds]
    base = pairs[0][0]
    lab, n_cols = base["cols"]["group"]
    ens = Ensemble(base["pop"], base["ep"], group=(base["labels"], base["n_groups"]), burden=T)
    rows = dict(first_step=1, stride=24, min_baseline=5, min_averted=3)
    res = ens.compare_burden(dict(vaccination_rate=1), dict(vaccination_rate=3), [dict(seed=s) for s in seeds], 900, where="group", what="occupancy", rows=rows,
                             quantiles=(0.5,))
    o = [tuple(ref.at_stop(w["full"], 900) for w in pair) for pair in pairs]
    for i, (b, c) in enumerate(o):
        for arm, x in (("_baseline", b), ("_current", c)):
            t = beds.totals(x, lab, n_cols, 900)
            for k in beds.TOTALS:
                same(res.totals[k + arm][i], t[k], "member %d: %s%s" % (i, k, arm))
    want_b = np.stack([beds.totals(b, lab, n_cols, 900)["bed_steps"].astype(np.int64) - beds.totals(c, lab, n_cols, 900)["bed_steps"].astype(np.int64) for b, c in o])
    assert np.array_equal(res.bed_days_averted(), want_b / 24.0) and res.bed_days_averted().shape == (3, n_cols) and (want_b > 0).any()
    same(res.deaths_averted(), np.stack([beds.totals(b, lab, n_cols, 900)["deaths"].astype(np.int64) - beds.totals(c, lab, n_cols, 900)["deaths"] for b, c in o]), "deaths averted")
    assert int(res.totals["bed_steps_baseline"][0].sum()) == 57336 and int(res.totals["bed_steps_current"][0].sum()) == 50400
    planes = [tuple(ref.series(x, "occupancy", lab, n_cols, 900, 1, 38, 24) for x in pair) for pair in o]
    acc = beds.fold_paired(planes, 5, 3)
    same(res.summary["hit"], acc["hit"], "the paired accumulators: hit")
    same(res.summary["defined"], acc["defined"], "the paired accumulators: defined")
    assert res.summary["members"] == 3 and np.array_equal(res.summary["mean_baseline"], acc["sum_baseline"].astype(np.float64) / 3)
    diff = np.stack([p[0].astype(np.int64) - p[1].astype(np.int64) for p in planes])
    same(res.averted_quantiles[0].astype(np.int64), np.sort(diff, axis=0)[1], "the median of beds averted")
    with pytest.raises(ValueError):
        ens.compare_burden({}, dict(index_cases=[1]), [dict(seed=1)], 10)
    with pytest.raises(ValueError):
        ens.compare_burden({}, {}, [dict(seed=1)], 10, quantiles=(0.5,))
    res.dump(str(tmp_path))
    saved = np.load(str(tmp_path / "ensemble_burden_compare.npz"))
    assert (saved["bed_days_averted"] == res.bed_days_averted()).all() and (saved["deaths_averted"] == res.deaths_averted()).all() and str(saved["what"]) == "occupancy"
    assert (saved["summary_hit"] == acc["hit"]).all() and (saved["quantiles"] == res.averted_quantiles).all()
    # compare() goes through the same member loop and gives what it gave
    cmp = ens.compare(dict(vaccination_rate=1), dict(vaccination_rate=3), [dict(seed=321)], 900, where="all")
    assert int(cmp.records_baseline["infected"][0].max()) == int(base["run"]["records"]["infected"].max())
    assert int(cmp.counts[0, 0, _lib.CMP_AVERTED]) > 0 and (cmp.records_policy["time_step"][0] == np.arange(1, 901)).all()
    ens.close()


# ---- grids capped to one and three workgroups --------------------------------------------------------------------------------------
CSRC = bg.CSRC


def beds_sites():
    """[(first line, last line)] of every grid_capped call of esim_host_beds.h, as test_burden_gpu.burden_sites finds them."""
    lines = open(os.path.join(CSRC, "esim_host_beds.h")).read().split("\n")
    out = []
    for no, line in enumerate(lines, 1):
        if re.search(r"\bgrid_capped\(", line) and not line.lstrip().startswith("//"):
            last = no
            while not lines[last - 1].split("//")[0].rstrip().endswith(";"):
                last += 1
            out.append((no, last))
    return out


def everybody_admitted(sim_seen):
    """W2 with every case admitted: lists of 1835 entries, so that the consumers' grids are clipped at three workgroups too."""
    world = ref.world_w2()
    tables = dict(T, admit_thr=np.full(8, 0xFFFFFFFF, np.uint32))
    full = ref.outcomes(world["run"]["onset"], world["labels"], tables, lambda s: int(world["ep"].seed), world["pop"].citizen_id_base)
    o = ref.at_stop(full, 900)
    assert int(o["admitted"].sum()) >= 1835 - 1                                     # (a block's first word can be 0xFFFFFFFF)
    sim = new_sim(world, tables)
    sim.run(900)
    sim.keep_burden_baseline()
    same_cases(sim, o, "everybody admitted")
    check_compare(sim, world["cols"], o, 900, o, 900, "everybody admitted")
    # a fold of many cells: the fold kernels' grid is clipped too
    lab, n_cols = world["cols"]["group"]
    sim.ensemble_begin_burden_series("group", "occupancy", 1, 900, 1, 50)
    sim.ensemble_fold()
    same(sim.ensemble_read_series()["sum"], ref.series(o, "occupancy", lab, n_cols, 900).astype(np.uint64), "everybody admitted: a fold of 7200 cells")
    sim.ensemble_begin_burden_paired("group", "admissions", 1, 900, 1, True)
    sim.ensemble_fold()
    got = sim.ensemble_read_paired()
    same(got["sum_baseline"], beds.rows(o, "admissions", lab, n_cols, 900, cumulative=True).astype(np.uint64), "everybody admitted: a paired fold of 7200 cells")
    same(got["sum_current"], got["sum_baseline"], "... its current side")
    sim_seen(sim)
    sim.close()


@pytest.mark.parametrize("cap", (1, 3))
def test_grids_capped_to_one_and_three_workgroups(cap, monkeypatch, tmp_path):
    monkeypatch.setenv("ESIM_GRID_CAP", str(cap))
    seen, collect = {}, {}

    def note(sim, into=None):
        for site, r in sim.debug_launches().items():
            m = re.fullmatch(r"esim_host_beds\.h:(\d+)", site)
            if m and r["clipped"]:
                line = int(m.group(1))
                seen[line] = max(seen.get(line, 0), r["max_trips"])
                if into is not None:
                    into[line] = max(into.get(line, 0), r["max_trips"])

    base, policy = beds.pair_a()
    sim = check_pair(base, policy, POLICY["fixture_a"], "fixture A, cap %d" % cap)
    note(sim, collect)
    sim.close()
    for name in ("w2", "w2_seed"):
        sim = check_pair(*beds.PAIRS[name](), POLICY[name], "%s, cap %d" % (name, cap))
        note(sim)
        sim.close()
    sim = check_pair(*areas100_pair(), dict(vaccination_rate=6), "100 areas, cap %d" % cap)
    note(sim)
    sim.close()
    everybody_admitted(note)
    # the edges and the ensemble kinds once more under the cap
    test_all_thresholds_zero_an_empty_list()
    for stop in (96, 120):
        test_a_baseline_shorter_than_the_run_keeps_what_lies_beyond_it_and_refuses_windows_beyond_it(stop)
    test_population_that_is_not_home_sorted()
    test_the_baseline_survives_restart_reset_snapshot_and_rollback_and_what_drops_it()
    test_both_arms_as_branches_from_one_snapshot_under_another_seed()
    test_burden_series_kind_over_four_seeds_and_the_flag_hazard()
    test_burden_paired_kind_over_four_seeds_and_the_flag_hazard()
    test_ensemble_run_with_the_burden_series_kind_and_its_dump(tmp_path / "run")
    test_ensemble_compare_burden_and_its_dump(tmp_path / "compare")
    test_error_table()
    test_a_shard_and_a_communicator_of_two_ranks_are_refused()
    sites = beds_sites()
    assert len(sites) == 5
    for first, last in sites:
        trips = max((t for line, t in seen.items() if first <= line <= last), default=0)
        assert trips >= (3 if cap == 1 else 2), "esim_host_beds.h:%d under ESIM_GRID_CAP=%d: clipped with %d trips" % (first, cap, trips)
    if cap == 1:
        # fixture A's log has over 700 entries: the wavefront compaction of k_beds_collect runs across trips and workgroups' worth of entries
        first, last = sites[0]
        assert "k_beds_collect" in "".join(open(os.path.join(CSRC, "esim_host_beds.h")).read().split("\n")[first - 1:last])
        assert max((t for line, t in collect.items() if first <= line <= last), default=0) >= 3


# ---- errors -------------------------------------------------------------------------------------------------------------------------
def outputs(n_cols, fill=12345):
    out = {k: np.full(n_cols, fill, np.uint64 if k.startswith("bed") else np.uint32) for k in ("bed_b", "bed_c", "adm_b", "adm_c", "dth_b", "dth_c")}
    out["rows_b"], out["rows_c"] = np.full((4, n_cols), fill, np.uint32), np.full((4, n_cols), fill, np.uint32)
    out["cases"] = np.full((3, 8), fill, np.uint32)
    out["died"] = np.full(8, 77, np.uint8)
    out["n"] = np.full(1, fill, np.uint32)
    return out


def untouched(out, fill=12345, n_too=True):
    return all((v == (77 if k == "died" else fill)).all() for k, v in out.items() if n_too or k != "n")


def calls(lib, ctx, out, where, first=1, last=10, n_rows=4, what=_lib.BURDEN_OCCUPANCY):
    """The return codes of the calls that compute or begin: compare, compare_series, begin_burden_series, begin_burden_paired."""
    p = lambda k: out[k].ctypes.data_as(u64p if out[k].dtype == np.uint64 else u32p)
    return (lib.esim_burden_compare(ctx, where, first, last, p("bed_b"), p("bed_c"), p("adm_b"), p("adm_c"), p("dth_b"), p("dth_c")),
            lib.esim_burden_compare_series(ctx, where, what, first, n_rows, 1, 0, p("rows_b"), p("rows_c")),
            lib.esim_ensemble_begin_burden_series(ctx, where, what, first, n_rows, 1, 1),
            lib.esim_ensemble_begin_burden_paired(ctx, where, what, first, n_rows, 1, 0, 1, 1))


def kept_calls(lib, ctx, out):
    """keep, info, read, drop."""
    c = out["cases"]
    return (lib.esim_burden_baseline_keep(ctx), lib.esim_burden_baseline_info(ctx, None, None, None, None),
            lib.esim_burden_baseline_read(ctx, c[0].ctypes.data_as(u32p), c[1].ctypes.data_as(u32p), c[2].ctypes.data_as(u32p), out["died"].ctypes.data_as(u8p), 8,
                                          out["n"].ctypes.data_as(u32p)),
            lib.esim_burden_baseline_drop(ctx))


def test_error_table():
    world = ref.world_w2()
    pop, ep, labels, n_groups = world["pop"], world["ep"], world["labels"], world["n_groups"]
    n10 = int(ref.at_stop(world["full"], 10)["admitted"].sum())                                                          # the admitted index cases
    assert 0 < n10 <= 8
    lib = _lib.load()
    ALL, HOME, GROUP = _lib.BY_ALL, _lib.AREA_HOME, _lib.BY_GROUP
    out = outputs(pop.n_areas)
    p = lambda k: out[k].ctypes.data_as(u64p if out[k].dtype == np.uint64 else u32p)

    def fresh():
        for k, v in out.items():
            v[...] = 77 if k == "died" else 12345

    bare = C.c_void_p()
    _lib.check(lib.esim_create(C.byref(ep), C.byref(bare)))
    assert calls(lib, bare, out, HOME) == (ESTATE,) * 4 and kept_calls(lib, bare, out) == (ESTATE,) * 4                # before an upload
    lib.esim_destroy(bare)
    assert calls(lib, None, out, HOME) == (EINVAL,) * 4 and kept_calls(lib, None, out) == (EINVAL,) * 4                 # null context
    sim = Simulator(pop, ep)
    sim.run(10)
    ctx = sim._ctx
    assert calls(lib, ctx, out, HOME) == (ESTATE,) * 4 and b"esim_burden_set" in lib.esim_last_error(ctx)               # no tables set
    assert kept_calls(lib, ctx, out) == (ESTATE,) * 4 and untouched(out)
    sim.set_groups(labels, n_groups)
    sim.set_burden(T)
    got = calls(lib, ctx, out, HOME)
    assert got[:2] == (ESTATE, ESTATE) and b"burden baseline" in lib.esim_last_error(ctx) and got[2:] == (0, 0)          # tables, no baseline: the begins need none
    assert lib.esim_ensemble_fold(ctx) == ESTATE and b"burden baseline" in lib.esim_last_error(ctx)                      # ... the paired fold does
    assert untouched(out)
    assert kept_calls(lib, ctx, out) == (0, 0, 0, 0) and out["n"][0] == n10 and (out["cases"][:, n10:] == 12345).all()   # kept, read into room for 8, dropped
    assert (out["cases"][1, :n10] <= out["cases"][2, :n10]).all() and lib.esim_burden_baseline_info(ctx, None, None, None, None) == ESTATE
    fresh()
    assert lib.esim_burden_baseline_keep(ctx) == 0
    assert lib.esim_burden_baseline_read(ctx, None, None, None, None, 0, None) == EINVAL                                 # null n_out
    assert lib.esim_burden_baseline_read(ctx, p("cases"), None, None, None, n10 - 1, p("n")) == ERANGE and out["n"][0] == n10   # the sized call
    assert (out["cases"] == 12345).all() and lib.esim_burden_baseline_read(ctx, None, None, None, None, n10, p("n")) == 0  # every array NULL
    fresh()
    for where in (_lib.AREA_CURRENT, _lib.BY_SETTING, 5, -1):
        assert calls(lib, ctx, out, where) == (EINVAL,) * 4, where
    for what in (3, -1):
        assert calls(lib, ctx, None_out(out), HOME, what=what)[1:] == (EINVAL,) * 3, what
    assert calls(lib, ctx, None_out(out), HOME, n_rows=0)[1:] == (EINVAL,) * 3                                           # no rows
    assert lib.esim_burden_compare_series(ctx, HOME, 1, 1, 4, 0, 0, p("rows_b"), p("rows_c")) == EINVAL                  # stride 0
    assert lib.esim_ensemble_begin_burden_series(ctx, HOME, 1, 1, 4, 0, 1) == EINVAL and lib.esim_ensemble_begin_burden_paired(ctx, HOME, 1, 1, 4, 0, 0, 1, 1) == EINVAL
    assert lib.esim_burden_compare_series(ctx, HOME, _lib.BURDEN_OCCUPANCY, 1, 4, 1, 1, p("rows_b"), p("rows_c")) == EINVAL   # cumulative occupancy
    assert lib.esim_ensemble_begin_burden_paired(ctx, HOME, _lib.BURDEN_OCCUPANCY, 1, 4, 1, 1, 1, 1) == EINVAL
    assert lib.esim_ensemble_begin_burden_paired(ctx, HOME, _lib.BURDEN_DEATHS, 1, 4, 1, 1, 1, 0) == EINVAL              # min_averted 0
    assert calls(lib, ctx, out, HOME, first=0) == (ERANGE,) * 4                                                          # first_step 0
    assert lib.esim_burden_compare(ctx, HOME, 5, 4, p("bed_b"), p("bed_c"), p("adm_b"), p("adm_c"), p("dth_b"), p("dth_c")) == ERANGE   # last_step < first_step
    assert lib.esim_burden_compare(ctx, ALL, 1, 11, p("bed_b"), p("bed_c"), p("adm_b"), p("adm_c"), p("dth_b"), p("dth_c")) == ERANGE   # beyond the steps run
    assert lib.esim_burden_compare_series(ctx, ALL, 1, 8, 4, 1, 0, p("rows_b"), p("rows_c")) == ERANGE
    assert untouched(out)
    sim.set_groups(None)                                                                                                  # the labels gone: tables and baseline with them
    assert calls(lib, ctx, out, ALL) == (ESTATE,) * 4 and kept_calls(lib, ctx, out) == (ESTATE,) * 4 and untouched(out)
    sim.set_burden(dict(T, admit_thr=T["admit_thr"][-1:], death_thr=T["death_thr"][-1:]))                                 # one group needs no labels ...
    assert lib.esim_burden_baseline_keep(ctx) == 0 and calls(lib, ctx, out, GROUP) == (ESTATE,) * 4 and untouched(out)   # ... by group does
    sim.set_groups(labels, n_groups)
    sim.set_burden(T)
    sim.run(890)                                                                                                          # the context is usable afterwards
    sim.keep_burden_baseline()
    o = ref.at_stop(world["full"], 900)
    check_compare(sim, world["cols"], o, 900, o, 900, "after the refusals")
    assert lib.esim_burden_compare(ctx, GROUP, 1, 900, *([None] * 6)) == 0 and lib.esim_burden_compare_series(ctx, GROUP, 1, 1, 4, 1, 0, None, None) == 0
    sim.close()


def None_out(out):
    """Outputs of their own for a call of which one part may succeed."""
    return {k: v.copy() for k, v in out.items()}


def test_a_shard_and_a_communicator_of_two_ranks_are_refused():
    lib = _lib.load()
    whole = Population.synthetic("york", n_citizens=20000, n_areas=64, citizens_per_school=2500, n_seeds=20)
    cuts = whole.even_cuts(2)
    s0, s1 = whole.shard(cuts, 0), whole.shard(cuts, 1)
    out = outputs(whole.n_areas, 4242)
    out["died"][:] = 77
    ep = _lib.default_params(exposure_chance=0.004, seed=123)
    one, keep_arrays = bg.params_of(dict(T, admit_thr=T["admit_thr"][-1:], death_thr=T["death_thr"][-1:]))

    def communicator(sim, rank_1_row):
        def allreduce(user, which, host_ptr, n_u32):
            if which == 8:                               # the set-up's layout check: rank 1's row, as its process would add it
                a = (C.c_uint32 * n_u32).from_address(host_ptr)
                a[5:10] = rank_1_row
            return 0
        cb = _lib.ALLREDUCE_FN(allreduce)
        _lib.check(lib.esim_comm_init_callback(sim._ctx, cb, None, 0, 2), sim._ctx)
        return cb                                        # (kept alive by the caller)

    sim = Simulator(s0, ep)
    assert calls(lib, sim._ctx, out, _lib.BY_ALL, 1, 1, 1) == (ESTATE,) * 4 and lib.esim_burden_baseline_keep(sim._ctx) == ESTATE    # a shard
    assert untouched(out, 4242)
    sim.close()
    sim = Simulator(whole, ep)
    sim.run(120)
    assert lib.esim_burden_set(sim._ctx, C.byref(one)) == 0
    sim.keep_burden_baseline()
    assert calls(lib, sim._ctx, out, _lib.AREA_HOME, 1, 120, 4)[:2] == (0, 0)
    for v in out.values():
        v[...] = 77 if v.dtype == np.uint8 else 4242
    keep = communicator(sim, [whole.n_citizens, 0, whole.n_citizens, 0, 0])                   # rank 1 holds nobody
    assert calls(lib, sim._ctx, out, _lib.AREA_HOME, 1, 120, 4) == (ESTATE,) * 4 and b"ranks" in lib.esim_last_error(sim._ctx) and untouched(out, 4242)
    assert lib.esim_burden_baseline_keep(sim._ctx) == ESTATE and b"ranks" in lib.esim_last_error(sim._ctx)
    assert lib.esim_burden_baseline_info(sim._ctx, None, None, None, None) == 0               # the baseline kept before stays
    del keep
    sim.close()
