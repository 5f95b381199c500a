"""The hospital burden (esim_burden_outcomes, _series, _summary) and the lists of admitted cases (esim_burden_baseline_*,
esim_burden_compare, esim_burden_compare_series, the burden-series kind of the ensemble accumulators) at the limits of the severity
tables and at the 27 edges of esim_params (tests/_burden_edges.py; tests/test_burden_edges.py checks on the CPU that no case is
inert and that a nearly right rule would show): a. every table set, b. the LDS boundaries of the kernels, c. the 27 cases under
table set edge_e, d. six of them at pipeline level 0 on the permuted world, e. grids capped to one and three workgroups, f. what
esim_burden_set refuses at the same edges, g. the seam of a rollback under another seed at its exact step.  Every comparison is
exact integer equality against the numpy reference over the CPU oracle (tests/_burden_ref.py, tests/_beds_ref.py).

Not reached at test size, and not faked: the `keyed == false` path of k_beds_rows needs more than 2^32 cells of rows, and the
`at >= l.cap` guard of k_beds_collect a list longer than the log it was made from."""
import ctypes as C
import re

import numpy as np
import pytest

import _beds_ref as beds
import _burden_edges as be
import _burden_ref as ref
import _replay_edges as edges
import _setting_ref as setting
import test_beds_gpu as bd
import test_burden_gpu as bg
from epidemicsimulator_amd import Simulator, _lib

pytestmark = pytest.mark.gpu

N, NEVER, WHERES, WHATS = be.N, be.NEVER, ref.WHERES, ref.WHATS
EINVAL = -1
same = bg.same
LDS_ROWS = ((64, 6), (65, 6))                    # (n_rows, stride) from step 1: with 64 columns 4096 cells, the last size k_beds_rows builds in LDS, and 4160
CAPPED_SETS = ("bins_64", "groups_1024", "one_group_65")


def started(w, level=None):
    """The run of the world under its tables, its own records against the oracle's first."""
    sim = Simulator(w["pop"], setting.copy_params(w["ep"]))
    if level is not None:
        sim.set_pipeline(level)
    sim.set_groups(w["labels"], w["n_groups"])
    sim.set_burden(w["tables"])
    rec = sim.run(N)
    for k in ("exposures_building", "exposures_bus", "infected", "vaccinated_now"):
        same(rec[k], w["run"]["records"][k], "the run itself vs the oracle: " + k)
    return sim


def check_run(sim, w, note):
    """Outcomes, the three series by all / home / group at stride 1 and at stride 24 from step 3, the summaries."""
    bg.check_world(sim, w["cols"], be.outcomes(w), N, note, series=be.SERIES, summaries=be.spans(w))


def check_lists(sim, w, note):
    """The kept list, its info, and the run against itself: totals and rows of both sides against the reference, nothing averted."""
    o = be.outcomes(w)
    sim.keep_burden_baseline()
    bd.same_cases(sim, o, note)
    info = sim.burden_baseline_info()
    assert info["steps"] == N and info["params"].seed == w["ep"].seed and info["n_admitted"] == int(o["admitted"].sum()), note
    bd.check_compare(sim, w["cols"], o, N, o, N, note + ", against itself", spans=[s[:2] for s in be.spans(w)[::2]], series=be.SERIES)
    for where in WHERES:
        got = sim.burden_compare(where)
        assert not any(got[k + "_averted"].any() for k in beds.TOTALS) and (got["bed_steps_baseline"].any() or not o["admitted"].any()), (note, where)
        for what in WHATS:
            b, c = sim.burden_compare_series(what, where, stride=1)
            same(b, c, "%s: %s by %s, the run against itself" % (note, what, where))


def check_everything(sim, w, note):
    check_run(sim, w, note)
    check_lists(sim, w, note)


def check_rows(sim, w, where, note, shapes=LDS_ROWS):
    """Rows of the given shapes from step 1 through every way that makes rows: esim_burden_series (the log), esim_burden_compare_series
    (both lists) and one fold of the burden-series kind (the scratch list); a list must be kept."""
    o = be.outcomes(w)
    lab, n_cols = w["cols"][where]
    for n_rows, stride in shapes:
        for what in WHATS:
            want = ref.series(o, what, lab, n_cols, N, 1, n_rows, stride)
            tag = "%s: %s by %s, %d rows of %d columns" % (note, what, where, n_rows, n_cols)
            same(sim.burden_series(what, where, 1, n_rows, stride), want, tag + ", burden_series")
            b, c = sim.burden_compare_series(what, where, 1, n_rows, stride)
            same(b, want, tag + ", compare_series, baseline")
            same(c, want, tag + ", compare_series, current")
            sim.ensemble_begin_burden_series(where, what, 1, n_rows, stride, min_count=2)
            sim.ensemble_fold()
            got = sim.ensemble_read_series()
            assert got["members"] == 1, tag
            same(got["sum"], want.astype(np.uint64), tag + ", the fold's sum")
            same(got["hit"], (want >= 2).astype(np.uint32), tag + ", the fold's hit")
            same(got["sumsq"], want.astype(np.uint64) ** 2, tag + ", the fold's sumsq")


def table_set(name, note=None):
    w = be.world(name)
    sim = bg.check_stops(w, (N,), note or name, tables=w["tables"], series=be.SERIES, summaries=be.spans(w))
    check_lists(sim, w, note or name)
    return sim, w


# ---- a. every table set; b. the LDS boundaries -----------------------------------------------------------------------------------------
def test_bins_64_every_bin_of_both_cdfs():
    sim, w = table_set("bins_64")
    # the stride-1 rows by home are 400 x 8 = 3200 cells (LDS), by all 400 cells: check_lists went through both
    assert w["cols"]["home"][1] * N == 3200 and w["cols"]["all"][1] * N == 400
    got = sim.burden_outcomes()
    a = got["admit_step"] != NEVER
    n_delay, n_stay = got["admit_step"][a].astype(np.int64) - w["full"]["onset"][a], got["end_step"][a].astype(np.int64) - got["admit_step"][a] - 1
    assert sorted(set(n_delay.tolist())) == list(range(65)) and sorted(set(n_stay.tolist())) == list(range(65))
    bg.check_untouched(sim, w)
    sim.close()


@pytest.mark.parametrize("name", ("bins_64_unit_max", "bins_0_unit_max"))
def test_units_of_65535_end_steps_of_millions_beside_the_died_bit(name):
    sim, w = table_set(name)
    o = be.outcomes(w)
    got, want = sim.burden_baseline_cases(), beds.cases(o)
    assert got["end_step"].dtype == np.uint32 and (got["end_step"] < 2 ** 31).all() and (got["end_step"] > N).all()
    same(got["died"], want["died"], name + ": died of the kept list")
    assert int(got["end_step"].max()) == int(o["end_step"][o["admitted"]].max()) >= (8_000_000 if name == "bins_64_unit_max" else 65535)
    assert sim.burden_baseline_info()["n_died"] == int(want["died"].sum()) > 0
    if name == "bins_0_unit_max":                    # everybody in a bed from the onset to beyond the run: the running count of cases
        occ = sim.burden_series("occupancy", "all")[:, 0]
        same(occ, np.cumsum(np.bincount(w["full"]["onset"][o["case"]], minlength=N + 1))[1:].astype(np.uint32), "the running count of cases")
    sim.close()


def test_flat_cdf_repeated_entries_and_both_extremes():
    sim, w = table_set("flat_cdf")
    sim.close()


def test_groups_1024_the_whole_threshold_table_and_1024_columns():
    sim, w = table_set("groups_1024")
    assert w["cols"]["group"][1] == 1024 and len(sim.burden()["admit_thr"]) == 1024
    check_rows(sim, w, "group", "groups_1024", shapes=((4, 96), (5, 96)))        # 4096 and 5120 cells of 1024 columns
    sim.close()


@pytest.mark.parametrize("name", ("one_group_64", "one_group_65"))
def test_64_and_65_columns_and_rows_of_4096_cells_and_more(name):
    sim, w = table_set(name)
    n_cols = w["cols"]["group"][1]
    assert n_cols == int(name[-2:]) and len(sim.burden()["admit_thr"]) == 1
    check_rows(sim, w, "group", name)
    if n_cols == 64:
        assert [r * n_cols for r, _ in LDS_ROWS] == [4096, 4160]
    bg.check_untouched(sim, w)
    sim.close()


# ---- c. the 27 cases under edge_e ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", be.CASES)
def test_every_case_of_the_parameter_edges_under_edge_e(name):
    w = be.world("edge_e", name)
    sim = started(w)
    check_everything(sim, w, name)
    bg.check_untouched(sim, w)
    # the kept list against the same case under another seed
    other = be.world("edge_e", name, False, be.OTHER_SEED)
    sim.restart(seed=be.OTHER_SEED)
    sim.run(N)
    bd.check_compare(sim, w["cols"], be.outcomes(w), N, be.outcomes(other), N, name + ", the kept list against another seed")
    bd.same_cases(sim, be.outcomes(w), name + ", the kept list after the second run")
    bg.check_untouched(sim, other)
    sim.close()


# ---- d. six cases at pipeline level 0 on the permuted world ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", edges.SECOND_FORM)
def test_sequential_steps_on_the_permuted_world(name):
    w = be.world("edge_e", name, True)
    sim = started(w, level=0)
    check_everything(sim, w, name + ", permuted, level 0")
    bg.check_untouched(sim, w)
    sim.close()


# ---- e. grids capped to one and three workgroups --------------------------------------------------------------------------------------
def note_launches(sim, seen):
    for site, r in sim.debug_launches().items():
        m = re.fullmatch(r"(esim_host_burden\.h|esim_host_beds\.h):(\d+)", site)
        if m and r["clipped"]:
            key = (m.group(1), int(m.group(2)))
            seen[key] = max(seen.get(key, 0), r["max_trips"])


@pytest.mark.parametrize("cap", (1, 3))
def test_table_sets_with_grids_capped_and_every_launch_site_clipped(cap, monkeypatch):
    monkeypatch.setenv("ESIM_GRID_CAP", str(cap))
    seen = {}
    for name in CAPPED_SETS:
        sim, w = table_set(name, "%s, cap %d" % (name, cap))
        if name == "one_group_65":
            check_rows(sim, w, "group", "%s, cap %d" % (name, cap))
        note_launches(sim, seen)
        sim.close()
    assert int(be.outcomes(be.world("bins_64"))["admitted"].sum()) > 3 * 256          # the lists' consumers are clipped as well
    for file, sites, n_sites in (("esim_host_burden.h", bg.burden_sites(), 3), ("esim_host_beds.h", bd.beds_sites(), 5)):
        assert len(sites) == n_sites
        for first, last in sites:
            trips = max((t for (f, line), t in seen.items() if f == file and first <= line <= last), default=0)
            assert trips >= (3 if cap == 1 else 2), "%s:%d under ESIM_GRID_CAP=%d: clipped with %d trips" % (file, first, cap, trips)


@pytest.mark.parametrize("name", edges.SECOND_FORM)
@pytest.mark.parametrize("cap", (1, 3))
def test_second_form_cases_with_grids_capped(cap, name, monkeypatch):
    monkeypatch.setenv("ESIM_GRID_CAP", str(cap))
    w = be.world("edge_e", name)
    sim = started(w)
    check_everything(sim, w, "%s, cap %d" % (name, cap))
    seen = {}
    note_launches(sim, seen)
    sim.close()
    assert len(seen) >= 6 and max(seen.values()) >= (3 if cap == 1 else 2), seen


# ---- f. what esim_burden_set refuses at the same edges: the tables in force and a kept list stay ---------------------------------------
def test_refusals_at_the_limits_leave_the_tables_and_the_kept_list_alone():
    w = be.world("bins_64")
    o, t = be.outcomes(w), w["tables"]
    sim = started(w)
    sim.keep_burden_baseline()
    one_down = np.array([7, 9, 8], np.uint32)                                            # a CDF that descends by one
    refused = (dict(delay_cdf=np.arange(65)), dict(stay_cdf=np.arange(65)), dict(delay_unit=0), dict(stay_unit=0), dict(delay_unit=65536), dict(stay_unit=65536),
               dict(admit_thr=np.zeros(1025, np.uint32), death_thr=np.zeros(1025, np.uint32)), dict(delay_cdf=one_down), dict(stay_cdf=one_down))
    for bad in refused:
        p, arrays = bg.params_of(t, **dict(bad))
        assert sim.lib.esim_burden_set(sim._ctx, C.byref(p)) == EINVAL, sorted(bad)
        got = sim.burden()
        for k in ("admit_thr", "death_thr", "delay_cdf", "stay_cdf"):
            same(got[k], t[k], "the tables in force after a refusal: %s" % k)
        assert (got["delay_unit"], got["stay_unit"]) == (1, 1)
    bd.same_cases(sim, o, "the kept list after the refusals")
    assert sim.burden_baseline_info()["steps"] == N
    check_run(sim, w, "after the refusals")
    assert not sim.burden_compare("home")["bed_steps_averted"].any()
    # the limits themselves are taken, and drop the list with the tables they replace
    p, arrays = bg.params_of(be.SETS["bins_64_unit_max"][0])
    assert sim.lib.esim_burden_set(sim._ctx, C.byref(p)) == 0
    with pytest.raises(_lib.EsimError):
        sim.burden_baseline_info()
    sim.close()


# ---- g. the seam at its exact step -----------------------------------------------------------------------------------------------------
def test_the_seam_of_a_rollback_at_its_exact_step():
    """Cases with their onset on the snapshot's step draw under the snapshot's seed, those of the next step under the new one.  The
    onsets come from the device's exposure log (no programme: they follow from it alone): this pins the seam rule, not the onsets."""
    s = be.seam()
    old, new = be.SEAM_SEEDS
    sim = Simulator(s.pop, setting.copy_params(s.ep))
    sim.set_groups(s.labels, s.n_groups)
    sim.set_burden(s.tables)
    first_leg = sim.run(s.step)
    same(first_leg["exposures_building"], s.run["records"]["exposures_building"][:s.step], "the first leg vs the oracle")
    sim.snapshot()
    sim.run(be.SEAM_RUN_ON)
    sim.rollback(seed=new)
    sim.run(N - s.step)
    assert sim._steps == N and sim.snapshot_step() == s.step and not sim.records_so_far()["vaccination_active"].any()
    cit, step, _ = sim.exposure_events()
    onset = np.full(s.pop.n_citizens, NEVER, np.int64)
    onset[cit] = step.astype(np.int64) + int(s.ep.exposed_time) + 1
    onset[np.unique(s.pop.seeds)] = 0
    onset[onset > N] = NEVER
    same(np.where(onset <= s.step + 1, onset, NEVER), np.where(s.run["onset"] <= s.step + 1, s.run["onset"], NEVER), "the onsets the first leg decides")
    assert ((onset == s.step).sum(), (onset == s.step + 1).sum()) == s.at and ((onset > s.step + 1) & (onset != NEVER)).sum() > 30
    full = be.seam_outcomes(s, onset)
    assert be.differs(be.seam_outcomes(s, onset, strict=True), full)
    cols = {where: ref._curve_ref.labels_for(s.pop, where, (s.labels, s.n_groups)) for where in WHERES}
    first, last = max(1, s.step - 30), min(N, s.step + 30)
    bg.check_world(sim, cols, full, N, "the seam at step %d" % s.step, series=be.SERIES, summaries=[(1, N, 1), (1, N, 10), (first, last, 1), (first, last, 10)])
    sim.keep_burden_baseline()
    bd.same_cases(sim, full, "a list kept after the rollback")
    bd.check_compare(sim, cols, full, N, full, N, "the list kept after the rollback against the run", spans=((1, N), (s.step, s.step + 1)), series=be.SERIES)
    sim.close()
