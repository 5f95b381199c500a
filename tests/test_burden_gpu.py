"""Hospital burden on the device -- esim_burden_outcomes, esim_burden_series, esim_burden_summary and the peaks kind of the ensemble
accumulators over the bed occupancy -- against tests/_burden_ref.py: numpy over the onsets the CPU oracle shows and the oracle
library's Philox block.  Every comparison is exact equality of whole integer arrays."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _area_ref
import _area_status_ref
import _burden_ref as ref
import _curve_ref
from epidemicsimulator_amd import Ensemble, Population, Simulator, _lib
from epidemicsimulator_amd.ensemble import PEAKS_ARRAYS, peaks_summary

pytestmark = pytest.mark.gpu

FIELDS = [f for f in _lib.RECORD_FIELDS if f != "reserved"]
NEVER, WHERES, WHATS, KEYS = ref.NEVER, ref.WHERES, ref.WHATS, ref.KEYS
EINVAL, ESTATE, ERANGE = -1, -4, -5
T = ref.table_set_t()
u32p, u64p, u8p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint8)
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "epidemicsimulator_amd", "csrc")


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, "%s: %s %s, expected %s %s" % (what, got.dtype, got.shape, want.dtype, want.shape)
    if not (got == want).all():
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d entries differ, first at %s: got %d, expected %d"
                             % (what, len(bad), bad[0].tolist(), int(got[tuple(bad[0])]), int(want[tuple(bad[0])])))


def same_summary(got, want, what):
    assert sorted(got) == sorted(KEYS), what
    for k in KEYS:
        same(got[k], want[k], "%s: %s" % (what, k))


def same_outcomes(sim, o, what):
    got = sim.burden_outcomes()
    same(got["admit_step"], o["admit_step"].astype(np.uint32), what + ": admit_step")
    same(got["end_step"], o["end_step"].astype(np.uint32), what + ": end_step")
    same(got["died"], o["died"], what + ": died")


def windows(t):
    """(first_step, n_rows, stride) of the series calls after t steps: every step, every day, and a window that starts inside the run."""
    out = [(1, None, 1)]
    if t >= 48:
        out += [(1, None, 24), (t // 3, None, 24), (t // 2, min(40, t - t // 2 + 1), 1)]
    return out


def check_world(sim, cols, o, t, note, series=None, summaries=None):
    """Everything the library gives after t steps against the outcomes `o` of the reference.  series: the (first_step, n_rows,
    stride) of the series calls instead of windows(t); summaries: the (first_step, last_step, threshold) of the summary calls."""
    same_outcomes(sim, o, note)
    for where in WHERES:
        lab, n_cols = cols[where]
        for what in WHATS:
            for first, n_rows, stride in (windows(t) if series is None else series):
                same(sim.burden_series(what, where, first, n_rows, stride), ref.series(o, what, lab, n_cols, t, first, n_rows, stride),
                     "%s: %s by %s from step %d, stride %d" % (note, what, where, first, stride))
        spans = summaries if summaries is not None else [(1, t, 1), (1, t, 10)] + ([(t // 3, t - 7, 10), (t // 2, t // 2, 1)] if t >= 48 else [])
        for first, last, threshold in spans:
            same_summary(sim.burden_summary(where, first, last, threshold), ref.summary(o, lab, n_cols, t, first, last, threshold),
                         "%s: summary by %s, steps %d..%d, threshold %d" % (note, where, first, last, threshold))


def check_stops(world, stops, note, tables=T, **windows_of_check_world):
    sim = Simulator(world["pop"], world["ep"])
    sim.set_groups(world["labels"], world["n_groups"])
    sim.set_burden(tables)
    done = 0
    for s in stops:
        sim.run(s - done)
        done = s
        check_world(sim, world["cols"], ref.at_stop(world["full"], s), s, "%s, %d steps run" % (note, s), **windows_of_check_world)
    return sim


def check_untouched(sim, world):
    got = sim.records_so_far()
    for f in FIELDS:
        same(got[f], world["run"]["records"][f][:len(got)], "record field %s" % f)
    state = sim.download_state()
    for k in ("status", "timer", "current_building", "on_bus", "eligible"):
        same(state[k], world["run"]["final_state"][k], "final state %s" % k)


# ---- both worlds at every stop; the calls leave the run alone ---------------------------------------------------------------------
@pytest.mark.parametrize("name", ("fixture_a", "w2"))
def test_outcomes_series_and_summary_at_every_stop_and_the_calls_leave_the_run_alone(name):
    world, stops = (ref.fixture_a(), ref.FIXTURE_A_STOPS) if name == "fixture_a" else (ref.world_w2(), ref.W2_STOPS)
    sim = check_stops(world, stops, name)
    check_untouched(sim, world)
    if name == "fixture_a":
        # at the stops 96 and 300 ends (and at 300 admissions) lie beyond the run: they are in the outcomes and in no row
        o = ref.at_stop(world["full"], 700)
        inside = o["admitted"] & (o["admit_step"] >= 1) & (o["admit_step"] <= 700)
        assert int(sim.burden_series("admissions").sum()) == int(inside.sum()) <= 152
        assert (sim.burden_summary("group")["peak"] == 0).sum() == 2                     # two age bands without an admission
    else:
        # a vaccination while Infected leaves the outcome standing; one while Exposed makes no case
        o, run = ref.at_stop(world["full"], 900), world["run"]
        got = sim.burden_outcomes()
        assert int(((got["admit_step"] != NEVER) & run["vax_infected"]).sum()) == 64 and not ((got["admit_step"] != NEVER) & run["vax_exposed"]).any()
        assert int(o["admitted"].sum()) == 475
    sim.close()


# ---- more columns than the LDS table of k_burden_events holds ------------------------------------------------------------------------
def areas100():
    """100 Output Areas of 30 citizens: by home area the admissions and deaths are counted in global memory, a wavefront at a time."""
    if "areas100" not in _cache:
        pop = Population.synthetic("york", n_citizens=3000, n_areas=100, citizens_per_school=1500, n_seeds=10)
        ep = _lib.default_params(exposure_chance=0.05, lockdown_threshold=2.0, mask_pt_threshold=2.0, mask_everywhere_threshold=2.0,
                                 vaccination_threshold=0.05, vaccination_rate=2, seed=11, max_steps=600)
        labels, n_groups = pop.age_bands(ref._group_ref.AGE_EDGES)
        world = ref.build(pop, ep, labels, n_groups, 600)
        o = ref.at_stop(world["full"], 600)
        assert pop.n_areas > 64 and int(o["admitted"].sum()) >= 50 and int(o["died"].sum()) >= 10                    # (65 and 17)
        assert len(np.unique(world["cols"]["home"][0][o["admitted"]])) >= 20 and world["run"]["vax_infected"].any()   # admissions in 34 areas
        _cache["areas100"] = world
    return _cache["areas100"]


_cache = {}


def test_more_columns_than_the_lds_table_of_the_events_kernel():
    world = areas100()
    sim = check_stops(world, (300, 600), "100 areas")
    check_untouched(sim, world)
    sim.close()


# ---- the summary against the library's own rows -----------------------------------------------------------------------------------
def test_summary_against_the_stride_1_rows_of_the_library():
    world = ref.world_w2()
    sim = check_stops(world, (ref.W2_STEPS,), "w2")
    for where in WHERES:
        for first, last, threshold in ((1, 900, 1), (300, 650, 10)):
            occ = sim.burden_series("occupancy", where, first, last - first + 1).astype(np.int64)
            want = _curve_ref.summarize(occ, 1, occ.shape[0], threshold)
            for k in ("peak_step", "first_at_least", "last_at_least"):                # (rows count from first_step)
                want[k] = np.where(want[k] != NEVER, want[k].astype(np.int64) + first - 1, NEVER).astype(np.uint32)
            got = sim.burden_summary(where, first, last, threshold)
            for k in KEYS[:5]:
                same(got[k], want[k], "%s by %s, steps %d..%d vs the rows" % (k, where, first, last))
            same(got["bed_steps"], want["person_steps"], "bed_steps by %s" % where)
            for what in ("admissions", "deaths"):
                same(got[what], sim.burden_series(what, where, first, last - first + 1).sum(axis=0, dtype=np.uint32), "%s by %s vs the rows" % (what, where))
    sim.close()


# ---- identity: everybody admitted at onset for the Infected interval is the Infected curve ---------------------------------------
def test_identity_with_the_infected_curve_on_fixture_a():
    world = ref.fixture_a()
    pop, ep = world["pop"], world["ep"]
    tables = dict(admit_thr=np.array([0xFFFFFFFF], np.uint32), death_thr=np.array([0], np.uint32), delay_cdf=np.zeros(0, np.uint32),
                  stay_cdf=np.zeros(0, np.uint32), delay_unit=1, stay_unit=int(ep.infected_time) + 1)
    assert not (world["full"]["block"][world["full"]["case"], 0] == 0xFFFFFFFF).any() and not world["run"]["vax_infected"].any()
    sim = Simulator(pop, ep)
    sim.set_groups(world["labels"], world["n_groups"])
    sim.set_burden(tables)
    sim.run(700)
    for where in WHERES:
        for first, last, threshold in ((1, 700, 1), (250, 600, 5)):
            b, c = sim.burden_summary(where, first, last, threshold), sim.curve_summary(where, "infected", first, last, threshold)
            for k in KEYS[:5]:
                same(b[k], c[k], "identity by %s, steps %d..%d: %s" % (where, first, last, k))
            same(b["bed_steps"], c["person_steps"], "identity by %s: bed_steps" % where)
            assert not b["deaths"].any()
    assert int(sim.burden_summary("all")["peak"][0]) == int(world["run"]["records"]["infected"].max())
    sim.close()


# ---- all thresholds 0 ---------------------------------------------------------------------------------------------------------------
def test_all_thresholds_zero():
    world = ref.world_w2()
    sim = Simulator(world["pop"], world["ep"])
    sim.set_groups(world["labels"], world["n_groups"])
    sim.set_burden(dict(T, admit_thr=np.zeros(8, np.uint32), death_thr=np.zeros(8, np.uint32)))
    sim.run(500)
    got = sim.burden_outcomes()
    assert (got["admit_step"] == NEVER).all() and (got["end_step"] == NEVER).all() and not got["died"].any()
    for where in WHERES:
        for what in WHATS:
            assert not sim.burden_series(what, where).any(), (what, where)
        s = sim.burden_summary(where, 1, 500, 1)
        for k in ("peak", "steps_at_least", "bed_steps", "admissions", "deaths"):
            assert not s[k].any(), (where, k)
        for k in ("peak_step", "first_at_least", "last_at_least"):
            assert (s[k] == NEVER).all(), (where, k)
    sim.close()


# ---- citizens that are not home-sorted ----------------------------------------------------------------------------------------------
def test_population_that_is_not_home_sorted():
    pop, ep = _area_ref.fixture_a()
    per = _area_ref.permuted(pop)
    labels, n_groups = per.age_bands(ref._group_ref.AGE_EDGES)
    world = ref.build(per, ep, labels, n_groups, 500)
    assert (np.diff(_area_status_ref.home_area_labels(per).astype(np.int64)) < 0).any() and int(ref.at_stop(world["full"], 500)["admitted"].sum()) >= 20
    sim = check_stops(world, (500,), "permuted")
    check_untouched(sim, world)
    sim.close()


# ---- a branch after a rollback under another seed: the seam rule ------------------------------------------------------------------
def test_branch_after_rollback_under_another_seed():
    """No vaccination programme, so that the onsets follow from the exposure log alone: the snapshot's seed draws the cases with an
    onset up to the snapshot's step, the new seed the later ones."""
    pop, _, labels, n_groups = ref.w2()
    ep = _lib.default_params(exposure_chance=0.02, lockdown_threshold=2.0, mask_pt_threshold=2.0, mask_everywhere_threshold=2.0,
                             vaccination_threshold=2.0, seed=321, max_steps=600)
    sim = Simulator(pop, ep)
    sim.set_groups(labels, n_groups)
    sim.set_burden(T)
    sim.run(250)
    sim.snapshot()
    sim.run(60)
    sim.rollback(seed=99)
    sim.run(350)
    assert sim._steps == 600 and not sim.records_so_far()["vaccination_active"].any()
    cit, step, _ = sim.exposure_events()
    onset = np.full(pop.n_citizens, NEVER, np.int64)
    onset[cit] = step.astype(np.int64) + int(ep.exposed_time) + 1
    onset[np.unique(pop.seeds)] = 0
    onset[onset > 600] = NEVER
    assert ((onset <= 250).sum() > 30) and ((onset > 250) & (onset != NEVER)).sum() > 30
    full = ref.outcomes(onset, labels, T, lambda s: 321 if s <= 250 else 99, pop.citizen_id_base)
    for wrong in (lambda s: 321, lambda s: 99):
        assert (ref.outcomes(onset, labels, T, wrong)["admitted"] != full["admitted"]).any()
    cols = {where: _curve_ref.labels_for(pop, where, (labels, n_groups)) for where in WHERES}
    check_world(sim, cols, full, 600, "branch")
    sim.close()


# ---- esim_restart keeps the tables, an upload and a drop do not -------------------------------------------------------------------
def test_restart_keeps_the_tables_and_what_drops_them():
    world = ref.world_w2()
    pop, ep, labels, n_groups = world["pop"], world["ep"], world["labels"], world["n_groups"]
    sim = Simulator(pop, ep)
    sim.set_groups(labels, n_groups)
    sim.set_burden(T)
    got = sim.burden()
    for k in ("admit_thr", "death_thr", "delay_cdf", "stay_cdf"):
        same(got[k], T[k], "the tables in force: %s" % k)
    assert (got["delay_unit"], got["stay_unit"]) == (24, 24)
    sim.run(100)
    sim.restart(seed=7)
    sim.restart(seed=int(ep.seed))
    sim.run(402)
    check_world(sim, world["cols"], ref.at_stop(world["full"], 402), 402, "after esim_restart")
    sim.set_groups(labels, n_groups)                                         # the same count: kept
    assert sim.burden()["admit_thr"].size == 8
    sim.set_groups(labels % 4, 4)                                            # another count: dropped
    with pytest.raises(_lib.EsimError) as e:
        sim.burden()
    assert e.value.code == ESTATE
    sim.set_burden(dict(T, admit_thr=T["admit_thr"][:1], death_thr=T["death_thr"][:1]))   # one group needs no labels and survives any
    sim.set_groups(None)
    assert sim.burden()["admit_thr"].size == 1 and sim.burden_summary("all")["admissions"][0] > 0
    sim.drop_burden()
    with pytest.raises(_lib.EsimError):
        sim.burden_summary("all")
    sim.close()


# ---- the peaks kind over four seeds -------------------------------------------------------------------------------------------------
def w2_of_seed(seed):
    pop, ep, labels, n_groups = ref.w2()
    ep.seed = seed
    return ref.build(pop, ep, labels, n_groups, 600)


def test_peaks_kind_over_four_seeds_and_the_median_of_the_peak():
    seeds = (321, 5, 6, 7)
    worlds = [w2_of_seed(s) for s in seeds]
    pop, labels, n_groups = worlds[0]["pop"], worlds[0]["labels"], worlds[0]["n_groups"]
    spec = dict(where="group", first_step=50, last_step=600, threshold=10)
    lab, n_cols = worlds[0]["cols"]["group"]
    want_each = []
    for w in worlds:
        s = ref.summary(ref.at_stop(w["full"], 600), lab, n_cols, 600, 50, 600, 10)
        want_each.append(dict(s, person_steps=s["bed_steps"]))
    assert any((a["peak"] != b["peak"]).any() for a, b in zip(want_each, want_each[1:]))
    sim = Simulator(pop, worlds[0]["ep"])
    sim.set_groups(labels, n_groups)
    sim.set_burden(T)
    sim.ensemble_begin_burden_peaks(min_peak=20, **spec)
    sim.ensemble_keep_members(4, "value")
    for seed, want in zip(seeds, want_each):
        sim.restart(seed=seed)
        sim.run(600)
        sim.ensemble_fold()
        same_summary(sim.burden_summary(**spec), {k: want[k] for k in KEYS}, "member of seed %d" % seed)
    got, want = sim.ensemble_read_peaks(), _curve_ref.fold(want_each, 20)
    assert got["members"] == 4 and want["hit"].any() and (want["hit"] < 4).any()
    for k in _curve_ref.PEAKS_KEYS:
        same(got[k], want[k], "accumulator %s" % k)
    peaks = np.sort(np.stack([w["peak"] for w in want_each]), axis=0)
    same(sim.ensemble_quantiles((0.5,))[0, 0], peaks[1], "the median of the peak (inverted CDF: the second smallest of four)")
    same(sim.ensemble_exceedance((20,))[0, 0], (peaks >= 20).sum(axis=0).astype(np.uint32), "members with a peak of 20 beds or more")
    # a status-curve begin replaces the kind; the fold then summarises the status again
    sim.ensemble_begin_peaks("group", "infected", 50, 600, 10, 20)
    sim.ensemble_fold()
    same(sim.ensemble_read_peaks()["sum_peak"], sim.curve_summary("group", "infected", 50, 600, 10)["peak"].astype(np.uint64), "the status kind after the burden kind")
    # without tables the fold of the burden kind is refused
    sim.ensemble_begin_burden_peaks(min_peak=20, **spec)
    sim.drop_burden()
    assert sim.lib.esim_ensemble_fold(sim._ctx) == ESTATE and sim.ensemble_read_peaks()["members"] == 0
    sim.close()


def test_ensemble_run_with_the_burden_peaks_kind_and_its_dump(tmp_path):
    seeds = (321, 5)
    worlds = [w2_of_seed(s) for s in seeds]
    pop, ep, labels, n_groups = worlds[0]["pop"], worlds[0]["ep"], worlds[0]["labels"], worlds[0]["n_groups"]
    lab, n_cols = worlds[0]["cols"]["group"]
    ens = Ensemble(pop, ep, group=(labels, n_groups), burden=T)
    area = dict(kind="burden_peaks", where="group", threshold=10, min_peak=20, quantiles=(0.5,), exceed=(20,))
    res = ens.run([dict(seed=s) for s in seeds], 600, area=area)
    singles = []
    for w in worlds:
        s = ref.summary(ref.at_stop(w["full"], 600), lab, n_cols, 600, 1, 600, 10)
        singles.append(dict(s, person_steps=s["bed_steps"]))
    want = peaks_summary(_curve_ref.fold(singles, 20))
    a = res.area
    assert res.area_kind == "burden_peaks" and a["members"] == 2 and a["defined"].shape == (n_groups,)
    for k in PEAKS_ARRAYS:
        assert np.array_equal(a[k], want[k], equal_nan=True), k
    same(a["quantiles"][0], np.minimum(singles[0]["peak"], singles[1]["peak"]), "the lower of two peaks")
    same(a["exceed"][0], sum((s["peak"] >= 20).astype(np.uint32) for s in singles), "members at 20 beds or more")
    with pytest.raises(ValueError):
        ens.run([dict(seed=1)], 50, stop_when_done=True, area=area)
    res.dump(str(tmp_path))
    saved = np.load(str(tmp_path / "ensemble_area_burden.npz"))
    assert int(saved["members"]) == 2 and (saved["peak_mean"] == a["peak_mean"]).all() and (saved["p_peak"] == a["p_peak"]).all()
    assert not os.path.exists(str(tmp_path / "ensemble_area_peaks.npz"))
    ens.simulator.close()


# ---- grids capped to one and three workgroups --------------------------------------------------------------------------------------
def burden_sites():
    """[(first line, last line)] of every grid_capped call of esim_host_burden.h (the compiler reports the line where a launch
    macro's call ends)."""
    lines = open(os.path.join(CSRC, "esim_host_burden.h")).read().split("\n")
    out = []
    for no, line in enumerate(lines, 1):
        if re.search(r"\bgrid_capped\(", line) and not line.lstrip().startswith("//"):
            last = no
            while not lines[last - 1].split("//")[0].rstrip().endswith(";"):
                last += 1
            out.append((no, last))
    return out


@pytest.mark.parametrize("cap", (1, 3))
def test_grids_capped_to_one_and_three_workgroups(cap, monkeypatch):
    monkeypatch.setenv("ESIM_GRID_CAP", str(cap))
    seen = {}
    for world, stops, note in ((ref.fixture_a(), ref.FIXTURE_A_STOPS, "fixture A"), (ref.world_w2(), ref.W2_STOPS, "w2"), (areas100(), (600,), "100 areas")):
        sim = check_stops(world, stops, "%s, cap %d" % (note, cap))
        for site, r in sim.debug_launches().items():
            m = re.fullmatch(r"esim_host_burden\.h:(\d+)", site)
            if m and r["clipped"]:
                seen[int(m.group(1))] = max(seen.get(int(m.group(1)), 0), r["max_trips"])
        sim.close()
    sites = burden_sites()
    assert len(sites) == 3
    for first, last in sites:
        trips = max((t for line, t in seen.items() if first <= line <= last), default=0)
        assert trips >= (3 if cap == 1 else 2), "esim_host_burden.h:%d under ESIM_GRID_CAP=%d: clipped with %d trips" % (first, cap, trips)


# ---- errors -------------------------------------------------------------------------------------------------------------------------
def params_of(tables, **over):
    """(esim_burden_params, the arrays it points into) with fields overridden after the fact."""
    arr = {k: np.ascontiguousarray(tables[k], np.uint32) for k in ("admit_thr", "death_thr", "delay_cdf", "stay_cdf")}
    for k in arr:
        if over.get(k) is not None:
            arr[k] = np.ascontiguousarray(over.pop(k), np.uint32)
    p = _lib.BurdenParams(arr["admit_thr"].size, arr["admit_thr"].ctypes.data_as(u32p), arr["death_thr"].ctypes.data_as(u32p), tables["delay_unit"],
                          arr["delay_cdf"].size, arr["delay_cdf"].ctypes.data_as(u32p), tables["stay_unit"], arr["stay_cdf"].size, arr["stay_cdf"].ctypes.data_as(u32p))
    for k, v in over.items():                    # (None: a null pointer)
        setattr(p, k, v)
    return p, arr


def outputs(n_cols, n_citizens, fill=12345):
    out = {k: np.full(n_cols, fill, np.uint64 if k == "bed_steps" else np.uint32) for k in KEYS}
    out["rows"] = np.full((4, n_cols), fill, np.uint32)
    out["admit"], out["end"], out["died"] = np.full(n_citizens, fill, np.uint32), np.full(n_citizens, fill, np.uint32), np.full(n_citizens, 77, np.uint8)
    return out


def calls(lib, ctx, out, where, first=1, last=10, n_rows=4):
    """The return codes of the three computing calls and the begin, with `out` as their outputs."""
    ptrs = [out[k].ctypes.data_as(u64p if k == "bed_steps" else u32p) for k in KEYS]
    return (lib.esim_burden_summary(ctx, where, first, last, 1, *ptrs),
            lib.esim_burden_series(ctx, where, _lib.BURDEN_OCCUPANCY, first, n_rows, 1, out["rows"].ctypes.data_as(u32p)),
            lib.esim_burden_outcomes(ctx, out["admit"].ctypes.data_as(u32p), out["end"].ctypes.data_as(u32p), out["died"].ctypes.data_as(u8p)),
            lib.esim_ensemble_begin_burden_peaks(ctx, where, first, last, 1, 1))


def untouched(out, fill=12345):
    return all((v == (77 if k == "died" else fill)).all() for k, v in out.items())


def test_error_table():
    world = ref.world_w2()
    pop, ep, labels, n_groups = world["pop"], world["ep"], world["labels"], world["n_groups"]
    lib = _lib.load()
    ALL, HOME, GROUP = _lib.BY_ALL, _lib.AREA_HOME, _lib.BY_GROUP
    out = outputs(pop.n_areas, pop.n_citizens)
    good, keep = params_of(T)
    bare = C.c_void_p()
    _lib.check(lib.esim_create(C.byref(ep), C.byref(bare)))
    assert lib.esim_burden_set(bare, C.byref(good)) == ESTATE and calls(lib, bare, out, HOME) == (ESTATE,) * 4      # before an upload
    lib.esim_destroy(bare)
    assert lib.esim_burden_set(None, C.byref(good)) == EINVAL and calls(lib, None, out, HOME) == (EINVAL,) * 4       # null context
    sim = Simulator(pop, ep)
    sim.run(10)
    ctx = sim._ctx
    assert calls(lib, ctx, out, HOME) == (ESTATE,) * 4 and b"esim_burden_set" in lib.esim_last_error(ctx)            # no tables set
    assert lib.esim_burden_get(ctx, *([None] * 9)) == ESTATE
    assert lib.esim_burden_set(ctx, C.byref(good)) == ESTATE                                                          # eight groups, labels missing
    sim.set_groups(labels % 4, 4)
    assert lib.esim_burden_set(ctx, C.byref(good)) == ESTATE                                                          # ... a group count that differs
    sim.set_groups(labels, n_groups)
    for bad in (dict(delay_cdf=np.arange(65)), dict(stay_cdf=np.arange(65)), dict(delay_cdf=T["delay_cdf"][::-1]), dict(stay_cdf=[5, 4]), dict(delay_unit=0),
                dict(delay_unit=65536), dict(stay_unit=0), dict(stay_unit=65536), dict(n_groups=0), dict(n_groups=1025), dict(admit_thr=None)):
        p, arrays = params_of(T, **bad)
        assert lib.esim_burden_set(ctx, C.byref(p)) == EINVAL, bad
    assert lib.esim_burden_set(ctx, None) == EINVAL and calls(lib, ctx, out, HOME) == (ESTATE,) * 4                  # the refusals set nothing
    p, arrays = params_of(T, delay_cdf=np.arange(64), stay_cdf=np.full(64, 7), delay_unit=65535, stay_unit=65535)     # the limits themselves are taken
    assert lib.esim_burden_set(ctx, C.byref(p)) == 0
    assert lib.esim_burden_set(ctx, C.byref(good)) == 0
    for where in (_lib.AREA_CURRENT, _lib.BY_SETTING, 5, -1):
        got = calls(lib, ctx, out, where)
        assert got[0] == got[1] == got[3] == EINVAL, where                                                            # by the area stood in, and anything else
    ptrs = [out[k].ctypes.data_as(u64p if k == "bed_steps" else u32p) for k in KEYS]
    rows = out["rows"].ctypes.data_as(u32p)
    assert lib.esim_burden_summary(ctx, HOME, 1, 10, 0, *ptrs) == EINVAL                                              # threshold 0
    assert lib.esim_ensemble_begin_burden_peaks(ctx, HOME, 1, 10, 1, 0) == EINVAL                                     # min_peak 0
    for what, n_rows, stride, ptr in ((3, 4, 1, rows), (-1, 4, 1, rows), (1, 0, 1, rows), (1, 4, 0, rows), (1, 4, 1, None)):
        assert lib.esim_burden_series(ctx, HOME, what, 1, n_rows, stride, ptr) == EINVAL
    assert lib.esim_burden_summary(ctx, HOME, 0, 10, 1, *ptrs) == ERANGE and lib.esim_burden_series(ctx, HOME, 1, 0, 4, 1, rows) == ERANGE   # first_step 0
    assert lib.esim_burden_summary(ctx, HOME, 5, 4, 1, *ptrs) == ERANGE                                               # last_step < first_step
    assert lib.esim_burden_summary(ctx, ALL, 1, 11, 1, *ptrs) == ERANGE and lib.esim_burden_series(ctx, HOME, 1, 8, 4, 1, rows) == ERANGE    # beyond the steps run
    assert lib.esim_ensemble_begin_burden_peaks(ctx, HOME, 0, 10, 1, 1) == ERANGE
    out["admit"][:] = 12345; out["end"][:] = 12345; out["died"][:] = 77                                               # (the outcomes call above succeeded)
    assert untouched(out)
    sim.set_groups(None)                                                                                              # the labels gone: the tables with them
    assert calls(lib, ctx, out, ALL) == (ESTATE,) * 4 and untouched(out)
    sim.set_groups(labels, n_groups)
    sim.set_burden(T)
    sim.run(890)                                                                                                      # the context is usable afterwards
    check_world(sim, world["cols"], ref.at_stop(world["full"], 900), 900, "after the refusals")
    assert lib.esim_burden_summary(ctx, GROUP, 1, 900, 1, *([None] * 8)) == 0                                         # every output NULL: the call still runs
    assert lib.esim_burden_outcomes(ctx, None, None, None) == 0
    sim.close()


def test_a_shard_and_a_communicator_of_two_ranks_are_refused():
    lib = _lib.load()
    whole = Population.synthetic("york", n_citizens=20000, n_areas=64, citizens_per_school=2500, n_seeds=20)
    cuts = whole.even_cuts(2)
    s0, s1 = whole.shard(cuts, 0), whole.shard(cuts, 1)
    out = outputs(whole.n_areas, whole.n_citizens, 4242)
    ep = _lib.default_params(exposure_chance=0.004, seed=123)
    one, keep_arrays = params_of(dict(T, admit_thr=T["admit_thr"][-1:], death_thr=T["death_thr"][-1:]))

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
    assert lib.esim_burden_set(sim._ctx, C.byref(one)) == ESTATE and b"shard" in lib.esim_last_error(sim._ctx)       # a shard without a communicator
    assert calls(lib, sim._ctx, out, _lib.BY_ALL, 1, 1, 1) == (ESTATE,) * 4 and untouched(out, 4242)
    keep = communicator(sim, [s0.n_citizens, s1.n_citizens, whole.n_citizens, s1.n_shared_buildings, s1.n_shared_rooms])
    assert lib.esim_burden_set(sim._ctx, C.byref(one)) == ESTATE and b"ranks" in lib.esim_last_error(sim._ctx)       # ... and with one of two ranks
    assert calls(lib, sim._ctx, out, _lib.BY_ALL, 1, 1, 1) == (ESTATE,) * 4 and untouched(out, 4242)
    sim.close()
    sim = Simulator(whole, ep)
    sim.run(120)
    assert lib.esim_burden_set(sim._ctx, C.byref(one)) == 0
    sim.ensemble_begin_burden_peaks("home", 1, 120, 1, 1)
    sim.ensemble_fold()
    before = sim.ensemble_read_peaks()
    assert before["members"] == 1 and before["defined"].any()
    keep = communicator(sim, [whole.n_citizens, 0, whole.n_citizens, 0, 0])                   # rank 1 holds nobody
    assert calls(lib, sim._ctx, out, _lib.AREA_HOME, 1, 120, 4) == (ESTATE,) * 4 and b"ranks" in lib.esim_last_error(sim._ctx) and untouched(out, 4242)
    assert lib.esim_ensemble_fold(sim._ctx) == ESTATE and b"ranks" in lib.esim_last_error(sim._ctx)   # the fold's own refusal: the kind is still in force
    after = sim.ensemble_read_peaks()
    assert after["members"] == 1
    for k in _curve_ref.PEAKS_KEYS:
        same(after[k], before[k], "accumulator %s after the refused fold" % k)
    del keep
    sim.close()
