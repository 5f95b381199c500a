"""The output kernels with their grids capped to one and to three workgroups (ESIM_GRID_CAP), so that the grid-stride loops make
their second and later trips on the small worlds that have a reference: a workgroup's LDS table stays live over trips, the last
wavefront of a trip is partial, the workgroups of one launch make different numbers of trips, a workgroup per entry reuses its
shared state.  Every comparison is the exact one of the family's own GPU test module -- its checking helper, or, where the checks
of an ensemble kind are the body of a test, that test called as a function --, against the numpy and oracle references of
tests/_*_ref.py, with no tolerance.

The records of esim_debug_launches are read from every simulator as it is closed: after a family's calls they must show a
launch that the cap clipped and whose loop made at least three trips (cap 1) or two (cap 3), and over the module every launch
site of the host code must have been clipped with three trips or more (test_every_launch_site_was_clipped)."""
import os
import re

import numpy as np
import pytest

import _area_ref
import _area_status_ref
import _arrival_ref
import _chain_ref as chain
import _compare_ref as cr
import _curve_ref as curve
import _ens_transmission_ref as ens_ref
import _flow_ref as flow
import _group_ref
import _household_ref as hh
import _place_ref as pl
import _setting_ref as ref_mod
import _snapshot_ref as snap
import _tree_ref as tree
import test_area_flows_gpu as t_flows
import test_area_status_series_gpu as t_status
import test_contact_hours_gpu as t_contacts
import test_curve_summary_gpu as t_curves
import test_ensemble_series_gpu as t_ens_series
import test_ensemble_transmission_gpu as t_ens_trans
import test_exposure_settings_gpu as t_settings
import test_households_gpu as t_households
import test_place_outbreaks_gpu as t_places
import test_policy_compare_gpu as t_compare
import test_snapshot_gpu as t_snapshot
import test_transmission_chains_gpu as t_chains
import test_transmission_events_gpu as t_events
import test_transmission_tree_gpu as t_tree
from epidemicsimulator_amd import Population, Simulator, _lib
from test_parity_gpu import assert_same_records

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "epidemicsimulator_amd", "csrc")
CAPS = (1, 3)
MIN_TRIPS = {1: 3, 3: 2}                 # what a family must reach under the cap
NEVER = _lib.NEVER
STATUS = _area_status_ref.STATUS
SEEN = {}                                # site -> the most trips of a batch of calls in which the cap clipped it, over the module
TABLE = {}                               # (cap, site) -> [launches, clipped, max_trips] over the module (printed by the last test)

# The host code whose launch sites the last test wants clipped, and the macros the product build leaves undefined (a site in a
# branch that is not compiled cannot be reached).
SITE_FILES = ["esim_host_%s.h" % k for k in ("outputs", "settings", "tree", "household", "places", "contacts", "flows", "events", "curves", "compare",
                                             "ensrows", "snapshot", "upload")]
NOT_DEFINED = ()
# Sites that need not be clipped: only such whose item count is a constant independent of the population.  There is none.
ALLOWED_UNCLIPPED = {}


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, "%s: shape %s, expected %s" % (what, got.shape, want.shape)
    bad = np.flatnonzero(got.ravel() != want.ravel())
    assert bad.size == 0, "%s: %d of %d differ, first at %d: got %s, expected %s" % (what, bad.size, got.size, bad[0], got.ravel()[bad[0]], want.ravel()[bad[0]])


# ---- the cap, and the records of every simulator closed under it ----------------------------------------------------------------
@pytest.fixture(params=CAPS, ids=["cap%d" % c for c in CAPS])
def cap(request, monkeypatch):
    monkeypatch.setenv("ESIM_GRID_CAP", str(request.param))
    return request.param


@pytest.fixture
def launches(cap, monkeypatch):
    """{site: record} summed over the simulators closed during the test (each is read just before it is destroyed)."""
    got = {}
    close = Simulator.close

    def harvesting_close(self):
        if self._ctx:
            for site, r in self.debug_launches().items():
                g = got.setdefault(site, {"launches": 0, "clipped": 0, "max_trips": 0})
                g["launches"] += r["launches"]
                g["clipped"] += r["clipped"]
                g["max_trips"] = max(g["max_trips"], r["max_trips"])
        close(self)

    monkeypatch.setattr(Simulator, "close", harvesting_close)
    yield got


def bitten(launches, cap, family):
    """The cap did something to the family's calls; the records join the module's union."""
    assert launches, "%s: no launch was recorded under ESIM_GRID_CAP=%d" % (family, cap)
    sites = once("launch sites", launch_sites)
    for site, r in launches.items():
        assert re.fullmatch(r"esim_host_[a-z]+\.h:\d+", site), site
        site = canonical(site, sites)
        assert 1 <= r["launches"] and r["clipped"] <= r["launches"] and r["max_trips"] >= 1, (site, r)
        if r["clipped"]:
            SEEN[site] = max(SEEN.get(site, 0), r["max_trips"])
        t = TABLE.setdefault((cap, site), [0, 0, 0])
        t[0] += r["launches"]; t[1] += r["clipped"]; t[2] = max(t[2], r["max_trips"])
    best = max((r["max_trips"] for r in launches.values() if r["clipped"]), default=0)
    assert best >= MIN_TRIPS[cap], "%s under ESIM_GRID_CAP=%d: the longest loop of a clipped launch made %d trips, %d are asked for" % (family, cap, best, MIN_TRIPS[cap])


# ---- the worlds beside those of the reference modules ---------------------------------------------------------------------------
_cache = {}


def once(key, make):
    """make() computed once per session: the references this module needs beside those the reference modules cache."""
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def areas800():
    """800 Output Areas of ten citizens, no interventions: (pop, ep, n, tree reference, chains).  The kernels that run a lane per
    area -- k_flow_resolve, k_ensemble_fold_peaks --, the folds over rows of areas and the tables over 10 936 buildings make
    several trips here; 396 exposures reach 253 areas."""
    if "areas800" not in _cache:
        pop = Population.synthetic("york", n_citizens=8000, n_areas=800, citizens_per_school=4000, n_seeds=12, p_public_transport=0.4)
        ep = _lib.default_params(exposure_chance=0.03, lockdown_threshold=2.0, vaccination_threshold=2.0, mask_pt_threshold=2.0, mask_everywhere_threshold=2.0,
                                 max_steps=500)
        n = 400
        ref = tree.reference(pop, ep, n, ref_mod.reference(pop, ep, n))
        assert pop.n_areas >= 769 and pop.n_buildings > 8192
        assert int((ref["step"] > 0).sum()) >= 300 and int((flow.invasion(ref, pop)["step"] != NEVER).sum()) >= 200
        _cache["areas800"] = (pop, ep, n, ref, chain.chains(ref, pop))
    return _cache["areas800"]


def rooms():
    """714 rooms in four schools (two citizens in five teach, in offices of twelve): (pop, ep, n, tree reference, sus_until).
    k_place_schools runs a lane per room."""
    if "rooms" not in _cache:
        pop = Population.synthetic("york", n_citizens=20000, n_areas=64, citizens_per_school=5000, n_seeds=20, p_teaching=0.4)
        ep = _lib.default_params(exposure_chance=0.004, vaccination_threshold=0.01, lockdown_threshold=0.02, seed=123, max_steps=400)
        n = 300
        ref = tree.reference(pop, ep, n, ref_mod.reference(pop, ep, n))
        assert pop.n_rooms >= 513 and int((ref["setting"] == tree.S).sum()) >= 100
        _cache["rooms"] = (pop, ep, n, ref, hh.sus_until(pop, ep, n))
    return _cache["rooms"]


def run_of(pop, ep, n, groups=None):
    sim = Simulator(pop, ref_mod.copy_params(ep))
    if groups is not None:
        sim.set_groups(*groups)
    sim.run(n)
    return sim


def long_route_exposures(ref):
    """Logged bus exposures on a route longer than a bus: the entries k_tree_route and k_contact_route work on."""
    return int(((ref["setting"] == tree.T) & (ref["step"] > 0) & (ref["n_buses"] >= 2)).sum())


# ---- 1. the families --------------------------------------------------------------------------------------------------------------
def test_settings(cap, launches):
    sim, pop, n, ref = t_settings.started("fixture_a")
    t_settings.check_all(sim, pop, ref, n, "fixture A, cap %d" % cap, windows=(dict(first_step=200, n_rows=6, stride=24),))
    sim.close()
    pop, ep, n, ref, _ = areas800()
    sim = run_of(pop, ep, n, t_settings.labels_of(pop))
    t_settings.check_all(sim, pop, once("areas800 settings", lambda: ref_mod.reference(pop, ep, n)), n, "800 areas, cap %d" % cap)
    sim.close()
    bitten(launches, cap, "settings")


@pytest.mark.parametrize("name", ("fixture_a", "bus", "spread"))
def test_tree_offspring_reproduction_and_mixing(name, cap, launches):
    if name == "spread":
        # 14 119 entries in ten generation windows: the launches per window (k_tree_gen) make several trips
        pop, ep, n, ref, _ = flow.cached("spread")
        sim = run_of(pop, ep, n, t_tree.labels_of(pop))
    else:
        sim, pop, n, ref = t_tree.started(name)
    if name == "bus":
        assert long_route_exposures(ref) >= 8                        # k_tree_route takes several entries per workgroup
    t_tree.check_all(sim, pop, ref, n, "%s, cap %d" % (name, cap))
    sim.close()
    bitten(launches, cap, "tree")


def test_chains_outbreaks_and_ages(cap, launches):
    for name in ("fixture_a", "deep"):
        sim, pop, ep, n, ref, ch = t_chains.started(name)
        t_chains.check_all(sim, pop, ep, ref, ch, n, "%s, cap %d" % (name, cap))
        sim.close()
    pop, ep, n, ref, ch = flow.cached("spread")                      # more than 8192 entries: k_chain_ages' grid of 32 trips a lane is clipped
    sim = run_of(pop, ep, n)
    t_chains.check_all(sim, pop, ep, ref, ch, n, "spread, cap %d" % cap)
    sim.close()
    bitten(launches, cap, "chains")


def test_households(cap, launches):
    # (check_all: outbreaks, tables, SAR in one cell, at 5 groups, at 45 -- the last that fits the LDS -- and at 46)
    for name in ("fixture_a", "school"):                             # school: 2970 entries, the LDS form's four cases a lane are clipped
        sim, pop, ep, n, ref, house = t_households.started(name)
        t_households.check_all(sim, pop, n, ref, house, t_households.cached_pairs_of(name), "%s, cap %d" % (name, cap))
        sim.close()
    pop, ep, n, ref, _ = areas800()                                  # 10 936 buildings: k_list_tables' grid is clipped
    sus, house = once("areas800 sus", lambda: hh.sus_until(pop, ep, n)), dict(hh.households(ref, pop), jm=hh.all_pairs(ref, pop))
    sim = run_of(pop, ep, n)
    t_households.check_all(sim, pop, n, ref, house, lambda first, last, g: hh.pairs(ref, pop, ep, sus, first, last, hh.labels(pop, g) if g else None, max(1, g), jm=house["jm"]),
                           "800 areas, cap %d" % cap)
    sim.close()
    bitten(launches, cap, "households")


def test_places(cap, launches):
    # (check_kind: per place, tables, SAR in one cell, at 5 and 45 groups in LDS tiles, at 46 in global memory)
    sim = t_places.started("fixture_a")
    for kind in pl.KINDS:
        t_places.check_cached(sim, "fixture_a", kind, "fixture A, cap %d" % cap)
    sim.close()
    sim = t_places.started("edge")                                   # places around a wavefront, a workgroup's stretch, one tile and two
    for kind in ("work", "room"):
        t_places.check_cached(sim, "edge", kind, "edge, cap %d" % cap)
    sim.close()
    pop, ep, n, ref, sus = rooms()
    world = (pop, ep, n, ref, sus)
    busy = int(np.bincount(ref["step"][ref["step"] > 0]).argmax())
    windows = ((0, n), (max(1, n // 3), n // 2), (busy, busy))
    sim = run_of(pop, ep, n)
    for kind in ("room", "school"):
        t_places.check_kind(sim, pop, n, kind, pl.outbreaks(ref, pop, kind), lambda first, last, g, kind=kind: pl.pairs_counting(world, kind, first, last, g), windows,
                            "714 rooms, cap %d" % cap)
    sim.close()
    pop, ep, n, ref, _ = areas800()                                  # 10 936 buildings: k_list_tables' grid is clipped
    world = (pop, ep, n, ref, once("areas800 sus", lambda: hh.sus_until(pop, ep, n)))
    sim = run_of(pop, ep, n)
    t_places.check_kind(sim, pop, n, "work", pl.outbreaks(ref, pop, "work"), lambda first, last, g: pl.pairs_counting(world, "work", first, last, g), ((0, n), (100, 300)),
                        "800 areas, cap %d" % cap)
    sim.close()
    bitten(launches, cap, "places")


@pytest.mark.parametrize("name", ("fixture_a", "school", "bus"))
def test_contact_hours(name, cap, launches):
    # (check_all: one cell and per case; 5 groups in the LDS; on school also 32 groups, the last that fit it, and 33 in global memory.
    # fixture A: 146 routes, k_contact_route makes five trips over the bit set; bus: one route of 135 buses, whose entries a single
    # workgroup takes in turn -- one cell only, the walk of its 2693 riders by a few wavefronts is what takes the time)
    groups = {"fixture_a": (1, 5), "school": (1, 5, t_contacts.LDS_GROUPS, t_contacts.LDS_GROUPS + 1), "bus": (1,)}[name]
    sim, pop, ep, n, tr = t_contacts.started(name)
    if name == "bus":
        assert long_route_exposures(tree.cached("bus")[3]) >= 8      # k_contact_route takes several (step, route) items per workgroup
    t_contacts.check_all(sim, pop, n, tr, t_contacts.cached_rule_of(name), "%s, cap %d" % (name, cap), groups)
    sim.close()
    bitten(launches, cap, "contact hours")


def test_flows_imports_invasion_and_lineage_areas(cap, launches):
    sim, pop, ep, n, ref, ch = t_flows.started("fixture_a")
    t_flows.check_all(sim, pop, n, ref, ch, "fixture A, cap %d" % cap)
    sim.close()
    pop, ep, n, ref, ch = areas800()                                 # k_flow_resolve: a lane per area
    sim = run_of(pop, ep, n)
    t_flows.check_all(sim, pop, n, ref, ch, "800 areas, cap %d" % cap)
    sim.close()
    bitten(launches, cap, "flows")


def test_events_by_key_and_by_size(cap, launches):
    for name in ("fixture_a", "school"):                             # school: 2070 events, k_event_hist's grid of eight slots a lane is clipped
        sim, world = t_events.started(name)
        t_events.check_all(sim, world, "%s, cap %d" % (name, cap))
        sim.close()
    bitten(launches, cap, "events")


def test_compare_and_compare_series_with_the_baseline_kept(cap, launches):
    world, pair = "fixture_a", "masks"
    sim, pop, n, b, c, arm_b, arm_c = t_compare.both_arms(world, pair)
    t_compare.check_world(sim, pop, n, b, c, arm_b, arm_c, world, pair)
    sim.close()
    bitten(launches, cap, "compare")


def test_curve_summary(cap, launches):
    world = curve.fixture_a_rows()
    pop, ep, labels, n_groups, tables = world
    sim = Simulator(pop, ep)
    sim.set_groups(labels, n_groups)
    sim.run(t_curves.N_STEPS)
    for where in t_curves.WHERES:
        for status in t_curves.STATUS:
            t_curves.check(sim, tables, where, status, "cap %d" % cap)
            t_curves.check(sim, tables, where, status, "cap %d" % cap, first_step=250, last_step=600, threshold=5)
    sim.close()
    pop, ep, n, _, _ = areas800()                                    # 800 columns
    home = once("areas800 rows", lambda: curve.reference_rows(pop, ep, n, "home"))
    tables = {"home": home, "all": {"status_rows": home["status_rows"].sum(axis=1, keepdims=True)}}
    sim = run_of(pop, ep, n)
    for where in ("home", "all"):
        for status in t_curves.STATUS:
            t_curves.check(sim, tables, where, status, "800 areas, cap %d" % cap)
            t_curves.check(sim, tables, where, status, "800 areas, cap %d" % cap, first_step=100, last_step=350, threshold=2)
    sim.close()
    bitten(launches, cap, "curve summary")


def test_series_arrival_and_census(cap, launches):
    # area-status rows, the area rows and the group rows through their other entry points
    pop, ep, ref = _area_status_ref.fixture_a_tables()
    n = t_status.N_STEPS
    sim = Simulator(pop, ep)
    sim.run(n)
    t_status.check_records(sim, ref)
    t_status.check_all(sim, ref, n, "cap %d" % cap)
    t_status.check_all(sim, ref, n, "cap %d" % cap, first_step=5, stride=24)
    t_status.check_other_entry_points(sim, pop, ref, once("fixture_a exposure rows", lambda: _area_ref.reference_tables(pop, ep, n)["exposure_rows"]), n,
                                      "fixture A, cap %d" % cap)
    t_snapshot.assert_state(sim, ref["final_state"], "fixture A, cap %d" % cap)
    sim.close()
    # the groups: census, rows, arrival by group and by home area
    pop, ep, labels, n_groups = _group_ref.fixture_a_groups()
    gref = once("fixture_a groups", lambda: _group_ref.reference_tables(pop, ep, labels, n_groups, n))
    _, step, _ = once("fixture_a arrival", lambda: _arrival_ref.oracle_run(pop, ep, n))
    sim = run_of(pop, ep, n, (labels, n_groups))
    same(sim.group_census(), gref["status_rows"][n - 1], "group census, cap %d" % cap)
    for k, name in enumerate(STATUS):
        same(sim.group_series(name), gref["status_rows"][:, :, k], "group rows %s, cap %d" % (name, cap))
    same(sim.group_series("exposures"), gref["exposure_rows"], "group exposure rows, cap %d" % cap)
    same(sim.area_arrival("home"), _arrival_ref.arrival(_arrival_ref.home_area(pop), pop.n_areas, step, pop.seeds), "arrival by home area, cap %d" % cap)
    same(sim.area_arrival("group"), _arrival_ref.arrival(labels, n_groups, step, pop.seeds), "arrival by group, cap %d" % cap)
    sim.close()
    # 800 columns
    pop, ep, n, _, _ = areas800()
    ref = once("areas800 status", lambda: _area_status_ref.reference_tables(pop, ep, n))
    sim = run_of(pop, ep, n)
    t_status.check_all(sim, ref, n, "800 areas, cap %d" % cap)
    t_status.check_all(sim, ref, n, "800 areas, cap %d" % cap, first_step=7, n_rows=5, stride=48)
    sim.close()
    bitten(launches, cap, "series")


def test_snapshot_rollback_restart_and_restart_seeded(cap, launches):
    name, t, n = "york", 137, snap.N_STEPS
    pop, _ = snap.world(name)
    want_rec, want_state, want_log = snap.straight(name)

    def check(note):
        assert_same_records(sim.records_so_far(), want_rec)
        t_snapshot.assert_state(sim, want_state, note)
        t_snapshot.same_log(snap.log_sets(sim), want_log, note)

    sim = t_snapshot.new_sim(name)
    sim.run(t)
    sim.snapshot()
    sim.run(n - t)
    check("(first pass, cap %d)" % cap)
    sim.rollback()
    assert sim._steps == t
    sim.run(n - t)
    check("(after the rollback, cap %d)" % cap)
    sim.restart()
    sim.run(n)
    check("(after esim_restart, cap %d)" % cap)
    sim.restart(seeds=pop.seeds)
    sim.run(n)
    check("(after esim_restart_seeded, cap %d)" % cap)
    sim.close()
    bitten(launches, cap, "snapshot and restart")


def test_ensemble_folds(cap, launches):
    """The five kinds against the per-member calls, and those against the references, as the ensemble tests of each family do:
    the bodies of those tests, called as functions, on their worlds; and the kinds whose folds run over rows of areas again on
    the 800 areas, where a row has as many quads as three trips of one workgroup."""
    t_ens_series.test_area_rows_over_six_members_equal_numpy_over_the_series_calls_and_over_the_oracle("home", "incidence", 1)
    t_ens_series.test_area_rows_over_six_members_equal_numpy_over_the_series_calls_and_over_the_oracle("current", "infected", 2)
    t_ens_trans.test_settings_accumulators_equal_numpy_over_the_series_calls_and_over_the_reference(0)
    t_ens_trans.test_reproduction_accumulators_equal_numpy_over_the_series_calls_and_over_the_reference(0)
    t_compare.test_three_members_folded_against_members_compared_singly(once("paired members", t_compare.member_planes))
    t_curves.test_peaks_ensemble_kind(curve.fixture_a_rows())
    # 800 areas: three members; the first is the world's own run, whose rows the references give
    pop, ep, n, ref, _ = areas800()
    seeds = (int(ep.seed), 41, 42)
    window = dict(first_step=1, n_rows=3, stride=150)
    sim = Simulator(pop, ref_mod.copy_params(ep))

    def members():
        for seed in seeds:
            sim.restart(seed=seed)
            sim.run(n)
            yield seed

    sim.ensemble_begin_settings("home", None, min_cases=1, **window)
    xs = []
    for _ in members():
        xs.append(sim.setting_series("home", None, **window))
        sim.ensemble_fold()
    same(xs[0], ref_mod.rows(ref, pop, "home", 0xF, 1, 3, 150), "800 areas: the setting rows of the first member")
    ens_ref.same_fold(sim.ensemble_read_series(), ens_ref.fold_settings(xs, 1), t_ens_trans.SERIES_KEYS, "800 areas, settings")
    sim.ensemble_begin_reproduction("home", min_cohort=1, r=(1, 1), **window)
    xs = []
    for _ in members():
        xs.append(sim.reproduction_series("home", **window))
        sim.ensemble_fold()
    want = tree.reproduction_rows(ref, pop, "home", 1, 3, 150)
    same(xs[0][0], want[0], "800 areas: the cases of the first member")
    same(xs[0][1], want[1], "800 areas: the offspring of the first member")
    ens_ref.same_fold(sim.ensemble_read_reproduction(), ens_ref.fold_reproduction(xs, 1, (1, 1)), t_ens_trans.KEYS, "800 areas, reproduction")
    # peaks: a lane per area
    spec = dict(where="home", status="active", first_step=20, last_step=380, threshold=2)
    sim.ensemble_begin_peaks(min_peak=2, **spec)
    singles = []
    for _ in members():
        sim.ensemble_fold()
        singles.append(sim.curve_summary(**spec))
    home = once("areas800 rows", lambda: curve.reference_rows(pop, ep, n, "home"))
    t_curves.same_summary(singles[0], curve.summarize(curve.curves(home["status_rows"], "active"), 20, 380, 2), "800 areas: the summary of the first member")
    got, want = sim.ensemble_read_peaks(), curve.fold(singles, 2)
    assert got["members"] == 3 and want["hit"].any()
    for k in curve.PEAKS_KEYS:
        t_curves.same(got[k], want[k], "800 areas, peaks: %s" % k)
    # paired: the world's chance against two thirds of it
    policy = dict(exposure_chance=0.02)
    col, n_cols = cr.columns(pop, "home")
    pwin = dict(first_step=0, n_rows=7, stride=64, cumulative=True)
    sim.ensemble_begin_paired("home", min_baseline=2, min_averted=1, **pwin)
    singly = []
    for seed in seeds[:2]:
        t_compare.run_arm(sim, ep, dict(seed=seed), n)
        sim.keep_baseline()
        t_compare.run_arm(sim, ep, dict(policy, seed=seed), n)
        singly.append(sim.compare_series("home", **pwin))
        sim.ensemble_fold()
    b, c = once("areas800 planes", lambda: tuple(cr.steps_of_run(pop, ref_mod.copy_params(ep, **over), n)[0] for over in ({}, policy)))
    want_b, want_c = cr.series(b, c, col, n_cols, 0, 7, 64, True)
    assert np.array_equal(singly[0][0], want_b) and np.array_equal(singly[0][1], want_c), "800 areas: the event rows of the first member"
    got, want = sim.ensemble_read_paired(), cr.fold_paired(singly, 2, 1)
    assert got["members"] == 2 and want["hit"].any()
    for k in cr.PAIRED_KEYS:
        assert np.array_equal(got[k], want[k]), ("800 areas, paired", k)
    sim.close()
    bitten(launches, cap, "ensemble folds")


# ---- 2. a realistic log length: York, 5000 steps, capped against uncapped -------------------------------------------------------
def york_outputs(pop, n, half, over):
    """Every output of the families above at the end of n steps under the default parameters changed by `over` -- run to `half`, snapshot, on to n,
    rolled back and run to n again --, the comparison against a baseline kept from a run under another seed: {name: array}."""
    out = {}

    def put(name, value):
        if isinstance(value, dict):
            for k, v in value.items():
                put("%s.%s" % (name, k), v)
        elif isinstance(value, (tuple, list)):
            for i, v in enumerate(value):
                put("%s.%d" % (name, i), v)
        else:
            out[name] = np.asarray(value)

    ep = _lib.default_params(max_steps=5600, **over)
    sim = Simulator(pop, ep)
    lab, g = pop.age_bands([18, 40, 65])
    sim.set_groups(lab, g)
    sim.restart(seed=int(ep.seed) + 1)                               # the baseline: the same world under another seed
    sim.run(n)
    sim.keep_baseline()
    sim.restart(seed=int(ep.seed))
    sim.run(half)
    sim.snapshot()
    sim.run(n - half)
    sim.rollback()                                                   # the snapshot's own values: the same future again
    sim.run(n - half)
    put("records", sim.records_so_far())
    put("state", sim.download_state())
    put("log", sim.exposure_events())
    put("settings", sim.exposure_settings())
    put("setting_rows", sim.setting_series("home", first_step=5, stride=24))
    put("buildings", sim.building_exposures(1, n))
    put("tree", sim.transmission_tree())
    put("offspring", sim.offspring(1, n))
    put("reproduction", sim.reproduction_series("home", first_step=0, stride=24))
    put("mixing", sim.mixing_matrix())
    put("chains", sim.transmission_chains())
    put("outbreaks", sim.outbreaks())
    put("ages", sim.transmission_ages())
    put("hh", sim.household_outbreaks())
    put("hh_sizes", sim.household_final_sizes())
    put("hh_sar", sim.household_sar("all", 0, n, complete=False))
    put("hh_sar_g", sim.household_sar("group", 0, n, complete=False))
    for kind in pl.KINDS:
        put("place." + kind, sim.place_outbreaks(kind))
        put("place_sizes." + kind, sim.place_sizes(kind))
    for kind in ("work", "room"):
        put("place_sar." + kind, sim.place_sar(kind, "all", 0, n, complete=False))
        put("place_sar_g." + kind, sim.place_sar(kind, "group", 0, n, complete=False))
    busy = min(max(int(np.argmax(out["records"]["infected"])) + 1, 25), n - 24)
    put("contacts", sim.contact_hours("all", None, busy - 24, busy + 24, per_case=True))
    put("contacts_g", sim.contact_hours("group", None, busy - 24, busy + 24))
    put("flows", sim.area_flows())
    put("imports", sim.area_imports())
    put("invasion", sim.area_invasion())
    put("lineages", sim.lineage_areas())
    put("events", sim.transmission_events(order="size"))
    put("event_sizes", sim.event_sizes())
    put("compare", sim.compare("home", 0, n, citizens=True))
    put("compare_rows", sim.compare_series("home", 0, None, 24, True))
    for where in ("all", "home", "group"):
        put("curve." + where, sim.curve_summary(where, "active", 1, n, 5))
    put("area_rows", sim.area_series("exposures", first_step=3, stride=24))
    for what in STATUS + ("incidence",):
        put("status_rows." + what, sim.area_status_series(what, "home", first_step=3, stride=24))
    put("status_rows.current", sim.area_status_series("infected", "current", first_step=3, stride=24))
    put("group_rows", sim.group_series("infected", first_step=3, stride=24))
    put("group_exposures", sim.group_series("exposures", first_step=3, stride=24))
    put("arrival", sim.area_arrival("home"))
    put("arrival_g", sim.area_arrival("group"))
    put("census", sim.area_census("home"))
    put("group_census", sim.group_census())
    window = dict(first_step=24, n_rows=50, stride=96)
    sim.ensemble_begin_series("home", "infected", min_cases=2, **window)
    sim.ensemble_fold()
    put("fold_series", sim.ensemble_read_series())
    sim.ensemble_begin_settings("home", None, min_cases=1, **window)
    sim.ensemble_fold()
    put("fold_settings", sim.ensemble_read_series())
    sim.ensemble_begin_reproduction("home", min_cohort=1, r=(1, 1), **window)
    sim.ensemble_fold()
    put("fold_reproduction", sim.ensemble_read_reproduction())
    sim.ensemble_begin_paired("home", min_baseline=2, min_averted=1, cumulative=True, **window)
    sim.ensemble_fold()
    put("fold_paired", sim.ensemble_read_paired())
    sim.ensemble_begin_peaks(min_peak=3, where="home", status="active", first_step=1, last_step=n, threshold=2)
    sim.ensemble_fold()
    put("fold_peaks", sim.ensemble_read_peaks())
    records = sim.debug_launches()
    sim.close()
    return out, records


# York's epidemic is contained by its interventions: 2663 log entries in 5000 steps under the default parameters.  Without the
# interventions it takes most of the town, 164 864 entries: the log length of a production run (both counted with the CPU oracle).
YORK = {"default": ({}, 2000), "unmitigated": (dict(lockdown_threshold=2.0, vaccination_threshold=2.0, mask_pt_threshold=2.0, mask_everywhere_threshold=2.0), 150000)}


@pytest.mark.parametrize("world", sorted(YORK))
def test_york_5000_steps_capped_equals_uncapped(world, monkeypatch):
    """No oracle: the reference is the uncapped code.  197 603 citizens, so a lane per citizen makes 772 trips at cap 1; without
    the interventions a lane per log entry makes some 640 and a wavefront per entry some 41 000."""
    over, at_least = YORK[world]
    pop = Population.synthetic("york")
    n, half = 5000, 2500
    monkeypatch.delenv("ESIM_GRID_CAP", raising=False)
    plain, records = york_outputs(pop, n, half, over)
    assert records == {}                                             # nothing is recorded while the knob is unset
    entries = len(plain["log.0"])
    assert entries >= at_least and plain["flows.0"].size > 100 and plain["events.size"].size > 1000
    for cap in CAPS:
        monkeypatch.setenv("ESIM_GRID_CAP", str(cap))
        capped, records = york_outputs(pop, n, half, over)
        assert sorted(capped) == sorted(plain)
        for k in sorted(plain):
            a, b = plain[k], capped[k]
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), "%s, ESIM_GRID_CAP=%d: %s differs from the uncapped run" % (world, cap, k)
        assert max(r["max_trips"] for r in records.values() if r["clipped"]) >= entries // (4 * cap)       # (a wavefront per entry, four to a workgroup)


# ---- 3. the union ------------------------------------------------------------------------------------------------------------------
def launch_sites():
    """{"file:line": (file, first line, last line)} of every grid_capped / grid_clamp call of the host code that the product build
    compiles.  The last line is that of the statement's end: inside the arguments of a launch macro that spans several lines the
    compiler reports the line where the macro's call ends."""
    sites = {}
    for name in SITE_FILES:
        skip = []                                                    # one entry per open conditional on a macro of NOT_DEFINED: True while its text is skipped
        lines = open(os.path.join(CSRC, name)).read().split("\n")
        for no, line in enumerate(lines, 1):
            m = re.match(r"\s*#\s*(ifdef|ifndef|else|endif)\b\s*(\w*)", line)
            if m:
                kind, macro = m.groups()
                if kind in ("ifdef", "ifndef"):
                    skip.append((kind == "ifdef") if macro in NOT_DEFINED else None)
                elif kind == "else" and skip and skip[-1] is not None:
                    skip[-1] = not skip[-1]
                elif kind == "endif" and skip:
                    skip.pop()
                continue
            if any(skip):
                continue
            if re.search(r"\bgrid_(capped|clamp)\(", line) and not re.match(r"\s*(//|uint32_t grid_)", line):
                last = no
                while not lines[last - 1].split("//")[0].rstrip().endswith(";"):
                    last += 1
                sites["%s:%d" % (name, no)] = (name, no, last)
    return sites


def canonical(site, sites=None):
    """The name of launch_sites() for a site as the library reports it."""
    sites = launch_sites() if sites is None else sites
    name, line = site.split(":")
    hits = [k for k, (f, first, last) in sites.items() if f == name and first <= int(line) <= last]
    assert len(hits) == 1, "%s: %d launch sites of the host code span this line" % (site, len(hits))
    return hits[0]


def test_every_launch_site_was_clipped():
    """Runs last: over the module every launch site was clipped by the cap in a batch of calls whose longest loop made three trips
    or more.  Prints the per-site table (launches, clipped, largest trips, per cap)."""
    sites = launch_sites()
    assert len(sites) >= 55
    print("\nsite, then per cap: launches clipped max_trips")
    for site in sites:
        print("%-28s %s" % (site, "   ".join("cap %d: %5d %5d %6d" % ((cap,) + tuple(TABLE.get((cap, site), (0, 0, 0)))) for cap in CAPS)))
    unknown = sorted(set(SEEN) - set(sites))
    assert not unknown, "records of sites the scan of the host code does not know: %s" % unknown
    assert not set(ALLOWED_UNCLIPPED) - set(sites)
    missing = [s for s in sites if SEEN.get(s, 0) < 3 and s not in ALLOWED_UNCLIPPED]
    assert not missing, "launch sites never clipped with three trips or more: %s" % ", ".join("%s (%d)" % (s, SEEN.get(s, 0)) for s in missing)
