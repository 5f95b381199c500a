"""Ensembles on several contexts: esim_ensemble_merge, esim_ensemble_save / _load and Ensemble(devices=...).  Every
accumulator is an integer count or sum, so every comparison here is exact integer equality: a merged ensemble against the same
members folded in sequence on one context (existing code, pinned to numpy by the tests of every kind) and against the numpy sum
of the two read-outs taken before the merge, which is arithmetic independent of the library.  The world, the begins and the
readers are those of tests/test_ensemble_kinds_gpu.py."""
import ctypes as C

import numpy as np
import pytest

from epidemicsimulator_amd import Ensemble, Population, Simulator, _lib
from test_ensemble_kinds_gpu import BEDS, E, HORIZON, I, N_GROUPS, PEAKS, R, SPECS, STEPS, W, W5, labels_of, make_world

pytestmark = pytest.mark.gpu

EINVAL, ESTATE, ERANGE = -1, -4, -5
MEMBERS = 5
KEEP_WHATS = ("value", "peak_step", "duration")
CASES = [(name, what) for name in sorted(SPECS) for what in (KEEP_WHATS if "peaks" in name else ("value",))]


def same(a, b, what=""):
    """a and b are the same: dicts by key, sequences by element, arrays by dtype, shape and every bit (NaN equals NaN)."""
    if isinstance(a, dict):
        assert isinstance(b, dict) and sorted(a) == sorted(b), (what, sorted(a), sorted(b))
        for k in a:
            same(a[k], b[k], "%s[%r]" % (what, k))
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), (what, len(a), len(b))
        for i, (x, y) in enumerate(zip(a, b)):
            same(x, y, "%s[%d]" % (what, i))
    elif isinstance(a, np.ndarray):
        assert isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
        assert a.tobytes() == b.tobytes() or (a.dtype.kind == "f" and np.array_equal(a, b, equal_nan=True)), "%s differs" % what
    elif isinstance(a, float) and a != a:
        assert b != b, what
    else:
        assert a == b, (what, a, b)


def run_member(sim, members, m):
    seed, cases = members[m]
    sim.restart(seed=seed, seeds=cases)
    sim.run(STEPS)


def fold_members(sim, members, which):
    for m in which:
        run_member(sim, members, m)
        sim.ensemble_fold()


def read_all(sim, name):
    """What the kind's reader returns and, where the kind keeps members, the members kept."""
    out = {"acc": getattr(sim, SPECS[name][3])()}
    if SPECS[name][5] is not None:
        info = C.c_uint32(0)
        stored = sim.lib.esim_ensemble_members_info(sim._ctx, None, C.byref(info), None, None) == 0
        out["kept"] = sim.ensemble_members() if stored and info.value else None
    return out


def begin(sim, name, capacity=None, what="value"):
    SPECS[name][0](sim)
    if capacity is not None and SPECS[name][5] is not None:
        sim.ensemble_keep_members(capacity, what)


@pytest.fixture(scope="module")
def worlds():
    """Three contexts on one population and the five members every test folds: real runs under other seeds and index cases."""
    sims = [make_world() for _ in range(3)]
    pop = sims[0].population
    members = [(100 + m, pop.draw_index_cases(5, 100 + m)) for m in range(MEMBERS)]
    yield sims, members
    for s in sims:
        s.close()


@pytest.fixture(scope="module")
def pair():
    """Two contexts of their own for the refusals, which change labels and tables."""
    sims = [make_world(), make_world()]
    yield sims
    for s in sims:
        s.close()


# ---- 1. every kind: A folds members 0-2, B members 3-4, C all five; B merged into A is C -----------------------------------------
@pytest.mark.parametrize("name,what", CASES, ids=["%s/%s" % c for c in CASES])
def test_merged_equals_sequential_for_every_kind(worlds, name, what):
    (a, b, c), members = worlds
    keys = SPECS[name][4]
    for sim, cap in ((a, MEMBERS), (b, 2), (c, MEMBERS)):
        begin(sim, name, cap, what)
    fold_members(a, members, (0, 1, 2))
    fold_members(b, members, (3, 4))
    fold_members(c, members, range(MEMBERS))
    ra, rb = read_all(a, name), read_all(b, name)
    assert ra["acc"]["members"] == 3 and rb["acc"]["members"] == 2
    a.ensemble_merge(b)
    got, want = read_all(a, name), read_all(c, name)
    same(got, want, name + ": merged against sequential")
    assert got["acc"]["members"] == MEMBERS
    for k in keys:                                   # numpy over the two earlier read-outs: independent of the library
        total = ra["acc"][k] + rb["acc"][k]
        assert total.dtype == got["acc"][k].dtype and (got["acc"][k] == total).all(), (name, k)
    assert any(ra["acc"][k].any() for k in keys) and any(rb["acc"][k].any() for k in keys), name
    if "kept" in got:
        assert (got["kept"] == np.concatenate([ra["kept"], rb["kept"]])).all(), name       # slot for slot, in order
        assert a.ensemble_members_info()["kept"] == MEMBERS
        for call in (lambda s: s.ensemble_quantiles(ranks=(0, 2, 4)), lambda s: s.ensemble_quantiles((0.1, 0.5, 0.9), "linear"), lambda s: s.ensemble_exceedance((0, 1, 3, 2 ** 33)),
                     lambda s: s.ensemble_depth(), lambda s: s.ensemble_band(0.5), lambda s: s.ensemble_band(0.6, pooled=True), lambda s: s.ensemble_distances("l1"),
                     lambda s: s.ensemble_distances("differ", never_as=HORIZON)):
            same(call(a), call(c), name)
    same(read_all(b, name), rb, name + ": src after the merge")
    assert b.ensemble_members_info()["kept"] == 2 if "kept" in rb else True


# ---- 2. the shapes of the merge kernel: every tail of the 16 B accesses, the wavefront, the workgroup; pieces; capped grids --------
SHAPE_GROUPS = (1, 3, 4, 5, 63, 64, 65, 257, 1000)
_shape_reference = {}


def shape_world(groups):
    pop = Population.synthetic("york", n_citizens=1000, n_areas=3, citizens_per_school=1000, n_seeds=5)
    sim = Simulator(pop, _lib.default_params(exposure_chance=0.01, max_steps=120))
    sim.set_groups((np.arange(pop.n_citizens) * 7 % groups).astype(np.uint16), groups)
    return sim


def shape_fold(sim, seeds, capacity):
    sim.ensemble_begin("group", E | I | R, 1)
    sim.ensemble_keep_members(capacity)
    for s in seeds:
        sim.restart(seed=s)
        sim.run(120)
        sim.ensemble_fold()


@pytest.mark.parametrize("piece", (64, None))
@pytest.mark.parametrize("cap", (1, 3))
@pytest.mark.parametrize("groups", SHAPE_GROUPS)
def test_the_merge_kernel_at_every_tail_with_capped_grids_and_small_pieces(monkeypatch, groups, cap, piece):
    if groups not in _shape_reference:               # the three members folded in sequence, once per shape, without a knob
        monkeypatch.delenv("ESIM_GRID_CAP", raising=False)
        monkeypatch.delenv("ESIM_MERGE_PIECE", raising=False)
        ref = shape_world(groups)
        shape_fold(ref, (1, 2, 3), 3)
        _shape_reference[groups] = (ref.ensemble_read(), ref.ensemble_members())
        ref.close()
    monkeypatch.setenv("ESIM_GRID_CAP", str(cap))
    if piece is not None:
        monkeypatch.setenv("ESIM_MERGE_PIECE", str(piece))
    else:
        monkeypatch.delenv("ESIM_MERGE_PIECE", raising=False)
    a, b = shape_world(groups), shape_world(groups)
    try:
        shape_fold(a, (1, 2), 3)
        shape_fold(b, (3,), 1)
        ra, rb = a.ensemble_read(), b.ensemble_read()
        a.debug_launches(reset=True)
        a.ensemble_merge(b)
        got, kept = a.ensemble_read(), a.ensemble_members()
        want, want_kept = _shape_reference[groups]
        same(got, want, "%d groups" % groups)
        assert (kept == want_kept).all() and kept.shape == (3, 1, groups)
        for k in ("hit", "sum", "sumsq"):
            assert (got[k] == ra[k] + rb[k]).all(), k
        assert got["sum"].any() and rb["sum"].any()
        assert got["members"] == 3 and (got["hit"] < 3).any() if groups > 5 else True
        # the launches of the merge site: a piece of n cells takes ceil(n / 256) workgroups of one wavefront, four cells a lane
        sites = {k: v for k, v in a.debug_launches().items() if "esim_host_merge.h" in k}
        assert len(sites) == 1, sites
        rec = list(sites.values())[0]
        per = piece if piece is not None else 1 << 20
        pieces = [min(per, groups - at) for at in range(0, groups, per)]
        grids = [-(-n // 256) for n in pieces]
        assert rec["launches"] == len(pieces) and rec["clipped"] == sum(g > cap for g in grids), (rec, pieces)
        assert rec["max_trips"] == max(-(-n // (min(g, cap) * 256)) for n, g in zip(pieces, grids)), (rec, pieces)
        if groups == 1000 and piece is None:
            assert rec["clipped"] == 1 and rec["max_trips"] > 1, rec
        if piece is not None and groups > 64:
            assert rec["launches"] > 1, rec
    finally:
        a.close()
        b.close()


# ---- 3. save, then load ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,what", [("series home/incidence", "value"), ("peaks home", "peak_step"), ("reproduction home", "value"), ("paired home", "value")])
def test_save_then_load_restores_adds_and_resumes(worlds, name, what):
    (a, b, c), members = worlds
    begin(a, name, MEMBERS, what)
    fold_members(a, members, (0, 1, 2))
    blob = a.ensemble_save()
    size = C.c_size_t(0)
    _lib.check(a.lib.esim_ensemble_save_size(a._ctx, C.byref(size)), a._ctx)
    assert isinstance(blob, bytes) and size.value == len(blob) and blob[:4] == b"EENS"
    ra = read_all(a, name)
    # behind a fresh begin and keep on another context it restores
    begin(b, name, 6, what)
    # a blob with a byte cut off, with a byte added, cut inside its header, empty, the magic word alone: refused, nothing changes
    before = read_all(b, name)
    for bad in (blob[:-1], blob + b"\0", blob[:40], b"", b"EENS"):
        buf = np.frombuffer(bad, np.uint8)
        assert b.lib.esim_ensemble_load(b._ctx, C.c_void_p(buf.ctypes.data) if buf.size else None, buf.size) == EINVAL, len(bad)
    same(read_all(b, name), before, name + ": behind refused loads")
    b.ensemble_load(blob)
    same(read_all(b, name), ra, name + ": restored")
    # loaded twice it doubles every accumulator and the member counter
    b.ensemble_load(blob)
    twice = read_all(b, name)
    assert twice["acc"]["members"] == 6
    for k in SPECS[name][4]:
        assert (twice["acc"][k] == 2 * ra["acc"][k]).all() and ra["acc"][k].dtype == twice["acc"][k].dtype, (name, k)
    if "kept" in ra:
        assert (twice["kept"] == np.concatenate([ra["kept"]] * 2)).all()
    # saved, loaded behind a new begin and folded further it is the five members folded in sequence
    begin(b, name, MEMBERS, what)
    b.ensemble_load(blob)
    fold_members(b, members, (3, 4))
    begin(c, name, MEMBERS, what)
    fold_members(c, members, range(MEMBERS))
    same(read_all(b, name), read_all(c, name), name + ": resumed")
    # a blob of another ensemble, and one with more members than the store has room for: refused, nothing changes
    before = read_all(b, name)
    if "kept" in before:
        assert b.lib.esim_ensemble_load(b._ctx, blob, len(blob)) == ERANGE
    begin(a, "settings home", MEMBERS)
    with pytest.raises(_lib.EsimError) as err:
        a.ensemble_load(blob)
    assert err.value.code == EINVAL and "differs" in str(err.value)
    same(read_all(b, name), before, name + ": behind refused loads")


# ---- 4. refusals: checked on the host, both contexts untouched ---------------------------------------------------------------------
ALTERED = {     # per begin of SPECS the same begin with one parameter changed, and a word of the field's name in the refusal
    "census home": (lambda s: s.ensemble_begin("home", E | I | R, 3), "min_cases"),
    "census group": (lambda s: s.ensemble_begin("group", I, 6), "status_mask"),
    "arrival home": (lambda s: s.ensemble_begin_arrival("home", HORIZON + 1), "horizon"),
    "series home/incidence": (lambda s: s.ensemble_begin_series("home", "incidence", min_cases=2, **W), "min_cases"),
    "series current/infected": (lambda s: s.ensemble_begin_series("current", "exposed", min_cases=2, **W), "status"),
    "series group": (lambda s: s.ensemble_begin_series("group", "exposures", min_cases=3, **dict(W, first_step=2)), "first_step"),
    "settings by setting": (lambda s: s.ensemble_begin_settings("setting", min_cases=3, **dict(W, stride=24)), "stride"),
    "settings home": (lambda s: s.ensemble_begin_settings("home", ("household", "workplace"), min_cases=1, **W), "setting_mask"),
    "reproduction all": (lambda s: s.ensemble_begin_reproduction("all", min_cohort=1, r=(1, 5), **W), "r_den"),
    "reproduction home": (lambda s: s.ensemble_begin_reproduction("home", min_cohort=3, r=(1, 2), **W), "min_cohort"),
    "paired home": (lambda s: s.ensemble_begin_paired("home", min_baseline=0, min_averted=2, **W), "min_averted"),
    "paired all, cumulative": (lambda s: s.ensemble_begin_paired("all", cumulative=False, min_baseline=1, min_averted=2, **W), "cumulative"),
    "peaks home": (lambda s: s.ensemble_begin_peaks(min_peak=3, **dict(PEAKS, threshold=3)), "threshold"),
    "burden_peaks home": (lambda s: s.ensemble_begin_burden_peaks(min_peak=2, **dict(BEDS, last_step=STEPS - 1)), "last_step"),
    "burden_series home/occupancy": (lambda s: s.ensemble_begin_burden_series("home", "admissions", min_count=2, **W), "burden_what"),
    "burden_paired group/admissions": (lambda s: s.ensemble_begin_burden_paired("group", "admissions", cumulative=True, min_baseline=2, min_averted=1, **W), "min_baseline"),
    "series home/infected, five rows": (lambda s: s.ensemble_begin_series("home", "infected", min_cases=1, **dict(W5, n_rows=4)), "n_rows"),
}


def refused(dst, src, name_dst, name_src, code, word):
    """The merge of src into dst returns `code` with `word` in its text, and both read back what they read before."""
    before = read_all(dst, name_dst), read_all(src, name_src)
    assert dst.lib.esim_ensemble_merge(dst._ctx, src._ctx) == code, (name_dst, name_src)
    text = dst.lib.esim_last_error(dst._ctx).decode()
    assert word in text, (name_dst, name_src, text)
    same((read_all(dst, name_dst), read_all(src, name_src)), before, "%s <- %s" % (name_dst, name_src))


def test_a_merge_of_a_context_into_itself_or_without_a_begin_is_refused(pair):
    a, b = pair
    base = "series home/incidence"
    begin(a, base, 4)
    a.ensemble_fold()
    before = read_all(a, base)
    assert a.lib.esim_ensemble_merge(a._ctx, a._ctx) == EINVAL and a.lib.esim_ensemble_merge(a._ctx, None) == EINVAL and a.lib.esim_ensemble_merge(None, a._ctx) == EINVAL
    fresh = Simulator(a.population, _lib.default_params())        # uploaded, no begin since
    try:
        assert a.lib.esim_ensemble_merge(a._ctx, fresh._ctx) == ESTATE and "(src)" in a.lib.esim_last_error(a._ctx).decode()
        assert a.lib.esim_ensemble_merge(fresh._ctx, a._ctx) == ESTATE and "(dst)" in a.lib.esim_last_error(fresh._ctx).decode()
        size = C.c_size_t(0)
        assert a.lib.esim_ensemble_save_size(fresh._ctx, C.byref(size)) == ESTATE and a.lib.esim_ensemble_load(fresh._ctx, C.cast(b"EENS", C.c_void_p), 4) == ESTATE
    finally:
        fresh.close()
    same(read_all(a, base), before, "behind the refusals")


@pytest.mark.parametrize("name", sorted(ALTERED))
def test_one_changed_parameter_of_the_begin_is_refused_by_name(pair, name):
    a, b = pair
    begin(a, name, 4)
    ALTERED[name][0](b)
    if SPECS[name][5] is not None:
        b.ensemble_keep_members(4)
    a.ensemble_fold()
    b.ensemble_fold()
    refused(a, b, name, name, ESTATE, ALTERED[name][1])
    refused(b, a, name, name, ESTATE, ALTERED[name][1])


def test_another_kind_where_shape_store_groups_and_tables_are_refused(pair):
    a, b = pair
    base = "series home/incidence"

    def setup(name_b, keep_a=4, keep_b=4, what_b="value", name_a=base, what_a="value"):
        begin(a, name_a, keep_a, what_a)
        begin(b, name_b, keep_b, what_b)
        a.ensemble_fold()
        b.ensemble_fold()

    setup("settings home")                                   # another kind over the same shape
    refused(a, b, base, "settings home", ESTATE, "the kind")
    setup("burden_series home/occupancy")
    refused(a, b, base, "burden_series home/occupancy", ESTATE, "the kind")
    begin(a, base, 4)
    b.ensemble_begin_series("current", "incidence", min_cases=1, **W)   # another where
    b.ensemble_keep_members(4)
    a.ensemble_fold()
    b.ensemble_fold()
    refused(a, b, base, base, ESTATE, "where")
    begin(a, "series home/infected, five rows", 4)           # other rows
    b.ensemble_begin_series("home", "infected", min_cases=1, **W)
    b.ensemble_keep_members(4)
    a.ensemble_fold()
    b.ensemble_fold()
    refused(a, b, "series home/infected, five rows", "series home/infected, five rows", ESTATE, "n_rows")
    setup(base, keep_b=None)                                 # a store on one side only, either way
    refused(a, b, base, base, ESTATE, "the store")
    refused(b, a, base, base, ESTATE, "the store")
    setup("peaks home", what_b="duration", name_a="peaks home", what_a="value")     # another `what`
    refused(a, b, "peaks home", "peaks home", ESTATE, "the store's what")
    # other group sizes under the same number of groups
    other = labels_of(b.population).copy()
    other[:10] = 0
    b.set_groups(other, N_GROUPS)
    setup("series group", name_a="series group")
    refused(a, b, "series group", "series group", ESTATE, "the groups' sizes")
    b.set_groups(labels_of(b.population), N_GROUPS)
    setup("series group", name_a="series group")
    a.ensemble_merge(b)                                      # (the same sizes again: accepted)
    # other burden tables
    b.set_burden(_lib.burden_tables([0.5, 0.6, 0.4, 0.7], [0.3, 0.2, 0.4, 0.25], [0.3, 0.4, 0.3], [0.2, 0.3, 0.5], delay_unit=12, stay_unit=12))
    setup("burden_peaks home", name_a="burden_peaks home")
    refused(a, b, "burden_peaks home", "burden_peaks home", ESTATE, "the burden tables in force")


def test_the_store_takes_the_members_of_both_up_to_its_capacity_and_no_more(pair):
    a, b = pair
    name = "census home"
    begin(a, name, 4)
    begin(b, name, 3)
    for sim, folds in ((a, 2), (b, 3)):
        for _ in range(folds):
            sim.ensemble_fold()
    refused(a, b, name, name, ERANGE, "nothing was merged")   # 2 + 3: one above the capacity
    begin(b, name, 3)
    b.ensemble_fold()
    b.ensemble_fold()
    ra, rb = read_all(a, name), read_all(b, name)
    a.ensemble_merge(b)                                      # 2 + 2: exactly the capacity
    got = read_all(a, name)
    assert got["acc"]["members"] == 4 and a.ensemble_members_info() == dict(a.ensemble_members_info(), kept=4, capacity=4)
    assert (got["kept"] == np.concatenate([ra["kept"], rb["kept"]])).all() and (got["acc"]["sum"] == ra["acc"]["sum"] + rb["acc"]["sum"]).all()
    assert a.lib.esim_ensemble_fold(a._ctx) == ERANGE        # (and the store is full, as after four folds)
    # a src without a member folded: a valid call that changes nothing
    begin(a, name, 4)
    a.ensemble_fold()
    begin(b, name, 2)
    before = read_all(a, name)
    a.ensemble_merge(b)
    same(read_all(a, name), before, "an empty src")


# ---- 5. through Python: Ensemble(devices=...) against devices=None ------------------------------------------------------------------
WORLD = dict(n_citizens=600, n_areas=3, citizens_per_school=600, n_seeds=5)
RUN_AREA = dict(kind="series", where="home", what="incidence", first_step=1, n_rows=8, stride=25, quantiles=(0.25, 0.5, 0.75), exceed=(1, 3), band=0.5, clusters=2)


def ensemble_of(devices):
    pop = Population.synthetic("york", **WORLD)
    return Ensemble(pop, _lib.default_params(exposure_chance=0.01, vaccination_threshold=0.011, vaccination_rate=25, max_steps=STEPS, exposed_time=24, infected_time=72),
                    group=(labels_of(pop), N_GROUPS), devices=devices)


def ensemble_calls(ens):
    """name -> what the method returns, as the attributes of its result object."""
    out = {}
    out["run"] = vars(ens.run(ens.index_cases(5, n=5), STEPS, area=RUN_AREA, settings=dict(stride=50), reproduction=dict(stride=48)))
    out["forecast"] = vars(ens.forecast(80, ens.seeds(4), STEPS, area=dict(where="group", min_cases=2, quantiles=(0.5,))))
    out["compare"] = vars(ens.compare({}, {"lockdown_threshold": 0.001}, ens.seeds(3, first=7), STEPS, where="home", rows=dict(stride=50), quantiles=(0.5,)))
    out["households"] = vars(ens.households(ens.index_cases(3, n=5), STEPS, where="group"))
    return out


@pytest.fixture(scope="module")
def one_context():
    ens = ensemble_of(None)
    out = ensemble_calls(ens)
    two = vars(ens.run(ens.seeds(2), STEPS, area=RUN_AREA))
    ens.close()
    return out, two


def test_two_contexts_on_one_device_give_what_one_context_gives(one_context):
    ens = ensemble_of((0, 0))
    try:
        assert len(ens._lanes()) == 2 and ens._lanes()[0].simulator is ens.simulator and ens._lanes()[1].simulator is not ens.simulator
        got = ensemble_calls(ens)
    finally:
        ens.close()
    want = one_context[0]
    assert want["run"]["area"]["members"] == 5 and want["run"]["area"]["quantiles"].any() and want["compare"]["summary"]["members"] == 3
    for name in want:
        same(got[name], want[name], name)


def test_an_empty_block_changes_nothing(one_context):
    ens = ensemble_of((0, 0, 0))
    try:
        got = vars(ens.run(ens.seeds(2), STEPS, area=RUN_AREA))
    finally:
        ens.close()
    same(got, one_context[1], "two members on three contexts")


def test_an_exception_in_one_block_is_raised_once_the_others_have_joined():
    ens = ensemble_of((0, 0))
    try:
        with pytest.raises(_lib.EsimError):
            ens.run([{"seed": 1}, {"seed": 2}, {"seed": 3}, {"seed": 4, "vaccination_rate": 1 << 20}], STEPS, area=dict(where="home"))
        got = vars(ens.run(ens.seeds(2), STEPS, area=RUN_AREA))          # the contexts are usable afterwards
        assert got["area"]["members"] == 2
    finally:
        ens.close()


# ---- 6. two devices, where there are two ---------------------------------------------------------------------------------------------
def hip_device_count():
    """The devices that the HIP runtime libesim is linked against sees, asked of that runtime as this process has it loaded --
    not of a second runtime that another package would bring into the process."""
    _lib.load()
    with open("/proc/self/maps") as fh:
        paths = sorted({line.split()[-1] for line in fh if "libamdhip64" in line})
    assert len(paths) == 1, paths
    n = C.c_int(0)
    assert C.CDLL(paths[0]).hipGetDeviceCount(C.byref(n)) == 0
    return n.value


def test_two_devices_give_what_one_context_gives(one_context):
    if hip_device_count() < 2:
        pytest.skip("one GPU here: the peer transport between two devices (hipMemcpyPeerAsync across devices) needs at least two")
    ens = ensemble_of((0, 1))
    try:
        got = vars(ens.run(ens.index_cases(5, n=5), STEPS, area=RUN_AREA, settings=dict(stride=50), reproduction=dict(stride=48)))
    finally:
        ens.close()
    same(got, one_context[0]["run"], "devices=(0, 1)")
