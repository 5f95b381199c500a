"""What Simulator hands to the library and what it hands back, pinned without a GPU: a Simulator made without its
constructor over a fake population and a stand-in for the library that records every esim_* call -- a scalar argument as its
value, a pointer argument as its ctypes type -- and answers from a script.  Per case the calls made and the dtype and shape of
everything returned (or the type of the exception) are compared with tests/marshalling_calls.json, which was recorded from
the wrappers as they stood before their marshalling was folded into epidemicsimulator_amd/_marshal.py: a dtype, a column
count or a default of a window that drifts fails the case and prints both records.  One kind of record is younger than the
rest: a begin by group on a simulator without labels (which the library refuses) used to leave 0 columns to its reader in
five of the begins and 1 in the others; it is 1 in all now, and those records say so.  The file holds every distinct text
once (packed()); dump(collect(), path) writes it anew."""
import ctypes as C
import itertools
import json
import os

import numpy as np
import pytest

from epidemicsimulator_amd import Simulator, StatisticsRecorder, _lib

HERE = os.path.dirname(os.path.abspath(__file__))
SIZED = ("esim_get_seeds", "esim_download_exposure_log", "esim_routes", "esim_area_flows", "esim_lineage_areas", "esim_transmission_events")
KEPT = 40                                  # members the scripted store holds: more than RANKS_MAX distinct ranks can be asked for


CTYPES = {C.c_uint8: "u8", C.c_uint16: "u16", C.c_uint32: "u32", C.c_int32: "i32", C.c_uint64: "u64", C.c_int64: "i64", C.c_double: "f64"}


def arg(a):
    """One argument of a library call as text: an int as its value, None as -, a pointer as * and its type, byref(x) as & and
    x's type."""
    if a is None:
        return "-"
    if type(a) in (int, bool):
        return str(int(a))
    if isinstance(a, (int, np.integer)):
        return "%s:%d" % (type(a).__name__, a)
    if isinstance(a, C._Pointer):
        return "*" + CTYPES.get(a._type_, a._type_.__name__)
    if isinstance(a, (C.Array, C._SimpleCData, C.Structure)):
        return type(a).__name__
    if hasattr(a, "_obj"):
        return "&" + CTYPES.get(type(a._obj), type(a._obj).__name__)
    return repr(a)


def shape(x):
    """What a wrapper returned as text: arrays as dtype and shape, containers by element, a dict by sorted key."""
    if isinstance(x, np.ndarray):
        return "%s[%s]" % (x.dtype.name.replace("uint", "u").replace("int", "i").replace("float", "f"), ",".join(str(n) for n in x.shape))
    if isinstance(x, dict):
        return "{%s}" % ", ".join("%s: %s" % (k, shape(v)) for k, v in sorted(x.items()))
    if isinstance(x, (tuple, list)):
        return "(%s)" % ", ".join(shape(v) for v in x)
    if isinstance(x, C.Structure):
        return type(x).__name__
    return repr(x)


class Recorder:
    """Stands where the library would.  A sized call without buffers answers ESIM_ERANGE and n = 3 through its byref argument,
    the one with buffers ESIM_OK (empty=True: ESIM_OK and n = 0 at once); the calls that only report write the scripted numbers."""

    def __init__(self, empty=False, signed=0):
        self.calls, self.empty = [], empty
        self.writes = {"esim_ensemble_members_info": (64, KEPT, 0, signed), "esim_baseline_info": (60, 5), "esim_burden_get": (2, 24, 5, 24, 6),
                       "esim_snapshot_info": (0,)}

    def __getattr__(self, name):
        if not name.startswith("esim_"):
            raise AttributeError(name)

        def call(*args):
            assert args[0] is None, "%s: the context goes first" % name           # (the bare simulator's _ctx)
            self.calls.append("%s(%s)" % (name[5:], ",".join(arg(a) for a in args[1:])))
            refs = [a._obj for a in args if hasattr(a, "_obj") and isinstance(a._obj, C._SimpleCData)]
            if name in SIZED:
                refs[-1].value = 0 if self.empty else 3
                return _lib.ESIM_OK if self.empty or any(isinstance(a, C._Pointer) for a in args) else _lib.ESIM_ERANGE
            for ref, value in zip(refs, self.writes.get(name, ())):
                ref.value = value
            return _lib.ESIM_OK
        return call


class FakePopulation:
    n_citizens, n_areas, n_buildings, n_rooms = 10, 3, 5, 2


def bare_simulator(groups, steps, **script):
    sim = object.__new__(Simulator)
    sim.lib, sim._ctx, sim._steps, sim._n_groups, sim.population = Recorder(**script), None, steps, groups, FakePopulation()
    sim.params = _lib.default_params(max_steps=300, exposed_time=10, infected_time=20)
    sim.statistics_recorder = StatisticsRecorder()
    return sim


def record(groups, steps, chain, **script):
    """The chain of (method, keywords) on one fresh simulator: per link the library calls it made and what came back."""
    sim, out = bare_simulator(groups, steps, **script), []
    for name, kw in chain:
        del sim.lib.calls[:]
        try:
            got = shape(getattr(sim, name)(**kw))
        except Exception as e:                 # (the type is the record; nothing is run behind a link that raised)
            out.append("%s -> raises %s" % (" ".join(sim.lib.calls), type(e).__name__))
            break
        out.append("%s -> %s" % (" ".join(sim.lib.calls), got))
    return " | ".join(out)


def grid(**axes):
    """Every combination of the axes' values as keyword dicts; a value of DEFAULT leaves the keyword out."""
    for values in itertools.product(*axes.values()):
        yield {k: v for k, v in zip(axes, values) if v is not DEFAULT}


DEFAULT = object()
WHERES = ("current", "home", "group", "setting", "all", "areas", _lib.BY_GROUP)       # the five names, one that nobody takes, one code
ROWS = dict(first_step=(0, 1), n_rows=(None, 5))
WINDOW = dict(first_step=(0, 1), last_step=(None, 40))
SETTINGS = (None, "household", ("school", "transport"), 2, "bogus", 9)
STATUS_WHAT = ("susceptible", "infected", "vaccinated", "incidence", "exposures", "bogus", 3)
PROBS = tuple(i / 20 for i in range(21))


def chains():
    """{method: [chain, ...]}: the cases, before the four states of (_n_groups, _steps) multiply them."""
    c = {}

    def add(name, kws, *behind):
        c.setdefault(name, []).extend([(name, kw)] + list(behind) for kw in kws)

    # -- outputs --------------------------------------------------------------------------------------------------------------
    add("area_census", grid(where=WHERES))
    add("area_arrival", grid(where=WHERES))
    add("area_series", grid(what=("infected", "exposures", "bogus", 1), **ROWS))
    add("area_series", [dict(what="infected", stride=0), dict(what="infected", stride=0, n_rows=4), dict(what="infected", stride=7, first_step=3)])
    add("area_status_series", grid(what=("infected",), where=WHERES, **ROWS))
    add("area_status_series", grid(what=STATUS_WHAT, stride=(DEFAULT, 0, 7)))
    add("group_census", [{}])
    add("group_series", grid(what=STATUS_WHAT, **ROWS))
    add("group_series", [dict(what="exposed", stride=0), dict(what="exposed", stride=24)])
    add("setting_series", grid(where=WHERES, **ROWS))
    add("setting_series", grid(settings=SETTINGS, stride=(DEFAULT, 0, 7)))
    add("burden_series", grid(where=WHERES, **ROWS))
    add("burden_series", grid(what=("occupancy", "admissions", "deaths", "bogus", 1), stride=(DEFAULT, 0, 7)))
    add("reproduction_series", grid(where=WHERES, **ROWS))
    add("reproduction_series", [dict(stride=0), dict(stride=7, first_step=3), dict(first_step=-1)])
    for name in ("building_exposures", "offspring", "transmission_ages"):
        add(name, grid(**WINDOW))
    for name in ("mixing_matrix", "area_flows", "area_imports", "event_sizes"):
        add(name, grid(**WINDOW))
        add(name, grid(settings=SETTINGS))
    add("household_sar", grid(where=WHERES, complete=(True, False), **WINDOW))
    add("household_sar", [dict(first_step=80), dict(first_step=80, complete=False), dict(last_step=69), dict(last_step=70), dict(first_step=-1, last_step=5)])
    add("place_sar", grid(where=WHERES, complete=(True, False), **WINDOW))
    add("place_sar", grid(kind=("work", "room", "school", "bogus", 1), where=("all", "group")))
    add("place_sar", [dict(first_step=80), dict(first_step=80, complete=False)])
    add("place_outbreaks", grid(kind=("work", "room", "school", "bogus", 1)))
    add("place_sizes", grid(kind=("work", "room", "school", "bogus", 1)))
    add("contact_hours", grid(where=WHERES, per_case=(False, True), **WINDOW))
    add("contact_hours", grid(settings=SETTINGS))
    add("contact_rates", grid(where=WHERES, **WINDOW))
    add("transmission_events", grid(order=("key", "size", "bogus"), limit=(None, 2, 8)))
    add("transmission_events", grid(order=("key", "size"), **WINDOW))
    add("transmission_events", grid(settings=SETTINGS, min_size=(DEFAULT, 3)))
    add("compare", grid(where=WHERES, citizens=(False, True), **WINDOW))
    add("compare", [dict(first_step=5, last_step=4), dict(first_step=-1)])
    add("compare_series", grid(where=WHERES, cumulative=(False, True), **ROWS))
    add("compare_series", [dict(stride=0), dict(first_step=-1), dict(first_step=61), dict(first_step=60), dict(n_rows=0), dict(stride=7, first_step=3)])
    add("curve_summary", grid(where=WHERES, **WINDOW))
    add("curve_summary", grid(status=("exposed", "infected", "active", "bogus", 2), threshold=(DEFAULT, 5)))
    add("burden_summary", grid(where=WHERES, **WINDOW))
    add("burden_summary", [dict(threshold=5)])
    for name in ("seeds", "exposure_events", "routes", "lineage_areas", "outbreaks", "exposure_settings", "transmission_tree", "transmission_chains",
                 "household_outbreaks", "household_final_sizes", "area_invasion", "burden_outcomes", "burden", "download_state"):
        add(name, [{}])
    add("set_burden", [dict(p_admit=[0.1, 0.2], p_death=[0.01, 0.02], delay_pmf=[0.5, 0.25], stay_pmf=[0.2, 0.2, 0.2])])
    add("set_groups", [dict(labels=[0, 1, 2, 3, 4, 5, 6, 0, 1, 2]), dict(labels=[0] * 10, n_groups=4), dict(labels=None), dict(labels=[0, 1]), dict(labels=[70000] * 10)])
    add("restart", [{}, dict(seed=7), dict(seeds=[1, 2, 3]), dict(seeds=np.arange(4, dtype=np.int64), seed=9), dict(seeds=[-1]), dict(seeds=[[1, 2]]), dict(bogus=1)])
    add("rollback", [{}, dict(seed=7), dict(bogus=1), dict(params=_lib.default_params(seed=3))])

    # -- accumulators: every begin, then its reader and the calls on the members kept, which are sized by what the begin left ---
    def readers(reader, rows=True):
        part = [(reader, dict(first_row=1, n_rows=2))] if rows else []
        return [(reader, {})] + part + [("ensemble_members", dict(first_member=3, n_members=None, first_row=0, n_rows=None)),
                                        ("ensemble_quantiles", dict(probs=(0.5,))), ("ensemble_exceedance", dict(thresholds=(1, 5)))]
    add("ensemble_begin", grid(where=WHERES), *readers("ensemble_read", False))
    add("ensemble_begin", [dict(status_mask=2, min_cases=3)], ("ensemble_fold", {}), ("ensemble_read", {}))
    add("ensemble_begin_arrival", grid(where=WHERES), *readers("ensemble_read", False))
    add("ensemble_begin_arrival", grid(where=("home", "group"), horizon=(None, 50)), ("ensemble_read", {}))
    for name, reader, base in (("ensemble_begin_series", "ensemble_read_series", dict(what="infected")), ("ensemble_begin_settings", "ensemble_read_series", {}),
                               ("ensemble_begin_reproduction", "ensemble_read_reproduction", {}), ("ensemble_begin_paired", "ensemble_read_paired", {})):
        add(name, grid(where=WHERES, **{k: (v,) for k, v in base.items()}), *readers(reader))
        add(name, grid(where=WHERES, **dict(ROWS, **{k: (v,) for k, v in base.items()})), (reader, {}))
    add("ensemble_begin_series", grid(where=("home",), what=STATUS_WHAT, stride=(DEFAULT, 0, 7)), ("ensemble_read_series", {}))
    add("ensemble_begin_series", [dict(where="current", what="exposures", min_cases=3)], ("ensemble_read_series", {}))
    add("ensemble_begin_settings", grid(settings=SETTINGS, stride=(DEFAULT, 0, 7)), ("ensemble_read_series", {}))
    add("ensemble_begin_settings", [dict(min_cases=3)], ("ensemble_read_series", {}))
    add("ensemble_begin_reproduction", grid(stride=(0, 7), min_cohort=(DEFAULT, 2), r=(DEFAULT, (3, 2))), ("ensemble_read_reproduction", {}))
    add("ensemble_begin_paired", [dict(stride=0), dict(first_step=-1), dict(first_step=301), dict(first_step=300), dict(n_rows=0), dict(min_averted=0), dict(min_baseline=-1),
                                  dict(min_baseline=2, min_averted=3, stride=7, cumulative=True)], ("ensemble_read_paired", {}))
    for name, extra in (("ensemble_begin_peaks", {}), ("ensemble_begin_burden_peaks", {})):
        add(name, grid(where=WHERES), *readers("ensemble_read_peaks", False))
        add(name, grid(where=WHERES, **WINDOW), ("ensemble_read_peaks", {}))
        add(name, [dict(threshold=5, min_peak=4)], ("ensemble_read_peaks", {}))
    add("ensemble_begin_peaks", grid(status=("exposed", "infected", "active", "bogus", 2)), ("ensemble_read_peaks", {}))
    for name in ("ensemble_read", "ensemble_read_series", "ensemble_read_reproduction", "ensemble_read_paired", "ensemble_read_peaks", "ensemble_members",
                 "ensemble_members_info", "ensemble_fold"):
        add(name, [{}])                                                             # without any begin: the sizes they fall back to
    add("ensemble_keep_members", grid(capacity=(8,), what=(DEFAULT, "value", "peak_step", "duration", "bogus", 1)))
    add("ensemble_quantiles", grid(probs=(DEFAULT, PROBS, (), (0.5, 1.5)), method=("nearest", "linear", "bogus")))
    add("ensemble_quantiles", [dict(ranks=(3, 1, 2)), dict(ranks=range(20)), dict(probs=PROBS, first_row=0, n_rows=1)])
    add("ensemble_exceedance", [dict(thresholds=range(20)), dict(thresholds=()), dict(thresholds=(1, -2, 3), first_row=0, n_rows=1), dict(thresholds=range(16))])
    return c


def key(groups, steps, chain, script):
    link = chain[0]
    text = "g%d s%d %s" % (groups, steps, ", ".join("%s=%r" % (k, list(v) if isinstance(v, (range, np.ndarray)) else "Params" if isinstance(v, C.Structure) else v)
                                                   for k, v in link[1].items()))
    return text + "".join(" %s=%r" % kv for kv in script.items())


# the sized calls once more against a library with nothing to list, the signed store of the paired kind
SCRIPTS = {"seeds": dict(empty=True), "exposure_events": dict(empty=True), "routes": dict(empty=True), "lineage_areas": dict(empty=True), "outbreaks": dict(empty=True),
           "area_flows": dict(empty=True), "transmission_events": dict(empty=True), "ensemble_members": dict(signed=1), "ensemble_quantiles": dict(signed=1)}


def collect(method=None):
    """{method: {case: record}} of all cases, or of one method's."""
    out = {}
    for name, cases in chains().items():
        if method not in (None, name):
            continue
        scripts = [{}] + ([SCRIPTS[name]] if name in SCRIPTS else [])
        out[name] = {key(g, s, chain, script): record(g, s, chain, **script) for g in (0, 7) for s in (0, 100) for chain in cases for script in scripts}
    return out


def packed(records):
    """{method: {case: record}} as the file holds it: every distinct link of a chain once ("links"), every distinct record as the
    list of its links ("records"), and per method the records of its cases in the order collect() makes them ("cases")."""
    links, chains_, cases = {}, {}, {}
    for method, by_case in records.items():
        cases[method] = [chains_.setdefault(tuple(links.setdefault(l, len(links)) for l in r.split(" | ")), len(chains_)) for r in by_case.values()]
    return {"links": list(links), "records": [list(c) for c in chains_], "cases": cases}


def unpacked(doc):
    """{method: [record, ...]} from the file."""
    records = [" | ".join(doc["links"][i] for i in r) for r in doc["records"]]
    return {method: [records[i] for i in rows] for method, rows in doc["cases"].items()}


def dump(records, path):
    """Writes the file: a link or a method a line."""
    doc = packed(records)
    with open(path, "w") as f:
        f.write('{"links": [\n%s\n],\n"records": %s,\n"cases": {\n%s\n}}\n' % (
            ",\n".join(json.dumps(l) for l in doc["links"]), json.dumps(doc["records"], separators=(",", ":")),
            ",\n".join("%s: %s" % (json.dumps(m), json.dumps(rows, separators=(",", ":"))) for m, rows in sorted(doc["cases"].items()))))


with open(os.path.join(HERE, "marshalling_calls.json")) as _f:
    EXPECTED = unpacked(json.load(_f))


def test_every_method_with_cases_has_records_and_the_other_way_round():
    assert sorted(chains()) == sorted(EXPECTED)


@pytest.mark.parametrize("method", sorted(EXPECTED))
def test_calls_and_returns_are_the_recorded_ones(method):
    got, want = collect(method)[method], EXPECTED[method]
    assert len(got) == len(want)
    wrong = ["%s\n   got  %s\n   want %s" % (k, r, w) for (k, r), w in zip(got.items(), want) if r != w]
    assert not wrong, "%d of %d cases differ:\n%s" % (len(wrong), len(want), "\n".join(wrong[:12]))


