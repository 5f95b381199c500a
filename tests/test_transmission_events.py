"""Superspreading events, the CPU side: the numpy reference of tests/_event_ref.py is consistent with the transmissions of
tests/_flow_ref.py it was built beside, the worlds `bus` and `spread` hold what they are here for, and the ABI and Python surfaces
of esim_transmission_events and esim_routes are what include/esim.h says."""
import inspect
import os

import numpy as np
import pytest

import _event_ref as event
import _flow_ref as flow
from epidemicsimulator_amd import Simulator, _lib
from epidemicsimulator_amd.ensemble import Ensemble, EventResult
from test_area_flows import MASKS, sort_tile, windows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, S, T = event.H, event.W, event.S, event.T


def key_of(ev):
    return np.stack([ev[k].astype(np.int64) for k in ("step", "setting", "place", "bus")], axis=1)


def ascending(ev):
    k = key_of(ev)
    order = np.lexsort((k[:, 3], k[:, 2], k[:, 1], k[:, 0]))
    return (order == np.arange(len(order))).all() and (len(k) < 2 or (np.diff(k, axis=0) != 0).any(axis=1).all())


@pytest.mark.parametrize("name", flow.ALL_WORLDS)
def test_reference_agrees_with_the_transmissions(name):
    world = event.cached(name)
    pop, ep, n, ref, bus, route_of, table = world
    cap = int(ep.bus_capacity)
    residents = np.bincount(pop.home_building.astype(np.int64), minlength=pop.n_buildings)
    for mask in MASKS:
        for first, last in windows(ref, n):
            who, _, _ = flow.transmissions(ref, pop, mask, first, last)
            ev, tab = event.events(world, mask, first, last), event.sizes(world, mask, first, last)
            assert ascending(ev) and (ev["size"] >= 1).all()
            assert int(ev["size"].sum()) == who.size                                              # every transmission in one event
            assert tab[:, 0].sum() == 0 and tab[:, event.BINS - 1].sum() == 0                     # nothing as large as the last bin here
            per_setting = (tab.astype(np.int64) * np.arange(event.BINS)).sum(axis=1)
            assert (per_setting == np.bincount(ref["setting"][who], minlength=4)[:4]).all()
            assert (tab == np.bincount(ev["setting"].astype(np.int64) * event.BINS + np.minimum(ev["size"], event.BINS - 1),
                                       minlength=4 * event.BINS).reshape(4, event.BINS)).all()    # the table is the list's bincount
            assert ((mask >> ev["setting"].astype(np.int64)) & 1).all() and (ev["step"] >= first).all() and (ev["step"] <= last).all()
            on_bus, at_home = ev["setting"] == T, ev["setting"] == H
            assert (ev["bus"][~on_bus] == 0).all()
            assert (ev["size"][on_bus] <= cap - 1).all()                                          # a bus holds the infector too
            assert (ev["size"][at_home] <= residents[ev["place"][at_home]] - 1).all()
            assert (ev["place"][on_bus] < table["n_riders"].size).all()
            assert (ev["bus"][on_bus] * cap < table["n_riders"][ev["place"][on_bus]]).all()       # a bus that has a first seat
            # the list filtered on the host, and the order by size
            for min_size in (2, int(ev["size"].max(initial=1))):
                keep = ev["size"] >= min_size
                want = event.events(world, mask, first, last, min_size=min_size)
                for k in event.KEYS:
                    assert (want[k] == ev[k][keep]).all(), (k, min_size)
            by_size = event.events(world, mask, first, last, order="size")
            assert (np.diff(by_size["size"].astype(np.int64)) <= 0).all() and int(by_size["size"].sum()) == who.size
            for lo in np.flatnonzero(np.diff(by_size["size"].astype(np.int64)) == 0):           # ties ascend by key
                a, b = key_of(by_size)[lo], key_of(by_size)[lo + 1]
                assert tuple(a) < tuple(b)
    # windows that partition the run add up to the whole, list and table
    cuts = [1, max(2, n // 3), max(3, n // 2 + 1), n + 1]
    whole = event.events(world)
    parts = [event.events(world, flow.ALL, lo, hi - 1) for lo, hi in zip(cuts[:-1], cuts[1:])]
    for k in event.KEYS:
        assert (np.concatenate([p[k] for p in parts]) == whole[k]).all(), k
    assert (sum(event.sizes(world, flow.ALL, lo, hi - 1).astype(np.int64) for lo, hi in zip(cuts[:-1], cuts[1:])) == event.sizes(world)).all()


def test_routes_reference_matches_the_population():
    for name in ("fixture_a", "permuted", "bus", "spread"):
        pop, ep, n, ref, bus, route_of, table = event.cached(name)
        rides = (pop.flags & _lib.FLAG_USES_PUBLIC_TRANSPORT) != 0
        area = pop.building_area.astype(np.int64)
        assert ((route_of >= 0) == rides).all() and int(table["n_riders"].sum()) == int(rides.sum()) and (table["n_riders"] >= 1).all()
        assert (table["home_area"][route_of[rides]] == area[pop.home_building[rides]]).all()
        assert (table["work_area"][route_of[rides]] == area[pop.work_building[rides]]).all()
        pair = table["home_area"].astype(np.int64) * (pop.n_areas + 1) + table["work_area"]
        assert (np.diff(pair) > 0).all()                                                          # ascending by home area, then work area
        assert (np.bincount(route_of[rides], minlength=pair.size) == table["n_riders"]).all()


def bus_situation():
    """What `bus` is here for (the GPU tests call this too): one (route, step) carries more transmissions than a bus holds, and
    they fall on at least three buses -- the precondition that makes the split by bus tested."""
    world = event.cached("bus")
    pop, ep = world[0], world[1]
    cap = int(ep.bus_capacity)
    ev = event.events(world, 1 << T)
    assert ev["size"].size and (ev["bus"] > 0).any()
    pair, per_pair = np.unique(ev["step"].astype(np.int64) * 4096 + ev["place"], return_counts=True)
    total = np.bincount(np.searchsorted(pair, ev["step"].astype(np.int64) * 4096 + ev["place"]), weights=ev["size"]).astype(np.int64)
    top = int(total.argmax())
    assert cap == 20 and total[top] == 55 and total[top] > cap and per_pair[top] >= 3, (cap, total[top], per_pair[top])


def spread_situation():
    """What `spread` is here for: more events than two tiles of the device sort, most of them of one transmission, the largest
    in a school room."""
    world = event.cached("spread")
    ev = event.events(world)
    assert int(ev["size"].sum()) == 14119 and ev["size"].size >= 8776 and ev["size"].size > 2 * sort_tile()
    top = event.events(world, order="size")
    assert int(top["size"][0]) == 27 and int(top["setting"][0]) == S and int((ev["size"] == 1).sum()) >= 7808
    assert int(event.events(world, min_size=2)["size"].size) < ev["size"].size // 4                # what min_size = 2 saves


def test_bus_splits_one_route_and_step_into_at_least_three_buses():
    bus_situation()


def test_spread_has_more_events_than_two_sort_tiles():
    spread_situation()


def test_school_world_has_at_least_2063_events():
    world = event.cached("school")
    ev = event.events(world)
    assert int(ev["size"].sum()) == 2970 and ev["size"].size >= 2063


def test_abi_surface():
    text = open(os.path.join(ROOT, "include", "esim.h")).read()
    assert "#define ESIM_EVENT_BINS 256" in text and _lib.EVENT_BINS == event.BINS == 256
    assert "enum { ESIM_EVENTS_BY_KEY = 0, ESIM_EVENTS_BY_SIZE = 1 };" in text and (_lib.EVENTS_BY_KEY, _lib.EVENTS_BY_SIZE) == (0, 1)
    for decl in ("int  esim_transmission_events(esim_ctx *ctx, uint32_t setting_mask, uint32_t first_step, uint32_t last_step, uint32_t min_size, int order,",
                 "uint32_t *step, uint8_t *setting, uint32_t *place, uint32_t *bus, uint32_t *size /* [cap] each, any may be NULL */,",
                 "uint32_t cap, uint32_t *n_out, uint32_t *sizes /* [ESIM_N_SETTINGS * ESIM_EVENT_BINS] or NULL */);",
                 "int  esim_routes(esim_ctx *ctx, uint32_t *home_area, uint32_t *work_area, uint32_t *n_riders /* [cap] each, any may be NULL */, uint32_t cap, uint32_t *n_out);"):
        assert decl in text
    assert "esim_transmission_events" in open(os.path.join(ROOT, "README.md")).read()
    lib = _lib.load()
    for name in ("esim_transmission_events", "esim_routes"):
        assert name in _lib.SYMBOLS and getattr(lib, name).restype is not None
    # a null context is refused before anything touches a device
    assert lib.esim_transmission_events(None, 0xF, 1, 1, 1, 0, None, None, None, None, None, 0, None, None) == -1
    assert lib.esim_routes(None, None, None, None, 0, None) == -1


def test_python_surface(tmp_path):
    def defaults(f):
        return {k: p.default for k, p in inspect.signature(f).parameters.items() if p.default is not inspect.Parameter.empty}
    assert defaults(Simulator.transmission_events) == dict(settings=None, first_step=1, last_step=None, min_size=1, order="key", limit=None)
    assert defaults(Simulator.event_sizes) == dict(settings=None, first_step=1, last_step=None) and defaults(Simulator.routes) == {}
    assert list(inspect.signature(Ensemble.events).parameters) == ["self", "members", "n_steps", "settings", "first_step", "last_step", "top"]
    assert defaults(Ensemble.events) == dict(settings=None, first_step=1, last_step=None, top=16)
    # neither run() nor forecast() gained a keyword
    assert list(inspect.signature(Ensemble.run).parameters)[-2:] == ["settings", "reproduction"]
    assert list(inspect.signature(Ensemble.forecast).parameters)[-2:] == ["settings", "reproduction"]
    # a hand-made result: two members, top 3
    sizes = [np.zeros((4, 256), np.uint32), np.zeros((4, 256), np.uint32)]
    sizes[0][H, 1], sizes[0][H, 2], sizes[0][S, 5], sizes[1][T, 1] = 6, 2, 1, 4                    # member 0: 10 at home, 4 of them in events >= 2
    tops = [dict(step=np.array([30, 12], np.uint32), setting=np.array([S, H], np.uint8), place=np.array([3, 40], np.uint32), bus=np.array([0, 0], np.uint32),
                 size=np.array([5, 2], np.uint32)),
            dict(step=np.array([7, 8, 9], np.uint32), setting=np.array([T, T, T], np.uint8), place=np.array([1, 1, 2], np.uint32), bus=np.array([0, 2, 0], np.uint32),
                 size=np.array([1, 1, 1], np.uint32))]
    res = EventResult.gathered([{"seed": 1}, {"seed": 2}], sizes, tops, 3)
    assert res.members == [{"seed": 1}, {"seed": 2}] and res.sizes.shape == (2, 4, 256) and res.sizes.dtype == np.uint32
    for k in event.KEYS:
        assert getattr(res, k).shape == (2, 3) and getattr(res, k).dtype == np.uint32
    assert res.step[0].tolist() == [30, 12, _lib.NEVER] and res.size[0, 2] == _lib.NEVER and res.bus[1].tolist() == [0, 2, 0] and res.setting[0, 0] == S
    share = res.share_in_events(2)
    assert share.shape == (2, 4) and share[0, H] == 4 / 10 and share[0, S] == 1.0 and np.isnan(share[0, W]) and share[1, T] == 0.0
    assert (res.share_in_events(1)[~np.isnan(share)] == 1.0).all()
    res.dump(str(tmp_path))
    got = np.load(tmp_path / "ensemble_events.npz")
    assert (got["sizes"] == res.sizes).all()
    for k in event.KEYS:
        assert (got[k] == getattr(res, k)).all()
    none = EventResult.gathered([], [], [], 4)
    assert none.sizes.shape == (0, 4, 256) and none.step.shape == (0, 4)
    with pytest.raises(ValueError):
        Simulator.transmission_events(None, order="place")
