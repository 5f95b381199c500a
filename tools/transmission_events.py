"""Runs a preset and reports its superspreading events (esim_transmission_events): the size distribution per setting, the share of
transmission in events of at least 2, 5 and 10 infections, the sixteen largest events -- and times the call in its three uses
(the size table alone, the list by key at min_size 1 and 2, the top 16 by size), with esim_area_flows into a buffer sized for
every entry of the log (which shares the whole replay) from the same process beside them as the yardstick.  Prints one JSON line;
--out also writes it to a file (default profiles/transmission_events_<preset>.json).

    python tools/transmission_events.py [preset] [steps] [repeats] [--out FILE]

Every time is wall time around one synchronised library call (perf_counter; the calls end with their own stream wait), the tree
replay and the copies out included, after one warm-up call, as the median of `repeats` calls with the smallest and the largest
beside it.  The three parts of the pair engine -- insert, compact, sort (for the events: both sorts and the split into arrays) --
are device times between HIP events that the library records around them (esim_pair_stats), as shares of the median call."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from epidemicsimulator_amd import Population, Simulator, _lib  # noqa: E402
from area_flows import engine, timed  # noqa: E402

KEYS = ("step", "setting", "place", "bus", "size")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("preset", nargs="?", default="york")
    ap.add_argument("steps", nargs="?", type=int, default=5000)
    ap.add_argument("repeats", nargs="?", type=int, default=7)
    ap.add_argument("--out")
    a = ap.parse_args()
    pop = Population.synthetic(a.preset)
    out = {"preset": a.preset, "n_citizens": pop.n_citizens, "n_buildings": pop.n_buildings, "library": os.path.basename(_lib.LIB_PATH),
           "what": "wall ms around one synchronised call; median (min, max) of `repeats` calls after one warm-up call; the engine's parts: device ms between HIP events"}
    sim = Simulator(pop, _lib.default_params(max_steps=max(a.steps, 5000)))
    t0 = time.perf_counter()
    rec = sim.run(a.steps)
    n = len(rec)
    total = int(rec["exposures_building"].sum(dtype=np.int64) + rec["exposures_bus"].sum(dtype=np.int64))
    lib, ctx, cap = sim.lib, sim._ctx, total + len(sim.seeds())
    out.update(steps=n, run_ms=round((time.perf_counter() - t0) * 1e3, 2), log_entries=cap)
    u32p, n_out = C.POINTER(C.c_uint32), C.c_uint32(0)
    buf = {k: np.zeros(cap, np.uint8 if k == "setting" else np.uint32) for k in KEYS}
    ptr = [buf[k].ctypes.data_as(C.POINTER(C.c_uint8) if k == "setting" else u32p) for k in KEYS]
    sizes = np.zeros((_lib.N_SETTINGS, _lib.EVENT_BINS), np.uint32)

    def events(min_size, order, lists, n_cap, table):
        _lib.check(lib.esim_transmission_events(ctx, 0xF, 1, n, min_size, order, *(ptr if lists else [None] * 5), n_cap, C.byref(n_out),
                                                sizes.ctypes.data_as(u32p) if table else None), ctx)
        return n_out.value
    # the yardstick: the flows into a buffer sized for every entry of the log -- the same replay, one sort
    flow_ptr = [buf[k].ctypes.data_as(u32p) for k in ("step", "place", "bus")]
    _, out["area_flows_one_call"], parts = timed(lambda: _lib.check(lib.esim_area_flows(ctx, 0xF, 1, n, *flow_ptr, cap, C.byref(n_out)), ctx), a.repeats, sim.pair_stats)
    out["area_flows_engine"] = engine(parts, out["area_flows_one_call"])
    n_events, out["sizes_alone"], parts = timed(lambda: events(1, _lib.EVENTS_BY_SIZE, False, 0, True), a.repeats, sim.pair_stats)
    out["sizes_alone_engine"] = engine(parts, out["sizes_alone"])
    table = sizes.copy()
    for min_size in (1, 2):
        k = "by_key_min_size_%d" % min_size
        out[k + "_events"], out[k], parts = timed(lambda: events(min_size, _lib.EVENTS_BY_KEY, True, cap, False), a.repeats, sim.pair_stats)
        out[k + "_engine"] = engine(parts, out[k])
        if min_size == 1:
            by_key = {j: buf[j][:out[k + "_events"]].copy() for j in KEYS}
    _, out["top_16_by_size"], parts = timed(lambda: events(1, _lib.EVENTS_BY_SIZE, True, 16, False), a.repeats, sim.pair_stats)
    out["top_16_by_size_engine"] = engine(parts, out["top_16_by_size"])
    top = {j: buf[j][:min(16, n_events)].copy() for j in KEYS}
    # what the outputs say, and that they agree with each other
    want = np.bincount(by_key["setting"].astype(np.int64) * _lib.EVENT_BINS + np.minimum(by_key["size"], _lib.EVENT_BINS - 1), minlength=table.size).reshape(table.shape)
    if n_events != by_key["size"].size or not (table == want).all():
        raise SystemExit("the size table is not the bincount of the list")
    if top["size"].size and (int(top["size"][0]) != int(by_key["size"].max()) or (np.diff(top["size"].astype(np.int64)) > 0).any()):
        raise SystemExit("the top of the order by size is not the largest event of the list")
    transmissions = int(by_key["size"].sum(dtype=np.int64))
    routes = sim.routes()
    share = {str(k): round(int(by_key["size"][by_key["size"] >= k].sum(dtype=np.int64)) / transmissions, 5) if transmissions else None for k in (2, 5, 10)}
    out.update(events=n_events, transmissions=transmissions, events_of_size_1=int((by_key["size"] == 1).sum()), largest_event=int(by_key["size"].max(initial=0)),
               events_per_setting=table.sum(axis=1).tolist(), largest_per_setting=[int(np.flatnonzero(r).max(initial=0)) for r in table],
               share_of_transmission_in_events_of_at_least=share, n_routes=int(routes["n_riders"].size),
               largest=[{j: int(top[j][i]) for j in KEYS} for i in range(top["size"].size)])
    print("%d events over %d transmissions, %d of them of one transmission; the largest:" % (n_events, transmissions, out["events_of_size_1"]))
    for e in out["largest"]:
        where = "route %d (area %d -> %d), bus %d" % (e["place"], routes["home_area"][e["place"]], routes["work_area"][e["place"]], e["bus"]) if e["setting"] == _lib.SETTING_TRANSPORT \
            else "%s %d" % ("room" if e["setting"] == _lib.SETTING_SCHOOL else "building", e["place"])
        print("  step %5d  %-10s %-40s %4d transmissions" % (e["step"], _lib.SETTING_NAMES[e["setting"]], where, e["size"]))
    sim.close()
    path = a.out or os.path.join(ROOT, "profiles", "transmission_events_%s.json" % a.preset)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
