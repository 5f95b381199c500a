"""Runs a preset and reports how its epidemic travels between Output Areas: the ten heaviest flows between different areas
(esim_area_flows), the share of imported cases (esim_area_imports), the depth of the invasion forest (esim_area_invasion) and
the areas every introduction reached (esim_lineage_areas) -- and times the four calls, with esim_mixing_matrix (which shares the
tree replay with them) from the same process beside them as the yardstick.  Prints one JSON line; --out also writes it to a file
(default profiles/area_flows_<preset>.json).

    python tools/area_flows.py [preset] [steps] [repeats] [--out FILE]

Every time is wall time around one synchronised library call (perf_counter; the calls end with their own stream wait), the tree
replay and the copies out included, after one warm-up call, as the median of `repeats` calls with the smallest and the largest
beside it.  The three parts of the pair engine -- insert, compact, sort -- are device times between HIP events that the library
records around them (esim_pair_stats), as shares of the median call."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from epidemicsimulator_amd import Population, Simulator, _lib  # noqa: E402

AGE_EDGES = list(range(5, 95, 5))                  # 19 bands, for the mixing matrix


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "repeats": len(ms)}


def timed(fn, repeats, after=None):
    """(the last result, the times, what `after` returned behind every timed call)."""
    fn()
    ms, extra = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        ms.append((time.perf_counter() - t0) * 1e3)
        if after:
            extra.append(after())
    return out, stats(ms), extra


def engine(parts, call):
    """The pair engine's three parts as medians over the timed calls and as shares of the median call."""
    out = {k: int(parts[-1][k]) for k in ("distinct", "capacity", "dropped")}
    out["fill"] = round(out["distinct"] / out["capacity"], 6)
    for k in ("insert_ms", "compact_ms", "sort_ms"):
        out[k] = round(statistics.median(p[k] for p in parts), 4)
        out[k.replace("_ms", "_share")] = round(out[k] / call["median_ms"], 4)
    return out


def forest_depth(source_area):
    src = source_area.astype(np.int64)
    depth, cur = 0, np.flatnonzero(src != _lib.NO_AREA)
    while cur.size and depth <= src.size:
        depth += 1
        cur = src[cur]
        cur = cur[src[cur] != _lib.NO_AREA]
    return depth


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("preset", nargs="?", default="york")
    ap.add_argument("steps", nargs="?", type=int, default=5000)
    ap.add_argument("repeats", nargs="?", type=int, default=7)
    ap.add_argument("--out")
    a = ap.parse_args()
    pop = Population.synthetic(a.preset)
    labels, n_groups = pop.age_bands(AGE_EDGES)
    out = {"preset": a.preset, "n_citizens": pop.n_citizens, "n_areas": pop.n_areas, "library": os.path.basename(_lib.LIB_PATH),
           "what": "wall ms around one synchronised call; median (min, max) of `repeats` calls after one warm-up call; the engine's parts: device ms between HIP events"}
    sim = Simulator(pop, _lib.default_params(max_steps=max(a.steps, 5000)))
    sim.set_groups(labels, n_groups)
    t0 = time.perf_counter()
    rec = sim.run(a.steps)
    n = len(rec)
    total = int(rec["exposures_building"].sum(dtype=np.int64) + rec["exposures_bus"].sum(dtype=np.int64))
    out.update(steps=n, run_ms=round((time.perf_counter() - t0) * 1e3, 2), log_entries=total + len(sim.seeds()))
    mixing, out["mixing_matrix"], _ = timed(sim.mixing_matrix, a.repeats)           # the yardstick: a table on top of the same tree replay
    # the library call itself, sized for every entry of the log, beside the Python method's two calls (size, then fetch)
    lib, ctx, cap = sim.lib, sim._ctx, total + len(sim.seeds())
    buf, n_out = [np.zeros(cap, np.uint32) for _ in range(3)], C.c_uint32(0)
    ptr = [b.ctypes.data_as(C.POINTER(C.c_uint32)) for b in buf]
    _, out["area_flows_one_call"], parts = timed(lambda: _lib.check(lib.esim_area_flows(ctx, 0xF, 1, n, *ptr, cap, C.byref(n_out)), ctx), a.repeats, sim.pair_stats)
    out["area_flows_engine"] = engine(parts, out["area_flows_one_call"])
    (src, dst, count), out["area_flows"], _ = timed(sim.area_flows, a.repeats)
    imp, out["area_imports"], _ = timed(sim.area_imports, a.repeats)
    inv, out["area_invasion"], _ = timed(sim.area_invasion, a.repeats)
    _, out["lineage_areas_one_call"], parts = timed(lambda: _lib.check(lib.esim_lineage_areas(ctx, *ptr, cap, C.byref(n_out)), ctx), a.repeats, sim.pair_stats)
    out["lineage_areas_engine"] = engine(parts, out["lineage_areas_one_call"])
    (lin, where, cases), out["lineage_areas"], _ = timed(sim.lineage_areas, a.repeats)
    if int(count.sum(dtype=np.int64)) != int(mixing.sum(dtype=np.int64)):
        raise SystemExit("the flows do not add up to the transmissions of the mixing matrix")
    diag = src == dst
    if int(count[diag].sum(dtype=np.int64)) != int(imp["local"].sum(dtype=np.int64)) or int(count[~diag].sum(dtype=np.int64)) != int(imp["imported"].sum(dtype=np.int64)):
        raise SystemExit("the diagonal of the flows is not `local`, or the rest not `imported`")
    if not (inv["step"] == sim.area_arrival("home")).all() or int(cases.sum(dtype=np.int64)) > total + len(sim.seeds()):
        raise SystemExit("the invasion tree disagrees with the arrival times, or the lineages hold more cases than the log")
    off = np.flatnonzero(~diag)
    top = off[np.argsort(count[off], kind="stable")[::-1][:10]]
    imported, local = int(imp["imported"].sum(dtype=np.int64)), int(imp["local"].sum(dtype=np.int64))
    reached = np.bincount(lin, minlength=len(sim.seeds()))
    out.update(distinct_flow_pairs=int(src.size), off_diagonal_pairs=int(off.size), transmissions=imported + local, imported=imported,
               imported_share=round(imported / (imported + local), 5) if imported + local else None,
               heaviest_off_diagonal=[{"src": int(src[i]), "dst": int(dst[i]), "count": int(count[i])} for i in top],
               areas_reached=int((inv["step"] != _lib.NEVER).sum()), areas_with_a_source=int((inv["source_area"] != _lib.NO_AREA).sum()),
               invasion_forest_depth=forest_depth(inv["source_area"]), entry_setting=np.bincount(inv["setting"][inv["setting"] < _lib.N_SETTINGS], minlength=_lib.N_SETTINGS).tolist(),
               lineage_area_pairs=int(lin.size), areas_reached_per_introduction=reached.tolist())
    print("the ten heaviest flows between different areas (of %d distinct pairs, %d off the diagonal):" % (src.size, off.size))
    for i in top:
        print("  area %7d -> %7d: %6d transmissions" % (src[i], dst[i], count[i]))
    print("imported: %d of %d transmissions (%.2f %%); %d areas reached, %d of them from another area; the invasion forest is %d deep"
          % (imported, imported + local, 100.0 * imported / max(1, imported + local), out["areas_reached"], out["areas_with_a_source"], out["invasion_forest_depth"]))
    sim.close()
    path = a.out or os.path.join(ROOT, "profiles", "area_flows_%s.json" % a.preset)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
