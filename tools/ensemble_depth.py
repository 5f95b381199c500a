"""Times the curve-based ensemble statistics on a preset, every figure the wall time (perf_counter) around calls
that end synchronised, as the median of `repeats` repeats after one warm-up, with the smallest and the largest beside it:

  depth   esim_ensemble_depth, and
  band    esim_ensemble_band (the central half, per column and pooled), over 8, 32 and 64 kept members of
            census   the census by home area (one row),
            window   a weekly window by home area (168 rows of the Infected at the national peak),
            burden   the rows of burden_series("occupancy") by all (one column);
  host    beside them the route there was before: ensemble_members() to the host and the numpy restatement of
          tests/_depth_ref.py there, in the same process -- the depths and the central half per column.  It is quadratic in the
          members and linear in the cells: for the window it is timed at 8 members only, and once (--host-window-repeats).
          The tool stops if the two routes differ.

A call's wall time includes the copy of its output to the host (the depth table is 4 B per member and column, the three planes
of the band 12 B per cell), so the device time per kernel comes from runs of their own under `rocprofv3 --kernel-trace --stats`,
one child process per member count over the weekly window, before this process opens the device (--no-trace leaves them out).

The members are `distinct` runs (at most eight, other seeds), each folded several times until the store holds the member count,
as tools/ensemble_quantiles.py fills its store: the kernels' work does not depend on the values apart from the cells they skip.
Repeated members tie everywhere, which the counting rule takes as it takes any tie.  Prints one JSON line; --out also writes it
to a file (default profiles/ensemble_depth_<preset>.json).

    python tools/ensemble_depth.py [preset] [steps] [repeats] [--members 8 32 64] [--host-window-repeats 1] [--no-trace] [--out FILE]"""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _depth_ref as ref  # noqa: E402
from burden_compare import tables  # noqa: E402
from ensemble_quantiles import DISTINCT, MASK, timed, window_of  # noqa: E402
from epidemicsimulator_amd import Population, Simulator, _lib  # noqa: E402

PLANES = ("lo", "hi", "median", "deepest", "n_in")


def begin(sim, kind, window, burden_rows):
    if kind == "census":
        sim.ensemble_begin("home", MASK, 1)
    elif kind == "window":
        sim.ensemble_begin_series("home", "infected", min_cases=1, **window)
    else:
        sim.ensemble_begin_burden_series("all", "occupancy", 1, burden_rows, 24, 1)


def keep_members(sim, kind, window, burden_rows, steps, members):
    begin(sim, kind, window, burden_rows)
    sim.ensemble_keep_members(members)
    distinct = min(members, DISTINCT)
    for k in range(distinct):
        sim.restart(seed=2001 + k)
        sim.run(steps)
        for _ in range(members // distinct + (1 if k < members % distinct else 0)):
            sim.ensemble_fold()
    sim.synchronize()
    assert sim.ensemble_members_info()["kept"] == members


def case(sim, kind, window, burden_rows, steps, members, repeats, host_repeats):
    keep_members(sim, kind, window, burden_rows, steps, members)
    need = -(-members // 2)
    d, d_st = timed(sim.ensemble_depth, repeats)
    b, b_st = timed(lambda: sim.ensemble_band(need=need), repeats)
    _, p_st = timed(lambda: sim.ensemble_band(need=need, pooled=True), repeats)
    rows, cols = b["lo"].shape
    acc = sim.ensemble_read() if kind == "census" else sim.ensemble_read_series()
    out = {"members": members, "rows": rows, "cols": cols, "cells": rows * cols, "cells_some_member_reached": int((acc["sum"] != 0).sum()), "need": need,
           "compares_per_live_cell": 2 * members * int(2 ** np.ceil(np.log2(max(8, members)))),
           "depth": d_st, "band": b_st, "band_pooled": p_st}
    if host_repeats:
        def route():
            stack = sim.ensemble_members()
            return ref.depth(stack), ref.band(stack, need, False)
        (hd, hb), h_st = timed(route, host_repeats)
        if not ((hd == d["depth"]).all() and all((hb[k] == b[k]).all() for k in PLANES)):
            raise SystemExit("the device route and numpy over the members' planes differ (%s, %d members)" % (kind, members))
        out["planes_to_the_host_then_numpy"] = dict(h_st, bytes_over_the_bus=4 * members * rows * cols)
        out["speedup_depth_and_band"] = round(h_st["median_ms"] / (d_st["median_ms"] + b_st["median_ms"]), 2)
    return out


KERNELS = ("k_depth_", "k_members_select")


def setup(preset, steps):
    """(simulator, records, window, rows of the burden series) of a preset with groups and severity tables, run `steps` steps."""
    pop = Population.synthetic(preset)
    labels, n_groups = pop.occupation_groups()
    sim = Simulator(pop, _lib.default_params(max_steps=max(steps, 5000)))
    sim.set_groups(labels, n_groups)
    sim.set_burden(tables(n_groups))
    rec = sim.run(steps)
    return sim, rec, window_of(rec), (len(rec) - 1) // 24 + 1


def traced_child(preset, steps, members):
    """What runs under rocprofv3: the members of the weekly window kept, then three calls of each of the three reads."""
    sim, rec, window, burden_rows = setup(preset, steps)
    keep_members(sim, "window", window, burden_rows, len(rec), members)
    need = -(-members // 2)
    for _ in range(3):
        sim.ensemble_depth()
        sim.ensemble_band(need=need)
        sim.ensemble_band(need=need, pooled=True)
    sim.close()


def trace(preset, steps, members):
    """Device time per kernel of the feature over the weekly window: {kernel: dispatches, median, min and max in microseconds}."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "q", "--",
               sys.executable, os.path.abspath(__file__), preset, str(steps), "--traced-child", str(members)]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if p.returncode != 0:
            return {"error": "rocprofv3 run failed (%d): %s" % (p.returncode, (p.stderr or p.stdout)[-400:])}
        f = glob.glob(os.path.join(d, "**", "*_kernel_trace.csv"), recursive=True)
        rows = list(csv.DictReader(open(f[0]))) if f else []
    out = {}
    for name in KERNELS:
        for full in sorted({r.get("Kernel_Name", "") for r in rows if name in r.get("Kernel_Name", "")}):       # (a template's name starts with "void ")
            us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if r.get("Kernel_Name", "") == full]
            out[full.split("(")[0].replace("void ", "")] = {"dispatches": len(us), "median_us": round(statistics.median(us), 3), "min_us": round(min(us), 3), "max_us": round(max(us), 3)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("preset", nargs="?", default="york")
    ap.add_argument("steps", nargs="?", type=int, default=2000)
    ap.add_argument("repeats", nargs="?", type=int, default=7)
    ap.add_argument("--members", nargs="+", type=int, default=[8, 32, 64])
    ap.add_argument("--host-window-repeats", type=int, default=1, help="repeats of the host route for the weekly window at the smallest member count (0: leave it out)")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--traced-child", type=int, metavar="MEMBERS")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.traced_child:
        return traced_child(a.preset, a.steps, a.traced_child)
    traces = {}
    if not a.no_trace:                                            # (before this process opens the device)
        for members in a.members:
            traces["window_%d_members" % members] = trace(a.preset, a.steps, members)
            print("trace window %d: %s" % (members, json.dumps(traces["window_%d_members" % members])), file=sys.stderr, flush=True)
    sim, rec, window, burden_rows = setup(a.preset, a.steps)
    pop = sim.population
    out = {"preset": a.preset, "n_citizens": pop.n_citizens, "n_areas": pop.n_areas, "steps": len(rec), "window": window, "burden_rows": burden_rows,
           "what": "wall ms around synchronised calls; median (min, max) of `repeats` after one warm-up; the host route: ensemble_members() and tests/_depth_ref.py in numpy"}
    for kind in ("burden", "census", "window"):
        for members in a.members:
            if kind == "window":
                host = a.host_window_repeats if members == min(a.members) else 0
            else:
                host = a.repeats
            key = "%s_%d_members" % (kind, members)
            out[key] = case(sim, kind, window, burden_rows, len(rec), members, a.repeats, host)
            if key in traces:
                out[key]["device_time_per_kernel"] = traces[key]
            print("%s: %s" % (key, json.dumps(out[key])), file=sys.stderr, flush=True)
    sim.close()
    path = a.out or os.path.join(ROOT, "profiles", "ensemble_depth_%s.json" % a.preset)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
