"""Times the ensemble quantile maps on a preset, every figure the wall time (perf_counter) around calls that end
synchronised, as the median of `repeats` repeats after one warm-up, with the smallest and the largest beside it:

  fold       four members folded with and without esim_ensemble_keep_members -- the census by home area, and a weekly window
             (168 rows of the Infected by home area at the national peak); the members' runs apart;
  quantiles  esim_ensemble_quantiles (three ranks) and esim_ensemble_exceedance (two thresholds) over 8, 32 and 64 kept members
             of the census by home area, and over 8 and 32 members of the weekly window; beside them the route there was
             before: every member's plane copied to the host and np.partition over the stack (the window: at 8 members only).
             The tool stops if the two routes differ.

The members of the second part are `distinct` runs (at most eight, other seeds), each folded several times until the store holds
the member count: the kernels' work does not depend on the values apart from the cells they skip, and those are the cells no
member reached.  Per figure the bytes the device route has to move (the planes of the cells not skipped, the accumulator that
decides the skip, the output) and the rate that makes, to set against the 8 TB/s of the memory.  A call's wall time includes
the copy of its output to the host, so the device time per kernel comes from runs of their own under `rocprofv3 --kernel-trace
--stats`, one child process per (kind, member count), before this process opens the device.  Prints one JSON line; --out also
writes it to a file (default profiles/ensemble_quantiles_<preset>.json).

    python tools/ensemble_quantiles.py [preset] [steps] [repeats] [--no-trace] [--out FILE]"""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from epidemicsimulator_amd import Population, Simulator, _lib  # noqa: E402
from epidemicsimulator_amd.simulator import nearest_rank  # noqa: E402

MASK = (1 << _lib.EXPOSED) | (1 << _lib.INFECTED) | (1 << _lib.RECOVERED)
PROBS = (0.05, 0.5, 0.95)
THRESHOLDS = (1, 5)
FOLD_MEMBERS = 4
DISTINCT = 8


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "repeats": len(ms)}


def timed(call, repeats):
    """(the last result, stats of `repeats` calls after one warm-up)."""
    out, ms = call(), []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = call()
        ms.append((time.perf_counter() - t0) * 1e3)
    return out, stats(ms)


def begin(sim, kind, window):
    if kind == "census":
        sim.ensemble_begin("home", MASK, 1)
    else:
        sim.ensemble_begin_series("home", "infected", min_cases=1, **window)


def fold_times(sim, kind, window, steps, repeats, keep):
    ms = []
    for rep in range(repeats + 1):
        begin(sim, kind, window)
        if keep:
            sim.ensemble_keep_members(FOLD_MEMBERS)
        sim.synchronize()
        t = 0.0
        for k in range(FOLD_MEMBERS):
            sim.restart(seed=1001 + k)
            sim.run(steps)
            sim.synchronize()
            t0 = time.perf_counter()
            sim.ensemble_fold()
            sim.synchronize()
            t += time.perf_counter() - t0
        if rep:
            ms.append(t * 1e3)
    return stats(ms)


def keep_members(sim, kind, window, steps, members):
    """`members` members in the store: min(members, DISTINCT) runs, each folded as often as it takes."""
    begin(sim, kind, window)
    sim.ensemble_keep_members(members)
    distinct = min(members, DISTINCT)
    for k in range(distinct):
        sim.restart(seed=2001 + k)
        sim.run(steps)
        for _ in range(members // distinct + (1 if k < members % distinct else 0)):
            sim.ensemble_fold()
    sim.synchronize()
    assert sim.ensemble_members_info()["kept"] == members


def rate(n_bytes, st):
    return {"bytes": int(n_bytes), "GB_per_s_at_the_median": round(n_bytes / (st["median_ms"] * 1e-3) / 1e9, 2)}


def quantile_times(sim, kind, window, steps, members, repeats, host):
    keep_members(sim, kind, window, steps, members)
    ranks = sorted({nearest_rank(p, members) for p in PROBS})
    q, q_st = timed(lambda: sim.ensemble_quantiles(ranks=ranks), repeats)
    e, e_st = timed(lambda: sim.ensemble_exceedance(THRESHOLDS), repeats)
    acc = sim.ensemble_read() if kind == "census" else sim.ensemble_read_series()
    live = int((acc["sum"] != 0).sum())
    cells = int(acc["sum"].size)
    out = {"members": members, "cells": cells, "cells_some_member_reached": live, "ranks": ranks,
           "quantiles": dict(q_st, **rate(4 * members * live + 8 * cells + 4 * len(ranks) * cells, q_st)),
           "exceedance": dict(e_st, **rate(4 * members * live + 8 * cells + 4 * len(THRESHOLDS) * cells, e_st))}
    if host:
        def route():
            stack = sim.ensemble_members()
            return np.partition(stack, ranks, axis=0)[ranks], np.stack([(stack >= t).sum(axis=0) for t in THRESHOLDS])
        (hq, he), h_st = timed(route, repeats)
        if not ((hq == q).all() and (he == e).all()):
            raise SystemExit("the device route and numpy over the members' planes differ (%s, %d members)" % (kind, members))
        out["planes_to_the_host_then_numpy"] = dict(h_st, bytes_over_the_bus=4 * members * cells)
        out["speedup_quantiles_and_exceedance"] = round(h_st["median_ms"] / (q_st["median_ms"] + e_st["median_ms"]), 2)
    return out


CASES = (("census", (8, 32, 64)), ("window", (8, 32)))
KERNELS = ("k_members_select", "k_members_exceed", "k_members_keep")


def window_of(rec):
    peak = int(np.argmax(rec["infected"])) + 1
    w0 = max(1, min(peak - 84, len(rec) - 167))
    return dict(first_step=w0, n_rows=min(168, len(rec) - w0 + 1), stride=1)


def traced_child(preset, steps, kind, members):
    """What runs under rocprofv3: the members of one case kept, then three calls of each of the two reads."""
    sim = Simulator(Population.synthetic(preset), _lib.default_params(max_steps=max(steps, 5000)))
    window = window_of(sim.run(steps))
    keep_members(sim, kind, window, steps, members)
    ranks = sorted({nearest_rank(p, members) for p in PROBS})
    for _ in range(3):
        sim.ensemble_quantiles(ranks=ranks)
        sim.ensemble_exceedance(THRESHOLDS)
    sim.close()


def trace(preset, steps, kind, members):
    """Device time per kernel of the feature in one case: {kernel: dispatches, median, min and max in microseconds}."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "q", "--",
               sys.executable, os.path.abspath(__file__), preset, str(steps), "--traced-child", kind, str(members)]
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
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--traced-child", nargs=2, metavar=("KIND", "MEMBERS"))
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.traced_child:
        return traced_child(a.preset, a.steps, a.traced_child[0], int(a.traced_child[1]))
    traces = {}
    if not a.no_trace:                                            # (before this process opens the device)
        for kind, counts in CASES:
            for members in counts:
                traces["%s_%d_members" % (kind, members)] = trace(a.preset, a.steps, kind, members)
                print("trace %s %d: %s" % (kind, members, json.dumps(traces["%s_%d_members" % (kind, members)])), file=sys.stderr, flush=True)
    pop = Population.synthetic(a.preset)
    out = {"preset": a.preset, "n_citizens": pop.n_citizens, "n_areas": pop.n_areas, "steps": a.steps,
           "what": "wall ms around synchronised calls; median (min, max) of `repeats` after one warm-up"}
    sim = Simulator(pop, _lib.default_params(max_steps=max(a.steps, 5000)))
    rec = sim.run(a.steps)
    window = window_of(rec)
    out["window"] = window
    for kind in ("census", "window"):
        without, with_keep = fold_times(sim, kind, window, a.steps, a.repeats, False), fold_times(sim, kind, window, a.steps, a.repeats, True)
        cells = pop.n_areas * (1 if kind == "census" else window["n_rows"])
        out["fold_%s" % kind] = {"members": FOLD_MEMBERS, "cells": cells, "without_keeping": without, "with_keeping": with_keep,
                                 "kept_bytes_per_member": 4 * cells}
        print("fold %s: %s" % (kind, json.dumps(out["fold_%s" % kind])), file=sys.stderr, flush=True)
    for kind, counts in CASES:
        for members in counts:
            key = "%s_%d_members" % (kind, members)
            out[key] = quantile_times(sim, kind, window, a.steps, members, a.repeats, host=kind == "census" or members == 8)
            if key in traces:
                out[key]["device_time_per_kernel"] = traces[key]
            print("%s: %s" % (key, json.dumps(out[key])), file=sys.stderr, flush=True)
    sim.close()
    path = a.out or os.path.join(ROOT, "profiles", "ensemble_quantiles_%s.json" % a.preset)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
