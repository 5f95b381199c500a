"""Times the space-time ensemble on a preset: four members, the Infected rows by household area and by the area stood in,
over a 336-row window at the Infected peak and with stride 24 over the whole run, by two routes alternated in one process:

  (a) what a user did before esim_ensemble_begin_series: area_status_series per member (its rows copied to the host) and a
      numpy fold there;
  (b) ensemble_begin_series once, ensemble_fold per member, followed by synchronize().

The tool stops if the two routes' accumulators differ.  A figure is the wall time (perf_counter) that the four members of one
ensemble spend in the route, the members' runs apart, as the median of `repeats` ensembles after one warm-up ensemble, with the
smallest and the largest beside it.  Per window it also reports the fraction of cells, and of 16-byte pairs of sum / sumsq
cells, that are zero in a member -- what the fold kernel's zero-skip leaves untouched.  Then, in a child process of its own
under `rocprofv3 --kernel-trace --stats`, run once, the device time per kernel of route (b) alone.  Prints one JSON line; --out
also writes it to a file (default profiles/ensemble_series_<preset>.json).

    python tools/ensemble_series.py [preset] [steps] [repeats] [--no-trace] [--out FILE]"""
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

CONFIGS = (("home", "infected"), ("current", "infected"))
MEMBERS = [{"seed": 1001 + k} for k in range(4)]
MIN_CASES = 1
KERNELS = ("k_ensemble_fold_rows", "k_series_log", "k_series_vax", "k_area_occupancy", "k_series_prefix", "k_area_vax_replay")


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "repeats": len(ms)}


def windows(rec):
    peak = int(np.argmax(rec["infected"])) + 1
    w0 = max(1, min(peak - 168, len(rec) - 335))
    return {"window": dict(first_step=w0, n_rows=min(336, len(rec) - w0 + 1), stride=1),
            "stride24": dict(first_step=1, n_rows=(len(rec) - 1) // 24 + 1, stride=24)}


def traced_child(preset, steps):
    """What runs under rocprofv3: per window and configuration one begin and the four members' runs and folds."""
    sim = Simulator(Population.synthetic(preset), _lib.default_params(max_steps=max(steps, 5000)))
    rec = sim.run(steps)
    for win in windows(rec).values():
        for where, what in CONFIGS:
            sim.ensemble_begin_series(where, what, min_cases=MIN_CASES, **win)
            for m in MEMBERS:
                sim.restart(**m)
                sim.run(steps)
                sim.ensemble_fold()
            sim.synchronize()
    sim.close()


def trace(preset, steps):
    """Device time per kernel of route (b), summed over both windows and configurations, and the fold kernel's share of it."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "ens", "--",
               sys.executable, os.path.abspath(__file__), preset, str(steps), "--traced-child"]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=1100)
        if p.returncode != 0:
            return {"error": "rocprofv3 run failed (%d): %s" % (p.returncode, (p.stderr or p.stdout)[-400:])}
        f = glob.glob(os.path.join(d, "**", "*_kernel_trace.csv"), recursive=True)
        rows = list(csv.DictReader(open(f[0]))) if f else []
    out, total = {"folds": len(MEMBERS) * len(CONFIGS) * 2}, 0.0
    for name in KERNELS:
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if r.get("Kernel_Name", "").startswith(name)]
        if us:
            out[name] = {"dispatches": len(us), "median_us": round(statistics.median(us), 3), "min_us": round(min(us), 3), "max_us": round(max(us), 3),
                         "total_ms": round(sum(us) / 1e3, 3)}
            total += sum(us) / 1e3
    if "k_ensemble_fold_rows" in out and total > 0:
        out["fold_kernel_share_of_the_folds_kernel_time"] = round(out["k_ensemble_fold_rows"]["total_ms"] / total, 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("preset", nargs="?", default="york")
    ap.add_argument("steps", nargs="?", type=int, default=5000)
    ap.add_argument("repeats", nargs="?", type=int, default=7)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--traced-child", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.traced_child:
        return traced_child(a.preset, a.steps)
    pop = Population.synthetic(a.preset)
    out = {"preset": a.preset, "n_citizens": pop.n_citizens, "n_areas": pop.n_areas, "members": len(MEMBERS), "min_cases": MIN_CASES,
           "what": "wall ms the four members of one ensemble spend in the route (their runs apart); median (min, max) of `repeats` ensembles after one warm-up ensemble"}
    if not a.no_trace:
        out["trace"] = trace(a.preset, a.steps)                   # (before this process opens the device)
        print("trace done: %s" % json.dumps(out["trace"]), file=sys.stderr, flush=True)
    sim = Simulator(pop, _lib.default_params(max_steps=max(a.steps, 5000)))
    rec = sim.run(a.steps)
    out["steps"] = len(rec)
    for key, win in windows(rec).items():
        for where, what in CONFIGS:
            cells = win["n_rows"] * pop.n_areas
            host_ms, fold_ms, zero_cells, zero_pairs = [], [], [], []
            for rep in range(a.repeats + 1):                      # (the first ensemble is the warm-up, and the one compared)
                hit, tot, sq = np.zeros(cells, np.uint32), np.zeros(cells, np.uint64), np.zeros(cells, np.uint64)
                sim.ensemble_begin_series(where, what, min_cases=MIN_CASES, **win)
                sim.synchronize()
                ta = tb = 0.0
                for m in MEMBERS:
                    sim.restart(**m)
                    sim.run(a.steps)
                    t0 = time.perf_counter()
                    x = sim.area_status_series(what, where, **win).ravel()
                    hit += x >= MIN_CASES
                    x64 = x.astype(np.uint64)
                    tot += x64
                    sq += x64 * x64
                    t1 = time.perf_counter()
                    sim.ensemble_fold()
                    sim.synchronize()
                    t2 = time.perf_counter()
                    ta += t1 - t0
                    tb += t2 - t1
                    if rep == 0:
                        zero_cells.append(float((x == 0).mean()))
                        pairs = x[:cells - cells % 2].reshape(-1, 2)
                        zero_pairs.append(float((~pairs.any(axis=1)).mean()))
                if rep == 0:
                    got = sim.ensemble_read_series()
                    if got["members"] != len(MEMBERS) or not ((got["hit"].ravel() == hit).all() and (got["sum"].ravel() == tot).all() and (got["sumsq"].ravel() == sq).all()):
                        raise SystemExit("the accumulators of ensemble_fold differ from the numpy fold of area_status_series on (%s, %s) %s" % (where, what, win))
                    del got
                else:
                    host_ms.append(ta * 1e3)
                    fold_ms.append(tb * 1e3)
            a_s, b_s = stats(host_ms), stats(fold_ms)
            out["%s_%s_%s" % (where, what, key)] = dict(
                win, cells=cells, series_then_numpy=a_s, ensemble_fold=b_s,
                speedup=round(a_s["median_ms"] / b_s["median_ms"], 2),
                fold_below_by_more_than_the_host_routes_spread=bool(a_s["median_ms"] - b_s["median_ms"] > a_s["max_ms"] - a_s["min_ms"]),
                zero_cell_fraction_per_member=[round(z, 5) for z in zero_cells], zero_pair_fraction_per_member=[round(z, 5) for z in zero_pairs])
            print("%s %s %s: %s" % (where, what, key, json.dumps(out["%s_%s_%s" % (where, what, key)])), file=sys.stderr, flush=True)
    sim.close()
    path = a.out or os.path.join(ROOT, "profiles", "ensemble_series_%s.json" % a.preset)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
