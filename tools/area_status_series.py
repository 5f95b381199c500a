"""Times esim_area_status_series on a preset after its run: every (where, what) table over a 336-row window at the Infected
peak and with stride 24 over the whole run; beside them, alternated in one loop, esim_area_series(ESIM_SERIES_INFECTED) on the
same windows (the existing route to the one table both produce: it must give the same table, or the tool stops), and, for the
last row only, the host route (download_state followed by np.bincount).  Then, in a child process of its own under
`rocprofv3 --kernel-trace --stats`, the device time of the series kernels (esim_kernels_series.h), summed over all those calls.  Prints one JSON line; --out also writes it
to a file (default profiles/area_status_series_<preset>.json).

    python tools/area_status_series.py [preset] [steps] [repeats] [--no-trace] [--out FILE]

Every figure of the first part is wall time around one synchronised library call (perf_counter; the calls end with their own
stream wait), after one warm-up call, as the median of `repeats` calls with the smallest and the largest beside it."""
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

STATUS = ("susceptible", "exposed", "infected", "recovered", "vaccinated")
TABLES = [(where, what) for where in ("home", "current") for what in STATUS] + [("home", "incidence")]
KERNELS = ("k_series_log", "k_series_vax", "k_area_occupancy", "k_series_prefix", "k_area_vax_replay")
TRACE_CALLS = 3


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "repeats": len(ms)}


def timed(fn, repeats):
    fn()
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return out, stats(ms)


def windows(rec):
    peak = int(np.argmax(rec["infected"])) + 1
    w0 = max(1, min(peak - 168, len(rec) - 335))
    return {"window": dict(first_step=w0, n_rows=min(336, len(rec) - w0 + 1), stride=1), "stride24": dict(first_step=1, n_rows=None, stride=24)}


def traced_child(preset, steps):
    """What runs under rocprofv3: the run, then every table TRACE_CALLS times on both windows, and the existing Infected rows."""
    sim = Simulator(Population.synthetic(preset), _lib.default_params(max_steps=max(steps, 5000)))
    rec = sim.run(steps)
    for win in windows(rec).values():
        for where, what in TABLES:
            for _ in range(TRACE_CALLS):
                sim.area_status_series(what, where, **win)
        for _ in range(TRACE_CALLS):
            sim.area_series("infected", **win)
    sim.close()


def trace(preset, steps):
    """Device time per kernel, summed over all traced calls (both windows, every table TRACE_CALLS times)."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "ast", "--",
               sys.executable, os.path.abspath(__file__), preset, str(steps), "--traced-child"]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=1100)
        if p.returncode != 0:
            return {"error": "rocprofv3 run failed (%d): %s" % (p.returncode, (p.stderr or p.stdout)[-400:])}
        f = glob.glob(os.path.join(d, "**", "*_kernel_trace.csv"), recursive=True)
        rows = list(csv.DictReader(open(f[0]))) if f else []
    out = {"calls_per_table_and_window": TRACE_CALLS}
    for name in KERNELS:
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if r.get("Kernel_Name", "").startswith(name)]
        if us:
            out[name] = {"dispatches": len(us), "median_us": round(statistics.median(us), 3), "min_us": round(min(us), 3), "max_us": round(max(us), 3),
                         "total_ms": round(sum(us) / 1e3, 3)}
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
    out = {"preset": a.preset, "n_citizens": pop.n_citizens, "n_areas": pop.n_areas,
           "what": "wall ms around one synchronised call; median (min, max) of `repeats` calls after one warm-up call"}
    if not a.no_trace:
        out["trace"] = trace(a.preset, a.steps)                   # (before this process opens the device)
        print("trace done: %s" % json.dumps(out["trace"]), file=sys.stderr, flush=True)
    sim = Simulator(pop, _lib.default_params(max_steps=max(a.steps, 5000)))
    t0 = time.perf_counter()
    rec = sim.run(a.steps)
    out.update(steps=len(rec), run_ms=round((time.perf_counter() - t0) * 1e3, 2),
               last_record={k: int(rec[k][-1]) for k in STATUS},
               log_entries=int(rec["exposures_building"].sum(dtype=np.int64) + rec["exposures_bus"].sum(dtype=np.int64)) + len(np.unique(pop.seeds)))
    for key, win in windows(rec).items():
        shown = {k: v for k, v in win.items() if v is not None}
        for where, what in TABLES:
            table, t = timed(lambda: sim.area_status_series(what, where, **win), a.repeats)
            t.update(shown, rows=int(table.shape[0]))
            out["%s_%s_%s" % (where, what, key)] = t
        # the existing route to the Infected rows by the area stood in, alternated with the new one in one loop
        want = sim.area_series("infected", **win)
        got = sim.area_status_series("infected", "current", **win)
        if not (got == want).all():
            raise SystemExit("(CURRENT, INFECTED) differs from esim_area_series(ESIM_SERIES_INFECTED) on %s" % shown)
        old_ms, new_ms = [], []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            sim.area_series("infected", **win)
            t1 = time.perf_counter()
            sim.area_status_series("infected", "current", **win)
            old_ms.append((t1 - t0) * 1e3)
            new_ms.append((time.perf_counter() - t1) * 1e3)
        out["alternated_infected_%s" % key] = {"area_series": stats(old_ms), "area_status_series": stats(new_ms),
                                                "area_series_over_area_status_series": round(statistics.median(old_ms) / statistics.median(new_ms), 3)}

    def host_route():
        st = sim.download_state()
        key = pop.building_area[st["current_building"]].astype(np.int64) * 5 + st["status"]
        return np.bincount(key, minlength=pop.n_areas * 5).reshape(pop.n_areas, 5)

    want, t = timed(host_route, max(1, min(a.repeats, 3)))
    out["last_row_download_state_then_bincount_host"] = t
    for k, name in enumerate(STATUS):
        if not (sim.area_status_series(name, "current", first_step=len(rec), n_rows=1)[0] == want[:, k]).all():
            raise SystemExit("the last %s row differs from the downloaded state" % name)
    sim.close()
    path = a.out or os.path.join(ROOT, "profiles", "area_status_series_%s.json" % a.preset)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
