"""Times the read-backs by citizen group on a preset after its run: esim_group_census at 19 five-year age bands and at 1024
groups, beside esim_area_census(HOME) (its device-side peer) and the host route to the same table (download_state followed
by np.bincount by label) in the same process; esim_group_series, all six kinds, over a 336-step window at the Infected peak
and with stride 24 over the whole run.  Then, in a child process of its own under `rocprofv3 --kernel-trace --stats`, the
device time of k_group_census against its byte model (6 B per citizen).  Prints one JSON line; --out also writes it to a file.

    python tools/group_outputs.py [preset] [steps] [repeats] [--no-trace] [--out FILE]

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

HBM_PEAK = 8.0e12
KINDS = ("susceptible", "exposed", "infected", "recovered", "vaccinated", "exposures")
TRACE_CALLS = 8


def timed(fn, repeats):
    fn()
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return out, {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "repeats": repeats}


def labels_of(pop):
    bands, n_bands = pop.age_bands(np.arange(5, 95, 5))
    return bands, n_bands, (np.arange(pop.n_citizens) % _lib.MAX_GROUPS).astype(np.uint16)


def traced_child(preset, steps):
    """What runs under rocprofv3: the run, then TRACE_CALLS censuses at 19 groups and TRACE_CALLS at 1024."""
    pop = Population.synthetic(preset)
    bands, n_bands, many = labels_of(pop)
    sim = Simulator(pop, _lib.default_params(max_steps=max(steps, 5000)))
    sim.run(steps)
    for lab, n in ((bands, n_bands), (many, _lib.MAX_GROUPS)):
        sim.set_groups(lab, n)
        for _ in range(TRACE_CALLS):
            sim.group_census()
    sim.close()


def trace(preset, steps, n_citizens):
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "grp", "--",
               sys.executable, os.path.abspath(__file__), preset, str(steps), "--traced-child"]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=1100)
        if p.returncode != 0:
            return {"error": "rocprofv3 run failed (%d): %s" % (p.returncode, (p.stderr or p.stdout)[-400:])}
        f = glob.glob(os.path.join(d, "**", "*_kernel_trace.csv"), recursive=True)
        rows = list(csv.DictReader(open(f[0]))) if f else []
    out = {"model_bytes": 6 * n_citizens}
    for name in ("k_group_census", "k_group_finish"):
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
              for r in sorted(rows, key=lambda r: int(r["Start_Timestamp"])) if r.get("Kernel_Name", "").startswith(name)]
        if len(us) != 2 * TRACE_CALLS:
            out[name] = {"error": "%d dispatches in the trace, expected %d" % (len(us), 2 * TRACE_CALLS)}
            continue
        for key, part in (("19_groups", us[1:TRACE_CALLS]), ("1024_groups", us[TRACE_CALLS + 1:])):   # (each first call: warm-up)
            e = {"median_us": round(statistics.median(part), 3), "min_us": round(min(part), 3), "max_us": round(max(part), 3), "calls": len(part)}
            if name == "k_group_census":
                e["frac_hbm_peak"] = round(6 * n_citizens / (e["median_us"] * 1e-6) / HBM_PEAK, 4)
            out.setdefault(name, {})[key] = e
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
    n = pop.n_citizens
    out = {"preset": a.preset, "n_citizens": n, "n_areas": pop.n_areas,
           "what": "wall ms around one synchronised call; median (min, max) of `repeats` calls after one warm-up call"}
    if not a.no_trace:
        out["trace"] = trace(a.preset, a.steps, n)                # (before this process opens the device)
        print("trace done: %s" % json.dumps(out["trace"]), file=sys.stderr, flush=True)
    bands, n_bands, many = labels_of(pop)
    sim = Simulator(pop, _lib.default_params(max_steps=max(a.steps, 5000)))
    t0 = time.perf_counter()
    rec = sim.run(a.steps)
    out.update(steps=len(rec), run_ms=round((time.perf_counter() - t0) * 1e3, 2),
               last_record={k: int(rec[k][-1]) for k in ("susceptible", "exposed", "infected", "recovered", "vaccinated")},
               log_entries=int(rec["exposures_building"].sum(dtype=np.int64) + rec["exposures_bus"].sum(dtype=np.int64)) + len(np.unique(pop.seeds)),
               added_device_bytes={"19_groups": 2 * n + 24 * n_bands, "1024_groups": 2 * n + 24 * _lib.MAX_GROUPS})
    t0 = time.perf_counter()
    sim.set_groups(bands, n_bands)
    out["set_groups_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    table, t = timed(sim.group_census, a.repeats)
    t.update(model_bytes=6 * n, frac_hbm_peak_whole_call=round(6 * n / (t["median_ms"] * 1e-3) / HBM_PEAK, 4))
    out["group_census_19"] = t
    home, t = timed(lambda: sim.area_census("home"), a.repeats)
    out["area_census_home"] = t
    assert (table.sum(axis=0) == home.sum(axis=0)).all()

    def host_route():
        status = sim.download_state()["status"]
        return np.bincount(bands.astype(np.int64) * 5 + status, minlength=n_bands * 5).reshape(n_bands, 5)

    want, t = timed(host_route, max(1, min(a.repeats, 3)))
    assert (table == want).all()
    out["download_state_then_bincount_host"] = t
    out["group_census_19_speedup_vs_host"] = round(t["median_ms"] / out["group_census_19"]["median_ms"], 1)
    out["group_census_19_vs_area_census_home"] = round(out["group_census_19"]["median_ms"] / out["area_census_home"]["median_ms"], 3)
    peak = int(np.argmax(rec["infected"])) + 1
    w0 = max(1, min(peak - 168, len(rec) - 335))
    w_rows = min(336, len(rec) - w0 + 1)
    for what in KINDS:
        _, t = timed(lambda: sim.group_series(what, first_step=w0, n_rows=w_rows, stride=1), a.repeats)
        t.update(first_step=w0, n_rows=w_rows)
        out["series_%s_window" % what] = t
        _, t = timed(lambda: sim.group_series(what, stride=24), a.repeats)
        out["series_%s_stride24" % what] = t
    sim.set_groups(many, _lib.MAX_GROUPS)
    table, t = timed(sim.group_census, a.repeats)
    t.update(model_bytes=6 * n, frac_hbm_peak_whole_call=round(6 * n / (t["median_ms"] * 1e-3) / HBM_PEAK, 4))
    out["group_census_1024"] = t
    assert (table.sum(axis=0) == home.sum(axis=0)).all()
    sim.close()
    line = json.dumps(out)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    print(line)


if __name__ == "__main__":
    main()
