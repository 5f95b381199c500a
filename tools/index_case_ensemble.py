"""Times what an ensemble over the index cases adds on a preset: esim_restart_seeded beside esim_restart, esim_area_arrival beside
the host route (esim_download_exposure_log + numpy.minimum.at), and esim_ensemble_fold for the arrival kind beside the census
kind.  Writes profiles/index_case_ensemble_<preset>.json and prints it as one JSON line.

    python tools/index_case_ensemble.py PRESET [--steps N] [--no-trace]

Every wall figure is perf_counter around calls of the C ABI that end in esim_synchronize or in the call's own wait, after a
warm-up round, as the median of the repeats with the smallest and the largest beside it; what is compared alternates in one
loop of one process.  Unless --no-trace, a child process of its own then runs the arrival call and the arrival fold under
`rocprofv3 --kernel-trace --stats`: the kernels' device time against the byte model of k_area_arrival (4 B per log entry plus
two dependent 4 B gathers: household, area).  The atomics of k_area_arrival are not counted."""
import argparse
import csv
import ctypes as C
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
KERNELS = ("k_area_arrival", "k_ensemble_fold_arrival", "k_ensemble_fold", "k_area_census", "k_restart_words", "k_restart_books")
RESTART_REPEATS, ARRIVAL_REPEATS = 9, 7


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "repeats": len(ms)}


def clock(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def traced_child(preset, steps):
    """What runs under rocprofv3: an upload, the run, then the arrival call and the arrival fold ARRIVAL_REPEATS times each."""
    pop = Population.synthetic(preset)
    sim = Simulator(pop, _lib.default_params(max_steps=steps))
    sim.run(steps)
    sim.ensemble_begin_arrival("home")
    for _ in range(ARRIVAL_REPEATS):
        sim.area_arrival("home")
        sim.ensemble_fold()
        sim.synchronize()
    print("log_len %d" % sim.debug_counters()["log_len"])
    sim.close()


def trace(preset, steps):
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "arr", "--",
               sys.executable, os.path.abspath(__file__), preset, "--steps", str(steps), "--traced-child"]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if p.returncode != 0:
            return {"error": "rocprofv3 run failed (%d): %s" % (p.returncode, (p.stderr or p.stdout)[-400:])}
        kernels = {}
        for f in glob.glob(os.path.join(d, "**", "*_kernel_stats.csv"), recursive=True)[:1]:
            for r in csv.DictReader(open(f)):
                name = r["Name"].split("(")[0]
                if name in KERNELS:
                    kernels[name] = {"calls": int(r["Calls"]), "mean_us": round(float(r["AverageNs"]) / 1e3, 3), "min_us": round(float(r["MinNs"]) / 1e3, 3),
                                     "max_us": round(float(r["MaxNs"]) / 1e3, 3)}
        out = {"kernels": kernels}
        for line in p.stdout.splitlines():
            if line.startswith("log_len "):
                out["log_len"] = int(line.split()[1])
        if "k_area_arrival" in kernels and "log_len" in out:
            model = 12 * out["log_len"]
            s = kernels["k_area_arrival"]["mean_us"] * 1e-6
            out["k_area_arrival_model_bytes"] = model
            out["k_area_arrival_model_us_at_hbm_peak"] = round(model / HBM_PEAK * 1e6, 4)
            out["k_area_arrival_frac_of_model_rate"] = round(model / s / HBM_PEAK, 5)
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("preset")
    ap.add_argument("--steps", type=int, default=5000)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--traced-child", action="store_true")
    a = ap.parse_args()
    if a.traced_child:
        return traced_child(a.preset, a.steps)
    out = {"preset": a.preset, "steps": a.steps,
           "what": "wall ms around C ABI calls ending in esim_synchronize or in the call's own wait; median (min, max) after a warm-up round; the compared calls alternate in one loop"}
    if not a.no_trace:
        out["trace"] = trace(a.preset, a.steps)                   # (before this process opens the device)
        print("trace done: %s" % json.dumps(out["trace"]), file=sys.stderr, flush=True)
    pop = Population.synthetic(a.preset)
    out.update(n_citizens=pop.n_citizens, n_areas=pop.n_areas)
    sim = Simulator(pop, _lib.default_params(max_steps=a.steps))
    lib, ctx, p = sim.lib, sim._ctx, sim.params
    u32p = C.POINTER(C.c_uint32)
    ok = lambda rc: _lib.check(rc, ctx)
    sync = lambda: ok(lib.esim_synchronize(ctx))
    lists = {n: np.ascontiguousarray(pop.draw_index_cases(n, 1), np.uint32) for n in (10, 10000)}
    seeded = lambda n: ok(lib.esim_restart_seeded(ctx, C.byref(p), lists[n].ctypes.data_as(u32p), lists[n].size))

    # ---- 1. going back to step 0: plain, with 10 and with 10 000 index cases
    t = {"restart": [], "seeded_10": [], "seeded_10000": []}
    for i in range(RESTART_REPEATS + 1):
        row = {"restart": clock(lambda: (ok(lib.esim_restart(ctx, C.byref(p))), sync())),
               "seeded_10": clock(lambda: (seeded(10), sync())),
               "seeded_10000": clock(lambda: (seeded(10000), sync()))}
        if i:                                                      # round 0 warms up (and grows the device list once)
            for k, v in row.items():
                t[k].append(v)
    out["esim_restart_sync"] = summary(t["restart"])
    out["esim_restart_seeded_10_sync"] = summary(t["seeded_10"])
    out["esim_restart_seeded_10000_sync"] = summary(t["seeded_10000"])
    out["distinct_seeds"] = {str(n): int(np.unique(v).size) for n, v in lists.items()}

    # ---- 2. the arrival map after the run: on the device, and by the host route
    sim.restart(seeds=pop.seeds)
    sim.run(a.steps)
    home = pop.building_area[pop.home_building]
    table = np.zeros(pop.n_areas, np.uint32)
    n_log = C.c_uint32(0)
    lib.esim_download_exposure_log(ctx, None, None, None, 0, C.byref(n_log))
    cit, step, bus = np.zeros(n_log.value, np.uint32), np.zeros(n_log.value, np.uint32), np.zeros(n_log.value, np.uint8)
    host = np.zeros(pop.n_areas, np.uint32)

    def host_route():
        ok(lib.esim_download_exposure_log(ctx, cit.ctypes.data_as(u32p), step.ctypes.data_as(u32p), bus.ctypes.data_as(C.POINTER(C.c_uint8)), n_log.value, C.byref(n_log)))
        host[:] = _lib.NEVER
        np.minimum.at(host, home[cit], step)
        host[home[sim.seeds()]] = 0

    t = {"device": [], "host": []}
    for i in range(ARRIVAL_REPEATS + 1):
        row = {"device": clock(lambda: ok(lib.esim_area_arrival(ctx, _lib.AREA_HOME, table.ctypes.data_as(u32p)))), "host": clock(host_route)}
        if i:
            for k, v in row.items():
                t[k].append(v)
    if not (table == host).all():
        raise SystemExit("esim_area_arrival differs from the host route")
    out["exposure_log_entries"] = int(n_log.value)
    out["areas_reached"] = int((table != _lib.NEVER).sum())
    out["esim_area_arrival_call"] = summary(t["device"])
    out["download_exposure_log_plus_numpy"] = summary(t["host"])
    out["host_route_vs_call"] = round(out["download_exposure_log_plus_numpy"]["median_ms"] / out["esim_area_arrival_call"]["median_ms"], 1)

    # ---- 3. the fold of both kinds
    t = {"arrival": [], "census": []}
    for i in range(ARRIVAL_REPEATS + 1):
        sim.ensemble_begin_arrival("home"); sync()
        row = {"arrival": clock(lambda: (ok(lib.esim_ensemble_fold(ctx)), sync()))}
        sim.ensemble_begin("home"); sync()
        row["census"] = clock(lambda: (ok(lib.esim_ensemble_fold(ctx)), sync()))
        if i:
            for k, v in row.items():
                t[k].append(v)
    out["esim_ensemble_fold_arrival_sync"] = summary(t["arrival"])
    out["esim_ensemble_fold_census_sync"] = summary(t["census"])
    sim.close()
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "index_case_ensemble_%s.json" % a.preset), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
