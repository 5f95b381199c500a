"""Times the per-Output-Area read-backs on a preset after its run: esim_area_census (CURRENT, HOME) and esim_area_series
(both kinds: stride 1 over a 336-step window at the Infected peak, stride 24 over the whole run), beside the host routes to
the same tables, infected_per_area() and exposures_per_output_area(), in the same process.  Prints one JSON line.

    python tools/area_outputs.py [preset] [steps] [repeats]

Every figure is wall time around one synchronised library call (perf_counter; the calls end with their own stream wait), after
one warm-up call, as the median of `repeats` calls with the smallest and the largest beside it."""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from epidemicsimulator_amd import Population, Simulator, _lib  # noqa: E402

HBM_PEAK = 8.0e12


def timed(fn, repeats):
    fn()
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return out, {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "repeats": repeats}


def main():
    preset = sys.argv[1] if len(sys.argv) > 1 else "york"
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 5000
    repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 7
    pop = Population.synthetic(preset)
    sim = Simulator(pop, _lib.default_params(max_steps=max(steps, 5000)))
    t0 = time.perf_counter()
    rec = sim.run(steps)
    run_ms = (time.perf_counter() - t0) * 1e3
    n, n_log = pop.n_citizens, int(rec["exposures_building"].sum(dtype=np.int64) + rec["exposures_bus"].sum(dtype=np.int64)) + len(np.unique(pop.seeds))
    out = {"preset": preset, "steps": len(rec), "n_citizens": n, "n_areas": pop.n_areas, "n_buildings": pop.n_buildings,
           "log_entries": n_log, "run_ms": round(run_ms, 2),
           "added_device_bytes": 4 * pop.n_buildings + 4 * 5 * pop.n_areas}
    dbg = sim.debug_counters()
    has_work = pop.work_building != pop.home_building
    for where in ("current", "home"):
        table, t = timed(lambda: sim.area_census(where), repeats)
        # what the pass must read by its own model: the word and the home id of everybody, the work id of those at work,
        # one building_area entry per building met (citizens of a building sit next to each other)
        at_work = int(has_work.sum()) if (where == "current" and dbg["at_work"]) else 0
        model = 8 * n + 4 * at_work + 4 * pop.n_buildings
        t.update(model_bytes=model, frac_hbm_peak=round(model / (t["median_ms"] * 1e-3) / HBM_PEAK, 4))
        out["census_" + where] = t
        if where == "current":
            want, th = timed(sim.infected_per_area, max(1, min(repeats, 3)))
            assert (table[:, _lib.INFECTED] == want).all()
            out["infected_per_area_host"] = th
            out["census_current_speedup_vs_host"] = round(th["median_ms"] / t["median_ms"], 1)
    peak = int(np.argmax(rec["infected"])) + 1
    w0 = max(1, min(peak - 168, len(rec) - 335))
    w_rows = min(336, len(rec) - w0 + 1)
    for what in ("infected", "exposures"):
        _, t = timed(lambda: sim.area_series(what, first_step=w0, n_rows=w_rows, stride=1), repeats)
        t.update(first_step=w0, n_rows=w_rows, log_entries_per_s=round(n_log / (t["median_ms"] * 1e-3)))
        out["series_%s_window" % what] = t
        _, t = timed(lambda: sim.area_series(what, stride=24), repeats)
        t.update(log_entries_per_s=round(n_log / (t["median_ms"] * 1e-3)))
        out["series_%s_stride24" % what] = t
    t0 = time.perf_counter()
    lists = sim.exposures_per_output_area()
    out["exposures_per_output_area_host_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    if len(rec) * pop.n_areas <= 50_000_000:                      # the dense stride-1 table fits: the two routes must agree
        full = sim.area_series("exposures")
        assert {"OA%07d" % a: full[:, a][full[:, a] != 0].tolist() for a in np.flatnonzero(full.any(axis=0)).tolist()} == lists
    print(json.dumps(out))
    sim.close()


if __name__ == "__main__":
    main()
