"""Runs a preset and reports what the hospital-burden calls cost beside the calls they are built from: esim_burden_summary and
esim_curve_summary(infected) in the same process, by all, by the preset's occupation groups and by Output Area; and
esim_burden_series(occupancy) beside esim_group_series(infected) at the same shape.  The severity tables have one row per group.
Prints one JSON line; --out also writes it to a file (default profiles/burden_<preset>.json).

    python tools/hospital_burden.py [preset] [steps] [repeats] [--stride 24] [--out FILE]

Every time is wall time around one synchronised library call (perf_counter; the call ends with its own stream wait), temporary
device memory and the copies out included, after one warm-up call, as the median of `repeats` calls with the smallest and the
largest beside it.  The burden summary does the curve summary's work on fewer intervals plus one Philox block per case, so its
median should not exceed the curve summary's by more than the spread of that median: the file states both and the verdict.  The
time of k_burden_events itself is not in these figures: run this tool under `rocprofv3 --kernel-trace --stats` for it."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from epidemicsimulator_amd import Population, Simulator, _lib  # noqa: E402

ADMIT = (2, 2, 4, 8, 15, 30, 50, 70)            # per cent, cycled over the groups
DEATH = (0, 0, 1, 2, 5, 10, 25, 50)
DELAY = (5, 10, 20, 25, 20, 15)                 # days 0 .. 6
STAY = (10, 15, 15, 12, 10, 8, 7, 6, 5, 4, 3, 2, 2)   # days 1 .. 14


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "repeats": len(ms),
            "every_ms": [round(x, 4) for x in ms]}          # (in call order: a slow call shows where in the series it fell)


def timed(fn, repeats):
    """(the last result, the times) of `repeats` calls after one warm-up call."""
    fn()
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return out, stats(ms)


def percent(values):
    return np.array([(int(p) << 32) // 100 for p in values], np.uint32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("preset", nargs="?", default="uk64m")
    ap.add_argument("steps", nargs="?", type=int, default=5000)
    ap.add_argument("repeats", nargs="?", type=int, default=7)
    ap.add_argument("--stride", type=int, default=24)
    ap.add_argument("--out")
    a = ap.parse_args()
    pop = Population.synthetic(a.preset)
    labels, n_groups = pop.occupation_groups()
    sim = Simulator(pop, _lib.default_params(max_steps=max(a.steps, 5000)))
    sim.set_groups(labels, n_groups)
    sim.set_burden(dict(admit_thr=percent(ADMIT[g % 8] for g in range(n_groups)), death_thr=percent(DEATH[g % 8] for g in range(n_groups)),
                        delay_cdf=percent(np.cumsum(DELAY)), stay_cdf=percent(np.cumsum(STAY)), delay_unit=24, stay_unit=24))
    n = len(sim.run(a.steps))
    out = {"preset": a.preset, "n_citizens": pop.n_citizens, "n_areas": pop.n_areas, "n_groups": int(n_groups), "steps": n,
           "library": os.path.basename(_lib.LIB_PATH), "log_entries": int(len(sim.exposure_events()[0])),
           "what": "wall ms around one synchronised call; median (min, max) of `repeats` calls after one warm-up call"}
    got = {}
    for where in ("all", "group", "home"):
        got[where], t = timed(lambda: sim.burden_summary(where, 1, n, 1), a.repeats)
        out["burden_summary_" + where] = dict(t, pair_stats=sim.pair_stats(), columns=int(got[where]["peak"].size), admissions=int(got[where]["admissions"].sum()),
                                              deaths=int(got[where]["deaths"].sum()), largest_peak=int(got[where]["peak"].max()))
        _, c = timed(lambda: sim.curve_summary(where, "infected", 1, n, 1), a.repeats)
        out["curve_summary_" + where] = dict(c, pair_stats=sim.pair_stats())
        spread = c["max_ms"] - c["min_ms"]
        out["verdict_" + where] = {"burden_minus_curve_median_ms": round(t["median_ms"] - c["median_ms"], 4), "curve_spread_ms": round(spread, 4),
                                   "within_the_spread": bool(t["median_ms"] - c["median_ms"] <= spread)}
    if int(got["group"]["bed_steps"].sum()) != int(got["all"]["bed_steps"][0]) or int(got["home"]["bed_steps"].sum()) != int(got["all"]["bed_steps"][0]):
        raise SystemExit("the bed-steps by group or by area do not add up to the one column of all")
    n_rows = (n - 1) // a.stride + 1
    rows, out["burden_series_group"] = timed(lambda: sim.burden_series("occupancy", "group", 1, n_rows, a.stride), a.repeats)
    _, out["group_series_infected"] = timed(lambda: sim.group_series("infected", 1, n_rows, a.stride), a.repeats)
    out["series_shape"] = [int(n_rows), int(n_groups)]
    if int(rows.max()) > int(got["group"]["peak"].max()):
        raise SystemExit("an occupancy row exceeds the peak of the summary")
    out["k_burden_events_kernel_trace"] = "unmeasured here: the figure needs a kernel-trace run of its own"
    sim.close()
    print("%s, %d steps: burden_summary %.2f ms by all, %.2f ms by %d groups, %.2f ms by %d areas; curve_summary(infected) %.2f / %.2f / %.2f ms"
          % (a.preset, n, out["burden_summary_all"]["median_ms"], out["burden_summary_group"]["median_ms"], n_groups, out["burden_summary_home"]["median_ms"], pop.n_areas,
             out["curve_summary_all"]["median_ms"], out["curve_summary_group"]["median_ms"], out["curve_summary_home"]["median_ms"]))
    path = a.out or os.path.join(ROOT, "profiles", "burden_%s.json" % a.preset)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
