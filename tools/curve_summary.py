"""Runs a preset and reports what esim_curve_summary costs by all, by the occupation groups and by Output Area: the call's wall
time and the three parts of the pair engine (esim_pair_stats: insert, compact, sort), with the route there was before beside
it for the groups -- esim_group_series at stride 1 and the reduction in numpy -- whose result the call must reproduce.  By area
that route is not run: the size of the rows it would move is stated instead.  Prints one JSON line; --out also writes it to a
file (default profiles/curve_summary_<preset>.json).

    python tools/curve_summary.py [preset] [steps] [repeats] [--status infected] [--threshold 1] [--out FILE]

Every time is wall time around one synchronised library call (perf_counter; the call ends with its own stream wait), temporary
device memory and the copies out included, after one warm-up call, as the median of `repeats` calls with the smallest and the
largest beside it.  The times of the scan and the reduce kernels themselves are not in esim_pair_stats: run this tool under
`rocprofv3 --kernel-trace --stats` for them (k_curve_tile, k_curve_carry, k_curve_scan, k_curve_reduce)."""
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

NEVER = _lib.NEVER


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


def from_rows(rows, threshold):
    """The summary of rows [n_steps, n_cols] (row 0 = step 1) in numpy."""
    x = rows.astype(np.int64)
    steps = np.arange(1, x.shape[0] + 1, dtype=np.int64)[:, None]
    peak, at = x.max(axis=0), x >= threshold
    n_at = at.sum(axis=0)
    return {"peak": peak.astype(np.uint32), "peak_step": np.where(peak > 0, 1 + x.argmax(axis=0), NEVER).astype(np.uint32),
            "steps_at_least": n_at.astype(np.uint32),
            "first_at_least": np.where(n_at > 0, np.where(at, steps, 1 << 40).min(axis=0), NEVER).astype(np.uint32),
            "last_at_least": np.where(n_at > 0, np.where(at, steps, -1).max(axis=0), NEVER).astype(np.uint32),
            "person_steps": x.sum(axis=0).astype(np.uint64)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("preset", nargs="?", default="york")
    ap.add_argument("steps", nargs="?", type=int, default=5000)
    ap.add_argument("repeats", nargs="?", type=int, default=7)
    ap.add_argument("--status", default="infected", choices=("exposed", "infected", "active"))
    ap.add_argument("--threshold", type=int, default=1)
    ap.add_argument("--out")
    a = ap.parse_args()
    pop = Population.synthetic(a.preset)
    labels, n_groups = pop.occupation_groups()
    sim = Simulator(pop, _lib.default_params(max_steps=max(a.steps, 5000)))
    sim.set_groups(labels, n_groups)
    n = len(sim.run(a.steps))
    out = {"preset": a.preset, "n_citizens": pop.n_citizens, "n_areas": pop.n_areas, "n_groups": int(n_groups), "steps": n, "status": a.status,
           "threshold": a.threshold, "library": os.path.basename(_lib.LIB_PATH), "log_entries": int(len(sim.exposure_events()[0])),
           "what": "wall ms around one synchronised call; median (min, max) of `repeats` calls after one warm-up call"}
    got = {}
    for where in ("all", "group", "home"):
        got[where], t = timed(lambda: sim.curve_summary(where, a.status, 1, n, a.threshold), a.repeats)
        out["curve_summary_" + where] = dict(t, pair_stats=sim.pair_stats(), columns=int(got[where]["peak"].size),
                                             columns_with_a_case=int((got[where]["peak"] > 0).sum()), largest_peak=int(got[where]["peak"].max()))

    def old_route():
        rows = sum(sim.group_series(what).astype(np.int64) for what in (("exposed", "infected") if a.status == "active" else (a.status,)))
        return from_rows(rows, a.threshold)

    want, out["group_series_stride_1_and_numpy"] = timed(old_route, max(1, a.repeats // 2))
    for k, v in want.items():
        if (got["group"][k] != v).any():
            raise SystemExit("curve_summary by group differs from the rows of group_series in %s" % k)
    if int(got["group"]["person_steps"].sum()) != int(got["all"]["person_steps"][0]) or int(got["home"]["person_steps"].sum()) != int(got["all"]["person_steps"][0]):
        raise SystemExit("the person-steps by group or by area do not add up to the one column of all")
    out["rows_by_area_at_stride_1_bytes"] = int(pop.n_areas) * n * 4
    sim.close()
    print("%s, %d steps, %s: curve_summary %.2f ms by all, %.2f ms by %d groups, %.2f ms by %d areas; group_series + numpy %.1f ms; the rows by area would be %.2f GB"
          % (a.preset, n, a.status, out["curve_summary_all"]["median_ms"], out["curve_summary_group"]["median_ms"], n_groups, out["curve_summary_home"]["median_ms"],
             pop.n_areas, out["group_series_stride_1_and_numpy"]["median_ms"], out["rows_by_area_at_stride_1_bytes"] / 1e9))
    path = a.out or os.path.join(ROOT, "profiles", "curve_summary_%s.json" % a.preset)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
