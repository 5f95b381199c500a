"""Runs a preset twice -- a baseline and a policy run under the same seed -- and reports what the calls on the list of admitted
cases cost beside their nearest relatives, in the same process: esim_burden_compare against esim_burden_summary by all, by the
preset's occupation groups and by Output Area; one fold of the burden-series kind against the whole esim_burden_series call of the
same shape; esim_burden_baseline_keep beside esim_burden_outcomes; and, over four seeds, the standard error of
the bed-days averted paired against unpaired.  Prints one JSON line; --out also writes it to a file (default
profiles/beds_<preset>.json).

    python tools/burden_compare.py [preset] [steps] [repeats] [--stride 24] [--variance-preset NAME] [--skip-variance] [--kernel-stats CSV] [--out FILE]

Every time is wall time around one synchronised library call (perf_counter; the call ends with its own stream wait), temporary
device memory and the copies out included, after one warm-up call, as the median of `repeats` calls with the smallest and the
largest beside it.  The comparison does two collects and two passes over the admitted cases and uses no pair table, no sort and
no scan, so its median should not exceed the summary's by more than the spread of that median: the file states both and the
verdict.  Kernel times are not in these figures: run this tool under a kernel trace (--skip-variance) in a run of its own and
give the statistics it leaves to a second run with --kernel-stats."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from epidemicsimulator_amd import Ensemble, Population, Simulator, _lib  # noqa: E402
from hospital_burden import ADMIT, DEATH, DELAY, STAY, percent, timed  # noqa: E402


def tables(n_groups):
    return dict(admit_thr=percent(ADMIT[g % 8] for g in range(n_groups)), death_thr=percent(DEATH[g % 8] for g in range(n_groups)),
                delay_cdf=percent(np.cumsum(DELAY)), stay_cdf=percent(np.cumsum(STAY)), delay_unit=24, stay_unit=24)


def variance(preset, pop, steps, seeds=4):
    """The standard error of the bed-days averted over `seeds` members, masks 0.7 against 1.0: paired (both arms under one seed)
    against unpaired (what two separate ensembles of that size would quote)."""
    labels, n_groups = pop.occupation_groups()
    ens = Ensemble(pop, _lib.default_params(max_steps=steps), group=(labels, n_groups), burden=tables(n_groups))
    res = ens.compare_burden(dict(mask_effectiveness=0.7), dict(mask_effectiveness=1.0), Ensemble.seeds(seeds), steps)
    b, c = res.totals["bed_steps_baseline"][:, 0].astype(np.float64) / 24.0, res.totals["bed_steps_current"][:, 0].astype(np.float64) / 24.0
    ens.close()
    m = float(seeds)
    return {"preset": preset, "steps": steps, "members": seeds, "bed_days_baseline": b.tolist(), "bed_days_policy": c.tolist(),
            "mean_averted": float((b - c).mean()), "se_paired": float(np.std(b - c, ddof=1) / np.sqrt(m)),
            "se_unpaired": float(np.sqrt((np.var(b, ddof=1) + np.var(c, ddof=1)) / m))}


FAMILY = ("k_beds_", "k_burden_", "k_series_prefix", "k_ensemble_fold_rows", "k_ensemble_fold_paired", "k_area_vax_replay")


def kernel_stats(path):
    """The family's rows of the kernel statistics a kernel trace of this tool left (CSV: Name, Calls, TotalDurationNs, AverageNs,
    MinNs, MaxNs): {kernel: calls, avg_us, min_us, max_us}."""
    import csv
    out = {}
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            name = r["Name"].split("(")[0].split(" ")[-1]
            if name.startswith(FAMILY):
                out[name] = {"calls": int(r["Calls"]), "avg_us": round(float(r["AverageNs"]) / 1e3, 2), "min_us": round(float(r["MinNs"]) / 1e3, 2),
                             "max_us": round(float(r["MaxNs"]) / 1e3, 2)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("preset", nargs="?", default="uk64m")
    ap.add_argument("steps", nargs="?", type=int, default=5000)
    ap.add_argument("repeats", nargs="?", type=int, default=7)
    ap.add_argument("--stride", type=int, default=24)
    ap.add_argument("--variance-preset", help="another preset for the variance figures (default: the same population)")
    ap.add_argument("--skip-variance", action="store_true", help="leave the four-seed variance figures out (a kernel-trace run)")
    ap.add_argument("--kernel-stats", help="the kernel statistics (CSV) of a kernel trace of this tool, taken in a run of its own: the family's kernel times go into the file")
    ap.add_argument("--out")
    a = ap.parse_args()
    pop = Population.synthetic(a.preset)
    labels, n_groups = pop.occupation_groups()
    sim = Simulator(pop, _lib.default_params(max_steps=max(a.steps, 5000)))
    sim.set_groups(labels, n_groups)
    sim.set_burden(tables(n_groups))
    n = len(sim.run(a.steps))
    out = {"preset": a.preset, "n_citizens": pop.n_citizens, "n_areas": pop.n_areas, "n_groups": int(n_groups), "steps": n,
           "library": os.path.basename(_lib.LIB_PATH), "log_entries": int(len(sim.exposure_events()[0])),
           "what": "wall ms around one synchronised call; median (min, max) of `repeats` calls after one warm-up call"}
    _, out["burden_baseline_keep"] = timed(sim.keep_burden_baseline, a.repeats)
    _, out["burden_outcomes"] = timed(sim.burden_outcomes, a.repeats)
    info = sim.burden_baseline_info()
    out["baseline"] = {"steps": info["steps"], "n_admitted": info["n_admitted"], "n_died": info["n_died"], "list_bytes": 12 * info["n_admitted"]}
    kept = {where: sim.burden_summary(where, 1, n, 1) for where in ("all", "group", "home")}
    sim.restart(mask_effectiveness=1.0)
    sim.run(n)
    for where in ("all", "group", "home"):
        got, t = timed(lambda: sim.burden_compare(where, 1, n), a.repeats)
        now, s = timed(lambda: sim.burden_summary(where, 1, n, 1), a.repeats)
        for k in ("bed_steps", "admissions", "deaths"):
            if not (got[k + "_baseline"] == kept[where][k]).all() or not (got[k + "_current"] == now[k]).all():
                raise SystemExit("burden_compare by %s: %s differs from burden_summary" % (where, k))
        out["burden_compare_" + where] = dict(t, columns=int(got["bed_steps_baseline"].size), bed_days_averted=float(got["bed_steps_averted"].sum()) / 24.0,
                                              admissions_averted=int(got["admissions_averted"].sum()), deaths_averted=int(got["deaths_averted"].sum()))
        out["burden_summary_" + where] = s
        spread = s["max_ms"] - s["min_ms"]
        out["verdict_" + where] = {"compare_minus_summary_median_ms": round(t["median_ms"] - s["median_ms"], 4), "summary_spread_ms": round(spread, 4),
                                   "within_the_spread": bool(t["median_ms"] - s["median_ms"] <= spread)}
    n_rows = (n - 1) // a.stride + 1
    rows, out["burden_series_group"] = timed(lambda: sim.burden_series("occupancy", "group", 1, n_rows, a.stride), a.repeats)
    sim.ensemble_begin_burden_series("group", "occupancy", 1, n_rows, a.stride, 1)
    _, out["fold_burden_series_group"] = timed(sim.ensemble_fold, a.repeats)
    acc = sim.ensemble_read_series()
    if not (acc["sum"] == rows.astype(np.uint64) * acc["members"]).all():
        raise SystemExit("the folds of the burden-series kind do not add up to the rows of burden_series")
    out["series_shape"] = [int(n_rows), int(n_groups)]
    (b, c), out["burden_compare_series_group"] = timed(lambda: sim.burden_compare_series("occupancy", "group", 1, n_rows, a.stride), a.repeats)
    if not (c == rows).all():
        raise SystemExit("the current side of burden_compare_series differs from burden_series")
    sim.close()
    if not a.skip_variance:
        out["variance_reduction"] = variance(a.variance_preset or a.preset, Population.synthetic(a.variance_preset) if a.variance_preset else pop, n)
    out["kernel_trace"] = kernel_stats(a.kernel_stats) if a.kernel_stats else "unmeasured here: kernel times need a kernel-trace run of their own (--kernel-stats)"
    print("%s, %d steps: burden_compare %.2f ms by all, %.2f ms by %d groups, %.2f ms by %d areas; burden_summary %.2f / %.2f / %.2f ms; a fold %.2f ms, burden_series %.2f ms"
          % (a.preset, n, out["burden_compare_all"]["median_ms"], out["burden_compare_group"]["median_ms"], n_groups, out["burden_compare_home"]["median_ms"], pop.n_areas,
             out["burden_summary_all"]["median_ms"], out["burden_summary_group"]["median_ms"], out["burden_summary_home"]["median_ms"],
             out["fold_burden_series_group"]["median_ms"], out["burden_series_group"]["median_ms"]))
    path = a.out or os.path.join(ROOT, "profiles", "beds_%s.json" % a.preset)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
