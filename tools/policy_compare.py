"""Runs a preset twice under one seed -- the default parameters, then perfect masks (mask_effectiveness 1.0) -- and reports what
the paired comparison says (averted, added, first divergence; over a handful of seeds the paired against the unpaired standard
error of the cases averted) and what its calls cost: esim_baseline_keep, esim_compare by all / home / group, esim_compare_series
and a paired esim_ensemble_fold, with esim_area_census(ESIM_AREA_HOME) -- the existing pass with the same per-citizen traffic --
from the same process beside them as the yardstick.  Prints one JSON line; --out also writes it to a file (default
profiles/policy_compare_<preset>.json).

    python tools/policy_compare.py [preset] [steps] [repeats] [--members K] [--out FILE]

Every time is wall time around one synchronised library call (perf_counter; esim_baseline_keep and the fold are followed by
esim_synchronize, the others end with their own stream wait), temporary device memory and the copies out included, after one
warm-up call, as the median of `repeats` calls with the smallest and the largest beside it.  "model" is what the count kernel
moves by its own design -- 8 B per citizen for the two planes -- and the time that takes at the 6.3 TB/s a float4 copy reaches."""
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
from epidemicsimulator_amd.ensemble import paired_summary  # noqa: E402

AGE_EDGES = list(range(5, 95, 5))                  # 19 bands
POLICY = {"mask_effectiveness": 1.0}
HBM_COPY_TBS = 6.3                                 # what a float4 copy reaches on one MI355X


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "repeats": len(ms)}


def timed(fn, repeats):
    """(the last result, the times) of `repeats` calls after one warm-up call."""
    fn()
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return out, stats(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("preset", nargs="?", default="york")
    ap.add_argument("steps", nargs="?", type=int, default=5000)
    ap.add_argument("repeats", nargs="?", type=int, default=7)
    ap.add_argument("--members", type=int, default=4, help="seeds of the paired ensemble (the default seed and the next ones)")
    ap.add_argument("--out")
    a = ap.parse_args()
    pop = Population.synthetic(a.preset)
    labels, n_groups = pop.age_bands(AGE_EDGES)
    base = _lib.default_params(max_steps=max(a.steps, 5000))
    out = {"preset": a.preset, "n_citizens": pop.n_citizens, "n_areas": pop.n_areas, "n_groups": int(n_groups), "library": os.path.basename(_lib.LIB_PATH),
           "policy": POLICY, "what": "wall ms around one synchronised call; median (min, max) of `repeats` calls after one warm-up call"}
    sim = Simulator(pop, base)
    sim.set_groups(labels, n_groups)

    def keep():
        sim.keep_baseline()
        sim.synchronize()

    def fold():
        sim.ensemble_fold()
        sim.synchronize()

    rec = sim.run(a.steps)
    n = len(rec)
    _, out["baseline_keep"] = timed(keep, a.repeats)
    info = sim.baseline_info()
    sim.restart(base, **POLICY)
    sim.run(n)
    _, out["area_census_home"] = timed(lambda: sim.area_census("home"), a.repeats)          # the yardstick
    by_all, out["compare_all"] = timed(lambda: sim.compare("all", 0, n), a.repeats)
    by_home, out["compare_home"] = timed(lambda: sim.compare("home", 0, n), a.repeats)
    by_group, out["compare_group"] = timed(lambda: sim.compare("group", 0, n), a.repeats)
    _, out["compare_all_with_cls"] = timed(lambda: sim.compare("all", 0, n, citizens=True), a.repeats)
    rows, out["compare_series_home_stride24"] = timed(lambda: sim.compare_series("home", 0, None, 24), a.repeats)
    if (by_home["counts"].sum(0) != by_all["counts"][0]).any() or (by_group["counts"].sum(0) != by_all["counts"][0]).any():
        raise SystemExit("the columns by home or by group do not add up to the by-all row")
    if int(rows[0].sum(dtype=np.int64)) != info["n_cases"]:
        raise SystemExit("the baseline's rows do not add up to its log entries")
    window = dict(first_step=0, n_rows=n // 24 + 1, stride=24, cumulative=True)
    sim.ensemble_begin_paired("home", min_baseline=5, min_averted=1, **window)
    _, out["paired_fold_home_stride24"] = timed(fold, a.repeats)
    counts = by_all["counts"][0]
    moved = 8.0 * pop.n_citizens
    out.update(steps=n, baseline_log_entries=info["n_cases"], policy_log_entries=int(counts[_lib.CMP_BOTH] + counts[_lib.CMP_ADDED]),
               counts=dict(zip(_lib.CMP_NAMES, (int(x) for x in counts))), delay=int(by_all["delay"][0]), first_divergence=by_all["first_divergence"],
               areas_with_fewer_cases=int((by_home["counts"][:, _lib.CMP_AVERTED] > by_home["counts"][:, _lib.CMP_ADDED]).sum()),
               areas_with_more_cases=int((by_home["counts"][:, _lib.CMP_AVERTED] < by_home["counts"][:, _lib.CMP_ADDED]).sum()),
               model={"bytes_per_citizen": 8, "bytes": moved, "ms_at_%.1f_TBs" % HBM_COPY_TBS: round(moved / (HBM_COPY_TBS * 1e12) * 1e3, 4),
                      "share_of_hbm_peak_8_TBs_at_the_median_compare_all": round(moved / (out["compare_all"]["median_ms"] * 1e-3) / 8e12, 4)})
    # a handful of members, each its own baseline and policy run under one seed: the paired against the unpaired standard error
    seeds = [int(base.seed) + i for i in range(a.members)]
    sim.ensemble_begin_paired("all", min_baseline=1, min_averted=1, **window)
    members = []
    for seed in seeds:
        sim.restart(base, seed=seed)
        sim.run(n)
        sim.keep_baseline()
        sim.restart(base, seed=seed, **POLICY)
        sim.run(n)
        got = sim.compare("all", 0, n)
        members.append({"seed": seed, "counts": dict(zip(_lib.CMP_NAMES, (int(x) for x in got["counts"][0]))), "first_divergence": got["first_divergence"]})
        sim.ensemble_fold()
    s = paired_summary(sim.ensemble_read_paired(), 0, 24)
    last = {k: float(s[k][-1, 0]) for k in ("mean_baseline", "mean_policy", "mean_averted", "se_paired", "se_unpaired", "p_averted")}
    out["ensemble"] = dict(members=members, cumulative_to_the_last_step=last)
    sim.close()
    print("%s, %d steps, seed %d: %d cases averted, %d added, first divergence at step %s; over %d seeds the mean averted is %.1f, standard error %.1f paired against %.1f unpaired"
          % (a.preset, n, int(base.seed), counts[_lib.CMP_AVERTED], counts[_lib.CMP_ADDED], by_all["first_divergence"], a.members, last["mean_averted"], last["se_paired"], last["se_unpaired"]))
    path = a.out or os.path.join(ROOT, "profiles", "policy_compare_%s.json" % a.preset)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
