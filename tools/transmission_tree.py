"""Times the transmission-tree calls on a preset after its run -- esim_transmission_tree, esim_offspring, esim_reproduction_series
(one column, stride 24 from step 0) and esim_mixing_matrix (four age bands) -- with esim_exposure_settings from the same process
beside them for scale; and reports what the tree says: the cohort reproduction number per day, before and after the lockdown
starts, the offspring histogram, the share of transmissions caused by the top 10 % of infectors and the deepest generation.
Prints one JSON line; --out also writes it to a file (default profiles/transmission_tree_<preset>.json).

    python tools/transmission_tree.py [preset] [steps] [repeats] [--out FILE]

Every time is wall time around one synchronised library call (perf_counter; the calls end with their own stream wait), after
one warm-up call, as the median of `repeats` calls with the smallest and the largest beside it."""
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


def cohort_r(cases, offspring):
    c, o = int(cases.sum(dtype=np.int64)), int(offspring.sum(dtype=np.int64))
    return {"cases": c, "offspring": o, "R": round(o / c, 4) if c else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("preset", nargs="?", default="york")
    ap.add_argument("steps", nargs="?", type=int, default=5000)
    ap.add_argument("repeats", nargs="?", type=int, default=7)
    ap.add_argument("--out")
    a = ap.parse_args()
    pop = Population.synthetic(a.preset)
    out = {"preset": a.preset, "n_citizens": pop.n_citizens, "n_areas": pop.n_areas, "n_buildings": pop.n_buildings,
           "what": "wall ms around one synchronised call; median (min, max) of `repeats` calls after one warm-up call"}
    ep = _lib.default_params(max_steps=max(a.steps, 5000))
    sim = Simulator(pop, ep)
    sim.set_groups(*pop.age_bands([18, 40, 65]))
    t0 = time.perf_counter()
    rec = sim.run(a.steps)
    n = len(rec)
    total = int(rec["exposures_building"].sum(dtype=np.int64) + rec["exposures_bus"].sum(dtype=np.int64))
    out.update(steps=n, run_ms=round((time.perf_counter() - t0) * 1e3, 2), log_entries=total + len(np.unique(pop.seeds)))
    _, out["exposure_settings"] = timed(sim.exposure_settings, a.repeats)
    (infector, k, gen), out["transmission_tree"] = timed(sim.transmission_tree, a.repeats)
    counts, out["offspring"] = timed(lambda: sim.offspring(1, n), a.repeats)
    (cases, off), out["reproduction_series_all_stride24"] = timed(lambda: sim.reproduction_series("all"), a.repeats)
    matrix, out["mixing_matrix"] = timed(sim.mixing_matrix, a.repeats)
    # the four agree with each other and with the records
    if int(counts.sum(dtype=np.int64)) != total or int(matrix.sum(dtype=np.int64)) != total or int(off.sum(dtype=np.int64)) != total:
        raise SystemExit("offspring, matrix or cohort rows do not add up to the exposures of the records")
    if int((infector != _lib.NO_INFECTOR).sum()) != total:
        raise SystemExit("the tree does not hold one infector per exposure of the records")
    # cohort R per day (stride 24 from step 0; a row is complete once its last step's infectious period has run)
    complete = np.arange(len(cases)) * 24 + 23 + int(ep.exposed_time) + 1 + int(ep.infected_time) <= n
    r_day = [round(float(o) / float(c), 4) if c else None for c, o in zip(cases[:, 0], off[:, 0])]
    out["cohort_R_per_day"] = {"complete_days": int(complete.sum()), "R": r_day}
    out["cohort_R"] = {"whole_run": cohort_r(cases[complete], off[complete])}
    if rec["lockdown"].any():
        lock = int(np.argmax(rec["lockdown"])) + 1                   # the first step whose record has a lockdown: it holds from the next step on
        day = (lock + 1) // 24                                       # the first cohort row with steps under it
        out["cohort_R"].update(first_lockdown_step=lock, before_lockdown=cohort_r(cases[:day][complete[:day]], off[:day][complete[:day]]),
                               from_lockdown_on=cohort_r(cases[day:][complete[day:]], off[day:][complete[day:]]))
    # superspreading: offspring of everybody who was ever infectious
    infectors = counts[gen != _lib.NEVER].astype(np.int64)
    hist = np.bincount(np.minimum(infectors, 20))
    out["offspring_histogram"] = {"bins": "0 .. 19, 20 and more", "citizens": hist.tolist(), "max": int(infectors.max()) if infectors.size else 0,
                                  "mean": round(float(infectors.mean()), 4) if infectors.size else None}
    top = np.sort(infectors)[::-1][:max(1, infectors.size // 10)]
    out["top_10_percent_share"] = round(float(top.sum()) / float(total), 4) if total else None
    out["deepest_generation"] = int(gen[gen != _lib.NEVER].max()) if (gen != _lib.NEVER).any() else 0
    out["most_candidates"] = int(k.max())
    sim.close()
    path = a.out or os.path.join(ROOT, "profiles", "transmission_tree_%s.json" % a.preset)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
