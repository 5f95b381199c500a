"""Runs a preset with five-year age bands as groups and reports its household outbreaks: the household secondary attack rate by
age band of the case and of the contact (esim_household_sar), the final-size table (esim_household_final_sizes) and the
per-household arrays (esim_household_outbreaks) -- and times the three calls, with esim_mixing_matrix (which shares the tree
replay with the attack rate) and esim_building_exposures (which shares the settings replay with the other two) from the same
process beside them for scale.  Prints one JSON line; --out also writes it to a file (default
profiles/household_outputs_<preset>.json).

    python tools/household_outputs.py [preset] [steps] [repeats] [--out FILE]

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

AGE_EDGES = list(range(5, 95, 5))                  # 19 bands: 0-4, 5-9, ..., 85-89, 90+


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("preset", nargs="?", default="york")
    ap.add_argument("steps", nargs="?", type=int, default=5000)
    ap.add_argument("repeats", nargs="?", type=int, default=7)
    ap.add_argument("--out")
    a = ap.parse_args()
    pop = Population.synthetic(a.preset)
    labels, n_groups = pop.age_bands(AGE_EDGES)
    out = {"preset": a.preset, "n_citizens": pop.n_citizens, "n_buildings": pop.n_buildings, "n_groups": n_groups, "library": os.path.basename(_lib.LIB_PATH),
           "what": "wall ms around one synchronised call; median (min, max) of `repeats` calls after one warm-up call"}
    ep = _lib.default_params(max_steps=max(a.steps, 5000))
    sim = Simulator(pop, ep)
    sim.set_groups(labels, n_groups)
    t0 = time.perf_counter()
    rec = sim.run(a.steps)
    n = len(rec)
    total = int(rec["exposures_building"].sum(dtype=np.int64) + rec["exposures_bus"].sum(dtype=np.int64))
    out.update(steps=n, run_ms=round((time.perf_counter() - t0) * 1e3, 2), log_entries=total + len(sim.seeds()))
    # the yardsticks: what a user pays today for a table on top of the same replays
    mixing, out["mixing_matrix_household"] = timed(lambda: sim.mixing_matrix("household"), a.repeats)
    _, out["building_exposures"] = timed(sim.building_exposures, a.repeats)
    house, out["household_outbreaks"] = timed(sim.household_outbreaks, a.repeats)
    (final_size, intro_size), out["household_final_sizes"] = timed(sim.household_final_sizes, a.repeats)
    (at_all, sec_all), out["household_sar_all"] = timed(lambda: sim.household_sar("all", complete=False), a.repeats)
    (at, sec), out["household_sar_group"] = timed(lambda: sim.household_sar("group", complete=False), a.repeats)
    if int(house["cases"].sum(dtype=np.int64)) != total + len(sim.seeds()):
        raise SystemExit("the cases of the households do not add up to the exposure log")
    if int(final_size.sum(dtype=np.int64)) != int(intro_size.sum(dtype=np.int64)):
        raise SystemExit("the two tables do not hold the same households")
    if not (sec == mixing).all() or int(sec.sum()) != int(sec_all.sum()) or int(at.sum()) != int(at_all.sum()) or (sec > at).any():
        raise SystemExit("the secondary cases are not the household transmissions of the mixing matrix, or exceed the housemates at risk")
    # complete cohorts only, for the rates
    try:
        at, sec = sim.household_sar("group")
    except ValueError:
        print("no cohort is complete after %d steps: the rates below count cases that may still infect" % n)
    with np.errstate(invalid="ignore", divide="ignore"):
        sar = np.where(at > 0, sec.astype(np.float64) / at.astype(np.float64), np.nan)
    out.update(households=int(final_size.sum(dtype=np.int64)), households_with_a_case=int((house["cases"] > 0).sum()),
               households_introduced_twice_or_more=int((house["introductions"] >= 2).sum()),
               at_risk=int(at.sum()), secondary=int(sec.sum()), sar_all=round(float(sec.sum()) / float(at.sum()), 5) if at.sum() else None,
               sar_by_age_band=[[None if x != x else round(float(x), 4) for x in row] for row in sar],
               final_size=final_size.tolist(), introductions=intro_size.tolist())
    print("household secondary attack rate, rows: age band of the case, columns: of the contact (%d x %d, '-': nobody at risk)" % (n_groups, n_groups))
    for row in sar:
        print(" ".join("   - " if x != x else "%.3f" % x for x in row))
    top = max(1, int(np.flatnonzero(final_size.sum(axis=0)).max(initial=0)) + 1)
    print("households by size (rows) and cases (columns 0..%d); the last bin of either holds everything from 63 on" % (top - 1))
    for size in np.flatnonzero(final_size.sum(axis=1)).tolist():
        print("%3d: %s" % (size, " ".join("%8d" % x for x in final_size[size, :top])))
    sim.close()
    path = a.out or os.path.join(ROOT, "profiles", "household_outputs_%s.json" % a.preset)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
