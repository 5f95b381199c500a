"""Times the transmission-chain calls on a preset after its run -- esim_transmission_chains (both arrays), esim_outbreaks and
esim_transmission_ages -- with esim_transmission_tree (three arrays) and esim_reproduction_series (one column) from the same
process beside them for scale; and reports what the chains say: the outbreak every index case started, the share of
transmissions per decile of the infectious period, and the mean generation interval per setting.
Prints one JSON line; --out also writes it to a file (default profiles/transmission_chains_<preset>.json).

    python tools/transmission_chains.py [preset] [steps] [repeats] [--out FILE] [--ages-only]

Every time is wall time around one synchronised library call (perf_counter; the calls end with their own stream wait), after
one warm-up call, as the median of `repeats` calls with the smallest and the largest beside it.  --ages-only times
esim_transmission_ages alone: with ESIM_LIB pointing at the `ages-global` build of the library (make -C
epidemicsimulator_amd/csrc ages-global) it is the run that puts k_chain_ages with plain global atomics beside the LDS form."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("preset", nargs="?", default="york")
    ap.add_argument("steps", nargs="?", type=int, default=5000)
    ap.add_argument("repeats", nargs="?", type=int, default=7)
    ap.add_argument("--out")
    ap.add_argument("--ages-only", action="store_true")
    a = ap.parse_args()
    pop = Population.synthetic(a.preset)
    out = {"preset": a.preset, "n_citizens": pop.n_citizens, "library": os.path.basename(_lib.LIB_PATH),
           "what": "wall ms around one synchronised call; median (min, max) of `repeats` calls after one warm-up call"}
    ep = _lib.default_params(max_steps=max(a.steps, 5000))
    sim = Simulator(pop, ep)
    t0 = time.perf_counter()
    rec = sim.run(a.steps)
    n = len(rec)
    total = int(rec["exposures_building"].sum(dtype=np.int64) + rec["exposures_bus"].sum(dtype=np.int64))
    out.update(steps=n, run_ms=round((time.perf_counter() - t0) * 1e3, 2), log_entries=total + len(sim.seeds()),
               launches_per_pass=-(-n // (int(ep.exposed_time) + 1)))
    ages, out["transmission_ages"] = timed(sim.transmission_ages, a.repeats)
    if int(ages.sum(dtype=np.int64)) != total:
        raise SystemExit("the ages do not add up to the exposures of the records")
    if not a.ages_only:
        _, out["transmission_tree"] = timed(sim.transmission_tree, a.repeats)                     # the yardstick: three arrays copied out
        _, out["reproduction_series_all_stride24"] = timed(lambda: sim.reproduction_series("all"), a.repeats)
        (lineage, desc), out["transmission_chains"] = timed(sim.transmission_chains, a.repeats)
        table, out["outbreaks"] = timed(sim.outbreaks, a.repeats)
        if int(table["size"].sum(dtype=np.int64)) != total or int((lineage != _lib.NO_LINEAGE).sum()) != total + len(table["seeds"]):
            raise SystemExit("outbreak sizes or lineages do not add up to the exposures of the records")
        if not (desc[table["seeds"]] == table["size"]).all():
            raise SystemExit("the outbreak sizes are not the descendants of the index cases")
        out["outbreak_table"] = {k: table[k].tolist() for k in ("seeds", "size", "depth", "last_step")}
        print("%10s %10s %6s %10s" % ("index case", "size", "depth", "last step"))
        for row in zip(*(table[k].tolist() for k in ("seeds", "size", "depth", "last_step"))):
            print("%10d %10d %6d %10d" % row)
    # when during their infectious period people transmit: deciles of 0 .. infected_time
    it, et = int(ep.infected_time), int(ep.exposed_time)
    by_age = ages.sum(axis=0, dtype=np.int64)[:it + 1]
    decile = np.minimum(np.arange(it + 1) * 10 // (it + 1), 9)
    share = np.bincount(decile, weights=by_age, minlength=10) / max(1, total)
    out["share_per_infectious_age_decile"] = [round(float(x), 4) for x in share]
    # the mean generation interval, a + exposed_time + 1 (index cases counted by the same rule), per setting and overall
    a_of = np.arange(_lib.AGE_BINS, dtype=np.float64) + et + 1
    per = ages.sum(axis=1, dtype=np.int64)
    out["mean_generation_interval_steps"] = dict(
        {name: round(float((ages[s] * a_of).sum() / per[s]), 2) if per[s] else None for s, name in enumerate(_lib.SETTING_NAMES)},
        all=round(float((ages.sum(axis=0) * a_of).sum() / total), 2) if total else None)
    out["transmissions_per_setting"] = dict(zip(_lib.SETTING_NAMES, per.tolist()))
    print("share of transmissions per decile of the infectious period: " + " ".join("%.3f" % x for x in share))
    print("mean generation interval (steps): %s" % out["mean_generation_interval_steps"])
    sim.close()
    path = a.out or os.path.join(ROOT, "profiles", "transmission_chains_%s%s.json" % (a.preset, "_ages_only" if a.ages_only else ""))
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
