"""Runs a preset and reports its contact-hours at risk (esim_contact_hours): per setting the contact-hours, the transmissions
among them and the transmissions per contact-hour with exposure_chance beside it, before and after the step at which masks came
into force -- and times the call, with esim_transmission_tree(NULL, NULL, NULL), the replay it sits on, from the same process
beside it.  Prints one JSON line; --out also writes it to a file (default profiles/contact_hours_<preset>.json).

    python tools/contact_hours.py [preset] [steps] [repeats] [--out FILE]

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


def table(title, got, chance):
    print("%s (exposure_chance %.4g)" % (title, chance))
    print("  %-17s %16s %14s %10s" % ("setting", "contact-hours", "transmissions", "rate"))
    rows = {}
    for s, name in enumerate(_lib.SETTING_NAMES[:_lib.N_SETTINGS]):
        h, t = int(got["hours"][s].sum()), int(got["transmissions"][s].sum())
        rows[name] = {"hours": h, "transmissions": t, "rate": round(t / h, 6) if h else None}
        print("  %-17s %16d %14d %10s" % (name, h, t, "%.5f" % (t / h) if h else "-"))
    return rows


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
           "what": "wall ms around one synchronised call, the tree replay and the copies out included; median (min, max) of `repeats` calls after one warm-up call"}
    ep = _lib.default_params(max_steps=max(a.steps, 5000))
    sim = Simulator(pop, ep)
    sim.set_groups(labels, n_groups)
    t0 = time.perf_counter()
    rec = sim.run(a.steps)
    n = len(rec)
    total = int(rec["exposures_building"].sum(dtype=np.int64) + rec["exposures_bus"].sum(dtype=np.int64))
    out.update(steps=n, run_ms=round((time.perf_counter() - t0) * 1e3, 2), log_entries=total + len(sim.seeds()), exposure_chance=float(ep.exposure_chance))
    lib, ctx = sim.lib, sim._ctx
    # the yardstick: the replay the call sits on
    _, out["transmission_tree_null"] = timed(lambda: _lib.check(lib.esim_transmission_tree(ctx, None, None, None), ctx), a.repeats)
    mixing, out["mixing_matrix"] = timed(sim.mixing_matrix, a.repeats)
    whole, out["contact_hours_all"] = timed(lambda: sim.contact_hours("all"), a.repeats)
    by_group, out["contact_hours_group"] = timed(lambda: sim.contact_hours("group"), a.repeats)
    with_cases, out["contact_hours_all_per_case"] = timed(lambda: sim.contact_hours("all", per_case=True), a.repeats)
    for s, name in enumerate(_lib.SETTING_NAMES[:_lib.N_SETTINGS]):
        _, out["contact_hours_all_" + name] = timed(lambda: sim.contact_hours("all", (s,)), a.repeats)
    if (by_group["transmissions"] > by_group["hours"]).any() or (by_group["transmissions"].sum(axis=0) != mixing).any():
        raise SystemExit("the transmissions are not the mixing matrix split by setting, or exceed the contact-hours")
    if (by_group["hours"].sum(axis=(1, 2)) != whole["hours"][:, 0, 0]).any() or int(with_cases["per_case"].sum(dtype=np.int64)) != int(whole["hours"].sum()):
        raise SystemExit("the contact-hours by group or per case do not add up to the one cell")
    masked = np.flatnonzero(rec["mask_status"] != _lib.MASK_NONE)
    out["whole_run"] = table("steps 1..%d" % n, whole, ep.exposure_chance)
    if masked.size and 1 <= int(masked[0]) + 1 < n:                  # the record of step s decides the masks of step s + 1
        at = int(masked[0]) + 2
        out["masks_from_step"] = at
        out["before_masks"] = table("steps 1..%d, before masks" % (at - 1), sim.contact_hours("all", last_step=at - 1), ep.exposure_chance)
        out["with_masks"] = table("steps %d..%d, masks in force (effectiveness %.2f)" % (at, n, ep.mask_effectiveness), sim.contact_hours("all", first_step=at), ep.exposure_chance)
    else:
        print("no mask mandate came into force in %d steps" % n)
    sim.close()
    path = a.out or os.path.join(ROOT, "profiles", "contact_hours_%s.json" % a.preset)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
