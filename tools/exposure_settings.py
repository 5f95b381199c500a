"""Times the exposures-by-setting calls on a preset after its run -- esim_exposure_settings, esim_setting_series (by setting, by
household area) and esim_building_exposures -- over a 336-row window at the Infected peak and with stride 24 over the whole run,
with esim_area_status_series(HOME, INCIDENCE) on the same windows beside them for scale; and reports where the epidemic spread:
the share of exposures per setting before and after the lockdown starts.  Prints one JSON line; --out also writes it to a file
(default profiles/exposure_settings_<preset>.json).

    python tools/exposure_settings.py [preset] [steps] [repeats] [--out FILE]

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


def windows(rec):
    peak = int(np.argmax(rec["infected"])) + 1
    w0 = max(1, min(peak - 168, len(rec) - 335))
    return {"window": dict(first_step=w0, n_rows=min(336, len(rec) - w0 + 1), stride=1), "stride24": dict(first_step=1, n_rows=None, stride=24)}


def shares(rows):
    total = rows.sum(axis=0, dtype=np.int64)
    return {"exposures": int(total.sum()), **{name: (round(float(total[k]) / float(total.sum()), 4) if total.sum() else None) for k, name in enumerate(_lib.SETTING_NAMES)}}


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
    sim = Simulator(pop, _lib.default_params(max_steps=max(a.steps, 5000)))
    t0 = time.perf_counter()
    rec = sim.run(a.steps)
    n = len(rec)
    out.update(steps=n, run_ms=round((time.perf_counter() - t0) * 1e3, 2),
               log_entries=int(rec["exposures_building"].sum(dtype=np.int64) + rec["exposures_bus"].sum(dtype=np.int64)) + len(np.unique(pop.seeds)))
    (setting, building), out["exposure_settings"] = timed(sim.exposure_settings, a.repeats)
    for key, win in windows(rec).items():
        shown = {k: v for k, v in win.items() if v is not None}
        last = n if win["n_rows"] is None else win["first_step"] + win["n_rows"] - 1
        by_setting, t = timed(lambda: sim.setting_series("setting", **win), a.repeats)
        out["setting_series_by_setting_%s" % key] = dict(t, rows=int(by_setting.shape[0]), **shown)
        by_home, t = timed(lambda: sim.setting_series("home", **win), a.repeats)
        out["setting_series_by_home_%s" % key] = dict(t, rows=int(by_home.shape[0]), **shown)
        counts, t = timed(lambda: sim.building_exposures(win["first_step"], last), a.repeats)
        out["building_exposures_%s" % key] = dict(t, first_step=win["first_step"], last_step=last)
        incidence, t = timed(lambda: sim.area_status_series("incidence", "home", **win), a.repeats)
        out["area_status_series_home_incidence_%s" % key] = dict(t, rows=int(incidence.shape[0]), **shown)
        # the three agree with each other and with the rows that exist
        if not (by_home == incidence).all():
            raise SystemExit("setting_series by home, full mask, differs from the incidence rows on %s" % shown)
        if not (by_setting.sum(axis=1, dtype=np.int64) == by_home.sum(axis=1, dtype=np.int64)).all():
            raise SystemExit("setting_series by setting and by home disagree on %s" % shown)
        if int(counts.sum(dtype=np.int64)) != int(by_setting[:, :_lib.SETTING_TRANSPORT].sum(dtype=np.int64)):
            raise SystemExit("building_exposures disagrees with the building columns on %s" % shown)
    full = sim.setting_series("setting")
    if not ((full.sum(axis=1, dtype=np.int64) == rec["exposures_building"].astype(np.int64) + rec["exposures_bus"]).all() and (full[:, 3] == rec["exposures_bus"]).all()):
        raise SystemExit("the rows by setting do not add up to the records")
    out["shares"] = {"whole_run": shares(full)}
    if rec["lockdown"].any():
        lock = int(np.argmax(rec["lockdown"])) + 1                   # the first step whose record has a lockdown: it holds from the next step on
        out["shares"].update(first_lockdown_step=lock, before_lockdown=shares(full[:lock]), from_lockdown_on=shares(full[lock:]),
                             during_lockdowns=shares(full[1:][rec["lockdown"][:-1] != 0]))
    hot = np.argsort(counts)[::-1][:5]
    out["hottest_buildings_whole_run"] = [{"building": int(b), "type": int(pop.building_type[b]), "area": int(pop.building_area[b]), "exposures": int(counts[b])} for b in hot]
    out["unexposed_or_index"] = int((setting == _lib.SETTING_NONE).sum())
    sim.close()
    path = a.out or os.path.join(ROOT, "profiles", "exposure_settings_%s.json" % a.preset)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
