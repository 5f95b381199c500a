"""Times forecast ensembles on a preset: members branched from a snapshot against the same members run from step 0, and the
snapshot and rollback calls alone.  Writes profiles/forecast_<preset>.json and prints it as one JSON line.

    python tools/forecast_ensemble.py PRESET [--steps N] [--repeats K] [--out PATH]

The method of tools/ensemble_times.py: every figure is perf_counter around the synchronised member (the rollback or restart,
the run with its own wait for the records, esim_synchronize), after one warm-up member, as the median of K (at least 7)
repeats with the smallest and the largest beside it; everything is taken on one commit in one process.  The members differ
in seed and lockdown threshold only, so a branch and a run from step 0 do the same kind of work behind the snapshot.
  forecast_0.4 / forecast_0.7   a member through the snapshot taken at 0.4 / 0.7 of the run: esim_rollback + the remaining steps
  from_step_0                    the same member through esim_restart + all N steps
  snapshot / rollback            the call alone + esim_synchronize
The stream model of the word copy: 8 B per citizen (a word read, a word written) over the 8 TB/s HBM peak."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from epidemicsimulator_amd import Population, Simulator  # noqa: E402

HBM_PEAK = 8.0e12


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "repeats": len(ms)}


def clock(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def member(k):
    return {"seed": 1000 + k, "lockdown_threshold": 0.003 + 0.0002 * (k % 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("preset")
    ap.add_argument("--steps", type=int, default=5000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out")
    a = ap.parse_args()
    repeats = max(7, a.repeats)
    pop = Population.synthetic(a.preset)
    sim = Simulator(pop)
    base = sim.params
    out = {"preset": a.preset, "n_citizens": int(pop.n_citizens), "steps": a.steps, "repeats": repeats,
           "word_copy_model_bytes": 8 * int(pop.n_citizens), "word_copy_model_ms_at_hbm_peak": round(8 * int(pop.n_citizens) / HBM_PEAK * 1e3, 5)}

    def from_zero(k):
        sim.restart(base, **member(k))
        sim.run(a.steps)
        sim.synchronize()

    from_zero(0)                                                     # warm-up
    out["from_step_0"] = summary([clock(lambda k=k: from_zero(k)) for k in range(1, repeats + 1)])
    for share in (0.4, 0.7):
        t = max(1, min(a.steps - 1, int(a.steps * share)))
        sim.restart(base)
        sim.run(t)
        sim.synchronize()
        snap = [clock(lambda: (sim.snapshot(), sim.synchronize())) for _ in range(repeats + 1)][1:]

        def branch(k):
            sim.rollback(**member(k))
            sim.run(a.steps - t)
            sim.synchronize()

        branch(0)                                                    # warm-up
        out["forecast_%.1f" % share] = dict(summary([clock(lambda k=k: branch(k)) for k in range(1, repeats + 1)]), snapshot_step=t)
        back = [clock(lambda: (sim.rollback(), sim.synchronize())) for _ in range(repeats + 1)][1:]
        out["snapshot_at_%.1f" % share] = summary(snap)
        out["rollback_at_%.1f" % share] = summary(back)
    sim.close()
    path = a.out or os.path.join(ROOT, "profiles", "forecast_%s.json" % a.preset)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
