#!/usr/bin/env python3
"""Ensembles on several contexts, measured: members per second of Ensemble.run with devices=None, (0,), (0, 0) and,
where there are more devices, (0, 1, ...); the time of one esim_ensemble_merge of the shape the run used and of one over a
168-row weekly window, beside the bytes it moves; the time of esim_ensemble_save and esim_ensemble_load.  Wall times around
calls that end in a wait for the stream, medians (min .. max) of `--repeats` runs after a warm-up run.

    python tools/ensemble_devices.py --world york --steps 5000 --members 8 32 --out profiles/ensemble_devices_york.json
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from epidemicsimulator_amd import Ensemble, Population, Simulator, _lib      # noqa: E402


def hip_device_count():
    """The devices the HIP runtime of libesim sees, asked of that runtime as this process has it loaded."""
    import ctypes
    _lib.load()
    with open("/proc/self/maps") as fh:
        paths = sorted({line.split()[-1] for line in fh if "libamdhip64" in line})
    n = ctypes.c_int(0)
    if not paths or ctypes.CDLL(paths[0]).hipGetDeviceCount(ctypes.byref(n)) != 0:
        return 0
    return n.value


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def timed(call, repeats, before=None):
    """Wall seconds of call(), `repeats` times behind one warm-up; before() runs in front of each, untimed."""
    out = []
    for k in range(repeats + 1):
        if before is not None:
            before()
        t0 = time.perf_counter()
        call()
        out.append(time.perf_counter() - t0)
    return spread(out[1:])


def members_per_second(pop, params, devices, members, steps, repeats):
    ens = Ensemble(pop, params, devices=devices)
    try:
        area = dict(where="home", quantiles=(0.5,))
        t = timed(lambda: ens.run(Ensemble.seeds(members), steps, area=area), repeats)
    finally:
        ens.close()
    return {"seconds": t, "members_per_second": {k: members / t[j] for k, j in (("median", "median"), ("min", "max"), ("max", "min"))},
            "ms_per_member": 1e3 * t["median"] / members}


def merge_times(pop, params, steps, members, repeats, rows):
    """One merge of `members` members kept -- census by home area (rows=None) or a series of `rows` weekly rows -- and save / load."""
    a, b = Simulator(pop, params), Simulator(pop, params)
    try:
        def begin(sim, capacity):
            if rows is None:
                sim.ensemble_begin("home")
            else:
                sim.ensemble_begin_series("home", "incidence", first_step=max(1, steps - rows + 1), n_rows=min(rows, steps), stride=1)   # (the last week, a row an hour)
            sim.ensemble_keep_members(capacity)

        b.run(steps)
        begin(b, members)
        for _ in range(members):
            b.ensemble_fold()
        b.synchronize()
        a.run(steps)

        def fresh():
            begin(a, members)
            a.synchronize()

        def merge():
            a.ensemble_merge(b)
            a.synchronize()

        out = {"merge_s": timed(merge, repeats, fresh)}
        blob = b.ensemble_save()
        out["bytes"] = len(blob)
        out["save_s"] = timed(b.ensemble_save, repeats)

        def load():
            a.ensemble_load(blob)
            a.synchronize()

        out["load_s"] = timed(load, repeats, fresh)
        out["merge_GB_per_s"] = len(blob) / out["merge_s"]["median"] / 1e9
        out["cells"] = (rows or 1) * pop.n_areas
        return out
    finally:
        a.close()
        b.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--world", default="york")
    ap.add_argument("--steps", type=int, default=5000)
    ap.add_argument("--members", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n_dev = hip_device_count()
    pop = Population.synthetic(args.world)
    params = _lib.default_params(max_steps=args.steps)
    layouts = {"None": None, "(0,)": (0,), "(0, 0)": (0, 0)}
    if n_dev > 1:
        layouts[str(tuple(range(n_dev)))] = tuple(range(n_dev))
    doc = {"world": args.world, "citizens": pop.n_citizens, "areas": pop.n_areas, "steps": args.steps, "devices_present": n_dev, "repeats": args.repeats,
           "peer_transport_exercised": n_dev > 1, "run": {}, "merge": {}}
    for m in args.members:
        doc["run"][str(m)] = {name: members_per_second(pop, params, dev, m, args.steps, args.repeats) for name, dev in layouts.items()}
        doc["merge"][str(m)] = {"census": merge_times(pop, params, args.steps, m, args.repeats, None), "weekly_168_rows": merge_times(pop, params, args.steps, m, args.repeats, 168)}
        print(json.dumps({"members": m, "run": {k: v["ms_per_member"] for k, v in doc["run"][str(m)].items()},
                          "merge_ms": {k: 1e3 * v["merge_s"]["median"] for k, v in doc["merge"][str(m)].items()}}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(doc, fh, indent=1)


if __name__ == "__main__":
    main()
