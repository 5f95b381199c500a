"""Times the ensemble distances on a preset, every wall figure the time (perf_counter) around calls that end
synchronised, as the median of `repeats` repeats after one warm-up, with the smallest and the largest beside it:

  l1, differ   esim_ensemble_distances with either metric, over 8, 32 and 64 kept members of
                 census   the census by home area (one row),
                 window   a weekly window by home area (168 rows of the Infected at the national peak),
                 burden   the rows of burden_series("occupancy") by all (one column);
               per case the whole call, the live cells, the share of the tiles summed in 32 bits, and -- from a run of its own
               under `rocprofv3 --kernel-trace --stats`, one child process before this process opens the device (--no-trace
               leaves it out) -- the device time of k_dist and k_dist_mirror and the pair-cells a second it amounts to
               (live cells x C(members, 2) / kernel time).
  host         beside them the route there was before: ensemble_members() to the host and the sums of tests/_dist_ref.py in
               numpy there, in the same process.  It is quadratic in the members and linear in the cells: for the window it is
               timed at the smallest member count only, and once (--host-window-repeats).  The tool stops if the two routes differ.

The members are `distinct` runs (at most eight, other seeds), each folded several times until the store holds the member count,
as tools/ensemble_depth.py fills its store: repeated members are at distance 0, which costs the kernel what any pair costs.
Prints one JSON line; --out also writes it to a file (default profiles/ensemble_distances_<preset>.json).

    python tools/ensemble_distances.py [preset] [steps] [repeats] [--members 8 32 64] [--host-window-repeats 1] [--no-trace] [--out FILE]"""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _dist_ref as ref  # noqa: E402
from ensemble_depth import keep_members, setup  # noqa: E402
from ensemble_quantiles import timed  # noqa: E402

KINDS = ("burden", "census", "window")
METRICS = ("l1", "differ")
TRACED_CALLS = 3


def case(sim, kind, window, burden_rows, steps, members, repeats, host_repeats):
    keep_members(sim, kind, window, burden_rows, steps, members)
    out = {"members": members, "pairs": members * (members - 1) // 2}
    got = {}
    for metric in METRICS:
        got[metric], st = timed(lambda: sim.ensemble_distances(metric), repeats)
        info = sim.ensemble_distances_info()
        out[metric] = dict(st, tiles=info["tiles"], share_of_tiles_in_32_bits=round(info["tiles_32bit"] / info["tiles"], 4) if info["tiles"] else None)
    out.update(cells=got["l1"]["cells"], live_cells=got["l1"]["live_cells"])
    if host_repeats:
        def route():
            stack = sim.ensemble_members()
            return {metric: ref.distances(stack, metric) for metric in METRICS}
        host, h_st = timed(route, host_repeats)
        if not all((host[metric] == got[metric]["distances"]).all() for metric in METRICS):
            raise SystemExit("the device route and numpy over the members' planes differ (%s, %d members)" % (kind, members))
        out["planes_to_the_host_then_numpy"] = dict(h_st, bytes_over_the_bus=4 * members * out["cells"])
        out["speedup_both_metrics"] = round(h_st["median_ms"] / (out["l1"]["median_ms"] + out["differ"]["median_ms"]), 2)
    return out


def traced_child(preset, steps, member_counts):
    """What runs under rocprofv3: per kind and member count the members kept, then three calls with either metric, in the order
    trace() reads them back in."""
    sim, rec, window, burden_rows = setup(preset, steps)
    for kind in KINDS:
        for members in member_counts:
            keep_members(sim, kind, window, burden_rows, len(rec), members)
            for metric in METRICS:
                for _ in range(TRACED_CALLS):
                    sim.ensemble_distances(metric)
    sim.close()


def trace(preset, steps, member_counts):
    """Device time per kernel of the feature: {"<kind>_<members>_members": {metric: median, min and max in microseconds of
    k_dist, and of k_dist_mirror}}, the dispatches taken in the order of traced_child's calls."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "q", "--",
               sys.executable, os.path.abspath(__file__), preset, str(steps), "--members"] + [str(m) for m in member_counts] + ["--traced-child"]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=1100)
        if p.returncode != 0:
            return {"error": "rocprofv3 run failed (%d): %s" % (p.returncode, (p.stderr or p.stdout)[-400:])}
        f = glob.glob(os.path.join(d, "**", "*_kernel_trace.csv"), recursive=True)
        rows = list(csv.DictReader(open(f[0]))) if f else []
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    us = lambda name: [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if name in r.get("Kernel_Name", "")]
    main, mirror = us("k_dist<"), us("k_dist_mirror")
    want = len(KINDS) * len(member_counts) * len(METRICS) * TRACED_CALLS
    if len(main) != want or len(mirror) != want:
        return {"error": "%d dispatches of k_dist and %d of k_dist_mirror in the trace, %d expected" % (len(main), len(mirror), want)}
    out, at = {}, 0
    summary = lambda v: {"median_us": round(statistics.median(v), 3), "min_us": round(min(v), 3), "max_us": round(max(v), 3), "dispatches": len(v)}
    for kind in KINDS:
        for members in member_counts:
            entry = out["%s_%d_members" % (kind, members)] = {}
            for metric in METRICS:
                entry[metric] = {"k_dist": summary(main[at:at + TRACED_CALLS]), "k_dist_mirror": summary(mirror[at:at + TRACED_CALLS])}
                at += TRACED_CALLS
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("preset", nargs="?", default="york")
    ap.add_argument("steps", nargs="?", type=int, default=2000)
    ap.add_argument("repeats", nargs="?", type=int, default=7)
    ap.add_argument("--members", nargs="+", type=int, default=[8, 32, 64])
    ap.add_argument("--host-window-repeats", type=int, default=1, help="repeats of the host route for the weekly window at the smallest member count (0: leave it out)")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--traced-child", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.traced_child:
        return traced_child(a.preset, a.steps, a.members)
    traces = {}
    if not a.no_trace:                                            # (before this process opens the device)
        traces = trace(a.preset, a.steps, a.members)
        print("trace: %s" % json.dumps(traces), file=sys.stderr, flush=True)
    sim, rec, window, burden_rows = setup(a.preset, a.steps)
    pop = sim.population
    out = {"preset": a.preset, "n_citizens": pop.n_citizens, "n_areas": pop.n_areas, "steps": len(rec), "window": window, "burden_rows": burden_rows,
           "what": "wall ms around synchronised calls; median (min, max) of `repeats` after one warm-up; the host route: ensemble_members() and tests/_dist_ref.py in numpy; "
                   "device us per kernel from rocprofv3 --kernel-trace in a child process"}
    if "error" in traces:
        out["trace_error"] = traces["error"]
    for kind in KINDS:
        for members in a.members:
            if kind == "window":
                host = a.host_window_repeats if members == min(a.members) else 0
            else:
                host = a.repeats
            key = "%s_%d_members" % (kind, members)
            r = out[key] = case(sim, kind, window, burden_rows, len(rec), members, a.repeats, host)
            for metric in METRICS:
                if key in traces:
                    r[metric]["device_time_per_kernel"] = traces[key][metric]
                    us = traces[key][metric]["k_dist"]["median_us"]
                    r[metric]["pair_cells_per_second"] = float("%.4g" % (r["live_cells"] * r["pairs"] / (us * 1e-6))) if us else None
            print("%s: %s" % (key, json.dumps(r)), file=sys.stderr, flush=True)
    sim.close()
    path = a.out or os.path.join(ROOT, "profiles", "ensemble_distances_%s.json" % a.preset)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
