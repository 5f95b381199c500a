"""Times the policy grids on a preset, every wall figure the time (perf_counter) around calls that end synchronised,
as the median of `repeats` repeats after one warm-up, with the smallest and the largest beside it:

  arms         esim_ensemble_arms with every output, for 2, 4 and 8 arms over 8, 32 and 64 kept members of
                 census   the census by home area (one row),
                 window   a weekly window by home area (168 rows of the Infected at the national peak);
               per case the whole call, the live cells and -- from a run of its own under `rocprofv3 --kernel-trace --stats`, one
               child process before this process opens the device (--no-trace leaves it out) -- the device time of k_arms alone.
  exceedance   esim_ensemble_exceedance with one threshold at the same members and window: k_members_exceed reads the same keys
               once, so it is the yardstick for the read side.  The ratio of the two kernels' times is written beside them, and
               the arms kernel's bytes -- 4 B x members per live cell read, 24 B x arms per window cell written -- over its time as
               a fraction of 8 TB/s.
  host         the route there was before: ensemble_members() to the host and the rule of tests/_arms_ref.py in numpy there,
               in the same process.  For the window it is timed at the smallest member count only, and once
               (--host-window-repeats).  The tool stops if the two routes differ.

The members are `distinct` runs (at most eight, other seeds), each folded several times until the store holds the member count,
as tools/ensemble_depth.py fills its store: the arms of such a grid are no policies, which costs the kernel what any keys cost.
Prints one JSON line; --out also writes it to a file (default profiles/ensemble_arms_<preset>.json).

    python tools/ensemble_arms.py [preset] [steps] [repeats] [--members 8 32 64] [--arms 2 4 8] [--host-window-repeats 1] [--no-trace] [--out FILE]"""
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
import _arms_ref as ref  # noqa: E402
from ensemble_depth import keep_members, setup  # noqa: E402
from ensemble_quantiles import timed  # noqa: E402

KINDS = ("census", "window")
TABLES = ("best", "sole", "regret", "sum", "totals")
TRACED_CALLS = 3
HBM_BYTES_PER_SECOND = 8e12


def case(sim, kind, window, burden_rows, steps, members, arms_list, repeats, host_repeats):
    keep_members(sim, kind, window, burden_rows, steps, members)
    out = {"members": members}
    _, out["exceedance_one_threshold"] = timed(lambda: sim.ensemble_exceedance((1,)), repeats)
    for arms in arms_list:
        got, st = timed(lambda: sim.ensemble_arms(arms), repeats)
        cells = int(got["best"][0].size)
        out.update(cells=cells, live_cells=got["live_cells"])
        entry = out["%d_arms" % arms] = dict(st, bytes_read=4 * members * got["live_cells"], bytes_written=24 * arms * cells)
        if host_repeats:
            stack = [None]

            def route():
                stack[0] = sim.ensemble_members()
                return ref.arms(stack[0], arms)
            host, h_st = timed(route, host_repeats)
            if not all((host[k] == got[k]).all() for k in TABLES):
                raise SystemExit("the device route and numpy over the members' planes differ (%s, %d members, %d arms)" % (kind, members, arms))
            entry["planes_to_the_host_then_numpy"] = dict(h_st, bytes_over_the_bus=4 * members * cells)
            entry["speedup"] = round(h_st["median_ms"] / st["median_ms"], 2)
    return out


def traced_child(preset, steps, member_counts, arms_list):
    """What runs under rocprofv3: per kind and member count the members kept, then three calls of the exceedance and of every
    number of arms, in the order trace() reads them back in."""
    sim, rec, window, burden_rows = setup(preset, steps)
    for kind in KINDS:
        for members in member_counts:
            keep_members(sim, kind, window, burden_rows, len(rec), members)
            for _ in range(TRACED_CALLS):
                sim.ensemble_exceedance((1,))
            for arms in arms_list:
                for _ in range(TRACED_CALLS):
                    sim.ensemble_arms(arms)
    sim.close()


def trace(preset, steps, member_counts, arms_list):
    """Device time per kernel: {"<kind>_<members>_members": {"k_members_exceed": ..., "<arms>_arms": ...}}, median, min and max in
    microseconds, the dispatches taken in the order of traced_child's calls."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "q", "--",
               sys.executable, os.path.abspath(__file__), preset, str(steps), "--members"] + [str(m) for m in member_counts] + ["--arms"] + [str(a) for a in arms_list] + ["--traced-child"]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=1100)
        if p.returncode != 0:
            return {"error": "rocprofv3 run failed (%d): %s" % (p.returncode, (p.stderr or p.stdout)[-400:])}
        f = glob.glob(os.path.join(d, "**", "*_kernel_trace.csv"), recursive=True)
        rows = list(csv.DictReader(open(f[0]))) if f else []
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    us = lambda name: [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if name in r.get("Kernel_Name", "")]
    main, exceed = us("k_arms<"), us("k_members_exceed")
    cases = len(KINDS) * len(member_counts)
    if len(main) != cases * len(arms_list) * TRACED_CALLS or len(exceed) != cases * TRACED_CALLS:
        return {"error": "%d dispatches of k_arms and %d of k_members_exceed in the trace, %d and %d expected" % (len(main), len(exceed), cases * len(arms_list) * TRACED_CALLS,
                                                                                                                 cases * TRACED_CALLS)}
    out, at, at_x = {}, 0, 0
    summary = lambda v: {"median_us": round(statistics.median(v), 3), "min_us": round(min(v), 3), "max_us": round(max(v), 3), "dispatches": len(v)}
    for kind in KINDS:
        for members in member_counts:
            entry = out["%s_%d_members" % (kind, members)] = {"k_members_exceed": summary(exceed[at_x:at_x + TRACED_CALLS])}
            at_x += TRACED_CALLS
            for arms in arms_list:
                entry["%d_arms" % arms] = summary(main[at:at + TRACED_CALLS])
                at += TRACED_CALLS
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("preset", nargs="?", default="york")
    ap.add_argument("steps", nargs="?", type=int, default=2000)
    ap.add_argument("repeats", nargs="?", type=int, default=7)
    ap.add_argument("--members", nargs="+", type=int, default=[8, 32, 64])
    ap.add_argument("--arms", nargs="+", type=int, default=[2, 4, 8])
    ap.add_argument("--host-window-repeats", type=int, default=1, help="repeats of the host route for the weekly window at the smallest member count (0: leave it out)")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--traced-child", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    if any(m % arms for m in a.members for arms in a.arms):
        raise SystemExit("every member count must be a multiple of every number of arms")
    if a.traced_child:
        return traced_child(a.preset, a.steps, a.members, a.arms)
    traces = {}
    if not a.no_trace:                                            # (before this process opens the device)
        traces = trace(a.preset, a.steps, a.members, a.arms)
        print("trace: %s" % json.dumps(traces), file=sys.stderr, flush=True)
    sim, rec, window, burden_rows = setup(a.preset, a.steps)
    pop = sim.population
    out = {"preset": a.preset, "n_citizens": pop.n_citizens, "n_areas": pop.n_areas, "steps": len(rec), "window": window,
           "what": "wall ms around synchronised calls; median (min, max) of `repeats` after one warm-up; the host route: ensemble_members() and tests/_arms_ref.py in numpy; "
                   "device us per kernel from rocprofv3 --kernel-trace in a child process; bytes: 4 B x members per live cell read, 24 B x arms per window cell written"}
    if "error" in traces:
        out["trace_error"] = traces["error"]
    for kind in KINDS:
        for members in a.members:
            if kind == "window":
                host = a.host_window_repeats if members == min(a.members) else 0
            else:
                host = a.repeats
            key = "%s_%d_members" % (kind, members)
            r = out[key] = case(sim, kind, window, burden_rows, len(rec), members, a.arms, a.repeats, host)
            if key in traces:
                x_us = traces[key]["k_members_exceed"]["median_us"]
                r["exceedance_one_threshold"]["device_time_k_members_exceed"] = traces[key]["k_members_exceed"]
                for arms in a.arms:
                    e, t = r["%d_arms" % arms], traces[key]["%d_arms" % arms]
                    e["device_time_k_arms"] = t
                    e["k_arms_over_k_members_exceed"] = round(t["median_us"] / x_us, 3) if x_us else None
                    e["share_of_8_TB_per_second"] = round((e["bytes_read"] + e["bytes_written"]) / (t["median_us"] * 1e-6) / HBM_BYTES_PER_SECOND, 4) if t["median_us"] else None
            print("%s: %s" % (key, json.dumps(r)), file=sys.stderr, flush=True)
    sim.close()
    path = a.out or os.path.join(ROOT, "profiles", "ensemble_arms_%s.json" % a.preset)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
