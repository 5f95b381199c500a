"""Times the ensemble maps of transmission on a preset: one member is run, and its cohort reproduction rows and its exposures by
setting, both by household area with weekly rows (stride 168) over the whole run, go two ways, alternated in one process:

  (a) the host route a user had before: esim_reproduction_series(ESIM_AREA_HOME) / esim_setting_series(ESIM_AREA_HOME) with the
      same window into host memory (the yardstick; the numpy fold a user would add on top is not timed);
  (b) esim_ensemble_begin_reproduction / esim_ensemble_begin_settings once, then esim_ensemble_fold, which ends with its own
      stream wait.

The tool stops if the accumulators after the first fold differ from the numpy fold of the yardstick's rows.  A figure is the
wall time (perf_counter) around one call, as the median of `repeats` calls after one warm-up call, with the smallest and the
largest beside it.  The fold kernels' own device time is taken between HIP events by tests/native/ratio_probe.hip, compiled
here, which runs k_ensemble_fold_ratio and k_ensemble_fold_rows alone on the member's real rows; the bytes a launch moves are
counted from those rows by the kernels' skip rules and set against that time as a share of the 8 TB/s HBM peak.  Prints one JSON
line; --out also writes it to a file (default profiles/ensemble_transmission_<preset>.json).

    python tools/ensemble_transmission.py [preset] [steps] [repeats] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from epidemicsimulator_amd import Population, Simulator, _lib  # noqa: E402

HBM_PEAK = 8.0e12          # bytes per second, MI355X
WEEK = 168
u32p = C.POINTER(C.c_uint32)


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "repeats": len(ms)}


def alternated(first, second, repeats):
    """Wall ms of two calls taken in turns, after one warm-up of each."""
    first(), second()
    a, b = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        first()
        t1 = time.perf_counter()
        second()
        t2 = time.perf_counter()
        a.append((t1 - t0) * 1e3)
        b.append((t2 - t1) * 1e3)
    return stats(a), stats(b)


def build_probe(directory):
    out = os.path.join(directory, "libratio_probe.so")
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-I", os.path.join(ROOT, "epidemicsimulator_amd", "csrc"),
           "-I", os.path.join(ROOT, "include"), "-o", out, os.path.join(ROOT, "tests", "native", "ratio_probe.hip")]
    done = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if done.returncode != 0:
        raise RuntimeError("hipcc: " + done.stderr[-400:])
    lib = C.CDLL(out)
    lib.ratio_probe.restype = lib.rows_probe.restype = C.c_int
    lib.ratio_probe.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64] + [C.c_uint32] * 5 + [C.c_void_p] * 5
    lib.rows_probe.argtypes = [C.c_void_p, C.c_uint64] + [C.c_uint32] * 3 + [C.c_void_p] * 5
    return lib


def fours(a):
    """The cells in whole groups of four, [groups, 4] (the up to three cells of the tail move next to nothing)."""
    a = a.ravel()
    return a[:a.size - a.size % 4].reshape(-1, 4)


def ratio_bytes(c, o, min_cohort, r):
    """Bytes one launch of k_ensemble_fold_ratio loads and stores for these planes, by its skip rules."""
    c4, o4 = fours(c).astype(np.uint64), fours(o).astype(np.uint64)
    defined = c4 >= min_cohort
    hit = defined & (o4 * np.uint64(r[1]) >= c4 * np.uint64(r[0]))
    pairs = int(((c4[:, :2] | o4[:, :2]).any(1)).sum() + ((c4[:, 2:] | o4[:, 2:]).any(1)).sum())
    return {"planes": 8 * c.size, "defined": 32 * int(defined.any(1).sum()), "hit": 32 * int(hit.any(1).sum()), "sums": 160 * pairs,
            "groups_of_four_all_zero_share": round(float((~(c4 | o4).any(1)).mean()), 5)}


def rows_bytes(x, min_cases):
    """The same for k_ensemble_fold_rows."""
    x4 = fours(x)
    pairs = int(x4[:, :2].any(1).sum() + x4[:, 2:].any(1).sum())
    return {"plane": 4 * x.size, "hit": 32 * int((x4 >= min_cases).any(1).sum()), "sums": 64 * pairs, "zero_cell_share": round(float((x == 0).mean()), 5)}


def kernel_time(call, repeats, moved):
    """Device ms of one launch between HIP events, median (min, max) of `repeats` after a warm-up, and the bytes against it."""
    ms = C.c_float(0)
    times = []
    for i in range(repeats + 1):
        rc = call(C.byref(ms))
        if rc != 0:
            raise RuntimeError("probe returned %d" % rc)
        if i:
            times.append(float(ms.value))
    out = stats(times)
    total = sum(v for k, v in moved.items() if not k.endswith("share"))
    out.update(bytes_moved=total, bytes_by_part=moved, gb_per_s=round(total / (out["median_ms"] * 1e-3) / 1e9, 1),
               share_of_hbm_peak=round(total / (out["median_ms"] * 1e-3) / HBM_PEAK, 4))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("preset", nargs="?", default="york")
    ap.add_argument("steps", nargs="?", type=int, default=5000)
    ap.add_argument("repeats", nargs="?", type=int, default=7)
    ap.add_argument("--out")
    a = ap.parse_args()
    pop = Population.synthetic(a.preset)
    out = {"preset": a.preset, "n_citizens": pop.n_citizens, "n_areas": pop.n_areas, "library": os.path.basename(_lib.LIB_PATH),
           "what": "wall ms around one synchronised call, the yardstick and the fold in turns; median (min, max) of `repeats` calls after one warm-up call; kernels: device ms between HIP events"}
    sim = Simulator(pop, _lib.default_params(max_steps=max(a.steps, 5000)))
    t0 = time.perf_counter()
    rec = sim.run(a.steps)
    n = len(rec)
    lib, ctx = sim.lib, sim._ctx
    out.update(steps=n, run_ms=round((time.perf_counter() - t0) * 1e3, 2),
               log_entries=int(rec["exposures_building"].sum(dtype=np.int64) + rec["exposures_bus"].sum(dtype=np.int64)) + len(sim.seeds()))
    min_cohort, r, min_cases = 1, (1, 1), 1
    # ---- the cohort reproduction rows ----
    win = dict(first_step=0, n_rows=n // WEEK + 1, stride=WEEK)
    cells = win["n_rows"] * pop.n_areas
    cases, off = np.zeros((win["n_rows"], pop.n_areas), np.uint32), np.zeros((win["n_rows"], pop.n_areas), np.uint32)

    def series_r():
        _lib.check(lib.esim_reproduction_series(ctx, _lib.AREA_HOME, win["first_step"], win["n_rows"], win["stride"], cases.ctypes.data_as(u32p), off.ctypes.data_as(u32p)), ctx)

    def fold():
        _lib.check(lib.esim_ensemble_fold(ctx), ctx)
        _lib.check(lib.esim_synchronize(ctx), ctx)
    sim.ensemble_begin_reproduction("home", min_cohort=min_cohort, r=r, **win)
    series_r()
    fold()
    got = sim.ensemble_read_reproduction()
    c64, o64 = cases.astype(np.uint64), off.astype(np.uint64)
    want = {"defined": (cases >= min_cohort), "hit": (cases >= min_cohort) & (o64 * np.uint64(r[1]) >= c64 * np.uint64(r[0])), "sum_cases": c64, "sum_offspring": o64,
            "sumsq_cases": c64 * c64, "sumsq_offspring": o64 * o64, "sum_cross": c64 * o64}
    if got["members"] != 1 or not all((got[k] == want[k]).all() for k in want):
        raise SystemExit("the accumulators of the reproduction kind differ from the numpy fold of esim_reproduction_series")
    if ((off > 0) & (cases == 0)).any():
        raise SystemExit("a cell has offspring without cases")
    sim.ensemble_begin_reproduction("home", min_cohort=min_cohort, r=r, **win)
    y, f = alternated(series_r, fold, a.repeats)
    weekly_cases, weekly_off = cases.sum(1, dtype=np.int64), off.sum(1, dtype=np.int64)
    out["reproduction"] = dict(win, cells=cells, reproduction_series_to_host=y, ensemble_fold=f, fold_over_yardstick=round(f["median_ms"] / y["median_ms"], 3),
                               bytes_the_yardstick_copies_out=8 * cells, cells_with_cases=int((cases > 0).sum()), cells_with_r_at_least_1=int(want["hit"].sum()),
                               pooled_r_by_week=[round(float(o) / float(c), 3) if c else None for c, o in zip(weekly_cases, weekly_off)])
    print("reproduction: %s" % json.dumps(out["reproduction"]), file=sys.stderr, flush=True)
    # ---- the exposures by setting ----
    s_win = dict(first_step=1, n_rows=(n - 1) // WEEK + 1, stride=WEEK)
    s_cells = s_win["n_rows"] * pop.n_areas
    x = np.zeros((s_win["n_rows"], pop.n_areas), np.uint32)

    def series_s():
        _lib.check(lib.esim_setting_series(ctx, _lib.AREA_HOME, 0xF, s_win["first_step"], s_win["n_rows"], s_win["stride"], x.ctypes.data_as(u32p)), ctx)
    sim.ensemble_begin_settings("home", None, min_cases=min_cases, **s_win)
    series_s()
    fold()
    got = sim.ensemble_read_series()
    x64 = x.astype(np.uint64)
    if got["members"] != 1 or not ((got["hit"] == (x >= min_cases)).all() and (got["sum"] == x64).all() and (got["sumsq"] == x64 * x64).all()):
        raise SystemExit("the accumulators of the settings kind differ from the numpy fold of esim_setting_series")
    sim.ensemble_begin_settings("home", None, min_cases=min_cases, **s_win)
    y, f = alternated(series_s, fold, a.repeats)
    out["settings"] = dict(s_win, cells=s_cells, setting_series_to_host=y, ensemble_fold=f, fold_over_yardstick=round(f["median_ms"] / y["median_ms"], 3),
                           bytes_the_yardstick_copies_out=4 * s_cells, exposures=int(x.sum(dtype=np.int64)))
    print("settings: %s" % json.dumps(out["settings"]), file=sys.stderr, flush=True)
    sim.close()
    # ---- the fold kernels alone, on the member's rows ----
    try:
        with tempfile.TemporaryDirectory() as d:
            probe = build_probe(d)
            members = np.zeros(1, np.uint32)
            words, sums = [np.zeros(cells, np.uint32) for _ in range(2)], np.zeros((5, cells), np.uint64)
            out["k_ensemble_fold_ratio"] = kernel_time(
                lambda ms: probe.ratio_probe(cases.ctypes.data, off.ctypes.data, cells, 1, 0, min_cohort, r[0], r[1], members.ctypes.data, words[0].ctypes.data,
                                             words[1].ctypes.data, sums.ctypes.data, ms), a.repeats, ratio_bytes(cases, off, min_cohort, r))
            hit, tot, sq = np.zeros(s_cells, np.uint32), np.zeros(s_cells, np.uint64), np.zeros(s_cells, np.uint64)
            out["k_ensemble_fold_rows"] = kernel_time(
                lambda ms: probe.rows_probe(x.ctypes.data, s_cells, 1, 0, min_cases, members.ctypes.data, hit.ctypes.data, tot.ctypes.data, sq.ctypes.data, ms),
                a.repeats, rows_bytes(x, min_cases))
    except (RuntimeError, OSError, subprocess.SubprocessError) as e:
        out["kernels"] = {"error": str(e)}
    path = a.out or os.path.join(ROOT, "profiles", "ensemble_transmission_%s.json" % a.preset)
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
