"""Times the ensemble calls on a preset: going back to step 0 by esim_reset and by esim_restart, esim_ensemble_fold, and one
member end to end both ways.  Writes profiles/ensemble_restart_<preset>.json and prints it as one JSON line.

    python tools/ensemble_times.py PRESET MEMBERS [--steps N] [--parent-lib PATH] [--no-trace]

Every wall figure is perf_counter around calls of the C ABI alone (ctypes, no Simulator object around them) that end in
esim_synchronize or in esim_run's own wait, after one warm-up member, as the median of MEMBERS (at least 7) repeats with the
smallest and the largest beside it; reset and restart alternate in one loop.
--parent-lib: a libesim.so built from the parent commit; its esim_reset is timed in the same loop, on a context of its own
with the same population.  Unless --no-trace, a child process of its own then runs MEMBERS restarts under
`rocprofv3 --kernel-trace --memory-copy-trace --stats`: the restart kernels' device time, the bytes they must move (8 B per
citizen -- the word read and written -- plus the cleared tables, from the sizes) over the 8 TB/s HBM peak, and the copies the
restarts issued by direction."""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from epidemicsimulator_amd import Population, Simulator, _lib  # noqa: E402  (Simulator: the traced child)

HBM_PEAK = 8.0e12
RESTART_KERNELS = ("k_restart_words", "k_restart_books")


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "repeats": len(ms)}


def clock(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


class RawContext:
    """A context of its own through the C ABI alone (no Simulator around it, whose record keeping would be timed too): this
    build's library, or another build's (--parent-lib), with the same population and parameters."""

    def __init__(self, path, pop, params):
        self.lib = C.CDLL(path)
        vp = C.c_void_p
        sigs = [("esim_create", [C.POINTER(_lib.Params), C.POINTER(vp)]), ("esim_upload_population", [vp, C.POINTER(_lib.PopulationStruct)]),
                ("esim_reset", [vp]), ("esim_synchronize", [vp]), ("esim_destroy", [vp]),
                ("esim_run", [vp, C.c_uint32, C.c_int, C.POINTER(_lib.StepResult), C.POINTER(C.c_uint32)])]
        if hasattr(self.lib, "esim_restart"):
            sigs += [("esim_restart", [vp, C.POINTER(_lib.Params)]), ("esim_ensemble_begin", [vp, C.c_int, C.c_uint32, C.c_uint32]), ("esim_ensemble_fold", [vp])]
        for name, args in sigs:
            getattr(self.lib, name).argtypes = args
            getattr(self.lib, name).restype = None if name == "esim_destroy" else C.c_int
        self.params = params
        self.ctx = vp()
        self.ok(self.lib.esim_create(C.byref(params), C.byref(self.ctx)))
        ps = pop.as_struct()
        self.ok(self.lib.esim_upload_population(self.ctx, C.byref(ps)))
        self.buf = (_lib.StepResult * max(1, int(params.max_steps)))()

    def ok(self, rc):
        if rc:
            raise RuntimeError("libesim: error %d" % rc)

    def sync(self):
        self.ok(self.lib.esim_synchronize(self.ctx))

    def reset(self):
        self.ok(self.lib.esim_reset(self.ctx))

    def restart(self):
        self.ok(self.lib.esim_restart(self.ctx, C.byref(self.params)))

    def fold(self):
        self.ok(self.lib.esim_ensemble_fold(self.ctx))

    def run(self, n):
        done = C.c_uint32(0)
        self.ok(self.lib.esim_run(self.ctx, n, 0, self.buf, C.byref(done)))

    def close(self):
        self.lib.esim_destroy(self.ctx)


def traced_child(preset, members):
    """What runs under rocprofv3: an upload, one census as a marker behind the set-up's copies, then `members` restarts."""
    pop = Population.synthetic(preset)
    sim = Simulator(pop)
    sim.area_census("home")
    for i in range(members):
        sim.restart(seed=1000 + i)
        sim.synchronize()
    sim.close()


def trace(preset, members, pop):
    out = {"members": members}
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--memory-copy-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "ens", "--",
               sys.executable, os.path.abspath(__file__), preset, str(members), "--traced-child"]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if p.returncode != 0:
            return {"error": "rocprofv3 run failed (%d): %s" % (p.returncode, (p.stderr or p.stdout)[-400:])}

        def rows(suffix):
            f = glob.glob(os.path.join(d, "**", "*" + suffix), recursive=True)
            return list(csv.DictReader(open(f[0]))) if f else []

        kernels = {}
        for r in rows("_kernel_stats.csv"):
            name = r["Name"].split("(")[0]
            if name in RESTART_KERNELS:
                kernels[name] = {"calls": int(r["Calls"]), "mean_us": round(float(r["AverageNs"]) / 1e3, 3), "min_us": round(float(r["MinNs"]) / 1e3, 3),
                                 "max_us": round(float(r["MaxNs"]) / 1e3, 3)}
        out["kernels"] = kernels
        # the copies behind the marker (the first k_area_census): those of the restarts, besides the census' own two read-backs
        kt = rows("_kernel_trace.csv")
        marks = [int(r["End_Timestamp"]) for r in kt if r.get("Kernel_Name", "").startswith("k_area_census")]
        # the device work of a whole restart: first kernel or copy of it to the last (k_restart_words .. the log's copy), from the kernels
        words = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in kt if r.get("Kernel_Name", "").startswith("k_restart_words"))
        books = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in kt if r.get("Kernel_Name", "").startswith("k_restart_books"))
        if words and len(words) == len(books):
            span = [(b[1] - w[0]) / 1e3 for w, b in zip(words, books)]
            out["words_start_to_books_end_us"] = {"median": round(statistics.median(span), 3), "min": round(min(span), 3), "max": round(max(span), 3)}
        if marks:                                                  # every dispatch behind the marker: what the restarts ran on the device
            after = {}
            for r in kt:
                if int(r["Start_Timestamp"]) > marks[0]:
                    name = r.get("Kernel_Name", "?").split("(")[0]
                    after[name] = after.get(name, 0) + 1
            out["dispatches_after_setup"] = after
        copies = {}
        if marks:
            for r in rows("_memory_copy_trace.csv"):
                if int(r["Start_Timestamp"]) > marks[0]:
                    key = r.get("Direction", "?")
                    copies[key] = copies.get(key, 0) + 1
        out["copies_after_setup_by_direction"] = copies
    n = pop.n_citizens
    cleared = 4 * 4 * (pop.n_buildings + pop.n_rooms) + 8 * (5000 + 2) + 64 * (5000 + 1)        # marks (4 ring slots; routes apart), exp_step, records
    out["model_bytes"] = {"citizen_words_read_and_written": 8 * n, "cleared_tables_without_route_flags": cleared}
    if "k_restart_words" in kernels:
        s = kernels["k_restart_words"]["mean_us"] * 1e-6
        out["k_restart_words_frac_hbm_peak"] = round(8 * n / s / HBM_PEAK, 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("preset")
    ap.add_argument("members", type=int)
    ap.add_argument("--steps", type=int, default=5000)
    ap.add_argument("--parent-lib")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--traced-child", action="store_true")
    a = ap.parse_args()
    members = max(7, a.members)
    if a.traced_child:
        return traced_child(a.preset, members)
    pop = Population.synthetic(a.preset)
    out = {"preset": a.preset, "n_citizens": pop.n_citizens, "n_areas": pop.n_areas, "steps": a.steps, "repeats": members,
           "what": "wall ms around C ABI calls ending in esim_synchronize (or esim_run's own wait); median (min, max) after one warm-up member; reset and restart alternate in one loop"}
    if not a.no_trace:
        out["trace"] = trace(a.preset, members, pop)              # (before this process opens the device)
        print("trace done: %s" % json.dumps(out["trace"]), file=sys.stderr, flush=True)
    params = _lib.default_params(max_steps=max(a.steps, 1))
    sim = RawContext(_lib.LIB_PATH, pop, params)
    parent = RawContext(a.parent_lib, pop, params) if a.parent_lib else None
    sim.ok(sim.lib.esim_ensemble_begin(sim.ctx, _lib.AREA_HOME, 0b1110, 1))
    print("contexts ready", file=sys.stderr, flush=True)
    t = {k: [] for k in ("reset", "restart", "fold", "member_reset", "member_restart", "run", "parent_reset", "parent_member_reset")}
    for i in range(members + 1):
        sim.reset(); sim.run(a.steps)                              # a state to go back from
        row = {"reset": clock(lambda: (sim.reset(), sim.sync()))}
        sim.run(a.steps)
        row["restart"] = clock(lambda: (sim.restart(), sim.sync()))
        row["member_reset"] = clock(lambda: (sim.reset(), sim.run(a.steps)))        # (esim_run ends with its own wait)
        row["member_restart"] = clock(lambda: (sim.restart(), sim.run(a.steps)))
        row["fold"] = clock(lambda: (sim.fold(), sim.sync()))
        sim.reset()
        row["run"] = clock(lambda: sim.run(a.steps))
        if parent:
            parent.reset(); parent.run(a.steps)
            row["parent_reset"] = clock(lambda: (parent.reset(), parent.sync()))
            row["parent_member_reset"] = clock(lambda: (parent.reset(), parent.run(a.steps)))
        if i > 0:                                                  # member 0 warms everything up
            for k, v in row.items():
                t[k].append(v)
    out["esim_reset_sync"] = summary(t["reset"])
    out["esim_restart_sync"] = summary(t["restart"])
    out["esim_ensemble_fold_sync"] = summary(t["fold"])
    out["run_alone"] = summary(t["run"])
    out["member_reset_then_run"] = summary(t["member_reset"])
    out["member_restart_then_run"] = summary(t["member_restart"])
    if parent:
        out["parent_esim_reset_sync"] = summary(t["parent_reset"])
        out["parent_member_reset_then_run"] = summary(t["parent_member_reset"])
        out["restart_vs_parent_reset"] = round(out["parent_esim_reset_sync"]["median_ms"] / out["esim_restart_sync"]["median_ms"], 2)
        parent.close()
    out["restart_vs_reset"] = round(out["esim_reset_sync"]["median_ms"] / out["esim_restart_sync"]["median_ms"], 2)
    sim.close()
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "ensemble_restart_%s.json" % a.preset), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
