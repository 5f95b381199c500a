"""Runs a preset with five-year age bands as groups and reports its work place and school outbreaks: the size tables of the
three kinds of place (esim_place_sizes), the per-place arrays (esim_place_outbreaks) and the secondary attack rate of the work
places and of the school rooms, in one cell and by age band of the case and of the contact (esim_place_sar) -- and times the
calls, with esim_mixing_matrix (which shares the tree replay with the attack rate) beside them for scale.  Prints one JSON line;
--out also writes it to a file (default profiles/place_outbreaks_<preset>.json).

    python tools/place_outbreaks.py [preset] [steps] [--repeats 9] [--variant NAME=LIBRARY ...] [--out FILE]

Every --variant names another build of the library (make -C epidemicsimulator_amd/csrc places-tile-1024: the product's
sources with -DPLACE_TILE=...; or the library of another commit): the same run is made on a second context of that build in the same process, its esim_place_sar
is checked against the product's, and the two are timed in turns -- a warm-up call of each, then `repeats` times one call of
the product and one of the variant.  Every time is the time between two device events recorded on the null stream around one
library call (the calls are synchronous: they end with their own stream wait), as the median with the smallest and the largest
beside it; the wall time of the product's calls is printed beside it."""
import argparse
import ctypes as C
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


class DeviceClock:
    """Two HIP events on the null stream around a call."""

    def __init__(self):
        try:
            self.hip = C.CDLL("libamdhip64.so")
        except OSError:
            self.hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
        self.ev = [C.c_void_p(), C.c_void_p()]
        for e in self.ev:
            self._ok(self.hip.hipEventCreate(C.byref(e)))

    @staticmethod
    def _ok(code):
        if code != 0:
            raise SystemExit("HIP error %d from the event clock" % code)

    def ms(self, fn):
        self._ok(self.hip.hipEventRecord(self.ev[0], None))
        out = fn()
        self._ok(self.hip.hipEventRecord(self.ev[1], None))
        self._ok(self.hip.hipEventSynchronize(self.ev[1]))
        t = C.c_float(0)
        self._ok(self.hip.hipEventElapsedTime(C.byref(t), self.ev[0], self.ev[1]))
        return out, float(t.value)


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "repeats": len(ms)}


def timed(clock, fn, repeats):
    """(result, device-event stats, wall stats) of `repeats` calls after one warm-up call."""
    fn()
    dev, wall = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out, ms = clock.ms(fn)
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(ms)
    return out, dict(stats(dev), wall_median_ms=round(statistics.median(wall), 4))


def in_turns(clock, fn_a, fn_b, repeats):
    """Device-event stats of fn_a and of fn_b, called in turns after one warm-up call of each."""
    fn_a(), fn_b()
    a, b = [], []
    for _ in range(repeats):
        a.append(clock.ms(fn_a)[1])
        b.append(clock.ms(fn_b)[1])
    return stats(a), stats(b)


def simulator_on(library, pop, ep):
    """A Simulator whose context lives in another build of the library."""
    saved = (_lib.LIB_PATH, _lib._lib)
    _lib.LIB_PATH, _lib._lib = library, None
    try:
        return Simulator(pop, ep)
    finally:
        _lib.LIB_PATH, _lib._lib = saved


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("preset", nargs="?", default="york")
    ap.add_argument("steps", nargs="?", type=int, default=5000)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--variant", action="append", default=[], metavar="NAME=LIBRARY")
    ap.add_argument("--out")
    a = ap.parse_args()
    clock = DeviceClock()
    pop = Population.synthetic(a.preset)
    labels, n_groups = pop.age_bands(AGE_EDGES)
    out = {"preset": a.preset, "n_citizens": pop.n_citizens, "n_buildings": pop.n_buildings, "n_rooms": pop.n_rooms, "n_groups": n_groups,
           "library": os.path.basename(_lib.LIB_PATH),
           "what": "ms between two device events around one synchronous call; median (min, max) of `repeats` calls after a warm-up call; variants in turns with the product"}
    ep = _lib.default_params(max_steps=max(a.steps, 5000))
    sim = Simulator(pop, ep)
    sim.set_groups(labels, n_groups)
    rec = sim.run(a.steps)
    n = len(rec)
    log_entries = int(rec["exposures_building"].sum(dtype=np.int64) + rec["exposures_bus"].sum(dtype=np.int64)) + len(sim.seeds())
    out.update(steps=n, log_entries=log_entries)
    _, out["mixing_matrix_workplace"] = timed(clock, lambda: sim.mixing_matrix("workplace"), a.repeats)
    mixing = {"work": sim.mixing_matrix("workplace"), "room": sim.mixing_matrix("school")}
    for kind in _lib.PLACE_NAMES:
        ob, t_ob = timed(clock, lambda: sim.place_outbreaks(kind), a.repeats)
        (final_size, introduced), t_sz = timed(clock, lambda: sim.place_sizes(kind), a.repeats)
        real = ob["members"] > 0
        if int(final_size.sum(dtype=np.int64)) != int(real.sum()) or int(introduced.sum(dtype=np.int64)) != int(real.sum()):
            raise SystemExit("the tables do not hold every place once")
        # counted from shapes: the (case, member) pairs a call visits, and what it holds on the device while it runs
        pairs = int((ob["cases"].astype(np.int64) * ob["members"].astype(np.int64))[ob["members"] >= 2].sum())
        rows = 16 * len(ob["members"]) + (16 * pop.n_rooms if kind == "school" else 0)
        res = dict(places=int(real.sum()), with_a_case=int((ob["cases"] > 0).sum()), with_two_or_more=int((ob["cases"] >= 2).sum()),
                   largest=int(ob["members"].max(initial=0)), members=int(ob["members"].sum(dtype=np.int64)), cases=int(ob["cases"].sum(dtype=np.int64)),
                   introductions=int(ob["introductions"].sum(dtype=np.int64)), place_outbreaks=t_ob, place_sizes=t_sz, pairs_visited_at_most=pairs,
                   temporary_bytes_rows_and_tables=rows + 8192, final_size=final_size.tolist(), introduced=introduced.tolist())
        print("%s: %d places, %d with a case, %d with two or more; %d members, %d cases, %d of them introduced" %
              (kind, res["places"], res["with_a_case"], res["with_two_or_more"], res["members"], res["cases"], res["introductions"]))
        top = max(1, int(np.flatnonzero(final_size.sum(axis=0)).max(initial=0)) + 1)
        print("places by size bin (rows) and case bin (columns 0..%d); bin x = x below 16, then 16: 16-31, 17: 32-63, ..." % (top - 1))
        for size in np.flatnonzero(final_size.sum(axis=1)).tolist():
            print("%3d: %s" % (size, " ".join("%7d" % x for x in final_size[size, :top])))
        if kind != "school":
            (at_all, sec_all), res["place_sar_all"] = timed(clock, lambda: sim.place_sar(kind, "all", complete=False), a.repeats)
            (at, sec), res["place_sar_group"] = timed(clock, lambda: sim.place_sar(kind, "group", complete=False), a.repeats)
            if not (sec == mixing[kind]).all() or int(sec.sum()) != int(sec_all.sum()) or int(at.sum()) != int(at_all.sum()) or (sec > at).any():
                raise SystemExit("the secondary cases are not the transmissions of the mixing matrix in the setting, or exceed the members at risk")
            res["temporary_bytes_pair_tables"] = 16 * (1 + n_groups * n_groups)
            try:
                at, sec = sim.place_sar(kind, "group")               # complete cohorts only, for the rates
            except ValueError:
                print("no cohort is complete after %d steps: the rates below count cases that may still infect" % n)
            with np.errstate(invalid="ignore", divide="ignore"):
                sar = np.where(at > 0, sec.astype(np.float64) / at.astype(np.float64), np.nan)
            res.update(at_risk=int(at.sum()), secondary=int(sec.sum()), sar_all=round(float(sec.sum()) / float(at.sum()), 6) if at.sum() else None,
                       sar_by_age_band=[[None if x != x else round(float(x), 5) for x in row] for row in sar])
            print("%s secondary attack rate %s over %d pairs at risk" % (kind, res["sar_all"], res["at_risk"]))
        out[kind] = res
    # the other builds, each on a context of its own with the same run, in turns with the product
    for spec in a.variant:
        name, _, library = spec.partition("=")
        other = simulator_on(os.path.abspath(library), pop, ep)
        other.set_groups(labels, n_groups)
        other.run(a.steps)
        res = {"library": os.path.basename(library)}
        for kind in ("work", "room"):
            for where in ("all", "group"):
                if tuple(map(np.ndarray.tolist, other.place_sar(kind, where, complete=False))) != tuple(map(np.ndarray.tolist, sim.place_sar(kind, where, complete=False))):
                    raise SystemExit("variant %s: esim_place_sar(%s, %s) differs from the product's" % (name, kind, where))
                mine, its = in_turns(clock, lambda: sim.place_sar(kind, where, complete=False), lambda: other.place_sar(kind, where, complete=False), a.repeats)
                res["%s_%s" % (kind, where)] = {"product": mine, "variant": its}
                print("%-14s %-5s %-5s product %.3f ms (%.3f .. %.3f)   variant %.3f ms (%.3f .. %.3f)" %
                      (name, kind, where, mine["median_ms"], mine["min_ms"], mine["max_ms"], its["median_ms"], its["min_ms"], its["max_ms"]))
        out.setdefault("variants", {})[name] = res
        other.close()
    sim.close()
    path = a.out or os.path.join(ROOT, "profiles", "place_outbreaks_%s.json" % a.preset)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k not in _lib.PLACE_NAMES}))


if __name__ == "__main__":
    main()
