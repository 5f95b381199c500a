"""Host-side mirror of the reference's `sim::simulator::Simulator` over libesim.

Same names, argument meaning and side effects as the reference API that `run` and
`visualisation` call (sim/src/simulator.rs):
  Simulator.step()              -> bool      simulator.rs:131-152  (False = epidemic over)
  Simulator.simulate(output)    -> None      simulator.rs:108-127  (progress print every 50 steps,
                                             then the four JSON files of statistics.rs:113-150)
The compute is the HIP library; this file only marshals.
"""
import ctypes as C
import fractions
import json
import math
import os
import time

import numpy as np

from . import _lib
from .population import Population

DEBUG_ITERATION_PRINT = 50  # sim/src/config.rs:34


class StatisticsRecorder:
    """What `StatisticsRecorder` (sim/src/statistics.rs:97-204) keeps, filled from step results."""

    def __init__(self):
        self.global_stats = []       # StatisticEntry dicts, statistics.rs:208-215
        self.timer_entries = []      # per step {"Generate Exposures":..,"Apply Exposures":..,"Apply Interventions":..,"total":..}
        self.memory_usage_entries = []
        self.exposures_all = []      # exposures per time step ("All" series, statistics.rs:119-136)

    def push(self, rec, timings=None):
        self.global_stats.append({k: rec[k] for k in
                                  ("time_step", "susceptible", "exposed", "infected", "recovered", "vaccinated")})
        self.exposures_all.append(rec["exposures_building"] + rec["exposures_bus"])
        if timings is not None:
            self.timer_entries.append(timings)
        self.memory_usage_entries.append(_memory_usage())

    def push_block(self, arr):
        """The same for a block of records (structured array of esim_step_result) that came back from one
        device-resident run: no per-step Python work beyond list building."""
        cols = [arr[k].tolist() for k in ("time_step", "susceptible", "exposed", "infected", "recovered", "vaccinated")]
        keys = ("time_step", "susceptible", "exposed", "infected", "recovered", "vaccinated")
        self.global_stats.extend(dict(zip(keys, row)) for row in zip(*cols))
        self.exposures_all.extend((arr["exposures_building"].astype(np.int64) + arr["exposures_bus"]).tolist())
        self.memory_usage_entries.extend([_memory_usage()] * len(arr))

    def dump_to_file(self, directory, per_output_area=None):
        """statistics.rs:113-150. `dump_to_file` calls next() first, which appends one all-zero
        trailing StatisticEntry (Q14) -- reproduced so downstream notebooks see the same shape."""
        os.makedirs(directory, exist_ok=True)          # fs::create_dir_all(directory), statistics.rs:116
        stats = list(self.global_stats)
        stats.append({"time_step": len(stats) + 1, "susceptible": 0, "exposed": 0, "infected": 0,
                      "recovered": 0, "vaccinated": 0})
        with open(directory + "exposures.json", "w") as f:
            # "All"/"All": exposures per time step.  (The reference overwrites this entry with every place's own series while
            # it drains its map, statistics.rs:123-125, so what it leaves there is one arbitrary place's; the total is what
            # the name says.)  "OutputArea": statistics.rs:127-130.
            doc = {"All": {"All": self.exposures_all}}
            if per_output_area is not None:
                doc["OutputArea"] = per_output_area
            json.dump(doc, f)
        with open(directory + "timings.json", "w") as f:
            json.dump(self.timer_entries, f)
        with open(directory + "memory.json", "w") as f:
            json.dump(self.memory_usage_entries, f)
        with open(directory + "global_stats.json", "w") as f:
            json.dump(stats, f)


def _memory_usage():
    # config.rs:42-47 (VM size of the process, GB)
    try:
        with open("/proc/self/statm") as f:
            pages = int(f.read().split()[0])
        return "%.2f GB" % (pages * os.sysconf("SC_PAGE_SIZE") / 1024 / 1024 / 1024.0)
    except OSError:
        return "0.00 GB"


# -- the rank rules of the ensemble quantile maps (Simulator.ensemble_quantiles, Ensemble) -------
def check_probs(who, probs):
    """The probabilities as a list of floats; ValueError for one outside [0, 1] (NaN included)."""
    out = [float(p) for p in probs]
    for p in out:
        if not 0.0 <= p <= 1.0:
            raise ValueError("%s: a probability must lie in [0, 1], got %r" % (who, p))
    return out


def nearest_rank(p, m):
    """The 0-based rank of the inverted CDF among m members: the smallest value v with at least p * m members <= v, that is
    max(0, ceil(p * m) - 1).  p is taken as the decimal it was written as (0.05 is 1/20, not the binary number next to it), so
    that p * m is exact and 5 % of 20 members is the first of them."""
    x = fractions.Fraction(repr(float(p))) * int(m)
    return max(0, -((-x.numerator) // x.denominator) - 1)


def linear_ranks(p, m):
    """(lo, hi, frac): the neighbouring 0-based ranks of h = p * (m - 1) and the weight of the upper one, numpy's default
    ("linear") definition; hi == lo where h is a whole number."""
    h = float(p) * (int(m) - 1)
    lo = min(int(math.floor(h)), int(m) - 1)
    return lo, min(int(math.ceil(h)), int(m) - 1), h - lo


def interpolate_linear(lo, hi, frac):
    """float64: lo + (hi - lo) * frac per cell, NaN where either neighbour of an unsigned kind is _lib.NEVER."""
    a, b = np.asarray(lo).astype(np.float64), np.asarray(hi).astype(np.float64)
    out = a + (b - a) * float(frac)
    if np.asarray(lo).dtype == np.uint32:
        out[(np.asarray(lo) == _lib.NEVER) | (np.asarray(hi) == _lib.NEVER)] = np.nan
    return out


class Simulator:
    """`Simulator::from(builder)` (simulator.rs:601-644): takes a built population."""

    def __init__(self, population, params=None, area_code="synthetic", record_timings=False, area_codes=None):
        """record_timings: keep the reference's per-step function timers (statistics.rs:46-95,
        simulator.rs:137,140,143) -- GPU time of the three phases from HIP events; costs one
        synchronisation per step, so it is off unless asked for."""
        self.lib = _lib.load()
        self.area_code = area_code
        self.area_codes = area_codes          # Output Area codes (reference_io), for the keys of exposures.json
        self.population = population
        self.params = params if params is not None else _lib.default_params()
        self.current_population = population.n_citizens
        self.statistics_recorder = StatisticsRecorder()
        self._ctx = C.c_void_p()
        _lib.check(self.lib.esim_create(C.byref(self.params), C.byref(self._ctx)))
        ps = population.as_struct()
        _lib.check(self.lib.esim_upload_population(self._ctx, C.byref(ps)), self._ctx)
        self._steps = 0
        self.record_timings = bool(record_timings)
        self._last_phase = None
        if self.record_timings:
            self.enable_phase_timing(True)
            self._last_phase = self.phase_timings()

    # -- reference API -----------------------------------------------------------------
    def step(self):
        """Applies a single time step; returns False if the disease has finished."""
        r = _lib.StepResult()
        _lib.check(self.lib.esim_step(self._ctx, C.byref(r)), self._ctx)
        self._steps += 1
        rec = r.as_dict()
        timings = None
        if self.record_timings:
            now = self.phase_timings()
            timings = {k: now[k] - self._last_phase[k] for k in now}
            self._last_phase = now
        self.statistics_recorder.push(rec, timings)
        self.last = rec
        return bool(rec["disease_exists"])

    def simulate(self, output_name):
        """simulator.rs:108-127: steps until the disease is gone or max_time_step, a progress line after the steps
        with index 0, 50, 100, ... and the statistics dump.  With record_timings the loop is the reference's step by
        step; otherwise the steps between two progress lines are one device-resident run (esim_run with
        stop_when_done), which produces the same records without a host round trip per step."""
        start = time.time()
        max_time_step = int(self.params.max_steps)
        # A context that has already run (step(), run(), load_checkpoint()) continues from its own clock: the loop index of
        # simulator.rs:114 is the absolute step index self._steps, so the budget and the progress cadence stay the run's.
        if self.record_timings:
            while self._steps < max_time_step:
                time_step = self._steps
                if not self.step():
                    break
                if time_step % DEBUG_ITERATION_PRINT == 0:
                    self._progress(start)
                    start = time.time()
        else:
            self.enable_chunk_kernel_timing(True)       # feeds the phase keys of timings.json (below); off again when simulate() returns
            while self._steps < max_time_step:
                # the next progress line follows the step with index 0 (mod 50)
                done = self._steps
                n = 1 if done == 0 else DEBUG_ITERATION_PRINT - (done - 1) % DEBUG_ITERATION_PRINT
                n = min(n, max_time_step - done)
                t_block = time.time()
                arr = self.run(n, stop_when_done=True)
                if len(arr) == 0:
                    break
                # The phases of simulator.rs:137-143 do not exist separately in a device-resident run: a chunk pass works on up to
                # 96 steps at once.  Their keys are APPORTIONED: the device time of the block's chunk kernels (HIP events in front of
                # every kernel, esim_chunk_kernel_timings) by kernel -- marks + fold -> "Generate Exposures", draw + units -> "Apply
                # Exposures", plan / decisions / counts / books / scatter -> "Apply Interventions" -- spread evenly over the block's
                # steps; "total" is the block's wall time spread the same way.  Blocks whose steps ran in the sequential form (the step
                # that starts the vaccination programme) carry "total" only.
                per_step = (time.time() - t_block) / len(arr)
                entry = {"total": per_step}
                phases = self.chunk_phase_seconds()
                if sum(phases.values()) > 0.0:
                    entry = dict({k: v / len(arr) for k, v in phases.items()}, total=per_step)
                self.statistics_recorder.timer_entries.extend(dict(entry) for _ in range(len(arr)))
                self.last = {k: int(arr[k][-1]) for k in arr.dtype.names}
                if not self.last["disease_exists"]:
                    break
                if (self._steps - 1) % DEBUG_ITERATION_PRINT == 0:
                    self._progress(start)
                    start = time.time()
        if not self.record_timings:
            self.enable_chunk_kernel_timing(False)
        self.statistics_recorder.dump_to_file(output_name, self.exposures_per_output_area(self.area_codes))

    def _progress(self, start):
        print("Completed %3d time steps, in: %6s seconds  Statistics: %s,   Memory usage: %s" % (
            DEBUG_ITERATION_PRINT, "%.2f" % (time.time() - start), self.last, _memory_usage()))

    # -- device-resident loop ----------------------------------------------------------
    def run(self, n_steps, stop_when_done=False, clock=None):
        """`n_steps` of the loop of simulate() without host round trips; returns the records as a
        structured numpy array (fields of esim_step_result).  clock: a list that receives the wall seconds of the library
        call alone (esim_run: enqueue, device work, read-back of the records), without this method's own bookkeeping."""
        buf = (_lib.StepResult * max(1, n_steps))()
        n_done = C.c_uint32(0)
        t0 = time.perf_counter()
        rc = self.lib.esim_run(self._ctx, n_steps, int(stop_when_done), buf, C.byref(n_done))
        if clock is not None:
            clock.append(time.perf_counter() - t0)
        _lib.check(rc, self._ctx)
        self._steps += n_done.value
        arr = np.frombuffer(buf, dtype=RECORD_DTYPE, count=n_done.value).copy()
        self.statistics_recorder.push_block(arr)
        return arr

    def synchronize(self):
        _lib.check(self.lib.esim_synchronize(self._ctx), self._ctx)

    def reset(self):
        _lib.check(self.lib.esim_reset(self._ctx), self._ctx)
        self.statistics_recorder = StatisticsRecorder()
        self._steps = 0

    def restart(self, params=None, seeds=None, **overrides):
        """Back to step 0 under other parameters without a new upload (esim_restart): `params`, or the current parameters
        changed by `overrides` (e.g. seed=7).  The initial state is rebuilt on the device; the call does not wait for it.
        seeds: None keeps the initially infected citizens in force; an array of citizen indices replaces them
        (esim_restart_seeded; Population.draw_index_cases draws such a list the way the reference's builder does)."""
        p = _lib.Params()
        C.memmove(C.byref(p), C.byref(params if params is not None else self.params), C.sizeof(_lib.Params))
        for k, v in overrides.items():
            if not hasattr(p, k):
                raise AttributeError("esim_params has no field %r" % k)
            setattr(p, k, v)
        if seeds is None:
            _lib.check(self.lib.esim_restart(self._ctx, C.byref(p)), self._ctx)
        else:
            raw = np.asarray(seeds)
            if raw.ndim != 1 or (raw.size and (raw.dtype.kind not in "iu" or int(raw.min()) < 0 or int(raw.max()) > 0xFFFFFFFF)):
                raise ValueError("restart: seeds must be a one-dimensional array of citizen indices")
            arr = np.ascontiguousarray(raw, np.uint32)
            _lib.check(self.lib.esim_restart_seeded(self._ctx, C.byref(p), arr.ctypes.data_as(C.POINTER(C.c_uint32)), arr.size), self._ctx)
        self.params = p
        self.statistics_recorder = StatisticsRecorder()
        self._steps = 0

    # -- forecast ensembles: a snapshot on the device and branches from it (esim_snapshot, esim_rollback) -------
    def snapshot(self):
        """Keeps the state after the last completed step on the device, with the parameters in force (esim_snapshot): one
        snapshot per context, a later call replaces it.  Nothing proportional to the population moves to the host."""
        _lib.check(self.lib.esim_snapshot(self._ctx), self._ctx)

    def snapshot_step(self):
        """The step of the snapshot held (esim_snapshot_info); 0: none."""
        step = C.c_uint32(0)
        _lib.check(self.lib.esim_snapshot_info(self._ctx, C.byref(step), None), self._ctx)
        return int(step.value)

    def rollback(self, params=None, **overrides):
        """Back to the snapshot's step with other parameters in force from the next step on (esim_rollback): `params`, or the
        snapshot's own parameters changed by `overrides` (e.g. seed=7, lockdown_threshold=0.01), as restart applies them.  The
        times and the working hours must be the snapshot's.  The statistics recorder keeps the entries of the shared history."""
        step = C.c_uint32(0)
        p = _lib.Params()
        _lib.check(self.lib.esim_snapshot_info(self._ctx, C.byref(step), C.byref(p)), self._ctx)
        if params is not None:
            C.memmove(C.byref(p), C.byref(params), C.sizeof(_lib.Params))
        for k, v in overrides.items():
            if not hasattr(p, k):
                raise AttributeError("esim_params has no field %r" % k)
            setattr(p, k, v)
        own = params is None and not overrides
        _lib.check(self.lib.esim_rollback(self._ctx, None if own else C.byref(p)), self._ctx)
        self.params = p
        self._steps = int(step.value)
        sr = self.statistics_recorder
        if len(sr.global_stats) >= self._steps and len(sr.exposures_all) >= self._steps:
            del sr.global_stats[self._steps:], sr.exposures_all[self._steps:], sr.memory_usage_entries[self._steps:], sr.timer_entries[self._steps:]
        else:                                   # (a reset or restart in between emptied it: the history comes back from the records)
            self.statistics_recorder = StatisticsRecorder()
            self.statistics_recorder.push_block(self.records_so_far())

    # -- paired policy comparison: a kept baseline run and the run as it stands (esim_baseline_*, esim_compare*) -------
    @staticmethod
    def _compare_place(who, where):
        """`where` of the comparison calls as its code; anything but "all", "home" and "group" raises ValueError."""
        places = {"all": _lib.BY_ALL, "home": _lib.AREA_HOME, "group": _lib.BY_GROUP}
        if isinstance(where, str):
            if where not in places:
                raise ValueError("%s: where must be 'all', 'home' or 'group', got %r" % (who, where))
            return places[where]
        if isinstance(where, (bool, float)) or where not in places.values():
            raise ValueError("%s: where must be 'all', 'home' or 'group', got %r" % (who, where))
        return int(where)

    def _compare_cols(self, place):
        return 1 if place == _lib.BY_ALL else max(1, self._n_groups) if place == _lib.BY_GROUP else self.population.n_areas

    @staticmethod
    def _compare_rows(who, first_step, n_rows, stride, last):
        """(first_step, n_rows, stride) of event rows that may start at step 0, checked; n_rows=None: up to step `last` (a
        number, or a function that gives it: asked only once the other arguments stand)."""
        first, stride = int(first_step), int(stride)
        if first < 0 or stride < 1:
            raise ValueError("%s: first_step must be >= 0 and stride >= 1" % who)
        if n_rows is None:
            last = int(last() if callable(last) else last)
            n_rows = (last - first) // stride + 1 if first <= last else 0
        if int(n_rows) < 1:
            raise ValueError("%s: no rows (first_step %d lies beyond the last step, or n_rows < 1)" % (who, first))
        return first, int(n_rows), stride

    def keep_baseline(self):
        """Keeps the exposure step of every citizen of the run as it stands on the device (esim_baseline_keep): the baseline
        that compare() and compare_series() set a later run against.  It survives reset, restart, snapshot and rollback."""
        _lib.check(self.lib.esim_baseline_keep(self._ctx), self._ctx)

    def baseline_info(self):
        """{"steps", "n_cases", "params"} of the baseline kept (esim_baseline_info): the steps it ran, the entries of its
        exposure log (index cases included) and the parameters it ran under."""
        steps, cases, p = C.c_uint32(0), C.c_uint32(0), _lib.Params()
        _lib.check(self.lib.esim_baseline_info(self._ctx, C.byref(steps), C.byref(cases), C.byref(p)), self._ctx)
        return {"steps": int(steps.value), "n_cases": int(cases.value), "params": p}

    def drop_baseline(self):
        """Forgets the baseline kept (esim_baseline_drop)."""
        _lib.check(self.lib.esim_baseline_drop(self._ctx), self._ctx)

    def _compare_last(self):
        """The last step both runs have, the window's default end (without a baseline: of this run; the library refuses then)."""
        steps = C.c_uint32(0)
        if self.lib.esim_baseline_info(self._ctx, C.byref(steps), None, None) != _lib.OK:
            return self._steps
        return min(self._steps, int(steps.value))

    def compare(self, where="all", first_step=0, last_step=None, citizens=False):
        """The run as it stands against the baseline kept (esim_compare), a dict: counts, uint64 [n_cols, 5] -- per column the
        citizens that are a case (exposed in steps first_step .. last_step; step 0: the index cases) in both runs, in the
        baseline only (averted), in this run only (added), and of those in both the ones exposed earlier and later here
        (_lib.CMP_*); delay, int64 [n_cols]: the sum of (step here - step in the baseline) over the cases of both;
        first_divergence: the first step at which the two histories differ, None when they are identical; and with
        citizens=True cls, uint8 [n_citizens]: 0 neither, 1 both, 2 averted, 3 added.  where: "all" (one column), "home" (by
        the Output Area of the household) or "group".  last_step=None: the last step of the shorter run."""
        place = self._compare_place("compare", where)
        first = int(first_step)
        if first < 0 or (last_step is not None and int(last_step) < first):
            raise ValueError("compare: steps %d..%s are no window" % (first, last_step))
        last = self._compare_last() if last_step is None else int(last_step)
        cols = self._compare_cols(place)
        counts, delay, div = np.zeros((cols, _lib.CMP_N), np.uint64), np.zeros(cols, np.int64), C.c_uint32(0)
        cls = np.zeros(self.population.n_citizens, np.uint8) if citizens else None
        _lib.check(self.lib.esim_compare(self._ctx, place, first, last, counts.ctypes.data_as(C.POINTER(C.c_uint64)), delay.ctypes.data_as(C.POINTER(C.c_int64)),
                                         C.byref(div), cls.ctypes.data_as(C.POINTER(C.c_uint8)) if citizens else None), self._ctx)
        out = {"counts": counts, "delay": delay, "first_divergence": None if div.value == _lib.NEVER else int(div.value)}
        if citizens:
            out["cls"] = cls
        return out

    def compare_series(self, where="all", first_step=0, n_rows=None, stride=24, cumulative=False):
        """(baseline, current), uint32 [n_rows, n_cols] each (esim_compare_series): row i holds the cases of the `stride` steps
        from first_step + i * stride on in the baseline kept and in the run as it stands (step 0: the index cases); with
        cumulative=True the cases from first_step up to the row's last step.  baseline - current is the cases averted by row.
        where as for compare(); n_rows=None: up to the last step of the shorter run."""
        place = self._compare_place("compare_series", where)
        first, n_rows, stride = self._compare_rows("compare_series", first_step, n_rows, stride, self._compare_last)
        cols = self._compare_cols(place)
        base, cur = np.zeros((n_rows, cols), np.uint32), np.zeros((n_rows, cols), np.uint32)
        _lib.check(self.lib.esim_compare_series(self._ctx, place, first, n_rows, stride, int(bool(cumulative)), base.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                cur.ctypes.data_as(C.POINTER(C.c_uint32))), self._ctx)
        return base, cur

    def ensemble_begin_paired(self, where="all", first_step=0, n_rows=None, stride=24, cumulative=False, min_baseline=1, min_averted=1):
        """Accumulators over the paired rows (esim_ensemble_begin_paired): a member contributes the (baseline, current) rows
        compare_series(where, first_step, n_rows, stride, cumulative) would return for it.  Per cell ensemble_fold counts the
        members with at least min_baseline cases in the baseline (defined), those of them with baseline - current >=
        min_averted (hit), and sums both counts, their squares and their product, in integers on the device.  n_rows=None: up
        to the last step of the run (params.max_steps); ensemble_read_paired reads them."""
        place = self._compare_place("ensemble_begin_paired", where)
        first, n_rows, stride = self._compare_rows("ensemble_begin_paired", first_step, n_rows, stride, int(self.params.max_steps))
        if int(min_averted) < 1 or int(min_baseline) < 0:
            raise ValueError("ensemble_begin_paired: min_averted must be >= 1 and min_baseline >= 0")
        _lib.check(self.lib.esim_ensemble_begin_paired(self._ctx, place, first, n_rows, stride, int(bool(cumulative)), int(min_baseline), int(min_averted)), self._ctx)
        self._ens_rows = n_rows
        self._ens_n = self._compare_cols(place)

    PAIRED_KEYS = ("defined", "hit", "sum_baseline", "sum_current", "sumsq_baseline", "sumsq_current", "sum_cross")

    def ensemble_read_paired(self, first_row=0, n_rows=None):
        """{"members": int, "defined", "hit": uint32 [n, n_cols], "sum_baseline", "sum_current", "sumsq_baseline",
        "sumsq_current", "sum_cross": uint64 [n, n_cols]}: rows [first_row, first_row + n) of the accumulators begun by
        ensemble_begin_paired; n_rows=None: all from first_row on."""
        total = getattr(self, "_ens_rows", 0)
        n = max(0, total - int(first_row)) if n_rows is None else int(n_rows)
        cols = getattr(self, "_ens_n", 1)
        members = C.c_uint32(0)
        out = {k: np.zeros((n, cols), np.uint32 if i < 2 else np.uint64) for i, k in enumerate(self.PAIRED_KEYS)}
        ptrs = [out[k].ctypes.data_as(C.POINTER(C.c_uint32 if i < 2 else C.c_uint64)) for i, k in enumerate(self.PAIRED_KEYS)]
        _lib.check(self.lib.esim_ensemble_read_paired(self._ctx, int(first_row), n, C.byref(members), *ptrs), self._ctx)
        return dict(out, members=int(members.value))

    def seeds(self):
        """The distinct initially infected citizens in force, in the order of the exposure log (esim_get_seeds)."""
        n = C.c_uint32(0)
        rc = self.lib.esim_get_seeds(self._ctx, None, 0, C.byref(n))
        if rc not in (_lib.ESIM_OK, _lib.ESIM_ERANGE):
            _lib.check(rc, self._ctx)
        out = np.zeros(n.value, np.uint32)
        if n.value:
            _lib.check(self.lib.esim_get_seeds(self._ctx, out.ctypes.data_as(C.POINTER(C.c_uint32)), n.value, C.byref(n)), self._ctx)
        return out

    # -- per-Output-Area accumulators over the members of an ensemble (esim_ensemble_*) -------
    def ensemble_begin(self, where="home", status_mask=(1 << _lib.EXPOSED) | (1 << _lib.INFECTED) | (1 << _lib.RECOVERED), min_cases=1):
        code = {"current": _lib.AREA_CURRENT, "home": _lib.AREA_HOME, "group": _lib.BY_GROUP}.get(where, where)
        self._ens_n = self._n_groups if code == _lib.BY_GROUP else self.population.n_areas
        self._ens_rows = 1
        _lib.check(self.lib.esim_ensemble_begin(self._ctx, int(code), int(status_mask), int(min_cases)), self._ctx)

    def ensemble_begin_arrival(self, where="home", horizon=None):
        """Accumulators of the arrival step instead (esim_ensemble_begin_arrival): a member counts as a hit where the epidemic
        reached the area (where="home") or group (where="group") by step `horizon`; None: within whatever steps it ran."""
        code = {"current": _lib.AREA_CURRENT, "home": _lib.AREA_HOME, "group": _lib.BY_GROUP}.get(where, where)   # ("current": refused by the library)
        self._ens_n = self._n_groups if code == _lib.BY_GROUP else self.population.n_areas
        self._ens_rows = 1
        _lib.check(self.lib.esim_ensemble_begin_arrival(self._ctx, int(code), _lib.NEVER if horizon is None else int(horizon)), self._ctx)

    def ensemble_fold(self):
        """Adds the state as it stands to the accumulators, on the device; nothing is downloaded."""
        _lib.check(self.lib.esim_ensemble_fold(self._ctx), self._ctx)

    def ensemble_read(self):
        """{"members": int, "hit": uint32 [n], "sum": uint64 [n], "sumsq": uint64 [n]}, n = n_areas, or n_groups for
        accumulators begun by group."""
        na = getattr(self, "_ens_n", self.population.n_areas)
        members = C.c_uint32(0)
        hit, tot, sq = np.zeros(na, np.uint32), np.zeros(na, np.uint64), np.zeros(na, np.uint64)
        _lib.check(self.lib.esim_ensemble_read(self._ctx, C.byref(members), hit.ctypes.data_as(C.POINTER(C.c_uint32)),
                                               tot.ctypes.data_as(C.POINTER(C.c_uint64)), sq.ctypes.data_as(C.POINTER(C.c_uint64))), self._ctx)
        return {"members": int(members.value), "hit": hit, "sum": tot, "sumsq": sq}

    def ensemble_begin_series(self, where, what, first_step=1, n_rows=None, stride=1, min_cases=1):
        """Accumulators over the rows of a series instead (esim_ensemble_begin_series): a member contributes, cell for cell,
        the rows area_status_series(what, where), area_series("exposures") or group_series(what) would return for it with the
        same first_step, n_rows and stride.  where: "home", "current" or "group"; what: "susceptible", "exposed", "infected",
        "recovered", "vaccinated", or "incidence" / "exposures" (two names of the event rows: exposures of the `stride` steps
        from the row's on -- by "home" and "group" in buildings and on public transport, by "current" in buildings).
        n_rows=None: up to the last step of the run (params.max_steps).  The rows stay on the device; ensemble_fold adds
        hit += (x >= min_cases), sum += x, sumsq += x * x per cell there."""
        place = {"current": _lib.AREA_CURRENT, "home": _lib.AREA_HOME, "group": _lib.BY_GROUP}.get(where, where)
        code = {"susceptible": _lib.SUSCEPTIBLE, "exposed": _lib.EXPOSED, "infected": _lib.INFECTED, "recovered": _lib.RECOVERED,
                "vaccinated": _lib.VACCINATED, "incidence": _lib.ENSEMBLE_SERIES_EVENTS, "exposures": _lib.ENSEMBLE_SERIES_EVENTS}.get(what, what)
        if n_rows is None:
            last = int(self.params.max_steps)
            n_rows = (last - int(first_step)) // int(stride) + 1 if stride and 1 <= first_step <= last else 0
        _lib.check(self.lib.esim_ensemble_begin_series(self._ctx, int(place), int(code), int(first_step), int(n_rows), int(stride), int(min_cases)), self._ctx)
        self._ens_rows = int(n_rows)
        self._ens_n = self._n_groups if place == _lib.BY_GROUP else self.population.n_areas

    def ensemble_read_series(self, first_row=0, n_rows=None):
        """{"members": int, "hit": uint32 [n, n_cols], "sum": uint64 [n, n_cols], "sumsq": uint64 [n, n_cols]}: rows
        [first_row, first_row + n) of the accumulators begun by ensemble_begin_series; n_rows=None: all from first_row on."""
        total = getattr(self, "_ens_rows", 0)
        n = max(0, total - int(first_row)) if n_rows is None else int(n_rows)
        cols = getattr(self, "_ens_n", self.population.n_areas)
        members = C.c_uint32(0)
        hit, tot, sq = np.zeros((n, cols), np.uint32), np.zeros((n, cols), np.uint64), np.zeros((n, cols), np.uint64)
        _lib.check(self.lib.esim_ensemble_read_series(self._ctx, int(first_row), n, C.byref(members), hit.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                      tot.ctypes.data_as(C.POINTER(C.c_uint64)), sq.ctypes.data_as(C.POINTER(C.c_uint64))), self._ctx)
        return {"members": int(members.value), "hit": hit, "sum": tot, "sumsq": sq}

    def ensemble_begin_settings(self, where="home", settings=None, first_step=1, n_rows=None, stride=1, min_cases=1):
        """Accumulators over the exposures by setting (esim_ensemble_begin_settings): a member contributes, cell for cell, the
        rows setting_series(where, settings, first_step, n_rows, stride) would return for it.  where: "setting" (four columns),
        "home" or "group"; settings as setting_series takes them.  n_rows=None: up to the last step of the run
        (params.max_steps).  ensemble_fold adds hit += (x >= min_cases), sum += x, sumsq += x * x per cell on the device;
        ensemble_read_series reads them."""
        place = {"setting": _lib.BY_SETTING, "home": _lib.AREA_HOME, "group": _lib.BY_GROUP, "current": _lib.AREA_CURRENT}.get(where, where)   # ("current": refused by the library)
        if n_rows is None:
            last = int(self.params.max_steps)
            n_rows = (last - int(first_step)) // int(stride) + 1 if stride and 1 <= first_step <= last else 0
        _lib.check(self.lib.esim_ensemble_begin_settings(self._ctx, int(place), self._setting_mask(settings), int(first_step), int(n_rows), int(stride), int(min_cases)), self._ctx)
        self._ens_rows = int(n_rows)
        self._ens_n = _lib.N_SETTINGS if place == _lib.BY_SETTING else self._n_groups if place == _lib.BY_GROUP else self.population.n_areas

    def ensemble_begin_reproduction(self, where="home", first_step=0, n_rows=None, stride=24, min_cohort=1, r=(1, 1)):
        """Accumulators over the cohort rows (esim_ensemble_begin_reproduction): a member contributes the (cases, offspring) rows
        reproduction_series(where, first_step, n_rows, stride) would return for it.  where: "all" (one column), "home" or
        "group".  Per cell ensemble_fold counts the members with a cohort of at least min_cohort cases (defined), those of them
        with offspring / cases >= r[0] / r[1] (hit), and sums cases, offspring, their squares and their product, in integers on
        the device.  n_rows=None: up to the last step of the run (params.max_steps); ensemble_read_reproduction reads them."""
        place = {"all": _lib.BY_ALL, "home": _lib.AREA_HOME, "group": _lib.BY_GROUP, "current": _lib.AREA_CURRENT}.get(where, where)   # ("current": refused by the library)
        if n_rows is None:
            last = int(self.params.max_steps)
            n_rows = (last - int(first_step)) // int(stride) + 1 if stride and 0 <= first_step <= last else 0
        _lib.check(self.lib.esim_ensemble_begin_reproduction(self._ctx, int(place), int(first_step), int(n_rows), int(stride), int(min_cohort), int(r[0]), int(r[1])), self._ctx)
        self._ens_rows = int(n_rows)
        self._ens_n = 1 if place == _lib.BY_ALL else self._n_groups if place == _lib.BY_GROUP else self.population.n_areas

    REPRODUCTION_KEYS = ("defined", "hit", "sum_cases", "sum_offspring", "sumsq_cases", "sumsq_offspring", "sum_cross")

    def ensemble_read_reproduction(self, first_row=0, n_rows=None):
        """{"members": int, "defined", "hit": uint32 [n, n_cols], "sum_cases", "sum_offspring", "sumsq_cases", "sumsq_offspring",
        "sum_cross": uint64 [n, n_cols]}: rows [first_row, first_row + n) of the accumulators begun by
        ensemble_begin_reproduction; n_rows=None: all from first_row on."""
        total = getattr(self, "_ens_rows", 0)
        n = max(0, total - int(first_row)) if n_rows is None else int(n_rows)
        cols = getattr(self, "_ens_n", self.population.n_areas)
        members = C.c_uint32(0)
        out = {k: np.zeros((n, cols), np.uint32 if i < 2 else np.uint64) for i, k in enumerate(self.REPRODUCTION_KEYS)}
        ptrs = [out[k].ctypes.data_as(C.POINTER(C.c_uint32 if i < 2 else C.c_uint64)) for i, k in enumerate(self.REPRODUCTION_KEYS)]
        _lib.check(self.lib.esim_ensemble_read_reproduction(self._ctx, int(first_row), n, C.byref(members), *ptrs), self._ctx)
        return dict(out, members=int(members.value))

    # -- the shape of the epidemic curve per column (esim_curve_summary, esim_ensemble_begin_peaks) -------
    CURVE_STATUS = {"exposed": 1 << _lib.EXPOSED, "infected": 1 << _lib.INFECTED, "active": (1 << _lib.EXPOSED) | (1 << _lib.INFECTED)}
    CURVE_KEYS = ("peak", "peak_step", "steps_at_least", "first_at_least", "last_at_least", "person_steps")
    PEAKS_KEYS = ("defined", "hit", "sum_peak", "sumsq_peak", "sum_step", "sumsq_step", "sum_duration", "sumsq_duration")

    def _curve_args(self, who, where, status):
        """(`where` code, status mask, columns) of the curve calls; a bad `status` is refused here, before any library call."""
        if status not in self.CURVE_STATUS:
            raise ValueError("Simulator.%s: status must be 'exposed', 'infected' or 'active', got %r" % (who, status))
        place = {"all": _lib.BY_ALL, "home": _lib.AREA_HOME, "group": _lib.BY_GROUP, "current": _lib.AREA_CURRENT}.get(where, where)   # ("current": refused by the library)
        n_cols = 1 if place == _lib.BY_ALL else max(1, self._n_groups) if place == _lib.BY_GROUP else self.population.n_areas
        return int(place), self.CURVE_STATUS[status], n_cols

    def curve_summary(self, where="home", status="infected", first_step=1, last_step=None, threshold=1):
        """The shape of the epidemic curve per column (esim_curve_summary), a dict of [n_cols] arrays over the steps first_step ..
        last_step (None: the last step run) of x_s = the citizens of the column whose status after step s is `status`
        ("exposed", "infected", or "active": either): peak = max x_s; peak_step = the first step that attains it (_lib.NEVER
        where the peak is 0); steps_at_least = the steps with x_s >= threshold, first_at_least and last_at_least the first and
        the last of them (_lib.NEVER without one); person_steps = the sum of x_s (uint64).  where: "all" (one column), "home"
        (by the Output Area of the household) or "group".  Computed on the device from the exposure log; no rows are built."""
        place, mask, n_cols = self._curve_args("curve_summary", where, status)
        last = self._steps if last_step is None else int(last_step)
        out = {k: np.zeros(n_cols, np.uint64 if k == "person_steps" else np.uint32) for k in self.CURVE_KEYS}
        ptrs = [out[k].ctypes.data_as(C.POINTER(C.c_uint64 if k == "person_steps" else C.c_uint32)) for k in self.CURVE_KEYS]
        _lib.check(self.lib.esim_curve_summary(self._ctx, place, mask, int(first_step), last, int(threshold), *ptrs), self._ctx)
        return out

    def ensemble_begin_peaks(self, where="home", status="infected", first_step=1, last_step=None, threshold=1, min_peak=1):
        """Accumulators over the curve summaries (esim_ensemble_begin_peaks): ensemble_fold computes the member's
        curve_summary(where, status, first_step, last_step, threshold) on the device and adds per column defined += (peak >= 1),
        hit += (peak >= min_peak), the sums of the peak, of steps_at_least and of their squares over all members, and those of
        peak_step over the defined ones.  last_step=None: the last step of the run (params.max_steps).  ensemble_read_peaks
        reads them."""
        place, mask, n_cols = self._curve_args("ensemble_begin_peaks", where, status)
        last = int(self.params.max_steps) if last_step is None else int(last_step)
        _lib.check(self.lib.esim_ensemble_begin_peaks(self._ctx, place, mask, int(first_step), last, int(threshold), int(min_peak)), self._ctx)
        self._ens_rows = 1
        self._ens_n = n_cols

    def ensemble_read_peaks(self):
        """{"members": int, "defined", "hit": uint32 [n_cols], "sum_peak", "sumsq_peak", "sum_step", "sumsq_step", "sum_duration",
        "sumsq_duration": uint64 [n_cols]}: the accumulators begun by ensemble_begin_peaks."""
        cols = getattr(self, "_ens_n", self.population.n_areas)
        members = C.c_uint32(0)
        out = {k: np.zeros(cols, np.uint32 if i < 2 else np.uint64) for i, k in enumerate(self.PEAKS_KEYS)}
        ptrs = [out[k].ctypes.data_as(C.POINTER(C.c_uint32 if i < 2 else C.c_uint64)) for i, k in enumerate(self.PEAKS_KEYS)]
        _lib.check(self.lib.esim_ensemble_read_peaks(self._ctx, C.byref(members), *ptrs), self._ctx)
        return dict(out, members=int(members.value))

    # -- hospital burden: admissions, bed occupancy and deaths over a finished run (esim_burden_*) -------
    BURDEN_KEYS = ("peak", "peak_step", "steps_at_least", "first_at_least", "last_at_least", "bed_steps", "admissions", "deaths")

    def set_burden(self, tables=None, **kw):
        """The severity tables in force (esim_burden_set): the dict of _lib.burden_tables, or its arguments as keywords.  Tables
        of several groups need set_groups with as many groups first.  They stay through restart, snapshot and rollback."""
        t = dict(tables) if tables is not None else _lib.burden_tables(**kw)
        arr = {k: np.ascontiguousarray(t[k], np.uint32) for k in ("admit_thr", "death_thr", "delay_cdf", "stay_cdf")}
        if arr["admit_thr"].shape != arr["death_thr"].shape or arr["admit_thr"].ndim != 1:
            raise ValueError("Simulator.set_burden: admit_thr and death_thr must have one entry per group each")
        ptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))
        p = _lib.BurdenParams(arr["admit_thr"].size, ptr(arr["admit_thr"]), ptr(arr["death_thr"]), int(t.get("delay_unit", 24)), arr["delay_cdf"].size,
                              ptr(arr["delay_cdf"]), int(t.get("stay_unit", 24)), arr["stay_cdf"].size, ptr(arr["stay_cdf"]))
        _lib.check(self.lib.esim_burden_set(self._ctx, C.byref(p)), self._ctx)

    def drop_burden(self):
        _lib.check(self.lib.esim_burden_drop(self._ctx), self._ctx)

    def burden(self):
        """The tables in force as set_burden takes them (esim_burden_get); EsimError (ESTATE) without any."""
        n = [C.c_uint32(0) for _ in range(5)]               # n_groups, delay_unit, n_delay, stay_unit, n_stay
        _lib.check(self.lib.esim_burden_get(self._ctx, C.byref(n[0]), None, None, C.byref(n[1]), C.byref(n[2]), None, C.byref(n[3]), C.byref(n[4]), None), self._ctx)
        admit, death = np.zeros(n[0].value, np.uint32), np.zeros(n[0].value, np.uint32)
        delay, stay = np.zeros(_lib.BURDEN_BINS, np.uint32), np.zeros(_lib.BURDEN_BINS, np.uint32)
        ptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))
        _lib.check(self.lib.esim_burden_get(self._ctx, None, ptr(admit), ptr(death), None, None, ptr(delay), None, None, ptr(stay)), self._ctx)
        return dict(admit_thr=admit, death_thr=death, delay_cdf=delay[:n[2].value].copy(), stay_cdf=stay[:n[4].value].copy(),
                    delay_unit=int(n[1].value), stay_unit=int(n[3].value))

    def burden_outcomes(self):
        """{"admit_step", "end_step": uint32 [n_citizens], _lib.NEVER where the citizen is no admitted case; "died": bool
        [n_citizens]} (esim_burden_outcomes).  A case occupies a bed after the steps admit_step .. end_step - 1 and, where it
        dies, dies at end_step; both may lie beyond the steps run."""
        n = self.population.n_citizens
        admit, end, died = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint8)
        _lib.check(self.lib.esim_burden_outcomes(self._ctx, admit.ctypes.data_as(C.POINTER(C.c_uint32)), end.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                 died.ctypes.data_as(C.POINTER(C.c_uint8))), self._ctx)
        return {"admit_step": admit, "end_step": end, "died": died.astype(bool)}

    def _burden_where(self, where):
        place = {"all": _lib.BY_ALL, "home": _lib.AREA_HOME, "group": _lib.BY_GROUP, "current": _lib.AREA_CURRENT}.get(where, where)   # ("current": refused by the library)
        return int(place), 1 if place == _lib.BY_ALL else max(1, self._n_groups) if place == _lib.BY_GROUP else self.population.n_areas

    def burden_series(self, what="occupancy", where="all", first_step=1, n_rows=None, stride=1):
        """uint32 [n_rows, n_cols] over the steps already run (esim_burden_series): row i is step first_step + i * stride.
        what: "occupancy" (beds occupied after that step), "admissions" or "deaths" (those of the `stride` steps from that one
        on).  where: "all" (one column), "home" or "group".  n_rows=None: up to the last step run."""
        code = {k: i for i, k in enumerate(_lib.BURDEN_NAMES)}.get(what, what)
        place, n_cols = self._burden_where(where)
        return self._series(self.lib.esim_burden_series, (place, code), n_cols, first_step, n_rows, stride)

    def burden_summary(self, where="all", first_step=1, last_step=None, threshold=1):
        """curve_summary of the bed occupancy over first_step .. last_step (None: the last step run), a dict of [n_cols] arrays
        (esim_burden_summary): peak, peak_step, steps_at_least, first_at_least, last_at_least as there, bed_steps (uint64) the
        sum of the curve, and the admissions and deaths of the window."""
        place, n_cols = self._burden_where(where)
        last = self._steps if last_step is None else int(last_step)
        out = {k: np.zeros(n_cols, np.uint64 if k == "bed_steps" else np.uint32) for k in self.BURDEN_KEYS}
        ptrs = [out[k].ctypes.data_as(C.POINTER(C.c_uint64 if k == "bed_steps" else C.c_uint32)) for k in self.BURDEN_KEYS]
        _lib.check(self.lib.esim_burden_summary(self._ctx, place, int(first_step), last, int(threshold), *ptrs), self._ctx)
        return out

    def ensemble_begin_burden_peaks(self, where="all", first_step=1, last_step=None, threshold=1, min_peak=1):
        """The peaks kind of the accumulators over the bed occupancy (esim_ensemble_begin_burden_peaks): ensemble_fold computes
        the member's burden_summary(where, first_step, last_step, threshold) on the device and folds it as ensemble_begin_peaks
        folds a status curve; ensemble_read_peaks reads them.  last_step=None: the last step of the run (params.max_steps)."""
        place, n_cols = self._burden_where(where)
        last = int(self.params.max_steps) if last_step is None else int(last_step)
        _lib.check(self.lib.esim_ensemble_begin_burden_peaks(self._ctx, place, int(first_step), last, int(threshold), int(min_peak)), self._ctx)
        self._ens_rows = 1
        self._ens_n = n_cols

    # -- ensemble quantile maps: the members kept on the device, order statistics per cell (esim_ensemble_keep_members) -------
    KEEP_WHAT = {"value": _lib.KEEP_VALUE, "peak_step": _lib.KEEP_PEAK_STEP, "duration": _lib.KEEP_DURATION}

    def ensemble_keep_members(self, capacity, what="value"):
        """Keeps every member folded from here on the device, beside the accumulators of the begin in force (any kind but
        reproduction; call it behind the begin and in front of the first fold): capacity x rows x columns x 4 B.  A member's
        value per cell: the census count, the arrival step (_lib.NEVER: not reached by the horizon), the cell of the series or
        settings rows, baseline - current for the paired kind (signed), and for the peaks kind what="value" (the peak),
        "peak_step" (_lib.NEVER without a peak) or "duration" (steps_at_least).  With the store full, ensemble_fold refuses."""
        code = self.KEEP_WHAT.get(what, what)
        if not isinstance(code, int):
            raise ValueError("Simulator.ensemble_keep_members: what must be 'value', 'peak_step' or 'duration', got %r" % (what,))
        _lib.check(self.lib.esim_ensemble_keep_members(self._ctx, int(capacity), code), self._ctx)

    def ensemble_members_info(self):
        """{"capacity", "kept", "what", "signed"} of the store (esim_ensemble_members_info)."""
        cap, kept, what, signed = C.c_uint32(0), C.c_uint32(0), C.c_int(0), C.c_int(0)
        _lib.check(self.lib.esim_ensemble_members_info(self._ctx, C.byref(cap), C.byref(kept), C.byref(what), C.byref(signed)), self._ctx)
        names = {v: k for k, v in self.KEEP_WHAT.items()}
        return {"capacity": int(cap.value), "kept": int(kept.value), "what": names[int(what.value)], "signed": bool(signed.value)}

    def _members_rows(self, first_row, n_rows):
        total = max(1, int(getattr(self, "_ens_rows", 1)))
        return int(first_row), (total - int(first_row) if n_rows is None else int(n_rows)), int(getattr(self, "_ens_n", self.population.n_areas))

    def ensemble_members(self, first_member=0, n_members=None, first_row=0, n_rows=None):
        """[members, rows, cols]: the values kept, members in the order of their folds; int32 for the paired kind, uint32
        otherwise (esim_ensemble_read_members).  n_members=None: all from first_member on; n_rows=None: all from first_row on."""
        info = self.ensemble_members_info()
        first_row, n, cols = self._members_rows(first_row, n_rows)
        m = info["kept"] - int(first_member) if n_members is None else int(n_members)
        out = np.zeros((max(0, m), max(0, n), cols), np.uint32)
        _lib.check(self.lib.esim_ensemble_read_members(self._ctx, int(first_member), max(0, m), first_row, max(0, n), out.ctypes.data_as(C.POINTER(C.c_uint32))), self._ctx)
        return out.view(np.int32) if info["signed"] else out

    def _members_ranks(self, ranks, first_row, n_rows, signed):
        first_row, n, cols = self._members_rows(first_row, n_rows)
        ranks = np.ascontiguousarray(ranks, np.uint32).reshape(-1)
        out = np.zeros((ranks.size, max(0, n), cols), np.uint32)
        _lib.check(self.lib.esim_ensemble_quantiles(self._ctx, first_row, max(0, n), ranks.ctypes.data_as(C.POINTER(C.c_uint32)), ranks.size,
                                                    out.ctypes.data_as(C.POINTER(C.c_uint32))), self._ctx)
        return out.view(np.int32) if signed else out

    def ensemble_quantiles(self, probs=(0.05, 0.5, 0.95), method="nearest", first_row=0, n_rows=None, ranks=None):
        """[len(probs), rows, cols]: quantiles per cell over the members kept, selected on the device (esim_ensemble_quantiles).
        method="nearest": the inverted CDF, the smallest value v with at least p * M members <= v -- rank max(0, ceil(p * M) - 1),
        an exact integer array (int32 for the paired kind, uint32 otherwise; _lib.NEVER sorts last).  method="linear": numpy's
        default, the two neighbouring ranks of p * (M - 1) interpolated in float64, NaN where either is _lib.NEVER.  ranks=
        (0-based, any order, at most 16 a call here too) bypasses both and returns those order statistics."""
        info = self.ensemble_members_info()
        kept, signed = info["kept"], info["signed"]
        if ranks is not None:
            return self._members_ranks(ranks, first_row, n_rows, signed)
        if method not in ("nearest", "linear"):
            raise ValueError("Simulator.ensemble_quantiles: method must be 'nearest' or 'linear', got %r" % (method,))
        probs = check_probs("Simulator.ensemble_quantiles", probs)
        if kept == 0 or not probs:
            return self._members_ranks(np.zeros(len(probs), np.uint32), first_row, n_rows, signed)     # (the library's refusal)
        if method == "nearest":
            want = [nearest_rank(p, kept) for p in probs]
        else:
            pairs = [linear_ranks(p, kept) for p in probs]
            want = [r for lo, hi, _ in pairs for r in (lo, hi)]
        distinct = sorted(set(want))
        got = {}
        for i in range(0, len(distinct), _lib.RANKS_MAX):
            part = distinct[i:i + _lib.RANKS_MAX]
            for r, plane in zip(part, self._members_ranks(part, first_row, n_rows, signed)):
                got[r] = plane
        if method == "nearest":
            return np.stack([got[r] for r in want])
        return np.stack([interpolate_linear(got[lo], got[hi], frac) for lo, hi, frac in pairs])

    def ensemble_exceedance(self, thresholds, first_row=0, n_rows=None):
        """uint32 [len(thresholds), rows, cols]: the members kept whose value is >= each threshold, chosen after the folds
        (esim_ensemble_exceedance; at most 16 thresholds a call of the library, more are split here).  Signed comparison for the
        paired kind; where _lib.NEVER occurs (arrival, peak_step) a member at it counts as >= every threshold."""
        first_row, n, cols = self._members_rows(first_row, n_rows)
        thr = np.ascontiguousarray(thresholds, np.int64).reshape(-1)
        out = np.zeros((thr.size, max(0, n), cols), np.uint32)
        for i in range(0, max(1, thr.size), _lib.RANKS_MAX):                       # (out[i:i + k] is contiguous: the library writes into it)
            k = min(_lib.RANKS_MAX, thr.size - i)
            _lib.check(self.lib.esim_ensemble_exceedance(self._ctx, first_row, max(0, n), thr[i:].ctypes.data_as(C.POINTER(C.c_int64)), k,
                                                         out[i:].ctypes.data_as(C.POINTER(C.c_uint32))), self._ctx)
        return out

    def download_state(self):
        n = self.population.n_citizens
        out = {"status": np.zeros(n, np.uint8), "timer": np.zeros(n, np.uint16),
               "current_building": np.zeros(n, np.uint32), "on_bus": np.zeros(n, np.uint8),
               "eligible": np.zeros(n, np.uint8)}
        p = lambda a, t: a.ctypes.data_as(C.POINTER(t))
        _lib.check(self.lib.esim_download_state(
            self._ctx, p(out["status"], C.c_uint8), p(out["timer"], C.c_uint16),
            p(out["current_building"], C.c_uint32), p(out["on_bus"], C.c_uint8),
            p(out["eligible"], C.c_uint8)), self._ctx)
        return out

    # -- read access the reference's callers use ----------------------
    def citizen_output_area_lookup(self):
        """`Simulator::citizen_output_area_lookup` (simulator.rs:97, rebuilt at :200-231) as two arrays: the Output
        Area every citizen currently stands in and its position in that area's `citizens` list.  The reference's
        order inside an area depends on HashMap iteration; here it is ascending global index."""
        st = self.download_state()
        area = self.population.building_area[st["current_building"]].astype(np.uint32)
        order = np.lexsort((np.arange(area.size), area))
        local = np.empty(area.size, np.uint32)
        start = np.concatenate([[0], np.cumsum(np.bincount(area, minlength=self.population.n_areas))])
        local[order] = (np.arange(area.size) - start[area[order]]).astype(np.uint32)
        return area, local

    def exposure_events(self):
        """Every exposure so far as (citizen, time_step, on_bus) arrays, sorted by (time step, citizen): the
        `add_exposure` calls of the run (statistics.rs:181-195)."""
        n = C.c_uint32(0)
        rc = self.lib.esim_download_exposure_log(self._ctx, None, None, None, 0, C.byref(n))
        if rc not in (_lib.ESIM_OK, _lib.ESIM_ERANGE):
            _lib.check(rc, self._ctx)
        cit, step, bus = np.zeros(n.value, np.uint32), np.zeros(n.value, np.uint32), np.zeros(n.value, np.uint8)
        if n.value:
            p = lambda a, t: a.ctypes.data_as(C.POINTER(t))
            _lib.check(self.lib.esim_download_exposure_log(self._ctx, p(cit, C.c_uint32), p(step, C.c_uint32), p(bus, C.c_uint8),
                                                           n.value, C.byref(n)), self._ctx)
        order = np.lexsort((cit, step))
        return cit[order], step[order], bus[order]

    def exposures_per_output_area(self, area_codes=None):
        """What `exposures.json` holds under "OutputArea" (statistics.rs:119-136,156-171): per Output Area the number of
        building exposures in every time step that had any, in time order.  An exposure in a building is credited to the
        building's area (statistics.rs:186-190), which simulator.rs:324 makes the area the citizen stands in at that
        step: its work building's from the "starts work" arm to the "goes home" arm of an unlocked day
        (citizen.rs:176-206), its home's otherwise."""
        cit, step, bus = self.exposure_events()
        rec = self.records_so_far()
        pop = self.population
        # replay the schedule: the arm of step s runs iff no lockdown was in force, i.e. the record of step s - 1 has none
        at_work = np.zeros(len(rec) + 1, bool)
        cur = False
        for s in range(1, len(rec) + 1):
            if s == 1 or not rec["lockdown"][s - 2]:
                h = s % 24
                if h == self.params.start_hour:
                    cur = True
                elif h == self.params.end_hour:
                    cur = False
            at_work[s] = cur
        b = bus == 0
        c, s = cit[b], step[b]
        has_work = pop.work_building[c] != pop.home_building[c]
        where = np.where(at_work[s] & has_work, pop.work_building[c], pop.home_building[c])
        area = pop.building_area[where]
        out = {}
        order = np.lexsort((s, area))
        a_sorted, s_sorted = area[order], s[order]
        if len(a_sorted):
            key = a_sorted.astype(np.int64) * (len(rec) + 2) + s_sorted
            uniq, counts = np.unique(key, return_counts=True)
            for k, n in zip(uniq.tolist(), counts.tolist()):
                a = k // (len(rec) + 2)
                out.setdefault(area_codes[a] if area_codes else "OA%07d" % a, []).append(n)
        return out

    def records_so_far(self):
        n = self._steps
        buf = (_lib.StepResult * max(1, n))()
        _lib.check(self.lib.esim_read_records(self._ctx, 1, n, buf), self._ctx)
        return np.frombuffer(buf, dtype=RECORD_DTYPE, count=n).copy()

    # -- checkpoint / resume --------------------------------------------------------------
    def save_checkpoint(self, path):
        """Everything needed to continue this run later, bit for bit (esim_checkpoint_save), as one file."""
        size = C.c_size_t(0)
        _lib.check(self.lib.esim_checkpoint_size(self._ctx, C.byref(size)), self._ctx)
        buf = np.empty(size.value, np.uint8)
        _lib.check(self.lib.esim_checkpoint_save(self._ctx, buf.ctypes.data_as(C.c_void_p), size.value), self._ctx)
        with open(path, "wb") as f:
            buf.tofile(f)

    def load_checkpoint(self, path):
        """Continue a run saved by `save_checkpoint` with the same population and parameters."""
        buf = np.fromfile(path, np.uint8)
        _lib.check(self.lib.esim_checkpoint_restore(self._ctx, buf.ctypes.data_as(C.c_void_p), buf.size), self._ctx)
        # the number of steps done is in the control block; find it through the records
        probe = _lib.StepResult()
        lo, hi = 0, int(self.params.max_steps)
        while lo < hi:                                           # records are written in order: last one with a time step
            mid = (lo + hi + 1) // 2
            _lib.check(self.lib.esim_read_records(self._ctx, mid, 1, C.byref(probe)), self._ctx)
            if probe.time_step == mid:
                lo = mid
            else:
                hi = mid - 1
        self._steps = lo
        self.statistics_recorder = StatisticsRecorder()
        if lo:
            self.statistics_recorder.push_block(self.records_so_far())

    def infected_per_area(self):
        """Infected citizens per Output Area where they currently stand (the heat-map `visualisation` draws from
        `output_areas[..].citizens`, run/src/main.rs:246-259)."""
        st = self.download_state()
        area = self.population.building_area[st["current_building"]]
        return np.bincount(area[st["status"] == _lib.INFECTED], minlength=self.population.n_areas)

    def area_census(self, where="current"):
        """uint32 [n_areas, 5]: citizens per Output Area and DiseaseStatus after the last completed step, counted on the
        device (esim_area_census).  where: "current" (the area of the building a citizen stands in) or "home"."""
        code = {"current": _lib.AREA_CURRENT, "home": _lib.AREA_HOME}.get(where, where)
        out = np.zeros((self.population.n_areas, 5), np.uint32)
        _lib.check(self.lib.esim_area_census(self._ctx, int(code), out.ctypes.data_as(C.POINTER(C.c_uint32))), self._ctx)
        return out

    def area_arrival(self, where="home"):
        """uint32 [n_areas] (where="home") or [n_groups] (where="group"): the step at which a citizen of the area (by
        household) or group was first exposed, counted on the device from the exposure log (esim_area_arrival); 0 where an
        initially infected citizen lives, _lib.NEVER where the epidemic has not arrived in the steps run so far."""
        code = {"current": _lib.AREA_CURRENT, "home": _lib.AREA_HOME, "group": _lib.BY_GROUP}.get(where, where)   # ("current": refused by the library)
        out = np.zeros(max(1, self._n_groups) if code == _lib.BY_GROUP else self.population.n_areas, np.uint32)
        _lib.check(self.lib.esim_area_arrival(self._ctx, int(code), out.ctypes.data_as(C.POINTER(C.c_uint32))), self._ctx)
        return out

    def _series(self, call, codes, n_cols, first_step, n_rows, stride):
        """One of the three series calls: uint32 [n_rows, n_cols]; n_rows=None: up to the last step run."""
        if n_rows is None:
            n_rows = (self._steps - int(first_step)) // int(stride) + 1 if stride and 1 <= first_step <= self._steps else 0
        out = np.zeros((max(0, int(n_rows)), n_cols), np.uint32)
        _lib.check(call(self._ctx, *(int(c) for c in codes), int(first_step), int(n_rows), int(stride),
                        out.ctypes.data_as(C.POINTER(C.c_uint32))), self._ctx)
        return out

    def area_series(self, what, first_step=1, n_rows=None, stride=1):
        """uint32 [n_rows, n_areas] over the steps already run (esim_area_series): row i is step first_step + i * stride.
        what: "infected" (citizens Infected after that step, by the area they stand in) or "exposures" (building exposures
        of the `stride` steps from that one on, by area).  n_rows=None: up to the last step run."""
        code = {"infected": _lib.SERIES_INFECTED, "exposures": _lib.SERIES_EXPOSURES}.get(what, what)
        return self._series(self.lib.esim_area_series, (code,), self.population.n_areas, first_step, n_rows, stride)

    def area_status_series(self, what, where="home", first_step=1, n_rows=None, stride=1):
        """uint32 [n_rows, n_areas] over the steps already run (esim_area_status_series): row i is step first_step + i * stride.
        what: "susceptible", "exposed", "infected", "recovered", "vaccinated" (citizens with that status after the step, by
        the area of their household, where="home", or the area they stand in, where="current") or "incidence" (building and
        public-transport exposures of the `stride` steps from that one on, by the household's area; where="home" only).
        n_rows=None: up to the last step run."""
        code = {"susceptible": _lib.SUSCEPTIBLE, "exposed": _lib.EXPOSED, "infected": _lib.INFECTED, "recovered": _lib.RECOVERED,
                "vaccinated": _lib.VACCINATED, "incidence": _lib.AREA_SERIES_INCIDENCE}.get(what, what)
        place = {"current": _lib.AREA_CURRENT, "home": _lib.AREA_HOME}.get(where, where)
        return self._series(self.lib.esim_area_status_series, (place, code), self.population.n_areas, first_step, n_rows, stride)

    # -- the same by citizen group (esim_set_groups, esim_group_census, esim_group_series) -------
    _n_groups = 0

    def set_groups(self, labels, n_groups=None):
        """One label per citizen (copied to the device as uint16); n_groups=None: the largest label + 1.  labels=None drops
        them.  Population.age_bands() and Population.occupation_groups() make such labels."""
        if labels is None:
            _lib.check(self.lib.esim_set_groups(self._ctx, None, 0), self._ctx)
            self._n_groups = 0
            return
        raw = np.asarray(labels)
        if raw.shape != (self.population.n_citizens,):
            raise ValueError("set_groups: one label per citizen, got shape %s" % (raw.shape,))
        if raw.size and (int(raw.min()) < 0 or int(raw.max()) > 0xFFFF):
            raise ValueError("set_groups: labels must fit uint16")
        lab = np.ascontiguousarray(raw, np.uint16)
        if n_groups is None:
            n_groups = int(lab.max()) + 1 if lab.size else 1
        _lib.check(self.lib.esim_set_groups(self._ctx, lab.ctypes.data_as(C.POINTER(C.c_uint16)), int(n_groups)), self._ctx)
        self._n_groups = int(n_groups)

    def group_census(self):
        """uint32 [n_groups, 5]: citizens per group and DiseaseStatus after the last completed step, counted on the device
        (esim_group_census)."""
        out = np.zeros((max(1, self._n_groups), 5), np.uint32)
        _lib.check(self.lib.esim_group_census(self._ctx, out.ctypes.data_as(C.POINTER(C.c_uint32))), self._ctx)
        return out

    def group_series(self, what, first_step=1, n_rows=None, stride=1):
        """uint32 [n_rows, n_groups] over the steps already run (esim_group_series): row i is step first_step + i * stride.
        what: "susceptible", "exposed", "infected", "recovered", "vaccinated" (citizens of the group with that status after
        the step) or "exposures" (building and public-transport exposures of the `stride` steps from that one on, by the
        group of the exposed citizen).  n_rows=None: up to the last step run."""
        code = {"susceptible": _lib.SUSCEPTIBLE, "exposed": _lib.EXPOSED, "infected": _lib.INFECTED, "recovered": _lib.RECOVERED,
                "vaccinated": _lib.VACCINATED, "exposures": _lib.GROUP_SERIES_EXPOSURES}.get(what, what)
        return self._series(self.lib.esim_group_series, (code,), max(1, self._n_groups), first_step, n_rows, stride)

    # -- exposures by setting (esim_exposure_settings, esim_setting_series, esim_building_exposures) -------
    def exposure_settings(self):
        """(setting uint8 [n_citizens], building uint32 [n_citizens]): where every citizen was exposed, derived on the device
        from the exposure log by replaying the household draw (esim_exposure_settings).  setting: _lib.SETTING_HOUSEHOLD,
        SETTING_WORKPLACE, SETTING_SCHOOL, SETTING_TRANSPORT, or SETTING_NONE for a citizen never exposed and for the index
        cases; building: the building credited, _lib.NO_ROOM for public transport and for SETTING_NONE.  A tie between the
        household and the work side is credited to the household."""
        n = self.population.n_citizens
        setting, building = np.zeros(n, np.uint8), np.zeros(n, np.uint32)
        _lib.check(self.lib.esim_exposure_settings(self._ctx, setting.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                   building.ctypes.data_as(C.POINTER(C.c_uint32))), self._ctx)
        return setting, building

    @staticmethod
    def _setting_mask(settings):
        if settings is None:
            return (1 << _lib.N_SETTINGS) - 1
        if isinstance(settings, (str, int, np.integer)):
            settings = (settings,)
        mask = 0
        for s in settings:
            code = _lib.SETTING_NAMES.index(s) if isinstance(s, str) else int(s)
            if not 0 <= code < _lib.N_SETTINGS:
                raise ValueError("setting_series: unknown setting %r" % (s,))
            mask |= 1 << code
        return mask

    def setting_series(self, where="setting", settings=None, first_step=1, n_rows=None, stride=1):
        """uint32 [n_rows, n_cols] over the steps already run (esim_setting_series): row i holds the exposures, in buildings
        and on public transport, of the `stride` steps from first_step + i * stride on, restricted to `settings` (names out
        of "household", "workplace", "school", "transport", or their codes; None: all four).  where: "setting" (four columns),
        "home" (by the Output Area of the household) or "group".  n_rows=None: up to the last step run."""
        place = {"setting": _lib.BY_SETTING, "home": _lib.AREA_HOME, "group": _lib.BY_GROUP, "current": _lib.AREA_CURRENT}.get(where, where)   # ("current": refused by the library)
        n_cols = _lib.N_SETTINGS if place == _lib.BY_SETTING else max(1, self._n_groups) if place == _lib.BY_GROUP else self.population.n_areas
        return self._series(self.lib.esim_setting_series, (place, self._setting_mask(settings)), n_cols, first_step, n_rows, stride)

    def building_exposures(self, first_step=1, last_step=None):
        """uint32 [n_buildings]: the exposures of steps first_step .. last_step (None: the last step run) per building
        credited -- the hot-spot map (esim_building_exposures).  Public transport is not counted."""
        out = np.zeros(self.population.n_buildings, np.uint32)
        last = self._steps if last_step is None else int(last_step)
        _lib.check(self.lib.esim_building_exposures(self._ctx, int(first_step), last, out.ctypes.data_as(C.POINTER(C.c_uint32))), self._ctx)
        return out

    # -- who infected whom (esim_transmission_tree, esim_offspring, esim_reproduction_series, esim_mixing_matrix) -------
    def transmission_tree(self):
        """(infector, n_candidates, generation), uint32 [n_citizens] each, derived on the device from the exposure log
        (esim_transmission_tree).  infector: the citizen every exposure is credited to -- one of the Infected that stood where
        it happened, picked by a Philox draw of its own --, _lib.NO_INFECTOR for the index cases and for citizens never
        exposed; n_candidates: how many there were to pick from; generation: 0 for an index case, the infector's + 1
        otherwise, _lib.NEVER for a citizen never exposed."""
        n = self.population.n_citizens
        out = [np.zeros(n, np.uint32) for _ in range(3)]
        _lib.check(self.lib.esim_transmission_tree(self._ctx, *(a.ctypes.data_as(C.POINTER(C.c_uint32)) for a in out)), self._ctx)
        return tuple(out)

    def offspring(self, first_step=1, last_step=None):
        """uint32 [n_citizens]: how many of the citizens exposed in steps first_step .. last_step (None: the last step run)
        every citizen infected (esim_offspring)."""
        out = np.zeros(self.population.n_citizens, np.uint32)
        last = self._steps if last_step is None else int(last_step)
        _lib.check(self.lib.esim_offspring(self._ctx, int(first_step), last, out.ctypes.data_as(C.POINTER(C.c_uint32))), self._ctx)
        return out

    def reproduction_series(self, where="all", first_step=0, n_rows=None, stride=24):
        """(cases, offspring), uint32 [n_rows, n_cols] each (esim_reproduction_series): row i is the cohort exposed in the
        `stride` steps from first_step + i * stride on (step 0: the index cases), `cases` its size and `offspring` the
        citizens it infected, by the infector's column; offspring / cases is the cohort's case reproduction number.  where:
        "all" (one column), "home" (by the Output Area of the household) or "group".  n_rows=None: up to the last step run."""
        place = {"all": _lib.BY_ALL, "home": _lib.AREA_HOME, "group": _lib.BY_GROUP, "current": _lib.AREA_CURRENT}.get(where, where)   # ("current": refused by the library)
        n_cols = 1 if place == _lib.BY_ALL else max(1, self._n_groups) if place == _lib.BY_GROUP else self.population.n_areas
        if n_rows is None:
            n_rows = (self._steps - int(first_step)) // int(stride) + 1 if stride and 0 <= first_step <= self._steps else 0
        cases, offspring = (np.zeros((max(0, int(n_rows)), n_cols), np.uint32) for _ in range(2))
        _lib.check(self.lib.esim_reproduction_series(self._ctx, int(place), int(first_step), int(n_rows), int(stride),
                                                     cases.ctypes.data_as(C.POINTER(C.c_uint32)), offspring.ctypes.data_as(C.POINTER(C.c_uint32))), self._ctx)
        return cases, offspring

    def mixing_matrix(self, settings=None, first_step=1, last_step=None):
        """uint32 [n_groups, n_groups]: entry [g_infector, g_infectee] counts the transmissions of steps first_step ..
        last_step (None: the last step run) between the groups of set_groups, restricted to `settings` as setting_series
        takes them (esim_mixing_matrix)."""
        g = max(1, self._n_groups)
        out = np.zeros((g, g), np.uint32)
        last = self._steps if last_step is None else int(last_step)
        _lib.check(self.lib.esim_mixing_matrix(self._ctx, self._setting_mask(settings), int(first_step), last, out.ctypes.data_as(C.POINTER(C.c_uint32))), self._ctx)
        return out

    # -- transmission chains (esim_transmission_chains, esim_outbreaks, esim_transmission_ages) -------
    def transmission_chains(self):
        """(lineage, descendants), uint32 [n_citizens] each (esim_transmission_chains).  lineage: the position in seeds() of
        the index case at the root of the citizen's chain -- an index case carries its own --, _lib.NO_LINEAGE for a citizen
        never exposed; descendants: the citizens in the subtree below the citizen, itself not counted."""
        out = [np.zeros(self.population.n_citizens, np.uint32) for _ in range(2)]
        _lib.check(self.lib.esim_transmission_chains(self._ctx, *(a.ctypes.data_as(C.POINTER(C.c_uint32)) for a in out)), self._ctx)
        return tuple(out)

    def outbreaks(self):
        """The outbreak every index case started (esim_outbreaks), a dict of uint32 [n_seeds] arrays in the order of seeds():
        seeds, size (the descendants of the index case), depth (the largest generation of its lineage, 0 when it infected
        nobody) and last_step (the last exposure step of its lineage, 0 when none).  Nothing per citizen comes to the host."""
        seeds = self.seeds()
        out = {k: np.zeros(len(seeds), np.uint32) for k in ("size", "depth", "last_step")}
        n = C.c_uint32(0)
        _lib.check(self.lib.esim_outbreaks(self._ctx, *(out[k].ctypes.data_as(C.POINTER(C.c_uint32)) for k in ("size", "depth", "last_step")),
                                           len(seeds), C.byref(n)), self._ctx)
        return dict(out, seeds=seeds)

    def transmission_ages(self, first_step=1, last_step=None):
        """uint32 [4, 512]: entry [setting, a] counts the transmissions of steps first_step .. last_step (None: the last step
        run; the step is the infectee's) made in step a of the infector's infectious period, a = 0 its first Infected step
        (esim_transmission_ages).  For an infector that is not an index case the generation interval is a + exposed_time + 1."""
        out = np.zeros((_lib.N_SETTINGS, _lib.AGE_BINS), np.uint32)
        last = self._steps if last_step is None else int(last_step)
        _lib.check(self.lib.esim_transmission_ages(self._ctx, int(first_step), last, out.ctypes.data_as(C.POINTER(C.c_uint32))), self._ctx)
        return out

    # -- household outbreaks (esim_household_outbreaks, esim_household_final_sizes, esim_household_sar) -------
    def household_outbreaks(self):
        """Per building, a dict of uint32 [n_buildings] arrays (esim_household_outbreaks): cases (the residents in the exposure
        log, index cases included), introductions (of those, the index cases and the cases not infected at home) and first_step
        (the smallest cohort step among them, _lib.NEVER without a case)."""
        keys = ("cases", "introductions", "first_step")
        out = {k: np.zeros(self.population.n_buildings, np.uint32) for k in keys}
        _lib.check(self.lib.esim_household_outbreaks(self._ctx, *(out[k].ctypes.data_as(C.POINTER(C.c_uint32)) for k in keys)), self._ctx)
        return out

    def household_final_sizes(self):
        """(final_size, introductions), uint32 [64, 64] each (esim_household_final_sizes): entry [n, k] counts the households
        of n residents with k cases, or with k introductions; the last bin of either index holds everything from 63 on.
        Nothing per building or per citizen comes to the host."""
        out = [np.zeros((_lib.HH_BINS, _lib.HH_BINS), np.uint32) for _ in range(2)]
        _lib.check(self.lib.esim_household_final_sizes(self._ctx, *(a.ctypes.data_as(C.POINTER(C.c_uint32)) for a in out)), self._ctx)
        return tuple(out)

    def household_sar(self, where="all", first_step=0, last_step=None, complete=True):
        """(at_risk, secondary), uint64 [n_cols, n_cols] each (esim_household_sar): over the cases of cohort steps first_step ..
        last_step (step 0: the index cases), entry [g_case, g_contact] of at_risk counts the housemates still Susceptible when
        the case became infectious, of secondary those it infected at home; secondary / at_risk is the household secondary
        attack rate.  where: "all" (one cell) or "group".  last_step=None: the last step run.  complete=True clips last_step to
        the last complete cohort -- last_step + exposed_time + 1 + infected_time <= the steps run -- and raises ValueError when
        there is none; complete=False counts cohorts whose cases may still infect."""
        place = {"all": _lib.BY_ALL, "group": _lib.BY_GROUP}.get(where, where)
        n_cols = max(1, self._n_groups) if place == _lib.BY_GROUP else 1
        first = int(first_step)
        last = self._steps if last_step is None else int(last_step)
        if complete:
            done = self._steps - int(self.params.exposed_time) - 1 - int(self.params.infected_time)
            last = min(last, done)
            if last < max(first, 0):
                raise ValueError("household_sar: no complete cohort in steps %d..%d after %d steps (complete=False counts the open ones)" % (first, last if last_step is None else int(last_step), self._steps))
        at_risk, secondary = (np.zeros((n_cols, n_cols), np.uint64) for _ in range(2))
        _lib.check(self.lib.esim_household_sar(self._ctx, int(place), first, last, at_risk.ctypes.data_as(C.POINTER(C.c_uint64)),
                                               secondary.ctypes.data_as(C.POINTER(C.c_uint64))), self._ctx)
        return at_risk, secondary

    # -- work place and school outbreaks (esim_place_outbreaks, esim_place_sizes, esim_place_sar) -------
    @staticmethod
    def _place_kind(kind):
        return {"work": _lib.PLACE_WORK, "room": _lib.PLACE_ROOM, "school": _lib.PLACE_SCHOOL}.get(kind, kind)

    def place_outbreaks(self, kind="work"):
        """Per place, a dict of uint32 arrays (esim_place_outbreaks): members, cases (the members in the exposure log, index
        cases included), introductions (of those, the index cases and the cases not infected in the place's own setting) and
        first_step (the smallest cohort step among them, _lib.NEVER without a case).  kind: "work" (the non-school buildings
        and their workers, [n_buildings]), "room" (the school rooms and their participants, [n_rooms]) or "school" (the school
        buildings, all their rooms together, [n_buildings]).  A building or room without a member has 0 everywhere."""
        kind = self._place_kind(kind)
        n = self.population.n_rooms if kind == _lib.PLACE_ROOM else self.population.n_buildings
        keys = ("members", "cases", "introductions", "first_step")
        out = {k: np.zeros(n, np.uint32) for k in keys}
        _lib.check(self.lib.esim_place_outbreaks(self._ctx, int(kind), *(out[k].ctypes.data_as(C.POINTER(C.c_uint32)) for k in keys)), self._ctx)
        return out

    def place_sizes(self, kind="work"):
        """(final_size, introduced), uint32 [32, 32] each (esim_place_sizes): entry [bin(members), bin(k)] counts the places of
        the kind with k cases, or with k introductions; bin(x) = x below 16, then 16 for 16..31, 17 for 32..63 and so on."""
        out = [np.zeros((_lib.PLACE_BINS, _lib.PLACE_BINS), np.uint32) for _ in range(2)]
        _lib.check(self.lib.esim_place_sizes(self._ctx, int(self._place_kind(kind)), *(a.ctypes.data_as(C.POINTER(C.c_uint32)) for a in out)), self._ctx)
        return tuple(out)

    def place_sar(self, kind="work", where="all", first_step=0, last_step=None, complete=True):
        """(at_risk, secondary), uint64 [n_cols, n_cols] each (esim_place_sar): household_sar for the work places (kind="work")
        or the school rooms (kind="room") -- entry [g_case, g_contact] of at_risk counts the colleagues or class-mates still
        Susceptible when the case became infectious, of secondary those it infected there.  where, first_step, last_step and
        complete as for household_sar, with the same clipping and the same ValueError."""
        place = {"all": _lib.BY_ALL, "group": _lib.BY_GROUP}.get(where, where)
        n_cols = max(1, self._n_groups) if place == _lib.BY_GROUP else 1
        first = int(first_step)
        last = self._steps if last_step is None else int(last_step)
        if complete:
            done = self._steps - int(self.params.exposed_time) - 1 - int(self.params.infected_time)
            last = min(last, done)
            if last < max(first, 0):
                raise ValueError("place_sar: no complete cohort in steps %d..%d after %d steps (complete=False counts the open ones)" % (first, last if last_step is None else int(last_step), self._steps))
        at_risk, secondary = (np.zeros((n_cols, n_cols), np.uint64) for _ in range(2))
        _lib.check(self.lib.esim_place_sar(self._ctx, int(self._place_kind(kind)), int(place), first, last, at_risk.ctypes.data_as(C.POINTER(C.c_uint64)),
                                           secondary.ctypes.data_as(C.POINTER(C.c_uint64))), self._ctx)
        return at_risk, secondary

    # -- contact-hours at risk (esim_contact_hours) -------
    def contact_hours(self, where="all", settings=None, first_step=1, last_step=None, per_case=False):
        """dict: hours and transmissions, uint64 [4, n_cols, n_cols] each, and with per_case=True per_case, uint32 [n_citizens]
        (esim_contact_hours).  hours[s, g_infected, g_susceptible] counts the contact-hours of setting s in steps first_step ..
        last_step (None: the last step run): a Susceptible citizen taking the draw of a gathering in a step in which an
        Infected citizen is a candidate of it.  transmissions is the mixing matrix split by setting; transmissions <= hours
        cell for cell.  per_case[j]: the contact-hours with j as the Infected side.  where: "all" (one cell) or "group";
        settings as setting_series takes them (the planes of the others stay 0)."""
        place = {"all": _lib.BY_ALL, "group": _lib.BY_GROUP}.get(where, where)
        n_cols = max(1, self._n_groups) if place == _lib.BY_GROUP else 1
        last = self._steps if last_step is None else int(last_step)
        out = {k: np.zeros((_lib.N_SETTINGS, n_cols, n_cols), np.uint64) for k in ("hours", "transmissions")}
        cases = np.zeros(self.population.n_citizens, np.uint32) if per_case else None
        u64p = C.POINTER(C.c_uint64)
        _lib.check(self.lib.esim_contact_hours(self._ctx, int(place), self._setting_mask(settings), int(first_step), last, out["hours"].ctypes.data_as(u64p),
                                               out["transmissions"].ctypes.data_as(u64p), cases.ctypes.data_as(C.POINTER(C.c_uint32)) if per_case else None), self._ctx)
        if per_case:
            out["per_case"] = cases
        return out

    @staticmethod
    def _rate(transmissions, hours):
        """transmissions / hours as float64, NaN where hours == 0."""
        t, h = np.asarray(transmissions, np.float64), np.asarray(hours, np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(h > 0, t / h, np.nan)

    def contact_rates(self, where="all", settings=None, first_step=1, last_step=None):
        """float64 [4, n_cols, n_cols]: transmissions per contact-hour, contact_hours()'s transmissions / hours, NaN where there
        was no contact-hour.  In households, work places and buses this is close to exposure_chance; in school rooms far above
        it (a room draw uses the Infected count of the whole school and is taken once per Infected of the room)."""
        got = self.contact_hours(where, settings, first_step, last_step)
        return self._rate(got["transmissions"], got["hours"])

    # -- area flows (esim_area_flows, esim_area_imports, esim_area_invasion, esim_lineage_areas) -------
    def _pairs(self, call, args):
        """The three [n] arrays of a sparse output: one call with cap=0 for the number of pairs, then the real one -- two
        replays, but buffers of 12 B per pair instead of 12 B per entry of the exposure log."""
        n = C.c_uint32(0)
        code = call(self._ctx, *args, None, None, None, 0, C.byref(n))
        out = [np.zeros(n.value, np.uint32) for _ in range(3)]
        if code == _lib.ESIM_ERANGE:      # buffers of n pairs are needed -- or the steps lie outside the run, which the second call says again
            code = call(self._ctx, *args, *(a.ctypes.data_as(C.POINTER(C.c_uint32)) for a in out), n.value, C.byref(n))
        _lib.check(code, self._ctx)
        return tuple(out)

    def area_flows(self, settings=None, first_step=1, last_step=None):
        """(src, dst, count), uint32 [n_pairs] each (esim_area_flows): the distinct pairs (Output Area of the infector, of the
        infectee) over the transmissions of steps first_step .. last_step (None: the last step run), restricted to `settings`
        as setting_series takes them, ascending by (src, dst), and how many transmissions each pair saw.  Sized by one call with
        cap=0 before the real one.  Nothing per citizen comes to the host."""
        last = self._steps if last_step is None else int(last_step)
        return self._pairs(self.lib.esim_area_flows, (self._setting_mask(settings), int(first_step), last))

    def area_imports(self, settings=None, first_step=1, last_step=None):
        """Per Output Area, a dict of uint32 [n_areas] arrays (esim_area_imports) over the same transmissions as area_flows:
        local (both ends in the area), imported (the infectee lives there, the infector elsewhere) and exported (the other way
        round)."""
        keys = ("local", "imported", "exported")
        out = {k: np.zeros(self.population.n_areas, np.uint32) for k in keys}
        last = self._steps if last_step is None else int(last_step)
        _lib.check(self.lib.esim_area_imports(self._ctx, self._setting_mask(settings), int(first_step), last,
                                              *(out[k].ctypes.data_as(C.POINTER(C.c_uint32)) for k in keys)), self._ctx)
        return out

    def area_invasion(self):
        """The between-area invasion tree, a dict of [n_areas] arrays (esim_area_invasion): first_case (the earliest case
        living in the area, of several in one step the smallest citizen index; _lib.NO_INFECTOR without one), step (its cohort
        step, 0 for an index case, _lib.NEVER without a case: area_arrival("home")), source_area (the area of its infector,
        _lib.NO_AREA for an index case or no case) and setting (uint8, _lib.SETTING_NONE likewise).  step[source_area[a]] <
        step[a] wherever a source exists: a forest rooted at the areas of the index cases."""
        na = self.population.n_areas
        out = {k: np.zeros(na, np.uint32) for k in ("first_case", "step", "source_area")}
        out["setting"] = np.zeros(na, np.uint8)
        _lib.check(self.lib.esim_area_invasion(self._ctx, *(out[k].ctypes.data_as(C.POINTER(C.c_uint32)) for k in ("first_case", "step", "source_area")),
                                               out["setting"].ctypes.data_as(C.POINTER(C.c_uint8))), self._ctx)
        return out

    def lineage_areas(self):
        """(lineage, area, count), uint32 [n_pairs] each (esim_lineage_areas): the distinct pairs (position in seeds() of the
        index case at the root of the chain, Output Area) over all cases that have a lineage, ascending, and how many cases of
        that lineage live there.  np.bincount(lineage) is the number of areas every introduction reached."""
        return self._pairs(self.lib.esim_lineage_areas, ())

    def pair_stats(self):
        """What the pair engine did in the last area_flows(), lineage_areas() or curve_summary() call, or peaks fold (esim_pair_stats): a dict of insert_ms,
        compact_ms, sort_ms (device time, HIP events), distinct, capacity and dropped."""
        ms, counts = (C.c_double * 3)(), (C.c_uint32 * 3)()
        _lib.check(self.lib.esim_pair_stats(self._ctx, ms, counts), self._ctx)
        return dict(insert_ms=ms[0], compact_ms=ms[1], sort_ms=ms[2], distinct=int(counts[0]), capacity=int(counts[1]), dropped=int(counts[2]))

    # -- superspreading events (esim_transmission_events, esim_routes) -------
    _EVENT_KEYS = ("step", "setting", "place", "bus", "size")

    def _events(self, mask, first, last, min_size, order, out, cap, sizes=None):
        """One esim_transmission_events call into the arrays of `out` (None: no lists): (code, number of events)."""
        n = C.c_uint32(0)
        ptrs = [None] * 5 if out is None else [out[k].ctypes.data_as(C.POINTER(C.c_uint8 if k == "setting" else C.c_uint32)) for k in self._EVENT_KEYS]
        code = self.lib.esim_transmission_events(self._ctx, mask, first, last, int(min_size), int(order), *ptrs, int(cap), C.byref(n),
                                                 None if sizes is None else sizes.ctypes.data_as(C.POINTER(C.c_uint32)))
        return code, n.value

    def transmission_events(self, settings=None, first_step=1, last_step=None, min_size=1, order="key", limit=None):
        """The superspreading events (esim_transmission_events), a dict of [n_events] arrays: step, setting (uint8), place (the
        building, the room, or the position of the route in routes()), bus (0 off public transport) and size -- the
        transmissions of one step in one gathering (household, work place, school room, bus), over steps first_step ..
        last_step (None: the last step run), restricted to `settings` as setting_series takes them, events of at least
        min_size transmissions only.  order="key": ascending by (step, setting, place, bus), sized by one call with cap=0 before
        the real one; order="size": descending by size, ties ascending by that key, the first `limit` of them (None: all, sized
        the same way) in one call.  Nothing per citizen comes to the host."""
        if order not in ("key", "size"):
            raise ValueError("transmission_events: order must be 'key' or 'size', got %r" % (order,))
        mask, first = self._setting_mask(settings), int(first_step)
        last = self._steps if last_step is None else int(last_step)
        by = _lib.EVENTS_BY_SIZE if order == "size" else _lib.EVENTS_BY_KEY

        def arrays(n):
            return {k: np.zeros(n, np.uint8 if k == "setting" else np.uint32) for k in self._EVENT_KEYS}
        if order == "size" and limit is not None:
            out = arrays(int(limit))
            code, n = self._events(mask, first, last, min_size, by, out, int(limit))
            _lib.check(code, self._ctx)
            return {k: v[:min(n, int(limit))] for k, v in out.items()}
        code, n = self._events(mask, first, last, min_size, _lib.EVENTS_BY_KEY, None, 0)
        out = arrays(n)
        if code == _lib.ESIM_ERANGE:      # buffers of n events are needed -- or the steps lie outside the run, which the second call says again
            code, n = self._events(mask, first, last, min_size, by, out, n)
        _lib.check(code, self._ctx)
        return out

    def event_sizes(self, settings=None, first_step=1, last_step=None):
        """uint32 [4, 256] (the size table of esim_transmission_events): entry [s, b] counts the events of setting s with b
        transmissions over the window and the settings, the last bin open-ended; no list is built or sorted."""
        sizes = np.zeros((_lib.N_SETTINGS, _lib.EVENT_BINS), np.uint32)
        last = self._steps if last_step is None else int(last_step)
        code, _ = self._events(self._setting_mask(settings), int(first_step), last, 1, _lib.EVENTS_BY_SIZE, None, 0, sizes)
        _lib.check(code, self._ctx)
        return sizes

    def routes(self):
        """The public transport routes (esim_routes), a dict of uint32 [n_routes] arrays: home_area, work_area and n_riders, in
        the order transmission_events numbers them (ascending by home area, then work area)."""
        n = C.c_uint32(0)
        code = self.lib.esim_routes(self._ctx, None, None, None, 0, C.byref(n))
        keys = ("home_area", "work_area", "n_riders")
        out = {k: np.zeros(n.value, np.uint32) for k in keys}
        if code == _lib.ESIM_ERANGE:
            code = self.lib.esim_routes(self._ctx, *(out[k].ctypes.data_as(C.POINTER(C.c_uint32)) for k in keys), n.value, C.byref(n))
        _lib.check(code, self._ctx)
        return out

    def enable_kernel_timing(self, stride):
        _lib.check(self.lib.esim_enable_kernel_timing(self._ctx, int(stride)), self._ctx)

    def kernel_timings(self):
        ms = C.c_double(0)
        n = C.c_uint32(0)
        _lib.check(self.lib.esim_kernel_timings(self._ctx, C.byref(ms), C.byref(n)), self._ctx)
        return {"multi_kernel_step_ms": ms.value, "steps_timed": n.value}

    def set_small_step_limit(self, max_infected):
        """Steps with at most this many Infected citizens run in the persistent single-workgroup kernel
        (0 = always use the multi-workgroup kernels)."""
        _lib.check(self.lib.esim_set_small_step_limit(self._ctx, int(max_infected)), self._ctx)

    def set_tiny_chunk_limit(self, max_pairs):
        """Time-parallel chunks with at most this many (Infected citizen, step) pairs run as one launch of one workgroup
        (0 = always the wide form; default 2048)."""
        _lib.check(self.lib.esim_set_tiny_chunk_limit(self._ctx, int(max_pairs)), self._ctx)

    def set_pipeline(self, level):
        """0: sequential steps only; 1: chunks as one kernel per step; 2: time-parallel chunks; 3 (default): also under a vaccination
        programme.  Any level above 3 runs as 3."""
        _lib.check(self.lib.esim_set_pipeline(self._ctx, int(level)), self._ctx)

    def chunk_timing(self):
        ms, ns, nc = C.c_double(0), C.c_uint64(0), C.c_uint64(0)
        _lib.check(self.lib.esim_chunk_timing(self._ctx, C.byref(ms), C.byref(ns), C.byref(nc)), self._ctx)
        return {"chunk_ms": ms.value, "steps": ns.value, "chunks": nc.value}

    def debug_counters(self):
        """The control block's view of the last chunk (esim_debug_counters), by name."""
        out = (C.c_uint32 * 16)()
        _lib.check(self.lib.esim_debug_counters(self._ctx, out), self._ctx)
        return dict(zip(_lib.DEBUG_COUNTERS, (int(x) for x in out)))

    def debug_launches(self, reset=False):
        """What the output launches were sized to while ESIM_GRID_CAP is set (esim_debug_launches): {site: {"launches",
        "clipped", "max_trips"}}, a site being "<file>:<line>" of the host code.  Empty when the knob is unset.  reset: the
        records start anew after this read."""
        cap = _lib.LAUNCH_SITES_MAX
        names = C.create_string_buffer(cap * _lib.LAUNCH_SITE_CHARS)
        counts = (C.c_uint32 * (3 * cap))()
        n = C.c_uint32(0)
        _lib.check(self.lib.esim_debug_launches(self._ctx, names, counts, cap, C.byref(n), 1 if reset else 0), self._ctx)
        out = {}
        for i in range(n.value):
            raw = names.raw[i * _lib.LAUNCH_SITE_CHARS:(i + 1) * _lib.LAUNCH_SITE_CHARS]
            out[raw.split(b"\0", 1)[0].decode()] = {"launches": int(counts[3 * i]), "clipped": int(counts[3 * i + 1]), "max_trips": int(counts[3 * i + 2])}
        return out

    def vax_chunk_stats(self):
        """Steps run as chunks under a vaccination programme and how many of those chunks were cut short."""
        ns, nc = C.c_uint64(0), C.c_uint64(0)
        _lib.check(self.lib.esim_vax_chunk_stats(self._ctx, C.byref(ns), C.byref(nc)), self._ctx)
        nr = C.c_uint64(0)
        _lib.check(self.lib.esim_vax_repair_stats(self._ctx, C.byref(nr)), self._ctx)
        return {"steps": ns.value, "cuts": nc.value, "repairs": nr.value}

    def pipeline_timing(self):
        ms, nt, nr = C.c_double(0), C.c_uint64(0), C.c_uint64(0)
        _lib.check(self.lib.esim_pipeline_timing(self._ctx, C.byref(ms), C.byref(nt), C.byref(nr)), self._ctx)
        return {"k_pipe_ms": ms.value, "steps_timed": nt.value, "steps": nr.value}

    def small_kernel_timing(self):
        ms, n = C.c_double(0), C.c_uint64(0)
        _lib.check(self.lib.esim_small_kernel_timing(self._ctx, C.byref(ms), C.byref(n)), self._ctx)
        return {"k_small_ms": ms.value, "steps": n.value}

    def enable_chunk_kernel_timing(self, on=True):
        _lib.check(self.lib.esim_enable_chunk_kernel_timing(self._ctx, int(on)), self._ctx)

    def chunk_kernel_timings(self):
        """Device milliseconds and launches per kernel of the chunk pass since the last call (esim_chunk_kernel_timings)."""
        n = len(_lib.CHUNK_KERNELS)
        ms, calls = (C.c_double * n)(), (C.c_uint64 * n)()
        _lib.check(self.lib.esim_chunk_kernel_timings(self._ctx, ms, calls), self._ctx)
        return {k: {"ms": ms[i], "calls": int(calls[i])} for i, k in enumerate(_lib.CHUNK_KERNELS)}

    def chunk_phase_seconds(self):
        """The same grouped under the reference's three timer labels (simulator.rs:137,140,143), in seconds."""
        out = {"Generate Exposures": 0.0, "Apply Exposures": 0.0, "Apply Interventions": 0.0}
        for k, v in self.chunk_kernel_timings().items():
            if k == "tiny":
                # one launch holds all three phases: shared out by the kernel's own stage timers (tools/tiny_stages.py on uk64m:
                # entries and keys 10 %, the items' draws 40 %, census ahead, decisions and books 50 %)
                for phase, share in _lib.TINY_PHASE_SHARES.items():
                    out[phase] += share * v["ms"] * 1e-3
                continue
            out[_lib.PHASE_OF_KERNEL.get(k, "Apply Interventions")] += v["ms"] * 1e-3
        return out

    def enable_phase_timing(self, on=True):
        _lib.check(self.lib.esim_enable_phase_timing(self._ctx, int(on)), self._ctx)

    def phase_timings(self):
        t = (C.c_double * 4)()
        _lib.check(self.lib.esim_phase_timings(self._ctx, t), self._ctx)
        return {"Generate Exposures": t[0], "Apply Exposures": t[1], "Apply Interventions": t[2], "total": t[3]}

    def close(self):
        if self._ctx:
            self.lib.esim_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


RECORD_DTYPE = np.dtype([(n, np.uint32) for n in _lib.RECORD_FIELDS])
