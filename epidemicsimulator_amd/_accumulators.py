"""The accumulators of Simulator over the members of an ensemble, kept on the device (esim_ensemble_*): the begin of every
kind -- census, arrival, series, settings, reproduction, paired, peaks, burden peaks, burden series, burden paired --, the fold of the state as it stands,
the readers, and the members kept beside the accumulators for the quantile maps.  _Accumulators only holds methods: the state
and the helpers _n_cols and _last are Simulator's (simulator.py), _setting_mask, _compare_place, _compare_rows, _curve_args and
_burden_what the outputs' (_outputs.py) whose rows a member contributes.

A begin remembers the rows and columns it asked for (_begun): the readers and the calls on the members kept size their
buffers by them.  Its n_rows=None and last_step=None mean up to the last step of the run (params.max_steps).  The library
refuses a begin by group without labels (esim_set_groups)."""
import ctypes as C
import fractions
import math

import numpy as np

from . import _lib
from ._marshal import STATUS, default_rows, place_code, ptr, zeros


# -- the rank rules of the ensemble quantile maps (ensemble_quantiles below, Ensemble) -------
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


class _Accumulators:
    def _begun(self, n_rows, place):
        self._ens_rows, self._ens_n = int(n_rows), self._n_cols(place)

    def _begin_rows(self, first_step, n_rows, stride, lowest):
        return int(default_rows(first_step, stride, self._last(None, run=False), lowest) if n_rows is None else n_rows)

    # -- per Output Area or group: the census and the arrival step -------
    def ensemble_begin(self, where="home", status_mask=(1 << _lib.EXPOSED) | (1 << _lib.INFECTED) | (1 << _lib.RECOVERED), min_cases=1):
        place = place_code(where, "current home group")
        _lib.check(self.lib.esim_ensemble_begin(self._ctx, place, int(status_mask), int(min_cases)), self._ctx)
        self._begun(1, place)

    def ensemble_begin_arrival(self, where="home", horizon=None):
        """Accumulators of the arrival step instead (esim_ensemble_begin_arrival): a member counts as a hit where the epidemic
        reached the area (where="home") or group (where="group") by step `horizon`; None: within whatever steps it ran."""
        place = place_code(where, "current home group")
        _lib.check(self.lib.esim_ensemble_begin_arrival(self._ctx, place, _lib.NEVER if horizon is None else int(horizon)), self._ctx)
        self._begun(1, place)

    def ensemble_fold(self):
        """Adds the state as it stands to the accumulators, on the device; nothing is downloaded."""
        _lib.check(self.lib.esim_ensemble_fold(self._ctx), self._ctx)

    def _read_accumulators(self, call, keys, shape, first_row=None, n=None):
        """One read call: {key: array of `shape`, uint32 for "defined" and "hit", uint64 for the sums, "members": int}.  With
        first_row, the call takes the rows (first_row, n) in front of its outputs."""
        members = C.c_uint32(0)
        out = zeros(keys, shape, u64=[k for k in keys if k not in ("defined", "hit")])
        rows = () if first_row is None else (int(first_row), n)
        _lib.check(call(self._ctx, *rows, C.byref(members), *(ptr(out[k]) for k in keys)), self._ctx)
        return dict(out, members=int(members.value))

    def _read_rows(self, call, keys, first_row, n_rows, cols=None):
        """The rows [first_row, first_row + n) of accumulators over rows; n_rows=None: all from first_row on."""
        n = max(0, getattr(self, "_ens_rows", 0) - int(first_row)) if n_rows is None else int(n_rows)
        return self._read_accumulators(call, keys, (n, getattr(self, "_ens_n", cols or self.population.n_areas)), first_row, n)

    SERIES_KEYS = ("hit", "sum", "sumsq")

    def ensemble_read(self):
        """{"members": int, "hit": uint32 [n], "sum": uint64 [n], "sumsq": uint64 [n]}, n = n_areas, or n_groups for
        accumulators begun by group."""
        return self._read_accumulators(self.lib.esim_ensemble_read, self.SERIES_KEYS, getattr(self, "_ens_n", self.population.n_areas))

    # -- over the rows of a series, of the exposures by setting, of the cohorts and of the paired comparison -------
    def ensemble_begin_series(self, where, what, first_step=1, n_rows=None, stride=1, min_cases=1):
        """Accumulators over the rows of a series instead (esim_ensemble_begin_series): a member contributes, cell for cell,
        the rows area_status_series(what, where), area_series("exposures") or group_series(what) would return for it with the
        same first_step, n_rows and stride.  where: "home", "current" or "group"; what: "susceptible", "exposed", "infected",
        "recovered", "vaccinated", or "incidence" / "exposures" (two names of the event rows: exposures of the `stride` steps
        from the row's on -- by "home" and "group" in buildings and on public transport, by "current" in buildings).
        n_rows=None: up to the last step of the run (params.max_steps).  The rows stay on the device; ensemble_fold adds
        hit += (x >= min_cases), sum += x, sumsq += x * x per cell there."""
        place = place_code(where, "current home group")
        code = dict(STATUS, incidence=_lib.ENSEMBLE_SERIES_EVENTS, exposures=_lib.ENSEMBLE_SERIES_EVENTS).get(what, what)
        n_rows = self._begin_rows(first_step, n_rows, stride, 1)
        _lib.check(self.lib.esim_ensemble_begin_series(self._ctx, place, int(code), int(first_step), n_rows, int(stride), int(min_cases)), self._ctx)
        self._begun(n_rows, place)

    def ensemble_read_series(self, first_row=0, n_rows=None):
        """{"members": int, "hit": uint32 [n, n_cols], "sum": uint64 [n, n_cols], "sumsq": uint64 [n, n_cols]}: rows
        [first_row, first_row + n) of the accumulators begun by ensemble_begin_series; n_rows=None: all from first_row on."""
        return self._read_rows(self.lib.esim_ensemble_read_series, self.SERIES_KEYS, first_row, n_rows)

    def ensemble_begin_settings(self, where="home", settings=None, first_step=1, n_rows=None, stride=1, min_cases=1):
        """Accumulators over the exposures by setting (esim_ensemble_begin_settings): a member contributes, cell for cell, the
        rows setting_series(where, settings, first_step, n_rows, stride) would return for it.  where: "setting" (four columns),
        "home" or "group"; settings as setting_series takes them.  n_rows=None: up to the last step of the run
        (params.max_steps).  ensemble_fold adds hit += (x >= min_cases), sum += x, sumsq += x * x per cell on the device;
        ensemble_read_series reads them."""
        place = place_code(where, "setting home group current")
        n_rows = self._begin_rows(first_step, n_rows, stride, 1)
        _lib.check(self.lib.esim_ensemble_begin_settings(self._ctx, place, self._setting_mask(settings), int(first_step), n_rows, int(stride), int(min_cases)), self._ctx)
        self._begun(n_rows, place)

    def ensemble_begin_reproduction(self, where="home", first_step=0, n_rows=None, stride=24, min_cohort=1, r=(1, 1)):
        """Accumulators over the cohort rows (esim_ensemble_begin_reproduction): a member contributes the (cases, offspring) rows
        reproduction_series(where, first_step, n_rows, stride) would return for it.  where: "all" (one column), "home" or
        "group".  Per cell ensemble_fold counts the members with a cohort of at least min_cohort cases (defined), those of them
        with offspring / cases >= r[0] / r[1] (hit), and sums cases, offspring, their squares and their product, in integers on
        the device.  n_rows=None: up to the last step of the run (params.max_steps); ensemble_read_reproduction reads them."""
        place = place_code(where, "all home group current")
        n_rows = self._begin_rows(first_step, n_rows, stride, 0)
        _lib.check(self.lib.esim_ensemble_begin_reproduction(self._ctx, place, int(first_step), n_rows, int(stride), int(min_cohort), int(r[0]), int(r[1])), self._ctx)
        self._begun(n_rows, place)

    REPRODUCTION_KEYS = ("defined", "hit", "sum_cases", "sum_offspring", "sumsq_cases", "sumsq_offspring", "sum_cross")

    def ensemble_read_reproduction(self, first_row=0, n_rows=None):
        """{"members": int, "defined", "hit": uint32 [n, n_cols], "sum_cases", "sum_offspring", "sumsq_cases", "sumsq_offspring",
        "sum_cross": uint64 [n, n_cols]}: rows [first_row, first_row + n) of the accumulators begun by
        ensemble_begin_reproduction; n_rows=None: all from first_row on."""
        return self._read_rows(self.lib.esim_ensemble_read_reproduction, self.REPRODUCTION_KEYS, first_row, n_rows)

    def ensemble_begin_paired(self, where="all", first_step=0, n_rows=None, stride=24, cumulative=False, min_baseline=1, min_averted=1):
        """Accumulators over the paired rows (esim_ensemble_begin_paired): a member contributes the (baseline, current) rows
        compare_series(where, first_step, n_rows, stride, cumulative) would return for it.  Per cell ensemble_fold counts the
        members with at least min_baseline cases in the baseline (defined), those of them with baseline - current >=
        min_averted (hit), and sums both counts, their squares and their product, in integers on the device.  n_rows=None: up
        to the last step of the run (params.max_steps); ensemble_read_paired reads them."""
        place = self._compare_place("ensemble_begin_paired", where)
        first, n_rows, stride = self._compare_rows("ensemble_begin_paired", first_step, n_rows, stride, self._last(None, run=False))
        if int(min_averted) < 1 or int(min_baseline) < 0:
            raise ValueError("ensemble_begin_paired: min_averted must be >= 1 and min_baseline >= 0")
        _lib.check(self.lib.esim_ensemble_begin_paired(self._ctx, place, first, n_rows, stride, int(bool(cumulative)), int(min_baseline), int(min_averted)), self._ctx)
        self._begun(n_rows, place)

    PAIRED_KEYS = ("defined", "hit", "sum_baseline", "sum_current", "sumsq_baseline", "sumsq_current", "sum_cross")

    def ensemble_read_paired(self, first_row=0, n_rows=None):
        """{"members": int, "defined", "hit": uint32 [n, n_cols], "sum_baseline", "sum_current", "sumsq_baseline",
        "sumsq_current", "sum_cross": uint64 [n, n_cols]}: rows [first_row, first_row + n) of the accumulators begun by
        ensemble_begin_paired; n_rows=None: all from first_row on."""
        return self._read_rows(self.lib.esim_ensemble_read_paired, self.PAIRED_KEYS, first_row, n_rows, cols=1)

    # -- over the curve summaries: of a status (esim_ensemble_begin_peaks) and of the bed occupancy (esim_ensemble_begin_burden_peaks) -------
    PEAKS_KEYS = ("defined", "hit", "sum_peak", "sumsq_peak", "sum_step", "sumsq_step", "sum_duration", "sumsq_duration")

    def ensemble_begin_peaks(self, where="home", status="infected", first_step=1, last_step=None, threshold=1, min_peak=1):
        """Accumulators over the curve summaries (esim_ensemble_begin_peaks): ensemble_fold computes the member's
        curve_summary(where, status, first_step, last_step, threshold) on the device and adds per column defined += (peak >= 1),
        hit += (peak >= min_peak), the sums of the peak, of steps_at_least and of their squares over all members, and those of
        peak_step over the defined ones.  last_step=None: the last step of the run (params.max_steps).  ensemble_read_peaks
        reads them."""
        place, mask = self._curve_args("ensemble_begin_peaks", where, status)
        _lib.check(self.lib.esim_ensemble_begin_peaks(self._ctx, place, mask, int(first_step), self._last(last_step, run=False), int(threshold), int(min_peak)), self._ctx)
        self._begun(1, place)

    def ensemble_begin_burden_peaks(self, where="all", first_step=1, last_step=None, threshold=1, min_peak=1):
        """The peaks kind of the accumulators over the bed occupancy (esim_ensemble_begin_burden_peaks): ensemble_fold computes
        the member's burden_summary(where, first_step, last_step, threshold) on the device and folds it as ensemble_begin_peaks
        folds a status curve; ensemble_read_peaks reads them.  last_step=None: the last step of the run (params.max_steps)."""
        place = place_code(where, "all home group current")
        _lib.check(self.lib.esim_ensemble_begin_burden_peaks(self._ctx, place, int(first_step), self._last(last_step, run=False), int(threshold), int(min_peak)), self._ctx)
        self._begun(1, place)

    # -- over rows made from a member's list of admitted cases (esim_ensemble_begin_burden_series, esim_ensemble_begin_burden_paired) -------
    def ensemble_begin_burden_series(self, where="all", what="occupancy", first_step=1, n_rows=None, stride=24, min_count=1):
        """Accumulators over the rows of the hospital burden (esim_ensemble_begin_burden_series): a member contributes, cell for
        cell, the rows burden_series(what, where, first_step, n_rows, stride) would return for it; ensemble_fold adds
        hit += (x >= min_count) -- beds against a capacity --, sum += x, sumsq += x * x per cell on the device.  n_rows=None: up
        to the last step of the run (params.max_steps).  ensemble_read_series reads them."""
        place = self._compare_place("ensemble_begin_burden_series", where)
        n_rows = self._begin_rows(first_step, n_rows, stride, 1)
        _lib.check(self.lib.esim_ensemble_begin_burden_series(self._ctx, place, self._burden_what(what), int(first_step), n_rows, int(stride), int(min_count)), self._ctx)
        self._begun(n_rows, place)

    def ensemble_begin_burden_paired(self, where="all", what="occupancy", first_step=1, n_rows=None, stride=24, cumulative=False, min_baseline=1, min_averted=1):
        """The paired kind over the hospital burden (esim_ensemble_begin_burden_paired): a member contributes the (baseline,
        current) rows burden_compare_series(what, where, first_step, n_rows, stride, cumulative) would return for it, folded as
        ensemble_begin_paired folds the cases.  ensemble_read_paired reads them; the members kept are baseline - current."""
        place = self._compare_place("ensemble_begin_burden_paired", where)
        n_rows = self._begin_rows(first_step, n_rows, stride, 1)
        if int(min_averted) < 1 or int(min_baseline) < 0:
            raise ValueError("ensemble_begin_burden_paired: min_averted must be >= 1 and min_baseline >= 0")
        _lib.check(self.lib.esim_ensemble_begin_burden_paired(self._ctx, place, self._burden_what(what), int(first_step), n_rows, int(stride), int(bool(cumulative)),
                                                              int(min_baseline), int(min_averted)), self._ctx)
        self._begun(n_rows, place)

    def ensemble_read_peaks(self):
        """{"members": int, "defined", "hit": uint32 [n_cols], "sum_peak", "sumsq_peak", "sum_step", "sumsq_step", "sum_duration",
        "sumsq_duration": uint64 [n_cols]}: the accumulators begun by ensemble_begin_peaks."""
        return self._read_accumulators(self.lib.esim_ensemble_read_peaks, self.PEAKS_KEYS, getattr(self, "_ens_n", self.population.n_areas))

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

    def _members_planes(self, count, first_row, n_rows):
        """(first_row, n, zeroed uint32 [count, n, cols]) for the rows [first_row, first_row + n) of the members kept."""
        total = max(1, int(getattr(self, "_ens_rows", 1)))
        n = max(0, total - int(first_row) if n_rows is None else int(n_rows))
        return int(first_row), n, np.zeros((count, n, int(getattr(self, "_ens_n", self.population.n_areas))), np.uint32)

    def ensemble_members(self, first_member=0, n_members=None, first_row=0, n_rows=None):
        """[members, rows, cols]: the values kept, members in the order of their folds; int32 for the paired kind, uint32
        otherwise (esim_ensemble_read_members).  n_members=None: all from first_member on; n_rows=None: all from first_row on."""
        info = self.ensemble_members_info()
        m = max(0, info["kept"] - int(first_member) if n_members is None else int(n_members))
        first_row, n, out = self._members_planes(m, first_row, n_rows)
        _lib.check(self.lib.esim_ensemble_read_members(self._ctx, int(first_member), m, first_row, n, ptr(out)), self._ctx)
        return out.view(np.int32) if info["signed"] else out

    def _members_ranks(self, ranks, first_row, n_rows, signed):
        ranks = np.ascontiguousarray(ranks, np.uint32).reshape(-1)
        first_row, n, out = self._members_planes(ranks.size, first_row, n_rows)
        _lib.check(self.lib.esim_ensemble_quantiles(self._ctx, first_row, n, ptr(ranks), ranks.size, ptr(out)), self._ctx)
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
        thr = np.ascontiguousarray(thresholds, np.int64).reshape(-1)
        first_row, n, out = self._members_planes(thr.size, first_row, n_rows)
        for i in range(0, max(1, thr.size), _lib.RANKS_MAX):                       # (out[i:i + k] is contiguous: the library writes into it)
            k = min(_lib.RANKS_MAX, thr.size - i)
            _lib.check(self.lib.esim_ensemble_exceedance(self._ctx, first_row, n, ptr(thr[i:]), k, ptr(out[i:])), self._ctx)
        return out

    # -- curve-based statistics: the members kept ranked as whole curves (esim_ensemble_depth, esim_ensemble_band) -------
    def ensemble_depth(self, first_row=0, n_rows=None):
        """{"depth": uint32 [kept, n_cols], "total": uint64 [kept], "pairs": int, "rows": int, "mbd": float64 [kept, n_cols]}: the
        modified band depth of every member kept, per column, over the rows [first_row, first_row + n) of the store, counted on
        the device in integers (esim_ensemble_depth).  depth is the number of pairs of members whose band holds the member's key,
        summed over the rows; pairs = C(kept, 2); mbd = depth / (rows * pairs), NaN where that is 0 / 0.  total: depth summed
        over the columns.  n_rows=None: all from first_row on."""
        kept = self.ensemble_members_info()["kept"]
        first_row, n, _ = self._members_planes(0, first_row, n_rows)
        cols = int(getattr(self, "_ens_n", self.population.n_areas))
        depth, total = np.zeros((kept, cols), np.uint32), np.zeros(kept, np.uint64)
        _lib.check(self.lib.esim_ensemble_depth(self._ctx, first_row, n, ptr(depth), ptr(total)), self._ctx)
        pairs = kept * (kept - 1) // 2
        with np.errstate(invalid="ignore", divide="ignore"):
            mbd = depth.astype(np.float64) / np.float64(n * pairs)
        return {"depth": depth, "total": total, "pairs": pairs, "rows": n, "mbd": mbd}

    def ensemble_band(self, coverage=0.5, pooled=False, first_row=0, n_rows=None, need=None):
        """{"lo", "hi", "median": [n, n_cols], "deepest", "n_in": uint32 [n_cols], "need": int}: the envelope of the most central
        members kept and the deepest member's curve, over the rows [first_row, first_row + n) (esim_ensemble_band).  The
        need = max(1, ceil(coverage * kept)) deepest members are in, and every member that ties with the last of them; an
        explicit need overrides the coverage, which is taken as the decimal it was written as (nearest_rank).  lo and hi are
        the smallest and largest value over the members that are in, median the curve of member deepest[col]: a real run.
        pooled=False ranks the members per column; pooled=True by their depth summed over the columns, one set of members and
        one deepest member for the whole map.  int32 for the paired kind, uint32 otherwise (_lib.NEVER means what it means in
        the store).  n_rows=None: all from first_row on."""
        info = self.ensemble_members_info()
        kept = info["kept"]
        if need is None:
            if not 0.0 <= float(coverage) <= 1.0:
                raise ValueError("Simulator.ensemble_band: coverage must lie in [0, 1], got %r" % (coverage,))
            need = max(1, nearest_rank(coverage, kept) + 1)
        first_row, n, planes = self._members_planes(3, first_row, n_rows)
        cols = zeros(("deepest", "n_in"), planes.shape[2])
        _lib.check(self.lib.esim_ensemble_band(self._ctx, first_row, n, int(need), int(bool(pooled)), ptr(planes[0]), ptr(planes[1]), ptr(planes[2]),
                                               ptr(cols["deepest"]), ptr(cols["n_in"])), self._ctx)
        if info["signed"]:
            planes = planes.view(np.int32)
        return dict(cols, lo=planes[0], hi=planes[1], median=planes[2], need=int(need))

    # -- ensemble distances: the members kept compared pair by pair (esim_ensemble_distances) -------
    DIST_METRIC = {"l1": _lib.DIST_L1, "differ": _lib.DIST_DIFFER}

    def ensemble_distances(self, metric="l1", first_row=0, n_rows=None, never_as=None):
        """{"distances": uint64 [kept, kept], "live_cells": int, "cells": int, "metric": str}: the distance of every pair of
        members kept, summed on the device over the rows [first_row, first_row + n) of the store and all columns
        (esim_ensemble_distances).  metric="l1": the sum of |x_i - x_j| per cell; "differ": the cells in which the two differ.
        Exact integers, symmetric, the diagonal 0.  never_as: what _lib.NEVER counts as in the stores that hold it (arrival,
        peak_step) -- the horizon, say; None leaves it as it is.  cells: those of the window; live_cells: those of them the
        accumulators do not settle, which the kernel compared.  n_rows=None: all from first_row on."""
        code = self.DIST_METRIC.get(metric, metric)
        if not isinstance(code, int) or isinstance(code, bool):
            raise ValueError("Simulator.ensemble_distances: metric must be 'l1' or 'differ', got %r" % (metric,))
        kept = self.ensemble_members_info()["kept"]
        first_row, n, _ = self._members_planes(0, first_row, n_rows)
        out, live = np.zeros((kept, kept), np.uint64), C.c_uint64(0)
        _lib.check(self.lib.esim_ensemble_distances(self._ctx, first_row, n, code, _lib.NEVER if never_as is None else int(never_as), ptr(out), C.byref(live)), self._ctx)
        names = {v: k for k, v in self.DIST_METRIC.items()}
        return {"distances": out, "live_cells": int(live.value), "cells": n * int(getattr(self, "_ens_n", self.population.n_areas)), "metric": names.get(code, metric)}

    # -- ensembles on several contexts: the accumulators of one added into another, or through bytes (esim_ensemble_merge) -------
    def ensemble_merge(self, other):
        """Adds the accumulators of `other` -- a Simulator with the same begin in force on the same population -- into this
        one's and appends its kept members behind this one's (esim_ensemble_merge); `other` stays as it was.  Exact: the result
        is the ensemble folded in sequence.  The call does not wait for this simulator's stream: leave `other` alone until this
        one has been read or synchronized."""
        _lib.check(self.lib.esim_ensemble_merge(self._ctx, other._ctx), self._ctx)

    def ensemble_save(self):
        """The ensemble in force as bytes: its descriptor, its accumulators and its kept members (esim_ensemble_save)."""
        size = C.c_size_t(0)
        _lib.check(self.lib.esim_ensemble_save_size(self._ctx, C.byref(size)), self._ctx)
        buf = np.zeros(size.value, np.uint8)
        _lib.check(self.lib.esim_ensemble_save(self._ctx, C.cast(ptr(buf), C.c_void_p), size.value), self._ctx)
        return buf.tobytes()

    def ensemble_load(self, blob):
        """A merge from the bytes of ensemble_save: added into the begin in force, which must describe the same ensemble; behind
        a fresh begin (and ensemble_keep_members) it restores (esim_ensemble_load)."""
        buf = np.frombuffer(bytes(blob), np.uint8)
        _lib.check(self.lib.esim_ensemble_load(self._ctx, C.cast(ptr(buf), C.c_void_p) if buf.size else None, buf.size), self._ctx)

    def ensemble_distances_info(self):
        """{"tiles", "tiles_32bit", "tiles_partial"} of the last ensemble_distances (esim_ensemble_distances_info)."""
        t = [C.c_uint64(0) for _ in range(3)]
        _lib.check(self.lib.esim_ensemble_distances_info(self._ctx, *(C.byref(x) for x in t)), self._ctx)
        return dict(zip(("tiles", "tiles_32bit", "tiles_partial"), (int(x.value) for x in t)))

    # -- policy grids: the members kept read as replicates of arms run on common random numbers (esim_ensemble_arms) -------
    def ensemble_arms(self, n_arms, maximize=False, never_as=None, first_row=0, n_rows=None):
        """{"best", "sole": uint32 [n_arms, n, n_cols], "regret", "sum": uint64 [n_arms, n, n_cols], "totals": uint64 [replicates,
        n_arms], "live_cells": int, "replicates": int, "maximize": bool}: the members kept read as replicates of n_arms arms, slot = replicate *
        n_arms + arm -- the arms of a replicate folded one after the other under the same seed and index cases --, compared on the
        device over the rows [first_row, first_row + n) of the store and all columns (esim_ensemble_arms; the kinds without rows
        have one row, as in ensemble_quantiles).  Per cell and arm: best, the replicates in which the arm holds the smallest value
        of its replicate (the largest with maximize=True; ties all count); sole, those in which no other arm does; regret, the sum
        over the replicates of the distance to the best arm of the same replicate; sum, the arm's sum.  totals: every run's sum
        over the whole window (modulo 2^64).  never_as: what _lib.NEVER counts as in the stores that hold it (arrival, peak_step)
        -- the horizon, say; None leaves it as it is.  live_cells: the cells the accumulators do not settle, which the kernel read.
        The library refuses 0 or more than 16 arms, a number of members kept that is no multiple of n_arms, and the signed store
        of the paired kinds.  n_rows=None: all from first_row on."""
        a = int(n_arms)
        kept = self.ensemble_members_info()["kept"]
        first_row, n, _ = self._members_planes(0, first_row, n_rows)
        cols = int(getattr(self, "_ens_n", self.population.n_areas))
        width = min(max(a, 0), _lib.ARMS_MAX)                       # (of the buffers, whatever the library then says to n_arms)
        out = zeros(("best", "sole", "regret", "sum"), (width, n, cols), u64=("regret", "sum"))
        reps = kept // a if 0 < a <= _lib.ARMS_MAX and kept % a == 0 else 0
        totals, live = np.zeros((reps, width), np.uint64), C.c_uint64(0)
        _lib.check(self.lib.esim_ensemble_arms(self._ctx, a, int(bool(maximize)), _lib.NEVER if never_as is None else int(never_as), first_row, n,
                                               *(ptr(out[k]) for k in ("best", "sole", "regret", "sum")), ptr(totals) if reps else None, C.byref(live)), self._ctx)
        return dict(out, totals=totals, live_cells=int(live.value), replicates=reps, maximize=bool(maximize))
