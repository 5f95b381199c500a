"""Ensembles of one uploaded population: many Philox seeds of one world, or the same world under several parameter sets,
or under other index cases (where the outbreak starts), one member after another on ONE context (esim_restart,
esim_restart_seeded), summarised per step on the host and per Output Area -- or per citizen group -- on the device
(esim_ensemble_*); or, as a forecast, as branches from one snapshot of a shared history (esim_snapshot, esim_rollback).  The
population is validated, hashed and uploaded once per context: Ensemble(..., devices=(0, 1)) has a context per entry, each with
a copy of the population, hands every context a contiguous block of the members (split_members) on a thread of its own and
merges the contexts into the first (esim_ensemble_merge) -- the results are those of one context, bit for bit."""
import copy
import json
import os
import threading

import numpy as np

from . import _lib
from ._marshal import rate as _rate
from .simulator import RECORD_DTYPE, Simulator, check_probs

QUANTILES = (0.05, 0.25, 0.5, 0.75, 0.95)           # the rows of ensemble_stats.json
STAT_FIELDS = ("susceptible", "exposed", "infected", "recovered", "vaccinated", "exposures_building", "exposures_bus", "vaccinated_now")
_EVENT_FIELDS = ("exposures_building", "exposures_bus", "vaccinated_now", "n_riders")   # what happens IN a step: zero in a step that did not run


def _stack(rows, shape, dtype):
    """The members' tables of `shape` as one array [members, *shape] of `dtype`; without members [0, *shape]."""
    return np.stack(rows).astype(dtype) if rows else np.zeros((0,) + tuple(shape), dtype)


def pad_records(rec, n_steps):
    """`rec` (the records of a member that stopped early, time steps 1..len(rec)) as n_steps rows: the rows behind the last
    record carry its census and flags forward with time_step counting on, zero exposures, zero vaccinated_now and
    disease_exists = 0 -- summaries over members stay defined for every step.  A member without any record pads with zeros."""
    out = np.zeros(n_steps, RECORD_DTYPE)
    k = min(len(rec), n_steps)
    out[:k] = rec[:k]
    if k < n_steps:
        if k:
            out[k:] = rec[k - 1]
            for f in _EVENT_FIELDS:
                out[f][k:] = 0
        out["disease_exists"][k:] = 0
        out["time_step"][k:] = np.arange(k + 1, n_steps + 1, dtype=np.uint32)
    return out


def area_summary(members, hit, total, sumsq):
    """members, hit, mean = sum / members, var = population variance from sum and sumsq."""
    m = int(members)
    total, sumsq = np.asarray(total, np.float64), np.asarray(sumsq, np.float64)
    mean = total / m if m else np.zeros_like(total)
    var = np.maximum(sumsq / m - mean * mean, 0.0) if m else np.zeros_like(total)
    return {"members": m, "hit": np.asarray(hit, np.uint32), "mean": mean, "var": var}


def arrival_summary(members, hit, total, sumsq):
    """members, hit (members whose epidemic reached the entry by the horizon), and over those members the mean = sum / hit and
    the population variance of the arrival step; both NaN where hit == 0."""
    hit = np.asarray(hit, np.uint32)
    total, sumsq, h = np.asarray(total, np.float64), np.asarray(sumsq, np.float64), hit.astype(np.float64)
    mean = _rate(total, h)
    with np.errstate(invalid="ignore", divide="ignore"):
        var = np.where(hit > 0, np.maximum(sumsq / h - mean * mean, 0.0), np.nan)
    return {"members": int(members), "hit": hit, "mean": mean, "var": var}


def series_summary(members, hit, total, sumsq, first_step=1, stride=1):
    """area_summary over [n_rows, n_cols] accumulators, and steps: the step each row describes."""
    out = area_summary(members, hit, total, sumsq)
    out["steps"] = int(first_step) + int(stride) * np.arange(np.asarray(hit).shape[0], dtype=np.int64)
    return out


def _ratio_residuals(sx, sy, sxx, syy, sxy):
    """sum over members of (y_i * Sx - Sy * x_i)^2 = Sx^2 * sum y^2 - 2 Sx Sy * sum xy + Sy^2 * sum x^2 per cell, exactly, from the
    integer sums (Sx = sum x, Sy = sum y) and as float64: in int64 where every term stays below 2^60, in Python integers
    otherwise -- in floating point the three terms cancel to nothing where offspring is nearly proportional to cases."""
    arrays = [np.asarray(a, np.uint64) for a in (sx, sy, sxx, syy, sxy)]
    top = [int(a.max()) if a.size else 0 for a in arrays]
    if max(top[0], top[1]) ** 2 * max(top[2:]) < 1 << 60:
        sx, sy, sxx, syy, sxy = (a.astype(np.int64) for a in arrays)
    else:
        sx, sy, sxx, syy, sxy = (a.astype(object) for a in arrays)
    return (sx * sx * syy - 2 * sx * sy * sxy + sy * sy * sxx).astype(np.float64)


def reproduction_summary(acc, first_step=0, stride=24):
    """From Simulator.ensemble_read_reproduction(): members, defined, hit; cases_mean and offspring_mean over the members; r,
    the pooled case reproduction number sum_offspring / sum_cases of the cell, NaN where no member had a case; p_r = hit /
    defined, the share of the members with a cohort in the cell whose offspring / cases reached the threshold, NaN where none
    had one; r_se, the standard error of r by the delta method over members -- Var(r) = (s_oo - 2 r s_co + r^2 s_cc) / (members *
    cases_mean^2) with the sample covariances (ddof = 1) of cases and offspring over the members, which is sum_i (o_i - r c_i)^2 /
    (members - 1) in the numerator --, NaN for fewer than two members or no cases; and steps, the first step of every row's
    cohort."""
    m = int(acc["members"])
    sx, sy = np.asarray(acc["sum_cases"], np.uint64), np.asarray(acc["sum_offspring"], np.uint64)
    defined, hit = np.asarray(acc["defined"], np.uint32), np.asarray(acc["hit"], np.uint32)
    fx, fy = sx.astype(np.float64), sy.astype(np.float64)
    r, p_r = _rate(sy, sx), _rate(hit, defined)
    with np.errstate(invalid="ignore", divide="ignore"):
        if m >= 2:
            resid = _ratio_residuals(sx, sy, acc["sumsq_cases"], acc["sumsq_offspring"], acc["sum_cross"])
            r_se = np.where(sx > 0, np.sqrt(resid * (m / (m - 1.0))) / (fx * fx), np.nan)
        else:
            r_se = np.full(sx.shape, np.nan)
    return {"members": m, "defined": defined, "hit": hit, "cases_mean": fx / m if m else np.zeros_like(fx), "offspring_mean": fy / m if m else np.zeros_like(fy),
            "r": r, "p_r": p_r, "r_se": r_se, "steps": int(first_step) + int(stride) * np.arange(sx.shape[0], dtype=np.int64)}


def _spread(m, s, ss):
    """m * sum x^2 - (sum x)^2 = m * sum (x - mean)^2 per cell, exactly, from integer sums and as float64: in int64 where every
    term stays below 2^62, in Python integers otherwise."""
    s, ss = np.asarray(s), np.asarray(ss)
    top_s, top_ss = (int(np.abs(a).max()) if a.size else 0 for a in (s, ss))
    kind = np.int64 if max(top_s * top_s, m * top_ss) < 1 << 62 else object
    s, ss = s.astype(kind), ss.astype(kind)
    return (m * ss - s * s).astype(np.float64)


def paired_summary(acc, first_step=0, stride=24):
    """From Simulator.ensemble_read_paired(): members, defined, hit; mean_baseline, mean_policy and mean_averted = mean_baseline -
    mean_policy over the members; p_averted = hit / defined, the share of the members with enough baseline cases in the cell
    that averted at least min_averted of them, NaN where none had; se_paired, the standard error of mean_averted from the
    variance of the members' DIFFERENCES -- sum d^2 = sumsq_baseline - 2 sum_cross + sumsq_current, sample variance (ddof = 1) --;
    se_unpaired = sqrt((var_b + var_c) / members), what two separate ensembles of the same size would quote; both NaN for
    fewer than two members; and steps, the first step of every row."""
    m = int(acc["members"])
    sb, sc = np.asarray(acc["sum_baseline"], np.uint64), np.asarray(acc["sum_current"], np.uint64)
    sbb, scc, sbc = (np.asarray(acc[k], np.uint64) for k in ("sumsq_baseline", "sumsq_current", "sum_cross"))
    defined, hit = np.asarray(acc["defined"], np.uint32), np.asarray(acc["hit"], np.uint32)
    fb, fc = sb.astype(np.float64), sc.astype(np.float64)
    diff = sb.astype(np.int64) - sc.astype(np.int64)
    p_averted = _rate(hit, defined)
    if m >= 2:
        wide = max((int(a.max()) if a.size else 0) for a in (sbb, scc, sbc)) >= 1 << 60
        sq = (lambda a: a.astype(object)) if wide else (lambda a: a.astype(np.int64))
        sdd = sq(sbb) - 2 * sq(sbc) + sq(scc)                     # sum over members of (b - c)^2, exact
        scale = float(m) * m * (m - 1.0)                          # _spread / (m (m - 1)) is the sample variance; / m again its mean's
        se_paired = np.sqrt(np.maximum(_spread(m, diff, sdd), 0.0) / scale)
        se_unpaired = np.sqrt((np.maximum(_spread(m, sb, sbb), 0.0) + np.maximum(_spread(m, sc, scc), 0.0)) / scale)
    else:
        se_paired, se_unpaired = np.full(sb.shape, np.nan), np.full(sb.shape, np.nan)
    zeros = np.zeros_like(fb)
    return {"members": m, "defined": defined, "hit": hit, "mean_baseline": fb / m if m else zeros, "mean_policy": fc / m if m else zeros,
            "mean_averted": diff.astype(np.float64) / m if m else zeros, "p_averted": p_averted, "se_paired": se_paired, "se_unpaired": se_unpaired,
            "steps": int(first_step) + int(stride) * np.arange(sb.shape[0], dtype=np.int64)}


def peaks_summary(acc):
    """From Simulator.ensemble_read_peaks(): members, defined (members with a peak of at least 1), hit, p_peak = hit / members
    (NaN without members); peak_mean and peak_var, duration_mean and duration_var over all members (a member without a case
    counts as 0); peak_step_mean and peak_step_var over the defined members, NaN where there is none.  Population variances,
    from the integer sums."""
    m = int(acc["members"])
    defined, hit = np.asarray(acc["defined"], np.uint32), np.asarray(acc["hit"], np.uint32)
    out = {"members": m, "defined": defined, "hit": hit}
    d = defined.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        out["p_peak"] = hit.astype(np.float64) / m if m else np.full(hit.shape, np.nan)
        for name, key, n in (("peak", "peak", float(m)), ("duration", "duration", float(m)), ("peak_step", "step", d)):
            s, ss = np.asarray(acc["sum_" + key], np.float64), np.asarray(acc["sumsq_" + key], np.float64)
            mean = np.where(n > 0, s / n, np.nan)
            out[name + "_mean"], out[name + "_var"] = mean, np.where(n > 0, np.maximum(ss / n - mean * mean, 0.0), np.nan)
    return out


PEAKS_ARRAYS = ("defined", "hit", "p_peak", "peak_mean", "peak_var", "peak_step_mean", "peak_step_var", "duration_mean", "duration_var")
CLUSTER_ARRAYS = ("distances", "cluster_medoid", "cluster_label", "cluster_size", "cluster_silhouette", "cluster_curves", "cluster_cost", "cluster_metric")   # of ensemble_area_clusters.npz
BAND_ARRAYS = ("band_lo", "band_hi", "band_median", "band_deepest", "band_n_in", "band_need", "band_coverage", "band_pooled", "depth")     # of ensemble_area_band.npz


def _json_number(x):
    x = float(x)
    return None if x != x else x          # NaN (an arrival mean nobody contributed to) is written as null


class EnsembleResult:
    def __init__(self, records, n_done, members, area=None, area_codes=None, settings=None, reproduction=None, area_kind=None):
        self.records = records            # structured [members, n_steps]
        self.settings = settings          # uint32 [members, n_rows, 4]: every member's setting_series(where="setting"), or None
        self.reproduction = reproduction  # uint32 [members, n_rows, 2]: every member's reproduction_series("all"), (cases, offspring), or None
        self.n_done = np.asarray(n_done, np.uint32)
        self.members = list(members)      # the overrides of every member
        self.area = area                  # area_summary(...) or None
        self.area_codes = area_codes
        self.area_kind = area_kind        # the kind of run(area=dict(kind=...)) the summary came from, or None

    def quantiles(self, field, qs):
        """[len(qs), n_steps]: the quantiles of `field` over the members, per step."""
        if self.records.shape[0] == 0:
            return np.zeros((len(qs), self.records.shape[1]))
        return np.quantile(self.records[field].astype(np.float64), list(qs), axis=0)

    def mean(self, field):
        if self.records.shape[0] == 0:
            return np.zeros(self.records.shape[1])
        return self.records[field].astype(np.float64).mean(axis=0)

    def dump(self, directory):
        """ensemble_stats.json: per field the mean and the 5/25/50/75/95 % rows over the members; ensemble_areas.json: hit, mean
        and var per Output Area, keyed by its code where the Ensemble was given area_codes, else by its index (an arrival
        summary's mean and var are null where hit is 0).  A series summary goes to ensemble_area_series.npz instead -- steps,
        hit, mean, var, and codes where area codes were given -- and ensemble_areas.json is then null, as without a summary; the
        summary of area kind "settings" goes to ensemble_area_settings.npz the same way, that of kind "reproduction" to
        ensemble_area_reproduction.npz: steps, defined, hit, cases_mean, offspring_mean, r, p_r, r_se, members, and codes; that of
        kind "peaks" to ensemble_area_peaks.npz: the arrays of peaks_summary, members, and codes (kind "burden_peaks": the same of
        the bed occupancy, to ensemble_area_burden.npz); that of kind "burden_series" to ensemble_area_burden_series.npz, as a
        series summary.  The members' exposures by setting, where they
        were asked for, go to ensemble_settings.npz: settings [members, n_rows, 4] and the four names; their cohort rows to
        ensemble_reproduction.npz: reproduction [members, n_rows, 2] and the two names.  The quantile maps, where the area dict
        asked for them, go to ensemble_area_quantiles.npz: probs, quantiles, thresholds, exceed, steps for a summary over rows, and
        codes; every other file is what it is without them.  The central band, where the area dict asked for it (band=), goes to
        ensemble_area_band.npz the same way: band_lo, band_hi, band_median, band_deepest, band_n_in, band_need, band_coverage,
        band_pooled, depth, steps and codes.  The clusters (clusters=) go to ensemble_area_clusters.npz: distances, cluster_medoid,
        cluster_label, cluster_size, cluster_silhouette, cluster_curves, cluster_cost, cluster_metric, steps and codes."""
        os.makedirs(directory, exist_ok=True)
        stats = {"members": self.members, "n_done": self.n_done.tolist(), "fields": {}}
        for f in STAT_FIELDS:
            q = self.quantiles(f, QUANTILES)
            stats["fields"][f] = dict({"mean": self.mean(f).tolist()}, **{"q%02d" % round(100 * p): q[i].tolist() for i, p in enumerate(QUANTILES)})
        with open(os.path.join(directory, "ensemble_stats.json"), "w") as fh:
            json.dump(stats, fh)
        doc = None
        if self.area is not None and self.area_kind in ("peaks", "burden_peaks"):      # arrays by column: nine of them, too many for the JSON's three
            arrays = {k: self.area[k] for k in PEAKS_ARRAYS}
            arrays["members"] = np.asarray(self.area["members"], np.uint32)
            if self.area_codes is not None:
                arrays["codes"] = np.asarray(self.area_codes)
            np.savez(os.path.join(directory, "ensemble_area_burden.npz" if self.area_kind == "burden_peaks" else "ensemble_area_peaks.npz"), **arrays)
        elif self.area is not None and "steps" in self.area:     # a summary over rows: arrays by (row, column), too many for JSON
            a = self.area
            ratio = "r" in a
            arrays = {k: a[k] for k in (("steps", "defined", "hit", "cases_mean", "offspring_mean", "r", "p_r", "r_se") if ratio else ("steps", "hit", "mean", "var"))}
            if ratio:
                arrays["members"] = np.asarray(a["members"], np.uint32)
            if self.area_codes is not None:
                arrays["codes"] = np.asarray(self.area_codes)
            name = ("ensemble_area_reproduction.npz" if ratio else "ensemble_area_settings.npz" if self.area_kind == "settings" else
                    "ensemble_area_burden_series.npz" if self.area_kind == "burden_series" else "ensemble_area_series.npz")
            np.savez(os.path.join(directory, name), **arrays)
        elif self.area is not None:
            a = self.area
            key = (lambda i: self.area_codes[i]) if self.area_codes is not None else (lambda i: str(i))
            doc = {"members": a["members"],
                   "areas": {key(i): {"hit": int(a["hit"][i]), "mean": _json_number(a["mean"][i]), "var": _json_number(a["var"][i])} for i in range(len(a["hit"]))}}
        with open(os.path.join(directory, "ensemble_areas.json"), "w") as fh:
            json.dump(doc, fh)
        if self.area is not None and "probs" in self.area:           # the quantile maps: a file of their own, the others are what they are without
            extra = {k: self.area[k] for k in ("probs", "quantiles", "thresholds", "exceed") if self.area[k] is not None}
            if "steps" in self.area:
                extra["steps"] = self.area["steps"]
            if self.area_codes is not None:
                extra["codes"] = np.asarray(self.area_codes)
            np.savez(os.path.join(directory, "ensemble_area_quantiles.npz"), **extra)
        if self.area is not None and "band_lo" in self.area:         # the central band: a file of its own too
            extra = {k: np.asarray(self.area[k]) for k in BAND_ARRAYS}
            if "steps" in self.area:
                extra["steps"] = self.area["steps"]
            if self.area_codes is not None:
                extra["codes"] = np.asarray(self.area_codes)
            np.savez(os.path.join(directory, "ensemble_area_band.npz"), **extra)
        if self.area is not None and "cluster_medoid" in self.area:  # the clusters: a file of their own too
            extra = {k: np.asarray(self.area[k]) for k in CLUSTER_ARRAYS}
            if "steps" in self.area:
                extra["steps"] = self.area["steps"]
            if self.area_codes is not None:
                extra["codes"] = np.asarray(self.area_codes)
            np.savez(os.path.join(directory, "ensemble_area_clusters.npz"), **extra)
        if self.settings is not None:
            np.savez(os.path.join(directory, "ensemble_settings.npz"), settings=self.settings, names=np.asarray(_lib.SETTING_NAMES))
        if self.reproduction is not None:
            np.savez(os.path.join(directory, "ensemble_reproduction.npz"), reproduction=self.reproduction, names=np.asarray(("cases", "offspring")))


class OutbreakResult:
    """What Ensemble.outbreaks gathers: the outbreak table of every member, one row per member and one column per index case."""

    def __init__(self, members, seeds, size, depth, last_step, ages=None):
        self.members = list(members)      # the overrides of every member
        self.seeds = list(seeds)          # per member the index cases in force, in the order of its columns (members may differ in number)
        self.size = np.asarray(size, np.int64)            # int64 [members, max_seeds]; -1 where a member has fewer seeds
        self.depth = np.asarray(depth, np.int64)
        self.last_step = np.asarray(last_step, np.int64)
        self.ages = ages                  # uint32 [members, 4, 512]: every member's transmission_ages(), or None

    @classmethod
    def gathered(cls, members, tables, ages=None):
        """From every member's Simulator.outbreaks() dict, padded with -1 to the largest number of seeds."""
        width = max([len(t["seeds"]) for t in tables], default=0)
        cols = {k: np.full((len(tables), width), -1, np.int64) for k in ("size", "depth", "last_step")}
        for i, t in enumerate(tables):
            for k in cols:
                cols[k][i, :len(t["seeds"])] = t[k]
        return cls(members, [np.asarray(t["seeds"], np.uint32) for t in tables], cols["size"], cols["depth"], cols["last_step"],
                   None if ages is None else (np.stack(ages) if ages else np.zeros((0, _lib.N_SETTINGS, _lib.AGE_BINS), np.uint32)))

    def extinct(self, min_size=1):
        """bool [members, max_seeds]: the introductions that infected fewer than min_size citizens (false in the padding)."""
        return (self.size >= 0) & (self.size < int(min_size))

    def dump(self, directory):
        """ensemble_outbreaks.npz: size, depth, last_step and seeds (padded with -1 like them), and ages where they were asked for."""
        os.makedirs(directory, exist_ok=True)
        seeds = np.full(self.size.shape, -1, np.int64)
        for i, s in enumerate(self.seeds):
            seeds[i, :len(s)] = s
        arrays = dict(size=self.size, depth=self.depth, last_step=self.last_step, seeds=seeds)
        if self.ages is not None:
            arrays["ages"] = self.ages
        np.savez(os.path.join(directory, "ensemble_outbreaks.npz"), **arrays)


def _size_and_pair_tables(sizes, pairs, bins, n_cols):
    """The four stacked tables of HouseholdResult and PlaceResult from every member's two size tables, uint32 [bins, bins], and
    two pair tables, uint64 [n_cols, n_cols]."""
    return (*(_stack([t[i] for t in sizes], (bins, bins), np.uint32) for i in (0, 1)),
            *(_stack([t[i] for t in pairs], (n_cols, n_cols), np.uint64) for i in (0, 1)))


class HouseholdResult:
    """What Ensemble.households gathers: the final-size tables and the household pair tables of every member."""

    def __init__(self, members, final_size, introductions, at_risk, secondary):
        self.members = list(members)      # the overrides of every member
        self.final_size = np.asarray(final_size, np.uint32)          # uint32 [members, 64, 64]: households of n residents with k cases
        self.introductions = np.asarray(introductions, np.uint32)    # uint32 [members, 64, 64]: ... with k introductions
        self.at_risk = np.asarray(at_risk, np.uint64)                # uint64 [members, n_cols, n_cols]: (case, housemate at risk) pairs
        self.secondary = np.asarray(secondary, np.uint64)            # uint64 [members, n_cols, n_cols]: those infected at home by the case

    @classmethod
    def gathered(cls, members, sizes, pairs, n_cols=1):
        """From every member's Simulator.household_final_sizes() and household_sar() tuples."""
        return cls(members, *_size_and_pair_tables(sizes, pairs, _lib.HH_BINS, n_cols))

    def sar(self):
        """float64 [n_cols, n_cols]: the household secondary attack rate pooled over the members -- the sum of secondary
        divided by the sum of at_risk --, NaN where nobody was at risk."""
        return _rate(self.secondary.sum(axis=0), self.at_risk.sum(axis=0))

    def dump(self, directory):
        """ensemble_households.npz: final_size, introductions, at_risk, secondary and the pooled sar."""
        os.makedirs(directory, exist_ok=True)
        np.savez(os.path.join(directory, "ensemble_households.npz"), final_size=self.final_size, introductions=self.introductions,
                 at_risk=self.at_risk, secondary=self.secondary, sar=self.sar())


class PlaceResult:
    """What Ensemble.places gathers: the size tables and the pair tables of the work places, rooms or schools of every member."""

    def __init__(self, members, final_size, introduced, at_risk, secondary):
        self.members = list(members)      # the overrides of every member
        self.final_size = np.asarray(final_size, np.uint32)          # uint32 [members, 32, 32]: places of bin(size) with bin(k) cases
        self.introduced = np.asarray(introduced, np.uint32)          # uint32 [members, 32, 32]: ... with bin(k) introductions
        self.at_risk = np.asarray(at_risk, np.uint64)                # uint64 [members, n_cols, n_cols]: (case, member at risk) pairs
        self.secondary = np.asarray(secondary, np.uint64)            # uint64 [members, n_cols, n_cols]: those infected there by the case

    @classmethod
    def gathered(cls, members, sizes, pairs, n_cols=1):
        """From every member's Simulator.place_sizes() and place_sar() tuples."""
        return cls(members, *_size_and_pair_tables(sizes, pairs, _lib.PLACE_BINS, n_cols))

    def sar(self):
        """float64 [n_cols, n_cols]: the secondary attack rate pooled over the members -- the sum of secondary divided by the
        sum of at_risk --, NaN where nobody was at risk."""
        return _rate(self.secondary.sum(axis=0), self.at_risk.sum(axis=0))

    def attack_rate_by_size(self):
        """float64 [32]: per size bin, the share of the places (pooled over the members) that had at least one case, NaN for a
        bin without a place."""
        tab = self.final_size.sum(axis=0).astype(np.float64)
        places = tab.sum(axis=1)
        return _rate(places - tab[:, 0], places)

    def dump(self, directory):
        """ensemble_places.npz: final_size, introduced, at_risk, secondary, the pooled sar and attack_rate_by_size."""
        os.makedirs(directory, exist_ok=True)
        np.savez(os.path.join(directory, "ensemble_places.npz"), final_size=self.final_size, introduced=self.introduced,
                 at_risk=self.at_risk, secondary=self.secondary, sar=self.sar(), attack_rate_by_size=self.attack_rate_by_size())


class ContactResult:
    """What Ensemble.contacts gathers: the contact-hours and the transmissions of every member by setting."""

    def __init__(self, members, hours, transmissions):
        self.members = list(members)      # the overrides of every member
        self.hours = np.asarray(hours, np.uint64)                    # uint64 [members, 4, n_cols, n_cols]: contact-hours at risk
        self.transmissions = np.asarray(transmissions, np.uint64)    # uint64 [members, 4, n_cols, n_cols]: the transmissions among them

    @classmethod
    def gathered(cls, members, tables, n_cols=1):
        """From every member's Simulator.contact_hours() dict."""
        return cls(members, *(_stack([t[k] for t in tables], (_lib.N_SETTINGS, n_cols, n_cols), np.uint64) for k in ("hours", "transmissions")))

    def rate(self):
        """float64 [4, n_cols, n_cols]: transmissions per contact-hour pooled over the members -- the sum of transmissions
        divided by the sum of hours --, NaN where there was no contact-hour."""
        return _rate(self.transmissions.sum(axis=0), self.hours.sum(axis=0))

    def dump(self, directory):
        """ensemble_contacts.npz: hours, transmissions and the pooled rate."""
        os.makedirs(directory, exist_ok=True)
        np.savez(os.path.join(directory, "ensemble_contacts.npz"), hours=self.hours, transmissions=self.transmissions, rate=self.rate())


class FlowResult:
    """What Ensemble.flows gathers: the imports table and the invasion tree of every member, one row per member and one column
    per Output Area."""

    def __init__(self, members, local, imported, exported, step, source_area):
        self.members = list(members)      # the overrides of every member
        self.local = np.asarray(local, np.uint32)                    # uint32 [members, n_areas]: transmissions inside the area
        self.imported = np.asarray(imported, np.uint32)              # ... into the area from elsewhere
        self.exported = np.asarray(exported, np.uint32)              # ... out of the area
        self.step = np.asarray(step, np.uint32)                      # cohort step of the area's first case, _lib.NEVER without one
        self.source_area = np.asarray(source_area, np.uint32)        # the area it was infected from, _lib.NO_AREA for an index case or no case

    @classmethod
    def gathered(cls, members, imports, invasions, n_areas):
        """From every member's Simulator.area_imports() and area_invasion() dicts."""
        return cls(members, *(_stack([t[k] for t in imports], (n_areas,), np.uint32) for k in ("local", "imported", "exported")),
                   *(_stack([t[k] for t in invasions], (n_areas,), np.uint32) for k in ("step", "source_area")))

    def imported_share(self):
        """float64 [n_areas]: of the area's infected residents whose infector is known, the share infected by a resident of
        another area, pooled over the members -- the sum of imported divided by the sum of imported + local --, NaN where there
        are no cases."""
        imp = self.imported.sum(axis=0, dtype=np.uint64).astype(np.float64)
        tot = imp + self.local.sum(axis=0, dtype=np.uint64).astype(np.float64)
        return _rate(imp, tot)

    def dump(self, directory):
        """ensemble_flows.npz: local, imported, exported, step, source_area and the pooled imported_share."""
        os.makedirs(directory, exist_ok=True)
        np.savez(os.path.join(directory, "ensemble_flows.npz"), local=self.local, imported=self.imported, exported=self.exported,
                 step=self.step, source_area=self.source_area, imported_share=self.imported_share())


class EventResult:
    """What Ensemble.events gathers: the event-size table of every member and its `top` largest events, one row per member."""

    KEYS = ("step", "setting", "place", "bus", "size")

    def __init__(self, members, sizes, step, setting, place, bus, size):
        self.members = list(members)      # the overrides of every member
        self.sizes = np.asarray(sizes, np.uint32)                    # uint32 [members, 4, 256]: events per setting and size, the last bin open-ended
        self.step = np.asarray(step, np.uint32)                      # [members, top] each, descending by size; _lib.NEVER behind a member's last event
        self.setting = np.asarray(setting, np.uint32)
        self.place = np.asarray(place, np.uint32)
        self.bus = np.asarray(bus, np.uint32)
        self.size = np.asarray(size, np.uint32)

    @classmethod
    def gathered(cls, members, sizes, tops, top):
        """From every member's Simulator.event_sizes() table and Simulator.transmission_events(order="size", limit=top) dict."""
        table = _stack(sizes, (_lib.N_SETTINGS, _lib.EVENT_BINS), np.uint32)
        rows = {k: np.full((len(tops), int(top)), _lib.NEVER, np.uint32) for k in cls.KEYS}
        for i, t in enumerate(tops):
            for k in cls.KEYS:
                rows[k][i, :len(t[k])] = t[k]
        return cls(members, table, *(rows[k] for k in cls.KEYS))

    def share_in_events(self, min_size):
        """float64 [members, 4]: of the transmissions of a member in a setting, the share that took place in events of at least
        min_size transmissions, NaN without a transmission.  Exact while the last bin is empty: an event there counts as 255."""
        b = np.arange(_lib.EVENT_BINS, dtype=np.float64)
        weight = self.sizes.astype(np.float64) * b
        tot, big = weight.sum(axis=2), weight[:, :, min(int(min_size), _lib.EVENT_BINS):].sum(axis=2)
        return _rate(big, tot)

    def dump(self, directory):
        """ensemble_events.npz: sizes and the five [members, top] arrays of the largest events."""
        os.makedirs(directory, exist_ok=True)
        np.savez(os.path.join(directory, "ensemble_events.npz"), sizes=self.sizes, **{k: getattr(self, k) for k in self.KEYS})


class CompareResult:
    """What Ensemble.compare gathers: every member's comparison of its policy run with its own baseline run."""

    KEYS = ("steps", "defined", "hit", "mean_baseline", "mean_policy", "mean_averted", "p_averted", "se_paired", "se_unpaired")

    def __init__(self, members, counts, delay, first_divergence, records_baseline, records_policy, summary=None, where="all", area_codes=None):
        self.members = list(members)      # the overrides of every member
        self.counts = np.asarray(counts, np.uint64)                  # uint64 [members, n_cols, 5]: _lib.CMP_BOTH .. CMP_LATER
        self.delay = np.asarray(delay, np.int64)                     # int64 [members, n_cols]: sum of (step under the policy - step in the baseline) over BOTH
        self.first_divergence = np.asarray(first_divergence, np.int64)   # int64 [members]: the first step the arms differ at, -1 where they are identical
        self.records_baseline = records_baseline                     # structured [members, n_steps]
        self.records_policy = records_policy
        self.summary = summary            # paired_summary(...) where rows were asked for, else None
        self.where = where
        self.area_codes = area_codes
        self.quantile_probs = None        # float64 [n_q], and
        self.averted_quantiles = None     # [n_q, n_rows, n_cols]: quantiles over the members of baseline - policy per cell, where compare(quantiles=...) asked

    @classmethod
    def gathered(cls, members, tables, records_baseline, records_policy, n_cols, n_steps, summary=None, where="all", area_codes=None):
        """From every member's Simulator.compare() dict and the records of its two arms."""
        counts = _stack([t["counts"] for t in tables], (n_cols, _lib.CMP_N), np.uint64)
        delay = _stack([t["delay"] for t in tables], (n_cols,), np.int64)
        div = [-1 if t["first_divergence"] is None else t["first_divergence"] for t in tables]
        return cls(members, counts, delay, div, _stack(records_baseline, (n_steps,), RECORD_DTYPE), _stack(records_policy, (n_steps,), RECORD_DTYPE),
                   summary, where, area_codes)

    def averted(self):
        """int64 [members, n_cols]: the cases the policy averted net of those it added, AVERTED - ADDED."""
        c = self.counts.astype(np.int64)
        return c[..., _lib.CMP_AVERTED] - c[..., _lib.CMP_ADDED]

    def dump(self, directory):
        """ensemble_compare.npz: counts, delay, first_divergence, averted, the class names, and the arrays of the summary (with a
        summary_ prefix) where rows were asked for; codes where area codes name the columns."""
        os.makedirs(directory, exist_ok=True)
        arrays = dict(counts=self.counts, delay=self.delay, first_divergence=self.first_divergence, averted=self.averted(), names=np.asarray(_lib.CMP_NAMES))
        if self.summary is not None:
            arrays.update({"summary_" + k: self.summary[k] for k in self.KEYS})
            arrays["summary_members"] = np.asarray(self.summary["members"], np.uint32)
        if self.area_codes is not None:
            arrays["codes"] = np.asarray(self.area_codes)
        np.savez(os.path.join(directory, "ensemble_compare.npz"), **arrays)
        if self.averted_quantiles is not None:       # a file of its own: ensemble_compare.npz is what it is without them
            extra = dict(probs=self.quantile_probs, quantiles=self.averted_quantiles)
            if self.area_codes is not None:
                extra["codes"] = np.asarray(self.area_codes)
            np.savez(os.path.join(directory, "ensemble_area_quantiles.npz"), **extra)


class BurdenCompareResult:
    """What Ensemble.compare_burden gathers: every member's hospital burden under the policy against its own baseline run."""

    KEYS = CompareResult.KEYS
    TOTALS = ("bed_steps", "admissions", "deaths")

    def __init__(self, members, totals, records_baseline, records_policy, summary=None, where="all", what="occupancy", area_codes=None):
        self.members = list(members)      # the overrides of every member
        self.totals = totals              # {"bed_steps_baseline", "bed_steps_current", "admissions_baseline", ...}: [members, n_cols] each
        self.records_baseline = records_baseline                     # structured [members, n_steps]
        self.records_policy = records_policy
        self.summary = summary            # paired_summary(...) of the rows of `what` where rows were asked for, else None
        self.where, self.what = where, what
        self.area_codes = area_codes
        self.quantile_probs = None        # float64 [n_q], and
        self.averted_quantiles = None     # [n_q, n_rows, n_cols]: quantiles over the members of baseline - policy per cell, where compare_burden(quantiles=...) asked

    @classmethod
    def gathered(cls, members, tables, records_baseline, records_policy, n_cols, n_steps, summary=None, where="all", what="occupancy", area_codes=None):
        """From every member's Simulator.burden_compare() dict and the records of its two arms."""
        totals = {}
        for k in cls.TOTALS:
            for arm in ("_baseline", "_current"):
                totals[k + arm] = _stack([t[k + arm] for t in tables], (n_cols,), np.uint64 if k == "bed_steps" else np.uint32)
        return cls(members, totals, _stack(records_baseline, (n_steps,), RECORD_DTYPE), _stack(records_policy, (n_steps,), RECORD_DTYPE), summary, where, what, area_codes)

    def _averted(self, key):
        return self.totals[key + "_baseline"].astype(np.int64) - self.totals[key + "_current"].astype(np.int64)

    def bed_days_averted(self):
        """float64 [members, n_cols]: the bed-days the policy averted, (bed-steps of the baseline - of the policy run) / 24."""
        return self._averted("bed_steps") / 24.0

    def admissions_averted(self):
        """int64 [members, n_cols]."""
        return self._averted("admissions")

    def deaths_averted(self):
        """int64 [members, n_cols]."""
        return self._averted("deaths")

    def dump(self, directory):
        """ensemble_burden_compare.npz: the six totals, bed_days_averted, admissions_averted, deaths_averted, what, and the arrays
        of the summary (with a summary_ prefix) where rows were asked for; codes where area codes name the columns; probs and
        quantiles where they were asked for."""
        os.makedirs(directory, exist_ok=True)
        arrays = dict(self.totals, bed_days_averted=self.bed_days_averted(), admissions_averted=self.admissions_averted(), deaths_averted=self.deaths_averted(),
                      what=np.asarray(self.what))
        if self.summary is not None:
            arrays.update({"summary_" + k: self.summary[k] for k in self.KEYS})
            arrays["summary_members"] = np.asarray(self.summary["members"], np.uint32)
        if self.area_codes is not None:
            arrays["codes"] = np.asarray(self.area_codes)
        if self.averted_quantiles is not None:
            arrays.update(probs=self.quantile_probs, quantiles=self.averted_quantiles)
        np.savez(os.path.join(directory, "ensemble_burden_compare.npz"), **arrays)


_EXTRA_KEYS = ("band", "band_pooled", "clusters", "cluster_metric")       # of the area dict: what reads the kept members beside the quantile maps


def _keep_spec(who, kind, area, n_members=None, keys=("quantiles", "quantile_method", "exceed", "keep") + _EXTRA_KEYS):
    """The keys of the quantile maps, of the central band and of the clusters popped from `area` and checked before any library
    call: None where none is given, else dict(probs, method, thresholds, what) -- and, where band= or band_pooled= is given, band
    (the coverage) and band_pooled; where clusters= or cluster_metric= is given, clusters (k, 2 by default) and cluster_metric;
    with either, band_only (no key of the quantile maps beside them).  ValueError for the reproduction kind (a ratio per cell
    is not kept), a probability or a coverage outside [0, 1], an unknown method or metric, clusters below 1 or above the
    members, `keep` on another kind than peaks, or more members than the store takes."""
    given = {k: area.pop(k) for k in keys if k in area}
    if not given:
        return None
    if kind == "reproduction":
        raise ValueError("%s: the reproduction kind keeps no members (a ratio per cell is out of scope): no %s" % (who, ", ".join(sorted(given))))
    probs = check_probs(who, given.get("quantiles") or ())
    method = given.get("quantile_method", "nearest")
    if method not in ("nearest", "linear"):
        raise ValueError("%s: quantile_method must be 'nearest' or 'linear', got %r" % (who, method))
    what = given.get("keep", "value")
    if what not in Simulator.KEEP_WHAT or (what != "value" and kind not in ("peaks", "burden_peaks")):
        raise ValueError("%s: keep must be 'value', or for the peaks kind 'peak_step' or 'duration', got %r" % (who, what))
    if n_members is not None and int(n_members) > _lib.MEMBERS_MAX:
        raise ValueError("%s: %d members, the store of the quantile maps takes %d (ESIM_MEMBERS_MAX)" % (who, int(n_members), _lib.MEMBERS_MAX))
    spec = dict(probs=probs, method=method, thresholds=[int(t) for t in (given.get("exceed") or ())], what=what)
    if "band" in given or "band_pooled" in given:
        coverage = float(given.get("band", 0.5))
        if not 0.0 <= coverage <= 1.0:
            raise ValueError("%s: band is the coverage of the central region and must lie in [0, 1], got %r" % (who, given.get("band")))
        spec.update(band=coverage, band_pooled=bool(given.get("band_pooled", False)), band_only=all(k in _EXTRA_KEYS for k in given))
    if "clusters" in given or "cluster_metric" in given:
        k, metric = given.get("clusters", 2), given.get("cluster_metric", "l1")
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1 or (n_members is not None and k > int(n_members)):
            raise ValueError("%s: clusters is the number of medoids and must lie in 1..the members, got %r" % (who, k))
        if metric not in Simulator.DIST_METRIC:
            raise ValueError("%s: cluster_metric must be 'l1' or 'differ', got %r" % (who, metric))
        spec.update(clusters=int(k), cluster_metric=metric, band_only=all(k in _EXTRA_KEYS for k in given))
    return spec


def medoids(distances, k, max_swaps=1000):
    """Deterministic k-medoids (PAM) over a symmetric matrix of distances [M, M], as Simulator.ensemble_distances returns it: k
    real members that stand for the ensemble, and every member with the nearest of them.
    BUILD: the first medoid is the member with the smallest sum of distances to all; each further one the member that lowers
    the cost -- the sum over the members of the distance to their nearest medoid -- most.  SWAP: while a swap of a medoid
    against a member that is none lowers the cost, the one that lowers it most is made, max_swaps at the most.  Ties go to
    the lowest index everywhere, and the sums are exact integers.  The result is a local optimum under single swaps; for k = 1
    it is the medoid of the ensemble, the member with the smallest total distance.
    Returns {"medoid": int64 [k], ascending; "label": int64 [M], the position in `medoid` of the member's nearest medoid (a
    medoid is its own; ties to the lowest); "size": int64 [k]; "cost": int; "silhouette": float64 [M]}: (b - a) / max(a, b)
    with a the mean distance to the other members of the member's cluster and b the smallest mean distance to the members of
    another cluster; 0 for a member alone in its cluster, where a = b = 0, and for k = 1.  ValueError for a matrix that is not
    square, k < 1 or k > M."""
    d = np.asarray(distances)
    if d.ndim != 2 or d.shape[0] != d.shape[1]:
        raise ValueError("medoids: distances must be a square matrix, got shape %r" % (d.shape,))
    m, k = d.shape[0], int(k)
    if not 1 <= k <= m:
        raise ValueError("medoids: k must lie in 1..%d (the members), got %d" % (m, k))
    top = int(d.max()) if m else 0
    d = d.astype(np.int64) if top * m < 1 << 62 else np.array([[int(v) for v in row] for row in d.tolist()], object)   # (sums stay exact either way)
    chosen = [int(np.argmin(d.sum(axis=0)))]
    while len(chosen) < k:
        near = d[:, chosen].min(axis=1)
        cost = np.minimum(near[:, None], d).sum(axis=0)             # the cost with member h as one more medoid
        for c in chosen:
            cost[c] = near.sum() + 1                                # (never better than a member that is none: those cost <= near.sum())
        chosen.append(int(np.argmin(cost)))
    cost = d[:, chosen].min(axis=1).sum()
    for _ in range(int(max_swaps)):
        best = None
        for p in range(k):
            rest = [c for q, c in enumerate(chosen) if q != p]
            trial = np.minimum(d[:, rest].min(axis=1)[:, None], d).sum(axis=0) if rest else d.sum(axis=0)
            for c in chosen:
                trial[c] = cost                                     # (a medoid is no candidate)
            h = int(np.argmin(trial))
            if trial[h] < cost and (best is None or trial[h] < best[0]):
                best = (trial[h], p, h)
        if best is None:
            break
        cost, chosen[best[1]] = best[0], best[2]
    chosen.sort()
    to = d[:, chosen]
    label = np.argmin(to, axis=1).astype(np.int64)
    label[chosen] = np.arange(k)
    size = np.bincount(label, minlength=k).astype(np.int64)
    cost = int(sum(int(to[i, label[i]]) for i in range(m)))
    sil = np.zeros(m, np.float64)
    if k > 1:
        total = np.stack([d[:, label == q].sum(axis=1).astype(np.float64) for q in range(k)], axis=1)     # [M, k]: to the members of each cluster
        for i in range(m):
            own = label[i]
            if size[own] < 2:
                continue
            a = total[i, own] / (size[own] - 1)
            b = min(total[i, q] / size[q] for q in range(k) if q != own)
            sil[i] = (b - a) / max(a, b) if max(a, b) > 0 else 0.0
    return {"medoid": np.asarray(chosen, np.int64), "label": label, "size": size, "cost": cost, "silhouette": sil}


ARMS_CELL_KEYS = ("p_best", "p_sole", "expected_regret", "mean")                                  # of arms_summary: per arm and cell
ARMS_OVERALL_KEYS = ("overall_p_best", "overall_p_sole", "overall_regret", "overall_mean", "overall_choice")   # ... per arm over the whole window
ARMS_TABLE_KEYS = ("best", "sole", "regret", "sum", "totals")                                     # of Simulator.ensemble_arms


def arms_summary(tables):
    """From Simulator.ensemble_arms(): the decision figures of a grid of A policies run over S futures on common random numbers.
    Per arm and cell, float64 in the shape of the tables: p_best = best / S, the share of the futures in which the arm is the
    best one (ties all count); p_sole = sole / S, in which it alone is; expected_regret = regret / S, what choosing the arm costs
    against the best arm of the same future; mean = sum / S.  From totals [S, A], every run's sum over the whole window, the
    same four for the map as a whole, [A] each: overall_p_best, overall_p_sole, overall_regret, overall_mean -- the best arm of a
    future is then the one with the smallest total (the largest where the tables were made with maximize=True) -- and
    overall_choice, the arm of least overall regret, the smallest index on a tie (decided on the exact integer sums).  Beside
    them replicates, n_arms and maximize.  NaN everywhere for S = 0."""
    totals = np.asarray(tables["totals"], np.uint64)
    s, a = int(totals.shape[0]), int(np.asarray(tables["best"]).shape[0])
    maximize = bool(tables.get("maximize", False))
    out = {"replicates": s, "n_arms": a, "maximize": maximize}
    for name, key in zip(ARMS_CELL_KEYS, ("best", "sole", "regret", "sum")):
        out[name] = _rate(tables[key], np.full(np.asarray(tables[key]).shape, s, np.float64))
    t = [[int(v) for v in row] for row in totals.tolist()]          # exact: Python integers
    best = [max(row) if maximize else min(row) for row in t]
    n_best = [sum(1 for v in row if v == b) for row, b in zip(t, best)]
    over_runs = lambda f: [sum(f(r, arm) for r in range(s)) for arm in range(a)]
    regret = over_runs(lambda r, arm: abs(t[r][arm] - best[r]))
    over = {"overall_p_best": over_runs(lambda r, arm: int(t[r][arm] == best[r])), "overall_p_sole": over_runs(lambda r, arm: int(t[r][arm] == best[r] and n_best[r] == 1)),
            "overall_regret": regret, "overall_mean": over_runs(lambda r, arm: t[r][arm])}
    for k, v in over.items():
        out[k] = _rate(np.asarray([float(x) for x in v], np.float64), np.full(a, s, np.float64))
    out["overall_choice"] = min(range(a), key=lambda arm: (regret[arm], arm)) if a else -1
    return out


class GridResult:
    """What Ensemble.grid gathers: A policies run over the same S members -- seeds and index cases --, arm by arm."""

    def __init__(self, policies, members, records, n_done, arms, tables, area=None, area_kind=None, area_codes=None):
        self.policies = [dict(p) for p in policies]                  # the overrides of every arm
        self.members = list(members)      # the overrides of every replicate
        self.records = records            # structured [n_arms, members, n_steps]
        self.n_done = np.asarray(n_done, np.uint32)                  # [n_arms, members]
        self.arms = arms                  # arms_summary(tables)
        self.tables = tables              # Simulator.ensemble_arms(): best, sole, regret, sum [n_arms, n_rows, n_cols] ([n_arms, n_cols] for the kinds without rows), totals
        self.area = area                  # the summary of the kind as run() gives it, over ALL members x arms runs:
        self.area_mixes_arms = True       # ... it mixes the arms
        self.area_kind = area_kind
        self.area_codes = area_codes

    def dump(self, directory):
        """ensemble_grid.npz: p_best, p_sole, expected_regret, mean per arm and cell; overall_p_best, overall_p_sole,
        overall_regret, overall_mean per arm and overall_choice; the integer tables best, sole, regret, sum and totals
        [replicates, n_arms]; replicates, n_arms, maximize, live_cells; steps for a kind over rows, and codes where area codes
        name the columns."""
        os.makedirs(directory, exist_ok=True)
        arrays = {k: np.asarray(self.arms[k]) for k in ARMS_CELL_KEYS + ARMS_OVERALL_KEYS + ("replicates", "n_arms", "maximize")}
        arrays.update({k: np.asarray(self.tables[k]) for k in ARMS_TABLE_KEYS + ("live_cells",)})
        if self.area is not None and "steps" in self.area:
            arrays["steps"] = self.area["steps"]
        if self.area_codes is not None:
            arrays["codes"] = np.asarray(self.area_codes)
        np.savez(os.path.join(directory, "ensemble_grid.npz"), **arrays)


def split_members(n, k):
    """The members 0 .. n - 1 as k contiguous blocks [(begin, end), ...] in order, sized as evenly as possible, the earlier
    blocks the larger ones; with n < k the last blocks are empty."""
    n, k = int(n), int(k)
    if n < 0 or k < 1:
        raise ValueError("split_members: n must be >= 0 and k >= 1, got %d and %d" % (n, k))
    q, r = divmod(n, k)
    ends = [i * q + min(i, r) for i in range(k + 1)]
    return list(zip(ends[:-1], ends[1:]))


def _check_devices(devices):
    """devices of Ensemble(...) as a tuple of ordinals, before any context is created; None stays None."""
    if devices is None:
        return None
    out = tuple(devices)
    if not out:
        raise ValueError("Ensemble: devices must name at least one device (None: one context on the device of params)")
    for d in out:
        if isinstance(d, bool) or not isinstance(d, (int, np.integer)) or d < 0:
            raise ValueError("Ensemble: devices holds device ordinals >= 0, got %r" % (d,))
    return tuple(int(d) for d in out)


_KINDS = ("census", "arrival", "series", "settings", "reproduction", "peaks", "burden_peaks", "burden_series")
_ROW_KINDS = ("series", "settings", "reproduction", "peaks", "burden_peaks", "burden_series")      # a member that stopped early has no rows behind its last step


class Ensemble:
    """Owns one Simulator -- or one per entry of `devices` --; every member is a restart of one of them under the base parameters
    changed by the member's overrides."""

    def __init__(self, population, params=None, area_codes=None, group=None, burden=None, devices=None):
        """group: None, or (labels, n_groups) for Simulator.set_groups -- what run(area=dict(where="group", ...)) counts by.
        burden: None, or the tables of _lib.burden_tables for Simulator.set_burden, set once for every member -- what
        run(area=dict(kind="burden_peaks", ...)) and run(area=dict(kind="burden_series", ...)) summarise and compare_burden()
        compares (tables of several groups need `group` with as many).
        devices: None -- one context on the device of `params` --, or a sequence of device ordinals: one Simulator per entry,
        each with its own upload of the population, groups and burden tables; repeats are allowed, (0, 0) is two contexts on one
        device.  The first entry is self.simulator.  Every loop over members then hands each context a contiguous block of
        them (split_members) on a thread of its own and merges the contexts into the first in block order."""
        devices = _check_devices(devices)
        self._others = []
        self.area_codes = area_codes
        self._own_seeds = True            # the seeds in force are the uploaded population's
        for k, device in enumerate(devices if devices is not None else (None,)):
            p = params if device is None else _lib.with_overrides(params if params is not None else _lib.default_params(), {"device": device})
            sim = Simulator(population, p, area_codes=area_codes)
            if group is not None:
                sim.set_groups(*group)
            if burden is not None:
                sim.set_burden(burden)
            # (a context's base parameters carry its own device: esim_restart insists on it)
            if k == 0:
                self.simulator, self.base = sim, _lib.with_overrides(sim.params, {})
            else:
                lane = copy.copy(self)
                lane.simulator, lane.base, lane._others = sim, _lib.with_overrides(sim.params, {}), []
                self._others.append(lane)

    def _lanes(self):
        """The contexts as views of this Ensemble that differ in simulator, base and _own_seeds; the first is self."""
        return [self] + list(getattr(self, "_others", ()))

    def _each_member(self, members, body, prepare=None, merge=False):
        """The one loop over members: body(lane, member, prepared) for every member, in member order on one context; on several,
        block i of split_members on context i, each block on a thread of its own (the library calls release the GIL).
        prepare(lane) runs once per context in front of its block.  An exception in one thread stops the others at their next
        member and is raised once they have joined.  merge: the contexts' accumulators and kept members are then merged into
        the first in block order (Simulator.ensemble_merge), so that kept slot i is member i.  Returns body's results stacked
        in member order."""
        lanes = self._lanes()
        blocks = split_members(len(members), len(lanes))
        out, errors, stop = [[] for _ in lanes], [], threading.Event()

        def work(i):
            try:
                prepared = prepare(lanes[i]) if prepare is not None else None
                for m in members[blocks[i][0]:blocks[i][1]]:
                    if stop.is_set():
                        return
                    out[i].append(body(lanes[i], m, prepared))
            except BaseException as e:          # (raised below, once every thread has joined)
                errors.append((i, e))
                stop.set()

        active = [i for i in range(len(lanes)) if i == 0 or blocks[i][1] > blocks[i][0]]
        if len(active) == 1:
            work(0)
        else:
            threads = [threading.Thread(target=work, args=(i,)) for i in active]
            for t in threads:
                t.start()
            for t in threads:
                t.join()
        if errors:
            raise min(errors, key=lambda x: x[0])[1]
        if merge and len(active) > 1:
            for i in active[1:]:
                self.simulator.ensemble_merge(lanes[i].simulator)
            self.simulator.synchronize()        # (the merges have read the other contexts: those are free again)
        return [row for rows in out for row in rows]

    def _active_lanes(self, n_members):
        """The contexts that get a member, with the size of their block: the first always."""
        lanes = self._lanes()
        return [(lane, e - b) for i, (lane, (b, e)) in enumerate(zip(lanes, split_members(n_members, len(lanes)))) if i == 0 or e > b]

    def _area_kind(self, who, area, n_steps, stop_when_done=False, n_members=None):
        """area of run() / forecast() checked, before anything runs: (kind, the area dict without its kind), or (None, None).
        For the reproduction kind `complete` is resolved here: with complete=True (the default) and n_rows=None only the rows
        are taken whose cohort has had its whole infectious period by step n_steps.  The keys of the quantile maps -- quantiles,
        quantile_method, exceed, keep -- are checked and taken out of the dict here (self._keep_spec holds them, None without
        one): the begin call never sees them."""
        self._keep_spec = None
        if area is None:
            return None, None
        area = dict(area)
        kind = area.pop("kind", "census")
        if kind not in _KINDS:
            raise ValueError("Ensemble.%s: area kind must be 'census', 'arrival' or 'series', or 'settings', 'reproduction', 'peaks', 'burden_peaks' or 'burden_series', got %r" % (who, kind))
        self._keep_spec = _keep_spec("Ensemble." + who, kind, area, n_members)
        if kind in _ROW_KINDS and stop_when_done:
            raise ValueError("Ensemble.%s: area kind %r cannot go with stop_when_done=True (a member that stopped early has no "
                             "rows behind its last step, and the library refuses the fold)" % (who, kind))
        if kind == "settings" and area.get("n_rows") is None:
            first, stride = int(area.get("first_step", 1)), int(area.get("stride", 1))
            area["n_rows"] = (int(n_steps) - first) // stride + 1 if stride > 0 and 1 <= first <= int(n_steps) else 0
        if kind == "burden_series" and area.get("n_rows") is None:
            first, stride = int(area.get("first_step", 1)), int(area.get("stride", 24))
            area["n_rows"] = (int(n_steps) - first) // stride + 1 if stride > 0 and 1 <= first <= int(n_steps) else 0
        if kind in ("peaks", "burden_peaks") and area.get("last_step") is None:
            area["last_step"] = int(n_steps)
        if kind == "reproduction":
            complete = area.pop("complete", True)
            if area.get("n_rows") is None:
                first, stride = int(area.get("first_step", 0)), int(area.get("stride", 24))
                last = int(n_steps)
                if complete:      # a row is complete when its last step s satisfies s + exposed_time + 1 + infected_time <= n_steps (Simulator.household_sar)
                    last -= int(self.base.exposed_time) + 1 + int(self.base.infected_time)
                    n_rows = (last - first + 1) // stride if stride > 0 and first >= 0 else 0
                    if n_rows < 1:
                        raise ValueError("Ensemble.%s: no complete cohort row from step %d with stride %d after %d steps (a cohort exposed in step s is complete "
                                         "once s + exposed_time + 1 + infected_time steps have run; complete=False takes the open rows too)" % (who, first, stride, int(n_steps)))
                else:
                    n_rows = (last - first) // stride + 1 if stride > 0 and 0 <= first <= last else 0
                area["n_rows"] = n_rows
        return kind, area

    def _begin(self, kind, area, n_members=0):
        for lane, _ in self._active_lanes(n_members) if kind is not None else ():
            getattr(lane.simulator, {"census": "ensemble_begin", "arrival": "ensemble_begin_arrival", "series": "ensemble_begin_series",
                          "settings": "ensemble_begin_settings", "reproduction": "ensemble_begin_reproduction", "peaks": "ensemble_begin_peaks",
                          "burden_peaks": "ensemble_begin_burden_peaks", "burden_series": "ensemble_begin_burden_series"}[kind])(**area)

    def _keep_begin(self, n_members, what=None):
        """Behind the begin: the store of the quantile maps, where the area dict asked for them -- on the first context with
        the capacity of all members, on the others with that of their block."""
        what = self._keep_spec["what"] if what is None and self._keep_spec is not None else what
        if what is not None and n_members:
            for k, (lane, block) in enumerate(self._active_lanes(n_members)):
                lane.simulator.ensemble_keep_members(n_members if k == 0 else block, what)

    def _keep_summary(self, summary, kind, n_members, area=None):
        """The summary with probs, quantiles, thresholds and exceed added: [n_q, n_rows, n_cols], [n_q, n_cols] for the kinds
        without rows (census, arrival, peaks).  With band= in the area dict it gains band_lo, band_hi, band_median ([n_rows,
        n_cols], [n_cols] for the kinds without rows), band_deepest, band_n_in [n_cols], band_need, band_coverage, band_pooled
        and depth, the modified band depth [members, n_cols] (Simulator.ensemble_band, ensemble_depth).  With clusters= it
        gains distances [members, members] (Simulator.ensemble_distances; for the arrival kind ESIM_NEVER counts as the horizon
        of `area`), cluster_medoid, cluster_label, cluster_size, cluster_silhouette and cluster_cost (medoids), cluster_metric,
        and cluster_curves [k, n_rows, n_cols], the medoids' own planes ([k, n_cols] for the kinds without rows)."""
        spec = self._keep_spec
        if spec is None or summary is None or not n_members:
            return summary
        sim = self.simulator
        flat = (lambda a: a[:, 0]) if kind in ("census", "arrival", "peaks", "burden_peaks") else (lambda a: a)
        out = dict(summary)
        if not spec.get("band_only"):
            out.update(probs=np.asarray(spec["probs"], np.float64), thresholds=np.asarray(spec["thresholds"], np.int64))
            out["quantiles"] = flat(sim.ensemble_quantiles(spec["probs"], spec["method"])) if spec["probs"] else None
            out["exceed"] = flat(sim.ensemble_exceedance(spec["thresholds"])) if spec["thresholds"] else None
        if "band" in spec:
            b = sim.ensemble_band(spec["band"], spec["band_pooled"])
            row = (lambda a: a[0]) if kind in ("census", "arrival", "peaks", "burden_peaks") else (lambda a: a)
            out.update(band_lo=row(b["lo"]), band_hi=row(b["hi"]), band_median=row(b["median"]), band_deepest=b["deepest"], band_n_in=b["n_in"], band_need=b["need"],
                       band_coverage=spec["band"], band_pooled=spec["band_pooled"], depth=sim.ensemble_depth()["mbd"])
        if "clusters" in spec:
            horizon = (area or {}).get("horizon") if kind == "arrival" else None
            dist = sim.ensemble_distances(spec["cluster_metric"], never_as=horizon)["distances"]
            c = medoids(dist, min(spec["clusters"], dist.shape[0]))
            curves = np.concatenate([sim.ensemble_members(int(i), 1) for i in c["medoid"]])           # one member a call
            out.update(distances=dist, cluster_medoid=c["medoid"], cluster_label=c["label"], cluster_size=c["size"], cluster_silhouette=c["silhouette"],
                       cluster_cost=c["cost"], cluster_metric=spec["cluster_metric"], cluster_curves=flat(curves))
        return out

    def _summary(self, kind, area):
        sim = self.simulator
        if kind is None:
            return None
        if kind in ("peaks", "burden_peaks"):
            return peaks_summary(sim.ensemble_read_peaks())
        if kind == "reproduction":
            return reproduction_summary(sim.ensemble_read_reproduction(), area.get("first_step", 0), area.get("stride", 24))
        if kind in ("series", "settings", "burden_series"):
            r = sim.ensemble_read_series()
            return series_summary(r["members"], r["hit"], r["sum"], r["sumsq"], area.get("first_step", 1), area.get("stride", 24 if kind == "burden_series" else 1))
        r = sim.ensemble_read()
        return (arrival_summary if kind == "arrival" else area_summary)(r["members"], r["hit"], r["sum"], r["sumsq"])

    def _codes(self, area):
        """The area codes that name the summary's columns: none where they are groups, settings or the one column of "all"."""
        by_area = area is not None and area.get("where", "home") in ("home", "current", _lib.AREA_HOME, _lib.AREA_CURRENT)
        return self.area_codes if by_area or area is None else None

    @staticmethod
    def _settings_rows(who, settings, n_steps, stop_when_done=False):
        """settings of run() / forecast() checked, before anything runs: the arguments of Simulator.setting_series, or None."""
        if settings is None:
            return None
        unknown = set(settings) - {"first_step", "n_rows", "stride"}
        if unknown:
            raise ValueError("Ensemble.%s: settings takes first_step, n_rows and stride, got %s" % (who, sorted(unknown)))
        if stop_when_done:
            raise ValueError("Ensemble.%s: settings cannot go with stop_when_done=True (a member that stopped early has no rows "
                             "behind its last step)" % who)
        first, stride = int(settings.get("first_step", 1)), int(settings.get("stride", 1))
        n_rows = settings.get("n_rows")
        if n_rows is None:
            n_rows = (int(n_steps) - first) // stride + 1 if stride > 0 and 1 <= first <= int(n_steps) else 0
        return dict(first_step=first, n_rows=int(n_rows), stride=stride)

    @staticmethod
    def _settings_stack(rows, spec):
        return None if spec is None else (np.stack(rows) if rows else np.zeros((0, spec["n_rows"], _lib.N_SETTINGS), np.uint32))

    @staticmethod
    def _reproduction_rows(who, reproduction, n_steps, stop_when_done=False):
        """reproduction of run() / forecast() checked, before anything runs: the arguments of Simulator.reproduction_series, or None."""
        if reproduction is None:
            return None
        unknown = set(reproduction) - {"first_step", "n_rows", "stride"}
        if unknown:
            raise ValueError("Ensemble.%s: reproduction takes first_step, n_rows and stride, got %s" % (who, sorted(unknown)))
        if stop_when_done:
            raise ValueError("Ensemble.%s: reproduction cannot go with stop_when_done=True (a member that stopped early has no "
                             "rows behind its last step)" % who)
        first, stride = int(reproduction.get("first_step", 0)), int(reproduction.get("stride", 24))
        n_rows = reproduction.get("n_rows")
        if n_rows is None:
            n_rows = (int(n_steps) - first) // stride + 1 if stride > 0 and 0 <= first <= int(n_steps) else 0
        return dict(first_step=first, n_rows=int(n_rows), stride=stride)

    @staticmethod
    def _reproduction_stack(rows, spec):
        return None if spec is None else (np.stack(rows) if rows else np.zeros((0, spec["n_rows"], 2), np.uint32))

    def _reproduction_of_member(self, spec):
        cases, offspring = self.simulator.reproduction_series("all", **spec)
        return np.concatenate([cases, offspring], axis=1)

    @staticmethod
    def seeds(k, first=1):
        return [{"seed": int(first) + i} for i in range(int(k))]

    def index_cases(self, k, n=10, first=1):
        """k members that differ in where the outbreak starts AND in the Philox seed: member i runs under seed first + i from
        the index cases Population.draw_index_cases(n, first + i) draws (n = 10: STARTING_INFECTED_COUNT, config.rs:27)."""
        pop = self.simulator.population
        return [{"seed": int(first) + i, "index_cases": pop.draw_index_cases(n, int(first) + i).tolist()} for i in range(int(k))]

    @staticmethod
    def _members(members):
        members = [dict(m) for m in members]
        for m in members:
            if "index_cases" in m:
                m["index_cases"] = [int(x) for x in np.asarray(m["index_cases"]).ravel()]
        return members

    def _restart_member(self, m):
        """The simulator back at step 0 under the base parameters changed by member m's overrides, from m's index cases or,
        without any, the population's own."""
        sim = self.simulator
        over = {k: v for k, v in m.items() if k != "index_cases"}
        seeds = m.get("index_cases")
        if seeds is None and not self._own_seeds:
            seeds = sim.population.seeds
        sim.restart(self.base, seeds=seeds, **over)
        self._own_seeds = "index_cases" not in m

    def _gather(self, members, n_steps, *calls):
        """What outbreaks() .. events() share: every member (as for run()) is restarted and run for n_steps steps, and what each
        of `calls` returns for the simulator then is kept.  Returns (members, one list per call)."""
        members = self._members(members)

        def body(lane, m, _):
            lane._restart_member(m)
            lane.simulator.run(n_steps)
            return [call(lane.simulator) for call in calls]

        got = self._each_member(members, body)
        return (members, *([row[k] for row in got] for k in range(len(calls))))

    def _group_cols(self, where):
        """The columns of the pair tables: the groups given to Ensemble(...) for where="group", else one."""
        return max(1, self.simulator._n_groups) if where in ("group", _lib.BY_GROUP) else 1

    def outbreaks(self, members, n_steps, ages=False):
        """Which introduction took off: every member (as for run()) is run for n_steps steps and its outbreak table gathered
        (Simulator.outbreaks: size, depth and last step per index case) and, with ages=True, its infectious-age profile
        (Simulator.transmission_ages).  Returns an OutbreakResult."""
        calls = (lambda sim: sim.outbreaks(),) + ((lambda sim: sim.transmission_ages(),) if ages else ())
        members, tables, *profiles = self._gather(members, n_steps, *calls)
        return OutbreakResult.gathered(members, tables, profiles[0] if ages else None)

    def households(self, members, n_steps, where="all", first_step=0, last_step=None):
        """Household outbreaks over an ensemble: every member (as for run()) is run for n_steps steps and its final-size tables
        (Simulator.household_final_sizes) and household pair tables (Simulator.household_sar(where, first_step, last_step),
        complete cohorts only) gathered.  where="group" counts by the groups given to Ensemble(...).  Returns a HouseholdResult."""
        got = self._gather(members, n_steps, lambda sim: sim.household_final_sizes(), lambda sim: sim.household_sar(where, first_step, last_step))
        return HouseholdResult.gathered(*got, self._group_cols(where))

    def places(self, members, n_steps, kind="work", where="all", first_step=0, last_step=None):
        """Work place or school outbreaks over an ensemble: every member (as for run()) is run for n_steps steps and its size
        tables (Simulator.place_sizes(kind)) and, for kind "work" or "room", its pair tables (Simulator.place_sar(kind, where,
        first_step, last_step), complete cohorts only) gathered; kind "school" has no pairs, its two pair tables stay 0.
        where="group" counts by the groups given to Ensemble(...).  Returns a PlaceResult."""
        n_cols = self._group_cols(where)
        if kind in ("school", _lib.PLACE_SCHOOL):
            pairs = lambda sim: (np.zeros((n_cols, n_cols), np.uint64),) * 2
        else:
            pairs = lambda sim: sim.place_sar(kind, where, first_step, last_step)
        return PlaceResult.gathered(*self._gather(members, n_steps, lambda sim: sim.place_sizes(kind), pairs), n_cols)

    def contacts(self, members, n_steps, where="all", settings=None, first_step=1, last_step=None):
        """Contact-hours at risk over an ensemble: every member (as for run()) is run for n_steps steps and its two tables
        (Simulator.contact_hours(where, settings, first_step, last_step)) gathered.  where="group" counts by the groups given to
        Ensemble(...).  Returns a ContactResult."""
        got = self._gather(members, n_steps, lambda sim: sim.contact_hours(where, settings, first_step, last_step))
        return ContactResult.gathered(*got, self._group_cols(where))

    def flows(self, members, n_steps, settings=None, first_step=1, last_step=None):
        """How the epidemic travels, over an ensemble: every member (as for run()) is run for n_steps steps and its imports table
        (Simulator.area_imports(settings, first_step, last_step)) and invasion tree (Simulator.area_invasion) gathered.  Returns a
        FlowResult."""
        got = self._gather(members, n_steps, lambda sim: sim.area_imports(settings, first_step, last_step), lambda sim: sim.area_invasion())
        return FlowResult.gathered(*got, self.simulator.population.n_areas)

    def events(self, members, n_steps, settings=None, first_step=1, last_step=None, top=16):
        """Superspreading events over an ensemble: every member (as for run()) is run for n_steps steps and its event-size table
        (Simulator.event_sizes(settings, first_step, last_step)) and its `top` largest events
        (Simulator.transmission_events(..., order="size", limit=top)) gathered.  Returns an EventResult."""
        got = self._gather(members, n_steps, lambda sim: sim.event_sizes(settings, first_step, last_step),
                           lambda sim: sim.transmission_events(settings, first_step, last_step, order="size", limit=top))
        return EventResult.gathered(*got, top)

    def run(self, members, n_steps, stop_when_done=False, area=None, settings=None, reproduction=None):
        """members: iterable of override dicts (Ensemble.seeds, Ensemble.index_cases); beside fields of esim_params a dict may
        carry "index_cases": the citizens that start Infected in that member (one without starts from the population's own).
        area: None, or the arguments of esim_ensemble_begin as a dict (where, status_mask, min_cases); where="group" counts by
        the groups given to Ensemble(...), and the summary then has one entry per group; or dict(kind="arrival", where=...,
        horizon=...) for the arrival step instead (esim_ensemble_begin_arrival; the summary's mean and var are then over the
        members that reached the entry, NaN where none did); or dict(kind="series", where=..., what=..., first_step=...,
        n_rows=..., stride=..., min_cases=...) for the rows of a series (Simulator.ensemble_begin_series; the summary is a
        series_summary, [n_rows, n_cols]; not with stop_when_done=True: ValueError); or dict(kind="settings", where=...,
        settings=..., first_step=..., n_rows=..., stride=..., min_cases=...) for the exposures by setting per Output Area or
        group (Simulator.ensemble_begin_settings; a series_summary again); or dict(kind="reproduction", where=..., first_step=...,
        n_rows=..., stride=..., min_cohort=..., r=(num, den), complete=True) for the cohort rows (Simulator.
        ensemble_begin_reproduction; the summary is a reproduction_summary); or dict(kind="peaks", where=..., status=...,
        first_step=..., last_step=..., threshold=..., min_peak=...) for the shape of every member's curve per column
        (Simulator.ensemble_begin_peaks; last_step=None: n_steps; the summary is a peaks_summary); or dict(kind="burden_peaks",
        where=..., first_step=..., last_step=..., threshold=..., min_peak=...) for the same of every member's bed occupancy
        under the tables of Ensemble(..., burden=...) (Simulator.ensemble_begin_burden_peaks: per column P(peak occupancy >=
        min_peak) and the mean and deviation of peak, peak step and duration); or dict(kind="burden_series", what=..., where=...,
        first_step=..., n_rows=..., stride=..., min_count=...) for the rows of every member's hospital burden (Simulator.
        ensemble_begin_burden_series: the fan chart -- per row and column hit = the members with at least min_count, beds
        against a capacity, and mean and var; a series_summary).  With complete=True and n_rows=None only complete
        cohort rows are taken -- an incomplete cohort biases R down -- and ValueError is raised when there is none.  Neither goes
        with stop_when_done=True.
        Every kind but reproduction also takes quantiles=(0.05, 0.5, 0.95), quantile_method="nearest" or "linear", exceed=(1, 5)
        and, for peaks, keep="value", "peak_step" or "duration": the members' values per cell are then kept on the device
        (Simulator.ensemble_keep_members) and the summary gains probs, quantiles [n_q, n_rows, n_cols] ([n_q, n_cols] for the
        kinds without rows), thresholds and exceed -- the members at or above each threshold.  At most 256 members.
        They also take band=0.5 and band_pooled=False: the members are ranked as whole curves on the device (modified band
        depth, Simulator.ensemble_depth) and the summary gains band_lo and band_hi, the envelope of the most central
        ceil(band x members) of them, band_median, the curve of the deepest member -- a real run, unlike a row of quantiles --,
        band_deepest, band_n_in, band_need and depth [members, n_cols] (Simulator.ensemble_band); band_pooled=True ranks the
        members once for all columns, by default every column ranks its own.
        And clusters=k with cluster_metric="l1" or "differ": the members are compared pair by pair on the device
        (Simulator.ensemble_distances) and grouped round k of them (medoids): the summary gains distances, cluster_medoid,
        cluster_label, cluster_size, cluster_silhouette, cluster_cost, cluster_metric and cluster_curves, the medoids' own rows.
        settings: None, or dict(first_step=..., n_rows=..., stride=...): every member's exposures by setting
        (Simulator.setting_series(where="setting")) gathered on the host as EnsembleResult.settings, [members, n_rows, 4]; not
        with stop_when_done=True either.
        reproduction: None, or dict(first_step=..., n_rows=..., stride=...): every member's cohort rows
        (Simulator.reproduction_series("all")) gathered as EnsembleResult.reproduction, [members, n_rows, 2] = (cases,
        offspring); not with stop_when_done=True either.  Returns an EnsembleResult."""
        members = self._members(members)
        kind, area = self._area_kind("run", area, n_steps, stop_when_done, len(members))
        spec = self._settings_rows("run", settings, n_steps, stop_when_done)
        r_spec = self._reproduction_rows("run", reproduction, n_steps, stop_when_done)
        self._begin(kind, area, len(members))
        self._keep_begin(len(members))

        def body(lane, m, _):
            sim = lane.simulator
            lane._restart_member(m)
            rec = sim.run(n_steps, stop_when_done=stop_when_done)
            if area is not None:
                sim.ensemble_fold()
            return (len(rec), pad_records(rec, n_steps), sim.setting_series("setting", **spec) if spec is not None else None,
                    lane._reproduction_of_member(r_spec) if r_spec is not None else None)

        got = self._each_member(members, body, merge=area is not None)
        n_done, rows, by_setting, by_cohort = ([g[k] for g in got] for k in range(4))
        records = _stack(rows, (n_steps,), RECORD_DTYPE)
        summary = self._keep_summary(self._summary(kind, area), kind, len(members), area)
        return EnsembleResult(records, n_done, members, summary, self._codes(area), self._settings_stack(by_setting, spec),
                              self._reproduction_stack(by_cohort, r_spec), kind)

    def forecast(self, history_steps, members, n_steps, area=None, settings=None, reproduction=None):
        """Given the epidemic as it stands after `history_steps` steps under the base parameters, what happens next: the base
        run is made once and kept on the device (Simulator.snapshot), and every member is a branch from it -- a rollback under
        the base parameters changed by the member's overrides, then the remaining n_steps - history_steps steps.  members as
        for run(), without "index_cases" (the seeds belong to the shared history) and without other times or working hours (the
        library refuses them).  area, settings and reproduction: as for run(), folded / gathered once per member.  Returns an EnsembleResult whose records are
        [members, n_steps], the shared history repeated in every row."""
        members = [dict(m) for m in members]
        kind, area = self._area_kind("forecast", area, n_steps, False, len(members))
        spec = self._settings_rows("forecast", settings, n_steps)
        r_spec = self._reproduction_rows("forecast", reproduction, n_steps)
        history_steps, n_steps = int(history_steps), int(n_steps)
        if not 1 <= history_steps <= n_steps:
            raise ValueError("Ensemble.forecast: history_steps must be in 1..n_steps")
        if any("index_cases" in m for m in members):
            raise ValueError("Ensemble.forecast: a branch cannot change the index cases of the shared history")
        self._begin(kind, area, len(members))
        self._keep_begin(len(members))

        def body(lane, m, history):
            sim = lane.simulator
            sim.rollback(**m)
            rec = sim.run(n_steps - history_steps) if n_steps > history_steps else np.zeros(0, RECORD_DTYPE)
            if area is not None:
                sim.ensemble_fold()
            return (len(history) + len(rec), pad_records(np.concatenate([history, rec]), n_steps), sim.setting_series("setting", **spec) if spec is not None else None,
                    lane._reproduction_of_member(r_spec) if r_spec is not None else None)

        # (the history is run and kept on every context: it is deterministic, so the contexts' histories are identical)
        got = self._each_member(members, body, prepare=lambda lane: lane._shared_history(history_steps), merge=area is not None)
        n_done, rows, by_setting, by_cohort = ([g[k] for g in got] for k in range(4))
        records = _stack(rows, (n_steps,), RECORD_DTYPE)
        summary = self._keep_summary(self._summary(kind, area), kind, len(members), area)
        return EnsembleResult(records, n_done, members, summary, self._codes(area), self._settings_stack(by_setting, spec),
                              self._reproduction_stack(by_cohort, r_spec), kind)

    def _shared_history(self, history_steps):
        """The base run of history_steps steps made on this context and kept on the device (Simulator.snapshot); its records."""
        sim = self.simulator
        sim.restart(self.base, seeds=None if self._own_seeds else sim.population.seeds)
        self._own_seeds = True
        history = sim.run(history_steps)
        sim.snapshot()
        return history

    _FIXED_BY_HISTORY = ("exposed_time", "infected_time", "start_hour", "end_hour")

    def compare(self, baseline, policy, members, n_steps, history_steps=None, where="all", rows=None, quantiles=None, quantile_method="nearest"):
        """A policy against a baseline, member by member and PAIRED: every member (as for run()) is run for n_steps steps under
        the base parameters changed by `baseline` and by its own overrides, that run is kept on the device
        (Simulator.keep_baseline), and the member is run again under `policy` instead of `baseline` with the same seed and the
        same index cases.  The two runs share their random numbers, so what Simulator.compare(where) then counts -- gathered
        per member -- is the policy's effect and not noise.  baseline, policy: override dicts on the base parameters.
        rows: None, or dict(first_step=..., n_rows=..., stride=..., cumulative=..., min_baseline=..., min_averted=...): every
        member is also folded into the paired accumulators (Simulator.ensemble_begin_paired) and the result carries
        paired_summary of them.  history_steps: None, or the steps of a shared history that is run once under the base
        parameters and kept (Simulator.snapshot); both arms of every member are then branches from it (the rules of forecast():
        no "index_cases" in a member, no other times or working hours in baseline or policy -- ValueError).
        quantiles: None, or probabilities (with rows): the members' baseline - current per cell are kept on the device
        (Simulator.ensemble_keep_members) and CompareResult.averted_quantiles holds their quantiles, [n_q, n_rows, n_cols] --
        int32 for quantile_method="nearest", float64 for "linear".  Returns a CompareResult."""
        sim = self.simulator
        n_steps = int(n_steps)
        place = sim._compare_place("Ensemble.compare", where)
        baseline, policy, members, history_steps = self._paired_check("Ensemble.compare", baseline, policy, members, n_steps, history_steps)
        keep = _keep_spec("Ensemble.compare", "paired", dict(quantiles=quantiles, quantile_method=quantile_method), len(members)) if quantiles is not None else None
        if keep is not None and rows is None:
            raise ValueError("Ensemble.compare: quantiles are taken of the paired rows: give rows= too")
        if rows is not None:
            unknown = set(rows) - {"first_step", "n_rows", "stride", "cumulative", "min_baseline", "min_averted"}
            if unknown:
                raise ValueError("Ensemble.compare: rows takes first_step, n_rows, stride, cumulative, min_baseline and min_averted, got %s" % sorted(unknown))
            rows = dict(rows)
            first, n_rows, stride = sim._compare_rows("Ensemble.compare", rows.get("first_step", 0), rows.get("n_rows"), rows.get("stride", 24), n_steps)
            rows.update(first_step=first, n_rows=n_rows, stride=stride)
            for lane, _ in self._active_lanes(len(members)):
                lane.simulator.ensemble_begin_paired(where, **rows)
            if keep is not None:
                self._keep_begin(len(members), "value")
        tables, rec_b, rec_p = self._paired_members(baseline, policy, members, n_steps, history_steps, lambda s: s.keep_baseline(), lambda s: s.compare(where, 0, n_steps),
                                                    rows is not None)
        summary = None if rows is None else paired_summary(sim.ensemble_read_paired(), rows["first_step"], rows["stride"])
        codes = self.area_codes if place == _lib.AREA_HOME else None
        out = CompareResult.gathered(members, tables, rec_b, rec_p, sim._compare_cols(place), n_steps, summary, where, codes)
        if keep is not None and members and keep["probs"]:
            out.quantile_probs = np.asarray(keep["probs"], np.float64)
            out.averted_quantiles = sim.ensemble_quantiles(keep["probs"], keep["method"])
        return out

    def _paired_check(self, who, baseline, policy, members, n_steps, history_steps):
        """The arguments compare() and compare_burden() share, checked before anything runs: (baseline, policy, members,
        history_steps) as dicts, a list of dicts and an int or None."""
        baseline, policy = dict(baseline), dict(policy)
        members = self._members(members)
        if "index_cases" in baseline or "index_cases" in policy:
            raise ValueError("%s: the index cases belong to the member, not to an arm (the pairing needs the same ones in both)" % who)
        if history_steps is not None:
            history_steps = int(history_steps)
            if not 1 <= history_steps <= n_steps:
                raise ValueError("%s: history_steps must be in 1..n_steps" % who)
            if any("index_cases" in m for m in members):
                raise ValueError("%s: a branch cannot change the index cases of the shared history" % who)
            fixed = sorted(k for k in self._FIXED_BY_HISTORY if k in baseline or k in policy)
            if fixed:
                raise ValueError("%s: %s cannot change behind a shared history" % (who, ", ".join(fixed)))
        return baseline, policy, members, history_steps

    def _paired_members(self, baseline, policy, members, n_steps, history_steps, keep, table, fold):
        """The member loop compare() and compare_burden() share, behind their begins: the shared history once where asked for;
        then per member the baseline arm, keep(simulator), the policy arm, table(simulator) -- gathered -- and, with `fold`, the
        fold into the accumulators in force.  Returns (the tables, the padded records of the baseline arms, of the policy arms)."""
        def prepare(lane):
            return np.zeros(0, RECORD_DTYPE) if history_steps is None else lane._shared_history(history_steps)

        def arm(lane, history, over, m):
            sim = lane.simulator
            if history_steps is None:
                lane._restart_member(dict(over, **m))
                return sim.run(n_steps)
            sim.rollback(**dict(over, **m))
            rec = sim.run(n_steps - history_steps) if n_steps > history_steps else np.zeros(0, RECORD_DTYPE)
            return np.concatenate([history, rec])

        def body(lane, m, history):
            sim = lane.simulator
            rec_b = pad_records(arm(lane, history, baseline, m), n_steps)
            keep(sim)
            rec_p = pad_records(arm(lane, history, policy, m), n_steps)
            got = table(sim)
            if fold:
                sim.ensemble_fold()
            return got, rec_b, rec_p

        got = self._each_member(members, body, prepare=prepare, merge=fold)
        return tuple([g[k] for g in got] for k in range(3))

    def grid(self, policies, members, n_steps, history_steps=None, area=None, maximize=False, never_as=None):
        """A grid of policies over the same random futures: every member s (as for run(): a seed, index cases) is run once under
        each of `policies` -- 1 to 16 override dicts on the base parameters, the arms --, arm after arm, and every run is folded
        into the accumulators of `area` and kept on the device (Simulator.ensemble_keep_members): kept slot s * A + a is member
        s under arm a.  The arms of a member share their random numbers, as the two runs of compare() do, so that they differ by
        the policy alone.  Simulator.ensemble_arms then counts on the device, per cell, in how many futures each arm is the best
        one -- the smallest value, the largest with maximize=True --, in how many it alone, and its regret against the best arm
        of the same future; never_as is what _lib.NEVER counts as for the arrival kind and for peaks with keep="peak_step".
        area: an area dict as for run(), of any kind but "reproduction" (a ratio per cell is not kept); required.  At most 256
        runs, members x arms.  history_steps: None, or the steps of a shared history run once under the base parameters and
        kept (Simulator.snapshot); every run is then a branch from it, under the rules of compare(): no "index_cases" in a
        member, no other times or working hours in a policy.  "index_cases" in a policy is refused either way: they belong to
        the member.  On several contexts (devices=) each takes a contiguous block of members with all their arms, and the merge
        keeps the slots in order.  Returns a GridResult: records [n_arms, members, n_steps], arms (arms_summary), tables, and
        area, the summary of the kind over all runs -- which mixes the arms."""
        who = "Ensemble.grid"
        policies = [dict(p) for p in policies]
        n_steps = int(n_steps)
        if not 1 <= len(policies) <= _lib.ARMS_MAX:
            raise ValueError("%s: policies holds 1 to %d override dicts (ESIM_ARMS_MAX), got %d" % (who, _lib.ARMS_MAX, len(policies)))
        members = self._members(members)
        if not members:
            raise ValueError("%s: no members" % who)
        n_arms, n_runs = len(policies), len(policies) * len(members)
        if n_runs > _lib.MEMBERS_MAX:
            raise ValueError("%s: %d members x %d policies are %d runs, the store takes %d (ESIM_MEMBERS_MAX)" % (who, len(members), n_arms, n_runs, _lib.MEMBERS_MAX))
        for p in policies:
            history_steps = self._paired_check(who, p, p, members, n_steps, history_steps)[3]
        if area is None:
            raise ValueError("%s: area is required (the cells the arms are compared in)" % who)
        if dict(area).get("kind", "census") == "reproduction":
            raise ValueError("%s: the reproduction kind keeps no members (a ratio per cell is out of scope)" % who)
        kind, area = self._area_kind("grid", area, n_steps, False, n_runs)
        what = self._keep_spec["what"] if self._keep_spec is not None else "value"
        self._begin(kind, area, len(members))
        for k, (lane, block) in enumerate(self._active_lanes(len(members))):
            lane.simulator.ensemble_keep_members((len(members) if k == 0 else block) * n_arms, what)

        def prepare(lane):
            return np.zeros(0, RECORD_DTYPE) if history_steps is None else lane._shared_history(history_steps)

        def body(lane, m, history):
            sim, rows = lane.simulator, []
            for p in policies:
                if history_steps is None:
                    lane._restart_member(dict(p, **m))
                    rec = sim.run(n_steps)
                else:
                    sim.rollback(**dict(p, **m))
                    rec = np.concatenate([history, sim.run(n_steps - history_steps) if n_steps > history_steps else np.zeros(0, RECORD_DTYPE)])
                sim.ensemble_fold()
                rows.append((len(rec), pad_records(rec, n_steps)))
            return rows

        got = self._each_member(members, body, prepare=prepare, merge=True)
        records = np.stack([_stack([g[a][1] for g in got], (n_steps,), RECORD_DTYPE) for a in range(n_arms)])
        n_done = np.asarray([[g[a][0] for g in got] for a in range(n_arms)], np.uint32)
        tables = self.simulator.ensemble_arms(n_arms, maximize, never_as)
        if kind in ("census", "arrival", "peaks", "burden_peaks"):  # the kinds without rows: [n_arms, n_cols]
            tables.update({k: tables[k][:, 0] for k in ("best", "sole", "regret", "sum")})
        summary = self._keep_summary(self._summary(kind, area), kind, n_runs, area)
        return GridResult(policies, members, records, n_done, arms_summary(tables), tables, summary, kind, self._codes(area))

    def compare_burden(self, baseline, policy, members, n_steps, history_steps=None, where="all", what="occupancy", rows=None, quantiles=None):
        """compare() for the hospital burden under the tables of Ensemble(..., burden=...): every member is run under `baseline`,
        its admitted cases are kept on the device (Simulator.keep_burden_baseline), it is run again under `policy` with the same
        seed and index cases, and Simulator.burden_compare(where) over the steps 1 .. n_steps is gathered -- bed-steps,
        admissions and deaths of both arms per column.  A case's outcome is keyed by its onset: cases that keep theirs have the
        same outcome in both arms, which is what reduces the variance of the difference.  rows: None, or dict(first_step=...,
        n_rows=..., stride=..., cumulative=..., min_baseline=..., min_averted=...): every member is also folded into the
        burden-paired accumulators of `what` ("occupancy", "admissions" or "deaths"; Simulator.ensemble_begin_burden_paired)
        and the result carries paired_summary of them.  quantiles: None, or probabilities (with rows): the quantiles over the
        members of baseline - policy per cell, BurdenCompareResult.averted_quantiles (int32, the inverted CDF).  history_steps as
        for compare().  Returns a BurdenCompareResult."""
        sim = self.simulator
        n_steps = int(n_steps)
        who = "Ensemble.compare_burden"
        place = sim._compare_place(who, where)
        baseline, policy, members, history_steps = self._paired_check(who, baseline, policy, members, n_steps, history_steps)
        keep = _keep_spec(who, "paired", dict(quantiles=quantiles), len(members)) if quantiles is not None else None
        if keep is not None and rows is None:
            raise ValueError("%s: quantiles are taken of the paired rows: give rows= too" % who)
        if rows is not None:
            unknown = set(rows) - {"first_step", "n_rows", "stride", "cumulative", "min_baseline", "min_averted"}
            if unknown:
                raise ValueError("%s: rows takes first_step, n_rows, stride, cumulative, min_baseline and min_averted, got %s" % (who, sorted(unknown)))
            rows = dict(rows)
            first, stride = int(rows.get("first_step", 1)), int(rows.get("stride", 24))
            n_rows = rows.get("n_rows")
            if n_rows is None:
                n_rows = (n_steps - first) // stride + 1 if stride > 0 and 1 <= first <= n_steps else 0
            rows.update(first_step=first, n_rows=int(n_rows), stride=stride)
            for lane, _ in self._active_lanes(len(members)):
                lane.simulator.ensemble_begin_burden_paired(where, what, **rows)
            if keep is not None:
                self._keep_begin(len(members), "value")
        tables, rec_b, rec_p = self._paired_members(baseline, policy, members, n_steps, history_steps, lambda s: s.keep_burden_baseline(),
                                                    lambda s: s.burden_compare(where, 1, n_steps), rows is not None)
        summary = None if rows is None else paired_summary(sim.ensemble_read_paired(), rows["first_step"], rows["stride"])
        codes = self.area_codes if place == _lib.AREA_HOME else None
        out = BurdenCompareResult.gathered(members, tables, rec_b, rec_p, sim._compare_cols(place), n_steps, summary, where, what, codes)
        if keep is not None and members and keep["probs"]:
            out.quantile_probs = np.asarray(keep["probs"], np.float64)
            out.averted_quantiles = sim.ensemble_quantiles(keep["probs"], keep["method"])
        return out

    def close(self):
        for lane in self._lanes():
            lane.simulator.close()
