"""Expected results of esim_curve_summary and of the peaks ensemble kind, computed with numpy. Test infrastructure only.

The curves are the status rows of tests/_group_ref.py's reference_tables -- the CPU oracle stepped one step at a time and its
state binned by label after every step --, so nothing here comes from the library.  The home area is a label like any other
(tests/_area_status_ref.py's home_area_labels), and "all" is the label 0 for everybody."""
import functools

import numpy as np

import _area_ref
import _area_status_ref
import _group_ref

NEVER = 0xFFFFFFFF
EXPOSED, INFECTED = 1, 2
STATUS = ("exposed", "infected", "active")
KEYS = ("peak", "peak_step", "steps_at_least", "first_at_least", "last_at_least", "person_steps")
PEAKS_KEYS = ("defined", "hit", "sum_peak", "sumsq_peak", "sum_step", "sumsq_step", "sum_duration", "sumsq_duration")


def curves(status_rows, status):
    """x[s - 1, col] for the steps 1 .. n_steps from status rows [n_steps, n_cols, 5]."""
    rows = np.asarray(status_rows)
    if status == "active":
        return rows[:, :, EXPOSED].astype(np.int64) + rows[:, :, INFECTED]
    return rows[:, :, {"exposed": EXPOSED, "infected": INFECTED}[status]].astype(np.int64)


def summarize(x, first_step=1, last_step=None, threshold=1):
    """The six arrays of esim_curve_summary over the steps first_step .. last_step of x[s - 1, col]."""
    x = np.asarray(x, np.int64)
    last_step = x.shape[0] if last_step is None else last_step
    assert 1 <= first_step <= last_step <= x.shape[0] and threshold >= 1
    w = x[first_step - 1:last_step]
    steps = np.arange(first_step, last_step + 1, dtype=np.int64)[:, None]
    peak = w.max(axis=0)
    peak_step = np.where(peak > 0, first_step + w.argmax(axis=0), NEVER)            # (argmax: the first maximum)
    at = w >= threshold
    n_at = at.sum(axis=0)
    first = np.where(n_at > 0, np.where(at, steps, np.iinfo(np.int64).max).min(axis=0), NEVER)
    last = np.where(n_at > 0, np.where(at, steps, -1).max(axis=0), NEVER)
    return {"peak": peak.astype(np.uint32), "peak_step": peak_step.astype(np.uint32), "steps_at_least": n_at.astype(np.uint32),
            "first_at_least": first.astype(np.uint32), "last_at_least": last.astype(np.uint32), "person_steps": w.sum(axis=0).astype(np.uint64)}


def brute_force(x, first_step, last_step, threshold):
    """The same by a loop over the columns and the steps, as the header words it."""
    out = {k: [] for k in KEYS}
    for col in range(len(x[0])):
        peak, peak_step, n_at, first, last, total = 0, NEVER, 0, NEVER, NEVER, 0
        for s in range(first_step, last_step + 1):
            v = int(x[s - 1][col])
            if v > peak:
                peak, peak_step = v, s
            if v >= threshold:
                n_at += 1
                first = s if first == NEVER else first
                last = s
            total += v
        for k, v in zip(KEYS, (peak, peak_step, n_at, first, last, total)):
            out[k].append(v)
    return {k: np.asarray(v, np.uint64 if k == "person_steps" else np.uint32) for k, v in out.items()}


def fold(summaries, min_peak):
    """The accumulators of the peaks kind after folding the given summarize() results, and the member count."""
    n = len(summaries[0]["peak"])
    acc = {k: np.zeros(n, np.uint32 if k in ("defined", "hit") else np.uint64) for k in PEAKS_KEYS}
    for s in summaries:
        peak, dur = s["peak"].astype(np.uint64), s["steps_at_least"].astype(np.uint64)
        defined = s["peak"] >= 1
        step = np.where(defined, s["peak_step"], 0).astype(np.uint64)
        acc["defined"] += defined.astype(np.uint32)
        acc["hit"] += (s["peak"] >= min_peak).astype(np.uint32)
        acc["sum_peak"] += peak; acc["sumsq_peak"] += peak * peak
        acc["sum_step"] += step; acc["sumsq_step"] += step * step
        acc["sum_duration"] += dur; acc["sumsq_duration"] += dur * dur
    return dict(acc, members=len(summaries))


def labels_for(pop, where, group=None):
    """(labels, n_cols) of a `where` of the library: "all", "home", or "group" with group = (labels, n_groups)."""
    if where == "all":
        return np.zeros(pop.n_citizens, np.uint16), 1
    if where == "home":
        return _area_status_ref.home_area_labels(pop), pop.n_areas
    return np.asarray(group[0]), int(group[1])


def reference_rows(pop, ep, n_steps, where, group=None):
    """The oracle's tables by the labels of `where` (tests/_group_ref.py's reference_tables)."""
    labels, n_cols = labels_for(pop, where, group)
    return _group_ref.reference_tables(pop, ep, labels, n_cols, n_steps)


@functools.lru_cache(maxsize=None)
def fixture_a_rows():
    """(pop, ep, age-band labels, n_groups, {where: reference tables}) of fixture A over its 700 steps, computed once per session.
    The tables by home area are those of tests/_area_status_ref.py's cache, and the one column of "all" is the groups' summed."""
    pop, ep, labels, n_groups = _group_ref.fixture_a_groups()
    home = _area_status_ref.fixture_a_tables()[2]
    group = reference_rows(pop, ep, _area_ref.FIXTURE_A_STEPS, "group", (labels, n_groups))
    tables = {"home": {"status_rows": home["home"], "records": home["records"], "final_state": home["final_state"]},
              "all": {"status_rows": group["status_rows"].sum(axis=1, keepdims=True)}, "group": group}
    return pop, ep, labels, n_groups, tables
