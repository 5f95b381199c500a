"""What the ensemble accumulators over the transmission rows must hold, in numpy: the fold of a list of member rows into the
accumulators of esim_ensemble_begin_settings and esim_ensemble_begin_reproduction (uint64 throughout, which wraps as the device's
64-bit adds do), the host summary of the reproduction kind computed directly from the stacked member rows, and the worlds, members
and windows that tests/test_ensemble_transmission.py and tests/test_ensemble_transmission_gpu.py share.  Test infrastructure only."""
import functools

import numpy as np

import _setting_ref as ref_mod
import _tree_ref as tree

EPS = 2.0 ** -53
U64 = np.uint64


def fold_settings(rows, min_cases=1):
    """rows: per member the uint32 [n_rows, n_cols] of esim_setting_series."""
    x = np.stack([np.asarray(r) for r in rows]).astype(U64)
    return {"members": x.shape[0], "hit": (x >= U64(min_cases)).sum(0).astype(np.uint32), "sum": x.sum(0, dtype=U64), "sumsq": (x * x).sum(0, dtype=U64)}


def fold_reproduction(rows, min_cohort=1, r=(1, 1)):
    """rows: per member (cases, offspring), uint32 [n_rows, n_cols] each, as esim_reproduction_series returns them."""
    c = np.stack([np.asarray(a) for a, _ in rows]).astype(U64)
    o = np.stack([np.asarray(b) for _, b in rows]).astype(U64)
    defined = c >= U64(min_cohort)
    hit = defined & (o * U64(r[1]) >= c * U64(r[0]))                   # (both factors are below 2^32: the products fit)
    return {"members": c.shape[0], "defined": defined.sum(0).astype(np.uint32), "hit": hit.sum(0).astype(np.uint32),
            "sum_cases": c.sum(0, dtype=U64), "sum_offspring": o.sum(0, dtype=U64), "sumsq_cases": (c * c).sum(0, dtype=U64),
            "sumsq_offspring": (o * o).sum(0, dtype=U64), "sum_cross": (c * o).sum(0, dtype=U64)}


REPRODUCTION_KEYS = ("defined", "hit", "sum_cases", "sum_offspring", "sumsq_cases", "sumsq_offspring", "sum_cross")


def same_fold(got, want, keys, what=""):
    assert got["members"] == want["members"], (what, got["members"], want["members"])
    for k in keys:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        bad = np.flatnonzero(g.ravel() != w.ravel())
        assert bad.size == 0, "%s: %s differs in %d of %d cells, first at %d: got %s, expected %s" % (what, k, bad.size, g.size, bad[0], g.ravel()[bad[0]], w.ravel()[bad[0]])


def direct_summary(rows, min_cohort=1, r=(1, 1)):
    """r, p_r and r_se straight from the stacked member rows, in float64 (the counts are small integers: sums and products of
    them are exact).  r_se is the delta method over members with the sample covariances (ddof = 1):

        Var(r) = (s_oo - 2 r s_co + r^2 s_cc) / (members * mean(c)^2),   s_oo - 2 r s_co + r^2 s_cc = sum_i (o_i - r c_i)^2 / (members - 1)

    (the residuals o_i - r c_i sum to zero).  "r_se" takes the right-hand form, whose rounding error is absolute: a residual
    carries at most 3 EPS * sum(o), so r_se at most 3 EPS * r * members / sqrt(members - 1) -- se_atol(), per cell.  "r_se_cov"
    takes the left-hand form with np.cov's arithmetic; its three terms cancel where offspring is nearly proportional to cases, so it
    only agrees to about sqrt(EPS) * r there."""
    c = np.stack([np.asarray(a) for a, _ in rows]).astype(np.float64)
    o = np.stack([np.asarray(b) for _, b in rows]).astype(np.float64)
    m = c.shape[0]
    sc, so = c.sum(0), o.sum(0)
    defined = c >= min_cohort
    hit = defined & (o * r[1] >= c * r[0])
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(sc > 0, so / sc, np.nan)
        p_r = np.where(defined.sum(0) > 0, hit.sum(0) / defined.sum(0), np.nan)
        if m >= 2:
            e = o - ratio * c
            r_se = np.sqrt((e * e).sum(0) / (m - 1) / m) / (sc / m)
            dc, do = c - c.mean(0), o - o.mean(0)
            s_cc, s_oo, s_co = (dc * dc).sum(0) / (m - 1), (do * do).sum(0) / (m - 1), (dc * do).sum(0) / (m - 1)
            r_se_cov = np.sqrt(np.maximum(s_oo - 2 * ratio * s_co + ratio * ratio * s_cc, 0.0) / m) / (sc / m)
            r_se, r_se_cov = np.where(sc > 0, r_se, np.nan), np.where(sc > 0, r_se_cov, np.nan)
        else:
            r_se = r_se_cov = np.full(sc.shape, np.nan)
    return {"members": m, "r": ratio, "p_r": p_r, "r_se": r_se, "r_se_cov": r_se_cov, "cases_mean": sc / m, "offspring_mean": so / m}


def se_atol(members, ratio):
    """The absolute rounding error direct_summary's r_se may carry, per cell (its docstring); 0 where r is NaN."""
    return np.nan_to_num(4.0 * EPS * members / np.sqrt(max(members - 1, 1)) * ratio)


# ---- the worlds and their three members ----------------------------------------------------------------------------------------
AGE_EDGES = (16, 35, 50, 65)                                           # five groups: cell counts that are odd
EXTRA_SEEDS = (1001, 1002)                                             # beside the world's own seed
ROLLBACK_BRANCHES = ("rollback", "rollback_chance", "rollback_straight")


def labels_of(pop):
    return pop.age_bands(AGE_EDGES)


@functools.lru_cache(maxsize=None)
def members(world):
    """(population, parameters, steps, [(overrides, reference)] x 3): the members of an ensemble over a cached world of _tree_ref.
    A plain world gives its own seed and two more, each an esim_restart under the override; "rollback" gives the three
    branches _tree_ref caches -- under another seed and exposure_chance, under another exposure_chance, under the snapshot's
    own values --, each an esim_rollback under the override from the snapshot at step rollback_world()[2]."""
    if world == "rollback":
        pop, a, t, b, n = ref_mod.rollback_world()
        over = ({"seed": int(b.seed), "exposure_chance": b.exposure_chance}, {"exposure_chance": b.exposure_chance}, {})
        return pop, a, n, [(o, tree.cached(k)[3]) for o, k in zip(over, ROLLBACK_BRANCHES)]
    pop, ep, n, ref = tree.cached(world)
    out = [({"seed": int(ep.seed)}, ref)]
    for seed in EXTRA_SEEDS:
        ep_k = ref_mod.copy_params(ep, seed=seed)
        out.append(({"seed": seed}, tree.reference(pop, ep_k, n, ref_mod.reference(pop, ep_k, n))))
    return pop, ep, n, out


def reproduction_of(world, where, window):
    """Per member the (cases, offspring) rows of the window, from the references."""
    pop, _, _, mem = members(world)
    lab, n_groups = labels_of(pop)
    return [tree.reproduction_rows(ref, pop, where, window["first_step"], window["n_rows"], window["stride"], lab, n_groups) for _, ref in mem]


def settings_of(world, where, settings, window):
    """Per member the rows of esim_setting_series of the window, from the references.  settings: None or a tuple of codes."""
    pop, _, _, mem = members(world)
    lab, n_groups = labels_of(pop)
    mask = 0xF if settings is None else sum(1 << s for s in settings)
    return [ref_mod.rows(ref, pop, where, mask, window["first_step"], window["n_rows"], window["stride"], lab, n_groups) for _, ref in mem]


def W(first_step, n_rows, stride):
    return dict(first_step=first_step, n_rows=n_rows, stride=stride)


# (world, where, window, r, min_cohort) of the device comparisons.  The cell counts are 448, 25, 6, 7, 100 and 15: 0, 1, 2 and 3
# modulo 4 (more than one workgroup and the stride loop are the probe's, tests/test_ratio_probe_gpu.py).
# test_ensemble_transmission.py asserts that each of them has a cell that is hit, a defined cell that is not hit (not with
# r = (0, 1): there every defined cell is hit, which it asserts instead) and a cell below min_cohort in some member.
REPRODUCTION_CASES = (
    ("fixture_a", "home", W(0, 7, 100), (1, 1), 1),
    ("situations", "group", W(0, 5, 60), (3, 2), 20),
    ("bus", "home", W(1, 3, 30), (1, 1), 5),
    ("situations", "all", W(0, 7, 48), (0, 1), 60),
    ("rollback", "home", W(0, 5, 50), (1, 1), 1),
    ("rollback", "group", W(0, 3, 70), (3, 2), 10),
)

# (world, where, settings, window, min_cases): 448, 20, 6, 35 and 25 cells.  Each has a cell hit in some members only.
H, WK, S, T = tree.H, tree.W, tree.S, tree.T
SETTINGS_CASES = (
    ("fixture_a", "home", None, W(1, 7, 100), 1),
    ("situations", "setting", None, W(5, 5, 89), 2),
    ("bus", "home", (T,), W(1, 3, 66), 25),
    ("situations", "group", (H,), W(100, 7, 50), 1),
    ("rollback", "group", None, W(150, 5, 50), 40),
)
