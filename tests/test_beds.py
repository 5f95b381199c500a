"""The parts of the admitted-case list that need no GPU: the ABI's new exports declared and bound, every kernel launch of
esim_host_beds.h clamped by ESIM_GRID_CAP or listed as an exact cover, the family's kernels launched from that file alone, and the
reference module's counts of its three pairs (tests/_beds_ref.py asserts them as it builds a pair)."""
import os
import re

import numpy as np

import _beds_ref as beds
import _burden_ref as ref
from epidemicsimulator_amd import Simulator, _lib
from test_launch_sites import CSRC, ROOT, is_clamped, launches

NEW_EXPORTS = ("esim_burden_baseline_keep", "esim_burden_baseline_info", "esim_burden_baseline_drop", "esim_burden_baseline_read", "esim_burden_compare",
               "esim_burden_compare_series", "esim_ensemble_begin_burden_series", "esim_ensemble_begin_burden_paired")
# (kernel) -> why its grid is not clamped: launches whose grid covers the items exactly.
EXACT_COVER = {"k_series_prefix": "a lane per column, no loop (grid_for without a cap)"}


def test_the_new_exports_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "esim.h")).read()
    source = open(os.path.join(os.path.dirname(_lib.__file__), "_lib.py")).read()
    for name in NEW_EXPORTS:
        assert re.search(r"^int\s+%s\(" % name, header, re.M), name
        assert name in _lib.SYMBOLS and '"%s": (C.c_int' % name in source, name
    # the pairing property is part of the contract
    assert "keyed by (citizen, onset)" in header and "variance is reduced only for the cases whose onset does not move" in header
    for method in ("keep_burden_baseline", "burden_baseline_info", "drop_burden_baseline", "burden_baseline_cases", "burden_compare", "burden_compare_series",
                   "ensemble_begin_burden_series", "ensemble_begin_burden_paired"):
        assert callable(getattr(Simulator, method)), method


def test_every_launch_of_the_beds_host_file_is_clamped_or_an_exact_cover():
    seen, used, kernels = [], set(), []
    for kernel, grid, before in launches("esim_host_beds.h"):
        kernels.append(kernel)
        if is_clamped(grid, before):
            assert kernel not in EXACT_COVER, kernel
        elif kernel in EXACT_COVER:
            used.add(kernel)
        else:
            seen.append("%s with grid `%s`" % (kernel, grid))
    assert not seen, "launches that neither go through grid_capped / grid_clamp nor are listed as exact covers:\n" + "\n".join(seen)
    assert sorted(used) == sorted(EXACT_COVER)
    assert sorted(set(kernels)) == ["k_beds_collect", "k_beds_rows", "k_beds_totals", "k_ensemble_fold_paired", "k_ensemble_fold_rows", "k_series_prefix"]
    # the family's kernels are launched from this file alone, and it launches none of the burden family's
    for name in sorted(os.listdir(CSRC)):
        if name.startswith("esim_host_") and name != "esim_host_beds.h":
            assert not [k for k, _, _ in launches(name) if k.startswith("k_beds_")], name
    assert not [k for k in kernels if k.startswith("k_burden_")]
    # the consumers of a list draw nothing and stage nothing: the Philox block and the tables appear in the collecting kernel only
    text = open(os.path.join(CSRC, "esim_kernels_beds.h")).read()
    for kernel in ("k_beds_rows", "k_beds_totals"):
        body = text[text.index("void %s(" % kernel):]
        body = body[:body.index("\n}\n")]
        assert "burden_outcome" not in body and "burden_stage" not in body and "philox" not in body and "vax_step" not in body, kernel


def test_the_reference_counts_of_the_three_pairs():
    """The module asserts the issue's tables as it builds a pair; here what the GPU tests rely on beside them."""
    for name, make in beds.PAIRS.items():
        base, policy = make()
        assert base["pop"] is policy["pop"] and base["n_steps"] == policy["n_steps"], name
    base, policy = beds.pair_a()
    b, p = beds.cases(ref.at_stop(base["full"], 700)), beds.cases(ref.at_stop(policy["full"], 700))
    at = np.searchsorted(b["citizen"], p["citizen"])
    assert len(b["citizen"]) == 152 and len(p["citizen"]) == 137 and (b["citizen"][at] == p["citizen"]).all()          # a subset ...
    assert (b["admit_step"][at] == p["admit_step"]).all() and (b["end_step"][at] == p["end_step"]).all()                  # ... with identical stays
    assert (np.diff(b["citizen"].astype(np.int64)) > 0).all() and int(b["died"].sum()) == 42
    # a baseline kept at step 96 (the four admitted index cases): ends beyond its run are in the list; at step 120 admissions too
    early, later = beds.cases(ref.at_stop(base["full"], 96)), beds.cases(ref.at_stop(base["full"], 120))
    assert len(early["citizen"]) == 4 and (early["end_step"] > 96).sum() == 3 and (early["admit_step"] <= 96).all()
    assert len(later["citizen"]) == 10 and (later["admit_step"] > 120).any() and (later["end_step"] > 120).any()
    # the seed pair: equal admission totals, no stay shared
    base, policy = beds.pair_w2_seed()
    assert beds.overlap(base, policy)["other_stay"] == beds.overlap(base, policy)["admitted_both"] == 222


def test_the_reference_totals_equal_its_own_rows_summed():
    for make, n in ((beds.pair_a, 700), (beds.pair_w2, 900)):
        for world in make():
            o = ref.at_stop(world["full"], n)
            for where in ref.WHERES:
                lab, n_cols = world["cols"][where]
                for first, last in ((1, n), (200, 500), (n, n)):
                    t = beds.totals(o, lab, n_cols, n, first, last)
                    k = last - first + 1
                    assert (t["bed_steps"] == beds.rows(o, "occupancy", lab, n_cols, n, first, k).sum(axis=0, dtype=np.uint64)).all(), (where, first, last)
                    for what in ("admissions", "deaths"):
                        x = beds.rows(o, what, lab, n_cols, n, first, k)
                        assert (t[what] == x.sum(axis=0, dtype=np.uint32)).all(), (what, where, first, last)
                        assert (beds.rows(o, what, lab, n_cols, n, first, k, cumulative=True)[-1] == t[what]).all()
    # the accumulators of the two kinds over two members, by hand
    a, b = np.array([[3, 0], [5, 2]], np.uint32), np.array([[1, 0], [9, 2]], np.uint32)
    f = beds.fold_rows([a, b], 3)
    assert f["hit"].tolist() == [[1, 0], [2, 0]] and f["sum"].tolist() == [[4, 0], [14, 4]] and f["sumsq"].tolist() == [[10, 0], [106, 8]]
    p = beds.fold_paired([(a, b), (b, a)], 2, 2)
    assert p["defined"].tolist() == [[1, 0], [2, 2]] and p["hit"].tolist() == [[1, 0], [1, 0]] and p["sum_cross"].tolist() == [[6, 0], [90, 8]]
