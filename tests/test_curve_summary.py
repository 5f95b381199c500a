"""The numpy reference of esim_curve_summary (tests/_curve_ref.py) against a loop written as the header words the outputs, on a
ten-step example written out by hand; and what the Python binding refuses before it calls the library.  No GPU."""
import numpy as np
import pytest

import _curve_ref as ref
from epidemicsimulator_amd import Simulator
from epidemicsimulator_amd.ensemble import peaks_summary

NEVER = ref.NEVER

# x[s - 1][col], steps 1 .. 10.
#   col 0: the peak 4 is attained at steps 3 and 8 (a tie: the first one counts); 2 is reached twice, in steps 2 .. 4 and 7 .. 9
#   col 1: stays 0
#   col 2: one case from step 6 on, still there at the window's end
#   col 3: the peak at the first step, gone from step 4 on
EXAMPLE = [
    [1, 0, 0, 5],
    [2, 0, 0, 3],
    [4, 0, 0, 1],
    [3, 0, 0, 0],
    [1, 0, 0, 0],
    [0, 0, 1, 0],
    [2, 0, 1, 0],
    [4, 0, 1, 0],
    [2, 0, 1, 0],
    [1, 0, 1, 0],
]


def same(got, want, what):
    for k in ref.KEYS:
        assert got[k].dtype == want[k].dtype, (what, k)
        assert got[k].tolist() == want[k].tolist(), (what, k, got[k].tolist(), want[k].tolist())


def test_the_example_by_hand():
    got = ref.summarize(EXAMPLE, 1, 10, 2)
    assert got["peak"].tolist() == [4, 0, 1, 5]
    assert got["peak_step"].tolist() == [3, NEVER, 6, 1]                      # the tie of column 0 goes to step 3
    assert got["steps_at_least"].tolist() == [6, 0, 0, 2]                     # column 0: steps 2, 3, 4 and 7, 8, 9
    assert got["first_at_least"].tolist() == [2, NEVER, NEVER, 1]
    assert got["last_at_least"].tolist() == [9, NEVER, NEVER, 2]
    assert got["person_steps"].tolist() == [20, 0, 5, 9]
    assert got["person_steps"].dtype == np.uint64 and got["peak"].dtype == np.uint32


@pytest.mark.parametrize("first, last", [(1, 10), (4, 10), (1, 5), (4, 7), (8, 8), (6, 6), (10, 10)])
@pytest.mark.parametrize("threshold", [1, 2, 4, 6])
def test_the_reference_against_the_loop(first, last, threshold):
    same(ref.summarize(EXAMPLE, first, last, threshold), ref.brute_force(EXAMPLE, first, last, threshold), (first, last, threshold))


def test_random_curves_against_the_loop():
    rng = np.random.default_rng(11)
    x = rng.integers(0, 6, size=(40, 9)) * (rng.random((40, 9)) < 0.6)
    x[:, 4] = 0
    for first, last, threshold in ((1, 40, 1), (7, 33, 3), (20, 20, 5), (1, 40, 9)):
        same(ref.summarize(x, first, last, threshold), ref.brute_force(x.tolist(), first, last, threshold), (first, last, threshold))


def test_the_fold_of_the_example_and_its_summary():
    a, b = ref.summarize(EXAMPLE, 1, 10, 2), ref.summarize(EXAMPLE, 4, 10, 2)
    acc = ref.fold([a, b], min_peak=4)
    assert acc["members"] == 2
    assert acc["defined"].tolist() == [2, 0, 2, 1] and acc["hit"].tolist() == [2, 0, 0, 1]
    assert acc["sum_peak"].tolist() == [8, 0, 2, 5] and acc["sumsq_peak"].tolist() == [32, 0, 2, 25]
    assert acc["sum_step"].tolist() == [3 + 8, 0, 12, 1] and acc["sumsq_step"].tolist() == [9 + 64, 0, 72, 1]
    assert acc["sum_duration"].tolist() == [6 + 4, 0, 0, 2]
    s = peaks_summary(acc)
    assert s["members"] == 2 and s["p_peak"].tolist() == [1.0, 0.0, 0.0, 0.5]
    assert s["peak_mean"].tolist() == [4.0, 0.0, 1.0, 2.5] and s["peak_var"].tolist() == [0.0, 0.0, 0.0, 6.25]
    assert s["peak_step_mean"][0] == 5.5 and s["peak_step_var"][0] == 6.25 and np.isnan(s["peak_step_mean"][1]) and s["peak_step_mean"][3] == 1.0
    assert s["duration_mean"].tolist() == [5.0, 0.0, 0.0, 1.0] and s["duration_var"].tolist() == [1.0, 0.0, 0.0, 1.0]


def test_the_binding_refuses_a_bad_status_before_any_library_call():
    sim = object.__new__(Simulator)                 # no context, no library: a call into it would raise something else
    for method in (Simulator.curve_summary, Simulator.ensemble_begin_peaks):
        for status in ("recovered", "susceptible", 2, None):
            with pytest.raises(ValueError, match="status must be"):
                method(sim, status=status)
