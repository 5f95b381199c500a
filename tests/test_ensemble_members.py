"""The rank rules and the argument checks of the ensemble quantile maps, without a GPU: the inverted-CDF rank against its
definition in exact fractions, the linear method against numpy, what Ensemble._area_kind refuses before any library call, and the
new entry points in the header and in the symbol list."""
import fractions
import os
import re

import numpy as np
import pytest

import _members_ref as ref
from epidemicsimulator_amd import Ensemble, _lib
from epidemicsimulator_amd.simulator import check_probs, interpolate_linear, linear_ranks, nearest_rank

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEMBERS = tuple(range(1, 10)) + (64, 65, 256)
PROBS = ((0.0, "0"), (0.05, "1/20"), (0.25, "1/4"), (0.5, "1/2"), (0.75, "3/4"), (0.95, "19/20"), (1.0, "1"))
NEW = ("esim_ensemble_keep_members", "esim_ensemble_members_info", "esim_ensemble_read_members", "esim_ensemble_quantiles", "esim_ensemble_exceedance")


@pytest.mark.parametrize("m", MEMBERS + (20, 40, 100))
def test_nearest_rank_is_the_inverted_cdf(m):
    for p, exact in PROBS:
        want = ref.nearest_rank(exact, m)
        assert nearest_rank(p, m) == want, (p, m)
        # the definition once more, in words: at least p * m members are <= the value at the rank, and fewer up to the one before
        frac = fractions.Fraction(exact)
        assert want + 1 >= frac * m and (want == 0 or want < frac * m)
    assert nearest_rank(0.0, m) == 0 and nearest_rank(1.0, m) == m - 1


def test_five_percent_of_twenty_members_is_the_first_of_them():
    assert 0.07 * 100 > 7                                            # (in binary the product lands above the whole number: the rank must not)
    assert nearest_rank(0.05, 20) == 0 and nearest_rank(0.95, 20) == 18 and nearest_rank(0.35, 20) == 6 and nearest_rank(0.07, 100) == 6


def linear(stack, p):
    lo, hi, frac = linear_ranks(p, stack.shape[0])
    ordered = np.sort(stack, axis=0)
    return interpolate_linear(ordered[lo], ordered[hi], frac)


@pytest.mark.parametrize("m", MEMBERS)
def test_linear_equals_numpy(m):
    rng = np.random.default_rng(m)
    for dtype, lo, hi in ((np.uint32, 0, 1 << 31), (np.uint32, 0, 7), (np.int32, -50000, 50000)):
        stack = rng.integers(lo, hi, size=(m, 5, 7)).astype(dtype)
        for p, _ in PROBS + ((0.3, None), (0.999, None)):
            got, want = linear(stack, p), ref.linear_quantile(stack, p)
            assert got.dtype == np.float64 and np.allclose(got, want, rtol=1e-12, atol=0), (m, p)
    lo, hi, frac = linear_ranks(1.0, m)
    assert lo == hi == m - 1 and frac == 0.0 and linear_ranks(0.0, m) == (0, 0, 0.0)


def test_linear_is_nan_where_a_neighbour_is_never():
    stack = np.array([[3, 3, ref.NEVER, 0], [5, ref.NEVER, ref.NEVER, 0], [ref.NEVER, ref.NEVER, ref.NEVER, 7]], np.uint32)
    got = linear(stack, 0.25)                                        # between ranks 0 and 1
    assert got[0] == 4.0 and np.isnan(got[1]) and np.isnan(got[2]) and got[3] == 0.0
    got = linear(stack, 0.5)                                         # rank 1 alone: the neighbour above does not count
    assert got[0] == 5.0 and np.isnan(got[1]) and np.isnan(got[2]) and got[3] == 0.0
    signed = np.array([[-1], [-1]], np.int32)                        # (-1 is no "never" of a signed kind)
    assert linear(signed, 0.5)[0] == -1.0


def test_probabilities_outside_the_unit_interval_are_refused():
    assert check_probs("x", (0, 0.5, 1)) == [0.0, 0.5, 1.0]
    for bad in ((1.5,), (-0.01,), (0.5, float("nan"))):
        with pytest.raises(ValueError):
            check_probs("x", bad)


def test_area_kind_refuses_before_any_library_call():
    e = Ensemble.__new__(Ensemble)                                   # no simulator, no context: nothing here may reach the library
    e.base = _lib.default_params()
    series = dict(kind="series", where="home", what="infected", first_step=1, n_rows=3, stride=1)
    kind, area = e._area_kind("run", dict(series, quantiles=(0.05, 0.5, 0.95), quantile_method="linear", exceed=(1, 5)), 10, False, 6)
    assert kind == "series" and area == {k: v for k, v in series.items() if k != "kind"}       # the begin call never sees the new keys
    assert e._keep_spec == dict(probs=[0.05, 0.5, 0.95], method="linear", thresholds=[1, 5], what="value")
    assert e._area_kind("run", series, 10, False, 6)[1] == area and e._keep_spec is None
    assert e._area_kind("run", dict(kind="peaks", where="home", quantiles=(0.5,), keep="peak_step"), 10, False, 256)[0] == "peaks" and e._keep_spec["what"] == "peak_step"
    for bad, n in ((dict(kind="reproduction", where="home", quantiles=(0.5,)), 6), (dict(kind="reproduction", where="home", exceed=(1,)), 6),
                   (dict(series, quantiles=(0.5, 1.5)), 6), (dict(series, quantiles=(0.5,)), 257), (dict(series, exceed=(1,)), 257),
                   (dict(series, quantiles=(0.5,), quantile_method="median"), 6), (dict(series, quantiles=(0.5,), keep="duration"), 6),
                   (dict(kind="peaks", where="home", keep="width"), 6)):
        with pytest.raises(ValueError):
            e._area_kind("run", bad, 10, False, n)
    assert e._area_kind("run", dict(kind="reproduction", where="home", n_rows=2), 10, False, 257)[0] == "reproduction"    # (without the keys: as before)


def test_the_entry_points_are_declared_and_listed():
    header = open(os.path.join(ROOT, "include", "esim.h")).read()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(esim_ctx \*" % name, header), name
        assert name in _lib.SYMBOLS
    assert re.search(r"#define ESIM_MEMBERS_MAX\s+256\b", header) and re.search(r"#define ESIM_RANKS_MAX\s+16\b", header)
    assert re.search(r"ESIM_KEEP_VALUE = 0, ESIM_KEEP_PEAK_STEP = 1, ESIM_KEEP_DURATION = 2", header)
    assert (_lib.MEMBERS_MAX, _lib.RANKS_MAX, _lib.KEEP_VALUE, _lib.KEEP_PEAK_STEP, _lib.KEEP_DURATION) == (256, 16, 0, 1, 2)
    engine = open(os.path.join(ROOT, "epidemicsimulator_amd", "csrc", "esim_members.h")).read()
    assert "#define MEMBERS_MAX 256u" in engine and "#define MEMBERS_RANKS_MAX 16u" in engine


def test_the_host_side_arithmetic_under_the_host_sanitizers(tmp_path):
    """tests/native/members_host_check.hip, a program of its own that opens no device: the keys, the padded sizes, the thresholds
    at the ends of both ranges and the rank lists of esim_members.h, built with AddressSanitizer and UBSan for the host side.
    Where the environment preloads a library of its own into every process, the sanitizers' runtime could not come first: the
    program is then built and run without them, and checks the same arithmetic."""
    import subprocess
    exe = str(tmp_path / "members_host_check")
    sanitize = [] if os.environ.get("LD_PRELOAD") else ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17"] + sanitize + [
           "-I", os.path.join(ROOT, "epidemicsimulator_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "native", "members_host_check.hip")]
    built = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert built.returncode == 0, built.stderr[-2000:]
    ran = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert ran.returncode == 0 and "members_host_check: ok" in ran.stdout, (ran.returncode, ran.stdout[-500:], ran.stderr[-2000:])
