"""The curve-based ensemble statistics without a GPU: the counting rule of the depth against enumeration of all pairs, what the
central region does with ties, the Python wrappers against the call recorder of test_marshalling.py, the keys of the area dict,
and the two entry points in the header, in the library and in the bindings."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _depth_ref as ref
from _members_ref import NEVER, to_key
from epidemicsimulator_amd import Ensemble, _lib
from test_marshalling import KEPT, bare_simulator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("esim_ensemble_depth", "esim_ensemble_band")
KEYS = np.array([0, 1, 1, 2, 7, 400, NEVER], np.uint32)


# ---- the restatement ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", (1, 2, 3, 7, 9))
def test_the_counting_rule_equals_enumeration_of_all_pairs(m):
    rng = np.random.default_rng(m)
    stack = rng.choice(KEYS, size=(m, 6, 11))
    assert (np.sort(stack, axis=0)[:-1] == np.sort(stack, axis=0)[1:]).any() or m == 1          # ties are everywhere
    got, want = ref.depth(stack), ref.brute_depth(stack)
    assert got.dtype == np.uint64 and (got == want).all()
    assert (ref.total(stack) == want.sum(axis=1)).all()
    if m == 1:
        assert not got.any()
    else:
        assert got.min() >= 6 * (m - 1) and got.max() <= 6 * ref.pairs(m)          # a member's own pairs always hold it
    signed = rng.integers(-3, 4, size=(m, 6, 11)).astype(np.int32)
    assert (ref.depth(signed) == ref.brute_depth(signed)).all() and (ref.depth(to_key(signed)) == ref.depth(signed)).all()


STACK = np.array([[[0, 4], [0, 4]],            # member 0: the lowest in column 0, in the middle of column 1
                  [[3, 0], [3, 0]],            # 1 and 2 tie for the deepest of column 0 ...
                  [[3, 9], [3, 9]],
                  [[9, 4], [9, 5]],            # 3: the highest in column 0, central in column 1
                  [[5, 4], [5, 4]]], np.uint32)   # 4: ties with 0 in column 1


def test_ties_at_the_threshold_are_all_in_and_the_lowest_index_is_the_deepest():
    d = ref.depth(STACK)
    assert (d == ref.brute_depth(STACK)).all()
    assert d[1, 0] == d[2, 0] == d[:, 0].max()
    one = ref.band(STACK, 1, False)
    assert one["deepest"].tolist() == [1, 0] and (one["n_in"] > 1).all()                          # n_in > need: every tie is in
    assert one["n_in"].tolist() == [2, 2] and one["inside"][:, 0].tolist() == [False, True, True, False, False]
    assert one["lo"][:, 0].tolist() == [3, 3] and one["hi"][:, 0].tolist() == [3, 3] and (one["median"][:, 0] == 3).all()
    assert (ref.band(STACK, 5, False)["lo"] == STACK.min(axis=0)).all() and (ref.band(STACK, 5, False)["hi"] == STACK.max(axis=0)).all()
    pooled = ref.band(STACK, 1, True)
    assert (pooled["deepest"] == pooled["deepest"][0]).all() and (pooled["n_in"] == pooled["n_in"][0]).all()
    assert pooled["deepest"][0] == int(np.argmax(ref.total(STACK)))
    assert pooled["deepest"].tolist() != one["deepest"].tolist()                                  # pooled and per column differ here
    assert (pooled["median"] == STACK[pooled["deepest"][0]]).all()                                # one real member, every column
    for need in range(1, 6):
        for p in (False, True):
            b = ref.band(STACK, need, p)
            assert (b["n_in"] >= need).all() and (b["lo"] <= b["median"]).all() and (b["median"] <= b["hi"]).all()


# ---- the wrappers against the call recorder -----------------------------------------------------------------------------------------
def test_the_wrappers_make_the_recorded_calls_and_return_the_stated_shapes():
    sim = bare_simulator(0, 100)
    sim.ensemble_begin_series("home", "infected", first_step=1, n_rows=5)
    del sim.lib.calls[:]
    d = sim.ensemble_depth()
    assert sim.lib.calls == ["ensemble_members_info(&u32,&u32,&i32,&i32)", "ensemble_depth(0,5,*u32,*u64)"]
    assert d["depth"].dtype == np.uint32 and d["depth"].shape == (KEPT, 3) and d["total"].dtype == np.uint64 and d["total"].shape == (KEPT,)
    assert d["pairs"] == KEPT * (KEPT - 1) // 2 == 780 and d["rows"] == 5 and d["mbd"].dtype == np.float64 and d["mbd"].shape == (KEPT, 3)
    del sim.lib.calls[:]
    assert sim.ensemble_depth(first_row=1, n_rows=2)["rows"] == 2 and sim.lib.calls[-1] == "ensemble_depth(1,2,*u32,*u64)"
    assert np.isnan(sim.ensemble_depth(first_row=5)["mbd"]).all()                                # no rows: 0 / 0
    del sim.lib.calls[:]
    b = sim.ensemble_band()
    assert sim.lib.calls == ["ensemble_members_info(&u32,&u32,&i32,&i32)", "ensemble_band(0,5,20,0,*u32,*u32,*u32,*u32,*u32)"]
    assert sorted(b) == ["deepest", "hi", "lo", "median", "n_in", "need"] and b["need"] == 20
    for k in ("lo", "hi", "median"):
        assert b[k].dtype == np.uint32 and b[k].shape == (5, 3), k
    for k in ("deepest", "n_in"):
        assert b[k].dtype == np.uint32 and b[k].shape == (3,), k
    del sim.lib.calls[:]
    sim.ensemble_band(0.9, pooled=True, first_row=2, n_rows=3)
    assert sim.lib.calls[-1] == "ensemble_band(2,3,36,1,*u32,*u32,*u32,*u32,*u32)"
    sim.ensemble_band(0.9, need=7)
    assert sim.lib.calls[-1] == "ensemble_band(0,5,7,0,*u32,*u32,*u32,*u32,*u32)"                 # an explicit need overrides the coverage


def test_a_signed_store_comes_back_as_int32_planes():
    sim = bare_simulator(0, 100, signed=1)
    sim.ensemble_begin_paired("all", first_step=0, n_rows=4, stride=24)
    b = sim.ensemble_band(pooled=True)
    for k in ("lo", "hi", "median"):
        assert b[k].dtype == np.int32 and b[k].shape == (4, 1), k
    assert b["deepest"].dtype == np.uint32 and b["n_in"].dtype == np.uint32 and sim.ensemble_depth()["depth"].dtype == np.uint32


@pytest.mark.parametrize("kept, needs", ((40, (1, 20, 40)), (9, (1, 5, 9))))
def test_need_is_the_ceiling_of_the_coverage_in_exact_fractions(kept, needs):
    sim = bare_simulator(0, 100)
    sim.lib.writes["esim_ensemble_members_info"] = (64, kept, 0, 0)
    sim.ensemble_begin("home")
    assert tuple(sim.ensemble_band(c)["need"] for c in (0, 0.5, 1)) == needs
    assert sim.ensemble_band(0.05)["need"] == (2 if kept == 40 else 1) and sim.ensemble_band(0.35)["need"] == (14 if kept == 40 else 4)   # 0.35 * 40 is 14, not the 15 of binary
    del sim.lib.calls[:]
    for bad in (1.5, -0.1, float("nan")):
        with pytest.raises(ValueError):
            sim.ensemble_band(bad)
    assert not any(c.startswith("ensemble_band") for c in sim.lib.calls)


# ---- the keys of the area dict --------------------------------------------------------------------------------------------------------
def test_keep_spec_takes_the_band_keys_out_and_refuses_them_for_the_reproduction_kind():
    e = Ensemble.__new__(Ensemble)                                   # no simulator, no context: nothing here may reach the library
    e.base = _lib.default_params()
    series = dict(kind="series", where="home", what="infected", first_step=1, n_rows=3, stride=1)
    want = {k: v for k, v in series.items() if k != "kind"}
    kind, area = e._area_kind("run", dict(series, band=0.5, band_pooled=True), 10, False, 6)
    assert kind == "series" and area == want                         # the begin call never sees the new keys
    assert e._keep_spec["band"] == 0.5 and e._keep_spec["band_pooled"] is True and e._keep_spec["band_only"] and e._keep_spec["what"] == "value"
    assert e._area_kind("run", dict(series, band=0.9, quantiles=(0.5,)), 10, False, 6)[1] == want
    assert e._keep_spec["band"] == 0.9 and e._keep_spec["band_pooled"] is False and not e._keep_spec["band_only"] and e._keep_spec["probs"] == [0.5]
    assert e._area_kind("run", dict(series, quantiles=(0.5,)), 10, False, 6)[1] == want and "band" not in e._keep_spec       # without the keys: as before
    for bad, n in ((dict(kind="reproduction", where="home", band=0.5), 6), (dict(kind="reproduction", where="home", band_pooled=True), 6),
                   (dict(series, band=1.5), 6), (dict(series, band=-0.5), 6), (dict(series, band=0.5), 257)):
        with pytest.raises(ValueError) as err:
            e._area_kind("run", bad, 10, False, n)
        if bad.get("kind") == "reproduction":
            assert "the reproduction kind keeps no members" in str(err.value)      # the words of the other keys


# ---- the entry points -----------------------------------------------------------------------------------------------------------------
def test_the_entry_points_are_declared_exported_and_bound_with_the_headers_arity():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "esim.h")).read(), flags=re.S)
    lib = _lib.load()
    raw = C.CDLL(os.path.join(ROOT, "epidemicsimulator_amd", "libesim.so"))
    for name in NEW:
        proto = re.search(r"\bint\s+%s\s*\((esim_ctx \*.*?)\);" % name, header, re.S)
        assert proto, name
        assert name in _lib.SYMBOLS and hasattr(raw, name)
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == len(proto.group(1).split(",")), name
    assert lib.esim_ensemble_depth.argtypes[3:] == [C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
    assert lib.esim_ensemble_band.argtypes[1:5] == [C.c_uint32, C.c_uint32, C.c_uint32, C.c_int]
    csrc = os.path.join(ROOT, "epidemicsimulator_amd", "csrc")
    engine = open(os.path.join(csrc, "esim_depth.h")).read()
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', engine) == ["esim_members.h"]              # a probe can compile it alone
    assert '#include "esim_host_depth.h"' in open(os.path.join(csrc, "esim_api.hip")).read()
    make = open(os.path.join(csrc, "Makefile")).read()
    assert "esim_host_depth.h" in make and "esim_depth.h" in make.replace("esim_host_depth.h", "")
