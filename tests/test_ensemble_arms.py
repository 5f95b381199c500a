"""Policy grids without a GPU: the numpy reference pinned by a hand-worked example, arms_summary on its tables, the Python
wrapper against the call recorder of test_marshalling.py, the entry point in the header, the library and the bindings, the
refusals of Ensemble.grid that need no context, and the new kernel header compiled on its own for gfx950, where its kernels may
use no scratch memory."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import _arms_ref as ref
from epidemicsimulator_amd import Ensemble, _lib
from epidemicsimulator_amd import ensemble as ensemble_module
from epidemicsimulator_amd.ensemble import GridResult, arms_summary
from test_marshalling import KEPT, bare_simulator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "epidemicsimulator_amd", "csrc")
N = ref.NEVER

# 3 arms x 2 replicates x 4 cells, slot = replicate * 3 + arm.  Cell 0: two arms tie for best in replicate 0; cell 1: all arms
# equal in replicate 0; cell 2: ESIM_NEVER in three slots; cell 3: nothing special.
X = np.array([[5, 7, N, 9],
              [5, 7, 10, 2],
              [8, 7, 30, 4],
              [1, 3, N, 6],
              [2, 3, N, 6],
              [0, 9, 20, 1]], np.uint32)


def as_lists(t):
    return {k: np.asarray(t[k]).tolist() for k in ref.KEYS}


# ---- the reference itself -----------------------------------------------------------------------------------------------------------------
def test_the_reference_is_the_definition():
    got = as_lists(ref.arms(X, 3))
    assert got["best"] == [[1, 2, 0, 0], [1, 2, 1, 1], [1, 1, 1, 1]]
    assert got["sole"] == [[0, 0, 0, 0], [0, 0, 1, 1], [1, 0, 1, 1]]
    assert got["regret"] == [[1, 0, 2 * N - 30, 12], [2, 0, N - 20, 5], [3, 6, 20, 2]]
    assert got["sum"] == [[6, 10, 2 * N, 15], [7, 10, 10 + N, 8], [8, 16, 50, 5]]
    assert got["totals"] == [[21 + N, 24, 49], [10 + N, 11 + N, 30]]
    # ESIM_NEVER as 15: only cell 2 changes -- replicate 1 now has a tie between arms 0 and 1
    got = as_lists(ref.arms(X, 3, never_as=15))
    assert [row[2] for row in got["best"]] == [1, 2, 0] and [row[2] for row in got["sole"]] == [0, 1, 0]
    assert [row[2] for row in got["regret"]] == [5, 0, 25] and [row[2] for row in got["sum"]] == [30, 25, 50]
    assert got["totals"] == [[36, 24, 49], [25, 26, 30]]
    assert all(got[k] == as_lists(ref.arms(np.where(X == N, np.uint32(15), X), 3))[k] for k in ref.KEYS)
    # a store that cannot hold ESIM_NEVER ignores never_as; never_as = ESIM_NEVER leaves the keys as they are
    plain = as_lists(ref.arms(X, 3))
    assert as_lists(ref.arms(X, 3, never_as=15, has_never=False)) == plain and as_lists(ref.arms(X, 3, never_as=N)) == plain
    # the largest is the best
    got = as_lists(ref.arms(X, 3, maximize=True))
    assert got["best"] == [[0, 1, 2, 2], [1, 1, 1, 1], [1, 2, 0, 0]]
    assert got["sole"] == [[0, 0, 1, 1], [1, 0, 0, 0], [1, 1, 0, 0]]
    assert got["regret"] == [[4, 6, 0, 0], [3, 6, N - 10, 7], [2, 0, 2 * N - 50, 10]]
    assert got["sum"] == plain["sum"] and got["totals"] == plain["totals"]
    # one arm: best = sole = S, no regret; the arms of a cell: sole <= best, the soles sum to at most S
    one = ref.arms(X, 1)
    assert (one["best"] == 6).all() and (one["sole"] == 6).all() and not one["regret"].any() and one["totals"].shape == (6, 1)
    for maximize in (False, True):
        t = ref.arms(X, 3, maximize)
        assert (t["sole"] <= t["best"]).all() and (t["sole"].sum(axis=0) <= 2).all() and (t["best"].sum(axis=0) >= 2).all()
    # planes over rows and columns keep their shape
    t = ref.arms(X.reshape(6, 2, 2), 2)
    assert t["best"].shape == (2, 2, 2) and t["regret"].dtype == np.uint64 and t["totals"].shape == (3, 2)
    assert ref.live_cells(np.array([0, 1, 2, 0], np.uint64), np.array([1, 0, 3, 3], np.uint32), 1, 3) == 1


# ---- arms_summary -------------------------------------------------------------------------------------------------------------------------
def test_arms_summary_on_the_hand_worked_tables():
    t = ref.arms(X, 3, never_as=15)
    got = arms_summary(t)
    assert got["replicates"] == 2 and got["n_arms"] == 3 and got["maximize"] is False
    assert got["p_best"].tolist() == [[0.5, 1.0, 0.5, 0.0], [0.5, 1.0, 1.0, 0.5], [0.5, 0.5, 0.0, 0.5]]
    assert got["p_sole"].tolist() == [[0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.5, 0.5], [0.5, 0.0, 0.0, 0.5]]
    assert got["expected_regret"].tolist() == [[0.5, 0.0, 2.5, 6.0], [1.0, 0.0, 0.0, 2.5], [1.5, 3.0, 12.5, 1.0]]
    assert got["mean"].tolist() == [[3.0, 5.0, 15.0, 7.5], [3.5, 5.0, 12.5, 4.0], [4.0, 8.0, 25.0, 2.5]]
    assert all(got[k].dtype == np.float64 for k in ensemble_module.ARMS_CELL_KEYS)
    # the whole window: totals [[36, 24, 49], [25, 26, 30]] -- arm 1 wins replicate 0, arm 0 replicate 1
    assert got["overall_p_best"].tolist() == [0.5, 0.5, 0.0] and got["overall_p_sole"].tolist() == [0.5, 0.5, 0.0]
    assert got["overall_regret"].tolist() == [6.0, 0.5, 15.0] and got["overall_mean"].tolist() == [30.5, 25.0, 39.5]
    assert got["overall_choice"] == 1
    # the largest total is the best: arm 2 in both replicates
    up = arms_summary(dict(ref.arms(X, 3, True, 15), maximize=True))
    assert up["maximize"] is True and up["overall_p_best"].tolist() == [0.0, 0.0, 1.0] and up["overall_regret"].tolist() == [9.0, 14.5, 0.0] and up["overall_choice"] == 2
    # a tie of the regrets goes to the smallest index, and a tie within a replicate is nobody's sole win
    tie = dict(t, totals=np.array([[1, 1, 5], [3, 3, 9]], np.uint64))
    got = arms_summary(tie)
    assert got["overall_choice"] == 0 and got["overall_regret"].tolist() == [0.0, 0.0, 5.0]
    assert got["overall_p_best"].tolist() == [1.0, 1.0, 0.0] and got["overall_p_sole"].tolist() == [0.0, 0.0, 0.0]
    tie = dict(t, totals=np.array([[4, 2, 2], [1, 3, 3]], np.uint64))       # regrets 2, 2, 2
    assert arms_summary(tie)["overall_choice"] == 0 and arms_summary(tie)["overall_regret"].tolist() == [1.0, 1.0, 1.0]
    # sums beyond 2^53 are compared exactly before they are divided
    big = dict(t, totals=np.array([[(1 << 63) + 1, 1 << 63, (1 << 63) + 2]], np.uint64))
    got = arms_summary(big)
    assert got["overall_choice"] == 1 and got["overall_p_sole"].tolist() == [0.0, 1.0, 0.0] and got["overall_regret"].tolist() == [1.0, 0.0, 2.0]


# ---- the wrapper against the call recorder ------------------------------------------------------------------------------------------------
def test_the_wrapper_makes_the_recorded_calls_and_returns_the_stated_shapes():
    sim = bare_simulator(0, 100)
    sim.ensemble_begin_series("home", "infected", first_step=1, n_rows=5)
    del sim.lib.calls[:]
    t = sim.ensemble_arms(4)
    assert sim.lib.calls == ["ensemble_members_info(&u32,&u32,&i32,&i32)", "ensemble_arms(4,0,4294967295,0,5,*u32,*u32,*u64,*u64,*u64,&u64)"]
    assert sorted(t) == ["best", "live_cells", "maximize", "regret", "replicates", "sole", "sum", "totals"]
    assert all(t[k].shape == (4, 5, 3) for k in ("best", "sole", "regret", "sum")) and t["totals"].shape == (KEPT // 4, 4)
    assert t["best"].dtype == t["sole"].dtype == np.uint32 and t["regret"].dtype == t["sum"].dtype == t["totals"].dtype == np.uint64
    assert isinstance(t["live_cells"], int) and t["replicates"] == KEPT // 4 and t["maximize"] is False
    t = sim.ensemble_arms(8, maximize=True, never_as=120, first_row=1, n_rows=2)
    assert sim.lib.calls[-1] == "ensemble_arms(8,1,120,1,2,*u32,*u32,*u64,*u64,*u64,&u64)" and t["best"].shape == (8, 2, 3) and t["maximize"] is True
    sim.ensemble_arms(3)                                            # 40 members are no replicates of 3 arms: the library's refusal, no totals
    assert sim.lib.calls[-1] == "ensemble_arms(3,0,4294967295,0,5,*u32,*u32,*u64,*u64,-,&u64)"
    sim.ensemble_begin("home")                                      # a kind without rows: one row, as ensemble_quantiles
    assert sim.ensemble_arms(2)["sum"].shape == (2, 1, 3)


# ---- the entry point and the header ---------------------------------------------------------------------------------------------------------
def test_the_entry_point_is_declared_exported_and_bound_with_the_headers_arity():
    text = open(os.path.join(ROOT, "include", "esim.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"#define\s+ESIM_ARMS_MAX\s+16\b", header) and _lib.ARMS_MAX == 16
    lib = _lib.load()
    raw = C.CDLL(os.path.join(ROOT, "epidemicsimulator_amd", "libesim.so"))
    proto = re.search(r"\bint\s+esim_ensemble_arms\s*\((esim_ctx \*.*?)\);", header, re.S)
    assert proto and "esim_ensemble_arms" in _lib.SYMBOLS and hasattr(raw, "esim_ensemble_arms")
    fn = lib.esim_ensemble_arms
    u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    assert fn.restype is C.c_int and len(fn.argtypes) == len(proto.group(1).split(",")) == 12
    assert fn.argtypes[1:] == [C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, u32p, u32p, u64p, u64p, u64p, u64p]
    engine = open(os.path.join(CSRC, "esim_arms.h")).read()
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', engine) == ["esim_members.h"]                # a probe can compile it alone
    probe = open(os.path.join(ROOT, "tests", "native", "arms_probe.hip")).read()
    assert re.findall(r'#include\s+"([^"]+)"', probe) == ["esim_arms.h"]
    assert '#include "esim_host_arms.h"' in open(os.path.join(CSRC, "esim_api.hip")).read()
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert "esim_host_arms.h" in make and "esim_arms.h" in make.replace("esim_host_arms.h", "")
    assert ensemble_module.arms_summary is arms_summary and ensemble_module.GridResult is GridResult and hasattr(Ensemble, "grid")


# ---- Ensemble.grid: what is refused before anything runs -----------------------------------------------------------------------------------
def test_grid_refuses_before_anything_runs():
    e = Ensemble.__new__(Ensemble)                                   # no simulator, no context: nothing here may reach the library
    e.base = _lib.default_params()
    census = dict(where="home")
    two = [dict(mask_effectiveness=0.5), dict(mask_effectiveness=0.9)]
    seeds = Ensemble.seeds(3)
    bad = [
        dict(policies=two, members=Ensemble.seeds(129), n_steps=10, area=census),                           # 258 runs
        dict(policies=[dict(seed=i) for i in range(17)], members=seeds, n_steps=10, area=census),           # 17 arms
        dict(policies=[], members=seeds, n_steps=10, area=census),
        dict(policies=[dict(index_cases=[1, 2])] + two, members=seeds, n_steps=10, area=census),            # the index cases belong to the member
        dict(policies=two, members=seeds, n_steps=10, history_steps=0, area=census),
        dict(policies=two, members=seeds, n_steps=10, history_steps=11, area=census),
        dict(policies=two, members=[dict(seed=1, index_cases=[3])], n_steps=10, history_steps=5, area=census),
        dict(policies=two + [dict(infected_time=30)], members=seeds, n_steps=10, history_steps=5, area=census),
        dict(policies=[dict(start_hour=7)], members=seeds, n_steps=10, history_steps=5, area=census),
        dict(policies=two, members=seeds, n_steps=10, area=dict(kind="reproduction", where="home")),
        dict(policies=two, members=seeds, n_steps=10, area=dict(kind="bogus")),
        dict(policies=two, members=seeds, n_steps=10),                                                       # no area
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            e.grid(**kw)
    with pytest.raises(ValueError) as err:
        e.grid(two, Ensemble.seeds(129), 10, area=census)
    assert "258 runs" in str(err.value)
    with pytest.raises(ValueError) as err:
        e.grid(two, seeds, 10, area=dict(kind="reproduction", where="home"))
    assert "the reproduction kind keeps no members" in str(err.value)
    assert not hasattr(e, "simulator")


# ---- the kernel header alone ----------------------------------------------------------------------------------------------------------------
def test_the_header_compiles_alone_for_gfx950_and_its_kernels_use_no_scratch(tmp_path):
    """The resource query of test_kernel_resources.py on the probe, which includes esim_arms.h and nothing else of the library."""
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-fast-math", "-ffp-contract=off", "--cuda-device-only",
           "-Rpass-analysis=kernel-resource-usage", "-I", CSRC, "-c", "-o", str(tmp_path / "k.o"), os.path.join(ROOT, "tests", "native", "arms_probe.hip")]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    kernels, cur = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            kernels[cur] = {}
            continue
        m = re.search(r"remark:\s+([\w \[\]/]+): (\d+)", line)
        if m and cur:
            kernels[cur][m.group(1).strip()] = int(m.group(2))
    arms = {k: v for k, v in kernels.items() if "k_arms" in k}
    assert len(arms) == 4, sorted(kernels)                           # the arms padded to 2, 4, 8 and 16
    for name, r in arms.items():
        assert r.get("ScratchSize [bytes/lane]", 0) == 0, "%s uses %d bytes of scratch per lane" % (name, r["ScratchSize [bytes/lane]"])
        assert r.get("VGPRs Spill", 0) == 0 and r["VGPRs"] <= 128 and r["LDS Size [bytes/block]"] == 8 * 256, (name, r)
