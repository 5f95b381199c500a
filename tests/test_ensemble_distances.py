"""Ensemble distances without a GPU: medoids against brute force over every set of medoids, the keys of the area dict, the Python
wrapper against the call recorder of test_marshalling.py, the entry points in the header, the library and the bindings, and the
new kernel header compiled on its own for gfx950, where its kernels may use no scratch memory."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import _dist_ref as ref
from epidemicsimulator_amd import Ensemble, _lib
from epidemicsimulator_amd.ensemble import medoids
from test_marshalling import KEPT, bare_simulator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "epidemicsimulator_amd", "csrc")
NEW = ("esim_ensemble_distances", "esim_ensemble_distances_info")


# ---- the reference itself -----------------------------------------------------------------------------------------------------------------
def test_the_reference_is_the_definition():
    x = np.array([[0, 5, 0xFFFFFFFF, 7], [3, 5, 2, 0xFFFFFFFF], [0, 0, 0xFFFFFFFF, 7]], np.uint32)
    assert ref.distances(x, "l1").tolist() == [[0, 3 + 0xFFFFFFFD + 0xFFFFFFF8, 5], [3 + 0xFFFFFFFD + 0xFFFFFFF8, 0, 3 + 5 + 0xFFFFFFFD + 0xFFFFFFF8], [5, 3 + 5 + 0xFFFFFFFD + 0xFFFFFFF8, 0]]
    assert ref.distances(x, "differ").tolist() == [[0, 3, 1], [3, 0, 4], [1, 4, 0]]
    assert ref.distances(x, "l1", 10).tolist() == [[0, 3 + 8 + 3, 5], [14, 0, 3 + 5 + 8 + 3], [5, 19, 0]]
    assert ref.distances(x, "differ", 7)[0, 1] == 2                 # 7 against ESIM_NEVER as 7: the same
    signed = np.array([[-3, 4], [2, -(1 << 31)]], np.int32)
    assert ref.distances(signed, "l1")[0, 1] == 5 + 4 + (1 << 31)
    assert ref.live_cells(np.array([0, 1, 2, 0], np.uint64), np.array([1, 0, 3, 3], np.uint32), 1, 3) == 1


# ---- medoids ------------------------------------------------------------------------------------------------------------------------------
def swaps_of(medoid, m):
    for p in range(len(medoid)):
        for h in range(m):
            if h not in medoid:
                yield medoid[:p] + [h] + medoid[p + 1:]


@pytest.mark.parametrize("m", range(1, 9))
def test_medoids_against_brute_force_over_every_set_of_medoids(m):
    """PAM ends in a set of medoids that no single swap improves; that is all the algorithm promises, so the comparison with the
    best of all C(M, k) sets is: never below it, equal to it for k = 1 (BUILD's first step is the optimum), for k = M (cost 0)
    and for M - 1 (a swap reaches every set from every other), and never improved by one swap for any k."""
    rng = np.random.default_rng(m)
    for trial in range(6):
        if trial % 2:
            d = ref.distances(rng.integers(0, 40, size=(m, 5)).astype(np.uint32), "l1")
        else:
            d = ref.distances(rng.choice(np.array([0, 1, 0xFFFFFFFE], np.uint32), size=(m, 4)), "l1")          # many ties, sums beyond 32 bits
        for k in range(1, m + 1):
            got = medoids(d, k)
            best = ref.best_medoids(d, k)
            med = got["medoid"].tolist()
            assert med == sorted(set(med)) and len(med) == k and got["medoid"].dtype == np.int64
            cost, _ = ref.cost_of(d, med)
            assert got["cost"] == cost >= best and isinstance(got["cost"], int)
            if k in (1, m - 1, m):
                assert cost == best, (m, k, trial)
            assert all(ref.cost_of(d, s)[0] >= cost for s in swaps_of(med, m)), (m, k, trial)
            label = got["label"]
            assert label.shape == (m,) and (label[med] == np.arange(k)).all() and (got["size"] == np.bincount(label, minlength=k)).all() and got["size"].sum() == m
            assert all(int(d[i, med[label[i]]]) == int(d[i, med].min()) for i in range(m))                   # everybody with a nearest medoid
            assert all(label[i] == int(np.argmin(d[i, med])) for i in range(m) if i not in med)               # ... the first of equals
            s = got["silhouette"]
            assert s.dtype == np.float64 and s.shape == (m,) and (np.abs(s) <= 1.0).all() and (k > 1 or not s.any())
        if m:
            one = medoids(d, 1)
            assert one["medoid"][0] == int(np.argmin(d.astype(object).sum(axis=0))) and one["size"].tolist() == [m] and not one["label"].any()
            every = medoids(d, m)
            assert every["medoid"].tolist() == list(range(m)) and every["cost"] == 0 and every["label"].tolist() == list(range(m))
        with pytest.raises(ValueError):
            medoids(d, m + 1)
        with pytest.raises(ValueError):
            medoids(d, 0)


def test_medoids_are_deterministic_under_ties_and_find_two_clear_clusters():
    d = np.zeros((5, 5), np.uint64)                                 # all equal: the lowest indices, every member with the first
    got = medoids(d, 2)
    assert got["medoid"].tolist() == [0, 1] and got["label"].tolist() == [0, 1, 0, 0, 0] and got["cost"] == 0 and not got["silhouette"].any()
    tie = np.array([[0, 1, 1], [1, 0, 1], [1, 1, 0]], np.uint64)
    assert medoids(tie, 1)["medoid"].tolist() == [0] and medoids(tie, 2)["medoid"].tolist() == [0, 1] and medoids(tie, 2)["label"].tolist() == [0, 1, 0]
    x = np.array([[0, 0], [1, 0], [0, 1], [100, 100], [101, 100], [100, 102], [101, 101]], np.uint32)
    order = np.array([3, 0, 5, 1, 6, 2, 4])
    d = ref.distances(x[order], "l1")
    got = medoids(d, 2)
    far = order >= 3
    found = sorted(order[got["medoid"]].tolist())                   # (0, 0) is the one medoid of the near cluster; three members tie in the far one
    assert found[0] == 0 and found[1] in (3, 4, 6) and got["cost"] == 2 + 5
    assert len(set(got["label"][far])) == 1 and len(set(got["label"][~far])) == 1 and got["label"][far][0] != got["label"][~far][0]
    assert got["size"].tolist() in ([3, 4], [4, 3]) and (got["silhouette"] > 0.9).all()
    again = medoids(d.copy(), 2)
    assert all(np.array_equal(got[k], again[k]) for k in got)
    for p in (np.array([6, 5, 4, 3, 2, 1, 0]), np.array([2, 4, 6, 0, 1, 3, 5])):                       # the same clusters whatever the order of the members
        g = medoids(d[np.ix_(p, p)], 2)
        assert g["cost"] == got["cost"] and sorted(g["size"].tolist()) == [3, 4] and len(set(g["label"][far[p]])) == 1
    with pytest.raises(ValueError):
        medoids(np.zeros((2, 3)), 1)
    assert medoids(d, 2, max_swaps=0)["cost"] >= got["cost"]


# ---- the keys of the area dict ------------------------------------------------------------------------------------------------------------
def test_keep_spec_takes_the_cluster_keys_out_and_refuses_them_for_the_reproduction_kind():
    e = Ensemble.__new__(Ensemble)                                   # no simulator, no context: nothing here may reach the library
    e.base = _lib.default_params()
    series = dict(kind="series", where="home", what="infected", first_step=1, n_rows=3, stride=1)
    want = {k: v for k, v in series.items() if k != "kind"}
    kind, area = e._area_kind("run", dict(series, clusters=3), 10, False, 6)
    assert kind == "series" and area == want                         # the begin call never sees the new keys
    assert e._keep_spec["clusters"] == 3 and e._keep_spec["cluster_metric"] == "l1" and e._keep_spec["band_only"] and e._keep_spec["what"] == "value" and "band" not in e._keep_spec
    assert e._area_kind("run", dict(series, cluster_metric="differ"), 10, False, 6)[1] == want and e._keep_spec["clusters"] == 2 and e._keep_spec["cluster_metric"] == "differ"
    assert e._area_kind("run", dict(series, clusters=6, band=0.5), 10, False, 6)[1] == want and e._keep_spec["band_only"] and e._keep_spec["band"] == 0.5
    assert e._area_kind("run", dict(series, clusters=2, quantiles=(0.5,)), 10, False, 6)[1] == want and not e._keep_spec["band_only"] and e._keep_spec["probs"] == [0.5]
    assert e._area_kind("run", dict(series, quantiles=(0.5,)), 10, False, 6)[1] == want and "clusters" not in e._keep_spec   # without the keys: as before
    assert e._keep_spec == dict(probs=[0.5], method="nearest", thresholds=[], what="value")
    assert e._area_kind("run", dict(series), 10, False, 6)[1] == want and e._keep_spec is None
    for bad, n in ((dict(kind="reproduction", where="home", clusters=2), 6), (dict(kind="reproduction", where="home", cluster_metric="l1"), 6),
                   (dict(series, clusters=0), 6), (dict(series, clusters=7), 6), (dict(series, clusters=2.5), 6), (dict(series, clusters=True), 6),
                   (dict(series, cluster_metric="l2"), 6), (dict(series, clusters=2), 257)):
        with pytest.raises(ValueError) as err:
            e._area_kind("run", bad, 10, False, n)
        if bad.get("kind") == "reproduction":
            assert "the reproduction kind keeps no members" in str(err.value)


# ---- the wrapper against the call recorder ------------------------------------------------------------------------------------------------
def test_the_wrapper_makes_the_recorded_calls_and_returns_the_stated_shapes():
    sim = bare_simulator(0, 100)
    sim.ensemble_begin_series("home", "infected", first_step=1, n_rows=5)
    del sim.lib.calls[:]
    d = sim.ensemble_distances()
    assert sim.lib.calls == ["ensemble_members_info(&u32,&u32,&i32,&i32)", "ensemble_distances(0,5,0,4294967295,*u64,&u64)"]
    assert sorted(d) == ["cells", "distances", "live_cells", "metric"] and d["distances"].dtype == np.uint64 and d["distances"].shape == (KEPT, KEPT)
    assert d["cells"] == 15 and d["metric"] == "l1" and isinstance(d["live_cells"], int)
    assert sim.ensemble_distances("differ", first_row=1, n_rows=2, never_as=120)["cells"] == 6 and sim.lib.calls[-1] == "ensemble_distances(1,2,1,120,*u64,&u64)"
    assert sim.ensemble_distances(_lib.DIST_DIFFER)["metric"] == "differ"
    del sim.lib.calls[:]
    for bad in ("l2", None, 1.5, True):
        with pytest.raises(ValueError):
            sim.ensemble_distances(bad)
    assert not any(c.startswith("ensemble_distances") for c in sim.lib.calls)
    assert sorted(sim.ensemble_distances_info()) == ["tiles", "tiles_32bit", "tiles_partial"]


# ---- the entry points and the header --------------------------------------------------------------------------------------------------------
def test_the_entry_points_are_declared_exported_and_bound_with_the_headers_arity():
    text = open(os.path.join(ROOT, "include", "esim.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"#define\s+ESIM_DIST_L1\s+0\b", header) and re.search(r"#define\s+ESIM_DIST_DIFFER\s+1\b", header) and (_lib.DIST_L1, _lib.DIST_DIFFER) == (0, 1)
    lib = _lib.load()
    raw = C.CDLL(os.path.join(ROOT, "epidemicsimulator_amd", "libesim.so"))
    for name in NEW:
        proto = re.search(r"\bint\s+%s\s*\((esim_ctx \*.*?)\);" % name, header, re.S)
        assert proto, name
        assert name in _lib.SYMBOLS and hasattr(raw, name)
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == len(proto.group(1).split(",")), name
    assert lib.esim_ensemble_distances.argtypes[1:] == [C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    engine = open(os.path.join(CSRC, "esim_dist.h")).read()
    assert [i for i in re.findall(r'#include\s+[<"]([^>"]+)[>"]', engine) if not i.startswith("type_traits")] == ["esim_members.h"]     # a probe can compile it alone
    probe = open(os.path.join(ROOT, "tests", "native", "dist_probe.hip")).read()
    assert [i for i in re.findall(r'#include\s+"([^"]+)"', probe)] == ["esim_dist.h"]
    assert '#include "esim_host_dist.h"' in open(os.path.join(CSRC, "esim_api.hip")).read()
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert "esim_host_dist.h" in make and "esim_dist.h" in make.replace("esim_host_dist.h", "")


def test_the_header_compiles_alone_for_gfx950_and_its_kernels_use_no_scratch(tmp_path):
    """The resource query of test_kernel_resources.py on the probe, which includes esim_dist.h and nothing else of the library."""
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-fast-math", "-ffp-contract=off", "--cuda-device-only",
           "-Rpass-analysis=kernel-resource-usage", "-I", CSRC, "-c", "-o", str(tmp_path / "k.o"), os.path.join(ROOT, "tests", "native", "dist_probe.hip")]
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
    dist = {k: v for k, v in kernels.items() if "k_dist" in k}
    assert len(dist) == 7, sorted(kernels)                           # three tile sizes by two metrics, and the mirror
    for name, r in dist.items():
        assert r.get("ScratchSize [bytes/lane]", 0) == 0, "%s uses %d bytes of scratch per lane" % (name, r["ScratchSize [bytes/lane]"])
        assert r.get("VGPRs Spill", 0) == 0 and r["LDS Size [bytes/block]"] <= 64 * 1024, (name, r)
