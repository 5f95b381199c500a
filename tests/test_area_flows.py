"""Area flows, imports, the invasion tree and the (lineage, area) pairs, the CPU side: the numpy reference of tests/_flow_ref.py
is consistent with the settings, the tree, the chains and the arrival times it was built beside, the world `spread` holds what
it is here for, and the ABI and Python surfaces of the calls are what include/esim.h says."""
import inspect
import os
import re

import numpy as np
import pytest

import _arrival_ref as arrival
import _chain_ref as chain
import _flow_ref as flow
import _setting_ref as ref_mod
import _tree_ref as tree
from epidemicsimulator_amd import Simulator, _lib
from epidemicsimulator_amd.ensemble import Ensemble

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, S, T = _lib.SETTING_HOUSEHOLD, _lib.SETTING_SCHOOL, _lib.SETTING_TRANSPORT
MASKS = (flow.ALL, 1 << H, 1 << S, 1 << T)


def sort_tile():
    text = open(os.path.join(ROOT, "epidemicsimulator_amd", "csrc", "esim_pairs.h")).read()
    return int(re.search(r"#define PAIR_SORT_TILE (\d+)u", text).group(1))


def flow_identities(src, dst, count, imp, n_areas):
    """What holds between the flows and the imports of one window and mask, with no oracle needed.  The GPU tests call this too."""
    key = src.astype(np.int64) * n_areas + dst
    assert (np.diff(key) > 0).all() and (count >= 1).all()                                        # ascending, every pair once
    diag = src == dst
    on_diag, rows, cols = np.zeros(n_areas, np.int64), np.zeros(n_areas, np.int64), np.zeros(n_areas, np.int64)
    on_diag[src[diag]] = count[diag]
    np.add.at(rows, src, count)
    np.add.at(cols, dst, count)
    assert (on_diag == imp["local"]).all()
    assert (rows == imp["local"].astype(np.int64) + imp["exported"]).all() and (cols == imp["local"].astype(np.int64) + imp["imported"]).all()
    assert int(imp["imported"].sum()) == int(imp["exported"].sum())


def windows(ref, n):
    busy = int(np.bincount(ref["step"][ref["step"] > 0]).argmax())                                # the step with the most exposures
    return ((1, n), (max(1, n // 3), max(1, n // 2)), (busy, busy))


@pytest.mark.parametrize("name", flow.ALL_WORLDS)
def test_reference_agrees_with_the_settings_the_tree_and_the_chains(name):
    pop, ep, n, ref, ch = flow.cached(name)
    na, area = pop.n_areas, flow.home_area(pop)
    orphan = (ref["step"] >= 1) & (ref["setting"] < _lib.N_SETTINGS) & (ref["infector"] == flow.NONE)   # explained, but nobody to credit
    for mask in MASKS:
        for first, last in windows(ref, n):
            who, _, _ = flow.transmissions(ref, pop, mask, first, last)
            src, dst, count = flow.flows(ref, pop, mask, first, last)
            imp = flow.imports(ref, pop, mask, first, last)
            assert int(count.sum()) == who.size                                                   # every transmission in one pair
            flow_identities(src, dst, count, imp, na)
            # the infectees by home area: the ESIM_AREA_HOME rows of the settings over the window, less the entries without a candidate
            by_home = ref_mod.rows(ref, pop, "home", mask=mask, first_step=first, n_rows=1, stride=last - first + 1)[0]
            lost = orphan & (ref["step"] >= first) & (ref["step"] <= last) & (((mask >> np.minimum(ref["setting"], 4).astype(np.int64)) & 1) != 0)
            assert (imp["local"].astype(np.int64) + imp["imported"] + np.bincount(area[lost], minlength=na) == by_home).all()
            if mask == 1 << H:
                assert (src == dst).all()                                                         # housemates share an area
    # windows that partition the run add up to the whole
    cuts = [1, max(2, n // 3), max(3, n // 2 + 1), n + 1]
    whole = flow.flows(ref, pop)
    total = np.zeros((na, na), np.int64) if na <= 1024 else None
    parts = [flow.flows(ref, pop, flow.ALL, lo, hi - 1) for lo, hi in zip(cuts[:-1], cuts[1:])]
    assert sum(int(p[2].sum()) for p in parts) == int(whole[2].sum())
    if total is not None:
        for p in parts:
            np.add.at(total, (p[0], p[1]), p[2])
        assert (total[whole[0], whole[1]] == whole[2]).all() and int(total.sum()) == int(whole[2].sum())
    for k in ("local", "imported", "exported"):
        assert (sum(flow.imports(ref, pop, flow.ALL, lo, hi - 1)[k].astype(np.int64) for lo, hi in zip(cuts[:-1], cuts[1:])) == flow.imports(ref, pop)[k]).all()
    # the invasion tree
    inv = flow.invasion(ref, pop)
    assert (inv["step"] == arrival.arrival(area, na, ref["step"], pop.seeds)).all()
    has = inv["source_area"] != flow.NONE
    a = np.flatnonzero(has)
    assert (inv["source_area"][a] != a).all() and (inv["step"][inv["source_area"][a]] < inv["step"][a]).all()
    assert (inv["step"][a] >= 1).all() and (inv["setting"][a] < _lib.N_SETTINGS).all() and (inv["setting"][~has] == _lib.SETTING_NONE).all()
    assert ((inv["first_case"] == flow.NONE) == (inv["step"] == flow.NONE)).all()
    assert (area[inv["first_case"][inv["step"] != flow.NONE]] == np.flatnonzero(inv["step"] != flow.NONE)).all()
    assert (inv["step"][area[np.asarray(pop.seeds, np.int64)]] == 0).all()                      # the roots: the areas of the index cases
    assert flow.forest_depth(inv["source_area"]) <= na
    # the lineages
    lin, where, cnt = flow.lineage_areas(ch, pop)
    assert (np.diff(lin.astype(np.int64) * na + where) > 0).all()
    rooted = ch["lineage"] != flow.NONE
    assert int(cnt.sum()) == int(rooted.sum())
    if ref["empty"] == 0:                                                                         # every chain ends at an index case
        assert int(cnt.sum()) == int(ch["size"].sum()) + len(ch["seeds"])
    assert (np.bincount(lin, weights=cnt, minlength=len(ch["seeds"])) == np.bincount(ch["lineage"][rooted], minlength=len(ch["seeds"]))).all()


def situation():
    """What `spread` is here for, from its reference alone (the GPU tests call this too).  The counts in the comments were
    measured on the oracle."""
    pop, ep, n, ref, ch = flow.cached("spread")
    who, a_src, a_dst = flow.transmissions(ref, pop)
    src, dst, count = flow.flows(ref, pop)
    assert who.size == 14119 and ref["empty"] == 0
    cross = a_src != a_dst
    assert int(cross.sum()) == 4356 and (ref["setting"][who[cross]] == S).all()                   # all through the one school
    assert src.size == 2312 and src.size > sort_tile()                                            # more than one tile of the device sort
    inv = flow.invasion(ref, pop)
    assert int((inv["step"] != flow.NONE).sum()) == 253 and int((inv["source_area"] != flow.NONE).sum()) == 234
    assert int((inv["tied"] & (inv["step"] != flow.NONE)).sum()) == 98                            # first cases that the tie rule decides
    assert flow.lineage_areas(ch, pop)[0].size == 1042


def test_spread_has_more_distinct_pairs_than_one_sort_tile():
    situation()


def test_the_existing_worlds_have_between_1_and_125_distinct_pairs():
    sizes = {name: flow.flows(*_ref_pop(name))[0].size for name in chain.ALL_WORLDS}
    assert sizes["ties"] == sizes["as_u8"] == sizes["bus"] == 1 and sizes["permuted"] == 125 and max(sizes.values()) == 125, sizes


def _ref_pop(name):
    pop, ep, n, ref, ch = flow.cached(name)
    return ref, pop


def test_abi_surface():
    text = open(os.path.join(ROOT, "include", "esim.h")).read()
    assert "#define ESIM_NO_AREA 0xFFFFFFFFu" in text and _lib.NO_AREA == 0xFFFFFFFF
    for decl in ("int  esim_area_flows(esim_ctx *ctx, uint32_t setting_mask, uint32_t first_step, uint32_t last_step,",
                 "uint32_t *src, uint32_t *dst, uint32_t *count /* [cap] each, any may be NULL */, uint32_t cap, uint32_t *n_out);",
                 "int  esim_area_imports(esim_ctx *ctx, uint32_t setting_mask, uint32_t first_step, uint32_t last_step,",
                 "uint32_t *local, uint32_t *imported, uint32_t *exported /* [n_areas] each, any may be NULL */);",
                 "int  esim_area_invasion(esim_ctx *ctx, uint32_t *first_case, uint32_t *step, uint32_t *source_area /* [n_areas] each, any may be NULL */,",
                 "int  esim_lineage_areas(esim_ctx *ctx, uint32_t *lineage, uint32_t *area, uint32_t *count /* [cap] each, any may be NULL */,"):
        assert decl in text
    assert "step[source_area[a]] < step[a]" in text and "ESIM_PAIR_LOG2" in text and "smallest local citizen index" in text
    assert "ESIM_PAIR_LOG2" in open(os.path.join(ROOT, "README.md")).read()
    lib = _lib.load()
    for name in ("esim_area_flows", "esim_area_imports", "esim_area_invasion", "esim_lineage_areas", "esim_pair_stats"):
        assert name in _lib.SYMBOLS and getattr(lib, name).restype is not None
    # a null context is refused before anything touches a device
    assert lib.esim_area_flows(None, 0xF, 1, 1, None, None, None, 0, None) == -1
    assert lib.esim_area_imports(None, 0xF, 1, 1, None, None, None) == -1
    assert lib.esim_area_invasion(None, None, None, None, None) == -1
    assert lib.esim_lineage_areas(None, None, None, None, 0, None) == -1


def test_python_surface(tmp_path):
    from epidemicsimulator_amd.ensemble import FlowResult

    def defaults(f):
        return {k: p.default for k, p in inspect.signature(f).parameters.items() if p.default is not inspect.Parameter.empty}
    assert defaults(Simulator.area_flows) == defaults(Simulator.area_imports) == dict(settings=None, first_step=1, last_step=None)
    assert defaults(Simulator.area_invasion) == {} and defaults(Simulator.lineage_areas) == {}
    assert list(inspect.signature(Ensemble.flows).parameters) == ["self", "members", "n_steps", "settings", "first_step", "last_step"]
    assert defaults(Ensemble.flows) == dict(settings=None, first_step=1, last_step=None)
    # neither run() nor forecast() gained a keyword
    assert list(inspect.signature(Ensemble.run).parameters)[-2:] == ["settings", "reproduction"]
    assert list(inspect.signature(Ensemble.forecast).parameters)[-2:] == ["settings", "reproduction"]
    # a hand-made result: two members, three areas
    imports = [dict(local=np.array([4, 0, 1], np.uint32), imported=np.array([1, 0, 3], np.uint32), exported=np.array([3, 1, 0], np.uint32)),
               dict(local=np.array([2, 0, 0], np.uint32), imported=np.array([1, 0, 0], np.uint32), exported=np.array([0, 0, 1], np.uint32))]
    never, nowhere = _lib.NEVER, _lib.NO_AREA
    invasions = [dict(step=np.array([0, never, 30], np.uint32), source_area=np.array([nowhere, nowhere, 0], np.uint32)),
                 dict(step=np.array([26, never, 0], np.uint32), source_area=np.array([2, nowhere, nowhere], np.uint32))]
    res = FlowResult.gathered([{"seed": 1}, {"seed": 2}], imports, invasions, 3)
    assert res.members == [{"seed": 1}, {"seed": 2}]
    for k in ("local", "imported", "exported", "step", "source_area"):
        assert getattr(res, k).shape == (2, 3) and getattr(res, k).dtype == np.uint32
    assert res.local[1, 0] == 2 and res.step[0, 1] == never and res.source_area[1, 0] == 2
    share = res.imported_share()
    assert share.shape == (3,) and share[0] == 2 / 8 and np.isnan(share[1]) and share[2] == 3 / 4
    res.dump(str(tmp_path))
    got = np.load(tmp_path / "ensemble_flows.npz")
    for k in ("local", "imported", "exported", "step", "source_area"):
        assert (got[k] == getattr(res, k)).all()
    assert np.array_equal(got["imported_share"], share, equal_nan=True)
    none = FlowResult.gathered([], [], [], 5)
    assert none.local.shape == none.step.shape == (0, 5) and np.isnan(none.imported_share()).all()
