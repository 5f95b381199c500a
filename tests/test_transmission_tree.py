"""Who infected whom, the CPU side: the numpy reference of tests/_tree_ref.py finds somebody Infected present for every exposure
of the oracle, its counts add up to the records, every world holds the situation it was built for, and the ABI and Python
surfaces of the four calls are what include/esim.h says."""
import inspect
import os
import re

import numpy as np
import pytest

import _tree_ref as tree
from epidemicsimulator_amd import Simulator, _lib
from epidemicsimulator_amd.ensemble import Ensemble, EnsembleResult

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, S, T = tree.H, tree.W, tree.S, tree.T


@pytest.mark.parametrize("name", tree.ALL_WORLDS)
def test_every_exposure_has_a_candidate_and_every_infector_is_infected(name):
    pop, ep, n, ref = tree.cached(name)
    assert ref["empty"] == 0 and ref["not_infected"] == 0
    exposed = ref["step"] > 0
    inf, k, gen = ref["infector"], ref["n_candidates"], ref["generation"]
    assert (inf[exposed] < pop.n_citizens).all() and (k[exposed] >= 1).all()
    assert (inf[~exposed] == tree.NONE).all() and (k[~exposed] == 0).all()
    assert (gen[pop.seeds] == 0).all() and (gen[exposed] == gen[inf[exposed]] + 1).all()
    never = ~exposed
    never[pop.seeds] = False
    assert (gen[never] == tree.NONE).all()
    # an infector was exposed, or is an index case; nobody infects itself
    source = np.unique(inf[exposed])
    assert (exposed[source] | np.isin(source, pop.seeds)).all() and (inf[exposed] != np.flatnonzero(exposed)).all()
    rec = ref["records"]
    total = int(rec["exposures_building"].sum()) + int(rec["exposures_bus"].sum())
    assert tree.offspring(ref, pop, 1, n).sum() == total == exposed.sum()
    lab, n_groups = pop.age_bands([18, 40, 65])
    assert tree.mixing_matrix(ref, pop, lab, n_groups).sum() == total
    cases, off = tree.reproduction_rows(ref, pop, "all", 0, stride=1)
    assert cases[0, 0] == len(np.unique(pop.seeds)) and (cases[1:, 0] == rec["exposures_building"] + rec["exposures_bus"]).all()
    assert off.sum() == total


def situation(name):
    """What a world was built to contain, asserted from its reference alone (the GPU tests call this too).  The counts in the
    comments were measured on the oracle; the bounds leave slack below them."""
    pop, ep, n, ref = tree.cached(name)
    se, k, size, buses, gen = ref["setting"], ref["n_candidates"], ref["list_size"], ref["n_buses"], ref["generation"]
    if name == "school":
        assert ((se == W) & (k >= 65)).sum() >= 1                       # 4: more candidates than a wavefront has lanes
        assert ((se == S) & (k >= 2)).sum() >= 100                      # 264
        assert gen[gen != tree.NONE].max() >= 5                         # 7
    elif name == "as_u8":
        assert ((se == H) & (k >= 256)).sum() >= 10 and k[se == H].max() >= 257   # 34, 257
    elif name == "situations":
        assert ((se == T) & (size >= 65) & (size <= 2048) & (buses >= 2)).sum() >= 100   # 280
        assert ((se == T) & (buses >= 2)).sum() >= 200                  # 539
        rec = ref["records"]
        bus_hours = (int(ep.start_hour) - 1, int(ep.end_hour) - 1)
        frozen = (se == T) & ~np.isin(ref["step"] % 24, bus_hours)      # exposed on a bus the lockdown froze in place
        assert rec["lockdown"].any() and frozen.sum() >= 1
    elif name == "bus":
        long_route = (se == T) & (size > 2048)
        assert long_route.sum() >= 100 and (long_route & (k >= 2)).sum() >= 100   # 156, 135
        assert size[se == T].max() == 2693 and buses.max() == 135
    elif name == "fixture_a":
        rec = ref["records"]
        assert all((se == s).any() for s in range(_lib.N_SETTINGS)) and rec["lockdown"].any() and rec["vaccinated_now"].any()


@pytest.mark.parametrize("name", tree.WORLDS)
def test_every_world_holds_what_it_was_built_for(name):
    situation(name)


def test_rows_of_the_reference_agree_with_each_other():
    pop, ep, n, ref = tree.cached("school")
    lab, n_groups = pop.age_bands([18, 40, 65])
    full_c, full_o = tree.reproduction_rows(ref, pop, "all", 0, stride=1)
    for where, kw in (("home", {}), ("group", dict(labels=lab, n_groups=n_groups))):
        c, o = tree.reproduction_rows(ref, pop, where, 0, stride=1, **kw)
        assert (c.sum(axis=1) == full_c[:, 0]).all() and (o.sum(axis=1) == full_o[:, 0]).all()
    c24, o24 = tree.reproduction_rows(ref, pop, "all", 3, stride=24)
    assert (c24[:, 0] == np.add.reduceat(full_c[3:, 0], np.arange(0, n - 2, 24))).all()
    assert (o24[:, 0] == np.add.reduceat(full_o[3:, 0], np.arange(0, n - 2, 24))).all()
    m = tree.mixing_matrix(ref, pop, lab, n_groups)
    assert (m.sum(axis=0) == np.bincount(lab[ref["step"] > 0], minlength=n_groups)).all()
    assert (m.sum(axis=1) == np.bincount(lab, weights=tree.offspring(ref, pop, 1, n), minlength=n_groups)).all()


def test_abi_surface():
    text = open(os.path.join(ROOT, "include", "esim.h")).read()
    assert re.search(r"#define ESIM_NO_INFECTOR 0xFFFFFFFFu", text) and re.search(r"ESIM_BY_ALL = 4", text)
    assert re.search(r"ESIM_SLOT_INFECTOR = 5", open(os.path.join(ROOT, "epidemicsimulator_amd", "csrc", "philox.h")).read())
    assert _lib.NO_INFECTOR == 0xFFFFFFFF and _lib.BY_ALL == 4
    assert _lib.BY_ALL not in (_lib.AREA_CURRENT, _lib.AREA_HOME, _lib.BY_GROUP, _lib.BY_SETTING)
    lib = _lib.load()
    for name in ("esim_transmission_tree", "esim_offspring", "esim_reproduction_series", "esim_mixing_matrix"):
        assert name in _lib.SYMBOLS and getattr(lib, name).restype is not None
    for decl in ("int  esim_transmission_tree(esim_ctx *ctx, uint32_t *infector", "int  esim_offspring(esim_ctx *ctx, uint32_t first_step, uint32_t last_step, uint32_t *counts",
                 "int  esim_reproduction_series(esim_ctx *ctx, int where, uint32_t first_step, uint32_t n_rows, uint32_t stride,",
                 "int  esim_mixing_matrix(esim_ctx *ctx, uint32_t setting_mask, uint32_t first_step, uint32_t last_step,"):
        assert decl in text
    # a null context is refused before anything touches a device
    assert lib.esim_transmission_tree(None, None, None, None) == -1
    assert lib.esim_offspring(None, 1, 1, None) == -1
    assert lib.esim_reproduction_series(None, _lib.BY_ALL, 0, 1, 1, None, None) == -1
    assert lib.esim_mixing_matrix(None, 0xF, 1, 1, None) == -1


def test_python_surface():
    def defaults(f):
        return {k: p.default for k, p in inspect.signature(f).parameters.items() if p.default is not inspect.Parameter.empty}
    assert defaults(Simulator.transmission_tree) == {}
    assert defaults(Simulator.offspring) == dict(first_step=1, last_step=None)
    assert defaults(Simulator.reproduction_series) == dict(where="all", first_step=0, n_rows=None, stride=24)
    assert defaults(Simulator.mixing_matrix) == dict(settings=None, first_step=1, last_step=None)
    # the new keyword comes last: positional calls of run() and forecast() keep their meaning
    assert list(inspect.signature(Ensemble.run).parameters)[-2:] == ["settings", "reproduction"]
    assert list(inspect.signature(Ensemble.forecast).parameters)[-2:] == ["settings", "reproduction"]
    rows = Ensemble._reproduction_rows
    assert rows("run", None, 100) is None
    assert rows("run", dict(), 100) == dict(first_step=0, n_rows=5, stride=24)
    assert rows("run", dict(first_step=3, stride=7), 100) == dict(first_step=3, n_rows=14, stride=7)
    assert rows("run", dict(n_rows=7), 100) == dict(first_step=0, n_rows=7, stride=24)
    with pytest.raises(ValueError):
        rows("run", dict(where="home"), 100)
    with pytest.raises(ValueError):
        rows("run", dict(), 100, stop_when_done=True)
    assert EnsembleResult(np.zeros((0, 3), np.uint32), [], []).reproduction is None


def test_dump_writes_the_reproduction_rows(tmp_path):
    from epidemicsimulator_amd.simulator import RECORD_DTYPE
    rows = np.arange(2 * 3 * 2, dtype=np.uint32).reshape(2, 3, 2)
    EnsembleResult(np.zeros((2, 3), RECORD_DTYPE), [3, 3], [{}, {}], reproduction=rows).dump(str(tmp_path))
    got = np.load(tmp_path / "ensemble_reproduction.npz")
    assert (got["reproduction"] == rows).all() and got["names"].tolist() == ["cases", "offspring"]
    EnsembleResult(np.zeros((2, 3), RECORD_DTYPE), [3, 3], [{}, {}]).dump(str(tmp_path / "none"))
    assert not (tmp_path / "none" / "ensemble_reproduction.npz").exists()
