"""Transmission chains, the CPU side: the numpy reference of tests/_chain_ref.py is consistent with the tree it was built from and
with the records of the oracle, every world holds what it is here for, and the ABI and Python surfaces of the three calls are
what include/esim.h says."""
import inspect
import os

import numpy as np
import pytest

import _chain_ref as chain
import _setting_ref as ref_mod
import _tree_ref as tree
from epidemicsimulator_amd import Simulator, _lib
from epidemicsimulator_amd.ensemble import Ensemble

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = chain.NONE


def identities(pop, ep, n, infector, gen, step, total, got, ages, by_setting=None):
    """What holds between the tree (infector, generation, exposure step per citizen; `total` exposures in the records), the
    chains `got` (seeds, lineage, descendants, size, depth, last_step) and the age table, with no oracle needed.  The GPU tests
    call this too."""
    seeds, lineage, desc = got["seeds"].astype(np.int64), got["lineage"], got["descendants"]
    exposed = np.flatnonzero(infector != NONE)
    src = infector[exposed].astype(np.int64)
    assert (lineage[seeds] == np.arange(len(seeds))).all()
    assert (lineage[exposed] == lineage[src]).all()                                    # lineage[c] == lineage[infector[c]]
    never = np.ones(pop.n_citizens, bool)
    never[exposed] = False
    never[seeds] = False
    assert (lineage[never] == NONE).all() and (desc[never] == 0).all()
    below = np.zeros(pop.n_citizens, np.int64)
    np.add.at(below, src, desc[exposed].astype(np.int64) + 1)
    assert (desc == below).all()                                                       # descendants = sum over children (descendants + 1)
    assert int(got["size"].sum()) + len(seeds) == len(exposed) + len(seeds) == total + len(seeds)   # the length of the log
    assert (got["size"] == desc[seeds]).all()
    assert (got["size"] == np.bincount(lineage[lineage != NONE], minlength=len(seeds)) - 1).all()
    depth, last = np.zeros(len(seeds), np.int64), np.zeros(len(seeds), np.int64)
    np.maximum.at(depth, lineage[exposed], gen[exposed])
    np.maximum.at(last, lineage[exposed], step[exposed])
    assert (got["depth"] == depth).all() and (got["last_step"] == last).all()
    assert ages.shape == (_lib.N_SETTINGS, _lib.AGE_BINS) and int(ages.sum()) == total
    if by_setting is not None:
        assert (ages.sum(axis=1) == by_setting).all()
    assert (np.flatnonzero(ages.sum(axis=0)) <= int(ep.infected_time)).all()           # every non-zero bin lies in 0 .. infected_time


@pytest.mark.parametrize("name", chain.ALL_WORLDS)
def test_chains_of_the_reference_agree_with_the_tree_and_the_records(name):
    pop, ep, n, ref, ch = chain.cached(name)
    assert ref["empty"] == 0 and ref["not_infected"] == 0
    rec = ref["records"]
    total = int(rec["exposures_building"].sum()) + int(rec["exposures_bus"].sum())
    by_setting = ref_mod.rows(ref, pop, "setting", stride=n, n_rows=1)[0]
    identities(pop, ep, n, ref["infector"], ref["generation"], ref["step"], total, ch, chain.ages(ref, pop, ep), by_setting)
    assert (ch["seeds"] == chain.seeds_in_force(pop.seeds)).all() and len(ch["seeds"]) == len(np.unique(pop.seeds))
    # windows of the age table add up to the whole
    whole = chain.ages(ref, pop, ep)
    assert (chain.ages(ref, pop, ep, 1, n // 2) + chain.ages(ref, pop, ep, n // 2 + 1, n) == whole).all()


def situation(name):
    """What a world is here for, from its reference alone (the GPU tests call this too).  The counts in the comments were
    measured on the oracle; the bounds leave slack below them."""
    pop, ep, n, ref, ch = chain.cached(name)
    if name == "deep":
        gen = ref["generation"]
        assert len(ch["seeds"]) == 2 and int(ep.exposed_time) == 0                     # a window is one step
        assert gen[gen != NONE].max() >= 15                                            # 22
        assert (ch["size"] > 300).all()                                                # 781 and 666
        who, a = chain.infectious_age(ref, pop, ep)
        assert a.min() >= 0 and a.max() <= int(ep.infected_time)                       # generation intervals 1 .. 7
        st = tree.cohort_step(ref, pop)
        src = ref["infector"][who].astype(np.int64)
        assert ((st[src] >= 1) & (st[who] == st[src] + 1)).sum() >= 200                # 458 exposed one step after their infector was
    elif name == "school":
        inner = np.ones(pop.n_citizens, bool)
        inner[ch["seeds"]] = False
        assert ch["descendants"][inner].max() >= 50                                    # 88 below a citizen that is no index case
    elif name == "as_u8":
        assert len(ch["seeds"]) == 257 and (ch["size"] == 0).sum() >= 200              # most introductions infect nobody
    elif name == "fixture_a":
        assert len(ch["seeds"]) == 20 and (ch["size"] > 0).all()                       # all 20 lineages non-empty


@pytest.mark.parametrize("name", ["deep", "school", "as_u8", "fixture_a"])
def test_every_world_holds_what_it_is_here_for(name):
    situation(name)


def test_abi_surface():
    text = open(os.path.join(ROOT, "include", "esim.h")).read()
    assert "#define ESIM_NO_LINEAGE 0xFFFFFFFFu" in text and "#define ESIM_AGE_BINS   512" in text
    assert _lib.NO_LINEAGE == 0xFFFFFFFF and _lib.AGE_BINS == 512
    for decl in ("int  esim_transmission_chains(esim_ctx *ctx, uint32_t *lineage /* [n_citizens] or NULL */, uint32_t *descendants /* [n_citizens] or NULL */);",
                 "int  esim_outbreaks(esim_ctx *ctx, uint32_t *size, uint32_t *depth, uint32_t *last_step /* [cap] each, any may be NULL */,",
                 "uint32_t cap, uint32_t *n_out);",
                 "int  esim_transmission_ages(esim_ctx *ctx, uint32_t first_step, uint32_t last_step, uint32_t *counts /* [ESIM_N_SETTINGS * ESIM_AGE_BINS] */);"):
        assert decl in text
    assert "generation interval" in text.lower() and "a + exposed_time + 1" in text
    lib = _lib.load()
    for name in ("esim_transmission_chains", "esim_outbreaks", "esim_transmission_ages"):
        assert name in _lib.SYMBOLS and getattr(lib, name).restype is not None
    # a null context is refused before anything touches a device
    assert lib.esim_transmission_chains(None, None, None) == -1
    assert lib.esim_outbreaks(None, None, None, None, 0, None) == -1
    assert lib.esim_transmission_ages(None, 1, 1, None) == -1


def test_python_surface(tmp_path):
    from epidemicsimulator_amd.ensemble import OutbreakResult

    def defaults(f):
        return {k: p.default for k, p in inspect.signature(f).parameters.items() if p.default is not inspect.Parameter.empty}
    assert defaults(Simulator.transmission_chains) == {} and defaults(Simulator.outbreaks) == {}
    assert defaults(Simulator.transmission_ages) == dict(first_step=1, last_step=None)
    assert list(inspect.signature(Ensemble.outbreaks).parameters) == ["self", "members", "n_steps", "ages"]
    assert defaults(Ensemble.outbreaks) == dict(ages=False)
    # neither run() nor forecast() gained a keyword
    assert list(inspect.signature(Ensemble.run).parameters)[-2:] == ["settings", "reproduction"]
    assert list(inspect.signature(Ensemble.forecast).parameters)[-2:] == ["settings", "reproduction"]
    # a hand-made result: two members, of three seeds and of one
    tables = [dict(seeds=np.array([7, 3, 9], np.uint32), size=np.array([5, 0, 1], np.uint32), depth=np.array([2, 0, 1], np.uint32), last_step=np.array([40, 0, 12], np.uint32)),
              dict(seeds=np.array([4], np.uint32), size=np.array([0], np.uint32), depth=np.array([0], np.uint32), last_step=np.array([0], np.uint32))]
    ages = [np.zeros((4, 512), np.uint32), np.ones((4, 512), np.uint32)]
    res = OutbreakResult.gathered([{"seed": 1}, {"seed": 2}], tables, ages)
    assert res.members == [{"seed": 1}, {"seed": 2}] and [s.tolist() for s in res.seeds] == [[7, 3, 9], [4]]
    assert res.size.dtype == np.int64 and res.size.tolist() == [[5, 0, 1], [0, -1, -1]]
    assert res.depth.tolist() == [[2, 0, 1], [0, -1, -1]] and res.last_step.tolist() == [[40, 0, 12], [0, -1, -1]]
    assert res.ages.shape == (2, 4, 512)
    assert res.extinct().tolist() == [[False, True, False], [True, False, False]]
    assert res.extinct(min_size=2).tolist() == [[False, True, True], [True, False, False]]
    res.dump(str(tmp_path))
    got = np.load(tmp_path / "ensemble_outbreaks.npz")
    assert (got["size"] == res.size).all() and (got["depth"] == res.depth).all() and (got["last_step"] == res.last_step).all()
    assert got["seeds"].tolist() == [[7, 3, 9], [4, -1, -1]] and (got["ages"] == res.ages).all()
    none = OutbreakResult.gathered([], [])
    assert none.size.shape == (0, 0) and none.ages is None and none.extinct().shape == (0, 0)
    none.dump(str(tmp_path / "none"))
    assert "ages" not in np.load(tmp_path / "none" / "ensemble_outbreaks.npz").files
