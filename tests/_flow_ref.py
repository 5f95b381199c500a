"""Expected area flows, imports, invasion tree and (lineage, area) pairs of a run, computed with numpy from a
_tree_ref.reference() and the chains of _chain_ref (and so from the CPU oracle).  Test infrastructure only.

The area of a citizen is that of its household.  A transmission is an exposure of step >= 1 with an infector; the flows are
np.unique over src * n_areas + dst, the imports np.add.at, the first case of an area the minimum of (cohort step, citizen) over
its resident cases.  One more world, `spread`: 256 areas and one school for everybody, so that the infection crosses between
areas thousands of times and the distinct flow pairs exceed one tile of the device sort."""
import functools

import numpy as np

import _chain_ref as chain
import _setting_ref as ref_mod
import _tree_ref as tree
from epidemicsimulator_amd import Population, _lib

NONE = 0xFFFFFFFF
ALL = (1 << _lib.N_SETTINGS) - 1


def home_area(pop):
    return pop.building_area[pop.home_building].astype(np.int64)


def transmissions(ref, pop, mask=ALL, first_step=1, last_step=None):
    """(infectees, areas of their infectors, their own areas) over the transmissions of the window and mask."""
    last_step = ref["n_steps"] if last_step is None else last_step
    se, st = ref["setting"], ref["step"].astype(np.int64)
    keep = (ref["infector"] != NONE) & (se < _lib.N_SETTINGS) & (((mask >> np.minimum(se, 4).astype(np.int64)) & 1) != 0) & (st >= max(1, first_step)) & (st <= last_step)
    who = np.flatnonzero(keep)
    area = home_area(pop)
    return who, area[ref["infector"][who].astype(np.int64)], area[who]


def flows(ref, pop, mask=ALL, first_step=1, last_step=None):
    """What esim_area_flows returns: (src, dst, count), ascending by (src, dst)."""
    _, src, dst = transmissions(ref, pop, mask, first_step, last_step)
    key, count = np.unique(src * pop.n_areas + dst, return_counts=True)
    return (key // pop.n_areas).astype(np.uint32), (key % pop.n_areas).astype(np.uint32), count.astype(np.uint32)


def imports(ref, pop, mask=ALL, first_step=1, last_step=None):
    """What esim_area_imports returns: dict of local, imported, exported."""
    _, src, dst = transmissions(ref, pop, mask, first_step, last_step)
    out = {k: np.zeros(pop.n_areas, np.uint32) for k in ("local", "imported", "exported")}
    same = src == dst
    np.add.at(out["local"], dst[same], 1)
    np.add.at(out["imported"], dst[~same], 1)
    np.add.at(out["exported"], src[~same], 1)
    return out


def invasion(ref, pop):
    """What esim_area_invasion returns: dict of first_case, step, source_area, setting; and `tied`, the areas whose first case
    shares its cohort step with another resident case (the tie rule decided)."""
    na, area, st = pop.n_areas, home_area(pop), tree.cohort_step(ref, pop)
    out = dict(first_case=np.full(na, NONE, np.uint32), step=np.full(na, NONE, np.uint32), source_area=np.full(na, NONE, np.uint32),
               setting=np.full(na, _lib.SETTING_NONE, np.uint8))
    cases = np.flatnonzero(st >= 0)
    order = cases[np.lexsort((cases, st[cases], area[cases]))]       # by area, then cohort step, then citizen
    areas, first = np.unique(area[order], return_index=True)
    win = order[first]
    out["first_case"][areas], out["step"][areas] = win, st[win]
    src = ref["infector"][win]
    known = (src != NONE) & (st[win] >= 1)
    out["source_area"][areas[known]] = area[src[known].astype(np.int64)]
    out["setting"][areas[known]] = ref["setting"][win[known]]
    at_first = np.bincount(area[cases][st[cases] == out["step"][area[cases]]], minlength=na)
    out["tied"] = at_first >= 2
    return out


def lineage_areas(ch, pop):
    """What esim_lineage_areas returns: (lineage, area, count), ascending."""
    who = np.flatnonzero(ch["lineage"] != NONE)
    key, count = np.unique(ch["lineage"][who].astype(np.int64) * pop.n_areas + home_area(pop)[who], return_counts=True)
    return (key // pop.n_areas).astype(np.uint32), (key % pop.n_areas).astype(np.uint32), count.astype(np.uint32)


def forest_depth(source_area):
    """The largest number of hops from an area to the root of its tree in the invasion forest."""
    src = np.asarray(source_area).astype(np.int64)
    depth, cur = 0, np.flatnonzero(src != NONE)
    while cur.size and depth <= src.size:
        depth += 1
        cur = src[cur]
        cur = cur[src[cur] != NONE]
    return depth


def spread_world():
    """256 areas of about 80 citizens, one school that every student of the town goes to, no interventions: 14 119
    transmissions in 240 steps, 4 356 of them between areas, 2 312 distinct flow pairs."""
    pop = Population.synthetic("york", n_citizens=20000, n_areas=256, citizens_per_school=20000, n_seeds=20)
    ep = _lib.default_params(exposure_chance=0.03, exposed_time=24, infected_time=120, lockdown_threshold=2.0, vaccination_threshold=2.0,
                             mask_pt_threshold=2.0, mask_everywhere_threshold=2.0, seed=7, max_steps=300)
    return pop, ep, 240


@functools.lru_cache(maxsize=None)
def cached(name):
    """(population, parameters, steps, tree reference, chains) of a world of _chain_ref.ALL_WORLDS or of `spread`, once per session."""
    if name == "spread":
        pop, ep, n = spread_world()
        ref = tree.reference(pop, ep, n, ref_mod.reference(pop, ep, n))
        return pop, ep, n, ref, chain.chains(ref, pop)
    return chain.cached(name)


reseeded = chain.reseeded

ALL_WORLDS = chain.ALL_WORLDS + ("spread",)
