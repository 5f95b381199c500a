"""Expected lineage, descendants, outbreak table and infectious ages of a run, computed with numpy from a _tree_ref.reference()
(and so from the CPU oracle).  Test infrastructure only.

The citizens are ordered by exposure step; roots are propagated forward along the infectors and subtree sums backward; the
infectious age of a transmission is the infectee's step minus the infector's onset, from _tree_ref.cohort_step with onset 0 for
the index cases ("Infected from step 1").  One more world, `deep`: exposed_time 0, where a window of the device passes is a
single step and a wrong window order shows at once."""
import copy
import functools

import numpy as np

import _setting_ref as ref_mod
import _tree_ref as tree
from epidemicsimulator_amd import Population, _lib

NONE = 0xFFFFFFFF


def seeds_in_force(seeds):
    """The distinct index cases in the order of their first occurrence: what esim_get_seeds returns."""
    seeds = np.asarray(seeds, np.int64)
    _, first = np.unique(seeds, return_index=True)
    return seeds[np.sort(first)].astype(np.uint32)


def with_seeds(pop, seeds):
    """The same world with other index cases."""
    out = copy.copy(pop)
    out.seeds = np.ascontiguousarray(seeds, dtype=np.uint32)
    out.n_seeds = int(out.seeds.size)
    return out


def chains(ref, pop):
    """dict: seeds (in force), lineage, descendants per citizen; size, depth, last_step per index case."""
    n = pop.n_citizens
    seeds = seeds_in_force(pop.seeds)
    infector, gen = ref["infector"].astype(np.int64), ref["generation"]
    st = tree.cohort_step(ref, pop)
    lineage, desc = np.full(n, NONE, np.uint32), np.zeros(n, np.uint32)
    lineage[seeds] = np.arange(len(seeds), dtype=np.uint32)
    exposed = np.flatnonzero(st >= 1)
    order = exposed[np.argsort(st[exposed], kind="stable")]
    for c in order.tolist():                                         # roots forward: an infector was exposed in an earlier step
        if infector[c] != NONE:
            lineage[c] = lineage[infector[c]]
    for c in order[::-1].tolist():                                   # sums backward: every child comes before its infector
        if infector[c] != NONE:
            desc[infector[c]] += desc[c] + 1
    size, depth, last = desc[seeds].copy(), np.zeros(len(seeds), np.uint32), np.zeros(len(seeds), np.uint32)
    rooted = np.flatnonzero((lineage != NONE) & (st >= 1))
    np.maximum.at(depth, lineage[rooted], gen[rooted])
    np.maximum.at(last, lineage[rooted], st[rooted].astype(np.uint32))
    return dict(seeds=seeds, lineage=lineage, descendants=desc, size=size, depth=depth, last_step=last)


def infectious_age(ref, pop, ep):
    """(citizens with an infector, the infectious age of their transmission)."""
    st = tree.cohort_step(ref, pop)
    who = np.flatnonzero(ref["infector"] != NONE)
    src = ref["infector"][who].astype(np.int64)
    onset = np.where(st[src] == 0, 0, st[src] + int(ep.exposed_time) + 1)
    return who, st[who] - onset


def ages(ref, pop, ep, first_step=1, last_step=None):
    """What esim_transmission_ages returns: uint32 [4, 512]."""
    last_step = ref["n_steps"] if last_step is None else last_step
    who, a = infectious_age(ref, pop, ep)
    keep = (ref["step"][who] >= first_step) & (ref["step"][who] <= last_step) & (ref["setting"][who] < _lib.N_SETTINGS)
    out = np.zeros((_lib.N_SETTINGS, _lib.AGE_BINS), np.uint32)
    np.add.at(out, (ref["setting"][who][keep].astype(np.int64), a[keep]), 1)
    return out


def deep_world():
    """No Exposed period, a week of infectiousness, a high exposure chance and no interventions: two outbreaks of several
    hundred citizens each and more than twenty generations in 150 steps."""
    pop = Population.synthetic("york", n_citizens=1500, n_areas=4, citizens_per_school=750, n_seeds=3)
    ep = _lib.default_params(exposure_chance=0.05, exposed_time=0, infected_time=6, lockdown_threshold=2.0, vaccination_threshold=2.0,
                             mask_pt_threshold=2.0, mask_everywhere_threshold=2.0, seed=21, max_steps=200)
    return pop, ep, 150


@functools.lru_cache(maxsize=None)
def cached(name):
    """(population, parameters, steps, tree reference, chains) of a world of _tree_ref.ALL_WORLDS or of `deep`, once per session."""
    if name == "deep":
        pop, ep, n = deep_world()
        ref = tree.reference(pop, ep, n, ref_mod.reference(pop, ep, n))
    else:
        pop, ep, n, ref = tree.cached(name)
    return pop, ep, n, ref, chains(ref, pop)


@functools.lru_cache(maxsize=None)
def reseeded(name, seeds, n_steps):
    """The same for world `name` started from the index cases `seeds` (a tuple) and run for n_steps steps."""
    pop, ep, _, _ = tree.cached(name)
    pop = with_seeds(pop, seeds)
    ref = tree.reference(pop, ep, n_steps, ref_mod.reference(pop, ep, n_steps))
    return pop, ep, n_steps, ref, chains(ref, pop)


ALL_WORLDS = tree.ALL_WORLDS + ("deep",)
