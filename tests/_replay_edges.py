"""The replayed outputs at the edges of esim_params: the cases of tests/_param_edges.py on a world the replays accept, with the
references of every replay family (tests/_setting_ref.py, _tree_ref.py, _chain_ref.py, _household_ref.py, _flow_ref.py,
_event_ref.py, _contact_ref.py, _place_ref.py, _curve_ref.py) computed once per case by the functions those modules already
have.  tests/test_replay_edges.py checks on the CPU that every case reaches its edge, tests/test_replay_edges_gpu.py compares
the device with the references.  Importing this module and reading its tables needs neither libesim.so nor a device; world()
calls the library's population builder (host code) and cached() the CPU oracle.

The world is not _param_edges.world(): there citizens work in somebody's household, which the replays refuse (DESIGN 16
"Limits").  It is a builder-shaped town of 3 000 citizens in 8 areas, 459 buildings and 61 school rooms, home-sorted; a permuted
copy sends the residents through res_idx."""
import functools
import types

import numpy as np

import _area_ref
import _chain_ref as chain
import _contact_ref as contact
import _curve_ref as curve
import _event_ref as event
import _flow_ref as flow
import _household_ref as hh
import _param_edges as pe
import _place_ref as place
import _setting_ref as setting
import _tree_ref as tree
from epidemicsimulator_amd import Population, _lib

N = pe.N_STEPS
N_GROUPS = 5
H, W, S, T = tree.H, tree.W, tree.S, tree.T
NAMES = ("household", "workplace", "school", "transport")
MIN_PER_SETTING = 20
MIN_DEPTH = 3
# the cases that run again at pipeline level 0 on the permuted world, and once more with the output grids capped to one block
SECOND_FORM = ("hours_22_6", "hours_23_2", "exposed_time_0", "infected_time_1", "exposure_chance_1", "bus_capacity_2_31")


@functools.lru_cache(maxsize=None)
def world():
    return Population.synthetic("york", n_citizens=3000, n_areas=8, citizens_per_school=1500, n_seeds=12, p_public_transport=0.4)


@functools.lru_cache(maxsize=None)
def permuted_world():
    return _area_ref.permuted(world())


def n_index_cases():
    return len(set(world().seeds.tolist()))


# ---- the cases: _param_edges.CASES, with what this world needs changed ---------------------------------------------------------
# Parameters on top of a case's own, where its guards do not hold on this world under them.
#   hours_1_23: under BASE's lockdown_threshold the lockdown does not both come and go within 400 steps here.
OVERRIDES = {"hours_1_23": dict(lockdown_threshold=0.227)}

# Guards of _param_edges that name its own world, restated for this one.
#   infected_time_0: "every distinct seed Recovered from the first record on" counts the seeds of the world.
GUARDS = {"infected_time_0": (pe.no_exposures, pe.riders, lambda r: int(r["infected"].max()) == 0,
                              lambda r: bool((r["recovered"] == n_index_cases()).all()))}

# Settings a case cannot have, by construction (the guards of _param_edges say why): nothing is asked of them.
NO_EXPOSURES = ("infected_time_0", "exposure_chance_0")
WITHOUT = {"infected_time_0": (H, W, S, T), "exposure_chance_0": (H, W, S, T), "bus_capacity_1": (T,),
           "thresholds_0": (W, S, T)}         # (a lockdown from the second record on; the first step, hour 1, is no working hour)


# The deepest generation a case can reach.  Generation k is exposed in step (k - 1) * (exposed_time + 1) + 1 at the earliest, so
# N steps hold (N - 1) // (exposed_time + 1) + 1 generations at the most: two under exposed_time 200.
#   thresholds_0: the programme runs from the second record on at 25 a step and has vaccinated the town by step 121; generation 2
#   can be exposed from step 98 on, generation 3 only from step 195 on, when nobody is Susceptible any more.
DEPTH_AT_MOST = {"thresholds_0": 2}


def overrides(name):
    return dict(pe.CASES[name].over, **OVERRIDES.get(name, {}))


def params_dict(name):
    return dict(pe.BASE, **overrides(name))


def params_of(name):
    return _lib.default_params(**params_dict(name))


def guards_of(name):
    return GUARDS.get(name, pe.CASES[name].guards)


def allowed_settings(name):
    return tuple(s for s in (H, W, S, T) if s not in WITHOUT.get(name, ()))


def depth_asked(name):
    """The generation depth the case must reach: MIN_DEPTH, or the deepest it can reach where that is less."""
    reachable = (N - 1) // (int(params_of(name).exposed_time) + 1) + 1
    return min(MIN_DEPTH, reachable, DEPTH_AT_MOST.get(name, MIN_DEPTH))


def labels_of(pop):
    """(labels, n_groups) of every by-group comparison: _household_ref.labels, which follow neither households nor places."""
    return hh.labels(pop, N_GROUPS), N_GROUPS


# ---- the references of a case, once per session ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cached(name, permuted=False):
    """A namespace of the case on the world (or its permuted copy): pop, ep, n, labels, n_groups and the references --
    sref (settings), tref (tree), chains, sus (sus_until), households, jm (all_pairs), flows / imports / invasion (whole run, all
    settings), event_world, contact_obs / contact_rule (by the labels) / contact_rule_all (one cell) / contact_seen,
    place_outbreaks {kind}, status_rows (by home area, [n, n_areas, 5]); pairs(first, last, n_groups) and
    place_pairs(kind, first, last, n_groups) count the attack-rate tables."""
    pop = permuted_world() if permuted else world()
    ep = params_of(name)
    sref = setting.reference(pop, ep, N)
    tref = tree.reference(pop, ep, N, sref)
    lab, g = labels_of(pop)
    sus = hh.sus_until(pop, ep, N)
    jm = hh.all_pairs(tref, pop)
    obs, seen = contact.walk(pop, ep, N, tref, lab, g)
    rule = contact.rule(pop, ep, N, tref, lab, g, seen["vax"], seen["buses"], seen["world"])
    rule_all = contact.rule(pop, ep, N, tref, contact.labels_of(pop, 1), 1, seen["vax"], seen["buses"], seen["world"])
    prepared = (pop, ep, N, tref, sus)

    def pairs(first=0, last=None, n_groups=0):
        if n_groups:
            return hh.pairs(tref, pop, ep, sus, first, last, hh.labels(pop, n_groups), n_groups, jm=jm)
        return hh.pairs(tref, pop, ep, sus, first, last, jm=jm)

    def place_pairs(kind, first=0, last=None, n_groups=0):
        return place.pairs_counting(prepared, kind, first, last, n_groups)

    return types.SimpleNamespace(
        name=name, pop=pop, ep=ep, n=N, labels=lab, n_groups=g, sref=sref, tref=tref, chains=chain.chains(tref, pop), sus=sus,
        households=hh.households(tref, pop), jm=jm, pairs=pairs, event_world=event.world_of(pop, ep, N, tref),
        flows=flow.flows(tref, pop), imports=flow.imports(tref, pop), invasion=flow.invasion(tref, pop),
        contact_obs=obs, contact_rule=rule, contact_rule_all=rule_all, contact_seen=seen,
        place_outbreaks={kind: place.outbreaks(tref, pop, kind) for kind in ("work", "school")}, place_pairs=place_pairs,
        status_rows=curve.reference_rows(pop, ep, N, "home")["status_rows"])


def busiest_step(w):
    """The step with the most exposures (1 in a run without one)."""
    st = w.tref["step"]
    return int(np.bincount(st[st > 0]).argmax()) if (st > 0).any() else 1


def inner_window(w):
    """A window inside the run that holds its busiest step."""
    busy = busiest_step(w)
    return max(1, busy - 30), min(w.n, busy + 30)


def cohort_window(w):
    """A window of cohort steps for the attack rates: early enough that its cases are infectious well inside the run."""
    return w.n // 8, w.n // 2


def facts(w):
    """What the guards of the replays read off a case's references: exposures per setting, ties, frozen-bus households,
    vaccinated housemates, the deepest generation, commuters (a work place in another area) exposed in a building with the
    at-work bit on and off."""
    s, t = w.sref, w.tref
    exposed = s["step"] > 0
    gen = t["generation"][exposed & (t["generation"] != tree.NONE)]
    pop = w.pop
    area = pop.building_area
    commuter = (pop.work_building != pop.home_building) & (area[pop.work_building] != area[pop.home_building])
    at_work = contact.bits(w.ep, s["records"], w.n)[0][s["step"]]
    in_building = exposed & commuter & (s["setting"] != T)
    return dict(commuters_at_work=int((in_building & at_work).sum()), commuters_at_home=int((in_building & ~at_work).sum()),
                per_setting=[int((exposed & (s["setting"] == k)).sum()) for k in (H, W, S, T)], exposures=int(exposed.sum()),
                ties=int((s["home_ok"] & s["work_ok"]).sum()), bus_frozen=int(s["bus_frozen"].sum()),
                housemate_vaccinated=int(s["housemate_vaccinated"].sum()), depth=int(gen.max(initial=0)))
