"""Expected work place and school outbreaks of a run -- members, cases, introductions and first step per place, the two size
tables and the pair tables of the secondary attack rate --, computed with numpy on top of _household_ref.cached(name): the tree
reference and sus_until from the oracle's states, nothing derived twice.  Test infrastructure only.

The pairs have two independent references: a brute-force outer product (cases x members of every place, used only for places
of at most OUTER_MAX members) and a counting one (per place the sorted susceptible ends of its members, group by group, and a
searchsorted per case).  The world `edge` lives here: places at the sizes at which k_place_sar takes another path."""
import functools
import os
import re

import numpy as np

import _household_ref as hh
import _setting_ref as ref_mod
import _tree_ref as tree
from epidemicsimulator_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFF
BINS = 32
OUTER_MAX = 300
KINDS = ("work", "room", "school")
OWN = {"work": _lib.SETTING_WORKPLACE, "room": _lib.SETTING_SCHOOL, "school": _lib.SETTING_SCHOOL}
WORLDS = ("edge", "school", "ties", "fixture_a", "situations", "bus", "deep")


def header_tile():
    """PLACE_TILE as the kernels' header defines it."""
    text = open(os.path.join(ROOT, "epidemicsimulator_amd", "csrc", "esim_kernels_places.h")).read()
    return int(re.search(r"^#define PLACE_TILE (\d+)u$", text, re.M).group(1))


TILE = 2048                                  # mirrors PLACE_TILE (test_place_outbreaks.py compares it with header_tile())
EDGE_WORK = (1, 2, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1, 2 * TILE + 1)
EDGE_ROOMS = (1, 2, 63, 64, 65, 300)
EDGE_IDLE = 505


def edge_world():
    """One area, households of four with citizen i in household i % n_households.  Work places of EDGE_WORK workers -- around a
    wavefront, around a workgroup's stretch, around one tile and beyond two --, one school with rooms of EDGE_ROOMS, EDGE_IDLE
    citizens without a work place; the citizens of a place are neighbours in the order of the citizens.  The first member of
    every place starts Infected."""
    sizes = EDGE_WORK + EDGE_ROOMS
    n = sum(sizes) + EDGE_IDLE
    assert n % 4 == 0
    n_hh = n // 4
    school = n_hh + len(EDGE_WORK)
    home = np.arange(n) % n_hh
    work, room, seeds = home.copy(), np.full(n, _lib.NO_ROOM, np.int64), []
    at = 0
    for k, size in enumerate(sizes):
        seeds.append(at)
        if k < len(EDGE_WORK):
            work[at:at + size] = n_hh + k
        else:
            work[at:at + size], room[at:at + size] = school, k - len(EDGE_WORK)
        at += size
    btype = [_lib.HOUSEHOLD] * n_hh + [_lib.WORKPLACE] * len(EDGE_WORK) + [_lib.SCHOOL]
    pop = ref_mod._by_hand(home, work, np.zeros(n), np.zeros(len(btype)), btype, seeds, room=room, room_building=[school] * len(EDGE_ROOMS))
    ep = _lib.default_params(exposure_chance=0.0005, exposed_time=4, infected_time=30, start_hour=1, end_hour=23, vaccination_threshold=2.0,
                             lockdown_threshold=2.0, mask_pt_threshold=2.0, seed=17, max_steps=100)
    return pop, ep, 40


@functools.lru_cache(maxsize=None)
def cached(name):
    """(population, parameters, steps, tree reference, sus_until, settings reference or None) of a world, once per session."""
    if name == "edge":
        pop, ep, n = edge_world()
        sref = ref_mod.reference(pop, ep, n)
        return pop, ep, n, tree.reference(pop, ep, n, sref), hh.sus_until(pop, ep, n), sref
    pop, ep, n, ref, sus, _ = hh.cached(name)
    return pop, ep, n, ref, sus, ref_mod.cached(name)[3] if name in ref_mod.WORLDS else None


def place_of(pop, kind):
    """(place per citizen as int64, -1 for a citizen that is a member of none; number of places)."""
    home, work = pop.home_building.astype(np.int64), pop.work_building.astype(np.int64)
    has_work = work != home
    school = has_work & (pop.building_type[work] == _lib.SCHOOL)
    if kind == "work":
        return np.where(has_work & ~school, work, -1), pop.n_buildings
    if kind == "room":
        return np.where(school, pop.room.astype(np.int64), -1), pop.n_rooms
    return np.where(school, work, -1), pop.n_buildings


def bin_of(x):
    """The size bin of the tables (scalar or array)."""
    x = np.asarray(x, np.int64)
    log = np.floor(np.log2(np.maximum(x, 1))).astype(np.int64)
    return np.where(x < 16, x, np.minimum(BINS - 1, 12 + log))


def outbreaks(ref, pop, kind):
    """dict of per-place arrays: members, cases, introductions, first_step (NONE without a case)."""
    place, n_places = place_of(pop, kind)
    st = tree.cohort_step(ref, pop)
    member = place >= 0
    case = member & (st >= 0)
    intro = case & ((st == 0) | (ref["setting"] != OWN[kind]))
    first = np.full(n_places, NONE, np.int64)
    np.minimum.at(first, place[case], st[case])
    count = lambda which: np.bincount(place[which], minlength=n_places).astype(np.uint32)
    return dict(members=count(member), cases=count(case), introductions=count(intro), first_step=first.astype(np.uint32))


def sizes(ob):
    """(final_size, introduced) uint32 [32, 32] from outbreaks()."""
    real = ob["members"] > 0
    row = bin_of(ob["members"][real])
    out = []
    for k in ("cases", "introductions"):
        tab = np.zeros((BINS, BINS), np.uint32)
        np.add.at(tab, (row, bin_of(ob[k][real])), 1)
        out.append(tab)
    return tuple(out)


def _lists(pop, kind, max_members):
    """The member lists of the places of at most max_members members (None: all), as arrays of citizens."""
    place, n_places = place_of(pop, kind)
    order = np.argsort(place, kind="stable")
    order = order[place[order] >= 0]
    cuts = np.flatnonzero(np.diff(place[order])) + 1
    return [m for m in np.split(order, cuts) if len(m) and (max_members is None or len(m) <= max_members)]


def _setup(world, kind, first_step, last_step, n_groups):
    """world: the name of a cached world, or a (population, parameters, steps, tree reference, sus_until) tuple."""
    pop, ep, n, ref, sus = (cached(world) if isinstance(world, str) else world)[:5]
    last_step = n if last_step is None else last_step
    st, f = hh.first_infectious(ref, pop, ep)
    counted = (st >= first_step) & (st <= last_step) & (f <= n)
    g = max(1, n_groups)
    lab = hh.labels(pop, g).astype(np.int64) if n_groups else np.zeros(pop.n_citizens, np.int64)
    return pop, ref, sus, f, counted, lab, g


def pairs_outer(world, kind, first_step=0, last_step=None, n_groups=0, max_members=OUTER_MAX):
    """(at_risk, secondary) uint64 [n_cols, n_cols] over the places of at most max_members members: every (case, member) pair."""
    pop, ref, sus, f, counted, lab, g = _setup(world, kind, first_step, last_step, n_groups)
    at, sec = np.zeros((g, g), np.uint64), np.zeros((g, g), np.uint64)
    for mem in _lists(pop, kind, max_members):
        js = mem[counted[mem]]
        if not len(js):
            continue
        j, m = np.repeat(js, len(mem)), np.tile(mem, len(js))
        risk = (m != j) & (sus[m] >= f[j] - 1)
        hit = risk & (ref["infector"][m] == j) & (ref["setting"][m] == OWN[kind])
        np.add.at(at, (lab[j[risk]], lab[m[risk]]), 1)
        np.add.at(sec, (lab[j[hit]], lab[m[hit]]), 1)
    return at, sec


def pairs_counting(world, kind, first_step=0, last_step=None, n_groups=0, max_members=None):
    """The same by counting: per place and group of contact the sorted susceptible ends, a searchsorted per case; the secondary
    cases straight from the tree's edges."""
    pop, ref, sus, f, counted, lab, g = _setup(world, kind, first_step, last_step, n_groups)
    place, _ = place_of(pop, kind)
    at, sec = np.zeros((g, g), np.uint64), np.zeros((g, g), np.uint64)
    kept = np.zeros(pop.n_citizens, bool)
    for mem in _lists(pop, kind, max_members):
        kept[mem] = True
        js = mem[counted[mem]]
        if not len(js):
            continue
        need = f[js] - 1
        own = (sus[js] >= need).astype(np.int64)                      # a case at risk from itself would be counted below: taken off again
        for gm in range(g):
            ends = np.sort(sus[mem[lab[mem] == gm]])
            cnt = len(ends) - np.searchsorted(ends, need, side="left") - np.where(lab[js] == gm, own, 0)
            np.add.at(at[:, gm], lab[js], cnt.astype(np.uint64))
    m = np.flatnonzero((ref["infector"] != tree.NONE) & (ref["setting"] == OWN[kind]) & kept)
    j = ref["infector"][m].astype(np.int64)
    ok = (place[j] == place[m]) & counted[j] & (sus[m] >= f[j] - 1) & (j != m)
    np.add.at(sec, (lab[j[ok]], lab[m[ok]]), 1)
    return at, sec


@functools.lru_cache(maxsize=None)
def cached_outbreaks(name, kind):
    pop, ep, n, ref, sus, _ = cached(name)
    return outbreaks(ref, pop, kind)


@functools.lru_cache(maxsize=None)
def cached_pairs(name, kind, first_step=0, last_step=None, n_groups=0):
    """pairs_counting over all places of a cached world; n_groups 0: one cell, else by _household_ref.labels(pop, n_groups)."""
    return pairs_counting(name, kind, first_step, last_step, n_groups)


def windows(name):
    """The three windows of cohort steps the tests count in: the whole run, a stretch inside it, the busiest cohort step."""
    pop, ep, n, ref, sus, _ = cached(name)
    busy = int(np.bincount(ref["step"][ref["step"] > 0]).argmax())
    return ((0, n), (max(1, n // 3), n // 2), (busy, busy))
