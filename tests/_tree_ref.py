"""Expected infector, candidate count and generation of every exposure, computed with numpy from the CPU oracle.  Test
infrastructure only.

The oracle is stepped one step at a time, as _setting_ref.reference steps it.  Its state before a step gives who is Infected
after that step's tick, its state after the step where everybody stands and who is on a bus.  The setting and building of
every exposure are those of _setting_ref (the tie rule included); the candidates are the Infected standing where the exposure is
credited -- the residents at home, the workers of the work building in it, the participants of the citizen's own room in the
school, the Infected riders of the citizen's bus -- in ascending citizen index.  The bus order comes from orc_philox4x32_10 over
(global citizen, step, slot 3, 0), the pick from orc_u32(seed, global citizen, step, 5).  The worlds are those of _setting_ref
and one more, built for a route that is longer than the kernels keep in LDS."""
import ctypes as C
import functools

import numpy as np

import _oracle
import _setting_ref as ref_mod
from epidemicsimulator_amd import Population, _lib

SLOT_BUS_ORDER, SLOT_INFECTOR = 3, 5
NONE = 0xFFFFFFFF
H, W, S, T = _lib.SETTING_HOUSEHOLD, _lib.SETTING_WORKPLACE, _lib.SETTING_SCHOOL, _lib.SETTING_TRANSPORT
_u32p = C.POINTER(C.c_uint32)


def _groups(key, use):
    """{key value: ascending citizen indices} over the citizens where `use` holds."""
    who = np.flatnonzero(use)
    order = who[np.argsort(key[who], kind="stable")]
    vals, starts = np.unique(key[order], return_index=True)
    return dict(zip(vals.tolist(), np.split(order, starts[1:])))


def bus_keys(seed, ids, step):
    philox = _oracle.lib().orc_philox4x32_10
    key = (C.c_uint32 * 2)(seed & 0xFFFFFFFF, seed >> 32)
    out = (C.c_uint32 * 4)()
    keys = np.zeros(len(ids), np.uint32)
    for i, g in enumerate(ids.tolist()):
        philox((C.c_uint32 * 4)(g, step, SLOT_BUS_ORDER, 0), key, out)
        keys[i] = out[0]
    return keys


def reference(pop, ep, n_steps, sref, switch=None):
    """sref: _setting_ref.reference of the same run.  switch: None, or (T, ep_b) as there.  Returns a dict of per-citizen arrays:
    infector, n_candidates, generation, step, setting, and of every exposure the size of the member list walked (list_size),
    for a transport exposure the buses of its route (n_buses); empty: exposures without a candidate; not_infected: infectors
    that the exposure steps alone do not make Infected in the step."""
    n = pop.n_citizens
    home, work, room = pop.home_building.astype(np.int64), pop.work_building.astype(np.int64), pop.room.astype(np.int64)
    area = pop.building_area.astype(np.int64)
    has_work = work != home
    school = has_work & (pop.building_type[work] == _lib.SCHOOL)
    rides = (pop.flags & _lib.FLAG_USES_PUBLIC_TRANSPORT) != 0
    route_key = area[home] * (int(area.max()) + 1) + area[work]
    residents, workers = _groups(home, np.ones(n, bool)), _groups(work, has_work & ~school)
    rooms, routes = _groups(room, school), _groups(route_key, rides)
    orc = _oracle.Oracle(pop, _oracle.params_from_esim(ep))
    u32 = _oracle.lib().orc_u32
    cur_ep = ep
    et, it, cap = int(ep.exposed_time), int(ep.infected_time), int(ep.bus_capacity)
    infector, n_cand, gen = np.full(n, NONE, np.uint32), np.zeros(n, np.uint32), np.full(n, NONE, np.uint32)
    list_size, n_buses = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    exp_step = np.full(n, -10 ** 9, np.int64)
    exp_step[pop.seeds] = -(et + 1)                                   # Infected from step 1
    gen[pop.seeds] = 0
    empty = not_infected = 0
    setting = sref["setting"]
    prev = orc.state()
    for s in range(1, n_steps + 1):
        if switch is not None and s == switch[0] + 1:
            cur_ep = switch[1]
            C.memmove(orc.h, C.byref(_oracle.params_from_esim(cur_ep)), C.sizeof(_oracle.Params))
        orc.step()
        state = orc.state()
        infected = ((prev["status"] == _lib.EXPOSED) & (prev["timer"] >= et)) | ((prev["status"] == _lib.INFECTED) & (prev["timer"] < it))
        cur, on_bus = state["current_building"].astype(np.int64), state["on_bus"] != 0
        in_building = infected & ~on_bus
        seed = int(cur_ep.seed)
        keys = {}
        step, _ = orc.exposures()
        for c in np.flatnonzero(step == s).tolist():
            exp_step[c] = s
            se = int(setting[c])
            if se == H:
                members = residents[int(home[c])]
                cand = members[in_building[members] & (cur[members] == home[c])]
            elif se == W:
                members = workers[int(work[c])]
                cand = members[in_building[members] & (cur[members] == work[c])]
            elif se == S:
                members = rooms[int(room[c])]
                cand = members[in_building[members] & (cur[members] == work[c])]
            elif se == T:
                members = routes[int(route_key[c])]
                aboard = infected[members] & on_bus[members]
                n_buses[c] = (len(members) + cap - 1) // cap
                if len(members) > cap:
                    r = int(route_key[c])
                    if r not in keys:
                        k = bus_keys(seed, members + pop.citizen_id_base, s)
                        rank = np.empty(len(members), np.int64)
                        rank[np.lexsort((np.arange(len(members)), k))] = np.arange(len(members))
                        keys[r] = rank // cap
                    bus = keys[r]
                    aboard &= bus == bus[np.searchsorted(members, c)]
                cand = members[aboard]
            else:
                continue
            list_size[c] = len(members)
            n_cand[c] = len(cand)
            if len(cand) == 0:
                empty += 1
                continue
            u = int(u32(seed, c + pop.citizen_id_base, s, SLOT_INFECTOR))
            j = int(cand[(u * len(cand)) >> 32])
            infector[c] = j
            if gen[j] != NONE:
                gen[c] = gen[j] + 1
            if not exp_step[j] + et + 1 <= s <= exp_step[j] + et + 1 + it:
                not_infected += 1
        prev = state
    orc.close()
    return dict(infector=infector, n_candidates=n_cand, generation=gen, step=sref["step"], setting=setting, list_size=list_size, n_buses=n_buses,
                empty=empty, not_infected=not_infected, n_steps=n_steps, records=sref["records"])


def cohort_step(ref, pop):
    """The exposure step per citizen as the cohorts count it: 0 for an index case, -1 for a citizen never exposed."""
    st = ref["step"].astype(np.int64)
    st[st == 0] = -1
    st[pop.seeds] = 0
    return st


def offspring(ref, pop, first_step, last_step):
    keep = (ref["infector"] != NONE) & (ref["step"] >= first_step) & (ref["step"] <= last_step)
    return np.bincount(ref["infector"][keep], minlength=pop.n_citizens).astype(np.uint32)


def reproduction_rows(ref, pop, where, first_step=0, n_rows=None, stride=24, labels=None, n_groups=0):
    """(cases, offspring) as esim_reproduction_series returns them, from a reference()."""
    n_steps = ref["n_steps"]
    if n_rows is None:
        n_rows = (n_steps - first_step) // stride + 1
    n_cols = {"all": 1, "home": pop.n_areas, "group": n_groups}[where]
    col = np.zeros(pop.n_citizens, np.int64) if where == "all" else pop.building_area[pop.home_building].astype(np.int64) if where == "home" else labels.astype(np.int64)
    st = cohort_step(ref, pop)
    row = (st - first_step) // stride
    inside = (st >= first_step) & (st <= n_steps) & (row < n_rows)
    cases, off = np.zeros((n_rows, n_cols), np.uint32), np.zeros((n_rows, n_cols), np.uint32)
    np.add.at(cases, (row[inside], col[inside]), 1)
    src = ref["infector"][ref["infector"] != NONE].astype(np.int64)
    src = src[inside[src]]
    np.add.at(off, (row[src], col[src]), 1)
    return cases, off


def mixing_matrix(ref, pop, labels, n_groups, mask=0xF, first_step=1, last_step=None):
    last_step = ref["n_steps"] if last_step is None else last_step
    se = ref["setting"]
    keep = (ref["infector"] != NONE) & (se < 4) & (((mask >> np.minimum(se, 4).astype(np.int64)) & 1) != 0) & (ref["step"] >= first_step) & (ref["step"] <= last_step)
    out = np.zeros((n_groups, n_groups), np.uint32)
    np.add.at(out, (labels[ref["infector"][keep]].astype(np.int64), labels[keep].astype(np.int64)), 1)
    return out


def bus_world():
    """Two areas, nine of ten citizens on public transport: the route between the two areas has 2 693 riders in 135 buses, more
    than the 2 048 whose keys a wavefront keeps, and dozens of them are Infected at a time."""
    pop = Population.synthetic("york", n_citizens=3000, n_areas=2, citizens_per_school=1500, n_seeds=20, p_public_transport=0.9)
    ep = _lib.default_params(exposure_chance=0.01, exposed_time=24, infected_time=120, lockdown_threshold=2.0, vaccination_threshold=2.0,
                             mask_pt_threshold=2.0, seed=9, max_steps=300)
    return pop, ep, 200


@functools.lru_cache(maxsize=None)
def cached(name):
    """(population, parameters, steps, reference) of a world, computed once per session."""
    if name == "bus":
        pop, ep, n = bus_world()
        return pop, ep, n, reference(pop, ep, n, ref_mod.reference(pop, ep, n))
    pop, ep, n, sref = ref_mod.cached(name)
    switch = None
    if name in ("rollback", "rollback_chance"):
        _, a, t, b, _ = ref_mod.rollback_world()
        switch = (t, b if name == "rollback" else ref_mod.copy_params(a, exposure_chance=b.exposure_chance))
    return pop, ep, n, reference(pop, ep, n, sref, switch)


WORLDS = ("fixture_a", "ties", "as_u8", "school", "situations", "bus")
ALL_WORLDS = WORLDS + ("permuted", "rollback", "rollback_chance", "rollback_straight")
