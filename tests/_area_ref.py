"""Expected per-Output-Area tables, computed with numpy from the CPU oracle. Test infrastructure only.

The oracle is stepped one step at a time; after every step its per-citizen state gives the Infected row of that step
(citizens Infected, by the area of the building they stand in), and at the steps asked for the whole census table.  The
exposure rows come from `Oracle.exposures()`: the (step, area) of every citizen's add_exposure call, area 0xFFFFFFFF for
public transport, which no row holds."""
import numpy as np

import _oracle
from epidemicsimulator_amd import Population, _lib

BUS_AREA = 0xFFFFFFFF
FIXTURE_A_STEPS = 700


def fixture_a():
    """The world of smoke(): population and esim_params."""
    pop = Population.synthetic("york", n_citizens=20000, n_areas=64, citizens_per_school=5000, n_seeds=20)
    ep = _lib.default_params(exposure_chance=0.004, vaccination_threshold=0.01, lockdown_threshold=0.02, seed=123)
    return pop, ep


def permuted(pop, seed=2024):
    """The same world with its citizens renumbered by a fixed permutation: new citizen k is old citizen perm[k]."""
    perm = np.random.default_rng(seed).permutation(pop.n_citizens)
    inverse = np.empty_like(perm)
    inverse[perm] = np.arange(pop.n_citizens)
    arrays = dict(home_building=pop.home_building[perm], work_building=pop.work_building[perm], room=pop.room[perm],
                  flags=pop.flags[perm], age=pop.age[perm], occupation=pop.occupation[perm],
                  building_area=pop.building_area, building_type=pop.building_type, room_building=pop.room_building,
                  seeds=inverse[pop.seeds].astype(np.uint32), n_areas=pop.n_areas)
    return Population(**arrays)


def census_table(pop, state, where):
    """counts[area, status] of a per-citizen state: where = "current" or "home"."""
    bld = state["current_building"] if where == "current" else pop.home_building
    key = pop.building_area[bld].astype(np.int64) * 5 + state["status"]
    return np.bincount(key, minlength=pop.n_areas * 5).reshape(pop.n_areas, 5).astype(np.uint32)


def exposure_rows(pop, step, area, n_steps):
    """rows[s - 1, a] = building exposures of step s credited to area a."""
    rows = np.zeros((n_steps, pop.n_areas), np.uint32)
    keep = (step >= 1) & (step <= n_steps) & (area != BUS_AREA)
    np.add.at(rows, (step[keep].astype(np.int64) - 1, area[keep].astype(np.int64)), 1)
    return rows


def nonzero_lists(rows):
    """{area: [non-zero entries of its column, in step order]} -- the shape of exposures.json's "OutputArea"."""
    out = {}
    for a in np.flatnonzero(rows.any(axis=0)).tolist():
        col = rows[:, a]
        out[a] = col[col != 0].tolist()
    return out


def reference_tables(pop, ep, n_steps, census_steps=()):
    """Steps the oracle n_steps times.  Returns a dict: records, infected_rows [n_steps, n_areas], exposure_rows
    [n_steps, n_areas], census {step: {"current": table, "home": table}}, final_state, exposures (step, area)."""
    orc = _oracle.Oracle(pop, _oracle.params_from_esim(ep))
    records = np.zeros(n_steps, _oracle.RECORD_DTYPE)
    infected = np.zeros((n_steps, pop.n_areas), np.uint32)
    census = {}
    state = None
    for s in range(1, n_steps + 1):
        records[s - 1] = orc.step()
        state = orc.state()
        area = pop.building_area[state["current_building"]]
        infected[s - 1] = np.bincount(area[state["status"] == _lib.INFECTED], minlength=pop.n_areas)
        if s in census_steps:
            census[s] = {w: census_table(pop, state, w) for w in ("current", "home")}
    step, area = orc.exposures()
    orc.close()
    return {"records": records, "infected_rows": infected, "exposure_rows": exposure_rows(pop, step, area, n_steps),
            "census": census, "final_state": state, "exposures": (step, area)}
