"""Expected tables of esim_area_status_series, computed with numpy from the CPU oracle. Test infrastructure only.

By household area: the population's home area is a label like any other, so tests/_group_ref.py gives the status rows and the
exposure rows (buildings and public transport, the initially infected citizens not).  By the area stood in: the oracle is
stepped one step at a time and tests/_area_ref.py's census table of its state taken after every step."""
import functools

import numpy as np

import _area_ref
import _group_ref
import _oracle

STATUS = ("susceptible", "exposed", "infected", "recovered", "vaccinated")
TABLES = [(where, what) for where in ("home", "current") for what in STATUS] + [("home", "incidence")]      # all eleven


def home_area_labels(pop):
    return pop.building_area[pop.home_building].astype(np.uint16)


def reference_tables(pop, ep, n_steps):
    """Returns a dict: records, home [n_steps, n_areas, 5] and current [n_steps, n_areas, 5] (the census after every step),
    incidence [n_steps, n_areas], final_state."""
    assert pop.n_areas <= 1024
    g = _group_ref.reference_tables(pop, ep, home_area_labels(pop), pop.n_areas, n_steps)
    orc = _oracle.Oracle(pop, _oracle.params_from_esim(ep))
    current = np.zeros((n_steps, pop.n_areas, 5), np.uint32)
    for s in range(1, n_steps + 1):
        orc.step()
        current[s - 1] = _area_ref.census_table(pop, orc.state(), "current")
    orc.close()
    return {"records": g["records"], "home": g["status_rows"], "current": current, "incidence": g["exposure_rows"],
            "final_state": g["final_state"]}


@functools.lru_cache(maxsize=None)
def fixture_a_tables():
    """(pop, ep, reference tables) of tests/_area_ref.py's fixture A over its 700 steps, computed once per session."""
    pop, ep = _area_ref.fixture_a()
    return pop, ep, reference_tables(pop, ep, _area_ref.FIXTURE_A_STEPS)


def expected(ref, where, what, t_done, first_step=1, n_rows=None, stride=1):
    """The table the library must return for (where, what) after t_done steps, from tables that cover at least those steps."""
    if n_rows is None:
        n_rows = (t_done - first_step) // stride + 1
    if what == "incidence":
        full = ref["incidence"][:t_done]
        out = np.zeros((n_rows, full.shape[1]), np.uint32)
        for i in range(n_rows):
            lo = first_step + i * stride
            out[i] = full[lo - 1:lo - 1 + stride].sum(axis=0)
        return out
    return ref[where][first_step - 1:t_done:stride, :, STATUS.index(what)][:n_rows]
