"""Expected arrival-time tables, computed with numpy from the CPU oracle. Test infrastructure only.

`Oracle.exposures()` gives the step of every citizen's add_exposure call (0 = none; buildings and public transport alike).
The arrival step of a key -- the Output Area of the citizen's household, or its label -- is the smallest such step among its
citizens; a key that holds an initially infected citizen has 0, a key nobody of which was exposed NEVER."""
import numpy as np

import _oracle

NEVER = 0xFFFFFFFF


def home_area(pop):
    return pop.building_area[pop.home_building].astype(np.int64)


def arrival(keys, n_keys, step, seeds, upto=None):
    """uint32 [n_keys].  keys: one per citizen; step: Oracle.exposures()[0]; seeds: the initially infected citizens; upto:
    only the steps 1..upto count (None: all) -- the table as it stood after step `upto` of the same run."""
    keys, step = np.asarray(keys).astype(np.int64), np.asarray(step).astype(np.int64)
    out = np.full(n_keys, NEVER, np.uint32)
    hit = step >= 1
    if upto is not None:
        hit &= step <= upto
    np.minimum.at(out, keys[hit], step[hit].astype(np.uint32))
    out[keys[np.asarray(seeds, np.int64)]] = 0
    return out


def oracle_run(pop, ep, n_steps):
    """(records, step of every citizen's exposure, final state) of a fresh oracle run."""
    orc = _oracle.Oracle(pop, _oracle.params_from_esim(ep))
    orc.set_threads(16)
    rec = orc.run(n_steps)
    step, _ = orc.exposures()
    state = orc.state()
    orc.close()
    return rec, step, state
