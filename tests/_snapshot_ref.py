"""What the snapshot tests share: the two worlds, the parameter sets of a branch the oracle can follow, the step T the oracle
itself allows for it, and a checkpoint's bytes with the exposure log brought into a canonical order.  Test infrastructure only."""
import functools

import numpy as np

import _oracle
from epidemicsimulator_amd import Population, _lib
from test_ensemble_gpu import parity_world
from test_parity_gpu import AGGRESSIVE, random_population  # noqa: F401  (random_population: through parity_world)

N_STEPS = 500
FIELDS = [f for f in _lib.RECORD_FIELDS if f != "reserved"]

# Overrides that cannot act before an intervention does: the rate and the thresholds of interventions that start later under
# B than under A or not at all before them, and the masks' effectiveness, which no draw reads before a mask is worn.
BRANCH_B = {
    "parity": dict(vaccination_rate=25, vaccination_threshold=0.1, lockdown_threshold=0.07, mask_everywhere_threshold=0.05),
    "york": dict(vaccination_rate=100, vaccination_threshold=0.03, lockdown_threshold=0.05, mask_everywhere_threshold=0.02, mask_effectiveness=0.4),
}


@functools.lru_cache(maxsize=None)
def world(name):
    """(population, base parameters A) of random_population(5) / the 6000-citizen York of test_ensemble_gpu.py."""
    if name == "parity":
        pop, base, _ = parity_world()
        return pop, dict(base)
    pop = Population.synthetic("york", n_citizens=6000, n_areas=20, citizens_per_school=3000, n_seeds=12, p_public_transport=0.4)
    return pop, dict(AGGRESSIVE)


def oracle(name, overrides=()):
    pop, base = world(name)
    return _oracle.Oracle(pop, _oracle.params_from_esim(_lib.default_params(**dict(base, **dict(overrides)))))


@functools.lru_cache(maxsize=None)
def straight(name, branch=False):
    """The oracle's uninterrupted N_STEPS under A (or under A changed by BRANCH_B): records, final state, and every exposure as
    sorted (step, citizen, on_bus) rows -- what log_sets makes of a context's downloaded log."""
    orc = oracle(name, BRANCH_B[name] if branch else ())
    orc.set_threads(16)
    rec, state = orc.run(N_STEPS), orc.state()
    step, area = orc.exposures()
    orc.close()
    c = np.flatnonzero(step > 0)
    rows = np.stack([step[c].astype(np.int64), c.astype(np.int64), (area[c] == 0xFFFFFFFF).astype(np.int64)], 1)
    return rec, state, rows[np.lexsort((rows[:, 1], rows[:, 0]))]


@functools.lru_cache(maxsize=None)
def branch_step(name):
    """T for the branch under BRANCH_B: the last step up to which the oracle's records under A and under B agree in every
    field, minus 5 -- and whether the oracle's states under A and B after T steps are equal."""
    a, b = straight(name)[0], straight(name, True)[0]
    differ = np.zeros(N_STEPS, bool)
    for f in FIELDS:
        differ |= a[f] != b[f]
    agree = int(np.argmax(differ)) if differ.any() else N_STEPS          # records 1 .. agree are equal
    t = agree - 5
    same_state = False
    if t >= 1:
        oa, ob = oracle(name), oracle(name, BRANCH_B[name])
        oa.run(t), ob.run(t)
        sa, sb = oa.state(), ob.state()
        same_state = all((sa[k] == sb[k]).all() for k in sa)
        oa.close(), ob.close()
    return t, same_state, bool(differ.any())


def log_sets(sim):
    """The downloaded exposure log as one sorted array of (step, citizen, on_bus) rows: equal as sets per step iff equal."""
    cit, step, bus = sim.exposure_events()                           # (sorted by step, then citizen)
    return np.stack([step.astype(np.int64), cit.astype(np.int64), bus.astype(np.int64)], 1)


def checkpoint_parts(path, n_citizens):
    """A checkpoint file cut into its sections (esim_host_ckpt.h), the exposure log sorted inside every step: the order of the
    entries of one step is unspecified (they are appended through atomics), everything else is compared as it lies."""
    raw = np.fromfile(str(path), np.uint8)
    head_u32 = raw[:64].view(np.uint32)
    n, host_t, log_len, ctrl_bytes = int(head_u32[2]), int(head_u32[6]), int(head_u32[7]), int(head_u32[14])
    assert n == n_citizens
    slots, pos, parts = 8192, 128, {"header": raw[:128]}
    for key, nbytes in (("ctrl", ctrl_bytes), ("hist", 4 * slots), ("log_off", 4 * (slots + 1)), ("cit", 4 * n), ("log", 4 * log_len),
                        ("exp_step", 8 * (host_t + 1)), ("records", 64 * host_t)):
        parts[key] = raw[pos:pos + nbytes]
        pos += nbytes
    assert pos == raw.size
    log, off = parts["log"].view(np.uint32), parts["log_off"].view(np.uint32)
    slot = np.searchsorted(off, np.arange(log_len), side="right")
    parts["log"] = log[np.lexsort((log, slot))]
    return parts
