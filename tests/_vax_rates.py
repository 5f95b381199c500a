"""Vaccination rates of thousands, up to the limit of 8192 a step: the rejection walk over the Philox candidate sequence where
one batch of candidates cannot suffice, the hash set fills to more than half, and the cut at the rate falls in a second or later
batch.  The walk lives three times on the device (finish_phase, k_chunk_vax, k_area_vax_replay) and twice more sharded;
tests/test_vax_rates.py checks on the CPU that every case reaches its regime, tests/test_vax_rates_gpu.py runs the cases in
every execution form and through the replays.  Importing this module and reading its tables needs neither libesim.so nor a
device: the worlds call the library's population builder (host code), trace() the CPU oracle.

The two worlds are the smallest that hold the regimes: the eligible set has to exceed rate + riders (the plan condition of
k_chunk_vax) after the epidemic has made thousands ineligible."""
import functools
import os
import re

import numpy as np

import _oracle
from epidemicsimulator_amd import Population, _lib

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "epidemicsimulator_amd", "csrc")


def device_constant(name):
    """The value of `#define name <number>u` in esim_device.h, read as text: the tests follow the kernels' sizes, not a copy."""
    text = open(os.path.join(CSRC, "esim_device.h")).read()
    found = re.findall(r"^#define\s+%s\s+(\d+)u?\b" % re.escape(name), text, re.M)
    assert len(found) == 1, (name, found)
    return int(found[0])


VACC_BATCH = device_constant("VACC_BATCH")
VACC_TABLE = device_constant("VACC_TABLE")
VACC_MAX_RATE = device_constant("VACC_MAX_RATE")
VACC_WINDOW = device_constant("VACC_WINDOW")
PLAN_W = device_constant("PLAN_W")
FREE_MAX = device_constant("FREE_MAX")

BLOCK = 67               # steps of a block of the parity runs: no multiple of a Philox block of four steps nor of a chunk of 96
S, E, I, R, V = 0, 1, 2, 3, 4                                   # the oracle's status codes (esim.h)

BASE = dict(exposure_chance=0.01, lockdown_threshold=0.3, mask_pt_threshold=0.02, mask_everywhere_threshold=0.05,
            bus_capacity=20, seed=0x9E3779B97F4A7C15)

WORLDS = {
    "W40": dict(n_citizens=40000, n_areas=64, citizens_per_school=5000, n_seeds=40, p_public_transport=0.2),
    "W24": dict(n_citizens=24000, n_areas=40, citizens_per_school=4000, n_seeds=24, p_public_transport=0.2),
}
RIDERS = {"W40": 8004, "W24": 4909}                             # (tests/test_vax_rates.py checks them)


@functools.lru_cache(maxsize=None)
def world(name):
    return Population.synthetic("york", **WORLDS[name])


# The town of the seams between the two arms of the choice (test_vax_rates_gpu.py e.): under BASE and vaccination_threshold 0.05 the
# programme starts at step TOWN_TRIGGER with TOWN_ELIGIBLE citizens eligible, and no bus takes one of them afterwards -- a rate of
# exactly TOWN_ELIGIBLE takes the whole-set arm by equality (eligible_count <= rate), a lower one walks
TOWN = dict(n_citizens=9000, n_areas=16, citizens_per_school=3000, n_seeds=20, p_public_transport=0.2)
TOWN_TRIGGER, TOWN_ELIGIBLE, TOWN_THRESHOLD = 186, 6287, 0.05


@functools.lru_cache(maxsize=None)
def town():
    return Population.synthetic("york", **TOWN)


def n_riders(pop):
    return int(((pop.flags & 1) != 0).sum())


class Case:
    """trigger: the step whose decision starts the programme (the first step that vaccinates).  batches / slots: what the
    walk must reach in some step at least (the issue's table: most batches per step, most table slots used).  plans: whether
    elig_all > rate + riders, the condition under which k_chunk_vax plans a chunk, holds in every step under the programme or
    in none."""

    def __init__(self, world, rate, threshold, steps, trigger, eligible, batches, slots, plans, **over):
        self.world, self.rate, self.steps, self.trigger, self.eligible = world, rate, steps, trigger, eligible
        self.batches, self.slots, self.plans = batches, slots, plans
        self.over = dict(over, vaccination_rate=rate, vaccination_threshold=threshold)

    @property
    def params(self):
        return dict(BASE, **self.over)

    @property
    def pop(self):
        return world(self.world)


CASES = {
    "rate_1024": Case("W40", 1024, 0.05, 400, 226, 29801, 1, 2971, True),
    "rate_4095": Case("W40", 4095, 0.05, 400, 226, 29801, 2, 5616, True),
    "rate_4096": Case("W40", 4096, 0.05, 400, 226, 29801, 2, 5616, True),
    "rate_4097": Case("W40", 4097, 0.05, 400, 226, 29801, 2, 5616, True),
    "rate_8191": Case("W40", 8191, 0.05, 400, 226, 29801, 4, 10141, True),
    "rate_8192_early": Case("W40", 8192, 0.02, 400, 183, 33953, 3, 9144, True),
    "rate_8192_late": Case("W40", 8192, 0.26, 450, 324, 17282, 7, 8988, True, lockdown_threshold=0.9),
    "rate_8192_no_plan": Case("W24", 8192, 0.15, 400, 301, 11943, 7, 8418, False),
}
# what the issue asks of the table's rows at the least
MIN_BATCHES = {"rate_1024": 1, "rate_4095": 2, "rate_4096": 2, "rate_4097": 2, "rate_8191": 3, "rate_8192_early": 3,
               "rate_8192_late": 7, "rate_8192_no_plan": 7}
MIN_SLOTS = {"rate_8191": 9000, "rate_8192_early": 9000}
REPLAYED = ("rate_1024", "rate_4097", "rate_8192_early", "rate_8192_late")     # the cases whose replays are compared


def params_of(name):
    return _lib.default_params(**CASES[name].params)


# ---- Philox and the candidate sequence, restated in numpy -----------------------------------------------------------------------
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_LOW = np.uint64(0xFFFFFFFF)
_32 = np.uint64(32)


def philox4x32_10(c0, c1, c2, c3, seed):
    """Philox4x32-10 as orc_philox4x32_10 computes it, over arrays of counters (uint64 arrays that hold 32-bit values)."""
    c0, c1, c2, c3 = (np.asarray(c, np.uint64) & _LOW for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> _32) ^ c1 ^ np.uint64(k0), p1 & _LOW, (p0 >> _32) ^ c3 ^ np.uint64(k1), p0 & _LOW
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def candidates(seed, step, first, count, n):
    """Candidates first .. first + count - 1 of the step: block (i, step, 4, 0), mulhi64(w0 << 32 | w1, n)."""
    w0, w1, _, _ = philox4x32_10(np.arange(first, first + count, dtype=np.uint64), step, 4, 0, seed)
    n = np.uint64(n)
    return ((w0 * n + ((w1 * n) >> _32)) >> _32).astype(np.int64)       # (w0 * n + 2^32 - 1 < 2^64 for n < 2^32)


def walk_step(seed, step, eligible, rate):
    """One step's walk over the eligible set as it stands when the step chooses: batches of VACC_BATCH candidates until `rate`
    distinct eligible citizens were met.  (chosen in candidate order, candidates read, batches, distinct live keys inserted by
    the end of the last batch -- the whole of the last batch is inserted, also behind the cut)."""
    n = len(eligible)
    seen = np.zeros(n, bool)
    firsts, batches = [], 0
    have = 0
    while have < rate:
        j = candidates(seed, step, batches * VACC_BATCH, VACC_BATCH, n)
        batches += 1
        j = j[eligible[j]]
        _, idx = np.unique(j, return_index=True)
        j = j[np.sort(idx)]                                             # first occurrences inside the batch, in candidate order
        j = j[~seen[j]]                                                 # ... and across the batches of the step
        seen[j] = True
        firsts.append(j)
        have += len(j)
    firsts = np.concatenate(firsts)
    return firsts[:rate], batches * VACC_BATCH, batches, len(firsts)


# ---- the oracle's run of a case, step by step ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def trace(name):
    """The oracle's run of the case with what the guards and walk() need of every step: records [steps], and from the step
    before the trigger on the status and the eligible flags after every step (status[i], eligible[i]: after step first + i);
    the state at the end of every block of BLOCK steps, as OracleRun keeps it."""
    case = CASES[name]
    pop = case.pop
    orc = _oracle.Oracle(pop, _oracle.params_from_esim(params_of(name)))
    orc.set_threads(4)
    first = case.trigger - 1
    records, states, status, eligible = [], [], [], []
    done = 0
    while done < case.steps:
        n = min(BLOCK - done % BLOCK, case.steps - done, first - done) if done < first else 1
        records.append(orc.run(n))
        done += n
        if done >= first or done % BLOCK == 0:
            st = orc.state()
            if done % BLOCK == 0 or done == case.steps:
                states.append(st)
            if done >= first:
                status.append(st["status"]); eligible.append(st["eligible"] != 0)
    orc.close()
    return dict(records=np.concatenate(records), states=states, first=first, status=np.stack(status), eligible=np.stack(eligible))


class Run:
    """What test_parity_gpu.run_forms reads of an OracleRun, from the cached trace of a case."""

    def __init__(self, name):
        case, tr = CASES[name], trace(name)
        self.pop, self.params, self.block, self.stop, self.steps = case.pop, case.params, BLOCK, False, case.steps
        self.asked = [min(BLOCK, case.steps - a) for a in range(0, case.steps, BLOCK)]
        self.records = [tr["records"][a:a + n] for a, n in zip(range(0, case.steps, BLOCK), self.asked)]
        self.states = tr["states"]


def eligible_before_choice(tr, step):
    """The eligible set as step `step` chooses from it: the set left by the step before (at the trigger: the Susceptible of
    that moment, which the oracle's flags after the trigger step show -- a choice removes nobody from the set), without the
    citizens the step's own buses took out of it -- which are out of the flags after the step as well."""
    return tr["eligible"][step - tr["first"]]


@functools.lru_cache(maxsize=None)
def walk(name):
    """The numpy restatement of the walk over the oracle's eligible sets: a list, one entry per step under the programme, of
    dict(step, chosen, read, batches, slots)."""
    case, tr = CASES[name], trace(name)
    out = []
    for step in range(case.trigger, case.steps + 1):
        chosen, read, batches, slots = walk_step(case.params["seed"], step, eligible_before_choice(tr, step), case.rate)
        out.append(dict(step=step, chosen=chosen, read=read, batches=batches, slots=slots))
    return out
