"""Expected results of the hospital-burden calls (esim_burden_*), computed with numpy from the CPU oracle. Test infrastructure only.

The oracle is stepped one step at a time.  The onset of a citizen is the first s in 0 .. t_done after which its status is
Infected (s = 0: the initial state), read off the oracle's state -- not derived from the exposure log's arithmetic.  The Philox
block of a case comes from the oracle library's orc_philox4x32_10 over the counter (global id, onset, SLOT_BURDEN, 0), as
tests/_tree_ref.py's bus_keys calls it.  Everything else is numpy over whole arrays."""
import ctypes as C
import functools

import numpy as np

import _curve_ref
import _group_ref
import _oracle
from epidemicsimulator_amd import Population, _lib

NEVER = 0xFFFFFFFF
SLOT_BURDEN = 6
WHERES = ("all", "home", "group")
WHATS = ("admissions", "occupancy", "deaths")
KEYS = ("peak", "peak_step", "steps_at_least", "first_at_least", "last_at_least", "bed_steps", "admissions", "deaths")


def percent(values):
    """uint32 thresholds of percentages, in integer arithmetic."""
    return np.array([min((int(p) << 32) // 100, 0xFFFFFFFF) for p in values], np.uint32)


def table_set_t():
    """Table set T: admission and death by the 8 age bands of _group_ref.AGE_EDGES, delays of 0 .. 6 days, stays of 1 .. 14 days."""
    return dict(admit_thr=percent((2, 2, 4, 8, 15, 30, 50, 70)), death_thr=percent((0, 0, 1, 2, 5, 10, 25, 50)),
                delay_cdf=percent(np.cumsum((5, 10, 20, 25, 20, 15))), delay_unit=24,
                stay_cdf=percent(np.cumsum((10, 15, 15, 12, 10, 8, 7, 6, 5, 4, 3, 2, 2))), stay_unit=24)


def oracle_run(pop, ep, n_steps):
    """Steps the oracle n_steps times: dict(onset [n] -- NEVER for a citizen never Infected after a step --, vax_exposed,
    vax_infected (citizens Vaccinated after a step that were Exposed / Infected after the one before), records, final_state,
    exposure_step (the step of the citizen's exposure in the oracle's log, 0: none))."""
    orc = _oracle.Oracle(pop, _oracle.params_from_esim(ep))
    n = pop.n_citizens
    before = orc.state()["status"].copy()
    onset = np.where(before == _lib.INFECTED, 0, NEVER).astype(np.int64)
    vax_e, vax_i = np.zeros(n, bool), np.zeros(n, bool)
    records = np.zeros(n_steps, _oracle.RECORD_DTYPE)
    state = None
    for s in range(1, n_steps + 1):
        records[s - 1] = orc.step()
        state = orc.state()
        after = state["status"]
        onset[(after == _lib.INFECTED) & (onset == NEVER)] = s
        now = after == _lib.VACCINATED
        vax_e |= now & (before == _lib.EXPOSED)
        vax_i |= now & (before == _lib.INFECTED)
        before = after.copy()
    exposure_step = orc.exposures()[0].astype(np.int64)
    orc.close()
    return dict(onset=onset, vax_exposed=vax_e, vax_infected=vax_i, records=records, final_state=state, exposure_step=exposure_step)


def blocks(seed_of, ids, onset):
    """uint32 [n, 4]: the raw Philox block of every (global id, onset) under seed_of(onset)."""
    philox = _oracle.lib().orc_philox4x32_10
    out, w = np.zeros((len(ids), 4), np.uint32), (C.c_uint32 * 4)()
    for i, (g, s) in enumerate(zip(np.asarray(ids).tolist(), np.asarray(onset).tolist())):
        seed = int(seed_of(s))
        philox((C.c_uint32 * 4)(g, s, SLOT_BURDEN, 0), (C.c_uint32 * 2)(seed & 0xFFFFFFFF, seed >> 32), w)
        out[i] = w[:]
    return out


def outcomes(onset, groups, tables, seed_of, id_base=0):
    """The outcome of every citizen with an onset (onset != NEVER), whatever the steps run: dict of [n] arrays -- case, block
    [n, 4], admitted, admit_step, end_step (int64; NEVER where not admitted), died."""
    onset = np.asarray(onset, np.int64)
    n = len(onset)
    case = onset != NEVER
    idx = np.flatnonzero(case)
    w = np.zeros((n, 4), np.uint32)
    w[idx] = blocks(seed_of, idx + id_base, onset[idx])
    k = np.asarray(groups, np.int64)
    admit_thr, death_thr = np.asarray(tables["admit_thr"], np.uint32), np.asarray(tables["death_thr"], np.uint32)
    delay_cdf, stay_cdf = np.asarray(tables["delay_cdf"], np.uint32), np.asarray(tables["stay_cdf"], np.uint32)
    admitted = case & (w[:, 0] < admit_thr[k])
    n_delay = (delay_cdf[None, :] <= w[:, 1][:, None]).sum(axis=1)
    n_stay = (stay_cdf[None, :] <= w[:, 2][:, None]).sum(axis=1)
    admit = onset + int(tables["delay_unit"]) * n_delay
    end = admit + int(tables["stay_unit"]) * (1 + n_stay)
    return dict(case=case, block=w, admitted=admitted, admit_step=np.where(admitted, admit, NEVER), end_step=np.where(admitted, end, NEVER),
                died=admitted & (w[:, 3] < death_thr[k]), onset=onset)


def at_stop(full, t_done):
    """The outcomes of a run stopped after t_done steps: the cases whose onset lies inside it; their outcome stands."""
    inside = full["case"] & (full["onset"] <= t_done)
    adm = full["admitted"] & inside
    return dict(case=inside, admitted=adm, admit_step=np.where(adm, full["admit_step"], NEVER), end_step=np.where(adm, full["end_step"], NEVER),
                died=full["died"] & inside)


def occupancy(o, cols, n_cols, t_done):
    """x[s, col] for the steps 0 .. t_done: the beds occupied after step s."""
    x = np.zeros((t_done + 2, n_cols), np.int64)
    adm = np.flatnonzero(o["admitted"])
    a, e, c = o["admit_step"][adm], o["end_step"][adm], np.asarray(cols, np.int64)[adm]
    live = a <= t_done
    np.add.at(x, (a[live], c[live]), 1)
    np.add.at(x, (np.minimum(e[live], t_done + 1), c[live]), -1)
    return np.cumsum(x, axis=0)[:t_done + 1]


def events(o, what, cols, n_cols, t_done):
    """x[s, col] for the steps 0 .. t_done: the admissions / deaths of step s."""
    pick = np.flatnonzero(o["admitted"] if what == "admissions" else o["died"])
    step = (o["admit_step"] if what == "admissions" else o["end_step"])[pick]
    live = step <= t_done
    x = np.zeros((t_done + 1, n_cols), np.int64)
    np.add.at(x, (step[live], np.asarray(cols, np.int64)[pick][live]), 1)
    return x


def series(o, what, cols, n_cols, t_done, first_step=1, n_rows=None, stride=1):
    """uint32 [n_rows, n_cols] under the row conventions of esim_area_status_series."""
    if n_rows is None:
        n_rows = (t_done - first_step) // stride + 1
    steps = first_step + stride * np.arange(n_rows)
    assert first_step >= 1 and n_rows >= 1 and steps[-1] <= t_done
    if what == "occupancy":
        return occupancy(o, cols, n_cols, t_done)[steps].astype(np.uint32)
    x = events(o, what, cols, n_cols, t_done)
    padded = np.concatenate([x, np.zeros((stride, n_cols), np.int64)])           # (the last row's stride may reach beyond the run)
    return np.stack([padded[s:s + stride].sum(axis=0) for s in steps]).astype(np.uint32)


def summary(o, cols, n_cols, t_done, first_step=1, last_step=None, threshold=1):
    """The eight arrays of esim_burden_summary."""
    last_step = t_done if last_step is None else last_step
    s = _curve_ref.summarize(occupancy(o, cols, n_cols, t_done)[1:], first_step, last_step, threshold)
    out = {k: s[k] for k in KEYS[:5]}
    out["bed_steps"] = s["person_steps"]
    for what in ("admissions", "deaths"):
        out[what] = events(o, what, cols, n_cols, t_done)[first_step:last_step + 1].sum(axis=0).astype(np.uint32)
    return out


# ---- the two worlds ---------------------------------------------------------------------------------------------------------------
FIXTURE_A_STOPS = (1, 96, 300, 700)
W2_STEPS = 900
W2_STOPS = (1, 96, 402, 900)


def w2():
    """W2: 2000 citizens in 4 areas, a fast epidemic and a vaccination programme of one citizen a step, which vaccinates many
    while they are Infected and some while they are Exposed: population, esim_params, labels, n_groups."""
    pop = Population.synthetic("york", n_citizens=2000, n_areas=4, citizens_per_school=1000, n_seeds=10)
    ep = _lib.default_params(exposure_chance=0.02, lockdown_threshold=2.0, mask_pt_threshold=2.0, mask_everywhere_threshold=2.0,
                             vaccination_threshold=0.02, vaccination_rate=1, seed=321, max_steps=W2_STEPS)
    labels, n_groups = pop.age_bands(_group_ref.AGE_EDGES)
    return pop, ep, labels, n_groups


def table_groups(tables, labels):
    """The group of every citizen under `tables`: the labels, or group 0 for all under tables of one group, whatever the labels."""
    return np.asarray(labels) if len(tables["admit_thr"]) != 1 else np.zeros(len(labels), np.uint16)


def build(pop, ep, labels, n_groups, n_steps, tables=None, run=None):
    """dict(pop, ep, labels, n_groups, n_steps, tables, run = oracle_run, full = the outcomes under the tables, cols = {where: (labels,
    n_cols)}).  tables: None for table set T; tables of one group apply to everybody, and the labels only make the columns by
    group.  run: an oracle_run of (pop, ep, n_steps) made before, for several table sets over one run."""
    tables = table_set_t() if tables is None else tables
    run = oracle_run(pop, ep, n_steps) if run is None else run
    full = outcomes(run["onset"], table_groups(tables, labels), tables, lambda s: int(ep.seed), pop.citizen_id_base)
    cols = {where: _curve_ref.labels_for(pop, where, (labels, n_groups)) for where in WHERES}
    return dict(pop=pop, ep=ep, labels=np.asarray(labels), n_groups=n_groups, n_steps=n_steps, tables=tables, run=run, full=full, cols=cols)


def counts(world):
    """What the issue that introduced the feature states of a world, from the reference: a dict of plain numbers and lists."""
    run, full, n = world["run"], world["full"], world["n_steps"]
    o = at_stop(full, n)
    x = occupancy(o, world["cols"]["all"][0], 1, n)[:, 0]
    return dict(cases=int(o["case"].sum()), vax_exposed=int(run["vax_exposed"].sum()), vax_infected=int(run["vax_infected"].sum()),
                vax_infected_admitted=int((run["vax_infected"] & o["admitted"]).sum()), admitted=int(o["admitted"].sum()),
                by_band=np.bincount(world["labels"][o["admitted"]], minlength=world["n_groups"]).tolist(), deaths=int(o["died"].sum()),
                in_bed_at_end=int(x[n]), peak=int(x[1:].max()), peak_step=int(x[1:].argmax()) + 1, steps_at_least_10=int((x[1:] >= 10).sum()))


@functools.lru_cache(maxsize=None)
def fixture_a():
    """Fixture A with its 8 age bands over 700 steps."""
    pop, ep, labels, n_groups = _group_ref.fixture_a_groups()
    world = build(pop, ep, labels, n_groups, 700)
    got = counts(world)
    want = dict(cases=722, vax_exposed=99, vax_infected=0, vax_infected_admitted=0, admitted=152, by_band=[1, 0, 0, 7, 9, 26, 56, 53], deaths=42,
                in_bed_at_end=3, peak=87, peak_step=396, steps_at_least_10=431)
    assert got == want, "fixture A under table set T: %s, the issue states %s" % (got, want)
    return world


@functools.lru_cache(maxsize=None)
def world_w2():
    pop, ep, labels, n_groups = w2()
    world = build(pop, ep, labels, n_groups, W2_STEPS)
    got = counts(world)
    want = dict(cases=1835, vax_exposed=85, vax_infected=275, vax_infected_admitted=64, admitted=475, deaths=130, peak=236, peak_step=402)
    assert {k: got[k] for k in want} == want, "W2 under table set T: %s, the issue states %s" % (got, want)
    return world
