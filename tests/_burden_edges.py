"""The hospital burden and the lists of admitted cases at the limits of the severity tables and at the edges of esim_params: the
table sets, the cases they run on, their references (tests/_burden_ref.py over the CPU oracle, once per session) and what the
guards read off them.  tests/test_burden_edges.py checks on the CPU that every set and case reaches its edge and that the inputs
tell a nearly right rule from the right one; tests/test_burden_edges_gpu.py compares the device with the references.  Importing
this module and reading its tables needs neither libesim.so nor a device; world() calls the library's population builder (host
code) and the CPU oracle.

Every run is N = 400 steps on the town of tests/_replay_edges.py (3 000 citizens, 8 areas, 10 distinct index cases) or its
permuted copy.  Seven table sets run on one case of the parameter edges, TABLE_CASE; the eighth, edge_e, on all 27."""
import functools
import types

import numpy as np

import _burden_ref as ref
import _household_ref as hh
import _param_edges as pe
import _replay_edges as edges
from epidemicsimulator_amd import _lib

N = edges.N
NEVER = ref.NEVER
TABLE_CASE = "bus_capacity_2_31"
OTHER_SEED = 0x5DEECE66D1234567            # the second run of a case, against which its kept list is compared
ALL = [0xFFFFFFFF]
T = ref.table_set_t()
CDF_64 = [((j + 1) << 32) // 65 for j in range(64)]          # 65 equal bins: both counts take every value 0 .. 64
FLAT = [0, 0, 0x80000000, 0x80000000, 0xFFFFFFFF, 0xFFFFFFFF]


def _one(admit, death, **rest):
    return dict(admit_thr=np.asarray(admit, np.uint32), death_thr=np.asarray(death, np.uint32), **rest)


def _cdfs(cdf, unit):
    return dict(delay_cdf=np.asarray(cdf, np.uint32), delay_unit=unit, stay_cdf=np.asarray(cdf, np.uint32), stay_unit=unit)


def _groups_1024():
    rng = np.random.default_rng(5)
    admit = rng.integers(0, 1 << 32, 1024, dtype=np.uint64).astype(np.uint32)
    death = rng.integers(0, 1 << 32, 1024, dtype=np.uint64).astype(np.uint32)
    admit[0] = admit[1023] = 0xFFFFFFFF
    admit[1] = 0
    death[0] = 0
    death[1023] = 0xFFFFFFFF
    return dict(admit_thr=admit, death_thr=death, delay_cdf=T["delay_cdf"], delay_unit=5, stay_cdf=T["stay_cdf"], stay_unit=7)


ONE_GROUP = _one(ref.percent((40,)), ref.percent((30,)), delay_cdf=T["delay_cdf"], delay_unit=5, stay_cdf=T["stay_cdf"], stay_unit=7)

# name: (the tables as Simulator.set_burden takes them, the groups of the labels -- _household_ref.labels(pop, groups) -- that the
# tables index where they have several groups, and that make the columns of where="group" in any case)
SETS = {
    "bins_64": (_one(ALL, ref.percent((50,)), **_cdfs(CDF_64, 1)), edges.N_GROUPS),
    "bins_64_unit_max": (_one(ALL, ref.percent((50,)), **_cdfs(CDF_64, 65535)), edges.N_GROUPS),
    "bins_0_unit_max": (_one(ALL, ALL, **_cdfs([], 65535)), edges.N_GROUPS),
    "flat_cdf": (_one(ALL, ref.percent((50,)), **_cdfs(FLAT, 3)), edges.N_GROUPS),
    "groups_1024": (_groups_1024(), 1024),
    "one_group_64": (ONE_GROUP, 64),
    "one_group_65": (ONE_GROUP, 65),
    "edge_e": (dict(admit_thr=ref.percent((30, 50, 70, 100, 0)), death_thr=ref.percent((50, 0, 100, 25, 100)),
                    delay_cdf=ref.percent(np.cumsum((40, 20, 20, 10))), delay_unit=7,
                    stay_cdf=ref.percent(np.cumsum((20, 20, 20, 15, 15, 5))), stay_unit=5), edges.N_GROUPS),
}
TABLE_SETS = tuple(k for k in SETS if k != "edge_e")
CASES = tuple(pe.CASES)

# What a case of edge_e cannot have, by construction; the reference shows none there, and nothing is asked of it.
# Nobody vaccinated while Infected (in every other case some of them are admitted cases, whose outcome stands):
WITHOUT_VACCINATED_WHILE_INFECTED = {
    "exposed_time_200": "whoever the programme reaches was exposed after step 199, if at all, and is Infected beyond step 400",
    "infected_time_0": "nobody is Infected after any step",
    "infected_time_1": "at exposure_chance 1 the epidemic is over when the programme starts at record 194",
    "exposure_chance_0": "the index cases are the only cases, and the programme does not reach them",
    "vaccination_rate_0": "nobody is vaccinated",
    "vaccination_rate_8192": "everybody eligible is vaccinated in the programme's first step, while Susceptible",
}
# Nobody vaccinated while Exposed, although the programme vaccinates:
WITHOUT_VACCINATED_WHILE_EXPOSED = {
    "infected_time_1": "at exposure_chance 1 the epidemic is over when the programme starts at record 194: nobody is Exposed any more",
    "exposure_chance_0": "nobody is ever exposed",
    "vaccination_rate_8192": "everybody eligible is vaccinated in the programme's first step, while Susceptible",
}
# Citizens vaccinated while Exposed, none of whom would have had an onset inside the run:
VACCINATED_WHILE_EXPOSED_BEYOND_THE_RUN = {
    "exposed_time_200": "all of them were exposed after step 199: Infected 201 steps on, beyond step 400",
}
# Cases of edge_e in which an admission or an end of an admitted case lies beyond step N in the reference: they are in the outcomes and
# in the lists and in no row.  (The others: epidemics that are over early, under exposed_time 0 .. 3, infected_time 0 / 1, exposure_chance
# 0 / 1, vaccination_rate 8192 and thresholds_0.)
BEYOND_THE_RUN = ("exposed_time_94", "exposed_time_95", "exposed_time_97", "exposed_time_200", "encoding_limit_512", "hours_22_6", "hours_1_23",
                  "hours_9_11", "hours_23_2", "mask_effectiveness_0", "mask_effectiveness_1", "mask_effectiveness_1_5", "bus_capacity_1",
                  "bus_capacity_2_31", "vaccination_rate_0", "seed_0", "seed_max")
# The cases whose exposed_time is not the default: the onset rule must read the parameter.
EXPOSED_TIME_CASES = tuple(n for n in pe.CASES if pe.CASES[n].over.get("exposed_time", pe.DEFAULT_EXPOSED_TIME) != pe.DEFAULT_EXPOSED_TIME)
# The cases whose seed has a high word.
HIGH_WORD_CASES = tuple(n for n in pe.CASES if n != "seed_0")


def vaccinating(name):
    return pe.vaccinating in edges.guards_of(name)


def params_of(name, seed=None):
    over = edges.params_dict(name)
    if seed is not None:
        over["seed"] = seed
    return _lib.default_params(**over)


def population(permuted=False):
    return edges.permuted_world() if permuted else edges.world()


@functools.lru_cache(maxsize=None)
def run_of(name, permuted=False, seed=None):
    """_burden_ref.oracle_run of the case (under another seed where one is given), shared by every table set over it."""
    return ref.oracle_run(population(permuted), params_of(name, seed), N)


@functools.lru_cache(maxsize=None)
def world(set_name, case=TABLE_CASE, permuted=False, seed=None):
    """The world of _burden_ref.build for a table set over a case.  Shared: nobody writes to it."""
    tables, g = SETS[set_name]
    pop = population(permuted)
    return ref.build(pop, params_of(case, seed), hh.labels(pop, g), g, N, tables=tables, run=run_of(case, permuted, seed))


def outcomes(w):
    return ref.at_stop(w["full"], N)


def inner_window(w):
    """_replay_edges.inner_window over the oracle's exposure log."""
    return edges.inner_window(types.SimpleNamespace(tref={"step": w["run"]["exposure_step"]}, n=N))


def spans(w):
    """(first_step, last_step, threshold) of the summary calls: the whole run and the inner window, thresholds 1 and 10."""
    first, last = inner_window(w)
    return [(1, N, 1), (1, N, 10), (first, last, 1), (first, last, 10)]


SERIES = ((1, None, 1), (3, None, 24))           # (first_step, n_rows, stride) of the series calls


def bins(w):
    """(n_delay, n_stay) of the admitted cases: the table counts, read back off the reference's steps."""
    o, t = outcomes(w), w["tables"]
    a = o["admitted"]
    onset = w["full"]["onset"][a]
    return (o["admit_step"][a] - onset) // int(t["delay_unit"]), (o["end_step"][a] - o["admit_step"][a]) // int(t["stay_unit"]) - 1


def facts(w):
    """What the guards read off a world's reference: a dict of plain numbers."""
    o, run = outcomes(w), w["run"]
    a = o["admitted"]
    adm, end = o["admit_step"][a], o["end_step"][a]
    g = ref.table_groups(w["tables"], w["labels"])
    return dict(cases=int(o["case"].sum()), admitted=int(a.sum()), died=int(o["died"].sum()),
                admitted_inside=int(((adm >= 1) & (adm <= N)).sum()), admitted_at_0=int((adm == 0).sum()), admitted_beyond=int((adm > N).sum()),
                ends_inside=int((end <= N).sum()), ends_beyond=int((end > N).sum()), largest_end=int(end.max(initial=0)),
                by_group=np.bincount(g[a], minlength=len(w["tables"]["admit_thr"])), vax_exposed=int(run["vax_exposed"].sum()),
                vax_infected=int(run["vax_infected"].sum()), vax_infected_admitted=int((run["vax_infected"] & a).sum()))


# ---- nearly right rules, in numpy beside the reference ------------------------------------------------------------------------------
def variant(w, tables=None, groups=None, onset=None, seed_of=None):
    """The outcomes at step N under the world's inputs with some of them exchanged."""
    tables = w["tables"] if tables is None else tables
    groups = ref.table_groups(tables, w["labels"]) if groups is None else groups
    onset = w["run"]["onset"] if onset is None else onset
    seed_of = (lambda s: int(w["ep"].seed)) if seed_of is None else seed_of
    return ref.at_stop(ref.outcomes(onset, groups, tables, seed_of, w["pop"].citizen_id_base), N)


def differs(a, b, keys=("admit_step", "end_step", "died")):
    return any((np.asarray(a[k]) != np.asarray(b[k])).any() for k in keys)


def without_the_last_bin(w):
    t = w["tables"]
    return variant(w, tables=dict(t, delay_cdf=t["delay_cdf"][:-1], stay_cdf=t["stay_cdf"][:-1]))


def group_clamped(w, top):
    return variant(w, groups=np.minimum(ref.table_groups(w["tables"], w["labels"]), top))


def stay_without_its_first_unit(w):
    o = outcomes(w)
    return dict(o, end_step=np.where(o["admitted"], o["end_step"] - int(w["tables"]["stay_unit"]), NEVER))


def index_cases_at_onset_1(w):
    onset = w["run"]["onset"]
    return variant(w, onset=np.where(onset == 0, 1, onset))


def onset_by_rule(w, exposed_time):
    """The onsets by the arithmetic exposure step + exposed_time + 1 (index cases 0, beyond the run none) of everybody exposed."""
    step = w["run"]["exposure_step"]
    onset = np.where(step > 0, step + exposed_time + 1, NEVER)
    onset[np.unique(w["pop"].seeds)] = 0
    return np.where(onset > N, NEVER, onset)


def vaccinated_while_exposed_counted(w):
    run = w["run"]
    return variant(w, onset=np.where(run["vax_exposed"], onset_by_rule(w, int(w["ep"].exposed_time)), run["onset"]))


def seed_without_its_high_word(w):
    return variant(w, seed_of=lambda s: int(w["ep"].seed) & 0xFFFFFFFF)


def onset_under_the_default_exposed_time(w):
    run = w["run"]
    return variant(w, onset=np.where(run["onset"] != NEVER, onset_by_rule(w, pe.DEFAULT_EXPOSED_TIME), NEVER))


# ---- the seam at its exact step -----------------------------------------------------------------------------------------------------
SEAM_PARAMS = dict(exposure_chance=0.02, lockdown_threshold=2.0, mask_pt_threshold=2.0, mask_everywhere_threshold=2.0, vaccination_threshold=2.0,
                   seed=321, max_steps=N)
SEAM_SEEDS = (321, 99)
SEAM_RUN_ON = 40                                 # steps run beyond the snapshot before the rollback


@functools.lru_cache(maxsize=None)
def seam():
    """No programme, so that the onsets follow from the exposure log alone; tables bins_64.  step: the snapshot's step, the one in
    100 .. N - 41 with the most cases of onset `step` and of onset `step + 1` (the smaller of the two counts; the first such step).
    Both kinds were exposed exposed_time + 1 steps earlier, before the snapshot: the first leg, which the oracle runs, decides them."""
    pop = edges.world()
    ep = _lib.default_params(**SEAM_PARAMS)
    run = ref.oracle_run(pop, ep, N)
    assert not run["records"]["vaccination_active"].any() and int(ep.exposed_time) + 1 > 1
    onset = run["onset"]
    count = np.bincount(onset[onset != NEVER], minlength=N + 2)
    steps = np.arange(100, N - SEAM_RUN_ON)
    step = int(steps[np.minimum(count[steps], count[steps + 1]).argmax()])
    labels, g = edges.labels_of(pop)
    return types.SimpleNamespace(pop=pop, ep=ep, run=run, step=step, labels=labels, n_groups=g, tables=SETS["bins_64"][0],
                                 at=(int(count[step]), int(count[step + 1])))


def seam_outcomes(s, onset, strict=False):
    """The outcomes over `onset` with the seam at s.step: onsets up to it (strict: before it) draw under the first seed."""
    old, new = SEAM_SEEDS
    rule = (lambda t: old if t < s.step else new) if strict else (lambda t: old if t <= s.step else new)
    return ref.outcomes(onset, ref.table_groups(s.tables, s.labels), s.tables, rule, s.pop.citizen_id_base)
