"""Parameter sets at the edges of what esim_params allows -- the values the kernels' arithmetic is built around (chunk length,
status windows, hour tables, the 2^32 threshold, the seed's high word) -- on one small world in which everything happens.
tests/test_param_edges.py checks on the CPU that every case does what it is meant to (its guard over the oracle's records),
tests/test_param_edges_gpu.py runs the cases in every execution form.  Importing this module and reading its table needs
neither libesim.so nor a device (world() and the table are numpy and plain numbers); oracle_records() loads the CPU oracle and
reads the library's default parameters when it is called."""
import functools

import numpy as np

import _oracle
from epidemicsimulator_amd import Population, _lib

FREE_MAX = 96            # esim_device.h: steps of a chunk at most
SLOT_STEPS = 4           # steps of one Philox block (esim_u32_of)
TE_BIAS = 512            # exposed_time + infected_time + 2 at most (the state encoding)
VACC_MAX_RATE = 8192
MAX_STEP = 7600          # ESIM_MAX_STEP
DEFAULT_EXPOSED_TIME = 96        # esim_default_params (tests/test_param_edges.py checks the two against the library)
DEFAULT_INFECTED_TIME = 336
N_STEPS = 400
BLOCK = 67               # no multiple of 4 nor of any case's chunk length (1, 2, 3, 4, 95, 96)


def random_population(seed, n=700, n_areas=5, n_buildings=90, n_schools=3, rooms_per_school=4):
    """Anything the ABI allows, not just what the reference's builder produces: workplaces in other areas,
    people working in somebody's household, tiny and empty buildings, rooms with one member, citizens that
    are not sorted by home (exercises res_idx), duplicate seeds."""
    rng = np.random.default_rng(seed)
    b_area = rng.integers(0, n_areas, n_buildings).astype(np.uint32)
    b_type = rng.choice([_lib.HOUSEHOLD, _lib.WORKPLACE], n_buildings, p=[0.7, 0.3]).astype(np.uint8)
    schools = rng.choice(n_buildings, n_schools, replace=False)
    b_type[schools] = _lib.SCHOOL
    room_bld = np.repeat(schools, rooms_per_school).astype(np.uint32)
    not_school = np.nonzero(b_type != _lib.SCHOOL)[0]
    home = rng.choice(not_school, n).astype(np.uint32)                 # unsorted on purpose
    work = home.copy()
    room = np.full(n, _lib.NO_ROOM, np.uint32)
    kind = rng.random(n)
    w = kind < 0.45                                                    # works in any non-school building, any area
    work[w] = rng.choice(not_school, int(w.sum()))
    sc = (kind >= 0.45) & (kind < 0.8)                                 # school member in a random room
    r = rng.integers(0, len(room_bld), int(sc.sum()))
    room[sc] = r
    work[sc] = room_bld[r]
    flags = (rng.random(n) < 0.5).astype(np.uint8) | ((rng.random(n) < 0.6).astype(np.uint8) << 1)
    seeds = rng.integers(0, n, 9).astype(np.uint32)
    seeds[-1] = seeds[0]
    return Population(home_building=home, work_building=work, room=room, flags=flags, building_area=b_area,
                      building_type=b_type, room_building=room_bld, seeds=seeds, n_areas=n_areas)


@functools.lru_cache(maxsize=None)
def world():
    """2 500 citizens in 6 areas, 200 buildings, 2 schools of 3 rooms: riders and non-riders, mask-compliant citizens and
    others, school rooms, workplaces in other areas (tests/test_param_edges.py checks that)."""
    return random_population(31, n=2500, n_areas=6, n_buildings=200, n_schools=2, rooms_per_school=3)


# everything happens under these: exposures in buildings and on buses, a lockdown that comes and goes, all three mask states, a
# vaccination programme that runs for many steps; a seed whose high word is fully used (bit 63 set)
BASE = dict(exposure_chance=0.01, vaccination_rate=25, vaccination_threshold=0.08, lockdown_threshold=0.3,
            mask_pt_threshold=0.02, mask_everywhere_threshold=0.05, bus_capacity=20, seed=0x9E3779B97F4A7C15)


def chunk_len(params):
    """Steps of a chunk under these parameters (params_to_dev: xf_n)."""
    return min(FREE_MAX, params.get("exposed_time", DEFAULT_EXPOSED_TIME) + 1)


# ---- what makes a case non-trivial: predicates over the oracle's records of the N_STEPS steps ---------------------------------
def building(r): return int(r["exposures_building"].sum()) > 0
def bus(r): return int(r["exposures_bus"].sum()) > 0
def riders(r): return bool((r["n_riders"] > 0).any())
def vaccinating(r): return bool((r["vaccinated_now"] > 0).any())
def lockdown_on_and_off(r): return bool(r["lockdown"].any()) and not bool(r["lockdown"].all())
def all_masks(r): return set(r["mask_status"].tolist()) == {0, 1, 2}
def no_exposures(r): return int(r["exposures_building"].sum()) == 0 and int(r["exposures_bus"].sum()) == 0
def no_bus_exposures(r): return int(r["exposures_bus"].sum()) == 0
def programme_vaccinates_nobody(r): return bool(r["vaccination_active"].any()) and int(r["vaccinated"].max()) == 0
def lockdown_from_the_second_record(r): return bool(r["lockdown"][1:].all())
def masks_everywhere_from_the_second_record(r): return bool((r["mask_status"][1:] == 2).all())
def programme_from_the_second_record(r): return bool(r["vaccination_active"][1:].all())


def generations(n):
    """More exposures than n times the seeds: the short window is met by exposed citizens, not only by the seeds."""
    def check(r):
        return int(r["exposures_building"].sum()) + int(r["exposures_bus"].sum()) > n * world().n_seeds
    check.__name__ = "generations_%d" % n
    return check


EVERYTHING = (building, bus, riders, vaccinating, lockdown_on_and_off, all_masks)


def _without(*dropped):
    return tuple(g for g in EVERYTHING if g not in dropped)


class Case:
    def __init__(self, over, guards=EVERYTHING, why=""):
        self.over, self.guards, self.why = dict(over), tuple(guards), why

    @property
    def params(self):
        return dict(BASE, **self.over)

    @property
    def chunk(self):
        return chunk_len(self.params)


CASES = {}


def _case(name, over, guards=EVERYTHING, why=""):
    CASES[name] = Case(over, guards, why)


# -- exposed_time: the chunk is min(96, exposed_time + 1) steps -- shorter than a Philox block of four steps at 0..2, one block at
# 3, on both sides of FREE_MAX at 94 / 95 / 97, capped far below the window at 200
for _et in (0, 1, 2, 3, 94, 95, 97):
    _case("exposed_time_%d" % _et, dict(exposed_time=_et))
# 200: infected_time 300 keeps the sum inside the encoding (200 + 336 + 2 > 512).  Nobody exposed in the run is Infected before
# step 202: under BASE's thresholds no intervention but the masks would start in 400 steps, so the programme and the lockdown
# start at lower prevalence
_case("exposed_time_200", dict(exposed_time=200, infected_time=300, vaccination_threshold=0.03, lockdown_threshold=0.05))

# -- infected_time
# 0: the initially infected citizens recover in the tick of step 1, before that step's exposures are generated (the oracle's
# disease_tick, as the reference's), so nobody is ever exposed, whatever exposure_chance and however many seeds: the case pins
# the empty Infected window of the seeds (no Infected in any record, every distinct seed Recovered from the first on)
_case("infected_time_0", dict(infected_time=0),
      guards=(no_exposures, riders, lambda r: int(r["infected"].max()) == 0,
              lambda r: bool((r["recovered"] == len(set(world().seeds.tolist()))).all())),
      why="no exposures by construction: the seeds recover before the first exposures are generated")
# 1: Infected for two steps.  exposure_chance 1 and lower thresholds, so that the window is met by generations of exposed
# citizens and the programme and the lockdown still start.  With exposure_chance 1 a generation is exposed all at once and is
# Infected 96 + 1 = 97 = 1 (mod 24) hours later, for two hours: four generations are Infected at hours 1 to 7 and would never
# meet the default bus hours 8 / 9 and 16 / 17.  Working hours 3 to 11 put the bus hours at 2 / 3 and 10 / 11, so that citizens
# Infected for two steps do expose riders on buses
_case("infected_time_1", dict(infected_time=1, exposure_chance=1.0, start_hour=3, end_hour=11, vaccination_threshold=0.03,
                              lockdown_threshold=0.045),
      guards=EVERYTHING + (generations(10),))
_case("encoding_limit_512", dict(exposed_time=96, infected_time=414))                 # exposed + infected + 2 == TE_BIAS exactly

# -- working hours: a night shift (start > end), the longest day, the shortest (the four arms on four adjacent hours), a day
# that wraps midnight
for _s, _e in ((22, 6), (1, 23), (9, 11), (23, 2)):
    _case("hours_%d_%d" % (_s, _e), dict(start_hour=_s, end_hour=_e))

# -- exposure_chance: 1.0 makes the threshold 2^32 for every n >= 1 (no u32 holds it); 0.0 makes every threshold 0.  With 0.0
# nobody but the seeds is ever Infected (8 of 2 500 = 0.0032 until they recover at step 337), so the thresholds sit around that
# prevalence: the programme, the masks and a lockdown that ends with the seeds' recovery run over a table of zeros
_case("exposure_chance_1", dict(exposure_chance=1.0))
_case("exposure_chance_0", dict(exposure_chance=0.0, mask_pt_threshold=0.001, mask_everywhere_threshold=0.003,
                                vaccination_threshold=0.002, lockdown_threshold=0.0031),
      guards=(no_exposures, riders, vaccinating, lockdown_on_and_off), why="no exposures by definition")

# -- mask_effectiveness: 0 (the masked row equals the unmasked one), 1 (masked threshold 0), above 1 (a negative chance, which
# the signbit test clamps to 0)
for _name, _m in (("0", 0.0), ("1", 1.0), ("1_5", 1.5)):
    _case("mask_effectiveness_%s" % _name, dict(mask_effectiveness=_m))

# -- bus_capacity: 1 (every rider alone on a bus: no bus exposure is possible), larger than any route (and than an i32)
_case("bus_capacity_1", dict(bus_capacity=1), guards=_without(bus) + (no_bus_exposures,), why="a bus of one rider exposes nobody")
_case("bus_capacity_2_31", dict(bus_capacity=1 << 31))

# -- vaccination_rate: 0 (a programme that runs and vaccinates nobody), VACC_MAX_RATE (everybody eligible in the first step)
_case("vaccination_rate_0", dict(vaccination_rate=0), guards=_without(vaccinating) + (programme_vaccinates_nobody,),
      why="the programme is active and vaccinates nobody")
_case("vaccination_rate_8192", dict(vaccination_rate=VACC_MAX_RATE),
      guards=EVERYTHING + (lambda r: int(r["vaccinated_now"].max()) > 1024,))

# -- all four thresholds 0.0: every intervention is on from the first record's decision, so the lockdown holds in every record
# from the second on (nobody ever rides a bus: the first step, at hour 1, is no bus hour)
_case("thresholds_0", dict(lockdown_threshold=0.0, vaccination_threshold=0.0, mask_pt_threshold=0.0, mask_everywhere_threshold=0.0),
      guards=(building, vaccinating, lockdown_from_the_second_record, masks_everywhere_from_the_second_record, programme_from_the_second_record),
      why="lockdown from the second record on: no riders, no bus exposures")

# -- seed: both extremes of the 64-bit key (BASE's own seed has bit 63 set)
_case("seed_0", dict(seed=0))
_case("seed_max", dict(seed=2**64 - 1))

SHORT_CHUNK = [n for n, c in CASES.items() if c.chunk < FREE_MAX]          # the one-pass-chunk assertion applies
BLOCK_OF_ONE = [n for n, c in CASES.items() if c.chunk <= SLOT_STEPS]      # run a second time in blocks of one step
TIMING = ["exposed_time_0", "exposed_time_2", "exposed_time_200", "infected_time_0", "encoding_limit_512", "hours_22_6", "hours_1_23"]
LUT_CASES = [n for n, c in CASES.items() if "exposure_chance" in c.over or "mask_effectiveness" in c.over]


@functools.lru_cache(maxsize=None)
def oracle_records(name, steps=N_STEPS):
    """The oracle's records of the case's run."""
    o = _oracle.Oracle(world(), _oracle.params_from_esim(_lib.default_params(**CASES[name].params)))
    o.set_threads(4)
    r = o.run(steps)
    o.close()
    return r
