"""Populations that drive the one-pass chunk forms to their capacity limits (tests/test_chunk_edges.py checks on the CPU that
they do, tests/test_chunk_edges_gpu.py runs them), and the limits themselves as the kernels define them."""
import numpy as np

from epidemicsimulator_amd import Population, _lib

TINY_E = 64              # esim_kernels_tiny.h: Infected (log entries) of a chunk k_chunk_tiny takes
TINY_BUS = 8             # ... bus steps of a chunk it takes
TINY_BIG = 512           # ... (big route, bus step) pairs it holds (64 before: ERR_AT_BIGPAIRS past the 64th)
TINY_TASKS = 512         # ... units of TINY_INLINE (member, slot) pairs in its queue
TINY_INLINE = 256
CHUNK_BUS_STEPS = 32     # esim_device.h: bus steps of a one-pass chunk (k_decide cuts the chunk in front of the 33rd)
BIG_ROUTE = 64           # a route of more riders than this is "big" (ranked by a workgroup)
CHUNK = 96               # FREE_MAX: steps of a chunk at most


def items_cap(hash_log2):
    return (1 << hash_log2) // 4


def admitted_pairs(hash_log2):
    """Largest chunk_pairs (citizens Infected in some step of the chunk) future_body admits to the one-pass form."""
    return (items_cap(hash_log2) - 65536) // 4


def commuter_areas(n_areas, riders, seeds_per_area=1, household=4, uses_pt=True):
    """`n_areas` Output Areas; the `riders` citizens of area a live in households of `household` there and all work in one
    workplace in area (a + 1) % n_areas, so that each area is one route (home area, work area) of `riders` riders
    (esim_upload_population keys routes by the pair).  The first `seeds_per_area` citizens of every area are the seeds."""
    n = n_areas * riders
    c_area = np.repeat(np.arange(n_areas, dtype=np.uint32), riders)
    per_area_hh = -(-riders // household)
    local = np.tile(np.arange(riders, dtype=np.uint32), n_areas)
    home = c_area * per_area_hh + local // household
    n_hh = n_areas * per_area_hh
    work = (n_hh + (c_area + 1) % n_areas).astype(np.uint32)
    building_area = np.concatenate([np.repeat(np.arange(n_areas, dtype=np.uint32), per_area_hh),
                                    np.arange(n_areas, dtype=np.uint32)])
    building_type = np.concatenate([np.full(n_hh, _lib.HOUSEHOLD, np.uint8), np.full(n_areas, _lib.WORKPLACE, np.uint8)])
    flags = np.full(n, 1 if uses_pt else 0, np.uint8)
    seeds = (np.arange(n_areas, dtype=np.uint32)[:, None] * riders + np.arange(seeds_per_area, dtype=np.uint32)[None, :]).ravel()
    return Population(home_building=home, work_building=work, flags=flags, building_area=building_area,
                      building_type=building_type, seeds=seeds, n_areas=n_areas)


def big_workplaces(n_work=3, workers=3000, n_homes_areas=8, n_seeds=12):
    """`n_work` workplaces of `workers` each in area 0, their workers in households of four spread over `n_homes_areas` areas,
    nobody on public transport; the seeds work in those workplaces (round robin)."""
    n = n_work * workers
    home = (np.arange(n, dtype=np.uint32) // 4)
    n_hh = int(home.max()) + 1
    work = (n_hh + np.arange(n, dtype=np.uint32) % n_work).astype(np.uint32)
    building_area = np.concatenate([np.arange(n_hh, dtype=np.uint32) % n_homes_areas, np.zeros(n_work, np.uint32)])
    building_type = np.concatenate([np.full(n_hh, _lib.HOUSEHOLD, np.uint8), np.full(n_work, _lib.WORKPLACE, np.uint8)])
    seeds = np.arange(0, n_seeds * 37, 37, dtype=np.uint32)
    return Population(home_building=home, work_building=work, flags=np.zeros(n, np.uint8), building_area=building_area,
                      building_type=building_type, seeds=seeds, n_areas=n_homes_areas)


def routes(pop):
    """Route of every citizen (-1: no public transport) and riders per route, keyed as esim_upload_population keys them."""
    pt = (pop.flags & 1) != 0
    key = pop.building_area[pop.home_building].astype(np.int64) << 32 | pop.building_area[pop.work_building].astype(np.int64)
    uniq, inv = np.unique(key[pt], return_inverse=True)
    route = np.full(pop.n_citizens, -1, np.int64)
    route[pt] = inv
    return route, np.bincount(inv, minlength=len(uniq))


def bus_steps(rec):
    """Steps of a run (oracle records) in which riders are on a bus."""
    return rec["n_riders"] > 0


# -- the fixtures and their parameters (shared by the CPU guard and the GPU tests) -----------------------------------------
QUIET = dict(vaccination_threshold=2.0, lockdown_threshold=2.0, mask_pt_threshold=2.0, mask_everywhere_threshold=2.0)


def tiny_big_pairs():
    # 64 areas, one route of 72 riders each, one seed on each: 64 Infected on 64 distinct big routes, 8 bus steps in the first
    # chunk of 96 steps -> 512 (big route, bus step) pairs, TINY_BIG exactly
    return commuter_areas(64, 72), dict(QUIET, exposure_chance=0.002, seed=4101)


# A lockdown decided at the end of the first step, which is a bus hour (start_hour 2: the first step runs at hour 1): every
# later step keeps riders on the bus (Q8), so k_decide cuts the chunk at CHUNK_BUS_STEPS bus steps.
FROZEN = dict(vaccination_threshold=2.0, lockdown_threshold=0.005, mask_pt_threshold=2.0, mask_everywhere_threshold=2.0,
              start_hour=2, end_hour=17)
FROZEN_HASH_LOG2 = 19


def frozen_bus_big_pairs():
    # 8 200 areas, one route of 66 riders each, one seed on each: 8 200 big routes with an Infected rider in a chunk of 32 bus
    # steps -> 262 400 (big route, bus step) pairs, more than 2 * items_cap = 262 144 at ESIM_HASH_LOG2=19 (the list's size
    # before), 8 200 Infected well inside the admission's 16 384
    return commuter_areas(8200, 66), dict(FROZEN, exposure_chance=0.0005, seed=4102)


def pair_k_tight(frozen):
    # 300 areas, one route of 40 riders each (small routes), one seed each: every Infected rides its own small route in every
    # bus step of the chunk -- 8 a chunk, or CHUNK_BUS_STEPS under a lockdown freeze
    return commuter_areas(300, 40), dict(FROZEN if frozen else QUIET, exposure_chance=0.001, seed=4103 + int(frozen))


def tiny_task_spill():
    # 12 Infected working in three workplaces of 3 000: each workplace's worker list is 3 000 members x 32 at-work steps of a
    # chunk = 375 units of TINY_INLINE, 1 125 in all against a queue of TINY_TASKS
    return big_workplaces(), dict(QUIET, exposure_chance=0.00002, seed=4104)


ADMISSION_HASH_LOG2 = 19


def admission_boundary():
    # 16 000 seeds in households of four: chunk pairs start just below admitted_pairs(19) = 16 384, the first exposures (Infected
    # from step 98 on) push them above it, the seeds' recovery (step 337) takes them back below
    n = 120000
    home = np.arange(n, dtype=np.uint32) // 4
    n_hh = n // 4
    pop = Population(home_building=home, work_building=home.copy(), flags=np.zeros(n, np.uint8),
                     building_area=(np.arange(n_hh, dtype=np.uint32) % 64), building_type=np.zeros(n_hh, np.uint8),
                     seeds=np.arange(0, 4 * 16000, 4, dtype=np.uint32), n_areas=64)
    return pop, dict(QUIET, exposure_chance=0.00012, seed=4105)
