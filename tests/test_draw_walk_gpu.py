"""The draw pass where its walks change direction: member lists that end inside, at and beyond a staged block of
64 members, chunks that start off a multiple of four time steps (a slot of four steps then begins before the chunk), bus routes
around the capacity of a bus and of a wavefront, and buses too small for the division-free bus number.  Bit-equal to the CPU
oracle: every record, and the citizens' full state at the end of every block of steps.

One world holds it all (808 citizens): for every r in SIZES two Output Areas whose r commuters live in households of four, work
in one workplace of r members and ride one route of r riders (tests/_chunk_edges.py: commuter_areas) -- member lists and routes
of 20, 21, 41, 63, 64, 65 and 130.  A workplace with an Infected worker has a marked step in about a dozen slots of a chunk, so
the list of 130 is more than 1024 (member, slot) pairs: the wide form cuts it into units, the second of which starts at pair
1024, inside a member (1024 is no multiple of 9 .. 15); the one-launch form cuts every list here into units of 256 pairs."""
import numpy as np
import pytest

import _chunk_edges as ce
import _oracle
from epidemicsimulator_amd import Population, _lib
from test_parity_gpu import run_forms

pytestmark = pytest.mark.gpu

SIZES = (20, 21, 41, 63, 64, 65, 130)
FORMS = ("wide", "tinymax")
PARAMS = dict(ce.QUIET, exposure_chance=0.02, seed=5301)


def merged(parts):
    """The populations side by side: citizens, buildings and areas of each behind those of the one before."""
    home, work, flags, area, btype, seeds = [], [], [], [], [], []
    c0 = b0 = a0 = 0
    for p in parts:
        home.append(p.home_building + np.uint32(b0)); work.append(p.work_building + np.uint32(b0)); flags.append(p.flags)
        area.append(p.building_area + np.uint32(a0)); btype.append(p.building_type); seeds.append(p.seeds + np.uint32(c0))
        c0 += p.n_citizens; b0 += p.n_buildings; a0 += p.n_areas
    cat = np.concatenate
    return Population(home_building=cat(home), work_building=cat(work), flags=cat(flags), building_area=cat(area),
                      building_type=cat(btype), seeds=cat(seeds), n_areas=a0)


@pytest.fixture(scope="module")
def world():
    pop = merged([ce.commuter_areas(2, r) for r in SIZES])
    _, riders = ce.routes(pop)
    assert sorted(set(riders.tolist())) == list(SIZES) and pop.n_citizens == 2 * sum(SIZES)
    assert sorted(set(np.bincount(pop.work_building)[np.flatnonzero(pop.building_type == _lib.WORKPLACE)].tolist())) == list(SIZES)
    return pop


class Blocks:
    """What run_forms takes (test_parity_gpu.OracleRun), with blocks of the lengths given: a block's first chunk starts where the
    block does."""

    def __init__(self, pop, blocks, **params):
        self.pop, self.params, self.stop = pop, params, False
        orc = _oracle.Oracle(pop, _oracle.params_from_esim(_lib.default_params(**params)))
        self.asked, self.records, self.states = [], [], []
        for n in blocks:
            self.asked.append(n); self.records.append(orc.run(n)); self.states.append(orc.state())
        orc.close()


def chunk_counts(run, forms):
    """Runs the forms against the oracle run; returns per form the steps that ran as one-pass chunks."""
    steps = {}

    def observe(form, sim, i):
        if i < 0:
            sim.enable_kernel_timing(1)
            sim.enable_chunk_kernel_timing(True)
        else:
            steps[form] = steps.get(form, 0) + sim.chunk_timing()["steps"]      # (reading the counter resets it)

    run_forms(run, forms, observe)
    return steps


# chunks of 96 steps that start at t0 & 3 = 0 (step 0), 1 (steps 1 and 97) and 3 (step 3): 25 slots when t0 & 3 != 0.  The fourteen
# seeds are the Infected of a first chunk (the one-launch form takes it); the chunk from step 97 has hundreds (wide form only).
@pytest.mark.timeout(120)
@pytest.mark.parametrize("blocks", ((96, 1, 96), (1, 96), (3, 96)), ids=("t0_0_and_97", "t0_1", "t0_3"))
@pytest.mark.parametrize("bus_capacity", (20, 7), ids=("bus20", "bus7"))
def test_lists_across_staging_blocks_and_routes_around_a_bus(world, blocks, bus_capacity):
    run = Blocks(world, blocks, bus_capacity=bus_capacity, **PARAMS)
    rec = np.concatenate(run.records)
    # the run has what the walks are about: draws that succeed in buildings and on buses, Infected riding in every chunk
    assert rec["exposures_building"].sum() > 0 and rec["exposures_bus"].sum() > 0, (int(rec["exposures_building"].sum()), int(rec["exposures_bus"].sum()))
    assert all(ce.bus_steps(r).any() and r["infected"].min() > 0 for r in run.records if len(r) >= 96)
    steps = chunk_counts(run, FORMS)
    for form in FORMS:
        assert steps[form] >= sum(b for b in blocks if b >= 96), (form, steps)     # the long blocks ran as one-pass chunks
