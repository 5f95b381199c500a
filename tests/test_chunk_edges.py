"""CPU guard of the capacity fixtures (tests/_chunk_edges.py): each one reaches the limit its GPU case
(tests/test_chunk_edges_gpu.py) is meant to drive the chunk form to -- checked with the oracle and numpy over the population,
so that it stays true when the GPU tests are not run."""
import numpy as np

import _chunk_edges as ce
import _oracle
from epidemicsimulator_amd import _lib


def _oracle_run(pop, params, steps):
    o = _oracle.Oracle(pop, _oracle.params_from_esim(_lib.default_params(**params)))
    o.set_threads(4)
    r = o.run(steps)
    o.close()
    return r


def _seed_routes(pop):
    route, riders = ce.routes(pop)
    return route[pop.seeds], riders


def test_tiny_big_pairs_fixture_fills_the_tiny_forms_pair_list():
    pop, params = ce.tiny_big_pairs()
    sr, riders = _seed_routes(pop)
    assert len(np.unique(sr)) == len(sr) == ce.TINY_E and (riders[sr] > ce.BIG_ROUTE).all()
    r = _oracle_run(pop, params, ce.CHUNK)
    # the first chunk: its 64 Infected (nobody exposed in it is Infected before step 98) on a bus in 8 steps, no lockdown
    assert (r["infected"] == ce.TINY_E).all() and r["lockdown"].sum() == 0
    assert int(ce.bus_steps(r).sum()) == ce.TINY_BUS
    pairs = len(sr) * ce.TINY_BUS
    assert pairs == ce.TINY_BIG and pairs > 64                 # 64: the list's size before


def test_frozen_bus_fixture_exceeds_the_old_big_pair_list():
    pop, params = ce.frozen_bus_big_pairs()
    sr, riders = _seed_routes(pop)
    n_big = int((riders > ce.BIG_ROUTE).sum())
    assert len(np.unique(sr)) == len(sr) == n_big == 8200
    r = _oracle_run(pop, params, ce.CHUNK_BUS_STEPS)
    # a lockdown from the first step on, decided on a bus hour: riders on the bus in every step, so the chunk has 32 bus steps
    assert ce.bus_steps(r).all() and r["lockdown"].all() and (r["infected"] == len(sr)).all()
    cap = ce.items_cap(ce.FROZEN_HASH_LOG2)
    assert len(sr) <= ce.admitted_pairs(ce.FROZEN_HASH_LOG2)   # the chunk is admitted to the one-pass form ...
    pairs = n_big * ce.CHUNK_BUS_STEPS
    assert pairs > 2 * cap                                     # ... and registers more pairs than 2 * items_cap
    assert pairs <= min(cap // 4, n_big) * ce.CHUNK_BUS_STEPS  # the list's size now (esim_upload_population)


def test_pair_k_fixture_puts_every_infected_on_its_own_small_route():
    for frozen in (False, True):
        pop, params = ce.pair_k_tight(frozen)
        sr, riders = _seed_routes(pop)
        assert len(np.unique(sr)) == len(sr) == 300 and (riders[sr] <= ce.BIG_ROUTE).all()
        assert len(sr) > ce.TINY_E                              # the wide form's case
        n = ce.CHUNK_BUS_STEPS if frozen else ce.CHUNK
        r = _oracle_run(pop, params, n)
        assert (r["infected"] == len(sr)).all()
        assert int(ce.bus_steps(r).sum()) == (ce.CHUNK_BUS_STEPS if frozen else 8)
    # ESIM_GRID_CHUNK=16: 64 wavefronts of k_chunk_marks, ceil(300 / 64) = 5 entries in a full stretch, 5 x bus steps pairs =
    # PAIR_K(4 x 5, bus steps) -- no slack at 8 (2 x items_per_wave) nor at 32 ((32 + 3) / 4 x items_per_wave)
    per_wave = 4 * -(-300 // 64)
    for nbus in (8, 32):
        k = per_wave * ((nbus + 3) // 4 if nbus > 8 else 2)
        assert 5 * nbus == k


def test_tiny_task_fixture_overflows_the_task_queue():
    pop, params = ce.tiny_task_spill()
    assert pop.n_seeds <= ce.TINY_E
    p = _lib.default_params(**params)
    at_work = ce.CHUNK // 24 * (p.end_hour - p.start_hour)     # steps of a 96-step chunk at work
    workers = np.bincount(pop.work_building, minlength=pop.n_buildings)
    places = np.unique(pop.work_building[pop.seeds])
    units = sum(-(-int(workers[b]) * at_work // ce.TINY_INLINE) for b in places)
    assert units > ce.TINY_TASKS, units
    r = _oracle_run(pop, params, ce.CHUNK)
    assert (r["infected"] == pop.n_seeds).all()


def test_admission_fixture_crosses_the_bound_both_ways():
    pop, params = ce.admission_boundary()
    bound = ce.admitted_pairs(ce.ADMISSION_HASH_LOG2)
    r = _oracle_run(pop, params, 480)
    inf = r["infected"].astype(np.int64)
    # steps 1-96: the 16 000 seeds and nobody else (exposures are Infected from step 98 on): every chunk fits
    assert inf[:96].max() == pop.n_seeds <= bound
    # steps 193-336: more Infected than the bound in every single step, so no chunk of any length is admitted
    assert inf[192:336].min() > bound
    # from step 337 on the seeds have recovered: far below it again
    assert inf[336:].max() < bound // 4
