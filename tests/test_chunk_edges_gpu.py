"""The one-pass chunk forms at their capacity limits: each case is bit-exact against the oracle (records every step,
the full state at every block's end) and checks that the form under test did run at its limit, so that a change of the
fixtures cannot quietly move a case away from it.  tests/test_chunk_edges.py checks on the CPU that the fixtures reach the
limits."""
import numpy as np
import pytest

import _chunk_edges as ce
from test_parity_gpu import OracleRun, run_forms

pytestmark = pytest.mark.gpu


def _timed(sim, block):
    # the counters the cases read: chunk kernel launches (ESIM_CK_*) and the steps run as one-pass chunks
    if block < 0:
        sim.enable_kernel_timing(1)
        sim.enable_chunk_kernel_timing(True)
        return None
    return sim.chunk_timing()["steps"], sim.chunk_kernel_timings()["tiny"]["calls"]


def test_tiny_form_with_a_big_route_pair_on_every_entry_and_bus_step():
    # 64 Infected on 64 distinct routes of 72 riders, 8 bus steps: 512 (big route, bus step) pairs in the first chunk.  The
    # one-workgroup form held 64 and raised ESIM_ERANGE (ERR_AT_BIGPAIRS) on the 65th; it now holds TINY_E x TINY_BUS.
    pop, params = ce.tiny_big_pairs()
    run = OracleRun(pop, 480, ce.CHUNK, **params)
    assert int(ce.bus_steps(run.records[0]).sum()) == ce.TINY_BUS and run.records[0]["infected"].max() == ce.TINY_E
    seen = {}

    def observe(form, sim, i):
        if i == 0:
            seen[form] = _timed(sim, i) + (sim.debug_counters()["n_route_pairs_big"],)
        elif i < 0:
            _timed(sim, i)

    run_forms(run, ("vax", "tinymax", "wide"), observe)
    for form in ("vax", "tinymax"):
        steps, tiny, _ = seen[form]
        assert steps == ce.CHUNK and tiny >= 1, (form, seen[form])            # the first chunk: one pass, one tiny launch
    steps, tiny, big = seen["wide"]
    assert steps == ce.CHUNK and tiny == 0 and big == ce.TINY_BIG, seen["wide"]  # the same chunk's pairs, counted by the wide form


def test_frozen_bus_big_pairs_past_twice_the_item_capacity(monkeypatch):
    # A lockdown freezes riders on the bus (Q8): 32 bus steps in every chunk, 8 200 big routes with an Infected rider ->
    # 262 400 distinct (big route, bus step) pairs at ESIM_HASH_LOG2=19, past 2 * items_cap = 262 144, the size of the list
    # before (ESIM_ERANGE); it is now sized min(items_cap / 4, big routes) x CHUNK_BUS_STEPS.
    monkeypatch.setenv("ESIM_HASH_LOG2", str(ce.FROZEN_HASH_LOG2))
    pop, params = ce.frozen_bus_big_pairs()
    run = OracleRun(pop, 96, ce.CHUNK_BUS_STEPS, **params)
    first = run.records[0]
    assert ce.bus_steps(first).all() and first["lockdown"].all()
    want = (pop.n_citizens // 66) * ce.CHUNK_BUS_STEPS
    assert want > 2 * ce.items_cap(ce.FROZEN_HASH_LOG2)
    seen = {}

    def observe(form, sim, i):
        if i < 0:
            _timed(sim, i)
        else:
            seen.setdefault(form, []).append(_timed(sim, i)[:1] + (sim.debug_counters()["n_route_pairs_big"],))

    run_forms(run, ("wide", "vax"), observe)
    for form, blocks in seen.items():
        assert blocks[0] == (ce.CHUNK_BUS_STEPS, want), (form, blocks)


@pytest.mark.parametrize("frozen", (False, True), ids=("bus8", "bus32"))
@pytest.mark.parametrize("grid", (None, 16), ids=("grid_default", "grid16"))
def test_small_route_pairs_fill_every_wavefront_stretch(grid, frozen, monkeypatch):
    # Every Infected rides its own route of 40 riders in every bus step of the chunk: a wavefront of k_chunk_marks with
    # items_per_wave / 4 entries registers entries x bus steps pairs, which is PAIR_K(items_per_wave, bus steps) exactly for 8
    # and for 32 bus steps.  A stretch one pair too short raises ESIM_ERANGE.
    if grid:
        monkeypatch.setenv("ESIM_GRID_CHUNK", str(grid))
    pop, params = ce.pair_k_tight(frozen)
    block = ce.CHUNK_BUS_STEPS if frozen else ce.CHUNK
    run = OracleRun(pop, 3 * block, block, **params)
    assert int(ce.bus_steps(run.records[0]).sum()) == (ce.CHUNK_BUS_STEPS if frozen else 8)
    seen = {}

    def observe(form, sim, i):
        if i < 0:
            _timed(sim, i)
        elif i == 0:
            seen[form] = _timed(sim, i)[0], sim.debug_counters()["items_per_wave"]

    run_forms(run, ("wide", "vax"), observe)
    for form, (steps, per_wave) in seen.items():
        assert steps == block and per_wave >= 4 and per_wave % 4 == 0, (form, seen[form])
        if grid:
            # 64 wavefronts for 300 entries: five entries in most stretches, all on their own routes in every bus step
            assert per_wave == 4 * 5, (form, seen[form])


def test_admission_boundary_hands_over_both_ways(monkeypatch):
    # ESIM_HASH_LOG2=19: chunks of up to 16 384 Infected run in one pass.  16 000 seeds and the first exposures take the chunks
    # through that bound from step 97 on and the seeds' recovery brings them back at step 337: one-pass chunks, then the next
    # form down (pipelined or sequential steps), then one-pass chunks again -- and the same records and states throughout.
    monkeypatch.setenv("ESIM_HASH_LOG2", str(ce.ADMISSION_HASH_LOG2))
    pop, params = ce.admission_boundary()
    block = 48
    run = OracleRun(pop, 480, block, **params)
    per_block = {}

    def observe(form, sim, i):
        if i < 0:
            _timed(sim, i)
        else:
            per_block.setdefault(form, []).append(_timed(sim, i)[0])

    run_forms(run, ("vax", "wide", "tp"), observe)
    for form, steps in per_block.items():
        full = [s == block for s in steps]
        none = [s == 0 for s in steps]
        # one-pass at the start (16 000 Infected), declined while more than 16 384 are Infected in every step (blocks 4-6,
        # steps 193-336: no chunk of any length fits), one-pass again after the seeds' recovery
        assert full[0] and full[1] and none[4] and none[5] and none[6] and any(full[7:]), (form, steps)


def test_tiny_form_task_queue_overflows_into_self_draw():
    # 12 Infected working in three workplaces of 3 000: 1 125 units of TINY_INLINE pairs against a queue of TINY_TASKS -- the
    # wavefront that finds the queue full draws the rest of its list itself
    pop, params = ce.tiny_task_spill()
    run = OracleRun(pop, 288, ce.CHUNK, **params)
    seen = {}

    def observe(form, sim, i):
        if i < 0:
            _timed(sim, i)
        elif i == 0:
            seen[form] = _timed(sim, i)

    run_forms(run, ("vax", "tinymax", "wide"), observe)
    for form in ("vax", "tinymax"):
        assert seen[form][0] == ce.CHUNK and seen[form][1] >= 1, (form, seen[form])
