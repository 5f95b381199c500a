"""Every execution form at the edges of the parameter space (tests/_param_edges.py; tests/test_param_edges.py checks on the CPU
that no case is inert).  Everything is exact integer equality against the CPU oracle, or numpy over it.
  a. parity of all eight forms in every case, the short chunks checked to have run as one-pass chunks
  b. the derived outputs (series tables, arrival, exposure log) at the timing and hour edges
  c. one context taken through the edges by esim_restart, a snapshot and rollback at a chunk of three steps, refused restarts
  d. a checkpoint at the encoding limit"""
import ctypes as C
import functools

import numpy as np
import pytest

import _area_status_ref as asr
import _arrival_ref
import _oracle
import _param_edges as pe
from epidemicsimulator_amd import Simulator, _lib
from test_parity_gpu import SMALL_LIMITS, OracleRun, assert_same_records, run_forms, set_form

pytestmark = pytest.mark.gpu

N = pe.N_STEPS
STATE_KEYS = ("status", "timer", "current_building", "on_bus", "eligible")
EINVAL = -1


@functools.lru_cache(maxsize=None)
def oracle_run(name, block=pe.BLOCK):
    return OracleRun(pe.world(), N, block, threads=4, **pe.CASES[name].params)


def whole(name):
    """(records of the N steps, state after them) of the case's oracle run."""
    run = oracle_run(name)
    return np.concatenate(run.records), run.states[-1]


def assert_state(sim, want, note=""):
    got = sim.download_state()
    for k in STATE_KEYS:
        assert (got[k] == want[k]).all(), "%s %s" % (k, note)


def params_of(name):
    return _lib.default_params(**pe.CASES[name].params)


# ---- a. parity in every execution form ----------------------------------------------------------------------------------------
def free_steps(records):
    """Steps before the first record of a running vaccination programme: no form has a reason not to draw them as chunks."""
    active = np.concatenate(records)["vaccination_active"] != 0
    return int(np.argmax(active)) if active.any() else len(active)


BLOCKS = [(name, pe.BLOCK) for name in pe.CASES] + [(name, 1) for name in pe.BLOCK_OF_ONE]


@pytest.mark.parametrize("name,block", BLOCKS, ids=["%s-block%d" % nb for nb in BLOCKS])
def test_every_form_matches_the_oracle(name, block):
    """All eight forms against one oracle run of 400 steps: every field of every record, the full state at every block's end.
    Blocks of 67 steps are no multiple of a Philox block of four steps nor of any case's chunk; blocks of one step make
    esim_run(1) meet a chunk of 1..4 steps."""
    case = pe.CASES[name]
    run = oracle_run(name, block)
    assert run.steps == N
    run_forms(run, SMALL_LIMITS)
    if name not in pe.SHORT_CHUNK:
        return
    # The short chunk is what was tested, not sequential steps in its place: the two forms that draw chunks under a programme
    # too run once more with kernel timing on, since the bursts count the steps they ran as one-pass chunks only while it is on
    # (events around every burst and every timed step; the eight runs above are untimed).
    seen = {}

    def observe(form, sim, i):
        if i < 0:
            sim.enable_kernel_timing(1)
        elif i == len(run.asked) - 1:
            seen[form] = dict(sim.vax_chunk_stats(), chunks=sim.chunk_timing()["steps"])

    run_forms(run, ("vax", "wide"), observe)
    # Every step before the one whose decision starts the vaccination programme is drawn as a one-pass chunk of
    # min(96, exposed_time + 1) steps (k_decide ends the chunk in front of that step, which runs sequentially: one step of
    # slack, and one for the step before it, whose chunk the look-ahead may decline).
    free = free_steps(run.records)
    assert free >= 8, free
    for form in ("vax", "wide"):
        got = seen[form]        # chunks: steps run as one-pass chunks; steps / cuts / repairs: those under the programme
        print("%s block %d form %s: chunk of %d steps; %d steps before the programme; %s" % (name, block, form, case.chunk, free, got))
        assert got["chunks"] >= free - 2, (form, got, free)
        if block >= 8:
            # Under the programme the chunks' vaccinations are planned ahead (level 3) and every call of at least 8 steps goes
            # on in chunks (run_steps).  A planned chunk stops only where a citizen of its plan was exposed before the
            # citizen's turn (a cut): the step at the cut runs sequentially and the next chunk starts behind it, until the
            # first cut arms the repair of plans, after which a chunk is walked again instead of cut.  So all N steps but the
            # two at the programme's start and one per cut ran as one-pass chunks of the case's length.
            assert got["steps"] > 0 and got["chunks"] >= got["steps"], (form, got)
            assert got["chunks"] >= N - 2 - got["cuts"], (form, got, free)
        else:
            # a call of fewer than 8 steps under a programme runs sequential steps by design (run_steps): blocks of one step
            # hand over there, and only the steps before the programme are chunks (of one step each: the call's length)
            assert got["steps"] == 0 and got["chunks"] <= free, (form, got, free)


# ---- b. derived outputs at the timing edges -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def derived_reference(name):
    pop, ep = pe.world(), params_of(name)
    tables = asr.reference_tables(pop, ep, N)
    orc = _oracle.Oracle(pop, _oracle.params_from_esim(ep))
    orc.set_threads(4)
    rec = orc.run(N)
    step, area = orc.exposures()
    orc.close()
    c = np.flatnonzero(step > 0)
    rows = np.stack([step[c].astype(np.int64), c.astype(np.int64), (area[c] == 0xFFFFFFFF).astype(np.int64)], 1)
    return tables, rec, step, rows[np.lexsort((rows[:, 1], rows[:, 0]))]


def log_rows(sim):
    cit, step, bus = sim.exposure_events()                  # (sorted by step, then citizen)
    return np.stack([step.astype(np.int64), cit.astype(np.int64), bus.astype(np.int64)], 1)


@pytest.mark.parametrize("form", ("vax", None), ids=("default", "sequential"))
@pytest.mark.parametrize("name", pe.TIMING)
def test_derived_outputs_at_the_timing_edges(name, form):
    pop = pe.world()
    tables, rec, exp_step, want_log = derived_reference(name)
    assert_same_records(tables["records"], rec)
    # a strided window that starts inside an Infected interval: at the step with the most Infected (infected_time 0 has no
    # such step: nobody is Infected in any record, and the window starts at step 5)
    inf = rec["infected"].astype(np.int64)
    inf = inf[:N - 30]                                      # (at least five rows of stride 7 behind it)
    first = int(np.argmax(inf)) + 1 if inf.max() > 0 else 5
    sim = Simulator(pop, params_of(name))
    set_form(sim, form)
    assert_same_records(sim.run(N), rec)
    for where, what in asr.TABLES:
        got = sim.area_status_series(what, where)
        assert got.shape == (N, pop.n_areas)
        assert (got == asr.expected(tables, where, what, N)).all(), (where, what, "full window")
        got = sim.area_status_series(what, where, first_step=first, stride=7)
        want = asr.expected(tables, where, what, N, first_step=first, stride=7)
        assert got.shape == want.shape and len(want) >= 4 and (got == want).all(), (where, what, "stride 7 from step %d" % first)
    want_arrival = _arrival_ref.arrival(_arrival_ref.home_area(pop), pop.n_areas, exp_step, pop.seeds)
    assert (sim.area_arrival("home") == want_arrival).all()
    got_log = log_rows(sim)
    assert got_log.shape == want_log.shape and (got_log == want_log).all(), "exposure logs differ as sets per step"
    sim.close()


# ---- c. one context through the edges -----------------------------------------------------------------------------------------
THROUGH = ("exposed_time_0", "exposed_time_200", "exposed_time_2", "encoding_limit_512", "hours_22_6", "seed_0")
#          chunk of 1         96 (capped)          3                 96                    the hours      back to the defaults' times and hours


def test_one_context_through_the_edges():
    """A single context restarted from one edge to the next, short and long chunks alternating: 96 -> 1 -> 96 (exposed_time
    200) -> 3 -> 96 (the 512 limit) -> the night shift -> the default times and hours.  Whatever is derived from the
    parameters (the chunk length, the seeds' words, the threshold table, the hour tables) has to follow every restart."""
    pop = pe.world()
    sim = Simulator(pop, params_of("seed_max"))             # default times and hours: chunks of 96
    rec, state = whole("seed_max")
    assert_same_records(sim.run(N), rec)
    assert_state(sim, state, "before the first restart")
    for name in THROUGH:
        sim.restart(params=params_of(name))
        rec, state = whole(name)
        try:
            assert_same_records(sim.run(N), rec)
            assert_same_records(sim.records_so_far(), rec)
        except AssertionError as e:
            raise AssertionError("after the restart to %s: %s" % (name, e)) from e
        assert_state(sim, state, "after the restart to %s" % name)
    sim.close()


def test_snapshot_and_rollback_at_a_chunk_of_three_steps():
    name, t = "exposed_time_2", 137
    rec, state = whole(name)
    sim = Simulator(pe.world(), params_of("encoding_limit_512"))
    sim.run(50)
    sim.restart(params=params_of(name))                     # the context comes to the case by a restart
    head = sim.run(t)
    sim.snapshot()
    assert sim.snapshot_step() == t
    for attempt in (0, 1):
        if attempt:
            sim.rollback()                                  # under the snapshot's own parameters
            assert sim._steps == t
        tail = sim.run(N - t)
        assert_same_records(np.concatenate([head, tail]), rec)
        assert_same_records(sim.records_so_far(), rec)
        assert_state(sim, state, "(pass %d)" % attempt)
    sim.close()


@pytest.mark.parametrize("chance", (float("nan"), -0.25, 1.5))
def test_restart_refuses_an_exposure_chance_that_is_no_probability(chance):
    name = "exposed_time_3"
    rec, state = whole(name)
    sim = Simulator(pe.world(), params_of(name))
    assert_same_records(sim.run(N), rec)
    bad = params_of("hours_22_6")                           # everything else about it would change the run
    bad.exposure_chance = chance
    assert sim.lib.esim_restart(sim._ctx, C.byref(bad)) == EINVAL
    assert b"probability" in sim.lib.esim_last_error(sim._ctx)
    assert sim.lib.esim_restart_seeded(sim._ctx, C.byref(bad), None, 0) == EINVAL
    # the run stands as it was ...
    assert_same_records(sim.records_so_far(), rec)
    assert_state(sim, state, "after the refused restart")
    # ... and so do the parameters in force: esim_reset goes back to step 0 under those of the last accepted restart or create
    sim.reset()
    assert_same_records(sim.run(N), rec)
    assert_state(sim, state, "after the reset")
    sim.close()


def test_create_answers_ok_at_the_boundary():
    # tests/test_param_edges.py pins the refusals without a device; with one, what the check accepts is ESIM_OK exactly
    lib = _lib.load()
    for over in (dict(exposed_time=96, infected_time=414), dict(vaccination_rate=8192), dict(max_steps=7600), dict(start_hour=1, end_hour=23),
                 dict(start_hour=9, end_hour=11), dict(exposure_chance=1.0), dict(exposure_chance=0.0)):
        ctx = C.c_void_p()
        assert lib.esim_create(C.byref(_lib.default_params(**over)), C.byref(ctx)) == _lib.ESIM_OK, over
        lib.esim_destroy(ctx)


# ---- d. checkpoint at the encoding limit ----------------------------------------------------------------------------------------
def test_checkpoint_at_the_encoding_limit(tmp_path):
    # exposed_time 96, infected_time 414: the citizen word's time field is at its widest
    name, at = "encoding_limit_512", 130
    rec, state = whole(name)
    a = Simulator(pe.world(), params_of(name))
    first = a.run(at)
    path = str(tmp_path / "limit.bin")
    a.save_checkpoint(path)
    a.close()
    b = Simulator(pe.world(), params_of(name))
    b.load_checkpoint(path)
    assert b._steps == at
    rest = b.run(N - at)
    assert_same_records(np.concatenate([first, rest]), rec)
    assert_same_records(b.records_so_far(), rec)
    assert_state(b, state, "after the resumed run")
    b.close()
