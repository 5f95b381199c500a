"""esim_area_census / esim_area_series against tables computed with numpy from the CPU oracle (tests/_area_ref.py).
Every comparison is exact equality of integer arrays."""
import ctypes as C

import numpy as np
import pytest

import _area_ref
from epidemicsimulator_amd import Population, Simulator, _lib

pytestmark = pytest.mark.gpu

FIELDS = [f for f in _lib.RECORD_FIELDS if f != "reserved"]
STOPS = (180, 260, 300, 329, 700)
N_STEPS = _area_ref.FIXTURE_A_STEPS
S, E, I, R, V = range(5)


@pytest.fixture(scope="module")
def world():
    pop, ep = _area_ref.fixture_a()
    return pop, ep, _area_ref.reference_tables(pop, ep, N_STEPS, census_steps=STOPS)


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, "%s: shape %s, expected %s" % (what, got.shape, want.shape)
    if not (got == want).all():
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d entries differ, first at %s: got %d, expected %d"
                             % (what, len(bad), bad[0].tolist(), int(got[tuple(bad[0])]), int(want[tuple(bad[0])])))


def check_column_sums(col, records, s):
    """Column sums of a census taken after step s against the records (records[k] is step k + 1).

    A record holds the census of simulator.rs:178, taken BEFORE the step's vaccinations (simulator.rs:524-553), the
    citizens' state after the step has them applied.  So the sums equal the record of step s where the step vaccinated
    nobody; where it did, Vaccinated is what the NEXT record reports, Susceptible + Exposed have lost exactly the newly
    vaccinated, and Infected and Recovered equal the record (in this fixture nobody Infected or Recovered is ever
    vaccinated: the oracle vaccinates 99 Exposed citizens, tests/test_area_outputs.py pins the census)."""
    rec = records[s - 1]
    want = [int(rec[k]) for k in ("susceptible", "exposed", "infected", "recovered", "vaccinated")]
    col = [int(x) for x in col]
    if not int(rec["vaccination_active"]):
        assert col == want, "step %d: column sums %s, record %s" % (s, col, want)
        return
    assert col[I] == want[I] and col[R] == want[R], "step %d: %s vs record %s" % (s, col, want)
    if s < len(records):
        assert col[V] == int(records[s]["vaccinated"]), "step %d: Vaccinated %d, next record %d" % (s, col[V], int(records[s]["vaccinated"]))
    assert col[S] + col[E] == want[S] + want[E] - (col[V] - want[V])
    assert sum(col) == sum(want)


@pytest.mark.parametrize("pipeline", [None, 0], ids=["default", "sequential"])
def test_census_follows_the_oracle_and_the_calls_leave_the_run_alone(world, pipeline):
    """Checks 1 and 2: census CURRENT and HOME at the five stops, with the series calls interleaved; afterwards the records of
    all 700 steps and the final per-citizen state are the oracle's."""
    pop, ep, ref = world
    sim = Simulator(pop, ep)
    if pipeline is not None:
        sim.set_pipeline(pipeline)
    done = 0
    for s in STOPS:
        sim.run(s - done)
        done = s
        cur, home = sim.area_census("current"), sim.area_census("home")
        assert cur.dtype == np.uint32 and cur.shape == (pop.n_areas, 5)
        same(cur, ref["census"][s]["current"], "census CURRENT after step %d" % s)
        same(home, ref["census"][s]["home"], "census HOME after step %d" % s)
        check_column_sums(cur.sum(axis=0), ref["records"], s)
        check_column_sums(home.sum(axis=0), ref["records"], s)
        same(cur[:, I], sim.infected_per_area(), "Infected column vs infected_per_area() after step %d" % s)
        same(sim.area_series("infected"), ref["infected_rows"][:s], "Infected rows 1..%d" % s)
        same(sim.area_series("exposures"), ref["exposure_rows"][:s], "exposure rows 1..%d" % s)
        same(sim.area_series("infected", first_step=5, stride=7), ref["infected_rows"][4:s:7], "Infected rows, stride 7, at step %d" % s)
        same(sim.area_series("infected")[s - 1], cur[:, I], "Infected row %d vs the census" % s)
    got = sim.records_so_far()
    for f in FIELDS:
        same(got[f], ref["records"][f], "record field %s" % f)
    state = sim.download_state()
    for k in ("status", "timer", "current_building", "on_bus", "eligible"):
        same(state[k], ref["final_state"][k], "final state %s" % k)
    sim.close()


@pytest.fixture(scope="module")
def finished_run(world):
    pop, ep, ref = world
    sim = Simulator(pop, ep)
    sim.run(N_STEPS)
    yield sim
    sim.close()


def test_infected_series_all_rows_and_strides(world, finished_run):
    """Check 3: rows 1..700 at stride 1 are the oracle stepped row by row; strides 7 and 24 from step 5 are the matching
    rows of that table; the rows of the five stops are what the census gave there (the oracle's, by check 1)."""
    pop, ep, ref = world
    sim = finished_run
    full = sim.area_series("infected", first_step=1, n_rows=N_STEPS, stride=1)
    assert full.dtype == np.uint32
    same(full, ref["infected_rows"], "Infected rows 1..700")
    for stride in (7, 24):
        same(sim.area_series("infected", first_step=5, stride=stride), full[4::stride], "Infected rows from 5, stride %d" % stride)
        same(sim.area_series("infected", first_step=5, n_rows=3, stride=stride), full[4::stride][:3], "three rows, stride %d" % stride)
    for s in STOPS:
        same(full[s - 1], ref["census"][s]["current"][:, I], "Infected row %d vs the census at that step" % s)
    same(full.sum(axis=1), ref["records"]["infected"], "Infected row sums vs the records")


def test_exposure_series(world, finished_run):
    """Check 4: stride 1 is the reference table; its non-zero entries per area are exposures_per_output_area()'s lists;
    stride 24 is the stride-1 table summed in blocks of 24, the last block clipped."""
    pop, ep, ref = world
    sim = finished_run
    full = sim.area_series("exposures")
    same(full, ref["exposure_rows"], "exposure rows 1..700")
    lists = sim.exposures_per_output_area()
    assert {"OA%07d" % a: v for a, v in _area_ref.nonzero_lists(full).items()} == lists
    assert int(full.sum()) == 799
    blocks = sim.area_series("exposures", stride=24)
    n_blocks = (N_STEPS + 23) // 24
    padded = np.zeros((n_blocks * 24, pop.n_areas), np.uint32)
    padded[:N_STEPS] = full
    same(blocks, padded.reshape(n_blocks, 24, pop.n_areas).sum(axis=1), "exposure rows, stride 24")
    same(sim.area_series("exposures", first_step=5, stride=24), np.add.reduceat(full[4:], np.arange(0, N_STEPS - 4, 24), axis=0),
         "exposure rows from 5, stride 24")


def test_population_that_is_not_home_sorted(world):
    """Check 5: the citizens permuted, against the oracle run on the same permuted population, after 400 steps."""
    pop, ep, _ = world
    per = _area_ref.permuted(pop)
    ref = _area_ref.reference_tables(per, ep, 400, census_steps=(400,))
    sim = Simulator(per, ep)
    got = sim.run(400)
    for f in FIELDS:
        same(got[f], ref["records"][f], "record field %s" % f)
    same(sim.area_census("current"), ref["census"][400]["current"], "census CURRENT")
    same(sim.area_census("home"), ref["census"][400]["home"], "census HOME")
    same(sim.area_series("infected"), ref["infected_rows"], "Infected rows")
    same(sim.area_series("exposures"), ref["exposure_rows"], "exposure rows")
    sim.close()


def test_full_size_self_consistency():
    """Check 6: the york preset, default parameters, 5000 steps, no oracle run.

    The run is made in pieces of 50 steps with a census after each, so that every row of the stride-50 Infected series is
    compared with the census taken at that step (all areas, not only the sum).  A row sums to the record's `infected`
    minus the citizens that were Infected when the step's vaccinations took them (the record holds the census before
    them): equal wherever the step vaccinated nobody, never more."""
    pop = Population.synthetic("york")
    sim = Simulator(pop, _lib.default_params())
    at_stop = []
    for _ in range(100):
        sim.run(50)
        at_stop.append(sim.area_census("current")[:, I].copy())
    rec = sim.records_so_far()
    assert len(rec) == 5000
    rows = sim.area_series("infected", first_step=50, stride=50)
    same(rows, np.stack(at_stop), "Infected rows, stride 50, vs the census taken at those steps")
    sums, want = rows.sum(axis=1, dtype=np.int64), rec["infected"][49::50].astype(np.int64)
    # a step vaccinated nobody new iff the next record reports as many Vaccinated as its own (the last step has no next)
    v = rec["vaccinated"].astype(np.int64)
    quiet = np.append(v[50::50] == v[49:-1:50], not rec["vaccination_active"][-1])
    print("york: rows whose step vaccinated somebody new: %d of 100; Infected taken by those vaccinations, per row: %s"
          % (int((~quiet).sum()), (want - sums)[~quiet].tolist()))
    same(sums[quiet], want[quiet], "Infected row sums vs the records, steps without vaccinations")
    assert (sums <= want).all()
    total = sim.area_series("exposures", stride=5000)
    assert total.shape == (1, pop.n_areas)
    assert int(total.sum()) == int(rec["exposures_building"].sum(dtype=np.int64))
    cur, home = sim.area_census("current"), sim.area_census("home")
    # column sums against the last record: equal unless the last step vaccinated somebody (the record is the census before)
    want_last = [int(rec[-1][k]) for k in ("susceptible", "exposed", "infected", "recovered", "vaccinated")]
    for table in (cur, home):
        col = [int(x) for x in table.sum(axis=0)]
        print("york: column sums %s, last record %s" % (col, want_last))
        assert sum(col) == pop.n_citizens == sum(want_last)
        moved = col[V] - want_last[V]
        assert moved >= 0 and all(col[k] <= want_last[k] for k in (S, E, I, R))
        assert sum(want_last[k] - col[k] for k in (S, E, I, R)) == moved
        if not rec["vaccination_active"][-1]:
            assert col == want_last
    same(cur[:, I], sim.infected_per_area(), "Infected column vs infected_per_area()")
    same(home.sum(axis=1), np.bincount(pop.building_area[pop.home_building], minlength=pop.n_areas), "residents per area")
    sim.close()


def test_checkpoint_and_reset(world, tmp_path):
    """Check 7: a fresh Simulator that loads the checkpoint of step 300 answers as the uninterrupted run does at step 300;
    after reset() everybody is Susceptible but the seeds, Infected at home."""
    pop, ep, ref = world
    a = Simulator(pop, ep)
    a.run(300)
    path = str(tmp_path / "step300.ckpt")
    a.save_checkpoint(path)
    want = (a.area_census("current"), a.area_census("home"), a.area_series("infected"), a.area_series("exposures"))
    same(want[0], ref["census"][300]["current"], "census CURRENT at step 300")
    b = Simulator(pop, ep)
    b.load_checkpoint(path)
    got = (b.area_census("current"), b.area_census("home"), b.area_series("infected"), b.area_series("exposures"))
    for g, w, name in zip(got, want, ("census CURRENT", "census HOME", "Infected rows", "exposure rows")):
        same(g, w, name + " after load_checkpoint")
    same(got[2], ref["infected_rows"][:300], "Infected rows 1..300 after load_checkpoint")
    b.run(100)
    same(b.area_series("infected"), ref["infected_rows"][:400], "Infected rows 1..400, run continued from the checkpoint")
    b.reset()
    home_area = pop.building_area[pop.home_building]
    fresh = np.zeros((pop.n_areas, 5), np.uint32)
    fresh[:, S] = np.bincount(home_area, minlength=pop.n_areas)
    seeds = np.unique(pop.seeds)
    np.subtract.at(fresh[:, S], home_area[seeds], 1)
    np.add.at(fresh[:, I], home_area[seeds], 1)
    same(b.area_census("current"), fresh, "census CURRENT after reset")
    same(b.area_census("home"), fresh, "census HOME after reset")
    a.close()
    b.close()


def test_error_table(world):
    """Check 8: one assertion per line of the issue's error table."""
    pop, ep, _ = world
    lib = _lib.load()
    u32 = C.POINTER(C.c_uint32)
    census = np.zeros((pop.n_areas, 5), np.uint32)
    rows = np.zeros((4, pop.n_areas), np.uint32)
    pc, pr = census.ctypes.data_as(u32), rows.ctypes.data_as(u32)
    EINVAL, ESTATE, ERANGE = -1, -4, -5
    sim = Simulator(pop, ep)
    sim.run(10)
    ctx = sim._ctx
    assert lib.esim_area_census(None, _lib.AREA_CURRENT, pc) == EINVAL                      # null ctx
    assert lib.esim_area_series(None, _lib.SERIES_INFECTED, 1, 4, 1, pr) == EINVAL
    assert lib.esim_area_census(ctx, _lib.AREA_CURRENT, None) == EINVAL                     # null output
    assert lib.esim_area_series(ctx, _lib.SERIES_INFECTED, 1, 4, 1, None) == EINVAL
    assert lib.esim_area_census(ctx, 2, pc) == EINVAL                                       # unknown where
    assert lib.esim_area_series(ctx, 2, 1, 4, 1, pr) == EINVAL                              # unknown what
    assert lib.esim_area_series(ctx, _lib.SERIES_EXPOSURES, 1, 4, 0, pr) == EINVAL          # stride == 0
    assert lib.esim_area_series(ctx, _lib.SERIES_EXPOSURES, 1, 0, 1, pr) == EINVAL          # n_rows == 0
    bare = C.c_void_p()
    _lib.check(lib.esim_create(C.byref(ep), C.byref(bare)))
    assert lib.esim_area_census(bare, _lib.AREA_CURRENT, pc) == ESTATE                      # no population uploaded
    assert lib.esim_area_series(bare, _lib.SERIES_INFECTED, 1, 4, 1, pr) == ESTATE
    lib.esim_destroy(bare)
    assert lib.esim_area_series(ctx, _lib.SERIES_INFECTED, 0, 4, 1, pr) == ERANGE           # first_step == 0
    assert lib.esim_area_series(ctx, _lib.SERIES_INFECTED, 8, 4, 1, pr) == ERANGE           # last row = step 11 of 10
    assert lib.esim_area_series(ctx, _lib.SERIES_EXPOSURES, 2, 4, 3, pr) == ERANGE          # last row = step 11 of 10
    assert lib.esim_area_series(ctx, _lib.SERIES_INFECTED, 7, 4, 1, pr) == 0                # last row = step 10: fine
    assert lib.esim_area_series(ctx, _lib.SERIES_EXPOSURES, 1, 4, 3, pr) == 0
    with pytest.raises(_lib.EsimError):
        sim.area_series("infected", first_step=11)
    # a sticky device error comes back as the other read-backs report it
    probe = _lib.StepResult()
    _lib.check(lib.esim_debug_inject_error(ctx, ERANGE), ctx)
    want = lib.esim_read_records(ctx, 1, 1, C.byref(probe))
    assert want != 0
    assert lib.esim_area_census(ctx, _lib.AREA_HOME, pc) == want
    assert lib.esim_area_series(ctx, _lib.SERIES_INFECTED, 1, 4, 1, pr) == want
    sim.close()
