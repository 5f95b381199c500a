"""CPU side of the high vaccination rates (tests/_vax_rates.py): the numpy restatement of the rejection walk reproduces the
oracle, and every case reaches the regime its row of the table names -- batches per step, hash-set occupancy, the plan
condition, citizens vaccinated while Exposed, eligible citizens lost to buses -- so that no case of
tests/test_vax_rates_gpu.py can pass vacuously."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import _oracle
import _setting_ref as setting
import _vax_rates as vr
from epidemicsimulator_amd import _lib

EINVAL, ENODEVICE, ERANGE = -1, -2, -5


def test_the_table_needs_no_library():
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, ESIM_LIB=os.path.join(here, "no-such-library.so"), PYTHONPATH=os.pathsep.join([os.path.dirname(here), here]))
    code = ("import os; import _vax_rates as vr; from epidemicsimulator_amd import _lib; assert not os.path.exists(_lib.LIB_PATH); "
            "print(len(vr.CASES), vr.VACC_BATCH, vr.VACC_TABLE, vr.VACC_MAX_RATE, vr.VACC_WINDOW, vr.PLAN_W, sorted(vr.WORLDS))")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.split("\n")[0] == "8 4096 16384 8192 32768 4096 ['W24', 'W40']"


def test_the_constants_are_the_kernels_own():
    # read out of esim_device.h as text; the relations the kernels rely on, stated, not measured:
    # the hash set never fills -- at most rate - 1 keys before a step's last batch and one whole batch in it
    assert vr.VACC_MAX_RATE - 1 + vr.VACC_BATCH < vr.VACC_TABLE
    assert vr.VACC_TABLE & (vr.VACC_TABLE - 1) == 0 and vr.VACC_WINDOW % vr.VACC_BATCH == 0 and vr.PLAN_W == vr.VACC_BATCH
    assert max(c.rate for c in vr.CASES.values()) == vr.VACC_MAX_RATE
    assert {c.rate for c in vr.CASES.values()} >= {vr.VACC_BATCH - 1, vr.VACC_BATCH, vr.VACC_BATCH + 1, vr.VACC_MAX_RATE - 1}
    assert vr.BLOCK % 4 and vr.FREE_MAX % vr.BLOCK and vr.BLOCK % vr.FREE_MAX


def test_philox_restated_equals_the_oracles():
    L = _oracle.lib()
    seed = vr.BASE["seed"]
    key = (C.c_uint32 * 2)(seed & 0xFFFFFFFF, seed >> 32)
    ctrs = [(0, 1, 4, 0), (4095, 226, 4, 0), (28671, 450, 4, 0), (0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF)]
    got = vr.philox4x32_10(*(np.array(col, np.uint64) for col in zip(*ctrs)), seed)
    for i, ctr in enumerate(ctrs):
        out = (C.c_uint32 * 4)()
        L.orc_philox4x32_10((C.c_uint32 * 4)(*ctr), key, out)
        assert [int(w[i]) for w in got] == list(out), ctr
    # mulhi64(w0 << 32 | w1, n) against Python's integers
    for n in (24000, 40000, 2**32 - 1):
        w0, w1, _, _ = vr.philox4x32_10(np.arange(64, dtype=np.uint64), 300, 4, 0, seed)
        want = [(((int(a) << 32) | int(b)) * n) >> 64 for a, b in zip(w0, w1)]
        assert vr.candidates(seed, 300, 0, 64, n).tolist() == want


@pytest.mark.parametrize("name", sorted(vr.WORLDS))
def test_the_worlds(name):
    pop = vr.world(name)
    assert pop.n_citizens == vr.WORLDS[name]["n_citizens"] and pop.n_areas == vr.WORLDS[name]["n_areas"]
    assert vr.n_riders(pop) == vr.RIDERS[name]


@pytest.mark.parametrize("name", list(vr.CASES))
def test_the_walk_reproduces_the_oracle(name):
    """In every step under the programme the citizens whose status turns Vaccinated are exactly the chosen that were not
    Vaccinated already, the chosen are `rate` distinct eligible citizens, and the record says so."""
    case, tr, steps = vr.CASES[name], vr.trace(name), vr.walk(name)
    rec = tr["records"]
    assert len(rec) == case.steps and rec["disease_exists"].all() and (rec["time_step"] == np.arange(1, case.steps + 1)).all()
    assert len(steps) == case.steps - case.trigger + 1
    for s in steps:
        k = s["step"] - tr["first"]
        before, after, chosen = tr["status"][k - 1], tr["status"][k], s["chosen"]
        assert len(chosen) == case.rate == len(np.unique(chosen)) and vr.eligible_before_choice(tr, s["step"])[chosen].all()
        turned = np.flatnonzero((after == vr.V) & (before != vr.V))
        assert np.array_equal(turned, np.sort(chosen[before[chosen] != vr.V])), s["step"]
        assert (after[chosen] == vr.V).all()
        assert int(rec["vaccinated_now"][s["step"] - 1]) == case.rate                # the whole-set arm never runs
        assert int(rec["eligible_count"][s["step"] - 1]) == int(vr.eligible_before_choice(tr, s["step"]).sum()) > case.rate
        # stated: what keeps the probe loop of the hash set finite
        assert s["slots"] <= case.rate - 1 + vr.VACC_BATCH < vr.VACC_TABLE
        assert s["read"] == s["batches"] * vr.VACC_BATCH and case.rate <= s["slots"]
    assert not rec["vaccinated_now"][:case.trigger - 1].any() and not rec["vaccination_active"][:case.trigger - 1].any()


@pytest.mark.parametrize("name", list(vr.CASES))
def test_the_case_reaches_its_row_of_the_table(name):
    case, tr, steps = vr.CASES[name], vr.trace(name), vr.walk(name)
    rec = tr["records"]
    assert _create(**case.params) not in (EINVAL, ERANGE)                            # the library takes the parameter set
    assert int(rec["time_step"][np.argmax(rec["vaccinated_now"] > 0)]) == case.trigger
    under = rec[case.trigger - 1:]
    assert int(under["eligible_count"][0]) == case.eligible
    batches, slots = max(s["batches"] for s in steps), max(s["slots"] for s in steps)
    assert (batches, slots) == (case.batches, case.slots)
    assert batches >= vr.MIN_BATCHES[name] and slots >= vr.MIN_SLOTS.get(name, 0)
    if case.rate > vr.VACC_BATCH:
        assert min(s["batches"] for s in steps) >= 2                                 # one batch cannot suffice, by construction
    if case.rate in (vr.VACC_BATCH - 1, vr.VACC_BATCH):
        assert min(s["batches"] for s in steps) >= 2                                 # ... nor here: a batch of 4096 holds ineligible candidates
    # the cut at the rate falls inside the last batch, behind distinct live keys that are inserted and not chosen
    assert all(s["slots"] > case.rate for s in steps)
    # the plan condition of k_chunk_vax, elig_all > rate + riders: in every step under the programme, or in none
    plans = under["eligible_count"].astype(np.int64) > case.rate + vr.RIDERS[case.world]
    assert plans.all() if case.plans else not plans.any()
    # a sharded plan reads one batch of PLAN_W candidates per step: it reaches the rate in no step of these
    if name in ("rate_8192_early", "rate_4096"):
        assert min(s["batches"] for s in steps) >= 2 and vr.PLAN_W == vr.VACC_BATCH
    if name == "rate_1024":
        assert max(s["batches"] for s in steps) == 1


def test_thousands_are_vaccinated_while_exposed():
    # the relabelling of the census ahead (xf_adj, hist) for citizens that will never be Infected
    # (by the status a step earlier; Infected ones too at the lower rate, whose Infected interval ends with the vaccination)
    for name, least_e, least_i in (("rate_1024", 1000, 50), ("rate_8192_early", 100, 0)):
        tr, n_e, n_i = vr.trace(name), 0, 0
        for s in vr.walk(name):
            before = tr["status"][s["step"] - tr["first"] - 1][s["chosen"]]
            n_e += int((before == vr.E).sum()); n_i += int((before == vr.I).sum())
        assert n_e >= least_e and n_i >= least_i, (name, n_e, n_i)


def test_buses_take_eligible_citizens_behind_the_trigger():
    # what cuts or repairs a planned chunk: a citizen of the plan exposed on a bus before its turn
    case, rec = vr.CASES["rate_1024"], vr.trace("rate_1024")["records"]
    e = rec["eligible_count"].astype(np.int64)
    assert e[case.trigger - 1] - e[case.trigger - 1 + vr.FREE_MAX] >= 10
    assert (np.diff(e[case.trigger - 1:]) <= 0).all() and set(rec["mask_status"].tolist()) == {0, 1, 2}


@pytest.mark.parametrize("name", vr.REPLAYED)
def test_nothing_is_unexplained_in_the_replays_reference(name):
    case = vr.CASES[name]
    ref = setting.reference(case.pop, vr.params_of(name), case.steps)
    assert ref["unexplained"] == 0
    assert (ref["records"]["vaccinated_now"] == vr.trace(name)["records"]["vaccinated_now"]).all()
    if name == "rate_1024":
        assert int(ref["housemate_vaccinated"].sum()) >= 10


def test_the_town_of_the_seams():
    # a rate of exactly the eligible count takes the whole-set arm at the trigger and in every step behind it; 4097 a step walk
    pop = vr.town()
    p = dict(vr.BASE, vaccination_threshold=vr.TOWN_THRESHOLD, vaccination_rate=vr.TOWN_ELIGIBLE)
    orc = _oracle.Oracle(pop, _oracle.params_from_esim(_lib.default_params(**p)))
    rec = orc.run(vr.TOWN_TRIGGER + 60)
    orc.close()
    t = vr.TOWN_TRIGGER
    assert not rec["vaccinated_now"][:t - 1].any()
    assert (rec["vaccinated_now"][t - 1:] == vr.TOWN_ELIGIBLE).all() and (rec["eligible_count"][t - 1:] == vr.TOWN_ELIGIBLE).all()
    assert vr.VACC_BATCH + 1 < vr.TOWN_ELIGIBLE <= vr.VACC_MAX_RATE


def _create(**over):
    lib = _lib.load()
    ctx = C.c_void_p()
    rc = lib.esim_create(C.byref(_lib.default_params(**over)), C.byref(ctx))
    if rc == 0:
        lib.esim_destroy(ctx)
    return rc


@pytest.mark.parametrize("name", list(vr.CASES))
def test_create_accepts_every_case(name, has_gpu):
    rc = _create(**vr.CASES[name].params)
    assert rc == 0 if has_gpu else rc == ENODEVICE, rc
