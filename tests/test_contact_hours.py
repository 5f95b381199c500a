"""Contact-hours at risk, the CPU side: the two numpy references of tests/_contact_ref.py -- what one observes in the oracle's
per-step states, and the closed rule of include/esim.h -- agree cell for cell on every world, every transmission of the tree is one
of the contact-hours, the worlds hold what the GPU tests rely on, and the ABI and Python surfaces are what include/esim.h says."""
import inspect
import os

import numpy as np
import pytest

import _chain_ref as chain
import _contact_ref as ref
import _tree_ref as tree
from epidemicsimulator_amd import Simulator, _lib
from epidemicsimulator_amd.ensemble import ContactResult, Ensemble
from test_households import situation

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = _lib.SETTING_TRANSPORT


@pytest.mark.parametrize("name", chain.ALL_WORLDS + ("edge",))
def test_the_rule_reproduces_what_the_oracle_shows(name):
    pop, ep, n, tr, lab, observed, rule, seen = ref.cached(name)
    bad = np.argwhere(observed.hours != rule.hours)
    assert bad.size == 0, "%s: %d cells differ, first (step, setting, g_infected, g_susceptible) %s: observed %d, rule %d" % (
        name, len(bad), bad[0], observed.hours[tuple(bad[0])], rule.hours[tuple(bad[0])])
    hours = rule.window()
    print(name, "hours", hours.sum(axis=(1, 2)), "transmissions", ref.transmissions(tr, lab, 5).sum(axis=(1, 2)))
    # by one cell: the sum over the groups
    one = ref.cached_rule(name, 1)
    assert (one.hours[:, :, 0, 0] == rule.hours.sum(axis=(2, 3))).all()
    # every transmission is one of the contact-hours, in every window
    busy = int(np.bincount(tr["step"][tr["step"] > 0]).argmax())
    for first, last in ((1, n), (max(1, n // 3), n // 2), (busy, busy)):
        for g, tab in ((5, rule), (1, one)):
            trans = ref.transmissions(tr, ref.labels_of(pop, g), g, first, last)
            assert (trans <= tab.window(first, last)).all(), "%s: more transmissions than contact-hours in steps %d..%d by %d" % (name, first, last, g)
    assert int(ref.transmissions(tr, lab, 5).sum()) == int((tr["infector"] != tree.NONE).sum())
    # per case: the same contact-hours, summed the other way
    per_case = rule.per_case()
    assert int(per_case.sum()) == int(hours.sum()) and (per_case == seen["per_case"].sum(axis=0)).all()
    half = rule.per_case(max(1, n // 3), n // 2, mask=0b1001)
    assert int(half.sum()) == int(rule.window(max(1, n // 3), n // 2, mask=0b1001).sum())
    # the bus bit the rule derives from the records is the one the states show
    assert (ref.bits(ep, tr["records"], n)[1] == seen["bus_seen"]).all() or not seen["world"].rides.any()


@pytest.mark.parametrize("name", ["school", "situations", "fixture_a", "bus"])
def test_all_four_settings_have_contact_hours(name):
    rule = ref.cached(name)[6]
    assert (rule.window().sum(axis=(1, 2)) > 0).all()
    if name == "situations":
        situation(name)                                              # vaccinated Infected citizens and a frozen bus


def test_the_edge_world_holds_its_edges():
    pop, ep, n, tr, lab, observed, rule, seen = ref.cached("edge")
    w, cap = seen["world"], int(ep.bus_capacity)
    assert sorted(len(v) for v in w.riders.values()) == [cap, cap + 1]
    workers = np.bincount(pop.work_building[w.has_work], minlength=pop.n_buildings)
    assert sorted(workers[workers > 0].tolist()) == [64, 65]
    assert np.bincount(pop.home_building).max() == 65 and int(ep.exposed_time) == 0
    hours = rule.window().sum(axis=(1, 2))
    assert hours[0] > 0 and hours[1] > 0 and hours[T] > 0
    # both routes carried an Infected rider beside a Susceptible one
    long_route = next(v for v in w.riders.values() if len(v) == cap + 1)
    mark = np.zeros(pop.n_citizens, np.uint16)
    mark[long_route] = 1
    by_route = ref.rule(pop, ep, n, tr, mark, 2, seen["vax"], seen["buses"], w).window()[T]
    assert by_route[0, 0] > 0 and by_route[1, 1] > 0 and by_route[0, 1] == 0 and by_route[1, 0] == 0


def test_abi_surface():
    text = open(os.path.join(ROOT, "include", "esim.h")).read()
    for decl in ("int  esim_contact_hours(esim_ctx *ctx, int where, uint32_t setting_mask, uint32_t first_step, uint32_t last_step,",
                 "uint64_t *hours /* [4 * n_cols * n_cols] or NULL */, uint64_t *transmissions /* same, or NULL */,",
                 "uint32_t *per_case /* [n_citizens] or NULL */);"):
        assert decl in text
    assert "transmissions <= hours cell for cell" in text
    lib = _lib.load()
    assert "esim_contact_hours" in _lib.SYMBOLS and lib.esim_contact_hours.restype is not None
    assert lib.esim_contact_hours(None, _lib.BY_ALL, 0xF, 1, 1, None, None, None) == -1    # a null context is refused before anything touches a device


def test_python_surface(tmp_path):
    def defaults(f):
        return {k: p.default for k, p in inspect.signature(f).parameters.items() if p.default is not inspect.Parameter.empty}
    assert defaults(Simulator.contact_hours) == dict(where="all", settings=None, first_step=1, last_step=None, per_case=False)
    assert defaults(Simulator.contact_rates) == dict(where="all", settings=None, first_step=1, last_step=None)
    assert list(inspect.signature(Ensemble.contacts).parameters) == ["self", "members", "n_steps", "where", "settings", "first_step", "last_step"]
    assert defaults(Ensemble.contacts) == dict(where="all", settings=None, first_step=1, last_step=None)
    # the NaN rule of contact_rates
    hours = np.zeros((4, 2, 2), np.uint64)
    trans = np.zeros((4, 2, 2), np.uint64)
    hours[0, 0, 0], trans[0, 0, 0], hours[1, 1, 0] = 40, 4, 7
    rate = Simulator._rate(trans, hours)
    assert rate.dtype == np.float64 and rate[0, 0, 0] == 0.1 and rate[1, 1, 0] == 0.0 and np.isnan(rate[3]).all() and int(np.isnan(rate).sum()) == 14
    # a hand-made result: two members, two groups
    other_h, other_t = hours.copy(), trans.copy()
    other_h[0, 0, 0], other_t[0, 0, 0], other_h[3, 0, 1], other_t[3, 0, 1] = 60, 1, 8, 2
    res = ContactResult.gathered([{"seed": 1}, {"seed": 2}], [dict(hours=hours, transmissions=trans), dict(hours=other_h, transmissions=other_t)], n_cols=2)
    assert res.members == [{"seed": 1}, {"seed": 2}]
    assert res.hours.shape == res.transmissions.shape == (2, 4, 2, 2) and res.hours.dtype == res.transmissions.dtype == np.uint64
    pooled = res.rate()
    assert pooled.shape == (4, 2, 2) and pooled[0, 0, 0] == 5 / 100 and pooled[3, 0, 1] == 2 / 8 and pooled[1, 1, 0] == 0.0 and np.isnan(pooled[2]).all()
    res.dump(str(tmp_path))
    got = np.load(tmp_path / "ensemble_contacts.npz")
    assert (got["hours"] == res.hours).all() and (got["transmissions"] == res.transmissions).all() and np.array_equal(got["rate"], pooled, equal_nan=True)
    none = ContactResult.gathered([], [], n_cols=3)
    assert none.hours.shape == (0, 4, 3, 3) and np.isnan(none.rate()).all()
