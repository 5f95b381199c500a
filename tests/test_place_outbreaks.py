"""Work place and school outbreaks, the CPU side: the two pair references of tests/_place_ref.py agree with each other and with
the settings and the tree they were built beside, every world holds what it is here for, and the ABI and Python surfaces of
the three calls are what include/esim.h says."""
import inspect
import os

import numpy as np
import pytest

import _household_ref as hh
import _place_ref as pl
import _setting_ref as ref_mod
import _tree_ref as tree
from epidemicsimulator_amd import Simulator, _lib
from epidemicsimulator_amd.ensemble import Ensemble

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def table_identities(ob, final_size, introduced):
    """What holds between the per-place arrays and the two tables, with no oracle needed.  The GPU tests call this too."""
    real = ob["members"] > 0
    assert (ob["cases"] <= ob["members"]).all() and (ob["introductions"] <= ob["cases"]).all()
    assert ((ob["first_step"] == pl.NONE) == (ob["cases"] == 0)).all()
    assert (ob["introductions"][ob["cases"] > 0] >= 1).all()                                   # every outbreak of a place was introduced
    assert final_size.shape == introduced.shape == (pl.BINS, pl.BINS)
    assert int(final_size.sum()) == int(introduced.sum()) == int(real.sum())                   # every place once
    per_bin = np.bincount(pl.bin_of(ob["members"][real]), minlength=pl.BINS)
    assert (final_size.sum(axis=1) == per_bin).all() and (introduced.sum(axis=1) == per_bin).all()   # ... and in the row of its size
    assert int(final_size[:, 0].sum()) == int((ob["cases"][real] == 0).sum())
    assert (np.triu(final_size, 1)[:16, :16] == 0).all()                                      # no more cases than members, where the bins are exact


def test_the_world_follows_the_kernels_tile():
    assert pl.TILE == pl.header_tile()
    pop, ep, n = pl.edge_world()
    assert pop.n_citizens == sum(pl.EDGE_WORK) + sum(pl.EDGE_ROOMS) + pl.EDGE_IDLE == 12204 and n == 40
    assert tuple(np.bincount(pop.home_building)[:pop.n_citizens // 4]) == (4,) * (pop.n_citizens // 4)
    place, n_places = pl.place_of(pop, "work")
    assert tuple(np.bincount(place[place >= 0], minlength=n_places)[-13:-1]) == pl.EDGE_WORK
    assert tuple(np.bincount(pop.room[pop.room != _lib.NO_ROOM])) == pl.EDGE_ROOMS


def test_bins():
    assert [int(pl.bin_of(x)) for x in (0, 1, 15, 16, 31, 32, 63, 64, 2 ** 20, 2 ** 31)] == [0, 1, 15, 16, 16, 17, 17, 18, 31, 31]
    assert int(pl.bin_of(2 ** 19)) == 31 and int(pl.bin_of(2 ** 19 - 1)) == 30


@pytest.mark.parametrize("name", pl.WORLDS)
def test_the_two_pair_references_agree(name):
    for kind in ("work", "room"):
        for first, last in pl.windows(name):
            for g in (0, 5):
                a = pl.pairs_outer(name, kind, first, last, g)
                b = pl.pairs_counting(name, kind, first, last, g, max_members=pl.OUTER_MAX)
                assert (a[0] == b[0]).all() and (a[1] == b[1]).all(), (kind, first, last, g)


@pytest.mark.parametrize("name", pl.WORLDS)
def test_reference_agrees_with_the_settings_and_the_tree(name):
    pop, ep, n, ref, sus, sref = pl.cached(name)
    school = pop.building_type == _lib.SCHOOL
    for kind in pl.KINDS:
        ob = pl.cached_outbreaks(name, kind)
        table_identities(ob, *pl.sizes(ob))
        inside = ob["cases"] - ob["introductions"]
        place, _ = pl.place_of(pop, kind)
        members = place >= 0
        assert (inside == np.bincount(place[members & (ref["setting"] == pl.OWN[kind])], minlength=len(inside))).all()
        if sref is not None and kind != "room":                      # the buildings _setting_ref credits the exposures to
            credited = ref_mod.building_counts(sref, pop, 1, n)
            which = school if kind == "school" else pop.building_type == _lib.WORKPLACE
            assert (inside[which] == credited[which]).all()
    rooms, schools = pl.cached_outbreaks(name, "room"), pl.cached_outbreaks(name, "school")
    for k in ("members", "cases", "introductions"):                  # a school is the sum over its rooms
        assert (np.bincount(pop.room_building, weights=rooms[k], minlength=pop.n_buildings) == schools[k]).all()
    for kind in ("work", "room"):
        at, sec = pl.cached_pairs(name, kind)
        assert (sec <= at).all()
        for g in (1, 5):
            at_g, sec_g = pl.cached_pairs(name, kind, 0, None, g)
            assert (sec_g <= at_g).all() and int(at_g.sum()) == int(at.sum())
            # over the whole run every transmission of the setting is a secondary case: the mixing matrix restricted to it
            assert (sec_g == tree.mixing_matrix(ref, pop, hh.labels(pop, g), g, mask=1 << pl.OWN[kind])).all()
            cuts = [0, 1, n // 3, n // 2 + 1, n + 1]                 # windows that partition the cohorts add up to the whole
            parts = [pl.cached_pairs(name, kind, lo, hi - 1, g) for lo, hi in zip(cuts[:-1], cuts[1:])]
            assert (sum(p[0] for p in parts) == at_g).all() and (sum(p[1] for p in parts) == sec_g).all()


def situation(name):
    """What a world is here for, from its reference alone (the GPU tests call this too).  The counts in the comments were
    measured on the oracle; the bounds are floors below them."""
    pop, ep, n, ref, sus, _ = pl.cached(name)
    st = tree.cohort_step(ref, pop)
    if name == "edge":
        work, rooms = pl.cached_outbreaks(name, "work"), pl.cached_outbreaks(name, "room")
        assert ref["empty"] == 0 and int((ref["setting"][ref["step"] > 0] == _lib.SETTING_NONE).sum()) == 0     # no unexplained exposure
        assert tuple(work["members"][work["members"] > 0]) == pl.EDGE_WORK and tuple(rooms["members"]) == pl.EDGE_ROOMS
        big = work["members"] >= 255
        assert (work["cases"][big] >= 6).all()                                              # 20 to 24 in the 255..257 class
        largest = np.argsort(work["members"])[-4:]
        assert (work["cases"][largest] >= 700).all() and (work["cases"][largest] < work["members"][largest]).all()   # 1 496 / 1 504 / 1 362 / 3 254
        assert int(((st >= 0) & (hh.first_infectious(ref, pop, ep)[1] > n)).sum()) >= 900   # 1 075 cases not yet infectious at step 40
        assert (rooms["cases"][rooms["members"] >= 63] == rooms["members"][rooms["members"] >= 63]).any()   # rooms with every member a case
        assert int((work["members"] == 1).sum()) == 1 and int((rooms["members"] == 1).sum()) == 1            # places without a pair
    elif name == "school":
        assert int((pl.cached_outbreaks(name, "work")["cases"] >= 2).sum()) >= 26           # 52 work places with at least 2 cases
        assert int((pl.cached_outbreaks(name, "room")["cases"] >= 2).sum()) >= 30           # 60 such rooms
    elif name in ("fixture_a", "situations"):
        vaccinated = (st < 0) & (sus < hh.FOREVER)                                          # 19 170 and 3 959 vaccinated citizens
        assert int(vaccinated.sum()) >= (9000 if name == "fixture_a" else 1900)
        place, _ = pl.place_of(pop, "work")
        assert int((vaccinated & (place >= 0)).sum()) >= 500                                 # susceptibility of members ends by vaccination


@pytest.mark.parametrize("name", ["edge", "school", "fixture_a", "situations"])
def test_every_world_holds_what_it_is_here_for(name):
    situation(name)


def test_abi_surface():
    text = open(os.path.join(ROOT, "include", "esim.h")).read()
    assert "#define ESIM_PLACE_BINS 32" in text and _lib.PLACE_BINS == 32
    assert "enum { ESIM_PLACE_WORK = 0, ESIM_PLACE_ROOM = 1, ESIM_PLACE_SCHOOL = 2 };" in text
    assert (_lib.PLACE_WORK, _lib.PLACE_ROOM, _lib.PLACE_SCHOOL) == (0, 1, 2)
    for decl in ("int  esim_place_outbreaks(esim_ctx *ctx, int kind, uint32_t *members, uint32_t *cases, uint32_t *introductions, uint32_t *first_step);",
                 "int  esim_place_sizes(esim_ctx *ctx, int kind, uint32_t *final_size, uint32_t *introduced);",
                 "int  esim_place_sar(esim_ctx *ctx, int kind, int where, uint32_t first_step, uint32_t last_step,",
                 "uint64_t *at_risk, uint64_t *secondary);   /* [n_cols * n_cols] each, not both NULL */"):
        assert decl in text
    assert "min(31, 12 + floor(log2 x))" in text
    lib = _lib.load()
    for name in ("esim_place_outbreaks", "esim_place_sizes", "esim_place_sar"):
        assert name in _lib.SYMBOLS and getattr(lib, name).restype is not None
    # a null context is refused before anything touches a device
    assert lib.esim_place_outbreaks(None, _lib.PLACE_WORK, None, None, None, None) == -1
    assert lib.esim_place_sizes(None, _lib.PLACE_ROOM, None, None) == -1
    assert lib.esim_place_sar(None, _lib.PLACE_WORK, _lib.BY_ALL, 0, 0, None, None) == -1


def test_python_surface(tmp_path):
    from epidemicsimulator_amd.ensemble import PlaceResult

    def defaults(f):
        return {k: p.default for k, p in inspect.signature(f).parameters.items() if p.default is not inspect.Parameter.empty}
    assert defaults(Simulator.place_outbreaks) == dict(kind="work") and defaults(Simulator.place_sizes) == dict(kind="work")
    assert defaults(Simulator.place_sar) == dict(kind="work", where="all", first_step=0, last_step=None, complete=True)
    assert list(inspect.signature(Ensemble.places).parameters) == ["self", "members", "n_steps", "kind", "where", "first_step", "last_step"]
    assert defaults(Ensemble.places) == dict(kind="work", where="all", first_step=0, last_step=None)
    # a hand-made result: two members, two groups
    fs = [np.zeros((32, 32), np.uint32), np.zeros((32, 32), np.uint32)]
    fs[0][3, 0], fs[0][3, 1], fs[1][3, 2], fs[1][17, 0] = 6, 7, 9, 4
    at = [np.array([[10, 0], [4, 2]], np.uint64), np.array([[30, 0], [0, 2]], np.uint64)]
    sec = [np.array([[1, 0], [2, 0]], np.uint64), np.array([[3, 0], [0, 1]], np.uint64)]
    res = PlaceResult.gathered([{"seed": 1}, {"seed": 2}], [(fs[0], fs[1]), (fs[1], fs[0])], list(zip(at, sec)), n_cols=2)
    assert res.members == [{"seed": 1}, {"seed": 2}]
    assert res.final_size.shape == res.introduced.shape == (2, 32, 32) and res.final_size.dtype == np.uint32
    assert res.final_size[0, 3, 1] == 7 and res.introduced[0, 3, 2] == 9 and res.final_size[1, 3, 2] == 9
    assert res.at_risk.shape == res.secondary.shape == (2, 2, 2) and res.at_risk.dtype == np.uint64
    sar = res.sar()
    assert sar.shape == (2, 2) and sar[0, 0] == 4 / 40 and sar[1, 0] == 2 / 4 and sar[1, 1] == 1 / 4 and np.isnan(sar[0, 1])
    rate = res.attack_rate_by_size()
    assert rate.shape == (32,) and rate[3] == 16 / 22 and rate[17] == 0.0 and np.isnan(rate[4])
    res.dump(str(tmp_path))
    got = np.load(tmp_path / "ensemble_places.npz")
    assert (got["final_size"] == res.final_size).all() and (got["introduced"] == res.introduced).all()
    assert (got["at_risk"] == res.at_risk).all() and (got["secondary"] == res.secondary).all()
    assert np.array_equal(got["sar"], sar, equal_nan=True) and np.array_equal(got["attack_rate_by_size"], rate, equal_nan=True)
    none = PlaceResult.gathered([], [], [], n_cols=3)
    assert none.final_size.shape == (0, 32, 32) and none.at_risk.shape == (0, 3, 3) and np.isnan(none.sar()).all()
