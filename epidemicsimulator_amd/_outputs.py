"""The output families of Simulator, computed on the device from the state and the exposure log of the run as it stands:
area, group, settings, tree, chains, households, places, contacts, flows and events, the paired comparison with a kept
baseline, the curve summaries, the hospital burden and its comparison with a kept burden baseline.  _Outputs only holds methods: the state they use (lib, _ctx, _steps,
_n_groups, population, params) and the helpers _n_cols, _last and _complete_last are Simulator's (simulator.py); the
marshalling rules are _marshal's.

A `where` is given by name or by its code (_lib.AREA_*, _lib.BY_*): a name the call does not take raises ValueError before the
library is touched, a code passes through and the library refuses what it does not take.  A window first_step .. last_step
ends with last_step=None at the last step run; rows first_step, first_step + stride, ... go with n_rows=None up to there."""
import ctypes as C

import numpy as np

from . import _lib
from ._marshal import STATUS, default_rows, place_code, ptr, rate, sized, zeros


class _Outputs:
    # -- per Output Area (esim_area_census, esim_area_arrival, esim_area_series, esim_area_status_series) -------
    def area_census(self, where="current"):
        """uint32 [n_areas, 5]: citizens per Output Area and DiseaseStatus after the last completed step, counted on the
        device (esim_area_census).  where: "current" (the area of the building a citizen stands in) or "home"."""
        out = np.zeros((self.population.n_areas, 5), np.uint32)
        _lib.check(self.lib.esim_area_census(self._ctx, place_code(where, "current home"), ptr(out)), self._ctx)
        return out

    def area_arrival(self, where="home"):
        """uint32 [n_areas] (where="home") or [n_groups] (where="group"): the step at which a citizen of the area (by
        household) or group was first exposed, counted on the device from the exposure log (esim_area_arrival); 0 where an
        initially infected citizen lives, _lib.NEVER where the epidemic has not arrived in the steps run so far."""
        place = place_code(where, "current home group")
        out = np.zeros(self._n_cols(place), np.uint32)
        _lib.check(self.lib.esim_area_arrival(self._ctx, place, ptr(out)), self._ctx)
        return out

    def _series(self, call, codes, n_cols, first_step, n_rows, stride, lowest=1, outputs=1, flags=()):
        """One of the series calls: `outputs` arrays uint32 [n_rows, n_cols] (one: the array itself); n_rows=None: up to the
        last step run, from step `lowest` at the earliest.  flags: what the call takes between the stride and its outputs."""
        if n_rows is None:
            n_rows = default_rows(first_step, stride, self._steps, lowest)
        out = [np.zeros((max(0, int(n_rows)), n_cols), np.uint32) for _ in range(outputs)]
        _lib.check(call(self._ctx, *(int(c) for c in codes), int(first_step), int(n_rows), int(stride), *flags, *(ptr(a) for a in out)), self._ctx)
        return out[0] if outputs == 1 else tuple(out)

    def area_series(self, what, first_step=1, n_rows=None, stride=1):
        """uint32 [n_rows, n_areas] over the steps already run (esim_area_series): row i is step first_step + i * stride.
        what: "infected" (citizens Infected after that step, by the area they stand in) or "exposures" (building exposures
        of the `stride` steps from that one on, by area).  n_rows=None: up to the last step run."""
        code = {"infected": _lib.SERIES_INFECTED, "exposures": _lib.SERIES_EXPOSURES}.get(what, what)
        return self._series(self.lib.esim_area_series, (code,), self.population.n_areas, first_step, n_rows, stride)

    def area_status_series(self, what, where="home", first_step=1, n_rows=None, stride=1):
        """uint32 [n_rows, n_areas] over the steps already run (esim_area_status_series): row i is step first_step + i * stride.
        what: "susceptible", "exposed", "infected", "recovered", "vaccinated" (citizens with that status after the step, by
        the area of their household, where="home", or the area they stand in, where="current") or "incidence" (building and
        public-transport exposures of the `stride` steps from that one on, by the household's area; where="home" only).
        n_rows=None: up to the last step run."""
        code = dict(STATUS, incidence=_lib.AREA_SERIES_INCIDENCE).get(what, what)
        return self._series(self.lib.esim_area_status_series, (place_code(where, "current home"), code), self.population.n_areas, first_step, n_rows, stride)

    # -- the same by citizen group (esim_set_groups, esim_group_census, esim_group_series) -------
    def set_groups(self, labels, n_groups=None):
        """One label per citizen (copied to the device as uint16); n_groups=None: the largest label + 1.  labels=None drops
        them.  Population.age_bands() and Population.occupation_groups() make such labels."""
        if labels is None:
            _lib.check(self.lib.esim_set_groups(self._ctx, None, 0), self._ctx)
            self._n_groups = 0
            return
        raw = np.asarray(labels)
        if raw.shape != (self.population.n_citizens,):
            raise ValueError("set_groups: one label per citizen, got shape %s" % (raw.shape,))
        if raw.size and (int(raw.min()) < 0 or int(raw.max()) > 0xFFFF):
            raise ValueError("set_groups: labels must fit uint16")
        lab = np.ascontiguousarray(raw, np.uint16)
        if n_groups is None:
            n_groups = int(lab.max()) + 1 if lab.size else 1
        _lib.check(self.lib.esim_set_groups(self._ctx, ptr(lab), int(n_groups)), self._ctx)
        self._n_groups = int(n_groups)

    def group_census(self):
        """uint32 [n_groups, 5]: citizens per group and DiseaseStatus after the last completed step, counted on the device
        (esim_group_census)."""
        out = np.zeros((self._n_cols(_lib.BY_GROUP), 5), np.uint32)
        _lib.check(self.lib.esim_group_census(self._ctx, ptr(out)), self._ctx)
        return out

    def group_series(self, what, first_step=1, n_rows=None, stride=1):
        """uint32 [n_rows, n_groups] over the steps already run (esim_group_series): row i is step first_step + i * stride.
        what: "susceptible", "exposed", "infected", "recovered", "vaccinated" (citizens of the group with that status after
        the step) or "exposures" (building and public-transport exposures of the `stride` steps from that one on, by the
        group of the exposed citizen).  n_rows=None: up to the last step run."""
        code = dict(STATUS, exposures=_lib.GROUP_SERIES_EXPOSURES).get(what, what)
        return self._series(self.lib.esim_group_series, (code,), self._n_cols(_lib.BY_GROUP), first_step, n_rows, stride)

    # -- exposures by setting (esim_exposure_settings, esim_setting_series, esim_building_exposures) -------
    def exposure_settings(self):
        """(setting uint8 [n_citizens], building uint32 [n_citizens]): where every citizen was exposed, derived on the device
        from the exposure log by replaying the household draw (esim_exposure_settings).  setting: _lib.SETTING_HOUSEHOLD,
        SETTING_WORKPLACE, SETTING_SCHOOL, SETTING_TRANSPORT, or SETTING_NONE for a citizen never exposed and for the index
        cases; building: the building credited, _lib.NO_ROOM for public transport and for SETTING_NONE.  A tie between the
        household and the work side is credited to the household."""
        n = self.population.n_citizens
        setting, building = np.zeros(n, np.uint8), np.zeros(n, np.uint32)
        _lib.check(self.lib.esim_exposure_settings(self._ctx, ptr(setting), ptr(building)), self._ctx)
        return setting, building

    @staticmethod
    def _setting_mask(settings):
        if settings is None:
            return (1 << _lib.N_SETTINGS) - 1
        if isinstance(settings, (str, int, np.integer)):
            settings = (settings,)
        mask = 0
        for s in settings:
            code = _lib.SETTING_NAMES.index(s) if isinstance(s, str) else int(s)
            if not 0 <= code < _lib.N_SETTINGS:
                raise ValueError("setting_series: unknown setting %r" % (s,))
            mask |= 1 << code
        return mask

    def setting_series(self, where="setting", settings=None, first_step=1, n_rows=None, stride=1):
        """uint32 [n_rows, n_cols] over the steps already run (esim_setting_series): row i holds the exposures, in buildings
        and on public transport, of the `stride` steps from first_step + i * stride on, restricted to `settings` (names out
        of "household", "workplace", "school", "transport", or their codes; None: all four).  where: "setting" (four columns),
        "home" (by the Output Area of the household) or "group".  n_rows=None: up to the last step run."""
        place = place_code(where, "setting home group current")
        return self._series(self.lib.esim_setting_series, (place, self._setting_mask(settings)), self._n_cols(place), first_step, n_rows, stride)

    def _window(self, call, codes, shape, first_step, last_step):
        """One of the calls that count over a window into one table: uint32 of `shape` over steps first_step .. last_step."""
        out = np.zeros(shape, np.uint32)
        _lib.check(call(self._ctx, *codes, int(first_step), self._last(last_step), ptr(out)), self._ctx)
        return out

    def building_exposures(self, first_step=1, last_step=None):
        """uint32 [n_buildings]: the exposures of steps first_step .. last_step (None: the last step run) per building
        credited -- the hot-spot map (esim_building_exposures).  Public transport is not counted."""
        return self._window(self.lib.esim_building_exposures, (), self.population.n_buildings, first_step, last_step)

    # -- who infected whom (esim_transmission_tree, esim_offspring, esim_reproduction_series, esim_mixing_matrix) -------
    def _tables(self, call, codes, count, shape):
        """`count` uint32 tables of `shape`, the outputs of call(ctx, *codes, ...), as a tuple."""
        out = [np.zeros(shape, np.uint32) for _ in range(count)]
        _lib.check(call(self._ctx, *codes, *(ptr(a) for a in out)), self._ctx)
        return tuple(out)

    def transmission_tree(self):
        """(infector, n_candidates, generation), uint32 [n_citizens] each, derived on the device from the exposure log
        (esim_transmission_tree).  infector: the citizen every exposure is credited to -- one of the Infected that stood where
        it happened, picked by a Philox draw of its own --, _lib.NO_INFECTOR for the index cases and for citizens never
        exposed; n_candidates: how many there were to pick from; generation: 0 for an index case, the infector's + 1
        otherwise, _lib.NEVER for a citizen never exposed."""
        return self._tables(self.lib.esim_transmission_tree, (), 3, self.population.n_citizens)

    def offspring(self, first_step=1, last_step=None):
        """uint32 [n_citizens]: how many of the citizens exposed in steps first_step .. last_step (None: the last step run)
        every citizen infected (esim_offspring)."""
        return self._window(self.lib.esim_offspring, (), self.population.n_citizens, first_step, last_step)

    def reproduction_series(self, where="all", first_step=0, n_rows=None, stride=24):
        """(cases, offspring), uint32 [n_rows, n_cols] each (esim_reproduction_series): row i is the cohort exposed in the
        `stride` steps from first_step + i * stride on (step 0: the index cases), `cases` its size and `offspring` the
        citizens it infected, by the infector's column; offspring / cases is the cohort's case reproduction number.  where:
        "all" (one column), "home" (by the Output Area of the household) or "group".  n_rows=None: up to the last step run."""
        place = place_code(where, "all home group current")
        return self._series(self.lib.esim_reproduction_series, (place,), self._n_cols(place), first_step, n_rows, stride, lowest=0, outputs=2)

    def mixing_matrix(self, settings=None, first_step=1, last_step=None):
        """uint32 [n_groups, n_groups]: entry [g_infector, g_infectee] counts the transmissions of steps first_step ..
        last_step (None: the last step run) between the groups of set_groups, restricted to `settings` as setting_series
        takes them (esim_mixing_matrix)."""
        g = self._n_cols(_lib.BY_GROUP)
        return self._window(self.lib.esim_mixing_matrix, (self._setting_mask(settings),), (g, g), first_step, last_step)

    # -- transmission chains (esim_transmission_chains, esim_outbreaks, esim_transmission_ages) -------
    def transmission_chains(self):
        """(lineage, descendants), uint32 [n_citizens] each (esim_transmission_chains).  lineage: the position in seeds() of
        the index case at the root of the citizen's chain -- an index case carries its own --, _lib.NO_LINEAGE for a citizen
        never exposed; descendants: the citizens in the subtree below the citizen, itself not counted."""
        return self._tables(self.lib.esim_transmission_chains, (), 2, self.population.n_citizens)

    def outbreaks(self):
        """The outbreak every index case started (esim_outbreaks), a dict of uint32 [n_seeds] arrays in the order of seeds():
        seeds, size (the descendants of the index case), depth (the largest generation of its lineage, 0 when it infected
        nobody) and last_step (the last exposure step of its lineage, 0 when none).  Nothing per citizen comes to the host."""
        seeds, keys = self.seeds(), ("size", "depth", "last_step")
        out = zeros(keys, len(seeds))
        _lib.check(self.lib.esim_outbreaks(self._ctx, *(ptr(out[k]) for k in keys), len(seeds), C.byref(C.c_uint32(0))), self._ctx)
        return dict(out, seeds=seeds)

    def transmission_ages(self, first_step=1, last_step=None):
        """uint32 [4, 512]: entry [setting, a] counts the transmissions of steps first_step .. last_step (None: the last step
        run; the step is the infectee's) made in step a of the infector's infectious period, a = 0 its first Infected step
        (esim_transmission_ages).  For an infector that is not an index case the generation interval is a + exposed_time + 1."""
        return self._window(self.lib.esim_transmission_ages, (), (_lib.N_SETTINGS, _lib.AGE_BINS), first_step, last_step)

    # -- household outbreaks (esim_household_outbreaks, esim_household_final_sizes, esim_household_sar) -------
    def _by_key(self, call, codes, keys, shape, **dtypes):
        """{key: array of `shape`} as zeros() makes them, the outputs of call(ctx, *codes, ...) in the order of `keys`."""
        out = zeros(keys, shape, **dtypes)
        _lib.check(call(self._ctx, *codes, *(ptr(out[k]) for k in keys)), self._ctx)
        return out

    def household_outbreaks(self):
        """Per building, a dict of uint32 [n_buildings] arrays (esim_household_outbreaks): cases (the residents in the exposure
        log, index cases included), introductions (of those, the index cases and the cases not infected at home) and first_step
        (the smallest cohort step among them, _lib.NEVER without a case)."""
        return self._by_key(self.lib.esim_household_outbreaks, (), ("cases", "introductions", "first_step"), self.population.n_buildings)

    def household_final_sizes(self):
        """(final_size, introductions), uint32 [64, 64] each (esim_household_final_sizes): entry [n, k] counts the households
        of n residents with k cases, or with k introductions; the last bin of either index holds everything from 63 on.
        Nothing per building or per citizen comes to the host."""
        return self._tables(self.lib.esim_household_final_sizes, (), 2, (_lib.HH_BINS, _lib.HH_BINS))

    def _sar(self, who, call, codes, where, first_step, last_step, complete):
        """The two pair tables of household_sar and place_sar, uint64 [n_cols, n_cols] each."""
        place = place_code(where, "all group")
        last = self._complete_last(who, first_step, last_step) if complete else self._last(last_step)
        out = [np.zeros((self._n_cols(place),) * 2, np.uint64) for _ in range(2)]
        _lib.check(call(self._ctx, *codes, place, int(first_step), last, *(ptr(a) for a in out)), self._ctx)
        return tuple(out)

    def household_sar(self, where="all", first_step=0, last_step=None, complete=True):
        """(at_risk, secondary), uint64 [n_cols, n_cols] each (esim_household_sar): over the cases of cohort steps first_step ..
        last_step (step 0: the index cases), entry [g_case, g_contact] of at_risk counts the housemates still Susceptible when
        the case became infectious, of secondary those it infected at home; secondary / at_risk is the household secondary
        attack rate.  where: "all" (one cell) or "group".  last_step=None: the last step run.  complete=True clips last_step to
        the last complete cohort -- last_step + exposed_time + 1 + infected_time <= the steps run -- and raises ValueError when
        there is none; complete=False counts cohorts whose cases may still infect."""
        return self._sar("household_sar", self.lib.esim_household_sar, (), where, first_step, last_step, complete)

    # -- work place and school outbreaks (esim_place_outbreaks, esim_place_sizes, esim_place_sar) -------
    @staticmethod
    def _place_kind(kind):
        return int({"work": _lib.PLACE_WORK, "room": _lib.PLACE_ROOM, "school": _lib.PLACE_SCHOOL}.get(kind, kind))

    def place_outbreaks(self, kind="work"):
        """Per place, a dict of uint32 arrays (esim_place_outbreaks): members, cases (the members in the exposure log, index
        cases included), introductions (of those, the index cases and the cases not infected in the place's own setting) and
        first_step (the smallest cohort step among them, _lib.NEVER without a case).  kind: "work" (the non-school buildings
        and their workers, [n_buildings]), "room" (the school rooms and their participants, [n_rooms]) or "school" (the school
        buildings, all their rooms together, [n_buildings]).  A building or room without a member has 0 everywhere."""
        kind = self._place_kind(kind)
        n = self.population.n_rooms if kind == _lib.PLACE_ROOM else self.population.n_buildings
        return self._by_key(self.lib.esim_place_outbreaks, (kind,), ("members", "cases", "introductions", "first_step"), n)

    def place_sizes(self, kind="work"):
        """(final_size, introduced), uint32 [32, 32] each (esim_place_sizes): entry [bin(members), bin(k)] counts the places of
        the kind with k cases, or with k introductions; bin(x) = x below 16, then 16 for 16..31, 17 for 32..63 and so on."""
        return self._tables(self.lib.esim_place_sizes, (self._place_kind(kind),), 2, (_lib.PLACE_BINS, _lib.PLACE_BINS))

    def place_sar(self, kind="work", where="all", first_step=0, last_step=None, complete=True):
        """(at_risk, secondary), uint64 [n_cols, n_cols] each (esim_place_sar): household_sar for the work places (kind="work")
        or the school rooms (kind="room") -- entry [g_case, g_contact] of at_risk counts the colleagues or class-mates still
        Susceptible when the case became infectious, of secondary those it infected there.  where, first_step, last_step and
        complete as for household_sar, with the same clipping and the same ValueError."""
        return self._sar("place_sar", self.lib.esim_place_sar, (self._place_kind(kind),), where, first_step, last_step, complete)

    # -- contact-hours at risk (esim_contact_hours) -------
    def contact_hours(self, where="all", settings=None, first_step=1, last_step=None, per_case=False):
        """dict: hours and transmissions, uint64 [4, n_cols, n_cols] each, and with per_case=True per_case, uint32 [n_citizens]
        (esim_contact_hours).  hours[s, g_infected, g_susceptible] counts the contact-hours of setting s in steps first_step ..
        last_step (None: the last step run): a Susceptible citizen taking the draw of a gathering in a step in which an
        Infected citizen is a candidate of it.  transmissions is the mixing matrix split by setting; transmissions <= hours
        cell for cell.  per_case[j]: the contact-hours with j as the Infected side.  where: "all" (one cell) or "group";
        settings as setting_series takes them (the planes of the others stay 0)."""
        place = place_code(where, "all group")
        n_cols = self._n_cols(place)
        out = zeros(("hours", "transmissions"), (_lib.N_SETTINGS, n_cols, n_cols), u64=("hours", "transmissions"))
        cases = np.zeros(self.population.n_citizens, np.uint32) if per_case else None
        _lib.check(self.lib.esim_contact_hours(self._ctx, place, self._setting_mask(settings), int(first_step), self._last(last_step),
                                               ptr(out["hours"]), ptr(out["transmissions"]), ptr(cases)), self._ctx)
        if per_case:
            out["per_case"] = cases
        return out

    _rate = staticmethod(rate)

    def contact_rates(self, where="all", settings=None, first_step=1, last_step=None):
        """float64 [4, n_cols, n_cols]: transmissions per contact-hour, contact_hours()'s transmissions / hours, NaN where there
        was no contact-hour.  In households, work places and buses this is close to exposure_chance; in school rooms far above
        it (a room draw uses the Infected count of the whole school and is taken once per Infected of the room)."""
        got = self.contact_hours(where, settings, first_step, last_step)
        return rate(got["transmissions"], got["hours"])

    # -- area flows (esim_area_flows, esim_area_imports, esim_area_invasion, esim_lineage_areas) -------
    def _pairs(self, call, args):
        """The three [n] arrays of a sparse output, sized by one call with cap=0 before the real one (_marshal.sized) -- two
        replays, but buffers of 12 B per pair instead of 12 B per entry of the exposure log."""
        code, out = sized(lambda ptrs, cap, n: call(self._ctx, *args, *ptrs, cap, n), lambda n: [np.zeros(n, np.uint32) for _ in range(3)])
        _lib.check(code, self._ctx)
        return tuple(out)

    def area_flows(self, settings=None, first_step=1, last_step=None):
        """(src, dst, count), uint32 [n_pairs] each (esim_area_flows): the distinct pairs (Output Area of the infector, of the
        infectee) over the transmissions of steps first_step .. last_step (None: the last step run), restricted to `settings`
        as setting_series takes them, ascending by (src, dst), and how many transmissions each pair saw.  Sized by one call with
        cap=0 before the real one.  Nothing per citizen comes to the host."""
        last = self._last(last_step)
        return self._pairs(self.lib.esim_area_flows, (self._setting_mask(settings), int(first_step), last))

    def area_imports(self, settings=None, first_step=1, last_step=None):
        """Per Output Area, a dict of uint32 [n_areas] arrays (esim_area_imports) over the same transmissions as area_flows:
        local (both ends in the area), imported (the infectee lives there, the infector elsewhere) and exported (the other way
        round)."""
        last = self._last(last_step)
        return self._by_key(self.lib.esim_area_imports, (self._setting_mask(settings), int(first_step), last), ("local", "imported", "exported"), self.population.n_areas)

    def area_invasion(self):
        """The between-area invasion tree, a dict of [n_areas] arrays (esim_area_invasion): first_case (the earliest case
        living in the area, of several in one step the smallest citizen index; _lib.NO_INFECTOR without one), step (its cohort
        step, 0 for an index case, _lib.NEVER without a case: area_arrival("home")), source_area (the area of its infector,
        _lib.NO_AREA for an index case or no case) and setting (uint8, _lib.SETTING_NONE likewise).  step[source_area[a]] <
        step[a] wherever a source exists: a forest rooted at the areas of the index cases."""
        return self._by_key(self.lib.esim_area_invasion, (), ("first_case", "step", "source_area", "setting"), self.population.n_areas, u8=("setting",))

    def lineage_areas(self):
        """(lineage, area, count), uint32 [n_pairs] each (esim_lineage_areas): the distinct pairs (position in seeds() of the
        index case at the root of the chain, Output Area) over all cases that have a lineage, ascending, and how many cases of
        that lineage live there.  np.bincount(lineage) is the number of areas every introduction reached."""
        return self._pairs(self.lib.esim_lineage_areas, ())

    def pair_stats(self):
        """What the pair engine did in the last area_flows(), lineage_areas() or curve_summary() call, or peaks fold (esim_pair_stats): a dict of insert_ms,
        compact_ms, sort_ms (device time, HIP events), distinct, capacity and dropped."""
        ms, counts = (C.c_double * 3)(), (C.c_uint32 * 3)()
        _lib.check(self.lib.esim_pair_stats(self._ctx, ms, counts), self._ctx)
        return dict(insert_ms=ms[0], compact_ms=ms[1], sort_ms=ms[2], distinct=int(counts[0]), capacity=int(counts[1]), dropped=int(counts[2]))

    # -- superspreading events (esim_transmission_events, esim_routes) -------
    _EVENT_KEYS = ("step", "setting", "place", "bus", "size")

    def transmission_events(self, settings=None, first_step=1, last_step=None, min_size=1, order="key", limit=None):
        """The superspreading events (esim_transmission_events), a dict of [n_events] arrays: step, setting (uint8), place (the
        building, the room, or the position of the route in routes()), bus (0 off public transport) and size -- the
        transmissions of one step in one gathering (household, work place, school room, bus), over steps first_step ..
        last_step (None: the last step run), restricted to `settings` as setting_series takes them, events of at least
        min_size transmissions only.  order="key": ascending by (step, setting, place, bus), sized by one call with cap=0 before
        the real one; order="size": descending by size, ties ascending by that key, the first `limit` of them (None: all, sized
        the same way) in one call.  Nothing per citizen comes to the host."""
        if order not in ("key", "size"):
            raise ValueError("transmission_events: order must be 'key' or 'size', got %r" % (order,))
        window = (self._setting_mask(settings), int(first_step), self._last(last_step), int(min_size))
        by = _lib.EVENTS_BY_SIZE if order == "size" else _lib.EVENTS_BY_KEY

        def arrays(n):
            return zeros(self._EVENT_KEYS, n, u8=("setting",))

        def call(ptrs, cap, n):         # (the sizing call, the one without buffers, asks by key: nothing is sorted for a count)
            how = _lib.EVENTS_BY_KEY if ptrs[0] is None else by
            return self.lib.esim_transmission_events(self._ctx, *window, how, *ptrs, int(cap), n, None)
        if order == "size" and limit is not None:
            out, n = arrays(int(limit)), C.c_uint32(0)
            _lib.check(call([ptr(a) for a in out.values()], limit, C.byref(n)), self._ctx)
            return {k: v[:min(n.value, int(limit))] for k, v in out.items()}
        code, out = sized(call, arrays)
        _lib.check(code, self._ctx)
        return out

    def event_sizes(self, settings=None, first_step=1, last_step=None):
        """uint32 [4, 256] (the size table of esim_transmission_events): entry [s, b] counts the events of setting s with b
        transmissions over the window and the settings, the last bin open-ended; no list is built or sorted."""
        sizes, n = np.zeros((_lib.N_SETTINGS, _lib.EVENT_BINS), np.uint32), C.c_uint32(0)
        _lib.check(self.lib.esim_transmission_events(self._ctx, self._setting_mask(settings), int(first_step), self._last(last_step), 1, _lib.EVENTS_BY_SIZE,
                                                     *[None] * 5, 0, C.byref(n), ptr(sizes)), self._ctx)
        return sizes

    def routes(self):
        """The public transport routes (esim_routes), a dict of uint32 [n_routes] arrays: home_area, work_area and n_riders, in
        the order transmission_events numbers them (ascending by home area, then work area)."""
        code, out = sized(lambda ptrs, cap, n: self.lib.esim_routes(self._ctx, *ptrs, cap, n), lambda n: zeros(("home_area", "work_area", "n_riders"), n))
        _lib.check(code, self._ctx)
        return out

    # -- paired policy comparison: a kept baseline run and the run as it stands (esim_baseline_*, esim_compare*) -------
    @staticmethod
    def _compare_place(who, where):
        """`where` of the comparison calls as its code; anything but "all", "home" and "group" raises ValueError."""
        places = {"all": _lib.BY_ALL, "home": _lib.AREA_HOME, "group": _lib.BY_GROUP}
        if isinstance(where, str):
            if where not in places:
                raise ValueError("%s: where must be 'all', 'home' or 'group', got %r" % (who, where))
            return places[where]
        if isinstance(where, (bool, float)) or where not in places.values():
            raise ValueError("%s: where must be 'all', 'home' or 'group', got %r" % (who, where))
        return int(where)

    @staticmethod
    def _compare_rows(who, first_step, n_rows, stride, last):
        """(first_step, n_rows, stride) of event rows that may start at step 0, checked; n_rows=None: up to step `last` (a
        number, or a function that gives it: asked only once the other arguments stand)."""
        first, stride = int(first_step), int(stride)
        if first < 0 or stride < 1:
            raise ValueError("%s: first_step must be >= 0 and stride >= 1" % who)
        if n_rows is None:
            n_rows = default_rows(first, stride, int(last() if callable(last) else last), 0)
        if int(n_rows) < 1:
            raise ValueError("%s: no rows (first_step %d lies beyond the last step, or n_rows < 1)" % (who, first))
        return first, int(n_rows), stride

    def keep_baseline(self):
        """Keeps the exposure step of every citizen of the run as it stands on the device (esim_baseline_keep): the baseline
        that compare() and compare_series() set a later run against.  It survives reset, restart, snapshot and rollback."""
        _lib.check(self.lib.esim_baseline_keep(self._ctx), self._ctx)

    def baseline_info(self):
        """{"steps", "n_cases", "params"} of the baseline kept (esim_baseline_info): the steps it ran, the entries of its
        exposure log (index cases included) and the parameters it ran under."""
        steps, cases, p = C.c_uint32(0), C.c_uint32(0), _lib.Params()
        _lib.check(self.lib.esim_baseline_info(self._ctx, C.byref(steps), C.byref(cases), C.byref(p)), self._ctx)
        return {"steps": int(steps.value), "n_cases": int(cases.value), "params": p}

    def drop_baseline(self):
        """Forgets the baseline kept (esim_baseline_drop)."""
        _lib.check(self.lib.esim_baseline_drop(self._ctx), self._ctx)

    def _compare_last(self):
        """The last step both runs have, the window's default end (without a baseline: of this run; the library refuses then)."""
        steps = C.c_uint32(0)
        if self.lib.esim_baseline_info(self._ctx, C.byref(steps), None, None) != _lib.OK:
            return self._steps
        return min(self._steps, int(steps.value))

    def compare(self, where="all", first_step=0, last_step=None, citizens=False):
        """The run as it stands against the baseline kept (esim_compare), a dict: counts, uint64 [n_cols, 5] -- per column the
        citizens that are a case (exposed in steps first_step .. last_step; step 0: the index cases) in both runs, in the
        baseline only (averted), in this run only (added), and of those in both the ones exposed earlier and later here
        (_lib.CMP_*); delay, int64 [n_cols]: the sum of (step here - step in the baseline) over the cases of both;
        first_divergence: the first step at which the two histories differ, None when they are identical; and with
        citizens=True cls, uint8 [n_citizens]: 0 neither, 1 both, 2 averted, 3 added.  where: "all" (one column), "home" (by
        the Output Area of the household) or "group".  last_step=None: the last step of the shorter run."""
        place = self._compare_place("compare", where)
        first = int(first_step)
        if first < 0 or (last_step is not None and int(last_step) < first):
            raise ValueError("compare: steps %d..%s are no window" % (first, last_step))
        last = self._compare_last() if last_step is None else int(last_step)
        cols = self._n_cols(place)
        counts, delay, div = np.zeros((cols, _lib.CMP_N), np.uint64), np.zeros(cols, np.int64), C.c_uint32(0)
        cls = np.zeros(self.population.n_citizens, np.uint8) if citizens else None
        _lib.check(self.lib.esim_compare(self._ctx, place, first, last, ptr(counts), ptr(delay), C.byref(div), ptr(cls)), self._ctx)
        out = {"counts": counts, "delay": delay, "first_divergence": None if div.value == _lib.NEVER else int(div.value)}
        if citizens:
            out["cls"] = cls
        return out

    def compare_series(self, where="all", first_step=0, n_rows=None, stride=24, cumulative=False):
        """(baseline, current), uint32 [n_rows, n_cols] each (esim_compare_series): row i holds the cases of the `stride` steps
        from first_step + i * stride on in the baseline kept and in the run as it stands (step 0: the index cases); with
        cumulative=True the cases from first_step up to the row's last step.  baseline - current is the cases averted by row.
        where as for compare(); n_rows=None: up to the last step of the shorter run."""
        place = self._compare_place("compare_series", where)
        first, n_rows, stride = self._compare_rows("compare_series", first_step, n_rows, stride, self._compare_last)
        base, cur = (np.zeros((n_rows, self._n_cols(place)), np.uint32) for _ in range(2))
        _lib.check(self.lib.esim_compare_series(self._ctx, place, first, n_rows, stride, int(bool(cumulative)), ptr(base), ptr(cur)), self._ctx)
        return base, cur

    # -- the shape of the epidemic curve per column (esim_curve_summary) -------
    CURVE_STATUS = {"exposed": 1 << _lib.EXPOSED, "infected": 1 << _lib.INFECTED, "active": (1 << _lib.EXPOSED) | (1 << _lib.INFECTED)}
    CURVE_KEYS = ("peak", "peak_step", "steps_at_least", "first_at_least", "last_at_least", "person_steps")

    def _curve_args(self, who, where, status):
        """(`where` code, status mask) of the curve calls; a bad `status` is refused here, before any library call."""
        if status not in self.CURVE_STATUS:
            raise ValueError("Simulator.%s: status must be 'exposed', 'infected' or 'active', got %r" % (who, status))
        return place_code(where, "all home group current"), self.CURVE_STATUS[status]

    def curve_summary(self, where="home", status="infected", first_step=1, last_step=None, threshold=1):
        """The shape of the epidemic curve per column (esim_curve_summary), a dict of [n_cols] arrays over the steps first_step ..
        last_step (None: the last step run) of x_s = the citizens of the column whose status after step s is `status`
        ("exposed", "infected", or "active": either): peak = max x_s; peak_step = the first step that attains it (_lib.NEVER
        where the peak is 0); steps_at_least = the steps with x_s >= threshold, first_at_least and last_at_least the first and
        the last of them (_lib.NEVER without one); person_steps = the sum of x_s (uint64).  where: "all" (one column), "home"
        (by the Output Area of the household) or "group".  Computed on the device from the exposure log; no rows are built."""
        place, mask = self._curve_args("curve_summary", where, status)
        return self._by_key(self.lib.esim_curve_summary, (place, mask, int(first_step), self._last(last_step), int(threshold)), self.CURVE_KEYS,
                            self._n_cols(place), u64=("person_steps",))

    # -- hospital burden: admissions, bed occupancy and deaths over a finished run (esim_burden_*) -------
    BURDEN_KEYS = ("peak", "peak_step", "steps_at_least", "first_at_least", "last_at_least", "bed_steps", "admissions", "deaths")

    def set_burden(self, tables=None, **kw):
        """The severity tables in force (esim_burden_set): the dict of _lib.burden_tables, or its arguments as keywords.  Tables
        of several groups need set_groups with as many groups first.  They stay through restart, snapshot and rollback."""
        t = dict(tables) if tables is not None else _lib.burden_tables(**kw)
        arr = {k: np.ascontiguousarray(t[k], np.uint32) for k in ("admit_thr", "death_thr", "delay_cdf", "stay_cdf")}
        if arr["admit_thr"].shape != arr["death_thr"].shape or arr["admit_thr"].ndim != 1:
            raise ValueError("Simulator.set_burden: admit_thr and death_thr must have one entry per group each")
        p = _lib.BurdenParams(arr["admit_thr"].size, ptr(arr["admit_thr"]), ptr(arr["death_thr"]), int(t.get("delay_unit", 24)), arr["delay_cdf"].size,
                              ptr(arr["delay_cdf"]), int(t.get("stay_unit", 24)), arr["stay_cdf"].size, ptr(arr["stay_cdf"]))
        _lib.check(self.lib.esim_burden_set(self._ctx, C.byref(p)), self._ctx)

    def drop_burden(self):
        _lib.check(self.lib.esim_burden_drop(self._ctx), self._ctx)

    def burden(self):
        """The tables in force as set_burden takes them (esim_burden_get); EsimError (ESTATE) without any."""
        n = [C.c_uint32(0) for _ in range(5)]               # n_groups, delay_unit, n_delay, stay_unit, n_stay
        _lib.check(self.lib.esim_burden_get(self._ctx, C.byref(n[0]), None, None, C.byref(n[1]), C.byref(n[2]), None, C.byref(n[3]), C.byref(n[4]), None), self._ctx)
        admit, death = np.zeros(n[0].value, np.uint32), np.zeros(n[0].value, np.uint32)
        delay, stay = np.zeros(_lib.BURDEN_BINS, np.uint32), np.zeros(_lib.BURDEN_BINS, np.uint32)
        _lib.check(self.lib.esim_burden_get(self._ctx, None, ptr(admit), ptr(death), None, None, ptr(delay), None, None, ptr(stay)), self._ctx)
        return dict(admit_thr=admit, death_thr=death, delay_cdf=delay[:n[2].value].copy(), stay_cdf=stay[:n[4].value].copy(),
                    delay_unit=int(n[1].value), stay_unit=int(n[3].value))

    def burden_outcomes(self):
        """{"admit_step", "end_step": uint32 [n_citizens], _lib.NEVER where the citizen is no admitted case; "died": bool
        [n_citizens]} (esim_burden_outcomes).  A case occupies a bed after the steps admit_step .. end_step - 1 and, where it
        dies, dies at end_step; both may lie beyond the steps run."""
        out = self._by_key(self.lib.esim_burden_outcomes, (), ("admit_step", "end_step", "died"), self.population.n_citizens, u8=("died",))
        return dict(out, died=out["died"].astype(bool))

    def burden_series(self, what="occupancy", where="all", first_step=1, n_rows=None, stride=1):
        """uint32 [n_rows, n_cols] over the steps already run (esim_burden_series): row i is step first_step + i * stride.
        what: "occupancy" (beds occupied after that step), "admissions" or "deaths" (those of the `stride` steps from that one
        on).  where: "all" (one column), "home" or "group".  n_rows=None: up to the last step run."""
        code = {k: i for i, k in enumerate(_lib.BURDEN_NAMES)}.get(what, what)
        place = place_code(where, "all home group current")
        return self._series(self.lib.esim_burden_series, (place, code), self._n_cols(place), first_step, n_rows, stride)

    def burden_summary(self, where="all", first_step=1, last_step=None, threshold=1):
        """curve_summary of the bed occupancy over first_step .. last_step (None: the last step run), a dict of [n_cols] arrays
        (esim_burden_summary): peak, peak_step, steps_at_least, first_at_least, last_at_least as there, bed_steps (uint64) the
        sum of the curve, and the admissions and deaths of the window."""
        place = place_code(where, "all home group current")
        return self._by_key(self.lib.esim_burden_summary, (place, int(first_step), self._last(last_step), int(threshold)), self.BURDEN_KEYS,
                            self._n_cols(place), u64=("bed_steps",))

    # -- hospital burden across runs: the admitted cases kept as a list on the device (esim_burden_baseline_*, esim_burden_compare*) -------
    @staticmethod
    def _burden_what(what):
        return int({k: i for i, k in enumerate(_lib.BURDEN_NAMES)}.get(what, what))

    def keep_burden_baseline(self):
        """Keeps the admitted cases of the run as it stands as a list on the device (esim_burden_baseline_keep): the baseline
        that burden_compare() and burden_compare_series() set a later run against.  It survives reset, restart, snapshot and
        rollback; set_burden, drop_burden and an upload drop it."""
        _lib.check(self.lib.esim_burden_baseline_keep(self._ctx), self._ctx)

    def burden_baseline_info(self):
        """{"steps", "n_admitted", "n_died", "params"} of the burden baseline kept (esim_burden_baseline_info)."""
        n, p = [C.c_uint32(0) for _ in range(3)], _lib.Params()
        _lib.check(self.lib.esim_burden_baseline_info(self._ctx, *(C.byref(x) for x in n), C.byref(p)), self._ctx)
        return {"steps": int(n[0].value), "n_admitted": int(n[1].value), "n_died": int(n[2].value), "params": p}

    def drop_burden_baseline(self):
        """Forgets the burden baseline kept (esim_burden_baseline_drop)."""
        _lib.check(self.lib.esim_burden_baseline_drop(self._ctx), self._ctx)

    def burden_baseline_cases(self):
        """The admitted cases of the burden baseline (esim_burden_baseline_read), a dict of [n_admitted] arrays sorted by
        citizen: citizen, admit_step, end_step (uint32) and died (bool).  The steps may lie beyond the baseline's run."""
        keys = ("citizen", "admit_step", "end_step", "died")
        code, out = sized(lambda ptrs, cap, n: self.lib.esim_burden_baseline_read(self._ctx, *ptrs, cap, n), lambda n: zeros(keys, n, u8=("died",)))
        _lib.check(code, self._ctx)
        order = np.argsort(out["citizen"], kind="stable")
        return {k: (out[k][order].astype(bool) if k == "died" else out[k][order]) for k in keys}

    def _burden_compare_last(self):
        """The last step both runs have (without a baseline: of this run; the library refuses then)."""
        steps = C.c_uint32(0)
        if self.lib.esim_burden_baseline_info(self._ctx, C.byref(steps), None, None, None) != _lib.OK:
            return self._steps
        return min(self._steps, int(steps.value))

    def burden_compare(self, where="all", first_step=1, last_step=None):
        """The run as it stands against the burden baseline kept, over the steps first_step .. last_step (None: the last step
        of the shorter run), a dict of [n_cols] arrays (esim_burden_compare): bed_steps_baseline, bed_steps_current (uint64),
        admissions_baseline, admissions_current, deaths_baseline, deaths_current (uint32) -- the totals burden_summary gave at
        the keep and gives now -- and bed_steps_averted, admissions_averted, deaths_averted (int64): baseline - current."""
        place = self._compare_place("burden_compare", where)
        last = self._burden_compare_last() if last_step is None else int(last_step)
        keys = ("bed_steps_baseline", "bed_steps_current", "admissions_baseline", "admissions_current", "deaths_baseline", "deaths_current")
        out = self._by_key(self.lib.esim_burden_compare, (place, int(first_step), last), keys, self._n_cols(place), u64=keys[:2])
        for k in ("bed_steps", "admissions", "deaths"):
            out[k + "_averted"] = out[k + "_baseline"].astype(np.int64) - out[k + "_current"].astype(np.int64)
        return out

    def burden_compare_series(self, what="occupancy", where="all", first_step=1, n_rows=None, stride=24, cumulative=False):
        """(baseline, current), uint32 [n_rows, n_cols] each (esim_burden_compare_series): the rows of burden_series(what, where,
        first_step, n_rows, stride) of the burden baseline kept and of the run as it stands; with cumulative=True (admissions
        and deaths only) the events from first_step up to the row's last step.  n_rows=None: up to the last step of the
        shorter run."""
        place = self._compare_place("burden_compare_series", where)
        if n_rows is None:
            n_rows = default_rows(first_step, stride, self._burden_compare_last(), 1)
        return self._series(self.lib.esim_burden_compare_series, (place, self._burden_what(what)), self._n_cols(place), first_step, n_rows, stride,
                            outputs=2, flags=(int(bool(cumulative)),))
