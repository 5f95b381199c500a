// esim_host_upload.h -- esim_upload_population in named steps, and the way back to step 0: esim_reset and esim_restart.
namespace {

// What the steps of an upload hand on to each other.
struct UploadHost {
    const esim_population *pop;
    uint32_t N, B, R, n_global;
    bool sharded;
    std::vector<uint8_t> fl;                     // static flags of every citizen (FL_*)
    std::vector<uint32_t> room_fixed;            // room of a school member, 0 for everybody else
    std::vector<uint32_t> route_off, riders, route_of;
    uint32_t n_routes = 0, max_route = 0, n_big_routes = 0;
    bool any_big = false;
    std::vector<uint32_t> res_off, res_idx, wrk_off, wrk_idx, room_off, room_idx;
    bool home_sorted = true;
    bool household_work = false;                 // a Household is the work place of a citizen who does not live in it
};

// ---- validate the population contract and derive the static flags
int upload_validate(esim_ctx_impl *c, UploadHost &u)
{
    const esim_population *pop = u.pop; const uint32_t N = u.N, B = u.B, R = u.R;
    if (!pop->home_building || !pop->work_building || !pop->room || !pop->flags || !pop->building_area || !pop->building_type)
        return fail(c, ESIM_EINVAL, "esim_upload_population: a required array is NULL");
    if (R && !pop->room_building) return fail(c, ESIM_EINVAL, "esim_upload_population: room_building is NULL");
    if (pop->n_seeds && !pop->seeds) return fail(c, ESIM_EINVAL, "esim_upload_population: seeds is NULL");
    u.n_global = pop->n_citizens_global ? pop->n_citizens_global : N;
    if ((uint64_t)pop->citizen_id_base + N > u.n_global) return fail(c, ESIM_EINVAL, "esim_upload_population: shard range exceeds n_citizens_global");
    u.sharded = u.n_global != N || pop->n_shared_buildings || pop->n_shared_rooms;
    u.fl.resize(N);
    for (uint32_t b = 0; b < B; ++b) {
        if (pop->building_area[b] >= pop->n_areas) return fail(c, ESIM_EINVAL, "esim_upload_population: building_area out of range");
        if (pop->building_type[b] > ESIM_SCHOOL) return fail(c, ESIM_EINVAL, "esim_upload_population: unknown building_type");
    }
    for (uint32_t r = 0; r < R; ++r)
        if (pop->room_building[r] >= B || pop->building_type[pop->room_building[r]] != ESIM_SCHOOL)
            return fail(c, ESIM_EINVAL, "esim_upload_population: room_building must name a School");
    u.room_fixed.assign(N, 0);
    for (uint32_t i = 0; i < N; ++i) {
        const uint32_t hb = pop->home_building[i], wb = pop->work_building[i];
        if (hb >= B || wb >= B) return fail(c, ESIM_EINVAL, "esim_upload_population: building index out of range");
        if (pop->building_type[hb] == ESIM_SCHOOL) return fail(c, ESIM_EINVAL, "esim_upload_population: a School cannot be a home");
        uint8_t f = pop->flags[i] & (FL_USES_PT | FL_MASK_COMPLIANT);
        if (pop->building_area[hb] == pop->building_area[wb]) f |= FL_SAME_AREA;
        if (hb != wb) {
            f |= FL_HAS_WORK;
            if (pop->building_type[wb] == ESIM_SCHOOL) {
                f |= FL_WORK_SCHOOL;
                if (pop->room[i] >= R || pop->room_building[pop->room[i]] != wb)
                    return fail(c, ESIM_EINVAL, "esim_upload_population: school member without a room of that school");
                u.room_fixed[i] = pop->room[i];
            }
            else if (pop->building_type[wb] == ESIM_HOUSEHOLD) u.household_work = true;
        }
        u.fl[i] = f;
    }
    for (uint32_t i = 0; i < pop->n_seeds; ++i)
        if (pop->seeds[i] >= N) return fail(c, ESIM_EINVAL, "esim_upload_population: seed index out of range");
    for (uint32_t i = 0; i < pop->n_shared_buildings; ++i)
        if (pop->shared_building_local[i] >= (int32_t)B) return fail(c, ESIM_EINVAL, "esim_upload_population: shared building out of range");
    for (uint32_t i = 0; i < pop->n_shared_rooms; ++i)
        if (pop->shared_room_local[i] >= (int32_t)R) return fail(c, ESIM_EINVAL, "esim_upload_population: shared room out of range");
    return ESIM_OK;
}

// FNV-1a over what the path reads of the population (checkpoints carry it, esim_checkpoint_restore compares it).  The seeds
// come last: *head receives the state before them, so that esim_restart_seeded can finish the hash with the list in force.
void fnv_mix(uint64_t &h, const void *p, size_t nbytes)
{
    const uint8_t *q = (const uint8_t *)p;
    for (size_t i = 0; i < nbytes; ++i) { h ^= q[i]; h *= 0x100000001b3ull; }
}

uint64_t hash_with_seeds(uint64_t head, const uint32_t *seeds, uint32_t n_seeds)
{
    if (n_seeds) fnv_mix(head, seeds, sizeof(uint32_t) * (size_t)n_seeds);
    return head;
}

uint64_t population_hash(const esim_population *pop, uint64_t *head)
{
    const size_t N = pop->n_citizens, B = pop->n_buildings, R = pop->n_rooms;
    uint64_t h = 0xcbf29ce484222325ull;
    fnv_mix(h, pop->home_building, sizeof(uint32_t) * N); fnv_mix(h, pop->work_building, sizeof(uint32_t) * N);
    fnv_mix(h, pop->room, sizeof(uint32_t) * N); fnv_mix(h, pop->flags, N);
    fnv_mix(h, pop->building_area, sizeof(uint32_t) * B); fnv_mix(h, pop->building_type, B);
    if (R) fnv_mix(h, pop->room_building, sizeof(uint32_t) * R);
    *head = h;
    return hash_with_seeds(h, pop->seeds, pop->n_seeds);
}

// ---- public transport routes: riders sharing (home area, work area), simulator.rs:181-186.
// Both travel directions group the same citizens, so one static list serves every bus step.
void upload_routes(UploadHost &u)
{
    const esim_population *pop = u.pop;
    std::vector<std::pair<uint64_t, uint32_t>> pairs;
    for (uint32_t i = 0; i < u.N; ++i)
        if (u.fl[i] & FL_USES_PT)
            pairs.emplace_back(((uint64_t)pop->building_area[pop->home_building[i]] << 32) | pop->building_area[pop->work_building[i]], i);
    std::sort(pairs.begin(), pairs.end());
    u.riders.resize(pairs.size()); u.route_of.assign(u.N, NO_ROUTE);
    for (size_t i = 0; i < pairs.size(); ++i) {
        if (i == 0 || pairs[i].first != pairs[i - 1].first) u.route_off.push_back((uint32_t)i);
        u.riders[i] = pairs[i].second;
        u.route_of[pairs[i].second] = (uint32_t)u.route_off.size() - 1;
    }
    u.n_routes = (uint32_t)u.route_off.size();
    u.route_off.push_back((uint32_t)pairs.size());
    for (uint32_t r = 0; r < u.n_routes; ++r) {
        const uint32_t sz = u.route_off[r + 1] - u.route_off[r];
        u.max_route = std::max(u.max_route, sz);
        if (sz > 64) { u.any_big = true; ++u.n_big_routes; for (uint32_t q = u.route_off[r]; q < u.route_off[r + 1]; ++q) u.fl[u.riders[q]] |= FL_BIG_ROUTE; }
    }
}

// ---- static member lists (the occupant lists the reference keeps per building:
// output_area.rs:172-180, simulator_builder.rs:1076,1100, building.rs:404-431)
void upload_member_lists(UploadHost &u)
{
    const esim_population *pop = u.pop;
    const std::vector<uint8_t> &fl = u.fl;
    auto csr = [](uint32_t n_keys, uint32_t n_items, auto key_of, auto use, std::vector<uint32_t> &off, std::vector<uint32_t> &idx) {
        off.assign((size_t)n_keys + 1, 0);
        for (uint32_t i = 0; i < n_items; ++i) if (use(i)) off[key_of(i) + 1]++;
        for (uint32_t k = 0; k < n_keys; ++k) off[k + 1] += off[k];
        idx.resize(off[n_keys]);
        std::vector<uint32_t> cur(off.begin(), off.end() - 1);
        for (uint32_t i = 0; i < n_items; ++i) if (use(i)) idx[cur[key_of(i)]++] = i;
    };
    csr(u.B, u.N, [&](uint32_t i) { return pop->home_building[i]; }, [&](uint32_t) { return true; }, u.res_off, u.res_idx);
    for (uint32_t i = 0; i < u.N && u.home_sorted; ++i) u.home_sorted = u.res_idx[i] == i;
    csr(u.B, u.N, [&](uint32_t i) { return pop->work_building[i]; },
        [&](uint32_t i) { return (fl[i] & FL_HAS_WORK) && !(fl[i] & FL_WORK_SCHOOL); }, u.wrk_off, u.wrk_idx);
    csr(u.R, u.N, [&](uint32_t i) { return u.room_fixed[i]; }, [&](uint32_t i) { return (fl[i] & FL_WORK_SCHOOL) != 0; }, u.room_off, u.room_idx);
}

uint32_t seed_te(const esim_ctx_impl *c) { return TE_BIAS - (c->P.exposed_time + 1u); }   // Infected(0) before step 1

// ---- what belonged to the population before goes; the population's own arrays, the member lists and the step's count tables
int upload_population_tables(esim_ctx_impl *c, const UploadHost &u)
{
    const esim_population *pop = u.pop; const uint32_t N = u.N, B = u.B, R = u.R;
    // a communicator belongs to the population it was set up for (its buffers are sized and its ranks checked against the
    // shard): a new upload invalidates it -- call esim_comm_init_* again afterwards
    comm_release(c);
    c->comm.fn = nullptr; c->comm.user = nullptr; c->comm.rank = 0; c->comm.world = 1;
    c->comm.xr = nullptr; c->comm.xr_n = 0;
    free_device(c);
    c->rs.seeds_dev = nullptr; c->rs.seeds_cap = 0;                // (freed with the rest; the ensemble accumulators go with the population)
    c->arrival = nullptr;
    c->ens = Ensemble();                                           // (no kind in force: every buffer and the members kept went with the rest)
    c->grp = Groups();                                             // (the labels belong to the population they were set for)
    c->snap = Snapshot();                                          // (so does a snapshot: its buffers went with the rest)
    c->base = Baseline();                                          // (and a kept baseline)
    c->beds = BedsBaseline();                                      // (and a kept burden baseline)
    c->burden = BurdenState();                                     // (and the severity tables: their groups are this population's labels)
    Dev &d = c->d;
    std::memset(&d, 0, sizeof d);
    d.n = N; d.n_global = u.n_global; d.id_base = pop->citizen_id_base; d.n_bld = B; d.n_room = R;
    d.n_pt = (uint32_t)u.riders.size(); d.n_routes = u.n_routes; c->n_routes = u.n_routes;
    d.max_route = u.max_route;
    c->route_tab.assign(3 * (size_t)u.n_routes, 0u);
    for (uint32_t r = 0; r < u.n_routes; ++r) {
        const uint32_t first = u.riders[u.route_off[r]];             // (every route has a rider)
        c->route_tab[r] = pop->building_area[pop->home_building[first]];
        c->route_tab[u.n_routes + r] = pop->building_area[pop->work_building[first]];
        c->route_tab[2 * (size_t)u.n_routes + r] = u.route_off[r + 1] - u.route_off[r];
    }
    int rc;
    if ((rc = dev_alloc(c, &d.cit, (size_t)N + 1))) return rc;
    if ((rc = dev_upload(c, &d.home, pop->home_building, N)) || (rc = dev_upload(c, &d.work, pop->work_building, N))) return rc;
    if ((rc = dev_upload(c, &d.room, u.room_fixed.data(), N))) return rc;
    if ((rc = dev_upload(c, &d.res_off, u.res_off.data(), u.res_off.size()))) return rc;
    if (!u.home_sorted) { if ((rc = dev_upload(c, &d.res_idx, u.res_idx.data(), u.res_idx.size()))) return rc; }
    else d.res_idx = nullptr;
    if ((rc = dev_upload(c, &d.wrk_off, u.wrk_off.data(), u.wrk_off.size())) || (rc = dev_upload(c, &d.wrk_idx, u.wrk_idx.data(), u.wrk_idx.size()))) return rc;
    if ((rc = dev_upload(c, &d.room_off, u.room_off.data(), u.room_off.size())) || (rc = dev_upload(c, &d.room_idx, u.room_idx.data(), u.room_idx.size()))) return rc;
    if ((rc = dev_upload(c, &d.room_bld, pop->room_building, R))) return rc;
    if ((rc = dev_upload(c, &d.bld_type, pop->building_type, B))) return rc;
    // the per-area read-backs: 4 B per building, and the count table of esim_area_census
    if ((rc = dev_upload(c, &d.bld_area, pop->building_area, B))) return rc;
    d.n_areas = pop->n_areas;
    if ((rc = dev_alloc(c, &c->area_cnt, (size_t)pop->n_areas * 5u))) return rc;
    const size_t per_parity = (size_t)B + R + u.n_routes;
    if ((rc = dev_alloc(c, &c->cnt_base, MARK_SLOTS * per_parity))) return rc;      // (esim_reset / esim_restart zero it)
    c->cnt_bytes = sizeof(uint32_t) * MARK_SLOTS * per_parity;
    if ((rc = dev_alloc(c, &d.exp_step, 2 * ((size_t)c->cap_steps + 2)))) return rc;
    if ((rc = dev_alloc_fill(c, &d.exp_part, (size_t)EXP_ROWS * 2u * FREE_MAX))) return rc;
    if ((rc = dev_alloc(c, &d.dec, FREE_MAX + 1))) return rc;
    return ESIM_OK;
}

// ---- the tables of the time-parallel chunks.  Every one is initialised at allocation: no kernel ever reads memory nobody
// wrote, whatever a diagnostics build leaves out -- and the consumers check what they read from these tables against the
// capacities, DESIGN.md 3.9.
int upload_chunk_tables(esim_ctx_impl *c, const UploadHost &u)
{
    const esim_population *pop = u.pop; const uint32_t N = u.N, B = u.B;
    Dev &d = c->d; int rc;
    // hash map of the time-parallel chunks: room for ~2 marks per (Infected, step) pair at < 1/2 load
    // slots for half the citizens (a quarter of that many items: a chunk in which up to ~3 % of the citizens are Infected
    // still runs in the one-pass form), between 2^20 and 2^26; ~440 B per slot, most of it spill counters that stay cold
    uint32_t cap = 1u << 20;
    while (cap < (1u << 26) && cap < N / 2u) cap <<= 1;
    if (const char *e = std::getenv("ESIM_HASH_LOG2")) cap = 1u << std::min(28, std::max(4, std::atoi(e)));
    d.hcap = cap;
    d.items_cap = cap / 4u;                     // load factor <= 1/4; one count vector of FREE_MAX steps per item
    if ((rc = dev_alloc_fill(c, &d.hkey, cap, 0xFF))) return rc;                              // HKEY_EMPTY
    if ((rc = dev_alloc_fill(c, &d.hitems, d.items_cap, 0xFF))) return rc;                    // ITEM_UNUSED
    if ((rc = dev_alloc_fill(c, &d.item_rec, d.items_cap))) return rc;
    if ((rc = dev_alloc_fill(c, &d.vec, (size_t)cap * FREE_MAX))) return rc;
    if ((rc = dev_alloc_fill(c, &d.slot_state, cap))) return rc;
    if ((rc = dev_alloc_fill(c, &d.slot_iv, (size_t)cap * SLOT_IV_STRIDE))) return rc;
    // deferred units: SUBQ queues; a queue that is full makes its producer draw the list itself, so the size is a
    // matter of speed only.  Room for the smaller of: every long member list marked in every step; a quarter of the
    // citizens -- twice over, since the queues fill unevenly.
    size_t units = 0;
    auto add_lists = [&](const std::vector<uint32_t> &off) {
        for (size_t i = 0; i + 1 < off.size(); ++i) {
            const size_t pairs = (size_t)(off[i + 1] - off[i]) * FREE_MAX;
            if (pairs > UNIT_INLINE) units += (pairs + UNIT_PAIRS - 1) / UNIT_PAIRS;
        }
    };
    add_lists(u.res_off); add_lists(u.wrk_off); add_lists(u.room_off);
    units = std::min<size_t>(units, (size_t)N / 8u + 65536u);
    d.unit_qcap = (uint32_t)std::max<size_t>(1024, units * 2u / SUBQ);
    if ((rc = dev_alloc_fill(c, &d.units, (size_t)d.unit_qcap * SUBQ, 0xFF))) return rc;      // code == UNIT_NOOP
    if ((rc = dev_alloc_fill(c, &d.route_pairs, (size_t)d.items_cap * (CHUNK_BUS_STEPS / 4u)))) return rc;   // (PAIR_K: up to CHUNK_BUS_STEPS / 4 per item id)
    // A (big route, bus step) pair is registered once a chunk, by the entry that first sets the step's bit on the route's item:
    // at most CHUNK_BUS_STEPS pairs per route item (k_decide), and at most one route item per entry -- items_cap / 4 of them
    // (k_chunk_marks' id-range check) and no more than there are big routes.  (2 * items_cap, the size before, is exceeded by a
    // lockdown that freezes riders on a bus: 32 bus steps in a chunk with more than items_cap / 16 big routes carrying an Infected.)
    d.big_pairs_cap = (uint32_t)std::max<size_t>(1, std::min<size_t>((size_t)d.items_cap / 4u, u.n_big_routes) * CHUNK_BUS_STEPS);
    if ((rc = dev_alloc_fill(c, &d.route_pairs_big, d.big_pairs_cap))) return rc;
    // (a school building's records are those of everybody who works or learns there: its members are in the room lists)
    std::vector<uint32_t> sch_members((size_t)B + 1, 0);
    for (uint32_t i = 0; i < N; ++i) if (u.fl[i] & FL_WORK_SCHOOL) sch_members[pop->work_building[i] + 1]++;
    for (uint32_t b = 0; b < B; ++b) sch_members[b + 1] += sch_members[b];
    std::vector<uint32_t> ovf_off(u.res_off.size());
    for (size_t i = 0; i < u.res_off.size(); ++i) ovf_off[i] = u.res_off[i] + u.wrk_off[i] + sch_members[i];
    if ((rc = dev_upload(c, &d.ovf_off, ovf_off.data(), ovf_off.size()))) return rc;
    c->longest_list = u.max_route;
    for (const std::vector<uint32_t> *off : { &u.res_off, &u.wrk_off, &u.room_off })
        for (size_t i = 1; i < off->size(); ++i) c->longest_list = std::max(c->longest_list, (*off)[i] - (*off)[i - 1]);
    {
        std::vector<int32_t> sch_of(B ? B : 1, -1);
        uint32_t n_sch = 0;
        for (uint32_t b = 0; b < B; ++b) if (pop->building_type[b] == ESIM_SCHOOL) sch_of[b] = (int32_t)n_sch++;
        d.n_sch = n_sch;
        if ((rc = dev_upload(c, &d.sch_of_bld, sch_of.data(), sch_of.size()))) return rc;
    }
    {
        // the records k_chunk_marks reads with one request each (Dev::where4, Dev::bld8), and the schools' difference arrays
        std::vector<uint4> w4(N ? N : 1);
        for (uint32_t i = 0; i < N; ++i) w4[i] = make_uint4(pop->home_building[i], pop->work_building[i], u.room_fixed[i], u.route_of[i]);
        if ((rc = dev_upload(c, &d.where4, w4.data(), w4.size()))) return rc;
        std::vector<BldRec> b8(B ? B : 1);
        for (uint32_t b = 0; b < B; ++b) b8[b] = BldRec{ u.res_off[b], u.res_off[b + 1], u.wrk_off[b], u.wrk_off[b + 1], (uint32_t)pop->building_type[b], ovf_off[b], ovf_off[b + 1], 0u };
        if ((rc = dev_upload(c, &d.bld8, b8.data(), b8.size()))) return rc;
        if ((rc = dev_alloc_fill(c, &d.sch_diff, (size_t)(d.n_sch ? d.n_sch : 1) * SD_REPL * 2u * FREE_MAX))) return rc;
    }
    d.ovf_room_base = ovf_off.back();
    d.ovf_n = d.ovf_room_base + u.room_off.back() + 1u;
    if ((rc = dev_alloc_fill(c, &d.ovf, (size_t)d.ovf_n))) return rc;
    d.n_wrk_idx = (uint32_t)u.wrk_idx.size(); d.n_room_idx = (uint32_t)u.room_idx.size();
    d.big_qcap = d.items_cap / SUBQ;             // (a slot is listed at most once a chunk, and there are at most items_cap of them)
    if ((rc = dev_alloc_fill(c, &d.big_list, (size_t)d.big_qcap * SUBQ * 3u))) return rc;
    if ((rc = dev_alloc_fill(c, &d.used_pref, CHUNK_WAVES_MAX + 1u))) return rc;
    if ((rc = dev_alloc_fill(c, &d.pair_cnt, 16384u)) || (rc = dev_alloc_fill(c, &d.used_cnt, 16384u))) return rc;
    if ((rc = dev_alloc_fill(c, &d.hot, (size_t)HOT_COUNT * HOT_STRIDE))) return rc;
    d.newexp_cap = N / SUBQ + 1u;                 // citizens with the same id & 63: nobody is listed twice in a chunk
    if ((rc = dev_alloc_fill(c, &d.newexp, (size_t)d.newexp_cap * SUBQ))) return rc;
    if ((rc = dev_alloc_fill(c, &d.cursor, (size_t)EXP_ROWS * FREE_MAX))) return rc;
    return ESIM_OK;
}

// ---- what the steps keep: touched lists, vaccination plan, census histogram, exposure log, control block, records, routes
int upload_step_tables(esim_ctx_impl *c, const UploadHost &u)
{
    const uint32_t N = u.N, B = u.B, R = u.R;
    Dev &d = c->d; int rc;
    const size_t per_parity = (size_t)B + R + u.n_routes;
    for (int p = 0; p < (int)MARK_SLOTS; ++p) {
        uint32_t *base = c->cnt_base + p * per_parity;
        d.cnt_bld[p] = base; d.cnt_room[p] = base + B; d.route_flag[p] = base + B + R;
        if ((rc = dev_alloc(c, &d.touched_bld[p], B)) || (rc = dev_alloc(c, &d.touched_room[p], R))) return rc;
        if ((rc = dev_alloc(c, &d.touched_route[p], u.n_routes)) || (rc = dev_alloc(c, &d.touched_route_big[p], u.n_routes))) return rc;
    }
    if ((rc = dev_alloc(c, &d.vax_ev, (size_t)FREE_MAX * VACC_MAX_RATE))) return rc;
    if ((rc = dev_alloc_fill(c, &d.vax_cnt, FREE_MAX)) || (rc = dev_alloc_fill(c, &d.vax_now, FREE_MAX))) return rc;
    if ((rc = dev_alloc_fill(c, &d.vax_delta, 4u * (FREE_MAX + 2u)))) return rc;
    if ((rc = dev_alloc_fill(c, &d.lost_list, LOST_CAP))) return rc;
    if ((rc = dev_alloc_fill(c, &d.xf_adj, FREE_MAX + 2u))) return rc;
    if ((rc = dev_alloc(c, &d.hist, TE_SLOTS)) || (rc = dev_alloc(c, &d.log, (size_t)N + 1)) || (rc = dev_alloc(c, &d.log_off, TE_SLOTS + 1))) return rc;
    {
        // the distinct seeds, for esim_restart (which writes their words and the head of the log from this array)
        const uint32_t *sd = nullptr;
        if ((rc = dev_upload(c, &sd, c->init_log.data(), c->init_log.size()))) return rc;
        c->rs.seeds_dev = const_cast<uint32_t *>(sd); c->rs.seeds_cap = c->init_log.size();
    }
    uint64_t lut[512];
    esim_threshold_lut(&c->P, lut);
    if ((rc = dev_upload(c, &d.thr, lut, 512))) return rc;
    if ((rc = dev_alloc(c, &d.ctrl, 1))) return rc;
    if ((rc = dev_alloc(c, &d.records, (size_t)c->cap_steps + 1))) return rc;
    if ((rc = dev_upload(c, &d.route_off, u.route_off.data(), u.route_off.size())) || (rc = dev_upload(c, &d.route_riders, u.riders.data(), u.riders.size()))) return rc;
    if ((rc = dev_upload(c, &d.route_of, u.route_of.data(), N))) return rc;
    const size_t big_scratch = u.any_big ? u.riders.size() : 0;
    if ((rc = dev_alloc(c, &d.bus_key, big_scratch)) || (rc = dev_alloc(c, &d.bus_idx, big_scratch))) return rc;
    if ((rc = dev_alloc(c, &d.bus_cnt, big_scratch)) || (rc = dev_alloc(c, &d.bus_flag, big_scratch))) return rc;
    params_to_dev(c);
    return ESIM_OK;
}

// ---- the shared tables of a shard and the exchange buffers (a context of one shard has them too: its kernels read them)
int upload_shard_tables(esim_ctx_impl *c, const UploadHost &u)
{
    const esim_population *pop = u.pop; const uint32_t B = u.B, R = u.R;
    Dev &d = c->d; int rc;
    d.n_shards = u.sharded ? 2u : 1u;
    d.n_shared_bld = pop->n_shared_buildings; d.n_shared_room = pop->n_shared_rooms;
    if ((rc = dev_upload(c, &d.shared_bld, pop->shared_building_local, pop->n_shared_buildings)) || (rc = dev_upload(c, &d.shared_room, pop->shared_room_local, pop->n_shared_rooms))) return rc;
    // the inverse of the shared tables: which shared slot a local building / room is (sharded chunks, k_shared_pack)
    std::vector<int32_t> of_b(B ? B : 1, -1), of_r(R ? R : 1, -1);
    for (uint32_t i = 0; i < pop->n_shared_buildings; ++i) if (pop->shared_building_local[i] >= 0) of_b[pop->shared_building_local[i]] = (int32_t)i;
    for (uint32_t i = 0; i < pop->n_shared_rooms; ++i) if (pop->shared_room_local[i] >= 0) of_r[pop->shared_room_local[i]] = (int32_t)i;
    if ((rc = dev_upload(c, &d.shared_of_bld, of_b.data(), of_b.size())) || (rc = dev_upload(c, &d.shared_of_room, of_r.data(), of_r.size()))) return rc;
    if ((rc = dev_alloc_fill(c, &d.xv, XV_HEADER + (size_t)FREE_MAX * (PLAN_W / 32u)))) return rc;
    if ((rc = dev_alloc_fill(c, &d.xc, FREE_MAX + 2u)) || (rc = dev_alloc_fill(c, &d.xl, FREE_MAX + 2u)) || (rc = dev_alloc_fill(c, &d.xe, XE_WORDS))) return rc;
    d.rank = 0; d.world = 1; d.xs = nullptr;
#ifdef ESIM_COUNT_WORK
    if ((rc = dev_alloc_fill(c, &d.work_cnt, (size_t)WK_N))) return rc;
#endif
#ifdef ESIM_WAVE_PROFILE
    if ((rc = dev_alloc_fill(c, &d.prof_buf, (size_t)16384 * 16))) return rc;
#endif
    c->xa_n = XA_HEADER + (size_t)d.n_shared_bld + d.n_shared_room;
    c->xb_n = XB_HEADER + VACC_WINDOW / 32u;
    if ((rc = dev_alloc_fill(c, &d.xa, c->xa_n)) || (rc = dev_alloc_fill(c, &d.xb, c->xb_n)) || (rc = dev_alloc_fill(c, &d.xf, FREE_MAX + 1))) return rc;
    return ESIM_OK;
}

// a pinned mirror of at least `want` elements (one element when want is 0): kept when it is long enough already
template <class T> int pinned_grow(esim_ctx_impl *c, T **p, size_t *have, size_t want)
{
    if (*have >= want) return ESIM_OK;
    if (*p) (void)hipHostFree(*p);
    *p = nullptr; *have = 0;
    HIP_TRY(c, hipHostMalloc((void **)p, sizeof(T) * std::max<size_t>(1, want), hipHostMallocDefault));
    *have = want;
    return ESIM_OK;
}

// ---- pinned mirrors (they outlive an upload: only the ones that are too short are made again)
int upload_pinned(esim_ctx_impl *c, const UploadHost &u)
{
    if (!c->pin.ctrl) HIP_TRY(c, hipHostMalloc((void **)&c->pin.ctrl, sizeof(Ctrl), hipHostMallocDefault));
    if (!c->rs.stage) HIP_TRY(c, hipHostMalloc((void **)&c->rs.stage, sizeof(*c->rs.stage), hipHostMallocDefault));
    if (!c->rs.ev) HIP_TRY(c, hipEventCreateWithFlags(&c->rs.ev, hipEventDisableTiming));
    if (int rc = pinned_grow(c, &c->pin.rec, &c->pin.rec_n, (size_t)c->cap_steps + 1)) return rc;
    return pinned_grow(c, &c->pin.area, &c->pin.area_n, (size_t)u.pop->n_areas * 5u);
}

// ---- grids, and the tuning knobs of the environment
void upload_tuning(esim_ctx_impl *c, const UploadHost &u)
{
    Tuning &t = c->tune;
    t.grid_citizens = grid_for(u.N, TPB, 2048);
    t.grid_infected = 1024;
    t.grid_expose = 1024;
    if (const char *e = std::getenv("ESIM_GRID_INFECTED")) t.grid_infected = (uint32_t)std::max(1, std::atoi(e));   // tuning knobs
    const char *gc = std::getenv("ESIM_GRID_CHUNK");
    t.grid_chunk_env = gc != nullptr;               // (small_chunk asks for it with every chunk it enqueues)
    if (gc) t.grid_chunk = (uint32_t)std::min((int)(CHUNK_WAVES_MAX * 64u / TPB), std::max(16, std::atoi(gc) / 16 * 16));   // whole groups of 64 wavefronts
    if (std::getenv("ESIM_TRACE_HOST")) c->tm.host_trace = true;
    if (const char *e = std::getenv("ESIM_VAX_REPAIR")) { t.vax_repair = std::atoi(e) != 0; t.vax_repair_always = std::atoi(e) >= 2; }
    if (const char *e = std::getenv("ESIM_TINY_PAIRS")) t.tiny_pairs = (uint32_t)std::max(0, std::atoi(e));
    if (const char *e = std::getenv("ESIM_SMALL_GRID")) t.small_grid = (uint32_t)std::max(0, std::atoi(e) / 16 * 16);
    if (const char *e = std::getenv("ESIM_SMALL_MULT")) t.small_mult = (uint32_t)std::min(16, std::max(1, std::atoi(e)));
    if (const char *e = std::getenv("ESIM_DRAW_MULT")) t.draw_mult = (uint32_t)std::min(4, std::max(1, std::atoi(e)));      // (16 384 wavefronts at most: Dev::pair_cnt)
    if (const char *e = std::getenv("ESIM_UNITS_MULT")) t.units_mult = (uint32_t)std::min(16, std::max(1, std::atoi(e)));
    if (const char *e = std::getenv("ESIM_GRID_EXPOSE")) t.grid_expose = (uint32_t)std::max(1, std::atoi(e));
    t.pair_log2 = 0u;
    if (const char *e = std::getenv("ESIM_PAIR_LOG2")) t.pair_log2 = (uint32_t)std::min(31, std::max(6, std::atoi(e)));     // (at least 64 slots)
    t.grid_cap = 0u;
    if (const char *e = std::getenv("ESIM_GRID_CAP")) t.grid_cap = (uint32_t)std::max(1, std::atoi(e));                     // (tests only: the output kernels' grids)
    t.merge_piece = 0u;
    if (const char *e = std::getenv("ESIM_MERGE_PIECE")) t.merge_piece = (uint32_t)std::min(1 << 30, std::max(4, (std::atoi(e) + 3) / 4 * 4));   // (tests only: whole groups of four cells)
    c->launches = LaunchLog();
}

}  // namespace

extern "C" int esim_upload_population(esim_ctx *ctx, const esim_population *pop)
{
    esim_ctx_impl *c = CTX(ctx);
    if (!c || !pop) return fail(c, ESIM_EINVAL, "esim_upload_population: null argument");
    HIP_TRY(c, hipSetDevice(c->P.device));
    UploadHost u;
    u.pop = pop; u.N = pop->n_citizens; u.B = pop->n_buildings; u.R = pop->n_rooms;
    int rc;
    if ((rc = upload_validate(c, u))) return rc;
    c->pop_hash = population_hash(pop, &c->pop_hash_head);
    upload_routes(u);
    upload_member_lists(u);
    // initial state: everyone Susceptible at home (citizen.rs:139-162), seeds Infected(0)
    c->init_state.resize(u.N);
    for (uint32_t i = 0; i < u.N; ++i) c->init_state[i] = CW_MAKE(TE_SUSCEPTIBLE, (uint32_t)u.fl[i]);
    c->init_log.clear();
    for (uint32_t i = 0; i < pop->n_seeds; ++i) {
        const uint32_t sc = pop->seeds[i];
        if (CW_TE(c->init_state[sc]) != seed_te(c)) { c->init_state[sc] = CW_MAKE(seed_te(c), (uint32_t)u.fl[sc]); c->init_log.push_back(sc); }
    }
    if ((rc = upload_population_tables(c, u))) return rc;
    if ((rc = upload_chunk_tables(c, u))) return rc;
    if ((rc = upload_step_tables(c, u))) return rc;
    if ((rc = upload_shard_tables(c, u))) return rc;
    if ((rc = upload_pinned(c, u))) return rc;
    upload_tuning(c, u);
    c->household_work = u.household_work;
    c->uploaded = true;
    return esim_reset(ctx);
}

namespace {

// The control block before step 1.
void initial_ctrl(const esim_ctx_impl *c, Ctrl *h)
{
    const uint32_t n_seeds = (uint32_t)c->init_log.size();
    std::memset(h, 0, sizeof *h);
    h->t = 1;
    h->mask = ESIM_MASK_NONE;
    h->n_susceptible = c->d.n - n_seeds;
    h->log_len = n_seeds;
}

// What the host knows of the run, back at step 1 (esim_reset and esim_restart; the device side is theirs).
void rewind_host(esim_ctx_impl *c)
{
    c->host_t = 1;
    c->stop_flag_dev = 0;
    c->last_chunk_pairs = (uint32_t)c->init_log.size();
    c->vax_chunk_steps = 0; c->vax_chunk_cuts = 0; c->elig_seen = false; c->repair_armed = false; c->quiet = false;
    c->pin.track = false; c->pin.ctrl_fresh = false;
    c->rest_t = 0;
    c->seam = Seam();                                              // (the history that starts here is drawn under one parameter set)
    c->draw_seam = DrawSeam();
    c->tm.clear();
}

}  // namespace

extern "C" int esim_reset(esim_ctx *ctx)
{
    esim_ctx_impl *c = CTX(ctx);
    if (!c || !c->uploaded) return fail(c, ESIM_ESTATE, "esim_reset: no population uploaded");
    if (int rc = drain(c)) return rc;
    const Dev &d = c->d;
    const uint32_t n_seeds = (uint32_t)c->init_log.size();
    Ctrl h;
    initial_ctrl(c, &h);
    HIP_TRY(c, hipMemcpy(d.ctrl, &h, sizeof h, hipMemcpyHostToDevice));
    if (d.n) HIP_TRY(c, hipMemcpy(d.cit, c->init_state.data(), sizeof(uint32_t) * (size_t)d.n, hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemset(c->cnt_base, 0, c->cnt_bytes));
    HIP_TRY(c, hipMemset(d.exp_step, 0, sizeof(uint32_t) * 2 * ((size_t)c->P.max_steps + 2)));
    HIP_TRY(c, hipMemset(d.records, 0, sizeof(esim_step_result) * ((size_t)c->P.max_steps + 1)));
    // census histogram and exposure log: the seeds are Infected(0) before step 1, i.e. "exposed" at
    // step -(exposed_time + 1)
    const uint32_t te = seed_te(c);
    std::vector<uint32_t> hist(TE_SLOTS, 0), off(TE_SLOTS + 1, 0);
    hist[te] = n_seeds;
    for (uint32_t k = te + 1; k <= TE_SLOTS; ++k) off[k] = n_seeds;
    HIP_TRY(c, hipMemcpy(d.hist, hist.data(), sizeof(uint32_t) * TE_SLOTS, hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(d.log_off, off.data(), sizeof(uint32_t) * (TE_SLOTS + 1), hipMemcpyHostToDevice));
    if (n_seeds) HIP_TRY(c, hipMemcpy(d.log, c->init_log.data(), sizeof(uint32_t) * n_seeds, hipMemcpyHostToDevice));
    rewind_host(c);
    return ESIM_OK;
}

namespace {

// What esim_restart and esim_restart_seeded refuse alike.
int restart_check(esim_ctx_impl *c, const esim_params *p, const std::string &who)
{
    if (!c->uploaded) return fail(c, ESIM_ESTATE, who + ": no population uploaded");
    if (c->comm.world > 1) return fail(c, ESIM_ESTATE, who + ": the context has a communicator of several ranks (the shards would have to agree on the parameters)");
    if (int rc = check_params(c, p, who)) return rc;
    if (p->device != c->P.device) return fail(c, ESIM_EINVAL, who + ": device must be the context's device");
    if (p->max_steps > c->cap_steps) return fail(c, ESIM_ERANGE, who + ": max_steps above the max_steps the context was created with (the record log's capacity)");
    return ESIM_OK;
}

// esim_reset with new parameters and without the host: nothing here waits for the stream or copies anything proportional to
// the population.  Host -> device go the control block and the threshold LUT (4.4 KB, from pinned memory) and, when the seeds
// are replaced, the distinct ones among them (4 B each, from pinned memory); the citizen words, the seeds' words, the census
// histogram and the log offsets are written by kernels, the rest is cleared or copied on the device.
// seeds != nullptr or replace: the distinct citizens of seeds[0 .. n_seeds), in the order of their first occurrence, become the
// seeds in force; every index has been checked by the caller.
int restart_enqueue(esim_ctx_impl *c, const esim_params *p, bool replace, const uint32_t *seeds, uint32_t n_seeds)
{
    HIP_TRY(c, hipSetDevice(c->P.device));
    // the staging blocks are the source of the previous restart's copies: they are long done unless restarts follow each
    // other with nothing in between (then this waits for those copies, not for the stream)
    if (c->rs.ev_used) HIP_TRY(c, hipEventSynchronize(c->rs.ev));
    if (replace) {
        // whatever can fail comes before the first change of the context: room for the list in pinned memory and on the device
        // (a longer device list takes the place of the old one: hipFree waits for the work that still reads that one)
        if (int rc = pinned_grow(c, &c->rs.seeds_stage, &c->rs.seeds_stage_n, n_seeds)) return rc;
        if (n_seeds > c->rs.seeds_cap) {
            uint32_t *grown = nullptr;
            if (int rc = dev_alloc(c, &grown, n_seeds)) return rc;
            dev_free(c, c->rs.seeds_dev);
            c->rs.seeds_dev = grown; c->rs.seeds_cap = n_seeds;
        }
    }
    c->P = *p;
    params_to_dev(c);
    const Dev &d = c->d;
    const uint32_t te = seed_te(c);
    if (replace) {
        // the old seeds' words back to Susceptible, the new ones set: O(old + new); a word that is set already is a duplicate
        // (esim_upload_population tells them the same way)
        for (uint32_t sc : c->init_log) c->init_state[sc] = CW_MAKE(TE_SUSCEPTIBLE, c->init_state[sc] & CW_FLAGS);
        c->init_log.clear();
        for (uint32_t i = 0; i < n_seeds; ++i) {
            const uint32_t sc = seeds[i];
            if (CW_TE(c->init_state[sc]) != te) { c->init_state[sc] = CW_MAKE(te, c->init_state[sc] & CW_FLAGS); c->init_log.push_back(sc); }
        }
        c->pop_hash = hash_with_seeds(c->pop_hash_head, seeds, n_seeds);
        c->snap.step = 0;                                          // (a snapshot belongs to the seeds it grew from: dropped, its buffers kept)
        if (!c->init_log.empty()) std::memcpy(c->rs.seeds_stage, c->init_log.data(), sizeof(uint32_t) * c->init_log.size());
    } else
        for (uint32_t sc : c->init_log) c->init_state[sc] = CW_MAKE(te, c->init_state[sc] & CW_FLAGS);   // (esim_reset's copy of the seeds' words)
    const uint32_t n_seeds_now = (uint32_t)c->init_log.size();
    Ctrl &h = c->rs.stage->h;
    initial_ctrl(c, &h);
    esim_threshold_lut(&c->P, c->rs.stage->lut);
    HIP_TRY(c, hipMemcpyAsync(d.ctrl, &h, sizeof h, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(const_cast<uint64_t *>(d.thr), c->rs.stage->lut, sizeof c->rs.stage->lut, hipMemcpyHostToDevice, c->stream));
    if (replace && n_seeds_now) HIP_TRY(c, hipMemcpyAsync(c->rs.seeds_dev, c->rs.seeds_stage, sizeof(uint32_t) * n_seeds_now, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipEventRecord(c->rs.ev, c->stream));
    c->rs.ev_used = true;
    if (d.n) hipLaunchKernelGGL(k_restart_words, dim3(grid_capped(c, ((size_t)d.n + 3u) / 4u, TPB, 2048)), dim3(TPB), 0, c->stream, d.cit, d.n);
    HIP_TRY(c, hipMemsetAsync(c->cnt_base, 0, c->cnt_bytes, c->stream));
    HIP_TRY(c, hipMemsetAsync(d.exp_step, 0, sizeof(uint32_t) * 2 * ((size_t)c->cap_steps + 2), c->stream));
    HIP_TRY(c, hipMemsetAsync(d.records, 0, sizeof(esim_step_result) * ((size_t)c->cap_steps + 1), c->stream));
    hipLaunchKernelGGL(k_restart_books, dim3(grid_for(std::max<size_t>(TE_SLOTS + 1u, n_seeds_now), TPB, 0xFFFFFFFFu)), dim3(TPB), 0, c->stream,
                       d.cit, d.n, c->rs.seeds_dev, n_seeds_now, te, d.hist, d.log_off);
    if (n_seeds_now) HIP_TRY(c, hipMemcpyAsync(d.log, c->rs.seeds_dev, sizeof(uint32_t) * n_seeds_now, hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(c, hipGetLastError());
    rewind_host(c);
    return ESIM_OK;
}

}  // namespace

extern "C" int esim_restart(esim_ctx *ctx, const esim_params *p)
{
    esim_ctx_impl *c = CTX(ctx);
    if (!c || !p) return fail(c, ESIM_EINVAL, "esim_restart: null argument");
    if (int rc = restart_check(c, p, "esim_restart")) return rc;
    return restart_enqueue(c, p, false, nullptr, 0);
}

extern "C" int esim_restart_seeded(esim_ctx *ctx, const esim_params *p, const uint32_t *seeds, uint32_t n_seeds)
{
    esim_ctx_impl *c = CTX(ctx);
    if (!c || !p) return fail(c, ESIM_EINVAL, "esim_restart_seeded: null argument");
    if (int rc = restart_check(c, p, "esim_restart_seeded")) return rc;
    if (n_seeds && !seeds) return fail(c, ESIM_EINVAL, "esim_restart_seeded: seeds is NULL");
    if (n_seeds > c->d.n) return fail(c, ESIM_ERANGE, "esim_restart_seeded: more seeds than citizens");
    for (uint32_t i = 0; i < n_seeds; ++i)
        if (seeds[i] >= c->d.n) return fail(c, ESIM_EINVAL, "esim_restart_seeded: seed index out of range");
    return restart_enqueue(c, p, true, seeds, n_seeds);
}

extern "C" int esim_get_seeds(esim_ctx *ctx, uint32_t *out, uint32_t cap, uint32_t *n_out)
{
    esim_ctx_impl *c = CTX(ctx);
    if (!c || !n_out) return fail(c, ESIM_EINVAL, "esim_get_seeds: null argument");
    if (!c->uploaded) return fail(c, ESIM_ESTATE, "esim_get_seeds: no population uploaded");
    const uint32_t n = (uint32_t)c->init_log.size();
    *n_out = n;
    if (n > cap || (n && !out)) return fail(c, ESIM_ERANGE, "esim_get_seeds: buffer too small (n_out holds the size needed)");
    if (n) std::memcpy(out, c->init_log.data(), sizeof(uint32_t) * n);
    return ESIM_OK;
}
