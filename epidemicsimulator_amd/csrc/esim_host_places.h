// esim_host_places.h -- work place and school outbreaks: esim_place_outbreaks, esim_place_sizes (on top of settings_enqueue /
// settings_finish) and esim_place_sar (on top of sar_begin / sar_finish of esim_host_household.h); the kernels: esim_kernels_household.h,
// esim_kernels_places.h; DESIGN 24.
// All three work in temporary device memory that lives as long as the call, and leave the context as it is.
namespace {

struct PlaceWork {
    DevTmp<uint32_t> tab;             // members, cases, introductions, first_step of the rooms or work places, of the schools
                                      // where they are asked for, then the two tables of PLACE_CELLS
    Place list, out;                  // what k_list_members fills; what the call delivers (the schools, or `list` again)
};

bool place_kind_known(int kind) { return kind == ESIM_PLACE_WORK || kind == ESIM_PLACE_ROOM || kind == ESIM_PLACE_SCHOOL; }

// The per-place pass behind an enqueued replay of the settings (q) and, where asked for, the two tables.
int place_enqueue(esim_ctx_impl *c, const std::string &who, int kind, const Setting &q, PlaceWork *w, bool tables)
{
    const Dev &d = c->d;
    const size_t n_list = kind == ESIM_PLACE_WORK ? d.n_bld : d.n_room, n_out = kind == ESIM_PLACE_ROOM ? d.n_room : d.n_bld;
    const size_t rows = 4 * n_list + (kind == ESIM_PLACE_SCHOOL ? 4 * n_out : 0), words = rows + 2 * (size_t)PLACE_CELLS;
    if (w->tab.alloc(words) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipStreamSynchronize(c->stream);                         // (the settings' kernels still read the host vectors of their work)
        return fail(c, ESIM_ENOMEM, who + ": no device memory for the places (16 B per building or room and 8 KB for the two tables)");
    }
    auto rows_at = [&](uint32_t *p, size_t n) { Place h; h.n_places = (uint32_t)n; h.members = p; h.cases = p + n; h.intro = p + 2 * n; h.first = p + 3 * n; h.final_size = h.intro_size = nullptr; return h; };
    w->list = rows_at(w->tab.p, n_list);
    w->out = kind == ESIM_PLACE_SCHOOL ? rows_at(w->tab.p + 4 * n_list, n_out) : w->list;
    w->out.final_size = w->tab.p + rows; w->out.intro_size = w->out.final_size + PLACE_CELLS;
    hipError_t e = hipMemsetAsync(w->tab.p, 0, sizeof(uint32_t) * std::max<size_t>(1, words), c->stream);
    if (e == hipSuccess && n_list) e = hipMemsetAsync(w->list.first, 0xFF, sizeof(uint32_t) * n_list, c->stream);   // (a population without a room has no row)
    if (e == hipSuccess && kind == ESIM_PLACE_SCHOOL && n_out) e = hipMemsetAsync(w->out.first, 0xFF, sizeof(uint32_t) * n_out, c->stream);
    if (e != hipSuccess) { (void)hipStreamSynchronize(c->stream); return fail(c, ESIM_ENODEVICE, who + ": " + hipGetErrorString(e)); }
    if (kind == ESIM_PLACE_WORK) hipLaunchKernelGGL(k_list_members<LIST_WORK>, dim3(grid_capped(c, d.n_wrk_idx, TPB, 4096)), dim3(TPB), 0, c->stream, d, q, w->list);
    else hipLaunchKernelGGL(k_list_members<LIST_ROOM>, dim3(grid_capped(c, d.n_room_idx, TPB, 4096)), dim3(TPB), 0, c->stream, d, q, w->list);
    if (kind == ESIM_PLACE_SCHOOL) hipLaunchKernelGGL(k_place_schools, dim3(grid_capped(c, d.n_room, TPB, 4096)), dim3(TPB), 0, c->stream, d, w->list, w->out);
    // (a workgroup of k_list_tables bins 32 places per lane at least before it hands over its table of 2048 counters at most)
    if (tables) hipLaunchKernelGGL(k_list_tables<false>, dim3(grid_capped(c, n_out, TPB * 32u, 1024, TPB)), dim3(TPB), 0, c->stream, d, w->out);
    return ESIM_OK;
}

}  // namespace

extern "C" int esim_place_outbreaks(esim_ctx *ctx, int kind, uint32_t *members, uint32_t *cases, uint32_t *introductions, uint32_t *first_step)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    const std::string who = "esim_place_outbreaks";
    if (!place_kind_known(kind)) return fail(c, ESIM_EINVAL, who + ": a `kind` that is none of ESIM_PLACE_WORK, ESIM_PLACE_ROOM, ESIM_PLACE_SCHOOL");
    if (int rc = settings_check(c, who)) return rc;
    HIP_TRY(c, hipSetDevice(c->P.device));
    SettingWork s;
    PlaceWork w;
    if (int rc = settings_enqueue(c, who, &s)) return rc;
    if (int rc = place_enqueue(c, who, kind, s.q, &w, false)) return rc;
    const int rc = settings_finish(c, who, &s);
    if (rc && rc != ESIM_ESIM) return rc;
    const size_t bytes = sizeof(uint32_t) * (size_t)w.out.n_places;
    if (members && bytes) HIP_TRY(c, hipMemcpy(members, w.out.members, bytes, hipMemcpyDeviceToHost));
    if (cases && bytes) HIP_TRY(c, hipMemcpy(cases, w.out.cases, bytes, hipMemcpyDeviceToHost));
    if (introductions && bytes) HIP_TRY(c, hipMemcpy(introductions, w.out.intro, bytes, hipMemcpyDeviceToHost));
    if (first_step && bytes) HIP_TRY(c, hipMemcpy(first_step, w.out.first, bytes, hipMemcpyDeviceToHost));
    return rc;
}

extern "C" int esim_place_sizes(esim_ctx *ctx, int kind, uint32_t *final_size, uint32_t *introduced)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    const std::string who = "esim_place_sizes";
    if (!place_kind_known(kind)) return fail(c, ESIM_EINVAL, who + ": a `kind` that is none of ESIM_PLACE_WORK, ESIM_PLACE_ROOM, ESIM_PLACE_SCHOOL");
    if (int rc = settings_check(c, who)) return rc;
    HIP_TRY(c, hipSetDevice(c->P.device));
    SettingWork s;
    PlaceWork w;
    if (int rc = settings_enqueue(c, who, &s)) return rc;
    if (int rc = place_enqueue(c, who, kind, s.q, &w, true)) return rc;
    const int rc = settings_finish(c, who, &s);
    if (rc && rc != ESIM_ESIM) return rc;
    if (final_size) HIP_TRY(c, hipMemcpy(final_size, w.out.final_size, sizeof(uint32_t) * PLACE_CELLS, hipMemcpyDeviceToHost));
    if (introduced) HIP_TRY(c, hipMemcpy(introduced, w.out.intro_size, sizeof(uint32_t) * PLACE_CELLS, hipMemcpyDeviceToHost));
    return rc;
}

extern "C" int esim_place_sar(esim_ctx *ctx, int kind, int where, uint32_t first_step, uint32_t last_step, uint64_t *at_risk, uint64_t *secondary)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    const std::string who = "esim_place_sar";
    if ((!at_risk && !secondary) || (where != ESIM_BY_ALL && where != ESIM_BY_GROUP) || (kind != ESIM_PLACE_WORK && kind != ESIM_PLACE_ROOM))
        return fail(c, ESIM_EINVAL, who + ": no output, a `where` that is neither ESIM_BY_ALL nor ESIM_BY_GROUP, or a `kind` that is neither ESIM_PLACE_WORK nor ESIM_PLACE_ROOM "
                                          "(the infector of a school exposure is somebody of the room)");
    SarWork k;
    PlaceWork pw;
    if (int rc = sar_begin(c, who, where, first_step, last_step, &k)) return rc;
    if (int rc = place_enqueue(c, who, kind, k.w.s.q, &pw, false)) return rc;
    const bool rooms = kind == ESIM_PLACE_ROOM;
    // a workgroup scans TPB places at a time; the grid stays wide, the long places lie where they lie
    const dim3 grid(grid_capped(c, pw.list.n_places, TPB, 16384));
#define PLACE_SAR_LAUNCH(MODE, ROOMS, LDS) hipLaunchKernelGGL((k_place_sar<MODE, ROOMS>), grid, dim3(TPB), LDS, c->stream, c->d, k.w.s.q, k.w.t, pw.list, k.s)
    if (k.mode == PAIRTAB_ONE_CELL) { if (rooms) PLACE_SAR_LAUNCH(PAIRTAB_ONE_CELL, true, 0); else PLACE_SAR_LAUNCH(PAIRTAB_ONE_CELL, false, 0); }
    else if (k.mode == PAIRTAB_LDS) { if (rooms) PLACE_SAR_LAUNCH(PAIRTAB_LDS, true, k.lds); else PLACE_SAR_LAUNCH(PAIRTAB_LDS, false, k.lds); }
    else { if (rooms) PLACE_SAR_LAUNCH(PAIRTAB_GLOBAL, true, 0); else PLACE_SAR_LAUNCH(PAIRTAB_GLOBAL, false, 0); }
#undef PLACE_SAR_LAUNCH
    return sar_finish(c, who, &k, at_risk, secondary);
}
