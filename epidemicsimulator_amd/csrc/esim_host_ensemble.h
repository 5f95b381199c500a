// esim_host_ensemble.h -- the state of the ensemble accumulators: the table of the kinds, the one begin (ens_begin) and
// the one read-out (ens_read) behind the entry points of every kind, and what esim_ensemble_fold runs per kind.  No kernel is
// launched here: a kind's own checks, its fold and the fold's launches are in the file of its family.
namespace {

typedef Ensemble::Rows Rows;

// The buffers of Rows a kind may own, one bit each; all but the last three hold [n_rows][n_cols] cells.
enum : uint32_t {
    B_HIT = 1u << 0, B_DEFINED = 1u << 1, B_P0 = 1u << 2, B_P1 = 1u << 3, B_SUM = 1u << 4, B_SUMSQ = 1u << 5, B_SUM_O = 1u << 6, B_SUMSQ_O = 1u << 7,
    B_CROSS = 1u << 8, B_SUM_D = 1u << 9, B_SUMSQ_D = 1u << 10,
    B_OCC = 1u << 11,                             // [2][n_cols]
    B_AW = 1u << 12, B_PIN_AW = 1u << 13,         // [cap_steps + 1] on the device, and the pinned Pinned::aw they are copied from
    B_MOMENTS = B_HIT | B_SUM | B_SUMSQ,
    B_RATIO = B_MOMENTS | B_DEFINED | B_SUM_O | B_SUMSQ_O | B_CROSS | B_P0 | B_P1,
    B_PEAKS = B_MOMENTS | B_DEFINED | B_SUM_O | B_SUMSQ_O | B_SUM_D | B_SUMSQ_D,
};
struct RowsWords { uint32_t bit; uint32_t *Rows::*p; bool acc; };             // acc: a begin zeroes it (the planes are zeroed by the fold)
struct RowsWide { uint32_t bit; unsigned long long *Rows::*p; };
constexpr RowsWords ENS_WORDS[] = { { B_HIT, &Rows::hit, true }, { B_DEFINED, &Rows::defined, true }, { B_P0, &Rows::p0, false }, { B_P1, &Rows::p1, false } };
constexpr RowsWide ENS_WIDE[] = { { B_SUM, &Rows::sum }, { B_SUMSQ, &Rows::sumsq }, { B_SUM_O, &Rows::sum_o }, { B_SUMSQ_O, &Rows::sumsq_o }, { B_CROSS, &Rows::cross },
                                   { B_SUM_D, &Rows::sum_d }, { B_SUMSQ_D, &Rows::sumsq_d } };

// The five read-outs: the entry point's name, how its refusal names the begin it serves, and the text of a begin that finds no
// memory for a kind it reads (nullptr: the allocation's own).
enum { READ_CELLS = 0, READ_SERIES, READ_REPRODUCTION, READ_PAIRED, READ_PEAKS, ENS_READERS };
struct ReaderInfo { const char *name, *begun, *no_memory; };
constexpr const char *NO_MEMORY_ROWS = ": no device memory for the accumulators and the row planes (ask for fewer rows)";
constexpr ReaderInfo ENS_READER[ENS_READERS] = {
    { "esim_ensemble_read", "esim_ensemble_begin since the upload", nullptr },
    { "esim_ensemble_read_series", "esim_ensemble_begin_series or esim_ensemble_begin_settings in force since the upload", NO_MEMORY_ROWS },
    { "esim_ensemble_read_reproduction", "begin of this kind in force since the upload", NO_MEMORY_ROWS },
    { "esim_ensemble_read_paired", "begin of this kind in force since the upload", NO_MEMORY_ROWS },
    { "esim_ensemble_read_peaks", "esim_ensemble_begin_peaks in force since the upload", ": no device memory for the accumulators (56 B per column)" },
};

// What is kept of a member (esim_ensemble_keep_members): nothing, the value per cell, the value with ESIM_NEVER among them, the
// signed difference of the two planes, or what the call's `what` picks of the member's summary (the peak's step has ESIM_NEVER).
enum { KEEP_NONE = 0, KEEP_PLAIN, KEEP_NEVER, KEEP_SIGNED, KEEP_SUMMARY };

// The table of the kinds, by Ensemble::Kind.  owns: the series kind owns p1 as well where its begin says `two`.  begin: as the
// refusal of esim_ensemble_read_series names it -- a burden kind by the kind whose accumulators and reader it shares.
struct KindInfo { uint32_t owns; int reader, keep; const char *begin; };
constexpr KindInfo ENS_KIND[Ensemble::ENS_KINDS] = {
    /* ENS_NONE          */ { 0u, -1, KEEP_NONE, "" },
    /* ENS_CENSUS        */ { B_MOMENTS, READ_CELLS, KEEP_PLAIN, "esim_ensemble_begin" },
    /* ENS_ARRIVAL       */ { B_MOMENTS, READ_CELLS, KEEP_NEVER, "esim_ensemble_begin_arrival" },
    /* ENS_SERIES        */ { B_MOMENTS | B_P0 | B_OCC | B_AW | B_PIN_AW, READ_SERIES, KEEP_PLAIN, "esim_ensemble_begin_series" },
    /* ENS_SETTINGS      */ { B_MOMENTS | B_P0, READ_SERIES, KEEP_PLAIN, "esim_ensemble_begin_settings" },
    /* ENS_REPRODUCTION  */ { B_RATIO, READ_REPRODUCTION, KEEP_NONE, "esim_ensemble_begin_reproduction" },
    /* ENS_PAIRED        */ { B_RATIO, READ_PAIRED, KEEP_SIGNED, "esim_ensemble_begin_paired" },
    /* ENS_PEAKS         */ { B_PEAKS, READ_PEAKS, KEEP_SUMMARY, "esim_ensemble_begin_peaks" },
    /* ENS_BURDEN_PEAKS  */ { B_PEAKS, READ_PEAKS, KEEP_SUMMARY, "esim_ensemble_begin_peaks" },
    /* ENS_BURDEN_SERIES */ { B_MOMENTS | B_P0, READ_SERIES, KEEP_PLAIN, "esim_ensemble_begin_settings" },
    /* ENS_BURDEN_PAIRED */ { B_RATIO, READ_PAIRED, KEEP_SIGNED, "esim_ensemble_begin_paired" },
};

uint32_t ens_owned(const Ensemble &e) { const Rows &r = e.rows; return ENS_KIND[e.kind].owns | (r.two ? B_P1 : 0u); }

void members_end(esim_ctx_impl *c);        // (esim_host_members.h)
int members_full(esim_ctx_impl *c);

// The buffers of a Rows back to the device (nothing may still be using them).
void rows_free(esim_ctx_impl *c, Rows *r)
{
    for (const RowsWords &w : ENS_WORDS) dev_free(c, r->*w.p);
    for (const RowsWide &w : ENS_WIDE) dev_free(c, r->*w.p);
    for (void *q : { (void *)r->members, (void *)r->occ, (void *)r->vax, (void *)r->aw }) dev_free(c, q);
    *r = Rows();
}

// The begin of every kind behind its entry point's own checks.  The buffers the table names are kept where the kind in force
// owns the same ones in the same shape; otherwise they are allocated before the earlier ones go, so that a refusal leaves
// everything as it was.  The accumulators are zeroed on the stream, and every field of the state is assigned: kind, where, n,
// valid, and the parameters as a whole.  Keeping members ends.
int ens_begin(esim_ctx_impl *c, const std::string &who, Ensemble::Kind kind, int where, uint32_t n_rows, uint32_t cols, const Ensemble::Par &par, bool two = false)
{
    Ensemble &e = c->ens;
    const KindInfo &k = ENS_KIND[kind];
    const uint32_t owns = k.owns | (two ? B_P1 : 0u);
    const size_t cells = (size_t)n_rows * cols;
    if (ens_owned(e) != owns || e.rows.n_rows != n_rows || e.rows.n_cols != cols) {
        Rows r;
        if ((owns & B_PIN_AW) && !c->pin.aw) HIP_TRY(c, hipHostMalloc((void **)&c->pin.aw, (size_t)c->cap_steps + 1u, hipHostMallocDefault));
        int rc = dev_alloc(c, &r.members, 1);
        for (const RowsWords &w : ENS_WORDS) if (!rc && (owns & w.bit)) rc = dev_alloc(c, &(r.*w.p), cells);
        for (const RowsWide &w : ENS_WIDE) if (!rc && (owns & w.bit)) rc = dev_alloc(c, &(r.*w.p), cells);
        if (!rc && (owns & B_OCC)) rc = dev_alloc(c, &r.occ, (size_t)cols * 2u);
        if (!rc && (owns & B_AW)) rc = dev_alloc(c, &r.aw, (size_t)c->cap_steps + 1u);
        if (rc) {
            (void)hipGetLastError();
            rows_free(c, &r);
            const char *text = ENS_READER[k.reader].no_memory;
            return text ? fail(c, ESIM_ENOMEM, who + text) : rc;
        }
        if (e.kind != Ensemble::ENS_NONE) HIP_TRY(c, hipStreamSynchronize(c->stream));   // (a fold on the stream may still be using the old ones)
        r.vax = e.rows.vax; e.rows.vax = nullptr;                    // (the series kind's 4 B per citizen, whatever the shape)
        rows_free(c, &e.rows);
        r.n_rows = n_rows; r.n_cols = cols; r.two = two;
        e.rows = r;
    }
    Rows &r = e.rows;
    const size_t room = std::max<size_t>(1, cells);
    HIP_TRY(c, hipMemsetAsync(r.members, 0, sizeof(uint32_t), c->stream));
    for (const RowsWords &w : ENS_WORDS) if (w.acc && (owns & w.bit)) HIP_TRY(c, hipMemsetAsync(r.*w.p, 0, sizeof(uint32_t) * room, c->stream));
    for (const RowsWide &w : ENS_WIDE) if (owns & w.bit) HIP_TRY(c, hipMemsetAsync(r.*w.p, 0, sizeof(unsigned long long) * room, c->stream));
    e.kind = kind; e.where = where; e.n = cols; e.valid = true; e.par = par;
    members_end(c);
    return ESIM_OK;
}

// The read-out behind the five esim_ensemble_read* entry points: refused unless a kind of this reader is in force, then rows
// [first_row, first_row + n) of the buffers named, any output NULL, behind the one wait for whatever is on the stream.
struct ReadWords { uint32_t *out; uint32_t *Rows::*from; };
struct ReadWide { uint64_t *out; unsigned long long *Rows::*from; };
int ens_read(esim_ctx_impl *c, int reader, uint32_t first_row, uint32_t n, uint32_t *members, std::initializer_list<ReadWords> words, std::initializer_list<ReadWide> sums)
{
    const Ensemble &e = c->ens;
    const KindInfo &k = ENS_KIND[e.kind];
    const std::string who = ENS_READER[reader].name;
    const bool live = c->uploaded && e.valid && e.kind != Ensemble::ENS_NONE;
    if (live && k.reader != reader && reader == READ_CELLS)
        return fail(c, ESIM_ESTATE, who + ": the accumulators in force were begun over rows (read them with esim_ensemble_read_series, or with esim_ensemble_read_reproduction those of esim_ensemble_begin_reproduction)");
    if (live && k.reader != reader && reader == READ_SERIES && k.reader != READ_CELLS)
        return fail(c, ESIM_ESTATE, who + ": the accumulators in force were begun by " + k.begin + " (read them with " + ENS_READER[k.reader].name + ")");
    if (!live || k.reader != reader)
        return fail(c, ESIM_ESTATE, who + ": no population uploaded, or no " + ENS_READER[reader].begun + " (or, by group, since esim_set_groups)");
    const Rows &r = e.rows;
    if ((uint64_t)first_row + n > r.n_rows) return fail(c, ESIM_ERANGE, who + ": rows outside the accumulators");
    HIP_TRY(c, hipSetDevice(c->P.device));
    Ctrl h; int rc;
    if ((rc = read_ctrl(c, &h))) return rc;                        // (the wait for the folds enqueued so far)
    const size_t at = (size_t)first_row * r.n_cols, cells = (size_t)n * r.n_cols;
    if (members) HIP_TRY(c, hipMemcpy(members, r.members, sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (const ReadWords &w : words)
        if (w.out && cells) HIP_TRY(c, hipMemcpy(w.out, r.*w.from + at, sizeof(uint32_t) * cells, hipMemcpyDeviceToHost));
    for (const ReadWide &s : sums)
        if (s.out && cells) HIP_TRY(c, hipMemcpy(s.out, r.*s.from + at, sizeof(uint64_t) * cells, hipMemcpyDeviceToHost));
    return ctrl_error(c, h);
}

// The two counters and five sums of the kinds with two planes, as their fold kernels take them.
RatioAcc ratio_acc(const Rows &r)
{
    RatioAcc a;
    a.defined = r.defined; a.hit = r.hit; a.members = r.members; a.sum_c = r.sum; a.sum_o = r.sum_o; a.sq_c = r.sumsq; a.sq_o = r.sumsq_o; a.cross = r.cross;
    return a;
}

// One member folded into the accumulators of a kind, each in the file of its family.
int fold_census(esim_ctx_impl *c);         // (esim_host_outputs.h)
int fold_arrival(esim_ctx_impl *c);
int fold_series(esim_ctx_impl *c);
int fold_transmission(esim_ctx_impl *c);   // (esim_host_ensrows.h: the settings and the reproduction kind)
int fold_paired(esim_ctx_impl *c);         // (esim_host_compare.h)
int fold_peaks(esim_ctx_impl *c);          // (esim_host_curves.h)
int fold_burden_peaks(esim_ctx_impl *c);   // (esim_host_burden.h)
int fold_beds(esim_ctx_impl *c);           // (esim_host_beds.h: the burden-series and the burden-paired kind)

}  // namespace

extern "C" int esim_ensemble_fold(esim_ctx *ctx)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    if (!c->uploaded || !c->ens.valid || c->ens.kind == Ensemble::ENS_NONE)
        return fail(c, ESIM_ESTATE, "esim_ensemble_fold: no population uploaded, or no esim_ensemble_begin since the upload (or, by group, since esim_set_groups)");
    if (int rc = members_full(c)) return rc;
    switch (c->ens.kind) {
    case Ensemble::ENS_CENSUS: return fold_census(c);
    case Ensemble::ENS_ARRIVAL: return fold_arrival(c);
    case Ensemble::ENS_SERIES: return fold_series(c);
    case Ensemble::ENS_SETTINGS: case Ensemble::ENS_REPRODUCTION: return fold_transmission(c);
    case Ensemble::ENS_PAIRED: return fold_paired(c);
    case Ensemble::ENS_PEAKS: return fold_peaks(c);
    case Ensemble::ENS_BURDEN_PEAKS: return fold_burden_peaks(c);
    case Ensemble::ENS_BURDEN_SERIES: case Ensemble::ENS_BURDEN_PAIRED: return fold_beds(c);
    case Ensemble::ENS_NONE: case Ensemble::ENS_KINDS: break;
    }
    return ESIM_ESTATE;
}
