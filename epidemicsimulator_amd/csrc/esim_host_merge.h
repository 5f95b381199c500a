// esim_host_merge.h -- ensembles on several contexts: esim_ensemble_merge adds the accumulators of another context's
// kind in force into this one's and appends its kept members; esim_ensemble_save / _save_size / _load are the same through a
// byte buffer.  Every accumulator is an integer count or sum, so an ensemble split over contexts and merged is bit for bit the
// ensemble folded in sequence.  The descriptor and the blob's layout: esim_merge.h; the kernel: esim_kernels_merge.h.  Both
// entry points bring the other side's accumulators to this context's device piece by piece, into one staging buffer of bounded
// size -- hipMemcpyPeerAsync from a context (a device-to-device copy on one device), a host-to-device copy from a blob -- and
// launch k_ensemble_merge per piece on this context's stream.  The kept planes are copied straight into their slots.
#include "esim_merge.h"

namespace {

static_assert(MERGE_KINDS == (uint32_t)Ensemble::ENS_KINDS, "esim_merge.h counts the kinds of Ensemble::Kind");
static_assert(MERGE_KEPT_MAX == (uint32_t)ESIM_MEMBERS_MAX && MERGE_GROUPS_MAX == (uint32_t)ESIM_MAX_GROUPS, "esim_merge.h repeats two limits of esim.h");
static_assert(sizeof ENS_WIDE / sizeof *ENS_WIDE == MERGE_WIDE, "MergeArgs holds a slot for every u64 sum of the table");

// The accumulators among the u32 buffers of the table, in its order (the planes are a member's temporaries).
constexpr uint32_t merge_words_owned(uint32_t owns) { uint32_t n = 0u; for (const RowsWords &w : ENS_WORDS) if (w.acc && (owns & w.bit)) ++n; return n; }
constexpr uint32_t merge_wide_owned(uint32_t owns) { uint32_t n = 0u; for (const RowsWide &w : ENS_WIDE) if (owns & w.bit) ++n; return n; }
constexpr bool merge_table_agrees()
{
    for (uint32_t k = 0u; k < MERGE_KINDS; ++k)
        if (merge_kind_bufs(k).words != merge_words_owned(ENS_KIND[k].owns) || merge_kind_bufs(k).wide != merge_wide_owned(ENS_KIND[k].owns)) return false;
    return true;
}
static_assert(merge_table_agrees(), "esim_merge.h counts the accumulators of every kind as the table of esim_host_ensemble.h owns them");

bool merge_burden_kind(Ensemble::Kind k) { return k == Ensemble::ENS_BURDEN_PEAKS || k == Ensemble::ENS_BURDEN_SERIES || k == Ensemble::ENS_BURDEN_PAIRED; }

// The descriptor of the begin in force.
MergeDesc merge_desc_of(const esim_ctx_impl *c)
{
    const Ensemble &e = c->ens;
    const Ensemble::Par &p = e.par;
    MergeDesc d;
    uint32_t *f = d.f;
    f[MF_KIND] = (uint32_t)e.kind; f[MF_WHERE] = (uint32_t)e.where; f[MF_N_ROWS] = e.rows.n_rows; f[MF_N_COLS] = e.rows.n_cols; f[MF_TWO] = e.rows.two ? 1u : 0u;
    f[MF_STATUS_MASK] = p.status_mask; f[MF_SETTING_MASK] = p.setting_mask; f[MF_HORIZON] = p.horizon; f[MF_STATUS] = (uint32_t)p.status; f[MF_BURDEN_WHAT] = (uint32_t)p.burden_what;
    f[MF_FIRST] = p.first; f[MF_STRIDE] = p.stride; f[MF_LAST] = p.last; f[MF_THRESHOLD] = p.threshold; f[MF_MIN_HIT] = p.min_hit; f[MF_MIN_DEFINED] = p.min_defined;
    f[MF_R_NUM] = p.r_num; f[MF_R_DEN] = p.r_den; f[MF_MIN_AVERTED] = p.min_averted; f[MF_CUMULATIVE] = p.cumulative ? 1u : 0u;
    f[MF_POP_HASH_LO] = (uint32_t)c->pop_hash_head; f[MF_POP_HASH_HI] = (uint32_t)(c->pop_hash_head >> 32); f[MF_N_CITIZENS] = c->d.n;
    const Ensemble::Store &s = e.store;
    if (s.planes) { f[MF_STORE] = 1u; f[MF_STORE_WHAT] = (uint32_t)s.what; f[MF_STORE_SIGNED] = s.is_signed ? 1u : 0u; f[MF_STORE_NEVER] = s.has_never ? 1u : 0u; }
    if (e.where == ESIM_BY_GROUP) d.groups = c->grp.sizes;
    if (merge_burden_kind(e.kind) && c->burden.set) {
        const BurdenState &b = c->burden;
        d.burden = { b.n_groups, b.n_delay, b.n_stay, b.delay_unit, b.stay_unit };
        d.burden.insert(d.burden.end(), b.host.begin(), b.host.end());
    }
    f[MF_N_GROUPS] = (uint32_t)d.groups.size(); f[MF_N_BURDEN] = (uint32_t)d.burden.size();
    return d;
}

// What both sides of a merge, a save and a load must be: uploaded, a begin in force, one rank, no shard.  err: the context the
// refusal's text goes to (a merge reports about src on dst).
int merge_ready(esim_ctx_impl *err, const esim_ctx_impl *c, const std::string &who, const char *side)
{
    if (!c->uploaded) return fail(err, ESIM_ESTATE, who + ": no population uploaded" + side);
    if (!c->ens.valid || c->ens.kind == Ensemble::ENS_NONE)
        return fail(err, ESIM_ESTATE, who + ": no begin in force since the upload (or, by group, since esim_set_groups)" + side);
    if (c->comm.world > 1 || c->d.n_global != c->d.n)
        return fail(err, ESIM_ESTATE, who + ": the context has a communicator of several ranks or holds a shard (the rule of esim_restart)" + side);
    return ESIM_OK;
}

// Where the other ensemble comes from: a context (src) or the bytes of a blob behind its header (acc, then planes).
struct MergeFrom {
    const esim_ctx_impl *src;
    const uint8_t *acc, *planes, *members;       // a blob: the accumulators, the kept planes, the u32 member counter
};

// bytes from the other side to `to` on c's device, on c's stream.
hipError_t merge_fetch(esim_ctx_impl *c, const MergeFrom &from, void *to, const void *dev_src, const uint8_t *host_src, size_t bytes)
{
    if (!bytes) return hipSuccess;
    if (from.src) return hipMemcpyPeerAsync(to, c->P.device, dev_src, from.src->P.device, bytes, c->stream);
    return hipMemcpyAsync(to, host_src, bytes, hipMemcpyHostToDevice, c->stream);
}

// The other ensemble added into c's, everything enqueued on c's stream, nothing waited for.  The checks are the caller's:
// the descriptors agree and the store has room for kept_src more members.
int merge_apply(esim_ctx_impl *c, const MergeFrom &from, uint32_t kept_src, uint32_t folds_src)
{
    Ensemble &e = c->ens;
    Rows &r = e.rows;
    const uint32_t owns = ens_owned(e);
    const size_t cells = (size_t)r.n_rows * r.n_cols;
    const uint32_t n_words = merge_words_owned(owns), n_wide = merge_wide_owned(owns);
    const size_t knob = c->tune.merge_piece ? c->tune.merge_piece : MERGE_PIECE_CELLS;
    const size_t piece = std::min<size_t>(knob, (std::max<size_t>(cells, 1u) + 3u) / 4u * 4u);      // (a multiple of four cells: every 16 B access aligned)
    HIP_TRY(c, hipSetDevice(c->P.device));
    const size_t need = 16u + piece * (4u * n_words + 8u * n_wide);
    if (e.merge_stage_bytes < need) {
        uint8_t *p = nullptr;
        if (dev_alloc(c, &p, need)) { (void)hipGetLastError(); return fail(c, ESIM_ENOMEM, "esim_ensemble_merge / esim_ensemble_load: no device memory for the staging buffer"); }
        dev_free(c, e.merge_stage);                  // (hipFree waits for whatever still reads the smaller one)
        e.merge_stage = p; e.merge_stage_bytes = need;
    }
    // the staging buffer: the member counter in its first 16 B, then a region of `piece` cells per buffer the kind owns
    uint32_t *stage_members = (uint32_t *)e.merge_stage;
    size_t blob_at = 0u;                             // of the buffer in turn inside a blob's accumulators
    for (size_t at = 0u; at == 0u || at < cells; at += piece) {
        const size_t n = std::min(piece, cells - at);
        MergeArgs a;
        std::memset(&a, 0, sizeof a);
        a.n = n;
        uint8_t *stage = e.merge_stage + 16u;
        blob_at = 0u;
        uint32_t iw = 0u, id = 0u;
        for (const RowsWords &w : ENS_WORDS) {
            if (!w.acc || !(owns & w.bit)) { if (w.acc) ++iw; continue; }
            HIP_TRY(c, merge_fetch(c, from, stage, from.src ? from.src->ens.rows.*w.p + at : nullptr, from.src ? nullptr : from.acc + blob_at + 4u * at, 4u * n));
            a.src_w[iw] = (const uint32_t *)stage; a.dst_w[iw] = r.*w.p + at;
            stage += 4u * piece; blob_at += 4u * cells; ++iw;
        }
        for (const RowsWide &w : ENS_WIDE) {
            if (!(owns & w.bit)) { ++id; continue; }
            HIP_TRY(c, merge_fetch(c, from, stage, from.src ? from.src->ens.rows.*w.p + at : nullptr, from.src ? nullptr : from.acc + blob_at + 8u * at, 8u * n));
            a.src_d[id] = (const unsigned long long *)stage; a.dst_d[id] = r.*w.p + at;
            stage += 8u * piece; blob_at += 8u * cells; ++id;
        }
        if (at == 0u) {
            HIP_TRY(c, merge_fetch(c, from, stage_members, from.src ? from.src->ens.rows.members : nullptr, from.members, sizeof(uint32_t)));
            a.src_members = stage_members; a.dst_members = r.members;
        }
        hipLaunchKernelGGL(k_ensemble_merge, dim3(grid_capped(c, n, MERGE_TPB * MERGE_LANE_CELLS, MERGE_GRID)), dim3(MERGE_TPB), 0, c->stream, a);
        HIP_TRY(c, hipGetLastError());
    }
    Ensemble::Store &s = e.store;
    if (s.planes && kept_src) {
        HIP_TRY(c, merge_fetch(c, from, s.planes + (size_t)s.kept * cells, from.src ? from.src->ens.store.planes : nullptr, from.planes, sizeof(uint32_t) * cells * kept_src));
        s.kept += kept_src;
    }
    e.folds += folds_src;
    return ESIM_OK;
}

}  // namespace

extern "C" int esim_ensemble_merge(esim_ctx *dst_ctx, esim_ctx *src_ctx)
{
    esim_ctx_impl *c = CTX(dst_ctx), *s = CTX(src_ctx);
    const std::string who = "esim_ensemble_merge";
    if (!c || !s) return fail(c, ESIM_EINVAL, who + ": null context");
    if (c == s) return fail(c, ESIM_EINVAL, who + ": dst and src are the same context");
    if (int rc = merge_ready(c, c, who, " (dst)")) return rc;
    if (int rc = merge_ready(c, s, who, " (src)")) return rc;
    if (const char *field = merge_desc_diff(merge_desc_of(c), merge_desc_of(s)))
        return fail(c, ESIM_ESTATE, who + ": the two contexts do not describe the same ensemble: " + field + " differs");
    const Ensemble::Store &mine = c->ens.store, &theirs = s->ens.store;
    if (mine.planes && (uint64_t)mine.kept + theirs.kept > mine.capacity)
        return fail(c, ESIM_ERANGE, who + ": dst keeps " + std::to_string(mine.kept) + " members and src " + std::to_string(theirs.kept) + ", the store of dst takes " +
                                    std::to_string(mine.capacity) + "; nothing was merged");
    // (a src without a member folded goes the same way: its accumulators are zero, and a cell with nothing to add is not written)
    // everything src has enqueued is done before dst's stream reads its buffers; no event is shared between the contexts
    HIP_TRY(c, hipSetDevice(s->P.device));
    HIP_TRY(c, hipStreamSynchronize(s->stream));
    MergeFrom from = { s, nullptr, nullptr, nullptr };
    return merge_apply(c, from, theirs.planes ? theirs.kept : 0u, s->ens.folds);
}

extern "C" int esim_ensemble_save_size(esim_ctx *ctx, size_t *bytes)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    const std::string who = "esim_ensemble_save_size";
    if (!bytes) return fail(c, ESIM_EINVAL, who + ": null output");
    if (int rc = merge_ready(c, c, who, "")) return rc;
    *bytes = (size_t)merge_blob_bytes(merge_desc_of(c), c->ens.store.planes ? c->ens.store.kept : 0u);
    return ESIM_OK;
}

extern "C" int esim_ensemble_save(esim_ctx *ctx, void *buf, size_t cap)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    const std::string who = "esim_ensemble_save";
    if (!buf) return fail(c, ESIM_EINVAL, who + ": null buffer");
    if (int rc = merge_ready(c, c, who, "")) return rc;
    const Ensemble &e = c->ens;
    const MergeDesc d = merge_desc_of(c);
    const uint32_t kept = e.store.planes ? e.store.kept : 0u;
    if ((uint64_t)cap < merge_blob_bytes(d, kept)) return fail(c, ESIM_ERANGE, who + ": buffer smaller than esim_ensemble_save_size");
    HIP_TRY(c, hipSetDevice(c->P.device));
    Ctrl h; int rc;
    if ((rc = read_ctrl(c, &h))) return rc;          // (the wait for the folds and merges enqueued so far)
    MergeCounts n = { 0u, e.folds, kept };
    HIP_TRY(c, hipMemcpy(&n.members, e.rows.members, sizeof(uint32_t), hipMemcpyDeviceToHost));
    uint8_t *p = (uint8_t *)buf;
    merge_pack_header(d, n, p); p += merge_header_bytes(d);
    const uint32_t owns = ens_owned(e);
    const size_t cells = (size_t)e.rows.n_rows * e.rows.n_cols;
    auto pull = [&](const void *src, size_t bytes) -> int { if (bytes) HIP_TRY(c, hipMemcpy(p, src, bytes, hipMemcpyDeviceToHost)); p += bytes; return ESIM_OK; };
    for (const RowsWords &w : ENS_WORDS) if (w.acc && (owns & w.bit)) if ((rc = pull(e.rows.*w.p, sizeof(uint32_t) * cells))) return rc;
    for (const RowsWide &w : ENS_WIDE) if (owns & w.bit) if ((rc = pull(e.rows.*w.p, sizeof(uint64_t) * cells))) return rc;
    if (kept) if ((rc = pull(e.store.planes, sizeof(uint32_t) * cells * kept))) return rc;
    return ctrl_error(c, h);
}

extern "C" int esim_ensemble_load(esim_ctx *ctx, const void *buf, size_t bytes)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    const std::string who = "esim_ensemble_load";
    if (!buf) return fail(c, ESIM_EINVAL, who + ": null buffer");
    if (int rc = merge_ready(c, c, who, "")) return rc;
    const Ensemble &e = c->ens;
    const MergeDesc mine = merge_desc_of(c);
    MergeCounts n; size_t header = 0u; const char *field = nullptr;
    switch (merge_blob_check(buf, bytes, mine, e.store.planes ? e.store.capacity - e.store.kept : 0u, &n, &header, &field)) {
    case MERGE_PARSE_OK: break;
    case MERGE_NOT_A_BLOB: return fail(c, ESIM_EINVAL, who + ": not a saved ensemble of this library version");
    case MERGE_TRUNCATED: return fail(c, ESIM_EINVAL, who + ": truncated blob");
    case MERGE_FOREIGN: return fail(c, ESIM_EINVAL, who + ": the blob was saved from another ensemble than the begin in force describes: " + field + " differs");
    case MERGE_KEPT_RANGE: return fail(c, ESIM_ERANGE, who + ": the blob keeps " + std::to_string(n.kept) + " members, more than the store in force has room for; nothing was loaded");
    case MERGE_LENGTH: return fail(c, ESIM_EINVAL, who + ": the blob's length is not what its descriptor and its kept members imply (truncated, or bytes behind its end)");
    }
    const uint8_t *p = (const uint8_t *)buf;
    const size_t cells = (size_t)e.rows.n_rows * e.rows.n_cols;
    MergeFrom from = { nullptr, p + header, p + header + cells * (size_t)merge_cell_bytes(mine), p + header - 12u };
    if (int rc = merge_apply(c, from, n.kept, n.folds)) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));      // (the copies read the caller's buffer: done before it is the caller's again)
    return ESIM_OK;
}
