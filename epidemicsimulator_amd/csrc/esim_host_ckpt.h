// esim_host_ckpt.h -- checkpoint / restore: everything a step reads that is not part of the uploaded population ----------------------
namespace {
struct CkptHeader {
    uint32_t magic, version, n, n_global, id_base, max_steps, host_t, log_len;
    uint32_t exposed_time, infected_time, vaccination_rate, bus_capacity, start_hour, end_hour, ctrl_bytes, layout_id;
    uint64_t seed;
    uint64_t pop_hash;
    double thresholds[6];
};
const uint32_t CKPT_MAGIC = 0x4D495345u /* "ESIM" */, CKPT_VERSION = 3u;

// What a checkpoint's bytes mean depends on how this build lays the state out: the citizen word's fields, the exposure-step
// bias and sentinels, the control block's fields.  The header carries a hash of all of that; a checkpoint written by a build
// with another layout (an older library, a diagnostics build that moved a field) is refused instead of reinterpreted.
constexpr uint32_t layout_mix(uint32_t h, uint32_t v) { return (h ^ v) * 16777619u; }
constexpr uint32_t ckpt_layout_id()
{
    uint32_t h = 2166136261u;
    const uint32_t parts[] = {
        CKPT_VERSION, (uint32_t)sizeof(Ctrl), (uint32_t)sizeof(esim_step_result), (uint32_t)sizeof(Decision),
        (uint32_t)offsetof(Ctrl, t), (uint32_t)offsetof(Ctrl, lockdown), (uint32_t)offsetof(Ctrl, mask), (uint32_t)offsetof(Ctrl, vacc_active),
        (uint32_t)offsetof(Ctrl, have_elig), (uint32_t)offsetof(Ctrl, trigger_step), (uint32_t)offsetof(Ctrl, elig_count), (uint32_t)offsetof(Ctrl, at_work),
        (uint32_t)offsetof(Ctrl, bus_dir), (uint32_t)offsetof(Ctrl, steps_done), (uint32_t)offsetof(Ctrl, error), (uint32_t)offsetof(Ctrl, n_susceptible),
        (uint32_t)offsetof(Ctrl, n_vaccinated), (uint32_t)offsetof(Ctrl, log_len), (uint32_t)offsetof(Ctrl, chunk_pairs), (uint32_t)offsetof(Ctrl, peer_error),
        CW_TE_SHIFT, CW_BUS_EXPOSED, CW_FLAGS, CW_VAX_SHIFT, CW_VAX_MASK, CW_PLAN_SKIP, TE_SUSCEPTIBLE, TE_VACCINATED, TE_RECOVERED, TE_BIAS, TE_SLOTS,
        FL_USES_PT, FL_MASK_COMPLIANT, FL_SAME_AREA, FL_WORK_SCHOOL, FL_HAS_WORK, FL_BIG_ROUTE, MARK_SLOTS, FREE_MAX };
    for (uint32_t v : parts) h = layout_mix(h, v);
    return h;
}

void ckpt_header(const esim_ctx_impl *c, const Ctrl &h, CkptHeader *o)
{
    std::memset(o, 0, sizeof *o);
    o->magic = CKPT_MAGIC; o->version = CKPT_VERSION; o->n = c->d.n; o->n_global = c->d.n_global; o->id_base = c->d.id_base;
    o->max_steps = c->P.max_steps; o->host_t = c->host_t; o->log_len = h.log_len;
    o->exposed_time = c->P.exposed_time; o->infected_time = c->P.infected_time; o->vaccination_rate = c->P.vaccination_rate;
    o->bus_capacity = c->P.bus_capacity; o->start_hour = c->P.start_hour; o->end_hour = c->P.end_hour; o->ctrl_bytes = (uint32_t)sizeof(Ctrl); o->layout_id = ckpt_layout_id();
    o->seed = c->P.seed; o->pop_hash = c->pop_hash;
    const double th[6] = { c->P.exposure_chance, c->P.mask_effectiveness, c->P.lockdown_threshold, c->P.vaccination_threshold,
                           c->P.mask_pt_threshold, c->P.mask_everywhere_threshold };
    std::memcpy(o->thresholds, th, sizeof th);
}

// A run that was rolled back to a snapshot under another seed or vaccination rate has a history drawn under two parameter sets;
// the header names one, and the format does not change for it.
std::string seam_refusal() { return "the run was branched from a snapshot under another seed or vaccination_rate (esim_rollback): a checkpoint's header can name one parameter set only"; }

size_t ckpt_bytes(const CkptHeader &k)
{
    return sizeof(CkptHeader) + k.ctrl_bytes + sizeof(uint32_t) * ((size_t)TE_SLOTS + TE_SLOTS + 1 + k.n + k.log_len + 2u * ((size_t)k.host_t + 1u)) +
           sizeof(esim_step_result) * (size_t)k.host_t;
}
}  // namespace

extern "C" int esim_checkpoint_size(esim_ctx *ctx, size_t *bytes)
{
    esim_ctx_impl *c = CTX(ctx);
    if (!c || !c->uploaded || !bytes) return fail(c, ESIM_ESTATE, "no population uploaded");
    if (c->seam.step) return fail(c, ESIM_ESTATE, "esim_checkpoint_size: " + seam_refusal());
    HIP_TRY(c, hipSetDevice(c->P.device));
    Ctrl h;
    const int rc = read_ctrl(c, &h);
    if (rc) return rc;
    CkptHeader k;
    ckpt_header(c, h, &k);
    *bytes = ckpt_bytes(k);
    return ESIM_OK;
}

extern "C" int esim_checkpoint_save(esim_ctx *ctx, void *buf, size_t cap)
{
    esim_ctx_impl *c = CTX(ctx);
    if (!c || !c->uploaded || !buf) return fail(c, ESIM_ESTATE, "no population uploaded");
    if (c->seam.step) return fail(c, ESIM_ESTATE, "esim_checkpoint_save: " + seam_refusal());
    HIP_TRY(c, hipSetDevice(c->P.device));
    const Dev &d = c->d;
    Ctrl h; int rc;
    if ((rc = read_ctrl(c, &h)) || (rc = ctrl_error(c, h))) return rc;
    CkptHeader k;
    ckpt_header(c, h, &k);
    if (cap < ckpt_bytes(k)) return fail(c, ESIM_ERANGE, "esim_checkpoint_save: buffer smaller than esim_checkpoint_size");
    uint8_t *p = (uint8_t *)buf;
    std::memcpy(p, &k, sizeof k); p += sizeof k;
    std::memcpy(p, &h, sizeof h); p += sizeof h;
    auto pull = [&](const void *src, size_t bytes) -> int { if (bytes) HIP_TRY(c, hipMemcpy(p, src, bytes, hipMemcpyDeviceToHost)); p += bytes; return ESIM_OK; };
    if ((rc = pull(d.hist, sizeof(uint32_t) * TE_SLOTS))) return rc;
    if ((rc = pull(d.log_off, sizeof(uint32_t) * (TE_SLOTS + 1)))) return rc;
    if ((rc = pull(d.cit, sizeof(uint32_t) * (size_t)d.n))) return rc;
    if ((rc = pull(d.log, sizeof(uint32_t) * (size_t)h.log_len))) return rc;
    if ((rc = pull(d.exp_step, sizeof(uint32_t) * 2u * ((size_t)c->host_t + 1u)))) return rc;
    if ((rc = pull(d.records, sizeof(esim_step_result) * (size_t)c->host_t))) return rc;
    return ESIM_OK;
}

extern "C" int esim_checkpoint_restore(esim_ctx *ctx, const void *buf, size_t bytes)
{
    esim_ctx_impl *c = CTX(ctx);
    if (!c || !c->uploaded || !buf) return fail(c, ESIM_ESTATE, "no population uploaded");
    if (bytes < sizeof(CkptHeader)) return fail(c, ESIM_EINVAL, "esim_checkpoint_restore: not a checkpoint");
    CkptHeader k, mine;
    std::memcpy(&k, buf, sizeof k);
    Ctrl zero;
    std::memset(&zero, 0, sizeof zero);
    ckpt_header(c, zero, &mine);
    if (k.magic != CKPT_MAGIC || k.version != CKPT_VERSION || k.ctrl_bytes != sizeof(Ctrl)) return fail(c, ESIM_EINVAL, "esim_checkpoint_restore: not a checkpoint of this library version");
    if (k.layout_id != ckpt_layout_id()) return fail(c, ESIM_EINVAL, "esim_checkpoint_restore: the checkpoint was written by a build with another state layout (citizen word / control block); it is refused, not reinterpreted");
    if (k.n != mine.n || k.n_global != mine.n_global || k.id_base != mine.id_base || k.seed != mine.seed || k.exposed_time != mine.exposed_time ||
        k.infected_time != mine.infected_time || k.vaccination_rate != mine.vaccination_rate || k.bus_capacity != mine.bus_capacity ||
        k.start_hour != mine.start_hour || k.end_hour != mine.end_hour || k.pop_hash != mine.pop_hash || std::memcmp(k.thresholds, mine.thresholds, sizeof k.thresholds) != 0)
        return fail(c, ESIM_EINVAL, "esim_checkpoint_restore: the checkpoint was taken with another population, shard or parameter set");
    if (k.host_t == 0 || k.host_t - 1u > c->P.max_steps || k.log_len > k.n) return fail(c, ESIM_EINVAL, "esim_checkpoint_restore: steps beyond this context's max_steps");
    if (bytes < ckpt_bytes(k)) return fail(c, ESIM_EINVAL, "esim_checkpoint_restore: truncated checkpoint");
    int rc = esim_reset(ctx);                                     // clean marks, chunk tables are clean between calls anyway
    if (rc) return rc;
    const Dev &d = c->d;
    const uint8_t *p = (const uint8_t *)buf + sizeof k;
    Ctrl h;
    std::memcpy(&h, p, sizeof h); p += sizeof h;
    // the control block goes to the device as it is: it must be the one of a context at rest at that step
    if (h.t != k.host_t || h.log_len != k.log_len || h.error != 0u || h.steps_done + 1u != k.host_t || h.n_susceptible > k.n || h.n_vaccinated > k.n)
        return fail(c, ESIM_EINVAL, "esim_checkpoint_restore: the control block does not match the checkpoint's header (corrupt file)");
    h.chunk_ok = 0; h.chunk_parallel = 0; h.chunk_done = 0; h.n_items = 0; h.n_newexp = 0; h.n_units = 0; h.unit_next = 0;
    h.n_route_pairs_big = 0; h.prev_n_items = 0; h.prev_per_wave = 0; h.items_per_wave = 0; h.small_done = 0;
    h.future_t0 = 0; h.n_riders = 0; h.peer_error = 0;
    for (int z = 0; z < 5; ++z) h.counts[z] = 0;
    // marks of the last step are only ever cleared, never read, by the step after it: start without them
    for (uint32_t z = 0; z < MARK_SLOTS; ++z) { h.n_touched_bld[z] = 0; h.n_touched_room[z] = 0; h.n_touched_route[z] = 0; h.n_touched_route_big[z] = 0; }
    auto push = [&](void *dst, size_t nb) -> int { if (nb) HIP_TRY(c, hipMemcpy(dst, p, nb, hipMemcpyHostToDevice)); p += nb; return ESIM_OK; };
    if ((rc = push(d.hist, sizeof(uint32_t) * TE_SLOTS))) return rc;
    if ((rc = push(d.log_off, sizeof(uint32_t) * (TE_SLOTS + 1)))) return rc;
    if ((rc = push(d.cit, sizeof(uint32_t) * (size_t)d.n))) return rc;
    if ((rc = push(d.log, sizeof(uint32_t) * (size_t)k.log_len))) return rc;
    if ((rc = push(d.exp_step, sizeof(uint32_t) * 2u * ((size_t)k.host_t + 1u)))) return rc;
    if ((rc = push(d.records, sizeof(esim_step_result) * (size_t)k.host_t))) return rc;
    HIP_TRY(c, hipMemcpy(d.ctrl, &h, sizeof h, hipMemcpyHostToDevice));
    // (esim_reset above rewound the host to step 1: what follows is the checkpoint's own state, not step 0's)
    c->stop_flag_dev = h.stop_when_done;                          // (the saved block's flag is now the device's: esim_run compares against it)
    c->host_t = k.host_t;
    c->last_chunk_pairs = h.chunk_pairs;
    c->elig_seen = h.have_elig != 0u;
    return ESIM_OK;
}
