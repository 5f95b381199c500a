// esim_host_shard.h -- the exchange between shards, the communicator's set-up, sharded chunks and esim_run_sharded.
// SUM all-reduces of small uint32 device buffers (the commuter exchange and the census).  Two transports:
// RCCL over xGMI, with the communicator owned by the library and the collective enqueued on the context's own stream between
// its kernels (no host synchronisation per step); or a caller-supplied function (tests on one GPU: gloo through the Python
// binding), which is called with the stream drained.  librccl is loaded on first use, so a build without it still runs.
namespace {

// the entry points of librccl the exchange uses, each named once (their types from rccl.h)
#define RCCL_ENTRIES(X) X(GetUniqueId) X(CommInitRank) X(CommDestroy) X(CommAbort) X(Send) X(Recv) X(GroupStart) X(GroupEnd) X(AllReduce) X(GetErrorString)
struct RcclApi {
#define X(f) decltype(&nccl##f) f = nullptr;
    RCCL_ENTRIES(X)
#undef X
    bool ok = false;
};

RcclApi &rccl()
{
    static RcclApi api;
    static bool tried = false;
    if (tried) return api;
    tried = true;
    void *h = nullptr;
    // a copy the process has loaded already (e.g. the one PyTorch ships) is reused: one RCCL runtime per process
    for (const char *name : { "librccl.so", "librccl.so.1" }) if ((h = dlopen(name, RTLD_NOW | RTLD_NOLOAD))) break;
    if (!h) for (const char *name : { "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1" }) if ((h = dlopen(name, RTLD_NOW | RTLD_GLOBAL))) break;
    if (!h) return api;
    api.ok = true;
#define X(f) if (!(api.f = (decltype(api.f))dlsym(h, "nccl" #f))) api.ok = false;
    RCCL_ENTRIES(X)
#undef X
    return api;
}

void comm_release(esim_ctx_impl *c)
{
    if (c->comm.nccl && rccl().ok) rccl().CommDestroy(c->comm.nccl);
    c->comm.nccl = nullptr;
}

// SUM all-reduce of n uint32 at device pointer buf over the shards, in place, ordered after everything enqueued so far.
// `which` names the buffer for a caller's transport (0 A, 1 B, 2 F, 3 plan liveness, 4 commuter records, 5 cuts, 6 records).
int exchange_buf(esim_ctx_impl *c, int which, uint32_t *buf, size_t n)
{
    c->comm.calls++;
    if (c->comm.nccl) {
        ncclResult_t r = rccl().AllReduce(buf, buf, n, ncclUint32, ncclSum, c->comm.nccl, c->stream);
        if (r != ncclSuccess) return fail(c, ESIM_ENODEVICE, std::string("ncclAllReduce: ") + rccl().GetErrorString(r));
        return ESIM_OK;
    }
    if (c->comm.fn) {
        // the caller's transport works on host memory: stage through a host buffer with the stream drained
        c->comm.stage.resize(n);
        HIP_TRY(c, hipMemcpyAsync(c->comm.stage.data(), buf, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        if (c->comm.fn(c->comm.user, which, c->comm.stage.data(), n) != 0) return fail(c, ESIM_ENODEVICE, "the caller's all-reduce failed");
        HIP_TRY(c, hipMemcpyAsync(buf, c->comm.stage.data(), sizeof(uint32_t) * n, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        return ESIM_OK;
    }
    return fail(c, ESIM_ESTATE, "sharded run without a communicator (esim_comm_init_rccl / esim_comm_init_callback)");
}

// All-to-all: rank s sends the `seg` words at out + d * seg to rank d, and receives rank r's words for it at in + r * seg.  RCCL:
// one group of ncclSend / ncclRecv pairs on the context's stream (every pair of shards talks over its own xGMI link).  A caller's
// transport only has a SUM all-reduce: the ranks' rows of the [sender][receiver] matrix are summed and each picks its column.
int exchange_alltoall(esim_ctx_impl *c, int which, const uint32_t *out, uint32_t *in, size_t seg)
{
    const int W = c->comm.world, me = c->comm.rank;
    if (W <= 1) return ESIM_OK;
    c->comm.calls++;
    if (c->comm.nccl) {
        ncclResult_t r = rccl().GroupStart();
        for (int p = 0; p < W && r == ncclSuccess; ++p) {
            if (p == me) continue;
            r = rccl().Send(out + (size_t)p * seg, seg, ncclUint32, p, c->comm.nccl, c->stream);
            if (r == ncclSuccess) r = rccl().Recv(in + (size_t)p * seg, seg, ncclUint32, p, c->comm.nccl, c->stream);
        }
        const ncclResult_t e = rccl().GroupEnd();
        if (r == ncclSuccess) r = e;
        if (r != ncclSuccess) return fail(c, ESIM_ENODEVICE, std::string("ncclSend/ncclRecv: ") + rccl().GetErrorString(r));
        return ESIM_OK;
    }
    if (c->comm.fn) {
        const size_t n = (size_t)W * W * seg;
        c->comm.stage.assign(n, 0u);
        HIP_TRY(c, hipMemcpyAsync(c->comm.stage.data() + (size_t)me * W * seg, out, sizeof(uint32_t) * (size_t)W * seg, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        for (size_t i = 0; i < seg; ++i) c->comm.stage[((size_t)me * W + me) * seg + i] = 0u;          // (nothing goes to oneself)
        if (c->comm.fn(c->comm.user, which, c->comm.stage.data(), n) != 0) return fail(c, ESIM_ENODEVICE, "the caller's all-reduce failed");
        for (int p = 0; p < W; ++p)
            if (p != me) HIP_TRY(c, hipMemcpyAsync(in + (size_t)p * seg, c->comm.stage.data() + ((size_t)p * W + me) * seg, sizeof(uint32_t) * seg, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        return ESIM_OK;
    }
    return fail(c, ESIM_ESTATE, "sharded run without a communicator (esim_comm_init_rccl / esim_comm_init_callback)");
}

// what the exchange of sharded chunks needs once the number of ranks is known; and the ranks' shards are checked against each
// other -- one world (n_citizens_global, shared tables of the same size), rank r holding the r-th stretch of the global
// citizen ids -- with one small all-reduce: a communicator over shards that do not belong together would run without an
// error and give wrong records.
int comm_buffers(esim_ctx_impl *c)
{
    if (!c->uploaded) return fail(c, ESIM_ESTATE, "esim_comm_init: upload the population first");
    HIP_TRY(c, hipSetDevice(c->P.device));
    Dev &d = c->d; int rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    dev_free(c, d.xs); dev_free(c, d.xs_out); dev_free(c, (void *)d.shared_mask);
    d.xs = nullptr; d.xs_out = nullptr; d.shared_mask = nullptr;
    if (c->comm.xr) { dev_free(c, c->comm.xr); c->comm.xr = nullptr; c->comm.xr_n = 0; }
    d.rank = (uint32_t)c->comm.rank; d.world = (uint32_t)c->comm.world;
    const size_t n = (size_t)d.world * (1u + 3u * (size_t)XS_CAP_MAX);
    d.xs_cap = 4096u;
    if (const char *e = std::getenv("ESIM_XS_CAP")) d.xs_cap = (uint32_t)std::min<long>(XS_CAP_MAX, std::max<long>(1, std::atol(e)));   // (tests: a segment that has to grow)
    if ((rc = dev_alloc_fill(c, &d.xs, n))) return rc;
    // the layout check
    const uint32_t W = d.world;
    std::vector<uint32_t> rows((size_t)W * 5u, 0u);
    uint32_t *mine = &rows[(size_t)d.rank * 5u];
    mine[0] = d.id_base; mine[1] = d.n; mine[2] = d.n_global; mine[3] = d.n_shared_bld; mine[4] = d.n_shared_room;
    DevTmp<uint32_t> dv;                 // (freed on every way out)
    if (const hipError_t e = dv.alloc(rows.size())) return alloc_failed(c, e);
    HIP_TRY(c, hipMemcpy(dv.p, rows.data(), sizeof(uint32_t) * rows.size(), hipMemcpyHostToDevice));
    if ((rc = exchange_buf(c, 8, dv.p, rows.size())) || (rc = wait_stream(c))) return rc;
    if (hipMemcpy(rows.data(), dv.p, sizeof(uint32_t) * rows.size(), hipMemcpyDeviceToHost) != hipSuccess) return fail(c, ESIM_ENODEVICE, "esim_comm_init: read-back of the layout check failed");
    uint64_t next = 0;
    for (uint32_t r = 0; r < W; ++r) {
        const uint32_t *q = &rows[(size_t)r * 5u];
        if (q[2] != d.n_global || q[3] != d.n_shared_bld || q[4] != d.n_shared_room || q[0] != next) {
            char msg[256];
            std::snprintf(msg, sizeof msg, "esim_comm_init: rank %u holds citizens [%u, %u) of %u with %u / %u shared buildings / rooms -- not shard %u of the world this rank's shard belongs to "
                          "(expected ids from %llu, %u citizens in all, %u / %u shared)", r, q[0], q[0] + q[1], q[2], q[3], q[4], r, (unsigned long long)next, d.n_global, d.n_shared_bld, d.n_shared_room);
            return fail(c, ESIM_EINVAL, msg);
        }
        next += q[1];
    }
    if (next != d.n_global) return fail(c, ESIM_EINVAL, "esim_comm_init: the ranks' shards do not add up to n_citizens_global (world size differs from the number of shards)");
    // which shards have members in each shared building: every shard sets its own bit where it has, the bits are summed
    uint32_t *mask = nullptr;
    if ((rc = dev_alloc(c, &mask, (size_t)d.n_shared_bld + 1u))) return rc;
    d.shared_mask = mask;
    std::vector<uint32_t> bits((size_t)d.n_shared_bld + 1u, 0u);
    std::vector<int32_t> local((size_t)d.n_shared_bld + 1u, -1);
    if (d.n_shared_bld) HIP_TRY(c, hipMemcpy(local.data(), d.shared_bld, sizeof(int32_t) * d.n_shared_bld, hipMemcpyDeviceToHost));
    for (uint32_t k = 0; k < d.n_shared_bld; ++k) bits[k] = local[k] >= 0 ? 1u << d.rank : 0u;
    HIP_TRY(c, hipMemcpy(mask, bits.data(), sizeof(uint32_t) * bits.size(), hipMemcpyHostToDevice));
    if ((rc = exchange_buf(c, 9, mask, bits.size()))) return rc;
    if ((rc = wait_stream(c))) return rc;
    return dev_alloc_fill(c, &d.xs_out, n);
}

int exchange(esim_ctx_impl *c, int which)
{
    Dev &d = c->d;
    uint32_t *buf = which == 2 ? d.xf : which ? d.xb : d.xa;
    const size_t n = which == 2 ? c->xf_n + 1 : which ? c->xb_n : c->xa_n;
    return exchange_buf(c, which, buf, n);
}

// The host's wait for a stream that holds RCCL collectives has a deadline: a peer that died or left (a crash, an exchange that
// failed on its side) would otherwise leave this rank inside a collective for ever.  On expiry the communicator is aborted
// (ncclCommAbort ends the collective kernels), the context is left without one, and the call fails with ESIM_ETIMEDOUT -- the
// caller is expected to exit with an error, as the reference does when step() fails (run/src/main.rs:306-308).
int wait_stream(esim_ctx_impl *c)
{
    if (!c->comm.nccl) { HIP_TRY(c, hipStreamSynchronize(c->stream)); return ESIM_OK; }
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        const hipError_t e = hipStreamQuery(c->stream);
        if (e == hipSuccess) return ESIM_OK;
        if (e != hipErrorNotReady) return fail(c, ESIM_ENODEVICE, std::string("hipStreamQuery: ") + hipGetErrorString(e));
        const double waited = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (waited > c->comm.timeout_s) {
            (void)rccl().CommAbort(c->comm.nccl);
            c->comm.nccl = nullptr;
            char msg[200];
            std::snprintf(msg, sizeof msg, "rank %d: no progress on the stream for %.1f s inside a sharded run (a peer left or died); the RCCL communicator was aborted",
                          c->comm.rank, waited);
            return fail(c, ESIM_ETIMEDOUT, msg);
        }
        if (waited > 2e-3) std::this_thread::sleep_for(std::chrono::microseconds(waited > 0.1 ? 1000 : 20));
    }
}

// Every read-back of the control block in a sharded run: the shards' error fields are summed first (k_status_pack ->
// all-reduce -> k_status_unpack), so every rank sees any rank's device-side error in the same collective and takes the same
// return decision from the same word.
int sync_status(esim_ctx_impl *c, bool ex, Ctrl *h)
{
    Dev &d = c->d; int rc;
    hipLaunchKernelGGL(k_status_pack, dim3(1), dim3(64), 0, c->stream, d);
    if (ex && (rc = exchange_buf(c, 7, d.xe, XE_WORDS))) return rc;
    hipLaunchKernelGGL(k_status_unpack, dim3(1), dim3(64), 0, c->stream, d);
    HIP_TRY(c, hipMemcpyAsync(c->pin.ctrl, d.ctrl, sizeof(Ctrl), hipMemcpyDeviceToHost, c->stream));
    if ((rc = wait_stream(c))) return rc;
    *h = *c->pin.ctrl;
    return ctrl_error(c, *h);       // (k_status_unpack raised any shard's error here too: every rank returns the same code)
}

}  // namespace

extern "C" int esim_comm_unique_id(void *out, size_t cap)
{
    if (!out || cap < sizeof(ncclUniqueId)) return ESIM_EINVAL;
    if (!rccl().ok) return fail(nullptr, ESIM_ENODEVICE, "librccl could not be loaded");
    ncclUniqueId id;
    ncclResult_t r = rccl().GetUniqueId(&id);
    if (r != ncclSuccess) return fail(nullptr, ESIM_ENODEVICE, std::string("ncclGetUniqueId: ") + rccl().GetErrorString(r));
    std::memcpy(out, &id, sizeof id);
    return ESIM_OK;
}

extern "C" int esim_comm_init_rccl(esim_ctx *ctx, const void *unique_id, size_t id_bytes, int rank, int world)
{
    esim_ctx_impl *c = CTX(ctx);
    if (!c || !unique_id || id_bytes < sizeof(ncclUniqueId) || rank < 0 || rank >= world || world > (int)ERR_MAX_WORLD) return fail(c, ESIM_EINVAL, "esim_comm_init_rccl: bad argument (0 <= rank < world <= 31)");
    if (!c->uploaded) return fail(c, ESIM_ESTATE, "esim_comm_init_rccl: upload the population first");
    if (!rccl().ok) return fail(c, ESIM_ENODEVICE, "librccl could not be loaded");
    HIP_TRY(c, hipSetDevice(c->P.device));
    if (c->comm.nccl) { rccl().CommDestroy(c->comm.nccl); c->comm.nccl = nullptr; }
    ncclUniqueId id;
    std::memcpy(&id, unique_id, sizeof id);
    ncclResult_t r = rccl().CommInitRank(&c->comm.nccl, world, id, rank);
    if (r != ncclSuccess) { c->comm.nccl = nullptr; return fail(c, ESIM_ENODEVICE, std::string("ncclCommInitRank: ") + rccl().GetErrorString(r)); }
    c->comm.rank = rank; c->comm.world = world; c->comm.fn = nullptr;
    const int rc = comm_buffers(c);
    if (rc) { comm_release(c); c->comm.rank = 0; c->comm.world = 1; c->d.rank = 0; c->d.world = 1; }
    return rc;
}

extern "C" int esim_comm_init_callback(esim_ctx *ctx, esim_allreduce_fn fn, void *user, int rank, int world)
{
    esim_ctx_impl *c = CTX(ctx);
    if (!c || !fn || rank < 0 || rank >= world || world > (int)ERR_MAX_WORLD) return fail(c, ESIM_EINVAL, "esim_comm_init_callback: bad argument (0 <= rank < world <= 31)");
    if (!c->uploaded) return fail(c, ESIM_ESTATE, "esim_comm_init_callback: upload the population first");
    if (c->comm.nccl) { rccl().CommDestroy(c->comm.nccl); c->comm.nccl = nullptr; }
    c->comm.fn = fn; c->comm.user = user; c->comm.rank = rank; c->comm.world = world;
    const int rc = comm_buffers(c);
    if (rc) { c->comm.fn = nullptr; c->comm.rank = 0; c->comm.world = 1; c->d.rank = 0; c->d.world = 1; }
    return rc;
}

extern "C" int esim_comm_set_timeout(esim_ctx *ctx, double seconds)
{
    esim_ctx_impl *c = CTX(ctx);
    if (!c || !(seconds > 0.0)) return fail(c, ESIM_EINVAL, "esim_comm_set_timeout: seconds must be positive");
    c->comm.timeout_s = seconds;
    return ESIM_OK;
}

extern "C" int esim_debug_inject_error(esim_ctx *ctx, int code)
{
    esim_ctx_impl *c = CTX(ctx);
    if (!c || !c->uploaded || code > -1 || code < -6) return fail(c, ESIM_EINVAL, "esim_debug_inject_error: code must be one of the ESIM_E* values");
    if (int rc = drain(c)) return rc;
    const uint32_t v = (uint32_t)(-code);
    HIP_TRY(c, hipMemcpy(&c->d.ctrl->error, &v, sizeof v, hipMemcpyHostToDevice));
    c->rest_t = 0;                                                 // (the pinned mirror no longer is the control block as it stands)
    return ESIM_OK;
}

extern "C" int esim_comm_stats(esim_ctx *ctx, uint64_t *collectives)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    if (collectives) *collectives = c->comm.calls;
    return ESIM_OK;
}

namespace {

// One time-parallel chunk of a sharded run: what the shards exchange once per chunk instead of once per step --
// the liveness of the plan's candidates (V), the Infected commuters to shared buildings (S, all-to-all), the Infected census
// ahead with the "cannot" word (F), the steps with a cut (C).  Kernels and collectives are enqueued on the context's stream.
int enqueue_sharded_chunk(esim_ctx_impl *c, uint32_t limit_t, bool vax)
{
    Dev &d = c->d;
    const ChunkPass p{ c, limit_t, false };
    const uint32_t n_ahead = p.n_ahead();
    const size_t xv_n = XV_HEADER + (size_t)FREE_MAX * (PLAN_W / 32u);
    int rc;
    p.future(n_ahead);
    if (vax) {
        hipLaunchKernelGGL(k_vax_live<false>, dim3(PLAN_W / TPB, FREE_MAX), dim3(TPB), 0, c->stream, d, n_ahead, limit_t);
        if ((rc = exchange_buf(c, 3, d.xv, xv_n))) return rc;
        p.vax_plan(1);
    }
    // the commuter exchange, all-to-all: a record goes to the shards that have members in its building;
    // segments of the same size between every pair of shards (their need is exchanged with the status, so they grow alike
    // everywhere).  One rank sends nothing.
    const size_t seg = 1u + 3u * (size_t)d.xs_cap;
    for (uint32_t r = 0; r < d.world; ++r) HIP_TRY(c, hipMemsetAsync(d.xs_out + (size_t)r * seg, 0, sizeof(uint32_t), c->stream));
    hipLaunchKernelGGL(k_shared_pack, dim3(256), dim3(TPB), 0, c->stream, d, n_ahead, limit_t);
    if ((rc = exchange_alltoall(c, 4, d.xs_out, d.xs, seg))) return rc;
    hipLaunchKernelGGL(k_shard_prep, dim3(1), dim3(128), 0, c->stream, d, n_ahead, limit_t);
    if ((rc = exchange(c, 2))) return rc;
    p.decide(n_ahead, 1, 1);
    p.front(false);
    if (vax && c->tune.vax_repair && (c->repair_armed || c->tune.vax_repair_always)) {
        // the repair of the plan (DESIGN.md 3.13 v), sharded: the shards agree on the step to walk again from (buffer L), exchange
        // the liveness of the candidates as it truly stood (buffer V a second time) and walk the same steps again
        p.lost();
        if ((rc = exchange_buf(c, 10, d.xl, FREE_MAX + 2u))) return rc;
        hipLaunchKernelGGL(k_lost_global, dim3(1), dim3(64), 0, c->stream, d);
        hipLaunchKernelGGL(k_vax_live<true>, dim3(PLAN_W / TPB, FREE_MAX), dim3(TPB), 0, c->stream, d, n_ahead, limit_t);
        if ((rc = exchange_buf(c, 3, d.xv, xv_n))) return rc;
        p.vax_repair(1);
    }
    p.count();
    if (vax && (rc = exchange_buf(c, 5, d.xc, FREE_MAX + 2u))) return rc;
    p.books(0, 0);
    p.scatter();
    p.vax_final();
    HIP_TRY(c, hipGetLastError());
    return ESIM_OK;
}

// n coupled steps: three device phases around the two per-step exchanges (the form every step can take)
int run_coupled_steps(esim_ctx_impl *c, uint32_t n, bool ex)
{
    int rc;
    for (uint32_t s = 0; s < n; ++s) {
        const bool tk = want_kernel_timing(c);
        if ((rc = enqueue_begin(c, tk))) return rc;
        if (ex && (rc = exchange(c, 0))) return rc;
        if ((rc = enqueue_exposures(c))) return rc;
        if (ex && (rc = exchange(c, 1))) return rc;
        if ((rc = enqueue_finish(c, tk))) return rc;
        if ((s & 255u) == 255u && (rc = wait_stream(c))) return rc;
    }
    c->comm.step_steps += n;
    return ESIM_OK;
}

}  // namespace

// Simulator::simulate's loop for one shard of a sharded population.  Steps run as time-parallel chunks with one round of
// exchanges per chunk wherever a chunk can run on every shard, and as coupled steps (three device phases around two exchanges
// per step) otherwise: the step that starts the vaccination programme, chunks that do not fit the one-pass form somewhere, plans
// that need more candidates than the exchanged window.  Every rank takes the same decisions from the same reduced words.
// Over RCCL nothing waits for the host inside a burst of chunks.
extern "C" int esim_run_sharded(esim_ctx *ctx, uint32_t n_steps, uint32_t *n_done)
{
    esim_ctx_impl *c = CTX(ctx);
    int rc = check_budget(c, n_steps);
    if (rc) return rc;
    if (c->d.n_shards > 1 && !c->comm.nccl && !c->comm.fn) return fail(c, ESIM_ESTATE, "esim_run_sharded: no communicator (esim_comm_init_rccl / esim_comm_init_callback)");
    HIP_TRY(c, hipSetDevice(c->P.device));
    Dev &d = c->d;
    const uint32_t first = c->host_t;
    c->rest_t = 0;
    // no early stop here (a shard's local census says nothing about the disease elsewhere, and shards that stopped at
    // different steps would issue different collectives): a flag an earlier esim_run left on the device is cleared
    static const uint32_t zero = 0u;
    HIP_TRY(c, hipMemcpyAsync(&d.ctrl->stop_when_done, &zero, sizeof zero, hipMemcpyHostToDevice, c->stream));
    c->stop_flag_dev = 0u;                                        // (esim_run compares against it before it writes the flag)
    // (a communicator on an unsharded context -- one rank -- still makes its collectives: the sums over one rank change nothing,
    // which is how the RCCL path is exercised on a one-GPU box)
    const bool ex = d.n_shards > 1 || c->comm.nccl || c->comm.fn;
    const bool chunks = ex && d.xs && c->tune.pipeline && c->tune.time_parallel && d.items_cap > 0;
    std::vector<std::pair<uint32_t, uint32_t>> local_ranges;     // [first step, count) whose records hold this shard's census
    uint32_t remaining = n_steps, stall = 0;
    Ctrl h;
    while (remaining > 0) {
        if (chunks && (!c->elig_seen || c->tune.vax_chunks)) {
            const uint32_t t_first = c->host_t, limit_t = t_first + remaining - 1u;
            const uint32_t bursts = stall ? 1u : std::min<uint32_t>((remaining + (uint32_t)c->xf_n - 1u) / (uint32_t)c->xf_n + (c->elig_seen ? 1u : 0u), 4u);
            for (uint32_t g = 0; g < bursts; ++g) if ((rc = enqueue_sharded_chunk(c, limit_t, c->elig_seen))) return rc;
            // every rank reads the same decision words: steps advanced (all shards run a chunk or none does), the summed error
            // fields, the segment need of every shard
            if ((rc = sync_status(c, ex, &h))) return rc;
            const uint32_t done = h.t - t_first;
            c->host_t = h.t; remaining -= done;
            c->comm.chunk_steps += done;
            if (h.vax_cuts > c->vax_chunk_cuts) c->repair_armed = true;  // (cuts are decided from summed words: every rank arms in the same burst)
            c->vax_chunk_cuts = h.vax_cuts; c->vax_chunk_repairs = h.vax_repairs;
            // the commuter segment follows the need (the same on every rank: the needs came with the status exchange)
            const uint32_t cap_before = d.xs_cap;
            while (d.xs_cap < XS_CAP_MAX && 2u * h.xs_need_all > d.xs_cap) d.xs_cap *= 2u;     // (xs_need_all: the maximum over the shards, from the status exchange)
            if (done) { local_ranges.emplace_back(t_first, done); stall = 0; continue; }
            if (std::getenv("ESIM_DEBUG"))
                std::fprintf(stderr, "[esim] rank %d: sharded chunk without progress at t=%u: chunk_ok=%u parallel=%u vax_chunk=%u vax_fail=%u cannot=%u xs_need=%u xs_cap=%u pairs=%u\n",
                             c->comm.rank, h.t, h.chunk_ok, h.chunk_parallel, h.vax_chunk, h.vax_fail, 0u, h.xs_need_all, cap_before, h.chunk_pairs);
            if (d.xs_cap != cap_before) continue;                        // the segment was too short: again with the longer one
            stall = std::min<uint32_t>(stall + 1u, 8u);
        }
        const uint32_t k = std::min<uint32_t>(remaining, (!chunks || (c->elig_seen && !c->tune.vax_chunks)) ? remaining : (stall <= 1u ? 1u : (stall <= 3u ? 8u : (uint32_t)c->xf_n)));
        if ((rc = run_coupled_steps(c, k, ex))) return rc;
        remaining -= k;
        if ((rc = sync_status(c, ex, &h))) return rc;
        c->elig_seen = h.have_elig != 0u;
    }
    // the records of the steps drawn as chunks: this shard's census -> everybody's
    for (auto &rg : local_ranges) {
        const size_t n = (size_t)rg.second * XR_FIELDS;
        if (n > c->comm.xr_n) {
            if ((rc = wait_stream(c))) return rc;                        // (the buffer being replaced may still be in use)
            if (c->comm.xr) dev_free(c, c->comm.xr);
            c->comm.xr = nullptr; c->comm.xr_n = 0;
            if ((rc = dev_alloc(c, &c->comm.xr, n))) return rc;
            c->comm.xr_n = n;
        }
        hipLaunchKernelGGL(k_records_pack, dim3(grid_for(rg.second, TPB, 64)), dim3(TPB), 0, c->stream, d, rg.first, rg.second, c->comm.xr);
        if (ex && (rc = exchange_buf(c, 6, c->comm.xr, n))) return rc;
        hipLaunchKernelGGL(k_records_unpack, dim3(grid_for(rg.second, TPB, 64)), dim3(TPB), 0, c->stream, d, rg.first, rg.second, c->comm.xr);
    }
    if ((rc = wait_stream(c))) return rc;
    if (n_done) *n_done = c->host_t - first;
    return ESIM_OK;
}

extern "C" int esim_shard_stats(esim_ctx *ctx, uint64_t *chunk_steps, uint64_t *coupled_steps)
{
    esim_ctx_impl *c = CTX(ctx); if (!c) return ESIM_EINVAL;
    if (chunk_steps) *chunk_steps = c->comm.chunk_steps;
    if (coupled_steps) *coupled_steps = c->comm.step_steps;
    return ESIM_OK;
}
