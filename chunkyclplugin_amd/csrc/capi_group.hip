// capi_group.hip — a group of contexts (chunky_group_create): its RCCL communicators and the one exchange per read-back.
#include "capi_internal.hpp"

// "rccl 2.22.3 (librccl.so.1), 8 ranks, grouped send/recv of the owned blocks"
static std::string rccl_detail(const chunky_ctx* g, int transport) {
    const RcclApi& api = rccl_api();
    char buf[256];
    snprintf(buf, sizeof buf, "rccl %d.%d.%d (%s), %zu rank(s), %s", api.version / 10000, (api.version / 100) % 100, api.version % 100,
             api.where.c_str(), g->comms.size(),
             transport == CHUNKY_TRANSPORT_RCCL_REDUCE ? "ncclReduce(sum) of the zero-padded framebuffers onto member 0"
             : transport == CHUNKY_TRANSPORT_RCCL_SENDRECV ? "grouped ncclSend / ncclRecv of the owned blocks to member 0"
                                                            : "communicator open, peer copies selected");
    return buf;
}

// Gives up the communicators (after an RCCL failure, or at shutdown): later read-backs use peer copies.
void group_close_rccl(chunky_ctx* g, bool abort) {
    const RcclApi& api = rccl_api();
    for (size_t i = 0; i < g->comms.size(); i++) {
        (void)hipSetDevice(g->members[i]->device);
        if (g->comms[i]) (void)(abort ? api.CommAbort(g->comms[i]) : api.CommDestroy(g->comms[i]));
    }
    g->comms.clear();
    (void)hipGetLastError();
}

// Waits until every stream of `streams` (on `devices`) has drained — WITHOUT blocking in the driver: an RCCL kernel whose peer or
// link died never completes, hipStreamSynchronize would then never return, and the one call that unblocks such a kernel,
// ncclCommAbort, could never be reached.  Polls hipStreamQuery and the communicators' asynchronous errors; returns CHUNKY_OK, or
// CHUNKY_E_HIP with the reason (an error RCCL noticed by itself, or the deadline) — the caller then aborts the communicators FIRST
// and only then synchronises.
static int group_wait(chunky_ctx* g, const std::vector<int>& devices, const std::vector<hipStream_t>& streams) {
    const RcclApi& api = rccl_api();
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<char> done(streams.size(), 0);
    if (g->exchange_timeout_ms == 0)  // (rigs: every exchange counts as hung, whether or not its kernels are still running)
        return fail(CHUNKY_E_HIP, "RCCL exchange unfinished after 0 ms (a hung collective: dead peer or link?)");
    for (unsigned spin = 0;; spin++) {
        bool all = true;
        for (size_t i = 0; i < streams.size(); i++) {
            if (done[i]) continue;
            (void)hipSetDevice(devices[i]);
            const hipError_t q = hipStreamQuery(streams[i]);
            if (q == hipSuccess) {
                done[i] = 1;
            } else if (q == hipErrorNotReady) {
                all = false;
                (void)hipGetLastError();
            } else {
                return fail(CHUNKY_E_HIP, "hipStreamQuery on device %d: %s", devices[i], hipGetErrorString(q));
            }
        }
        if ((spin & 15u) == 0u || all)  // a failure the communicator noticed by itself (a dead link, a dead peer)
            for (size_t i = 0; i < g->comms.size(); i++) {
                ncclResult_t async = ncclSuccess;
                if (api.CommGetAsyncError(g->comms[i], &async) == ncclSuccess && async != ncclSuccess)
                    return fail(CHUNKY_E_HIP, "RCCL communicator of member %zu: %s", i, api.str(async));
            }
        if (all) return CHUNKY_OK;
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (ms > (double)g->exchange_timeout_ms)
            return fail(CHUNKY_E_HIP, "RCCL exchange unfinished after %d ms (a hung collective: dead peer or link?)", g->exchange_timeout_ms);
        if (spin > 64) std::this_thread::sleep_for(std::chrono::microseconds(spin > 4096 ? 500 : 20));
    }
}

// First contact: ONE grouped send / receive of a known pattern from every member to member 0 through the communicators just
// created, under group_wait's deadline, and the bytes compared on the host.  RCCL stays the group's transport only if this
// machine, this process and this library file demonstrably move the right bytes; anything else — an error code, a hang, a
// wrong byte — is found HERE, at group creation, where the answer is "peer copies, and chunky_group_transport says why",
// not in the middle of a render.
// (`send` / `recv` belong to the caller: if the probe ends in a hung exchange they must outlive the abort — hipFree would wait
// for the stuck kernel)
static int group_probe_rccl(chunky_ctx* g, std::vector<DevBuf>& send, std::vector<DevBuf>& recv) {
    const RcclApi& api = rccl_api();
    const size_t n = g->members.size(), count = 1024;
    send.resize(n);
    recv.resize(n);
    std::vector<int> devices;
    std::vector<hipStream_t> streams;
    std::vector<float> host(count);
    for (size_t i = 0; i < n; i++) {
        chunky_ctx* m = g->members[i];
        for (size_t k = 0; k < count; k++) host[k] = (float)(i * 4096 + k + 1);
        HIP_TRY(hipSetDevice(m->device));
        HIP_TRY(send[i].upload(host.data(), count * 4, m->stream));  // (synchronises the member's stream)
        HIP_TRY(hipSetDevice(g->members[0]->device));
        HIP_TRY(recv[i].alloc(count * 4));
        HIP_TRY(hipMemsetAsync(recv[i].p, 0, count * 4, g->members[0]->stream));
        devices.push_back(m->device);
        streams.push_back(m->stream);
    }
    HIP_TRY(hipSetDevice(g->members[0]->device));
    HIP_TRY(hipStreamSynchronize(g->members[0]->stream));
    ncclResult_t rc = api.GroupStart();
    if (rc != ncclSuccess) return fail(CHUNKY_E_HIP, "probe: ncclGroupStart: %s", api.str(rc));
    ncclResult_t bad = ncclSuccess;
    const char* where = "";
    for (size_t i = 0; i < n && bad == ncclSuccess; i++) {
        (void)hipSetDevice(g->members[i]->device);
        if ((bad = api.Send(send[i].p, count, ncclFloat, 0, g->comms[i], g->members[i]->stream)) != ncclSuccess) where = "ncclSend";
        (void)hipSetDevice(g->members[0]->device);
        if (bad == ncclSuccess && (bad = api.Recv(recv[i].p, count, ncclFloat, (int)i, g->comms[0], g->members[0]->stream)) != ncclSuccess) where = "ncclRecv";
    }
    rc = api.GroupEnd();  // (always: the thread's group must be closed; a partial list is dealt with by the caller's abort)
    if (bad != ncclSuccess) return fail(CHUNKY_E_HIP, "probe: %s: %s", where, api.str(bad));
    if (rc != ncclSuccess) return fail(CHUNKY_E_HIP, "probe: ncclGroupEnd: %s", api.str(rc));
    if (int w = group_wait(g, devices, streams)) return w;
    HIP_TRY(hipSetDevice(g->members[0]->device));
    for (size_t i = 0; i < n; i++) {
        HIP_TRY(hipMemcpy(host.data(), recv[i].p, count * 4, hipMemcpyDeviceToHost));
        for (size_t k = 0; k < count; k++)
            if (host[k] != (float)(i * 4096 + k + 1))
                return fail(CHUNKY_E_HIP, "probe: member %zu's float %zu arrived as %g", i, k, (double)host[k]);
    }
    return CHUNKY_OK;
}

// One RCCL communicator over the members of a group (chunky_group_transport).  Never an error: without it the exchange
// runs on peer copies and transport_detail says why.
static void group_open_rccl(chunky_ctx* g, const int* devices, int n) {
    g->transport = CHUNKY_TRANSPORT_PEER_COPY;
    std::string want;
    bool try_shared = false, probe = true;
#ifdef CHUNKY_TUNING  // rigs of tests/test_gpu_rccl_transport.py and tools/: the shipping library reads none of these
    if (const char* env = getenv("CHUNKY_GROUP_TRANSPORT")) want = env;
    const char* self = getenv("CHUNKY_GROUP_SELF_EXCHANGE");
    g->self_exchange = self && *self && *self != '0';
    try_shared = getenv("CHUNKY_RCCL_TRY_SHARED") != nullptr;
    probe = getenv("CHUNKY_GROUP_NO_PROBE") == nullptr;
    if (const char* t = getenv("CHUNKY_GROUP_TIMEOUT_MS")) {
        const int v = atoi(t);
        if (v >= 0 && v <= 600000) g->exchange_timeout_ms = v;
    }
#endif
    if (want == "peer") {
        g->transport_detail = "peer copies: asked for by the environment";
        return;
    }
    for (int i = 0; i < n; i++)
        for (int j = 0; j < i; j++)
            if (devices[i] == devices[j] && !try_shared) {
                // (ncclCommInitAll refuses a device list with duplicates; CHUNKY_RCCL_TRY_SHARED lets the tests watch it do so)
                char buf[128];
                snprintf(buf, sizeof buf, "peer copies: members %d and %d share device %d (one RCCL rank per device)", j, i, devices[i]);
                g->transport_detail = buf;
                return;
            }
    const RcclApi& api = rccl_api();
    if (!api.usable()) {
        g->transport_detail = "peer copies: " + api.error;
        return;
    }
    g->comms.assign((size_t)n, nullptr);
    const ncclResult_t rc = api.CommInitAll(g->comms.data(), n, devices);
    if (rc != ncclSuccess) {
        g->comms.clear();
        (void)hipGetLastError();
        g->transport_detail = std::string("peer copies: ncclCommInitAll: ") + api.str(rc);
        return;
    }
    std::vector<DevBuf> probe_send, probe_recv;  // freed at the end of this function: after the abort and the drain below
    if (probe && group_probe_rccl(g, probe_send, probe_recv) != CHUNKY_OK) {
        const std::string why = tls_error;
        group_close_rccl(g, true);  // abort first (a hung probe kernel is unblocked by nothing else), then drain
        for (chunky_ctx* m : g->members) {
            (void)hipSetDevice(m->device);
            (void)hipStreamSynchronize(m->stream);
        }
        (void)hipGetLastError();
        g->transport_detail = "peer copies: RCCL failed its first exchange (" + why + ")";
        return;
    }
    g->transport = want == "rccl-reduce" ? CHUNKY_TRANSPORT_RCCL_REDUCE : CHUNKY_TRANSPORT_RCCL_SENDRECV;
    g->transport_detail = rccl_detail(g, g->transport) + (probe ? "; first exchange verified" : "");
}

extern "C" int chunky_group_create(const int* devices, int n, chunky_ctx** out) {
    if (!out) return fail(CHUNKY_E_INVALID, "chunky_group_create: out is NULL");
    *out = nullptr;
    if (!devices || n < 1 || n > 64) return fail(CHUNKY_E_INVALID, "chunky_group_create: 1..64 devices");
    std::unique_ptr<chunky_ctx> g(new chunky_ctx);
    for (int i = 0; i < n; i++) {
        chunky_ctx* m = nullptr;
        if (int rc = chunky_init(devices[i], &m)) {
            const std::string why = tls_error;
            for (chunky_ctx* c : g->members) (void)chunky_shutdown(c);
            return fail(rc, "chunky_group_create: member %d: %s", i, why.c_str());
        }
        g->members.push_back(m);
    }
    g->device = g->members[0]->device;
    g->name = g->members[0]->name;
    // the read-back exchange copies member i's blocks into member 0's memory: direct (xGMI) where peer access exists, staged
    // by the runtime where it does not — failing to enable it is not an error
    g->peer_status.assign((size_t)n, CHUNKY_PEER_LOCAL);
    for (int i = 1; i < n; i++) {
        if (devices[i] == devices[0]) continue;
        int can = 0;
        hipError_t e = hipSetDevice(devices[i]);
        if (e == hipSuccess) e = hipDeviceCanAccessPeer(&can, devices[i], devices[0]);
        if (e == hipSuccess && !can) {
            g->peer_status[(size_t)i] = CHUNKY_PEER_STAGED;
        } else if (e == hipSuccess) {
            e = hipDeviceEnablePeerAccess(devices[0], 0);
            if (e == hipErrorPeerAccessAlreadyEnabled) e = hipSuccess;
            g->peer_status[(size_t)i] = e == hipSuccess ? CHUNKY_PEER_DIRECT : -(int)e;
        } else {
            g->peer_status[(size_t)i] = -(int)e;
        }
        (void)hipGetLastError();
    }
    group_open_rccl(g.get(), devices, n);
    (void)hipSetDevice(g->device);
    *out = g.release();
    return CHUNKY_OK;
}

extern "C" int chunky_group_transport(chunky_ctx* ctx, int* transport, char* detail, int detail_len) {
    if (!ctx || !transport) return fail(CHUNKY_E_INVALID, "chunky_group_transport: NULL argument");
    std::lock_guard<std::recursive_mutex> g(ctx->mu);
    *transport = ctx->transport;
    if (detail && detail_len > 0) snprintf(detail, (size_t)detail_len, "%s", ctx->transport_detail.c_str());
    return CHUNKY_OK;
}

extern "C" int chunky_group_set_transport(chunky_ctx* ctx, int transport) {
    if (!ctx) return fail(CHUNKY_E_INVALID, "chunky_group_set_transport: NULL context");
    if (transport != CHUNKY_TRANSPORT_PEER_COPY && transport != CHUNKY_TRANSPORT_RCCL_SENDRECV && transport != CHUNKY_TRANSPORT_RCCL_REDUCE)
        return fail(CHUNKY_E_INVALID, "chunky_group_set_transport: unknown transport %d", transport);
    std::lock_guard<std::recursive_mutex> g(ctx->mu);
    if (transport == ctx->transport) return CHUNKY_OK;
    if (transport != CHUNKY_TRANSPORT_PEER_COPY && ctx->comms.empty())
        return fail(CHUNKY_E_STATE, "chunky_group_set_transport: no RCCL communicator (%s)", ctx->transport_detail.c_str());
    ctx->transport = transport;
    if (!ctx->comms.empty()) ctx->transport_detail = rccl_detail(ctx, transport);
    return CHUNKY_OK;
}

extern "C" int chunky_group_size(chunky_ctx* ctx) {
    if (!ctx) return fail(CHUNKY_E_INVALID, "chunky_group_size: NULL context");
    return ctx->members.empty() ? 1 : (int)ctx->members.size();
}

extern "C" int chunky_group_peer_status(chunky_ctx* ctx, int* out, int n) {
    if (!ctx || !out || n < chunky_group_size(ctx)) return fail(CHUNKY_E_INVALID, "chunky_group_peer_status: need room for %d members", ctx ? chunky_group_size(ctx) : 0);
    if (ctx->members.empty()) {
        out[0] = CHUNKY_PEER_LOCAL;
        return CHUNKY_OK;
    }
    for (size_t i = 0; i < ctx->members.size(); i++) out[i] = ctx->peer_status[i];
    return CHUNKY_OK;
}

extern "C" int chunky_group_device(chunky_ctx* ctx, int i) {
    if (!ctx || i < 0 || i >= chunky_group_size(ctx)) return fail(CHUNKY_E_INVALID, "chunky_group_device: no member %d", i);
    return ctx->members.empty() ? ctx->device : ctx->members[(size_t)i]->device;
}

// The one exchange per read-back of a group: every member but the first packs the pixels of the
// blocks it owns (3 floats each, in the order of its pixel slots), they travel into member 0's memory, and member 0
// scatters them into the image.  Blocks are disjoint, so this is the "reduce of per-tile radiance" with 1/n of the bytes
// per member and no arithmetic: the image is bit for bit what one GPU renders.  What carries them is the group's
// transport (chunky_group_transport): ONE grouped RCCL send / receive, or peer copies; CHUNKY_TRANSPORT_RCCL_REDUCE is
// the literal form instead — one ncclReduce(sum) of the zero-padded framebuffers.
static int gather_buffers(chunky_render* r, size_t i, size_t bytes) {
    chunky_render* pi = r->parts[i];
    if (r->gather_recv[i].bytes < bytes) {
        HIP_TRY(hipSetDevice(r->parts[0]->ctx->device));
        HIP_TRY(r->gather_recv[i].alloc(bytes));
    }
    HIP_TRY(hipSetDevice(pi->ctx->device));
    if (r->gather_send[i].bytes < bytes) {
        HIP_TRY(r->gather_send[i].alloc(bytes));
    }
    return CHUNKY_OK;
}
// member 0 scatters what arrived and the host waits for it
static int gather_scatter(chunky_render* r, size_t first) {
    chunky_render* p0 = r->parts[0];
    std::lock_guard<std::recursive_mutex> g0(p0->ctx->mu);
    HIP_TRY(hipSetDevice(p0->ctx->device));
    for (size_t i = first; i < r->parts.size(); i++)
        if (r->parts[i]->shard.n_local > 0)
            HIP_TRY(launch_gather(false, r->parts[i]->shard, p0->width, p0->height, p0->fb, (float*)r->gather_recv[i].p, p0->ctx->stream));
    HIP_TRY(hipStreamSynchronize(p0->ctx->stream));
    return CHUNKY_OK;
}

static int group_gather_peer(chunky_render* r) {
    const int dev0 = r->parts[0]->ctx->device;
    const size_t n = r->parts.size();
    for (size_t i = 1; i < n; i++) {
        chunky_render* pi = r->parts[i];
        std::lock_guard<std::recursive_mutex> gi(pi->ctx->mu);
        const size_t bytes = (size_t)pi->shard.n_local * 3 * sizeof(float);
        if (bytes == 0) continue;
        if (int rc = gather_buffers(r, i, bytes)) return rc;
        // on member i's stream, behind its queued passes: pack, then the copy across
        HIP_TRY(launch_gather(true, pi->shard, pi->width, pi->height, pi->fb, (float*)r->gather_send[i].p, pi->ctx->stream));
        if (pi->ctx->device == dev0)
            HIP_TRY(hipMemcpyAsync(r->gather_recv[i].p, r->gather_send[i].p, bytes, hipMemcpyDeviceToDevice, pi->ctx->stream));
        else
            HIP_TRY(hipMemcpyPeerAsync(r->gather_recv[i].p, dev0, r->gather_send[i].p, pi->ctx->device, bytes, pi->ctx->stream));
    }
    for (size_t i = 1; i < n; i++) {  // the members work side by side; the host waits for each in turn
        HIP_TRY(hipSetDevice(r->parts[i]->ctx->device));
        HIP_TRY(hipStreamSynchronize(r->parts[i]->ctx->stream));
    }
    return gather_scatter(r, 1);
}

// (inside an open ncclGroupStart: the thread's group has to be closed whatever happened — what was queued up to there may be
// a partial list, e.g. a Send whose Recv was never posted; the caller, group_gather, ABORTS the communicators before it waits
// for any stream, which is what unblocks such a kernel)
#define RCCL_TRY(expr)                                                                           \
    do {                                                                                         \
        const ncclResult_t e_ = (expr);                                                          \
        if (e_ != ncclSuccess) {                                                                 \
            if (in_group) (void)api.GroupEnd();                                                  \
            return fail(CHUNKY_E_HIP, "%s: %s", #expr, api.str(e_));                             \
        }                                                                                        \
    } while (0)

// Every member's stream drained of the passes queued on it (plain blocking waits: nothing of RCCL is on the streams yet), so
// that the deadline of the exchange that follows measures the exchange and not a long render before it.
static int group_drain_passes(chunky_render* r, std::vector<int>* devices, std::vector<hipStream_t>* streams) {
    for (chunky_render* part : r->parts) {
        HIP_TRY(hipSetDevice(part->ctx->device));
        HIP_TRY(hipStreamSynchronize(part->ctx->stream));
        devices->push_back(part->ctx->device);
        streams->push_back(part->ctx->stream);
    }
    return CHUNKY_OK;
}

// ONE grouped RCCL operation: member i's ncclSend of its packed blocks on its own stream (behind the pack kernel), member 0's
// matching ncclRecv's on its stream (ahead of the scatter kernels).  Every call that can fail for reasons of its own — buffer
// allocation, the pack launches, selecting a device — happens BEFORE ncclGroupStart.
static int group_gather_sendrecv(chunky_render* r) {
    const RcclApi& api = rccl_api();
    chunky_ctx* g = r->ctx;
    chunky_render* p0 = r->parts[0];
    const size_t n = r->parts.size(), first = g->self_exchange ? 0 : 1;
    bool in_group = false;
    std::vector<int> devices;
    std::vector<hipStream_t> streams;
    if (int rc = group_drain_passes(r, &devices, &streams)) return rc;
    for (size_t i = first; i < n; i++) {
        chunky_render* pi = r->parts[i];
        std::lock_guard<std::recursive_mutex> gi(pi->ctx->mu);
        const size_t bytes = (size_t)pi->shard.n_local * 3 * sizeof(float);
        if (bytes == 0) continue;
        if (int rc = gather_buffers(r, i, bytes)) return rc;
        HIP_TRY(launch_gather(true, pi->shard, pi->width, pi->height, pi->fb, (float*)r->gather_send[i].p, pi->ctx->stream));
    }
    RCCL_TRY(api.GroupStart());
    in_group = true;
    for (size_t i = first; i < n; i++) {
        chunky_render* pi = r->parts[i];
        const size_t count = (size_t)pi->shard.n_local * 3;
        if (count == 0) continue;
        (void)hipSetDevice(pi->ctx->device);  // (selected successfully a moment ago, in group_drain_passes)
        RCCL_TRY(api.Send(r->gather_send[i].p, count, ncclFloat, 0, g->comms[i], pi->ctx->stream));
        (void)hipSetDevice(p0->ctx->device);
        RCCL_TRY(api.Recv(r->gather_recv[i].p, count, ncclFloat, (int)i, g->comms[0], p0->ctx->stream));
    }
    in_group = false;
    RCCL_TRY(api.GroupEnd());
    if (int rc = group_wait(g, devices, streams)) return rc;  // the sends and the receives are complete, or the deadline has passed
    return gather_scatter(r, first);
}

// The literal form: every member clears what it does not own (after chunky_render_set_shard on a live render a member may still
// hold pixels of its old share; member 0 holds the blocks earlier read-backs left there), every framebuffer is then zero outside
// its member's own blocks, and ONE ncclReduce(sum) onto member 0 assembles the image in place.  (Pixels NO member owns — the
// other ranks' when the group itself is one rank of an outer chunky_render_set_shard split — are zero afterwards; the other two
// transports leave them as they were.)
static int group_gather_reduce(chunky_render* r) {
    const RcclApi& api = rccl_api();
    chunky_ctx* g = r->ctx;
    chunky_render* p0 = r->parts[0];
    const size_t n = r->parts.size();
    const size_t count = (size_t)p0->width * p0->height * 3;
    bool in_group = false;
    std::vector<int> devices;
    std::vector<hipStream_t> streams;
    if (int rc = group_drain_passes(r, &devices, &streams)) return rc;
    for (size_t i = 0; i < n; i++) {
        chunky_render* pi = r->parts[i];
        std::lock_guard<std::recursive_mutex> gi(pi->ctx->mu);
        HIP_TRY(hipSetDevice(pi->ctx->device));
        HIP_TRY(launch_clear_foreign(pi->shard, pi->width, pi->height, pi->fb, pi->ctx->stream));
    }
    RCCL_TRY(api.GroupStart());
    in_group = true;
    for (size_t i = 0; i < n; i++) {
        chunky_render* pi = r->parts[i];
        (void)hipSetDevice(pi->ctx->device);
        RCCL_TRY(api.Reduce(pi->fb, pi->fb, count, ncclFloat, ncclSum, 0, g->comms[i], pi->ctx->stream));
    }
    in_group = false;
    RCCL_TRY(api.GroupEnd());
    if (int rc = group_wait(g, devices, streams)) return rc;
    HIP_TRY(hipSetDevice(p0->ctx->device));
    return CHUNKY_OK;
}
#undef RCCL_TRY

int group_gather(chunky_render* r) {
    chunky_ctx* g = r->ctx;
    if (g->transport != CHUNKY_TRANSPORT_PEER_COPY && !g->comms.empty()) {
        const int rc = g->transport == CHUNKY_TRANSPORT_RCCL_REDUCE ? group_gather_reduce(r) : group_gather_sendrecv(r);
        if (rc == CHUNKY_OK) return rc;
        // An RCCL call failed: the render must not be lost with it.  The members' own blocks are intact (the exchange only
        // ever writes buffers of its own, and — the reduce — pixels of member 0's image that member 0 does not own), so the
        // same read-back runs again on peer copies, and so does every later one; chunky_group_transport says why.
        // ABORT FIRST: if an RCCL kernel sits unfinished on a member's stream (a dead peer, or the partial list of a call that
        // failed inside ncclGroupStart), only ncclCommAbort ends it — a stream wait before the abort would never return.
        const std::string why = tls_error;
        group_close_rccl(g, true);
        for (chunky_render* part : r->parts) {
            (void)hipSetDevice(part->ctx->device);
            (void)hipStreamSynchronize(part->ctx->stream);
        }
        (void)hipGetLastError();
        g->transport = CHUNKY_TRANSPORT_PEER_COPY;
        g->transport_detail = "peer copies: " + why;
    }
    return group_gather_peer(r);
}

extern "C" int chunky_render_gather(chunky_render* r) {
    if (r && !r->parts.empty()) {
        std::lock_guard<std::recursive_mutex> g(r->ctx->mu);
        return group_gather(r);
    }
    return chunky_render_sync(r);
}
