// capi_selftest.hip — self tests: device helpers called on their own.
#include "capi_internal.hpp"

extern "C" int chunky_selftest_math(chunky_ctx* ctx, int which, int n, const float* a, const float* b, float* out) {
    if (!ctx) return fail(CHUNKY_E_INVALID, "NULL context");
    if (!ctx->members.empty()) ctx = ctx->members[0];
    if (n < 0 || (n > 0 && (!a || !b || !out))) return fail(CHUNKY_E_INVALID, "selftest_math: bad arguments");
    if (n == 0) return CHUNKY_OK;
    std::lock_guard<std::recursive_mutex> g(ctx->mu);
    HIP_TRY(hipSetDevice(ctx->device));
    DevBuf da, db, dout;
    HIP_TRY(da.upload(a, (size_t)n * 4, ctx->stream));
    HIP_TRY(db.upload(b, (size_t)n * 4, ctx->stream));
    HIP_TRY(hipMalloc(&dout.p, (size_t)n * 4));
    HIP_TRY(launch_math_selftest(which, n, (const float*)da.p, (const float*)db.p, (float*)dout.p, ctx->stream));
    HIP_TRY(hipMemcpyAsync(out, dout.p, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return CHUNKY_OK;
}

extern "C" int chunky_selftest_plan_biome(const int32_t* plans16, int64_t n, int32_t* out16, int32_t* refusal) {
    if (n < 0 || (n > 0 && (!plans16 || !out16 || !refusal))) return fail(CHUNKY_E_INVALID, "selftest_plan_biome: bad arguments");
    for (int64_t i = 0; i < n; i++) {
        const int32_t* v = plans16 + 16 * i;
        RenderPlan p{};
        p.family = (KernelFamily)v[0], p.tree = v[1], p.park = v[2], p.words = v[3], p.group = v[4], p.depth = v[5];
        p.bvh = v[6] != 0, p.ext = v[7] != 0, p.stats = v[8] != 0, p.sorted = v[9] != 0, p.proj = v[10] != 0;
        p.lds = (size_t)(uint32_t)v[11], p.most = v[12], p.needs_list = v[13] != 0, p.status = (PlanStatus)v[14], p.ext_refusal = (ExtRefusal)v[15];
        const BiomePlan b = plan_biome(p);
        const RenderPlan& q = b.plan;
        const int32_t o[16] = {(int32_t)q.family, q.tree, q.park, q.words, q.group, q.depth, q.bvh, q.ext, q.stats, q.sorted, q.proj,
                               (int32_t)q.lds, q.most, q.needs_list, (int32_t)q.status, (int32_t)q.ext_refusal};
        memcpy(out16 + 16 * i, o, sizeof o);
        refusal[i] = (int32_t)b.refusal;
    }
    return CHUNKY_OK;
}

extern "C" int chunky_selftest_camera_rays(chunky_render* r, int32_t seed, float* out, int64_t n_floats) {
    if (r && !r->parts.empty()) return chunky_selftest_camera_rays(r->parts[0], seed, out, n_floats);
    LOCK_RENDER(r);
    if (!r->have_camera || r->cam.projector_type <= 0) return fail(CHUNKY_E_STATE, "selftest_camera_rays: the target has no projected camera");
    const int64_t need = (int64_t)r->width * r->height * 6;
    if (!out || n_floats != need) return fail(CHUNKY_E_INVALID, "selftest_camera_rays: need %lld floats, got %lld", (long long)need, (long long)n_floats);
    DevBuf dout;
    HIP_TRY(hipMalloc(&dout.p, (size_t)need * 4));
    HIP_TRY(launch_camera_rays_selftest(r->cam, seed, (float*)dout.p, r->ctx->stream));
    HIP_TRY(hipMemcpyAsync(out, dout.p, (size_t)need * 4, hipMemcpyDeviceToHost, r->ctx->stream));
    HIP_TRY(hipStreamSynchronize(r->ctx->stream));
    return CHUNKY_OK;
}

// the view comes from make_shard_view, as chunky_render_set_shard's does: the test sees what a render would see
extern "C" int chunky_selftest_shard_map(chunky_ctx* ctx, int mode, int width, int height, int rank, int world, int tile, int n,
                                         const uint32_t* pairs, int32_t* out, int32_t view_out[4]) {
    if (!ctx) return fail(CHUNKY_E_INVALID, "NULL context");
    if (!ctx->members.empty()) ctx = ctx->members[0];
    if (mode != 0 && mode != 1) return fail(CHUNKY_E_INVALID, "selftest_shard_map: mode %d", mode);
    if (n < 0 || n > (1 << 24) || (n > 0 && !out) || (mode == 1 && n > 0 && !pairs)) return fail(CHUNKY_E_INVALID, "selftest_shard_map: bad arguments");
    ShardView T{0, 1, 256, 0};
    if (mode == 0) {
        if (width <= 0 || height <= 0 || (int64_t)width * height > (1 << 30)) return fail(CHUNKY_E_INVALID, "bad image size %dx%d", width, height);
        if (world < 1 || rank < 0 || rank >= world || tile < 0) return fail(CHUNKY_E_INVALID, "set_shard: rank %d / world %d / tile %d", rank, world, tile);
        if (!make_shard_view(width, height, rank, world, tile, &T)) return fail(CHUNKY_E_INVALID, "selftest_shard_map: the share needs more than 2^31 pixel slots");
        // a block share maps slot -> block (slot / 256) * world + rank before it looks at n_local: only slot counts that keep that an int
        if (T.world != 1 && T.tile == 0 && n > 0 && (int64_t)((n - 1) >> 8) * T.world + T.rank > INT_MAX)
            return fail(CHUNKY_E_INVALID, "selftest_shard_map: %d slots of a block share of %d ranks leave the range of an int", n, world);
        if (view_out) {
            view_out[0] = T.rank; view_out[1] = T.world; view_out[2] = T.tile; view_out[3] = T.n_local;
        }
    }
    if (n == 0) return CHUNKY_OK;
    std::lock_guard<std::recursive_mutex> g(ctx->mu);
    HIP_TRY(hipSetDevice(ctx->device));
    DevBuf din, dout;
    const size_t out_bytes = (size_t)n * (mode == 0 ? 5 : 1) * 4;
    std::vector<uint32_t> triples;
    if (mode == 1) {  // (a, d) -> (a, m, s): the pair of the divisor made here, on the host, as launch_pool makes a launch's
        triples.resize((size_t)n * 3);
        for (int i = 0; i < n; i++) {
            const FastDiv f = fast_div(pairs[2 * (size_t)i + 1]);
            triples[3 * (size_t)i] = pairs[2 * (size_t)i];
            triples[3 * (size_t)i + 1] = f.m;
            triples[3 * (size_t)i + 2] = (uint32_t)f.s;
        }
        HIP_TRY(din.upload(triples.data(), triples.size() * 4, ctx->stream));
    }
    HIP_TRY(hipMalloc(&dout.p, out_bytes));
    HIP_TRY(launch_shard_map_selftest(mode, T, width, height, n, (const unsigned*)din.p, (int*)dout.p, ctx->stream));
    HIP_TRY(hipMemcpyAsync(out, dout.p, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return CHUNKY_OK;
}

extern "C" int chunky_selftest_helpers(chunky_scene* scene, int which, int tree, int n, const float* in, float* out, int32_t* tree_used) {
    if (scene && !scene->replicas.empty()) return chunky_selftest_helpers(scene->replicas[0], which, tree, n, in, out, tree_used);
    LOCK_SCENE(scene);
    if (n < 0 || (n > 0 && (!in || !out))) return fail(CHUNKY_E_INVALID, "selftest_helpers: bad arguments");
    if (n == 0) return CHUNKY_OK;
    SceneView S;
    if (int rc = scene_view(scene, &S)) return rc;
    DevBuf din, dout;
    hipStream_t st = scene->ctx->stream;
    HIP_TRY(din.upload(in, (size_t)n * 32 * sizeof(float), st));
    HIP_TRY(hipMalloc(&dout.p, (size_t)n * 12 * sizeof(float)));
    int used = 0;
    HIP_TRY(launch_helpers_selftest(S, which, tree, n, (const float*)din.p, (float*)dout.p, &used, st));
    HIP_TRY(hipMemcpyAsync(out, dout.p, (size_t)n * 12 * sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (tree_used) *tree_used = used;
    return CHUNKY_OK;
}

extern "C" int chunky_selftest_gamma_scan(chunky_ctx* ctx, int curve, uint32_t first_bits, uint64_t count, uint64_t* mismatches, float* worst_estimate) {
    if (!ctx || !mismatches) return fail(CHUNKY_E_INVALID, "selftest_gamma_scan: NULL argument");
    if (!ctx->members.empty()) ctx = ctx->members[0];
    if (count > (1ull << 32) || (curve != 0 && curve != 2)) return fail(CHUNKY_E_INVALID, "selftest_gamma_scan: curve=%d count=%llu", curve, (unsigned long long)count);
    std::lock_guard<std::recursive_mutex> g(ctx->mu);
    HIP_TRY(hipSetDevice(ctx->device));
    const float* table = nullptr;
    if (int rc = device_gamma_table(ctx, &table)) return rc;
    DevBuf out;
    HIP_TRY(hipMalloc(&out.p, 16));
    HIP_TRY(hipMemsetAsync(out.p, 0, 16, ctx->stream));
    HIP_TRY(launch_gamma_scan(first_bits, count, curve, table, (unsigned long long*)out.p, (float*)((char*)out.p + 8), ctx->stream));
    unsigned char host[16];
    HIP_TRY(hipMemcpyAsync(host, out.p, 16, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    memcpy(mismatches, host, 8);
    if (worst_estimate) memcpy(worst_estimate, host + 8, 4);
    return CHUNKY_OK;
}
