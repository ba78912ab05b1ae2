// capi_scene.hip — scene upload (the C++ counterpart of J/opencl/renderer/ClSceneLoader.java) and the kernel-side view of a scene.
#include "capi_internal.hpp"

// placement of the entity-BVH records (scene_records.cpp relayout_bvh_records): records in the breadth-first top, records per treelet; 0 = off
#ifndef CHUNKY_BVH_TOP_RECORDS
#define CHUNKY_BVH_TOP_RECORDS 0
#endif
#ifndef CHUNKY_BVH_TREELET_RECORDS
#define CHUNKY_BVH_TREELET_RECORDS 0
#endif
// top / treelet sizes of relayout_bvh_records; CHUNKY_BVH_LAYOUT="top,treelet" overrides them for tuning runs ("0,0" = the
// plain depth-first order of round 2)
static void bvh_layout_params(int* top, int* treelet) {
    *top = CHUNKY_BVH_TOP_RECORDS;
    *treelet = CHUNKY_BVH_TREELET_RECORDS;
#ifdef CHUNKY_TUNING
    if (const char* e = getenv("CHUNKY_BVH_LAYOUT")) {
        int a = 0, b = 0;
        if (sscanf(e, "%d,%d", &a, &b) == 2 && a >= 0 && b >= 0) {
            *top = a;
            *treelet = b;
        }
    }
#endif
}

extern "C" int chunky_scene_create(chunky_ctx* ctx, chunky_scene** out) {
    if (!ctx || !out) return fail(CHUNKY_E_INVALID, "chunky_scene_create: NULL argument");
    std::unique_ptr<chunky_scene> s(new chunky_scene);
    s->ctx = ctx;
    for (chunky_ctx* m : ctx->members) {  // a group: one replica per member
        chunky_scene* rep = nullptr;
        if (int rc = chunky_scene_create(m, &rep)) {
            for (chunky_scene* r : s->replicas) (void)chunky_scene_destroy(r);
            return rc;
        }
        s->replicas.push_back(rep);
    }
    *out = s.release();
    return CHUNKY_OK;
}

void scene_unref(chunky_scene* s) {
    if (--s->refs == 0) delete s;
}

extern "C" int chunky_scene_destroy(chunky_scene* scene) {
    if (scene && !scene->replicas.empty()) {
        const int rc = each_replica(scene, [&](chunky_scene* m_) { return chunky_scene_destroy(m_); });
        std::lock_guard<std::recursive_mutex> g(scene->ctx->mu);
        scene->replicas.clear();
        scene_unref(scene);  // render targets of the group keep the (now empty) shell alive until they are destroyed
        return rc;
    }
    LOCK_SCENE(scene);
    (void)hipStreamSynchronize(scene->ctx->stream);
    scene_unref(scene);
    return CHUNKY_OK;
}

extern "C" int chunky_scene_set_octree(chunky_scene* scene, const int32_t* tree, int64_t n, int depth) {
    FAN_SCENE(scene, chunky_scene_set_octree(m_, tree, n, depth));
    LOCK_SCENE(scene);
    if (int rc = check_ints(tree, n, "set_octree")) return rc;
    if (n < 1) return fail(CHUNKY_E_INVALID, "set_octree: empty tree");
    if (depth < 0 || depth > 30) return fail(CHUNKY_E_INVALID, "set_octree: depth %d out of range", depth);
    // every branch value must address a whole 8-int child group inside the array (K/octree.h:83-87)
    for (int64_t i = 0; i < n; i++) {
        int32_t v = tree[i];
        if (v > 0 && (int64_t)v + 8 > n) return fail(CHUNKY_E_INVALID, "set_octree: node %lld points outside the tree", (long long)i);
    }
    HIP_TRY(scene->octree.upload(tree, (size_t)n * 4, scene->ctx->stream));
    scene->octree_depth = depth;
    scene->host_octree.assign(tree, tree + n);
    scene->emitters_dirty = true;
    // wide re-layout for the fast lookup; scenes it cannot express keep the reference layout only
    scene->wide.release();
    scene->wide_meta = WideTree();
    int bits[kWideMaxLevels];
    int nlev = default_wide_levels(depth, bits);
#ifdef CHUNKY_TUNING
    if (const char* e = getenv("CHUNKY_DEBUG_WIDE_BITS")) {  // experiments: another split, e.g. "4,3,2" (16^3 top node)
        nlev = 0;
        for (const char* q = e; *q && nlev < kWideMaxLevels;) {
            bits[nlev++] = atoi(q);
            while (*q && *q != ',') q++;
            if (*q == ',') q++;
        }
    }
#endif
    const char* why = "";
    WideTree wt;
    if (build_wide_tree(tree, n, depth, bits, nlev, &wt, &why)) {
        scene->wide_meta = std::move(wt);
        scene->wide_dirty = true;  // annotated + uploaded by scene_view once the block palette is known
    }
    return CHUNKY_OK;
}

extern "C" int chunky_scene_load_octree(chunky_scene* scene, const int32_t* tree_data, int64_t n, int depth,
                                        const int32_t* block_mapping, int64_t n_mapping) {
    if (int rc = check_ints(tree_data, n, "load_octree")) return rc;
    if (int rc = check_ints(block_mapping, n_mapping, "load_octree mapping")) return rc;
    std::vector<int32_t> mapped((size_t)n);
    for (int64_t i = 0; i < n; i++) {  // ClSceneLoader.java:56-58
        int32_t v = tree_data[i];
        mapped[(size_t)i] = (v > 0 || -(int64_t)v >= n_mapping) ? v : -block_mapping[-v];
    }
    return chunky_scene_set_octree(scene, mapped.data(), n, depth);
}

extern "C" int chunky_scene_set_palette(chunky_scene* scene, int kind, const int32_t* data, int64_t n) {
    FAN_SCENE(scene, chunky_scene_set_palette(m_, kind, data, n));
    LOCK_SCENE(scene);
    if (int rc = check_ints(data, n, "set_palette")) return rc;
    DevBuf* dst = nullptr;
    switch (kind) {
        case CHUNKY_PALETTE_BLOCK: dst = &scene->blocks; break;
        case CHUNKY_PALETTE_MATERIAL: dst = &scene->materials; break;
        case CHUNKY_PALETTE_AABB: dst = &scene->aabbs; break;
        case CHUNKY_PALETTE_QUAD: dst = &scene->quads; break;
        case CHUNKY_PALETTE_TRIG: dst = &scene->trigs; break;
        default: return fail(CHUNKY_E_INVALID, "set_palette: unknown kind %d", kind);
    }
    HIP_TRY(dst->upload(data, (size_t)n * 4, scene->ctx->stream));
    switch (kind) {
        case CHUNKY_PALETTE_BLOCK: scene->host_blocks.assign(data, data + n); scene->wide_dirty = true; break;
        case CHUNKY_PALETTE_MATERIAL: scene->host_materials.assign(data, data + n); break;
        case CHUNKY_PALETTE_AABB: scene->host_aabbs.assign(data, data + n); break;
        case CHUNKY_PALETTE_QUAD: scene->host_quads.assign(data, data + n); break;
        case CHUNKY_PALETTE_TRIG: scene->host_trigs.assign(data, data + n); break;
        default: break;
    }
    if (kind != CHUNKY_PALETTE_TRIG) scene->derived_dirty = true;  // rebuilt by scene_view before the next launch
    if (kind == CHUNKY_PALETTE_BLOCK || kind == CHUNKY_PALETTE_MATERIAL) scene->emitters_dirty = true;
    if (kind == CHUNKY_PALETTE_TRIG || kind == CHUNKY_PALETTE_MATERIAL) scene->bvh_dirty = true;
    return CHUNKY_OK;
}

extern "C" int chunky_scene_set_bvh(chunky_scene* scene, int which, const int32_t* nodes, int64_t n) {
    FAN_SCENE(scene, chunky_scene_set_bvh(m_, which, nodes, n));
    LOCK_SCENE(scene);
    if (int rc = check_ints(nodes, n, "set_bvh")) return rc;
    if (which != CHUNKY_BVH_WORLD && which != CHUNKY_BVH_ACTOR) return fail(CHUNKY_E_INVALID, "set_bvh: which=%d", which);
    if (n < 7) return fail(CHUNKY_E_INVALID, "set_bvh: a BVH has at least one 7-int node (got %lld ints)", (long long)n);
    bool empty = nodes[0] == 0;  // K/bvh.h:23-32
    for (int k = 1; k <= 6 && empty; k++) {
        float f;
        memcpy(&f, &nodes[k], 4);
        empty = f != f;
    }
    // a malformed BVH would hang the traversal; the height bounds the to-visit stack
    std::vector<int32_t> host(nodes, nodes + n);
    int height = 0;
    if (!empty && !bvh_links_height(host, &height))
        return fail(CHUNKY_E_INVALID, "set_bvh: node link outside the array or cyclic, or a tree deeper than the reference's 64-entry stack");
    (which == CHUNKY_BVH_WORLD ? scene->world_height : scene->actor_height) = height;
    DevBuf& dst = which == CHUNKY_BVH_WORLD ? scene->world_bvh : scene->actor_bvh;
    HIP_TRY(dst.upload(nodes, (size_t)n * 4, scene->ctx->stream));
    (which == CHUNKY_BVH_WORLD ? scene->host_world_bvh : scene->host_actor_bvh).swap(host);
    scene->bvh_dirty = true;
    if (which == CHUNKY_BVH_WORLD) {
        scene->world_empty = empty;
        scene->have_world = true;
    } else {
        scene->actor_empty = empty;
        scene->have_actor = true;
    }
    return CHUNKY_OK;
}

extern "C" int chunky_scene_set_atlas(chunky_scene* scene, const uint8_t* rgba, int w, int h, int layers) {
    FAN_SCENE(scene, chunky_scene_set_atlas(m_, rgba, w, h, layers));
    LOCK_SCENE(scene);
    if (w <= 0 || h <= 0 || layers <= 0) return fail(CHUNKY_E_INVALID, "set_atlas: bad size %dx%dx%d", w, h, layers);
    size_t bytes = (size_t)w * h * layers * 4;
    if (rgba) {
        HIP_TRY(scene->atlas.upload(rgba, bytes, scene->ctx->stream));
    } else {
        HIP_TRY(scene->atlas.alloc(bytes));
        HIP_TRY(hipMemsetAsync(scene->atlas.p, 0, bytes, scene->ctx->stream));
        HIP_TRY(hipStreamSynchronize(scene->ctx->stream));
    }
    scene->atlas_w = w;
    scene->atlas_h = h;
    scene->atlas_layers = layers;
    return CHUNKY_OK;
}

extern "C" int chunky_scene_write_atlas_tile(chunky_scene* scene, int x, int y, int layer, int w, int h,
                                             const uint8_t* rgba) {
    FAN_SCENE(scene, chunky_scene_write_atlas_tile(m_, x, y, layer, w, h, rgba));
    LOCK_SCENE(scene);
    if (!scene->atlas.p) return fail(CHUNKY_E_STATE, "write_atlas_tile before set_atlas");
    if (!rgba || x < 0 || y < 0 || layer < 0 || w <= 0 || h <= 0 || x + w > scene->atlas_w || y + h > scene->atlas_h ||
        layer >= scene->atlas_layers)
        return fail(CHUNKY_E_INVALID, "write_atlas_tile: region outside the atlas");
    char* base = (char*)scene->atlas.p + (((size_t)layer * scene->atlas_h + y) * scene->atlas_w + x) * 4;
    HIP_TRY(hipMemcpy2DAsync(base, (size_t)scene->atlas_w * 4, rgba, (size_t)w * 4, (size_t)w * 4, h,
                             hipMemcpyHostToDevice, scene->ctx->stream));
    HIP_TRY(hipStreamSynchronize(scene->ctx->stream));
    return CHUNKY_OK;
}

extern "C" int chunky_scene_set_sky(chunky_scene* scene, const uint8_t* rgba, int w, int h, float intensity) {
    FAN_SCENE(scene, chunky_scene_set_sky(m_, rgba, w, h, intensity));
    LOCK_SCENE(scene);
    if (!rgba || w <= 0 || h <= 0) return fail(CHUNKY_E_INVALID, "set_sky: bad texture");
    // texels are converted once here with the same rt_unorm8 the kernels would apply per sample
    std::vector<float> texels((size_t)w * h * 4);
    for (size_t i = 0; i < texels.size(); i++) texels[i] = rt_unorm8(rgba[i]);
    HIP_TRY(scene->sky.upload(texels.data(), texels.size() * 4, scene->ctx->stream));
    scene->sky_w = w;
    scene->sky_h = h;
    scene->sky_intensity = intensity;
    return CHUNKY_OK;
}

// The emitter list exists only for CHUNKY_OPT_EMITTER_NEE and chunky_scene_emitters: built on first use after a change.
static int refresh_emitters(chunky_scene* s) {
    if (!s->emitters_dirty) return CHUNKY_OK;
    HIP_TRY(hipStreamSynchronize(s->ctx->stream));  // queued passes may still read the old list
    list_emitters(s->host_octree, s->octree_depth, s->host_blocks, s->host_materials, &s->host_emitters);
    s->emitters.release();
    if (!s->host_emitters.empty()) HIP_TRY(s->emitters.upload(s->host_emitters.data(), s->host_emitters.size() * 4, s->ctx->stream));
    s->emitters_dirty = false;
    return CHUNKY_OK;
}
extern "C" int chunky_scene_emitters(chunky_scene* scene, int32_t* out4, int32_t cap, int32_t* count) {
    if (scene && !scene->replicas.empty()) return chunky_scene_emitters(scene->replicas[0], out4, cap, count);  // replicas agree
    LOCK_SCENE(scene);
    if (!count || cap < 0 || (cap > 0 && !out4)) return fail(CHUNKY_E_INVALID, "scene_emitters: bad arguments");
    if (int rc = refresh_emitters(scene)) return rc;
    const int32_t n = (int32_t)(scene->host_emitters.size() / 4);
    *count = n;
    const int32_t give = n < cap ? n : cap;
    if (out4 && give > 0) memcpy(out4, scene->host_emitters.data(), (size_t)give * 16);
    return CHUNKY_OK;
}

extern "C" int chunky_scene_set_sun(chunky_scene* scene, const int32_t sun[6]) {
    FAN_SCENE(scene, chunky_scene_set_sun(m_, sun));
    LOCK_SCENE(scene);
    if (!sun) return fail(CHUNKY_E_INVALID, "set_sun: NULL");
    memcpy(scene->sun, sun, sizeof scene->sun);
    scene->have_sun = true;
    return CHUNKY_OK;
}

extern "C" int chunky_scene_set_biome_tints(chunky_scene* scene, const int32_t* rgb3, int x0, int z0, int size_x, int size_z) {
    FAN_SCENE(scene, chunky_scene_set_biome_tints(m_, rgb3, x0, z0, size_x, size_z));
    LOCK_SCENE(scene);
    if (size_x < 0 || size_z < 0) return fail(CHUNKY_E_INVALID, "set_biome_tints: negative size %d x %d", size_x, size_z);
    if ((size_x == 0) != (size_z == 0)) return fail(CHUNKY_E_INVALID, "set_biome_tints: size %d x %d (both 0 removes the map)", size_x, size_z);
    if ((rgb3 == nullptr) != (size_x == 0)) return fail(CHUNKY_E_INVALID, "set_biome_tints: NULL colours go with size 0 x 0 and only with it");
    if ((int64_t)size_x * size_z > CHUNKY_BIOME_MAX_CELLS)
        return fail(CHUNKY_E_INVALID, "set_biome_tints: %d x %d cells, at most %d", size_x, size_z, (int)CHUNKY_BIOME_MAX_CELLS);
    if (!rgb3) {
        HIP_TRY(hipStreamSynchronize(scene->ctx->stream));  // queued launches may still read the map
        scene->biome.release();
        scene->biome_x0 = scene->biome_z0 = scene->biome_size_x = scene->biome_size_z = 0;
        return CHUNKY_OK;
    }
    // (in stream order behind the launches that read the old map; the host array is the caller's again on return: DevBuf::upload)
    HIP_TRY(scene->biome.upload(rgb3, (size_t)size_x * size_z * 3 * sizeof(int32_t), scene->ctx->stream));
    scene->biome_x0 = x0, scene->biome_z0 = z0, scene->biome_size_x = size_x, scene->biome_size_z = size_z;
    return CHUNKY_OK;
}

static int rebuild_derived(chunky_scene* s) {
    const std::vector<int32_t>&B = s->host_blocks, &M = s->host_materials, &A = s->host_aabbs, &Q = s->host_quads;
    hipStream_t st = s->ctx->stream;
    HIP_TRY(hipStreamSynchronize(st));  // queued passes may still read the old copies
    s->block_info.release();
    s->quad_aux.release();
    s->mat8.release();
    s->aabb_rec.release();
    s->quad_rec.release();
    s->derived_dirty = false;
    // (also for an empty block or material palette: block_info then exists with every block marked as one that never hits — a
    // cube's material would lie outside the palette — and render_pool's sorted block tests rely on its existence)
    DerivedRecords d;
    derive_records(B, M, A, Q, &d);
    HIP_TRY(s->block_info.upload(d.info.data(), d.info.size() * 4, st));
    HIP_TRY(s->mat8.upload(d.mat8.data(), d.mat8.size() * 4, st));
    if (!d.aabb_rec.empty()) HIP_TRY(s->aabb_rec.upload(d.aabb_rec.data(), d.aabb_rec.size() * 4, st));
    if (!d.quad_rec.empty()) HIP_TRY(s->quad_rec.upload(d.quad_rec.data(), d.quad_rec.size() * 4, st));
    std::vector<float> aux;  // for quads that kept the packed path
    if (build_quad_aux(B, Q, &aux)) HIP_TRY(s->quad_aux.upload(aux.data(), aux.size() * 4, st));
    return CHUNKY_OK;
}

// Assemble the kernel-side view; Sun_new (K/sky.h:19-40) is evaluated here, on the host, with the
// same rt_math.h the device uses.
int scene_view(chunky_scene* s, SceneView* v, bool want_emitters) {
    if (!s->octree.p || s->octree_depth < 0) return fail(CHUNKY_E_STATE, "scene has no octree");
    if (!s->blocks.p || !s->materials.p) return fail(CHUNKY_E_STATE, "scene has no block/material palette");
    if (!s->atlas.p) return fail(CHUNKY_E_STATE, "scene has no texture atlas");
    if (!s->sky.p) return fail(CHUNKY_E_STATE, "scene has no sky texture");
    if (!s->have_sun) return fail(CHUNKY_E_STATE, "scene has no sun");
    if ((!s->world_empty || !s->actor_empty) && !s->trigs.p) return fail(CHUNKY_E_STATE, "scene has a BVH but no triangles");
    v->octree = (const int*)s->octree.p;
    v->blocks = (const int*)s->blocks.p;
    v->quads = (const int*)s->quads.p;
    v->aabbs = (const int*)s->aabbs.p;
    v->world_bvh = (const int*)s->world_bvh.p;
    v->actor_bvh = (const int*)s->actor_bvh.p;
    v->trigs = (const int*)s->trigs.p;
    v->atlas = (const uint32_t*)s->atlas.p;
    v->materials = (const int*)s->materials.p;
    v->sky = (const float4*)s->sky.p;
    v->octree_depth = s->octree_depth;
    v->atlas_w = s->atlas_w;
    v->atlas_h = s->atlas_h;
    v->atlas_layers = s->atlas_layers;
    v->sky_w = s->sky_w;
    v->sky_h = s->sky_h;
    v->sky_intensity = s->sky_intensity;
    v->sun_flags = s->sun[0];
    v->sun_tex_size = s->sun[1];
    v->sun_tex = s->sun[2];
    v->sun_intensity = bits_to_float(s->sun[3]);
    float phi = bits_to_float(s->sun[4]), theta = bits_to_float(s->sun[5]);
    float r = rt_fabs(rt_cos(phi));
    float swx = rt_cos(theta) * r, swy = rt_sin(phi), swz = rt_sin(theta) * r;
    float sux = 1, suy = 0, suz = 0;
    if (rt_fabs(swx) > 0.1f) {
        sux = 0;
        suy = 1;
    }
    // sv = normalize(cross(sw, su)); su = cross(sv, sw)
    float cx = rt_cross_c(swy, suz, swz, suy), cy = rt_cross_c(swz, sux, swx, suz), cz = rt_cross_c(swx, suy, swy, sux);
    float rl = rt_rlen3(cx, cy, cz);
    float svx = cx * rl, svy = cy * rl, svz = cz * rl;
    v->sw = f3{swx, swy, swz};
    v->sv = f3{svx, svy, svz};
    v->su = f3{rt_cross_c(svy, swz, svz, swy), rt_cross_c(svz, swx, svx, swz), rt_cross_c(svx, swy, svy, swx)};
    v->sun_radius_cos = rt_cos(0.03f);
    v->bvh_cull = 0;  // a render target's option: set by its launch sites
    v->world_bvh_empty = (s->world_empty || !s->world_bvh.p) ? 1 : 0;
    v->actor_bvh_empty = (s->actor_empty || !s->actor_bvh.p) ? 1 : 0;
    if (s->wide_dirty && s->wide_meta.nlev > 0) {
        annotate_wide_tree(&s->wide_meta, s->host_blocks.data(), (int64_t)s->host_blocks.size());
        s->model_leaf_permille = model_leaf_permille(s->host_octree, s->host_blocks);
        HIP_TRY(hipStreamSynchronize(s->ctx->stream));  // queued passes may still read the old copy
        HIP_TRY(s->wide.upload(s->wide_meta.data.data(), s->wide_meta.data.size() * 4, s->ctx->stream));
        s->wide_dirty = false;
    }
    if (s->derived_dirty)
        if (int rc = rebuild_derived(s)) return rc;
    if (s->bvh_dirty) {
        HIP_TRY(hipStreamSynchronize(s->ctx->stream));
        s->bvh_rec.release();
        s->tri_off = 0;
        if (!bvh_leaves_sound(s->host_world_bvh, s->world_empty, s->host_trigs, s->host_materials) ||
            !bvh_leaves_sound(s->host_actor_bvh, s->actor_empty, s->host_trigs, s->host_materials))
            return fail(CHUNKY_E_INVALID, "an entity BVH leaf or a triangle's material lies outside its palette");
        std::vector<int32_t> nodes, tris;
        int top = 0, treelet = 0;  // where the records sit (addresses only: the walk's order, tests and arithmetic do not see it)
        bvh_layout_params(&top, &treelet);
        if ((!s->world_empty || !s->actor_empty) &&
            build_bvh_records(s->host_world_bvh, s->world_empty, s->host_actor_bvh, s->actor_empty, s->host_trigs, s->host_materials, top, treelet,
                              &nodes, &tris, &s->world_root, &s->actor_root)) {
            if (nodes.empty()) nodes.resize(16, 0);  // both roots are leaves
            tris.resize(tris.size() + 20, 0);        // a step at the end of the last leaf reads one record past it
            // ONE allocation — nodes, then triangles — so the walk addresses either kind of record as a 32-bit byte offset off
            // one scalar base (a walk longer than 2 GiB of records keeps the packed arrays: build_bvh_records' index limits)
            s->tri_off = nodes.size() * 4;
            nodes.insert(nodes.end(), tris.begin(), tris.end());
            HIP_TRY(s->bvh_rec.upload(nodes.data(), nodes.size() * 4, s->ctx->stream));
        }
        s->bvh_dirty = false;
    }
    if (want_emitters)
        if (int rc = refresh_emitters(s)) return rc;
    v->emitters = want_emitters ? (const int4*)s->emitters.p : nullptr;
    v->n_emitters = want_emitters ? (int)(s->host_emitters.size() / 4) : 0;
    v->n_block_ints = (int)(s->host_blocks.size() < 0x7FFFFFFFu ? s->host_blocks.size() : 0x7FFFFFFFu);
    v->sort_blocks = s->model_leaf_permille >= kSortBlocksPermille ? 1 : 0;
    v->bvh_rec = (const int4*)s->bvh_rec.p;
    v->tri_rec = s->bvh_rec.p ? (const int4*)((const char*)s->bvh_rec.p + s->tri_off) : nullptr;
    v->tri_off = (unsigned)s->tri_off;
    v->world_root = s->world_root;
    v->actor_root = s->actor_root;
    v->quad_aux = (const float*)s->quad_aux.p;
    v->bvh_stack_entries = (s->world_height > s->actor_height ? s->world_height : s->actor_height) + 1;
    v->block_info = (const int4*)s->block_info.p;
    v->mat8 = (const int4*)s->mat8.p;
    v->aabb_rec = (const int4*)s->aabb_rec.p;
    v->quad_rec = (const int4*)s->quad_rec.p;
    {
        // which arrays kernels may address by 32-bit offsets (addr32.h): the sizes as they stand now, the derived arrays rebuilt above
        AddrBounds b;
        b.atlas_w = s->atlas_w, b.atlas_h = s->atlas_h, b.atlas_layers = s->atlas_layers, b.sky_w = s->sky_w, b.sky_h = s->sky_h;
        b.aabb_rec_bytes = s->aabb_rec.bytes, b.quad_rec_bytes = s->quad_rec.bytes;
        b.indices_checked = !s->derived_dirty && s->block_info.p != nullptr;
        v->addr32 = addr32_word(b);
#ifdef CHUNKY_TUNING
        if (const char* e = getenv("CHUNKY_ADDR32_MASK")) v->addr32 &= (unsigned)atoi(e);  // tests/test_gpu_addr32_parity.py: 0 = as a scene too large for the 32-bit forms
#endif
    }
    v->wide = s->wide_meta.nlev > 0 ? (const uint32_t*)s->wide.p : nullptr;
    v->wide_nlev = s->wide_meta.nlev;
    // (annotated above whenever the octree or the block palette changed; with no wide tree the world's own top: nothing is capped)
    v->hit_top = s->wide_meta.nlev > 0 ? s->wide_meta.hit_top : (int)(1u << (s->octree_depth < 31 ? s->octree_depth : 30));
    for (int i = 0; i < 6; i++) {
        v->wide_shift[i] = s->wide_meta.shift[i];
        v->wide_bits[i] = s->wide_meta.bits[i];
    }
    return CHUNKY_OK;
}

extern "C" int chunky_scene_hit_top(chunky_scene* scene, int32_t* hit_top) {
    if (scene && !scene->replicas.empty()) return chunky_scene_hit_top(scene->replicas[0], hit_top);  // replicas agree
    LOCK_SCENE(scene);
    if (!hit_top) return fail(CHUNKY_E_INVALID, "scene_hit_top: NULL");
    SceneView v;
    if (int rc = scene_view(scene, &v, false)) return rc;
    *hit_top = v.hit_top;
    return CHUNKY_OK;
}

extern "C" int chunky_scene_addr32(chunky_scene* scene, uint32_t* word) {
    if (scene && !scene->replicas.empty()) return chunky_scene_addr32(scene->replicas[0], word);  // replicas agree
    LOCK_SCENE(scene);
    if (!word) return fail(CHUNKY_E_INVALID, "scene_addr32: NULL");
    SceneView v;
    if (int rc = scene_view(scene, &v, false)) return rc;
    *word = v.addr32;
    return CHUNKY_OK;
}
