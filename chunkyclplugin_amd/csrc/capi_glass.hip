// capi_glass.hip — translucent blocks on a render target (include/chunky_hip.h, "translucent blocks"): setting and
// reading them, and the answers of the calls that have no glass kernels.  What needs no device is glass_host.cpp; the launch is
// chunky_render_passes' (capi_render.hip), the kernels are render_pool_glass.hip and render_pool_glass_bvh.hip.
#include "capi_internal.hpp"

extern "C" int chunky_render_set_translucency(chunky_render* r, const chunky_translucency* t) {
    if (r && !r->parts.empty()) {
        // every member or none: the check does not depend on the member, so it is made first, once
        std::lock_guard<std::recursive_mutex> g(r->ctx->mu);
        if (int rc = check_translucency("set_translucency", t, nullptr)) return rc;
        return each_part(r, [&](chunky_render* m_) { return chunky_render_set_translucency(m_, t); });
    }
    LOCK_RENDER(r);
    GlassSettings s;
    if (int rc = check_translucency("set_translucency", t, &s)) return rc;
    r->glass = s;  // (the parameters travel by value in the kernel arguments: launches already queued keep the ones they had)
    r->ad_resumable = false;  // what a pass renders changes: an adaptive run cannot continue across it
    return CHUNKY_OK;
}

extern "C" int chunky_render_translucency(chunky_render* r, chunky_translucency* out, int* enabled) {
    if (r && !r->parts.empty()) {
        std::lock_guard<std::recursive_mutex> g(r->ctx->mu);
        return chunky_render_translucency(r->parts[0], out, enabled);
    }
    LOCK_RENDER(r);
    if (!out) return fail(CHUNKY_E_INVALID, "render_translucency: NULL output");
    chunky_translucency t{};
    t.size = sizeof t;
    t.opaque_alpha = r->glass.opaque_alpha;
    t.max_crossings = r->glass.max_crossings;
    *out = t;
    if (enabled) *enabled = r->glass.on() ? 1 : 0;
    return CHUNKY_OK;
}

bool glass_params_of(const chunky_render* r, GlassParams* G) {
    if (!r->glass.on()) return false;
    if (G) {
        *G = GlassParams{};
        G->opaque_alpha = r->glass.opaque_alpha, G->max_crossings = r->glass.max_crossings;
    }
    return true;
}

// A call whose images hold light and whose kernels treat every hit as opaque refuses a target with translucency on: it never renders
// opaque glass
int refuse_glass(const char* who, const chunky_render* r) {
    if (!r->glass.on()) return CHUNKY_OK;
    return fail(CHUNKY_E_STATE, "%s: not supported with translucent blocks (chunky_render_set_translucency); turn translucency off (NULL) for this call", who);
}

GlassPlan glass_plan(const chunky_render* r, const SceneView& S) {
    return plan_glass(r->kernel_variant, scene_facts(S), r->opts, r->cam.projector_type, r->shard, 0, r->work_counter.p != nullptr, false, biome_map(r, nullptr),
                      r->fog.on());
}
