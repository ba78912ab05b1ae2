// capi_fog.hip — the ground-fog layer of a render target (include/chunky_hip.h, "ground fog"): setting and
// reading it, and the answers of the calls that have no fog kernels.  What needs no device is fog_host.cpp; the launch is
// chunky_render_passes' (capi_render.hip), the kernels are render_pool_fog.hip and render_pool_fog_bvh.hip.
#include "capi_internal.hpp"

extern "C" int chunky_render_set_fog(chunky_render* r, const chunky_fog* fog) {
    if (r && !r->parts.empty()) {
        // every member or none: the check does not depend on the member, so it is made first, once
        std::lock_guard<std::recursive_mutex> g(r->ctx->mu);
        if (int rc = check_fog("set_fog", fog, nullptr)) return rc;
        return each_part(r, [&](chunky_render* m_) { return chunky_render_set_fog(m_, fog); });
    }
    LOCK_RENDER(r);
    FogSettings s;
    if (int rc = check_fog("set_fog", fog, &s)) return rc;
    if (s.on())  // (a layer, not "off": the glass kernels have no medium)
        if (int rc = refuse_glass("set_fog", r)) return rc;
    r->fog = s;  // (the layer travels by value in the kernel arguments: launches already queued keep the one they had)
    r->ad_resumable = false;  // what a pass renders changes: an adaptive run cannot continue across it
    return CHUNKY_OK;
}

extern "C" int chunky_render_fog(chunky_render* r, chunky_fog* out) {
    if (r && !r->parts.empty()) {
        std::lock_guard<std::recursive_mutex> g(r->ctx->mu);
        return chunky_render_fog(r->parts[0], out);
    }
    LOCK_RENDER(r);
    if (!out) return fail(CHUNKY_E_INVALID, "render_fog: NULL output");
    chunky_fog f{};
    f.size = sizeof f;
    f.density = r->fog.density, f.y_min = r->fog.y_min, f.y_max = r->fog.y_max;
    for (int k = 0; k < 3; k++) f.color[k] = r->fog.color[k];
    *out = f;
    return CHUNKY_OK;
}

bool fog_params_of(const chunky_render* r, FogParams* F) {
    if (!r->fog.on()) return false;
    if (F) {
        *F = FogParams{};
        F->sigma = r->fog.density, F->y_min = r->fog.y_min, F->y_max = r->fog.y_max;
        for (int k = 0; k < 3; k++) F->color[k] = r->fog.color[k];
    }
    return true;
}

// A call whose images hold light and whose kernels have no medium refuses a target with a fog layer: it never renders clear air
int refuse_fog(const char* who, const chunky_render* r) {
    if (!r->fog.on()) return CHUNKY_OK;
    return fail(CHUNKY_E_STATE, "%s: not supported under fog (chunky_render_set_fog); turn fog off (density 0) for this call", who);
}

FogPlan fog_plan(const chunky_render* r, const SceneView& S) {
    return plan_fog(r->kernel_variant, scene_facts(S), r->opts, r->cam.projector_type, r->shard, 0, r->work_counter.p != nullptr, false, biome_map(r, nullptr));
}
