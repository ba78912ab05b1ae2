// fog_host.cpp — the ground-fog layer (chunky_render_set_fog): what can be decided without a device — the check of
// a caller's chunky_fog, and the self test of plan_fog.  Plain C++: no device code, no HIP type.
#include "fog_host.hpp"

#include <cmath>
#include <cstdio>
#include <cstring>

#include "../../include/chunky_hip.h"
#include "capi_error.hpp"
#include "launch_plan.hpp"

namespace {
constexpr size_t kFogFirstVersion = offsetof(chunky_fog, color) + sizeof(((chunky_fog*)nullptr)->color);  // the members of the first version
constexpr size_t kFogMaxSize = 4096;  // (a size beyond any version this struct will ever have is a caller's mistake, not a newer header)
}  // namespace

int check_fog(const char* who, const chunky_fog* fog, FogSettings* out) {
    if (!fog) {
        if (out) *out = FogSettings{};
        return CHUNKY_OK;
    }
    const size_t have = fog->size;
    if (have < kFogFirstVersion || have > kFogMaxSize)
        return fail(CHUNKY_E_INVALID, "%s: chunky_fog.size is %zu; this library knows %zu bytes (set size = sizeof(chunky_fog))", who, have, sizeof(chunky_fog));
    if (have > sizeof(chunky_fog)) {  // a newer caller: whatever it has that this library does not know must be unset
        const unsigned char* tail = (const unsigned char*)fog + sizeof(chunky_fog);
        for (size_t i = 0; i < have - sizeof(chunky_fog); i++)
            if (tail[i] != 0)
                return fail(CHUNKY_E_INVALID, "%s: chunky_fog of %zu bytes sets a member this library (%zu bytes) does not know", who, have, sizeof(chunky_fog));
    }
    chunky_fog f;
    if (!take_versioned(fog, have, kFogFirstVersion, &f)) return fail(CHUNKY_E_INVALID, "%s: chunky_fog.size %zu is too small", who, have);
    const float v[6] = {f.density, f.y_min, f.y_max, f.color[0], f.color[1], f.color[2]};
    for (float x : v)
        if (!std::isfinite(x)) return fail(CHUNKY_E_INVALID, "%s: a fog parameter is not finite", who);
    if (f.density < 0.0f) return fail(CHUNKY_E_INVALID, "%s: fog density %g is negative", who, (double)f.density);
    if (!(f.y_min < f.y_max)) return fail(CHUNKY_E_INVALID, "%s: the fog slab needs y_min < y_max, got [%g, %g]", who, (double)f.y_min, (double)f.y_max);
    for (int k = 0; k < 3; k++)
        if (f.color[k] < 0.0f || f.color[k] > 1.0f)
            return fail(CHUNKY_E_INVALID, "%s: fog colour component %d is %g, outside [0, 1]", who, k, (double)f.color[k]);
    if (out) {
        FogSettings s;
        if (f.density > 0.0f) {  // (density 0 is "off": nothing else is kept)
            s.density = f.density, s.y_min = f.y_min, s.y_max = f.y_max;
            for (int k = 0; k < 3; k++) s.color[k] = f.color[k];
        }
        *out = s;
    }
    return CHUNKY_OK;
}

extern "C" int chunky_fog_check(const chunky_fog* fog) { return check_fog("fog_check", fog, nullptr); }

extern "C" int chunky_selftest_plan_fog(const int32_t* rows8, int64_t n, int32_t* out8, char* text256) {
    using namespace chunky;
    if (n < 0 || (n > 0 && (!rows8 || !out8))) return fail(CHUNKY_E_INVALID, "selftest_plan_fog: bad arguments");
    for (int64_t i = 0; i < n; i++) {
        const int32_t* v = rows8 + 8 * i;
        SceneFacts F{};
        F.wide = v[3] != 0;
        F.wide_nlev = v[7];
        for (int k = 0; k < 6; k++) F.wide_bits[k] = 3;
        F.world_bvh_empty = v[4] == 0, F.actor_bvh_empty = true;
        F.bvh_stack_entries = 8;
        F.bvh_records = v[5] != 0;
        F.addr32 = kPoolAddr32Forms;
        F.sort_blocks = false, F.block_info = true;
        RenderOpts O{256, v[2], 13.0f, -1, 1, 0, 0, 0};
        ShardView T{0, 1, 256, 0};
        const FogPlan f = plan_fog(v[0], F, O, v[1], T, 1, true, false, v[6] != 0);
        const RenderPlan& p = f.plan;
        const int32_t o[8] = {(int32_t)p.status, (int32_t)f.refusal, p.tree, p.park, p.bvh, p.ext, (int32_t)p.family, 0};
        memcpy(out8 + 8 * i, o, sizeof o);
        if (text256) snprintf(text256 + 256 * i, 256, "%s", fog_refusal_text(f.refusal));
    }
    return CHUNKY_OK;
}
