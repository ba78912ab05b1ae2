// glass_host.cpp — translucent blocks (chunky_render_set_translucency): what can be decided without a device — the
// check of a caller's chunky_translucency, and the self test of plan_glass.  Plain C++: no device code, no HIP type.
#include "glass_host.hpp"

#include <cstdio>
#include <cstring>

#include "../../include/chunky_hip.h"
#include "capi_error.hpp"
#include "launch_plan.hpp"

namespace {
constexpr size_t kGlassFirstVersion = offsetof(chunky_translucency, max_crossings) + sizeof(((chunky_translucency*)nullptr)->max_crossings);  // the members of the first version
constexpr size_t kGlassMaxSize = 4096;  // (a size beyond any version this struct will ever have is a caller's mistake, not a newer header)
}  // namespace

int check_translucency(const char* who, const chunky_translucency* t, GlassSettings* out) {
    if (!t) {
        if (out) *out = GlassSettings{};
        return CHUNKY_OK;
    }
    const size_t have = t->size;
    if (have < kGlassFirstVersion || have > kGlassMaxSize)
        return fail(CHUNKY_E_INVALID, "%s: chunky_translucency.size is %zu; this library knows %zu bytes (set size = sizeof(chunky_translucency))", who, have,
                    sizeof(chunky_translucency));
    if (have > sizeof(chunky_translucency)) {  // a newer caller: whatever it has that this library does not know must be unset
        const unsigned char* tail = (const unsigned char*)t + sizeof(chunky_translucency);
        for (size_t i = 0; i < have - sizeof(chunky_translucency); i++)
            if (tail[i] != 0)
                return fail(CHUNKY_E_INVALID, "%s: chunky_translucency of %zu bytes sets a member this library (%zu bytes) does not know", who, have,
                            sizeof(chunky_translucency));
    }
    chunky_translucency g;
    if (!take_versioned(t, have, kGlassFirstVersion, &g)) return fail(CHUNKY_E_INVALID, "%s: chunky_translucency.size %zu is too small", who, have);
    if (!(g.opaque_alpha > 0.0f && g.opaque_alpha <= 1.0f))  // (a NaN fails both)
        return fail(CHUNKY_E_INVALID, "%s: opaque_alpha %g is outside (0, 1]", who, (double)g.opaque_alpha);
    if (g.max_crossings < 1 || g.max_crossings > 31)
        return fail(CHUNKY_E_INVALID, "%s: max_crossings %d is outside [1, 31]", who, (int)g.max_crossings);
    if (out) {
        GlassSettings s;
        s.enabled = true;
        s.opaque_alpha = g.opaque_alpha;
        s.max_crossings = (int)g.max_crossings;
        *out = s;
    }
    return CHUNKY_OK;
}

extern "C" int chunky_translucency_check(const chunky_translucency* t) { return check_translucency("translucency_check", t, nullptr); }

extern "C" int chunky_selftest_plan_glass(const int32_t* rows9, int64_t n, int32_t* out8, char* text256) {
    using namespace chunky;
    if (n < 0 || (n > 0 && (!rows9 || !out8))) return fail(CHUNKY_E_INVALID, "selftest_plan_glass: bad arguments");
    for (int64_t i = 0; i < n; i++) {
        const int32_t* v = rows9 + 9 * i;
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
        const GlassPlan g = plan_glass(v[0], F, O, v[1], T, 1, true, false, v[6] != 0, v[8] != 0);
        const RenderPlan& p = g.plan;
        const int32_t o[8] = {(int32_t)p.status, (int32_t)g.refusal, p.tree, p.park, p.bvh, p.ext, (int32_t)p.family, p.words};
        memcpy(out8 + 8 * i, o, sizeof o);
        if (text256) snprintf(text256 + 256 * i, 256, "%s", glass_refusal_text(g.refusal));
    }
    return CHUNKY_OK;
}
