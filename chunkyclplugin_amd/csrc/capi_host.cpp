// capi_host.cpp — entry points of include/chunky_hip.h that need no device: projected camera rays, java.util.Random, the wide-tree
// lookup and the tone map's threshold table.  Plain C++: no device code, no HIP type.
#include "capi_host.hpp"

#include <cmath>
#include <cstring>
#include <mutex>

#include "../../include/chunky_hip.h"
#include "camera_proj.h"
#include "canvas_host.hpp"
#include "canvas_window.h"
#include "capi_error.hpp"
#include "filter_alpha.h"
#include "rt_math.h"
#include "scene_records.hpp"
#include "widetree.hpp"

using namespace chunky;

int check_ints(const int32_t* p, int64_t n, const char* what) {
    if (n < 0 || (n > 0 && !p)) return fail(CHUNKY_E_INVALID, "%s: bad array (n=%lld)", what, (long long)n);
    return CHUNKY_OK;
}

// the decisions of scene_records.cpp behind SceneView::addr32, as entry points (tests/test_addr_bounds_cpu.py)
extern "C" int chunky_addr32_word(const int64_t dims[5], const uint64_t bytes[2], int indices_checked, uint32_t* word) {
    if (!dims || !bytes || !word) return fail(CHUNKY_E_INVALID, "addr32_word: NULL");
    AddrBounds b;
    b.atlas_w = dims[0], b.atlas_h = dims[1], b.atlas_layers = dims[2], b.sky_w = dims[3], b.sky_h = dims[4];
    b.aabb_rec_bytes = bytes[0], b.quad_rec_bytes = bytes[1];
    b.indices_checked = indices_checked != 0;
    *word = addr32_word(b);
    return CHUNKY_OK;
}

// projected cameras (types 1-5, 7, 8, camera_proj.h): 15 floats laid out as the pinhole camera's, all finite, settings[12] = 0 (the
// lens has a call of its own, chunky_render_set_lens), settings[14] > 0, settings[13] = 0 where the type has no use for it; the
// stacked ODS image has an eye offset >= 0 and an even height
static_assert(RT_PROJ_PARALLEL == CHUNKY_PROJ_PARALLEL && RT_PROJ_FISHEYE == CHUNKY_PROJ_FISHEYE && RT_PROJ_PANORAMIC == CHUNKY_PROJ_PANORAMIC &&
                  RT_PROJ_PANORAMIC_SLOT == CHUNKY_PROJ_PANORAMIC_SLOT && RT_PROJ_STEREOGRAPHIC == CHUNKY_PROJ_STEREOGRAPHIC &&
                  RT_PROJ_ODS == CHUNKY_PROJ_ODS && RT_PROJ_ODS_STACKED == CHUNKY_PROJ_ODS_STACKED, "camera_proj.h");
bool is_projected_type(int type) {
    return (type >= CHUNKY_PROJ_PARALLEL && type <= CHUNKY_PROJ_STEREOGRAPHIC) || type == CHUNKY_PROJ_ODS || type == CHUNKY_PROJ_ODS_STACKED;
}
int check_projected(const char* who, int type, const float* s, int64_t n, int height) {
    if (!is_projected_type(type))
        return fail(CHUNKY_E_INVALID, "%s: projector type %d is not a projected camera (1-5, 7, 8)", who, type);
    if (!s) return fail(CHUNKY_E_INVALID, "%s: NULL settings", who);
    if (n != 15) return fail(CHUNKY_E_INVALID, "%s: projector type %d needs 15 floats, got %lld", who, type, (long long)n);
    for (int i = 0; i < 15; i++)
        if (!std::isfinite(s[i])) return fail(CHUNKY_E_INVALID, "%s: settings[%d] is not finite", who, i);
    if (s[12] != 0.0f) return fail(CHUNKY_E_INVALID, "%s: settings[12] must be 0 for projector type %d (its lens is set by chunky_render_set_lens)", who, type);
    if (!(s[14] > 0.0f)) return fail(CHUNKY_E_INVALID, "%s: settings[14] must be > 0, got %g", who, (double)s[14]);
    if (s[13] != 0.0f && (type == CHUNKY_PROJ_FISHEYE || type == CHUNKY_PROJ_PANORAMIC || type == CHUNKY_PROJ_STEREOGRAPHIC))
        return fail(CHUNKY_E_INVALID, "%s: settings[13] must be 0 for projector type %d", who, type);
    if (type == CHUNKY_PROJ_ODS_STACKED) {
        if (s[13] < 0.0f) return fail(CHUNKY_E_INVALID, "%s: the stacked ODS image needs an eye offset >= 0, got %g", who, (double)s[13]);
        if (height % 2 != 0) return fail(CHUNKY_E_INVALID, "%s: the stacked ODS image needs an even height, got %d", who, height);
    }
    return CHUNKY_OK;
}
// the lens of a projected camera: finite, aperture >= 0, focus > 0 where there is an aperture
int check_lens(const char* who, float aperture, float focus) {
    if (!std::isfinite(aperture) || !std::isfinite(focus)) return fail(CHUNKY_E_INVALID, "%s: aperture and focus must be finite", who);
    if (aperture < 0.0f) return fail(CHUNKY_E_INVALID, "%s: aperture must be >= 0, got %g", who, (double)aperture);
    if (aperture > 0.0f && !(focus > 0.0f)) return fail(CHUNKY_E_INVALID, "%s: focus must be > 0 with an aperture, got %g", who, (double)focus);
    return CHUNKY_OK;
}

extern "C" int chunky_camera_rays_lens(int projector_type, const float* settings, int64_t n_floats, int width, int height, int32_t seed,
                                       float aperture, float focus, float* out) {
    if (int rc = check_projected("camera_rays", projector_type, settings, n_floats, height)) return rc;
    if (int rc = check_lens("camera_rays", aperture, focus)) return rc;
    if (width <= 0 || height <= 0 || (int64_t)width * height > INT32_MAX / 6)
        return fail(CHUNKY_E_INVALID, "camera_rays: bad size %dx%d", width, height);
    if (!out) return fail(CHUNKY_E_INVALID, "camera_rays: NULL output");
    const float half_width = (float)(width / (2.0 * height)), inv_height = (float)(1.0 / height);  // as set_camera
    for (int gid = 0; gid < width * height; gid++) {
        const RtRay r = rt_projected_ray(projector_type, settings, settings + 3, settings[13], settings[14], half_width, inv_height,
                                         height, aperture, focus, gid % width, gid / width, (unsigned)seed, gid);
        float* o = out + 6 * (size_t)gid;
        o[0] = r.ox; o[1] = r.oy; o[2] = r.oz;
        o[3] = r.dx; o[4] = r.dy; o[5] = r.dz;
    }
    return CHUNKY_OK;
}

// the same table for a window of a canvas (chunky_render_set_canvas): window pixel g is the canvas's pixel G — its jitter stream, its
// column and row, the canvas's half_width, inv_height and height — stored at g
extern "C" int chunky_camera_rays_window(int projector_type, const float* settings, int64_t n_floats, int width, int height, int canvas_width,
                                         int canvas_height, int x0, int y0, int32_t seed, float aperture, float focus, float* out) {
    if (int rc = check_canvas("camera_rays_window", width, height, canvas_width, canvas_height, x0, y0, projector_type)) return rc;
    if (int rc = check_projected("camera_rays_window", projector_type, settings, n_floats, canvas_height)) return rc;
    if (int rc = check_lens("camera_rays_window", aperture, focus)) return rc;
    if ((int64_t)width * height > INT32_MAX / 6) return fail(CHUNKY_E_INVALID, "camera_rays_window: bad size %dx%d", width, height);
    if (!out) return fail(CHUNKY_E_INVALID, "camera_rays_window: NULL output");
    const float half_width = (float)(canvas_width / (2.0 * canvas_height)), inv_height = (float)(1.0 / canvas_height);  // as set_camera
    const RtWindow w = rt_make_window(width, canvas_width, canvas_height, x0, y0);
    for (int g = 0; g < width * height; g++) {
        const RtCanvasPixel p = rt_canvas_pixel(g, g % width, g / width, w.x0, w.y0, w.row_skip, w.gid0);
        const RtRay r = rt_projected_ray(projector_type, settings, settings + 3, settings[13], settings[14], half_width, inv_height,
                                         w.canvas_height, aperture, focus, p.X, p.Y, (unsigned)seed, p.G);
        float* o = out + 6 * (size_t)g;
        o[0] = r.ox; o[1] = r.oy; o[2] = r.oz;
        o[3] = r.dx; o[4] = r.dy; o[5] = r.dz;
    }
    return CHUNKY_OK;
}

extern "C" int chunky_camera_rays(int projector_type, const float* settings, int64_t n_floats, int width, int height, int32_t seed, float* out) {
    return chunky_camera_rays_lens(projector_type, settings, n_floats, width, height, seed, 0.0f, 0.0f, out);
}

extern "C" int chunky_java_random_ints(int64_t seed, int32_t* out, int n) {
    if (n < 0 || (n > 0 && !out)) return fail(CHUNKY_E_INVALID, "java_random_ints: bad arguments");
    JavaRandom rnd(seed);
    for (int i = 0; i < n; i++) out[i] = rnd.next_int();
    return CHUNKY_OK;
}

// ------------------------------------------------------------------------------------ wide tree hook
extern "C" int chunky_widetree_lookup(const int32_t* tree, int64_t n_ints, int depth, const int32_t* level_bits,
                                      int n_levels, const int32_t* xyz, int n, int32_t* data_out, int32_t* level_out,
                                      int64_t* n_entries) {
    if (int rc = check_ints(tree, n_ints, "widetree_lookup")) return rc;
    if (n_ints < 1 || n < 0 || (n > 0 && (!xyz || !data_out || !level_out))) return fail(CHUNKY_E_INVALID, "widetree_lookup: bad arguments");
    int bits[kWideMaxLevels];
    int nlev;
    if (level_bits) {
        if (n_levels < 1 || n_levels > kWideMaxLevels) return fail(CHUNKY_E_INVALID, "widetree_lookup: 1..%d levels", kWideMaxLevels);
        nlev = n_levels;
        for (int i = 0; i < nlev; i++) bits[i] = level_bits[i];
    } else {
        nlev = default_wide_levels(depth, bits);
    }
    WideTree wt;
    const char* why = "";
    if (!build_wide_tree(tree, n_ints, depth, bits, nlev, &wt, &why)) return fail(CHUNKY_E_INVALID, "wide tree: %s", why);
    if (n_entries) *n_entries = (int64_t)wt.data.size();
    for (int i = 0; i < n; i++) {
        int x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
        if (((x | y | z) >> depth) != 0) return fail(CHUNKY_E_INVALID, "widetree_lookup: cell outside the world");
        int32_t e = 0;
        for (int l = 0; l < wt.nlev && e >= 0; l++) {
            const int sh = wt.shift[l], b = wt.bits[l], m = (1 << b) - 1;
            e = (int32_t)wt.data[(size_t)e + (size_t)(((((x >> sh) & m) << b) | ((y >> sh) & m)) << b | ((z >> sh) & m))];
        }
        if (e >= 0) return fail(CHUNKY_E_INVALID, "wide tree: lookup did not end in a leaf");
        level_out[i] = (e >> kWideLevelShift) & 15;
        const uint32_t ptr = (uint32_t)e & kWidePtrMask;
        data_out[i] = ptr == kWidePtrMask ? 0x7FFFFFFE : (int32_t)ptr;
    }
    return CHUNKY_OK;
}

extern "C" int chunky_widetree_hit_top(const int32_t* tree, int64_t n_ints, int depth, const int32_t* level_bits, int n_levels,
                                       const int32_t* blocks, int64_t n_block_ints, int32_t* hit_top) {
    if (int rc = check_ints(tree, n_ints, "widetree_hit_top")) return rc;
    if (int rc = check_ints(blocks, n_block_ints, "widetree_hit_top palette")) return rc;
    if (n_ints < 1 || !hit_top) return fail(CHUNKY_E_INVALID, "widetree_hit_top: bad arguments");
    int bits[kWideMaxLevels];
    int nlev;
    if (level_bits) {
        if (n_levels < 1 || n_levels > kWideMaxLevels) return fail(CHUNKY_E_INVALID, "widetree_hit_top: 1..%d levels", kWideMaxLevels);
        nlev = n_levels;
        for (int i = 0; i < nlev; i++) bits[i] = level_bits[i];
    } else {
        nlev = default_wide_levels(depth, bits);
    }
    WideTree wt;
    const char* why = "";
    if (!build_wide_tree(tree, n_ints, depth, bits, nlev, &wt, &why)) return fail(CHUNKY_E_INVALID, "wide tree: %s", why);
    annotate_wide_tree(&wt, blocks, n_block_ints);
    *hit_top = wt.hit_top;
    return CHUNKY_OK;
}

// ------------------------------------------------------------------------------------ tone map
// The last steps of the GAMMA and ACES curves for one channel value (post_processing_filter.cl:24-27, rgba.h:9-14) on the
// host, with the rt_pow the kernels and the checkers share: pow(c, 1/2.2) * 255 + 0.5 -> (uint), saturating -> min(255).
static unsigned gamma_byte_host(float c) {
    const float f = rt_pow(c, (float)(1.0 / 2.2)) * 255.0f + 0.5f;
    const unsigned u = !(f > 0.0f) ? 0u : (f >= 4294967296.0f ? 0xFFFFFFFFu : (unsigned)f);
    return u > 255u ? 255u : u;
}
// T[k] (k = 1..255) = the smallest non-negative float whose byte is >= k, by bisection over the float's bit pattern (the
// byte is a non-decreasing function of c: checked over every float by tests/test_filter.py); T[0] = 0.
const float* gamma_thresholds() {
    static float T[256];
    static std::once_flag once;
    std::call_once(once, [] {
        T[0] = 0.0f;
        for (int k = 1; k < 256; k++) {
            uint32_t lo = 0u, hi = 0x7F800000u;  // byte(+0) = 0 < k <= byte(+inf) = 255
            while (hi - lo > 1u) {
                const uint32_t mid = lo + (hi - lo) / 2;
                float c;
                memcpy(&c, &mid, 4);
                if (gamma_byte_host(c) >= (unsigned)k) hi = mid; else lo = mid;
            }
            memcpy(&T[k], &hi, 4);
        }
    });
    return T;
}
extern "C" int chunky_filter_alpha_bytes(const float* alpha, int64_t n, int32_t* out) {
    if (n < 0 || (n > 0 && (!alpha || !out))) return fail(CHUNKY_E_INVALID, "filter_alpha_bytes: bad arguments");
    for (int64_t i = 0; i < n; i++) out[i] = (int32_t)rt_alpha_byte(alpha[i]);
    return CHUNKY_OK;
}

extern "C" int chunky_filter_gamma_thresholds(float* out256) {
    if (!out256) return fail(CHUNKY_E_INVALID, "gamma_thresholds: NULL output");
    memcpy(out256, gamma_thresholds(), 256 * sizeof(float));
    return CHUNKY_OK;
}
