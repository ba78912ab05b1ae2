// window_fuzz.cpp — the device-free half of the canvas windows (csrc/canvas_host.cpp check_canvas, csrc/canvas_window.h
// rt_canvas_pixel) under AddressSanitizer + UBSan: random and extreme arguments at the checker against its rules restated in 64-bit
// arithmetic, and for every window it accepts the (g, px, py) -> (G, X, Y) helper at the window's corners and at random pixels
// against 64-bit arithmetic — an int that overflowed on the way would be a UBSan report.  Prints one JSON line.
#include <cstdint>
#include <cstdio>
#include <random>

#include "../../chunkyclplugin_amd/csrc/canvas_host.hpp"
#include "../../chunkyclplugin_amd/csrc/canvas_window.h"
#include "../../include/chunky_hip.h"

static long long failures = 0, accepted = 0, refused = 0, pixels = 0;

static bool expect_ok(int w, int h, int cw, int ch, int x0, int y0, int type) {
    if (w <= 0 || h <= 0 || cw <= 0 || ch <= 0) return false;
    if (x0 < 0 || y0 < 0) return false;
    if ((int64_t)x0 + w > (int64_t)cw || (int64_t)y0 + h > (int64_t)ch) return false;
    if ((int64_t)cw * (int64_t)ch > (int64_t)INT32_MAX) return false;
    if (type == CHUNKY_PROJ_ODS_STACKED && (ch & 1)) return false;
    return true;
}

static void pixel(int w, int cw, int ch, int x0, int y0, int px, int py) {
    const RtWindow win = rt_make_window(w, cw, ch, x0, y0);
    const int g = py * w + px;
    const RtCanvasPixel p = rt_canvas_pixel(g, px, py, win.x0, win.y0, win.row_skip, win.gid0);
    const int64_t X = (int64_t)x0 + px, Y = (int64_t)y0 + py, G = Y * (int64_t)cw + X;
    pixels++;
    if ((int64_t)p.X != X || (int64_t)p.Y != Y || (int64_t)p.G != G || G < 0 || G >= (int64_t)cw * ch || win.canvas_height != ch) {
        failures++;
        fprintf(stderr, "pixel (%d, %d) of a %d-wide window at (%d, %d) of %d x %d: got G %d X %d Y %d, want %lld %lld %lld\n", px, py, w, x0, y0, cw,
                ch, p.G, p.X, p.Y, (long long)G, (long long)X, (long long)Y);
    }
}

static void one(std::mt19937_64& rng, int w, int h, int cw, int ch, int x0, int y0, int type) {
    const bool want = expect_ok(w, h, cw, ch, x0, y0, type);
    const int rc = check_canvas("fuzz", w, h, cw, ch, x0, y0, type);
    if ((rc == CHUNKY_OK) != want || (rc != CHUNKY_OK && rc != CHUNKY_E_INVALID)) {
        failures++;
        fprintf(stderr, "check_canvas(%d x %d in %d x %d at (%d, %d), type %d) = %d, want %s\n", w, h, cw, ch, x0, y0, type, rc, want ? "OK" : "INVALID");
        return;
    }
    if (rc != CHUNKY_OK) {
        refused++;
        return;
    }
    accepted++;
    // the kernels only see targets of at most 2^30 pixels (chunky_render_create): g = py * w + px stays an int there
    if ((int64_t)w * h > ((int64_t)1 << 30)) return;
    const int xs[3] = {0, w / 2, w - 1}, ys[3] = {0, h / 2, h - 1};
    for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++) pixel(w, cw, ch, x0, y0, xs[a], ys[b]);
    for (int k = 0; k < 8; k++) pixel(w, cw, ch, x0, y0, (int)(rng() % (uint64_t)w), (int)(rng() % (uint64_t)h));
}

int main() {
    std::mt19937_64 rng(20260919);
    const int extremes[] = {INT32_MIN, INT32_MIN + 1, -65536, -2, -1, 0, 1, 2, 15, 16, 17, 33, 46340, 46341, 65535, 65536, 1 << 30, INT32_MAX - 1, INT32_MAX};
    const int n_ext = (int)(sizeof extremes / sizeof extremes[0]);
    const int types[] = {-1, 0, 1, 5, 7, 8};
    // every argument an extreme, the others random
    for (int round = 0; round < 200000; round++) {
        int v[6];
        for (int k = 0; k < 6; k++) {
            const uint64_t r = rng();
            switch (r & 3) {
                case 0: v[k] = extremes[(r >> 8) % (uint64_t)n_ext]; break;
                case 1: v[k] = (int)((r >> 8) % 70); break;
                case 2: v[k] = (int)((r >> 8) % 50000); break;
                default: v[k] = (int)(int32_t)(r >> 16); break;
            }
        }
        one(rng, v[0], v[1], v[2], v[3], v[4], v[5], types[rng() % 6]);
    }
    // windows that fit by construction, canvases up to the limit: small, poster-sized, one row or column of 2^31 - 1 pixels, 46340^2
    for (int round = 0; round < 200000; round++) {
        int cw, ch;
        switch (rng() % 5) {
            case 0: cw = 1 + (int)(rng() % 100), ch = 1 + (int)(rng() % 100); break;
            case 1: cw = 1 + (int)(rng() % 46340), ch = 1 + (int)(rng() % 46340); break;
            case 2: cw = INT32_MAX, ch = 1; break;
            case 3: cw = 1, ch = INT32_MAX; break;
            default: cw = 46340, ch = 46340; break;
        }
        const int w = 1 + (int)(rng() % (uint64_t)cw), h = 1 + (int)(rng() % (uint64_t)ch);
        int x0 = (int)(rng() % (uint64_t)(cw - w + 1)), y0 = (int)(rng() % (uint64_t)(ch - h + 1));
        if (rng() % 4 == 0) x0 = cw - w, y0 = ch - h;  // flush with the far edges
        one(rng, w, h, cw, ch, x0, y0, types[rng() % 6]);
        if (rng() % 8 == 0) one(rng, w, h, cw, ch, x0 + 1 + (cw - w - x0), y0, 0);  // one column too far
    }
    // the limit itself
    one(rng, 8, 8, 46341, 46341, 0, 0, 0);
    one(rng, 8, 8, 46340, 46340, 46332, 46332, 0);
    one(rng, 8, 8, 40000, 40000, 39990, 39985, 0);
    one(rng, 33, 17, 64, 47, 0, 0, CHUNKY_PROJ_ODS_STACKED);
    one(rng, 33, 17, 64, 48, 31, 31, CHUNKY_PROJ_ODS_STACKED);
    printf("{\"failures\": %lld, \"accepted\": %lld, \"refused\": %lld, \"pixels\": %lld}\n", failures, accepted, refused, pixels);
    return failures ? 1 : 0;
}
