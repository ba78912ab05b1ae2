/* camera_proj.h — the projected cameras (CHUNKY_PROJ_PARALLEL .. CHUNKY_PROJ_STEREOGRAPHIC, include/chunky_hip.h, DESIGN.md
 * section 11): the primary ray of one sample, computed from the pass seed.  One definition for both sides: the kernels call it
 * through primary_ray (rt_device.hpp) and chunky_camera_rays (capi_host.cpp) runs it on the host to build the equivalent table of
 * projector type -1.  Float arithmetic with the rt_math.h functions only, in the order written, built with -ffp-contract=off, so
 * the two sides agree bit for bit.
 *
 * The jitter has a stream of its own, (seed ^ 0x9E3779B9) + gid, and does not touch the path's state (seed + gid advanced once, as
 * on the pre-generated path, K/rayTracer.cl:55-57).  That is what makes a pass with a projected camera the reference's pass on
 * the table of these rays. */
#ifndef CHUNKY_CAMERA_PROJ_H
#define CHUNKY_CAMERA_PROJ_H

#include "rt_math.h"

#define RT_PROJ_PARALLEL 1
#define RT_PROJ_FISHEYE 2
#define RT_PROJ_PANORAMIC 3
#define RT_PROJ_PANORAMIC_SLOT 4
#define RT_PROJ_STEREOGRAPHIC 5
#define RT_PROJ_JITTER_KEY 0x9E3779B9u

typedef struct {
    float ox, oy, oz, dx, dy, dz;
} RtRay;

/* degrees to radians with float pi/180 (0x3C8EFA35) */
RT_FN float rt_rad(float v) { return v * 0.0174532924f; }

/* The ray of pixel (px, py) = (gid % width, gid / width) in the pass of seed `seed`, in world space.  s13 / s14 are settings[13] /
 * settings[14] of chunky_render_set_camera; pos and m as the pinhole camera's (ClCamera.java:42-52, m row-major). */
RT_FN RtRay rt_projected_ray(int type, const float* pos, const float* m, float s13, float s14, float half_width, float inv_height,
                             int px, int py, unsigned seed, int gid) {
    unsigned j = (seed ^ RT_PROJ_JITTER_KEY) + (unsigned)gid;
    const float jx = rt_pcg_float(&j);
    const float jy = rt_pcg_float(&j);
    const float x = -half_width + ((float)px + jx) * inv_height;                       /* primary_ray's own rounding */
    const float y = (float)(-0.5 + (double)(((float)py + jy) * inv_height));
    float lox = 0.0f, loy = 0.0f, loz = 0.0f, ldx, ldy, ldz;
    if (type == RT_PROJ_PARALLEL) {
        lox = s14 * x;
        loy = s14 * y;
        loz = -s13;
        ldx = 0.0f;
        ldy = 0.0f;
        ldz = 1.0f;
    } else if (type == RT_PROJ_FISHEYE) {
        const float ax = rt_rad(x * s14), ay = rt_rad(y * s14);
        const float a = rt_sqrt(ax * ax + ay * ay);
        if (a == 0.0f) {
            ldx = 0.0f;
            ldy = 0.0f;
            ldz = 1.0f;
        } else {
            const float s = rt_sin(a);
            ldx = s * (ax / a);
            ldy = s * (ay / a);
            ldz = rt_cos(a);
        }
    } else if (type == RT_PROJ_PANORAMIC) {
        const float ax = rt_rad(x * s14), ay = rt_rad(y * s14);
        const float c = rt_cos(ay);
        ldx = c * rt_sin(ax);
        ldy = rt_sin(ay);
        ldz = c * rt_cos(ax);
    } else if (type == RT_PROJ_PANORAMIC_SLOT) {
        const float ax = rt_rad(x * s14);
        ldx = rt_sin(ax);
        ldy = s13 * y;
        ldz = rt_cos(ax);
    } else { /* RT_PROJ_STEREOGRAPHIC */
        const float X = s14 * x, Y = s14 * y;
        const float r2 = X * X + Y * Y;
        const float q = 1.0f + r2;
        ldx = (2.0f * X) / q;
        ldy = (2.0f * Y) / q;
        ldz = (1.0f - r2) / q;
    }
    const float rl = rt_rlen3(ldx, ldy, ldz); /* normalize (rt_device.hpp), as calcViewRay normalises */
    ldx = ldx * rl;
    ldy = ldy * rl;
    ldz = ldz * rl;
    RtRay r;
    r.dx = rt_dot3(m[0], m[1], m[2], ldx, ldy, ldz);
    r.dy = rt_dot3(m[3], m[4], m[5], ldx, ldy, ldz);
    r.dz = rt_dot3(m[6], m[7], m[8], ldx, ldy, ldz);
    r.ox = rt_dot3(m[0], m[1], m[2], lox, loy, loz) + pos[0];
    r.oy = rt_dot3(m[3], m[4], m[5], lox, loy, loz) + pos[1];
    r.oz = rt_dot3(m[6], m[7], m[8], lox, loy, loz) + pos[2];
    return r;
}

#endif /* CHUNKY_CAMERA_PROJ_H */
