/* camera_proj.h — the projected cameras (CHUNKY_PROJ_PARALLEL .. CHUNKY_PROJ_STEREOGRAPHIC, CHUNKY_PROJ_ODS, CHUNKY_PROJ_ODS_STACKED,
 * include/chunky_hip.h) and their lens: the primary ray of one sample, computed from the pass seed.  One definition for both sides: the kernels call it
 * through primary_ray (rt_device.hpp) and chunky_camera_rays (capi_host.cpp) runs it on the host to build the equivalent table of
 * projector type -1.  Float arithmetic with the rt_math.h functions only, in the order written, built with -ffp-contract=off, so
 * the two sides agree bit for bit.
 *
 * The jitter has a stream of its own, (seed ^ 0x9E3779B9) + gid, and does not touch the path's state (seed + gid advanced once, as
 * on the pre-generated path, K/rayTracer.cl:55-57).  That is what makes a pass with a projected camera the reference's pass on
 * the table of these rays.  The lens (depth of field, chunky_render_set_lens) takes draws 3 and 4 of the same stream, so the
 * equivalence holds with a lens as without: the table is then chunky_camera_rays_lens'. */
#ifndef CHUNKY_CAMERA_PROJ_H
#define CHUNKY_CAMERA_PROJ_H

#include "rt_math.h"

#define RT_PROJ_PARALLEL 1
#define RT_PROJ_FISHEYE 2
#define RT_PROJ_PANORAMIC 3
#define RT_PROJ_PANORAMIC_SLOT 4
#define RT_PROJ_STEREOGRAPHIC 5
#define RT_PROJ_ODS 7          /* (6 stays unassigned) */
#define RT_PROJ_ODS_STACKED 8
#define RT_PROJ_JITTER_KEY 0x9E3779B9u

typedef struct {
    float ox, oy, oz, dx, dy, dz;
} RtRay;

/* degrees to radians with float pi/180 (0x3C8EFA35) */
RT_FN float rt_rad(float v) { return v * 0.0174532924f; }

/* The ray of pixel (px, py) = (gid % width, gid / width) in the pass of seed `seed`, in world space.  s13 / s14 are settings[13] /
 * settings[14] of chunky_render_set_camera; pos and m as the pinhole camera's (ClCamera.java:42-52, m row-major); height is the
 * image's (the stacked ODS image changes eye at height / 2); aperture / focus are chunky_render_set_lens', aperture 0 = no lens:
 * nothing more is drawn and nothing below the projection runs.
 * The image is the CANVAS (chunky_render_set_canvas, canvas_window.h): for a target that is a window of one, px, py and gid are the
 * pixel's column, row and index on the canvas, and half_width, inv_height and height the canvas's. */
RT_FN RtRay rt_projected_ray(int type, const float* pos, const float* m, float s13, float s14, float half_width, float inv_height,
                             int height, float aperture, float focus, int px, int py, unsigned seed, int gid) {
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
    } else if (type == RT_PROJ_ODS || type == RT_PROJ_ODS_STACKED) {
        /* omnidirectional stereo: every column looks along its own yaw th from a point of the circle of radius |e| = |s13| about
         * the camera, a quarter turn off the view direction; e > 0 is the right eye.  Stacked: the left eye's image on top. */
        const float th = x * (RT_PI_F / half_width);
        float y2 = y, eye = s13;
        if (type == RT_PROJ_ODS_STACKED) {
            const int top = py < height / 2;
            y2 = top ? 2.0f * y + 0.5f : 2.0f * y - 0.5f;
            eye = top ? -s13 : s13;
        }
        const float ph = rt_rad(y2 * s14);
        float st, ct, sp, cp;
        rt_sincos(th, &st, &ct);
        rt_sincos(ph, &sp, &cp);
        ldx = cp * st;
        ldy = sp;
        ldz = cp * ct;
        lox = eye * ct;
        loz = -(eye * st);
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
    if (aperture > 0.0f) {
        /* the lens: a point of the disc of radius `aperture` about lo, and the direction from it to where the lens-off ray is in
         * focus: PARALLEL on the plane `focus` in front of the origins' plane with the disc in that plane (local z = focus - b and
         * z = -b; b = 0: z = focus and z = 0), every other type on the sphere of radius `focus` about lo with the disc across ld */
        const float u1 = rt_pcg_float(&j);
        const float u2 = rt_pcg_float(&j);
        const float r = rt_sqrt(u1) * aperture;
        const float theta = (float)((double)(u2 * RT_PI_F) * 2.0); /* the pinhole lens's rounding (K/camera.h:24-27) */
        float st, ct;
        rt_sincos(theta, &st, &ct);
        const float rx = ct * r, ry = st * r;
        float fx, fy, fz, tx, ty, tz;
        if (type == RT_PROJ_PARALLEL) {
            fx = rx;
            fy = ry;
            fz = 0.0f;
            tx = 0.0f - fx;
            ty = 0.0f - fy;
            tz = focus - fz;
        } else {
            float ux, uy, uz;
            if (rt_fabs(ldx) > rt_fabs(ldy)) {
                ux = -ldz;
                uy = 0.0f;
                uz = ldx;
            } else {
                ux = 0.0f;
                uy = ldz;
                uz = -ldy;
            }
            const float ul = rt_rlen3(ux, uy, uz); /* (never 0 for a unit ld: the larger of |ld.x|, |ld.y| or ld.z is in it) */
            ux = ux * ul;
            uy = uy * ul;
            uz = uz * ul;
            const float vx = ldy * uz - ldz * uy; /* cross(ld, U) */
            const float vy = ldz * ux - ldx * uz;
            const float vz = ldx * uy - ldy * ux;
            fx = ux * rx + vx * ry;
            fy = uy * rx + vy * ry;
            fz = uz * rx + vz * ry;
            tx = ldx * focus - fx;
            ty = ldy * focus - fy;
            tz = ldz * focus - fz;
        }
        lox = lox + fx;
        loy = loy + fy;
        loz = loz + fz;
        const float tl = rt_rlen3(tx, ty, tz);
        ldx = tx * tl;
        ldy = ty * tl;
        ldz = tz * tl;
    }
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
