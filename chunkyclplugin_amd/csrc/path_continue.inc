// path_continue.inc — piece (b) of SHADE, the continuation of a path behind a finished trace, as text: the hit point becomes the origin
// and the hit colours the throughput (a main ray's hit), then the shadow ray towards the sun or the bounce from one sampling block, and
// the depth check.  Included where it runs, with these names in scope:
//   S, O        the scene and the options (read: S.su, sv, sw, sun_radius_cos, sun_flags; O.emitter_scale, max_depth)
//   L           the path (LaneState)
//   main_trace  the trace that ended was the path's ray, not a shadow ray
//   finished    bool, read and written: coming in, the path ended with the trace (a main ray in the sky) and nothing is drawn for it;
//               going out, the path is finished — otherwise L.o / L.d hold the ray trace_setup starts
// Two places include it: shade_phase (path_state.hpp), and render_pool's block test for the lanes it can tell will go on
// (render_pool.hip block_continues).  Text and not a function, so that shade_phase — and with it every kernel that only runs SHADE —
// compiles to the instructions it had with this block written in it (as a function inlined there the compiler orders the locals
// differently, and the sky's loads and blend come out in other registers).
    bool to_sun = false;  // start a shadow ray towards the sun; otherwise bounce
    if (finished) {
    } else if (main_trace) {
        // the hit point (K/kernel.h:21-23) becomes the origin of the shadow ray and stays there until the bounce
        L.o = L.o + L.d * (L.h.distance - kOffset);
        // applyRayColor (K/kernel.h:33-44)
        f3 c = mk3(L.h.color.x, L.h.color.y, L.h.color.z);
        L.throughput = L.throughput * c;
        L.radiance = L.radiance + (c * (L.h.emittance * O.emitter_scale)) * L.throughput;
        if (S.sun_flags & 1) to_sun = true;
    } else {
        L.shadow = false;
    }
    // Sun_sampleDirection (K/sky.h:68-93) for the lanes that start a shadow ray, nextPath (K/kernel.h:46-98)
    // for the lanes that bounce.  A lane does one or the other, and both have the same skeleton — two draws,
    // sin/cos of 2*pi*x2, a square root, a vector, its reciprocal length — so the expensive steps are issued
    // once for both kinds of lane and only the cheap vector algebra in between is specific.
    if (!finished) {
        const float x1 = rt_pcg_float(&L.rng), x2 = rt_pcg_float(&L.rng);
        float sn, cs;
        rt_sincos(2 * RT_PI_F * x2, &sn, &cs);
        const float cos_a = 1 - x1 + x1 * S.sun_radius_cos;          // sun: cosine of the angle off the sun axis
        const float root = rt_sqrt(to_sun ? 1 - cos_a * cos_a : x1);  // sun: sin_a; bounce: r
        const f3 n = L.h.normal;
        f3 a;        // sun: the unnormalised direction; bounce: the unnormalised tangent u
        float len2;  // its squared length, each written as the reference writes it
        if (to_sun) {
            const f3 u = S.su * (cs * root), v = S.sv * (sn * root), w = S.sw * cos_a;
            a = (u * v) + w;  // component-wise product, as the reference has it
            len2 = dot(a, a);
        } else {
            float xx, xy, xz = 0;
            if ((double)rt_fabs(n.x) > 0.1) {
                xx = 0;
                xy = 1;
            } else {
                xx = 1;
                xy = 0;
            }
            a = mk3(xy * n.z - xz * n.y, xz * n.x - xx * n.z, xx * n.y - xy * n.x);
            len2 = a.x * a.x + a.y * a.y + a.z * a.z;
        }
        const float rl = rcp_exact(rt_sqrt(len2));
        a = a * rl;
        if (to_sun) {
            L.d = a;
            L.shadow = true;  // (record.emittance = |dot(L.d, n)|, K/sky.h:90: evaluated where it is read, above)
        } else {
            const float tx = root * cs, ty = root * sn, tz = rt_sqrt(1 - x1);
            const float vx = a.y * n.z - a.z * n.y, vy = a.z * n.x - a.x * n.z, vz = a.x * n.y - a.y * n.x;
            L.d = f3{a.x * tx + vx * ty + n.x * tz, a.y * tx + vy * ty + n.y * tz, a.z * tx + vz * ty + n.z * tz};
            L.o = L.o + L.d * kOffset;
            L.depth += 1;
            L.h.distance = rt_inf();
            finished = !(L.depth < O.max_depth);
        }
    }
