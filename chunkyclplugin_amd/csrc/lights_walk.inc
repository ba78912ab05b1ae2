// lights_walk.inc — the body of the light-group kernels, included into light_kernel (lights.hip) and light_group_kernel
// (lights_groups.hip) with `LightOut` naming the tail of the kernel's arguments and GROUPS saying whether the emitter groups are folded
// (lights_device.hpp).  Text, not a function: as a function inlined into the kernels it compiled to other code than the kernel had.
    extern __shared__ int lds[];
    LdsStack stack{lds + threadIdx.x, (int)blockDim.x};
    const int lane = (int)(threadIdx.x & 63);
    for (;;) {
        auto a = first_hit_args<LightOut>();
        const int width = a->C.width, height = a->C.height, n_pixels = width * height;
        // every lane of the wave is here (both exits below are wave-uniform): lane 0 claims, the others take its value
        int unit = 0;
        if (lane == 0) unit = atomicAdd(a->counter, 1);
        unit = __builtin_amdgcn_readfirstlane(unit);
        if (unit >= a->n_units) break;
        const int gid = pool_slot_gid(arg_copy(&a->T), width, height, unit * kFirstHitUnit + lane);
        const bool mine = gid < n_pixels;  // (not a padding slot)
        const int n_passes = a->P.n, first_spp = a->P.first_spp;
        int px = 0, py = 0;
        if (mine) px = gid % width, py = gid / width;
        int state = mine ? LT_MAIN : LT_DONE;  // (a launch carries at least one pass)
        bool start = mine;                     // the lane begins the sample of its pass k
        int k = 0, depth = 0;
        unsigned rng = 0;
        f3 o = mk3(0, 0, 0), d = mk3(0, 0, 0), n0 = mk3(0, 0, 0), throughput = mk3(1, 1, 1);
        float reach = 0;  // the distance the trace's record starts with
        // the trace under way (light_octree_round): the distance marched, the steps taken (0: it begins) and the record's normal
        float dist_march = 0;
        int step = 0;
        f3 tn = mk3(0, 0, 0);
        LightSums sums;
#pragma unroll
        for (int g = 0; g < 4; g++) sums.g[g] = mk3(0, 0, 0);
        for (;;) {
            if (start) {  // K/rayTracer.cl:54-91
                auto b = first_hit_args<LightOut>();
                const unsigned seed = (unsigned)b->P.seed[k];
                const CameraView C = arg_copy(&b->C);
                const CanvasPixel cp = canvas_pixel(C, gid, px, py);
                rng = seed + (unsigned)cp.G;
                rt_pcg_next(&rng);
                const RayOD r = primary_ray<PROJ>(C, seed, gid, cp, rng, false);
                o = r.o, d = r.d;
                reach = rt_inf();
                step = 0, tn = mk3(0, 0, 0);
                depth = 0;
                throughput = mk3(1, 1, 1);
#pragma unroll
                for (int g = 0; g < 4; g++) sums.g[g] = mk3(0, 0, 0);
            }
            if (__ballot(state != LT_DONE) == 0) break;  // every lane has folded its last pass
            // the one trace site: a round of whatever kind of ray each lane has under way
            int answer = LR_GOES_ON;
            Hit h;
            h.distance = reach;
            h.material = 0;
            h.normal = tn;
            h.color = f4{0, 0, 0, 0};
            h.emittance = 0;
            h.spec = 0;
            if (state != LT_DONE) {
                auto t = first_hit_args<LightOut>();
                answer = light_trace_round<TREE, BVH, GROUPS>(arg_copy(&t->S), o, d, t->draw_depth, h, dist_march, step, stack);
                tn = h.normal;
            }
            // what the answer means to the lane whose trace has ended: each continuation appears once
            const bool traced = state != LT_DONE && answer != LR_GOES_ON, hit = answer == LR_HIT;
            bool bounce = false, fold = false;
            const bool sky = traced && !hit;  // a main ray that left the world, or a sun ray that met nothing
            float sky_e = 1.0f;                         // record.emittance = 1 for the main ray (K/rayTracer.cl:95)
            if (traced && state == LT_MAIN) {
                if (!hit) {
                    fold = true;
                } else {  // applyRayColor — K/kernel.h:33-44
                    o = o + d * (h.distance - kOffset);  // closest_hit's point
                    n0 = h.normal;
                    const f3 c = mk3(h.color.x, h.color.y, h.color.z);
                    throughput = throughput * c;
                    auto s = first_hit_args<LightOut>();
                    light_hit_term(sums, c, h.emittance, s->out.emitter_scale, throughput);
                    light_groups_hit<GROUPS>(gid, h, c, throughput);
                    if (s->S.sun_flags & 1) {
                        // the shadow record is a copy of the main record, distance included, traced from the point with no offset
                        d = sun_sample(arg_copy(&s->S), rng);
                        reach = h.distance;
                        step = 0, tn = mk3(0, 0, 0);
                        state = LT_SUN;
                    } else {
                        bounce = true;
                    }
                }
            } else if (traced && state == LT_SUN) {
                sky_e = rt_fabs(dot(d, n0));  // the |dot(sun direction, normal)| stored at the ray's start (K/sky.h:90), evaluated where it is read
                bounce = true;
            }
            if (sky) {  // intersectSky, before the bounce overwrites d
                auto s = first_hit_args<LightOut>();
                const SkyTexels q = sky_fetch(arg_copy(&s->S), d);
                light_sky_terms(sums, arg_copy(&s->S), q, d, throughput, sky_e);
                light_groups_unlit<GROUPS>(gid, q, throughput, sky_e);
            }
            if (bounce) {  // nextPath — K/kernel.h:46-98
                d = diffuse_bounce(n0, rng);
                o = o + d * kOffset;
                depth += 1;
                reach = rt_inf();
                step = 0, tn = mk3(0, 0, 0);
                state = LT_MAIN;
                if (!(depth < first_hit_args<LightOut>()->out.max_depth)) fold = true;
            }
            start = false;
            if (fold) {  // K/rayTracer.cl:109-112
                const int spp = first_spp + k;
                const float fs = (float)spp, fs1 = (float)(spp + 1);
                auto w = first_hit_args<LightOut>();
#pragma unroll
                for (int g = 0; g < 4; g++) {
                    float* p = w->out.img[g] + 3 * (size_t)gid;
                    const float m0 = p[0], m1 = p[1], m2 = p[2];
                    p[0] = light_fold(m0, fs, sums.g[g].x, fs1);
                    p[1] = light_fold(m1, fs, sums.g[g].y, fs1);
                    p[2] = light_fold(m2, fs, sums.g[g].z, fs1);
                }
                light_groups_fold<GROUPS>(gid, n_pixels, fs, fs1);
                k += 1;
                start = k < n_passes;
                state = start ? LT_MAIN : LT_DONE;
            }
        }
    }
