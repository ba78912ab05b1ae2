// pool_kernel.inc — the render_pool kernel template, included twice by render_pool.hip: as chunky::render_pool with
// CHUNKY_POOL_PROJ false (pinhole and pre-generated rays) and as chunky::proj::render_pool with it true (projected cameras,
// rt_device.hpp projected_ray).  One text, two kernels: the timed instantiations keep their code and registers exactly, and the
// projected camera runs every form they run.
// SORT: full cubes and model blocks are tested in phases of their own (on the re-laid-out tree, whose leaf entries say which a block is);
// plan_render (launch_plan.cpp) picks it for scenes with many model blocks
template <int TREE, int K, bool STATS, bool BVH = false, bool EXT = false, bool SORT = false>
__global__ void __launch_bounds__(256, ((STATS || EXT) ? 4 : (BVH ? CHUNKY_POOL_BVH_WAVES : CHUNKY_POOL_WAVES))) render_pool(CHUNKY_KERNEL_ARGS_HEAD WaveArgs unused_by_name) {
    constexpr int WORDS = CHUNKY_GLASS ? kPoolGlassWords : pool_words(EXT, BVH);  // 16-byte words of a parked path (pool_pack; launch_plan.hpp: the launch sizes the LDS with the same two functions)
    constexpr int END = BVH ? ST_TRACED : ST_SHADE;  // where a lane goes when the octree part of a trace ends
    // candidates sorted into full cubes (ST_BLOCK) and model blocks (ST_MODEL); not instantiated with entity BVHs or the extended
    // integrator (their pools are small: measured -4 % / -2 %)
    constexpr bool SPLIT = SORT;
    constexpr bool CONTINUES = CHUNKY_BLOCK_CONTINUES && !BVH && !EXT;  // the block test goes on where it hits (render_pool.hip block_continues)
    // upward rays end their march above the highest leaf that can be hit (path_state.hpp march_step): the plain kernels on the re-laid-out tree
    constexpr bool CAP = CHUNKY_MARCH_CAP && TREE != 0 && !BVH && !EXT;
    static_assert(!SORT || (TREE != 0 && !BVH && !EXT), "sorted block tests: the plain kernel on the re-laid-out tree only");
    extern __shared__ int lds[];
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
    PoolLds P{nullptr, nullptr, nullptr};
    PathStacks stacks{nullptr, 64 + K};
    {
        // per wave: K parked records, their tag / list scratch, then (BVH) one to-visit stack per path of the pool
        const unsigned depth = BVH ? fresh_args()->stack_bytes : 0u;  // entries per stack
        char* base = (char*)lds + wave * pool_wave_lds_bytes(K, WORDS, depth);
        P.park = (uint4*)base;
        P.tags = (int*)(base + K * 16 * WORDS);
        P.list = P.tags + K;
        stacks.base = (int*)(base + K * 16 * WORDS + K * 8);
        // every parked slot starts fresh (depth 255 in its flag word); with entity BVHs it also owns a to-visit stack
        if (lane < K) P.park[lane] = make_uint4(0u, 0u, kFreshDepth | (WORDS <= 7 ? 0u : (unsigned)(64 + lane) << 16), 0u);
    }
    LdsStack stack{lds, 0};  // render_waves' per-lane stacks are not used here
    LaneState L;
    L.h.material = 0;
    L.h.normal = mk3(0, 0, 0);
    L.h.color = f4{0, 0, 0, 0};
    L.h.emittance = 0;
    L.h.distance = 0;
    L.cand_data = 0;
    L.cand_level = 0;
    L.pass = 0;
    L.gid = -1;
    L.sidx = 0;
    L.pid = lane;
    L.tkind = 0;
    L.after_nee = false;
#if CHUNKY_FOG
    L.medium = false;
#endif
#if CHUNKY_GLASS
    L.crossings = 0;
    L.rm = L.rm_vertex = 0;
    L.clip = 0;
    L.n_vertex = L.o_vertex = mk3(0, 0, 0);
#endif
    L.pend = mk3(0, 0, 0);
    L.h.spec = 0;
    L.mean = mk3(0, 0, 0);
    L.slot = 0;
    L.serial = 0;
    L.steps = 0;
    L.rng = 0;
    L.depth = kFreshDepth;
    L.shadow = false;
    L.dist_march = 0;
    L.radiance = mk3(0, 0, 0);
    L.throughput = mk3(0, 0, 0);
    L.o = L.d = L.inv = L.far = mk3(0, 0, 0);
    L.oct_hit = false;
    L.trace_hit = false;
    L.bvh_cur = L.bvh_top = L.bvh_which = L.bvh_head = 0;
    L.bvh_base = nullptr;
    L.bvh_dist = 0;
    unsigned long long prof[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long swap_rounds = 0, swapped = 0;
    unsigned long long above = 0;  // (STATS) march lane-steps of upward rays at or above S.hit_top
    PartTimers parts{{0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, 0};
    unsigned long long t_begin = 0;
    if (STATS) t_begin = __builtin_amdgcn_s_memtime();
    XcdClaim claim{xcd_first_range(), 0u, 0u};
    int ranges_tried = 0;  // ranges this wave has found empty
    int st = ST_SHADE;  // fresh (L.depth == kFreshDepth): the first SHADE execution hands out samples
    int ptag = lane < K ? ST_SHADE : ST_DONE;
    wave_lds_fence();
    // the pool's census: paths waiting for each phase, in lanes and parked (taken at the END of an iteration, so that the loop has
    // one exit, at its head: a break in mid-loop makes the compiler define every loop-carried scalar on the exit path, with
    // v_readfirstlane of nothing, in every iteration)
    int c_march = 0, c_block = 0, c_shade = 0, c_bvh = 0, c_leaf = 0, c_model = 0;
    int model_age = 0;  // iterations since model blocks were last tested
    auto census = [&]() {
        if (BVH && __ballot(st == ST_TRACED)) {  // octree part of some traces just ended: entity BVHs next
            const SceneView S = arg_copy(&fresh_args()->S);
            if (st == ST_TRACED) st = rbvh_begin(S, L);
        }
        c_march = count_lanes(st == ST_MARCH) + count_lanes(ptag == ST_MARCH);
        c_block = count_lanes(st == ST_BLOCK) + count_lanes(ptag == ST_BLOCK);
        c_shade = count_lanes(st == ST_SHADE) + count_lanes(ptag == ST_SHADE);  // (fresh paths included)
        c_model = SPLIT ? count_lanes(st == ST_MODEL) + count_lanes(ptag == ST_MODEL) : 0;
        c_bvh = BVH ? count_lanes(st == ST_BVH) + count_lanes(ptag == ST_BVH) : 0;
        c_leaf = BVH ? count_lanes(st == ST_LEAF) + count_lanes(ptag == ST_LEAF) : 0;
    };
    census();
    while ((c_march | c_block | c_shade | c_bvh | c_leaf | c_model) != 0) {  // until every lane and every slot is ST_DONE
        // at most 64 paths run at once; among phases that can fill the wave SHADE and BLOCK go first (they feed the march)
        const int v_march = (c_march < 64 ? c_march : 64) * kWMarch, v_block = (c_block < 64 ? c_block : 64) * kWBlock,
                  v_shade = (c_shade < 64 ? c_shade : 64) * kWShade;
        // (written as integer arithmetic: as a chain of ?: on wave-uniform bools the compiler routes the choice through a VGPR)
        int X = (int)((unsigned)(v_march - v_block - 1) >> 31);  // 1 when v_block >= v_march, else 0
        int v_best = v_block > v_march ? v_block : v_march;
        if (v_shade >= v_best) {
            X = 2;
            v_best = v_shade;
        }
        if (SPLIT) {
            // Model blocks are a phase of their own: their tests cost three times the cube test, and the wave pays for them whenever ONE
            // lane has a model block.  How long they wait for company: a batch of T paths costs one execution per T arrivals, and
            // T / 2 slots of the pool while it gathers — the sum is least at T ~ sqrt(arrival rate), and with the rate estimated as
            // (waiting) / (iterations since the last execution) that is: run once waiting x iterations reaches a constant.  Where model
            // blocks are common (the city: 7 arrive per iteration) a wave's worth gathers first; where they are rare (the indoor room:
            // one in 40 iterations) three or four go together.
            const int v_model = (c_model < 64 ? c_model : 64) * kWModel;
            model_age += 1;
            if (v_model > v_best || c_model * model_age >= kModelFire) {
                X = ST_MODEL;
                v_best = v_model > v_best ? v_model : v_best;
                model_age = 0;
            }
        }
        if (BVH) {  // the walk through the entity BVHs (inner-node and leaf visits together) is one class of the pool
            const int c_walk = c_bvh + c_leaf;
            const int v_walk = (c_walk < 64 ? c_walk : 64) * kWWalk;
            if (v_walk > v_best) { X = 5; v_best = v_walk; }
        }
        unsigned long long t0 = 0;
        if (STATS) t0 = __builtin_amdgcn_s_memtime();
        if (K > 0) {
            const int n = pool_swap<K, WORDS>(P, L, st, ptag, X, lane);
            if (STATS && n) {
                swap_rounds += 1;
                swapped += (unsigned long long)n;
            }
        }
        if (STATS) {  // parts 4, 5, 6 of the profile: cycles in swaps, loop iterations, entries into the march loop
            parts.t[PT_FOLD] += __builtin_amdgcn_s_memtime() - t0;
            parts.t[PT_OPEN] += 1;
            parts.t[PT_HANDOUT] += X == 0 ? 1 : 0;
        }
        int n_exec = 0;
        // The phases are consecutive ifs, not one if / else-if chain, and X is made opaque between them (CHUNKY_PHASE_END): each phase
        // then updates the path state where it lives.  As alternatives of one chain the phases' results met in a join behind them, and
        // because the compiler lays the alternatives out one after the other — every later one reachable, as far as it can tell, from
        // the ones before — the state a later phase reads had to stay intact while an earlier one ran: SHADE and BLOCK copied the state
        // out of the loop's registers on entry (20 and 16 v_mov_b32), worked on the copies, and a block behind them moved all of it
        // back (28) — tools/isa_copies.py.  Exactly one of the ifs runs per iteration, as before.
        if (X == 0) {
            WaveArgPtr A = fresh_args();
            const SceneView Sm = arg_copy(&A->S);
            const RenderOpts Om = arg_copy(&A->O);
            const LaneMask entered = __ballot(st == ST_MARCH);
            int nm = __popcll(entered);
            n_exec = nm;
            const int parked_march = c_march - nm;  // marchers still parked after the swap
            // The wave stays in the march while it runs fuller than anything else could: lanes that leave join the paths
            // waiting for BLOCK or SHADE (`other` of them already), so it leaves once nm would drop below the larger of those
            // crowds — at worst every leaver joins it: nm < other + (n0 - nm) — or once enough lanes are free for a refill
            // from the parked marchers.  One bound, fixed on entry: the loop's bookkeeping is one popcount and one compare.
            const int other_b = c_block < 64 ? c_block : 64, other_s = c_shade < 64 ? c_shade : 64;
            int other = other_b > other_s ? other_b : other_s;
            if (SPLIT) {
                const int other_m = c_model < 64 ? c_model : 64;
                other = other > other_m ? other : other_m;
            }
            // (with entity BVHs the walkers are not counted: they are the pool's standing crowd and wait in any case)
            int stay = (other + nm + 1) >> 1;
            // ... and longer still when hardly any marcher is parked (fewer than kStayFewParked): leaving then means a swap round and a phase
            // that cannot be refilled afterwards, so the march goes on kStayLonger lanes emptier before it hands over.  Measured on the final
            // loop (round 6, after the iteration overhead fell): threshold x lanes 12 x 16 = 7 510 / 3 930 / 4 080 Msamples/s on headline / city /
            // indoor against 7 250 / 3 740 / 4 065 without; unconditional (-12 lanes) 7 430 / 3 880 / 4 010 — a scene whose pool is full of
            // marchers (the indoor room) is better off leaving early and refilling.
            // (with entity BVHs the pool is small and the walkers are its standing crowd: 6 lanes — 16 there costs the city with its entities 7 %)
            if (parked_march < kStayFewParked) stay -= BVH ? kStayLongerBvh : kStayLonger;
            if (K > 0 && parked_march >= kPoolRefill && stay < 65 - kPoolRefill) stay = 65 - kPoolRefill;
            if (stay < 1) stay = 1;
            LaneMask marching = entered, to_block = 0;
            // the exit-plane selectors (1.0 where the ray runs towards +axis) as three registers for the length of the loop — they
            // are not part of a parked path; as three lane masks they cost three v_cndmask per step (round 6: +0.9 %)
            L.far = far_of(L.inv);
            const LaneMask* far_masks = nullptr;
            int data, level, entry = 0;
            // a direction component that is exactly -0 (inv = -inf) is the one case in which the leaf exit has to guard against a
            // NaN (leaf_exit_distance): as good as never does a marching lane of the wave have one, and the loop then runs
            // without the three guards (+0.7 % on the bench)
            const float ninf = -rt_inf();
            const bool guard = ((__ballot(L.inv.x == ninf) | __ballot(L.inv.y == ninf) | __ballot(L.inv.z == ninf)) & entered) != 0;  // (masks on the scalar unit)
            if (guard)
                march_loop<TREE, true, STATS, CAP>(Sm, Om, L, marching, to_block, data, level, nm, stay, far_masks, prof, SPLIT ? &entry : nullptr, &above);
            else
                march_loop<TREE, false, STATS, CAP>(Sm, Om, L, marching, to_block, data, level, nm, stay, far_masks, prof, SPLIT ? &entry : nullptr, &above);
            const bool found = in_mask(to_block);
            L.cand_data = found ? data : L.cand_data;
            L.cand_level = found ? level : L.cand_level;
            const int st_found = SPLIT && (entry & 0x2000000) ? ST_MODEL : ST_BLOCK;  // bit 25 of a leaf entry: a model block (widetree.hpp kWideKindLow)
            st = found ? st_found : (in_mask(entered & ~marching & ~to_block) ? END : st);
            if (STATS) {
                prof[0] -= 1;
                prof[1] -= (unsigned long long)n_exec;
            }
        }
        CHUNKY_PHASE_END(X, "march");
        if (X == 1) {
            n_exec = count_lanes(st == ST_BLOCK);
            const SceneView S = arg_copy(&fresh_args()->S);
            if (st == ST_BLOCK) {
                st = block_phase<TREE, END, false, SPLIT ? kBlockCubes : kBlockAny, WORDS == 6>(S, L);
                if constexpr (CONTINUES) block_continues<END, WORDS>(S, L, st);  // a hit starts its shadow ray or bounce here (render_pool.hip)
            }
        }
        CHUNKY_PHASE_END(X, "block");
        if (SPLIT && X == ST_MODEL) {
            n_exec = count_lanes(st == ST_MODEL);
            if (STATS) parts.t[8] += (unsigned long long)n_exec + (1ull << 40);  // value 22 of the profile: lanes, and executions in bits 40 up
            const SceneView S = arg_copy(&fresh_args()->S);
            asm volatile("; chunky-mark models");  // (comments in the compiled kernel: tools/isa_scratch.py finds the model blocks' phase by them)
            if (st == ST_MODEL) {
                st = block_phase<TREE, END, false, kBlockModels, WORDS == 6>(S, L);
                if constexpr (CONTINUES) block_continues<END, WORDS>(S, L, st);
            }
            asm volatile("; chunky-mark models-end");
        }
        CHUNKY_PHASE_END(X, "model-blocks");
        if (BVH && X == 5) {
            // The walk: inner-node visits and triangle tests are one step function (rwalk_step: the same four 16-byte reads
            // from one array or the other), so a walker is ST_BVH throughout and the loop below counts that one state.  The
            // wave stays while enough walkers remain, or until enough lanes are free for a refill from parked walkers.
            const SceneView S = arg_copy(&fresh_args()->S);
            int nw = count_lanes(st == ST_BVH);
            n_exec = nw;
            const int parked_walk = c_bvh + c_leaf - nw;
            // The walk is nine tenths of the work in a scene with entities and everything else is cheap beside it: the other
            // phases are served as soon as a small crowd waits for them (vote weight kWWalk against 4), so that the pool stays
            // full of walkers; the wave leaves the walk when kWalkLeave lanes have finished theirs (they wait for SHADE now),
            // or when that many are free and parked walkers can take their place.
            int stay = nw - kWalkLeave + 1;
            if (K > 0 && parked_walk > 0) {
                const int refill = parked_walk < kWalkLeave ? parked_walk : kWalkLeave;
                if (stay < 65 - refill) stay = 65 - refill;
            }
            if (stay < 1) stay = 1;
            do {
                if (STATS) {
                    prof[3] += 1;
                    prof[4] += (unsigned long long)nw;
                }
                if (st == ST_BVH) st = rwalk_step(S, L, stacks);
                nw = count_lanes(st == ST_BVH);
            } while (nw >= stay);
            if (STATS) {
                prof[3] -= 1;
                prof[4] -= (unsigned long long)n_exec;
            }
        }
        CHUNKY_PHASE_END(X, "walk");
        if (X == 2) {
            n_exec = count_lanes(st == ST_SHADE);
            // Every vector load of the phases before has been waited for on the path that was taken, but not on every path the compiler
            // sees (a pre-generated ray's two loads are waited for in trace_setup, a block it cannot tell every lane with a new ray enters):
            // what it still counts as outstanding here it would wait for at the first touch of the register — in the middle of the
            // sampling block, with SHADE's own sky texels in the queue behind it (vector memory operations retire in order).  One
            // s_waitcnt vmcnt(0) here resets that.  It is not provably free — the counter also holds stores, such as the staging stores of
            // the SHADE before — but measured it is a net gain on all four configurations (EXPERIMENTS 7.2: headline +0.5 %).
            __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0), the other counters at their maximum
            WaveArgPtr A = fresh_args();
            const SceneView S = arg_copy(&A->S);
            const RenderOpts O = arg_copy(&A->O);
            const bool served = st == ST_SHADE;
            bool fresh = served && L.depth == kFreshDepth;  // holds no path: wants a sample
            if (served && !fresh) {
                if (WORDS == 6) march_registers_to_hit(L);
                st = EXT ? shade_phase_ext<TREE, BVH>(S, O, L) : shade_phase<TREE, BVH, STATS>(S, O, L, stack, &parts);
            }
            part_begin<STATS>(&parts);
            // what the deposit and the new-sample section read of the launch arguments: one burst of scalar loads, one wait (path_state.hpp sample_args)
            const SampleArgs N = sample_args<CHUNKY_POOL_PROJ>(A);
            if (st == ST_NEXT) {  // the path is finished: its radiance waits in the staging array for fold_kernel
                // streamed past the caches (nt): written once, read once by fold_kernel; the L2 stays with the tree
                float* __restrict__ out = N.staging + 3 * (size_t)(unsigned)L.sidx;
#if CHUNKY_STAGING_STORE == 1  // tuning builds (tools/variants.sh): plain stores, merged by the L2 (-2.3 % on the bench)
                out[0] = L.radiance.x, out[1] = L.radiance.y, out[2] = L.radiance.z;
#elif CHUNKY_STAGING_STORE == 2  // device-scope stores (sc1): written through the L2
                __hip_atomic_store(out, L.radiance.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(out + 1, L.radiance.y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(out + 2, L.radiance.z, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#elif CHUNKY_STAGING_STORE == 3  // system-scope stores (sc0 sc1)
                __hip_atomic_store(out, L.radiance.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                __hip_atomic_store(out + 1, L.radiance.y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                __hip_atomic_store(out + 2, L.radiance.z, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
#else
                __builtin_nontemporal_store(L.radiance.x, out);
                __builtin_nontemporal_store(L.radiance.y, out + 1);
                __builtin_nontemporal_store(L.radiance.z, out + 2);
#endif
                fresh = true;
            }
            part_end<STATS>(&parts, PT_DEPOSIT);
            // ---- new samples (K/rayTracer.cl:55-91).  Sample index = (tile of kSampleTile pixel slots, pass, slot in tile): a
            //      tile gets all its passes before the next tile starts, so the paths in flight on the whole GPU cover a few
            //      thousand neighbouring pixels — a part of the scene that stays in the 4 MB L2s (pass-major order spread
            //      them over a third of the image: L2 hit rate 91 %, 66 GB of fabric reads per launch instead of 4) ----
            const bool need = fresh;
            const unsigned sidx = xcd_claim(N.next + kXcdCounters, claim, ranges_tried, need, N.xcd_stripe, N.n_samples);  // convergent
            if (need && sidx != kClaimNone) {
                if (sidx >= N.n_samples) {
                    st = ST_DONE;
                    fresh = false;
                } else {
                    // sidx = ((tile * sub-blocks per tile + sub-block) * passes + pass) * kSubBlock + slot in the sub-block
                    const unsigned per_sub = (unsigned)N.n_passes * (unsigned)kSubBlock;
                    const unsigned sub = fast_quotient(sidx, N.div_sub), rem = sidx - sub * per_sub;  // sub = tile * (kSampleTile / kSubBlock) + sub-block
                    const unsigned pass = rem / (unsigned)kSubBlock;
                    // The pass's seed is requested as soon as the pass is known and waited for where rng is formed: the pixel decode runs under
                    // the load.  A padding slot (gid outside the image) fetches a seed it discards — the index is inside P.seed / seeds_dev
                    // for every sample index below n_samples, because pass < P.n.
                    const unsigned seed = (unsigned)(N.seeds_dev ? N.seeds_dev[pass] : A->P.seed[pass]);  // (seeds_dev is wave-uniform: launches longer than P.seed holds)
                    const int slot = (int)(sub * (unsigned)kSubBlock + (rem & (unsigned)(kSubBlock - 1)));
                    const SlotPixel px = pool_slot_pixel(N.T, N.C.width, N.C.height, slot, N.div_bw);
                    const int gid = px.gid;
                    if (gid < N.C.width * N.C.height) {  // else: a padding slot, nothing to render (the lane claims again)
                        const CanvasPixel cp = canvas_pixel(N.C, gid, px.x, px.y);  // (the identity unless the target is a window)
                        unsigned rng = seed + (unsigned)cp.G;
                        rt_pcg_next(&rng);
                        const RayOD pr = primary_ray<CHUNKY_POOL_PROJ>(N.C, seed, gid, cp, rng, false);
                        L.sidx = (int)sidx;
                        L.rng = rng;
                        L.o = pr.o;
                        L.d = pr.d;
                        L.radiance = mk3(0, 0, 0);
                        L.throughput = mk3(1, 1, 1);
                        L.depth = 0;
                        L.shadow = false;
                        L.tkind = 0;
                        L.after_nee = false;
#if CHUNKY_GLASS
                        L.crossings = 0;  // at the camera: inside no run
                        L.rm = L.rm_vertex = 0;
#endif
                        L.h.distance = rt_inf();
                        st = ST_SETUP;
                        fresh = false;
                    }
                }
            }
            part_end<STATS>(&parts, PT_NEWSAMPLE);
            if (fresh) {  // no sample this time (the tail of a batch, a padding slot): it asks again at the next SHADE
                st = ST_SHADE;
                L.depth = kFreshDepth;
            }
            if (st == ST_SETUP) st = trace_setup<END, false>(S, L);
            part_end<STATS>(&parts, PT_SETUP);
        }
        CHUNKY_PHASE_END(X, "shade");
        if (STATS) {
            const unsigned long long dt = __builtin_amdgcn_s_memtime() - t0;
#pragma unroll
            for (int k = 0; k < 3; k++)
                if (X == k) {
                    prof[3 * k] += 1;
                    prof[3 * k + 1] += (unsigned long long)n_exec;
                    prof[3 * k + 2] += dt;
                }
            if (X == ST_MODEL) parts.t[9] += dt;  // the model blocks' phase: value 23 of the profile
            if (X == 5) {  // the entity-BVH walk is profiled with BLOCK
                prof[3] += 1;
                prof[4] += (unsigned long long)n_exec;
                prof[5] += dt;
            }
        }
        census();
    }
    if (STATS && lane == 0) {
        unsigned long long* stats = fresh_args()->stats;
        for (int k = 0; k < 9; k++) atomicAdd(&stats[k], prof[k]);
        const unsigned long long life = __builtin_amdgcn_s_memtime() - t_begin;
        atomicAdd(&stats[9], life);
        atomicMax(&stats[10], life);
        atomicAdd(&stats[11], 1ull);
        atomicAdd(&stats[12], swap_rounds);
        atomicAdd(&stats[13], swapped);
        for (int k = 0; k < 10; k++) atomicAdd(&stats[14 + k], parts.t[k]);
        atomicAdd(&stats[24], above);  // chunky_render_march_above
    }
}
