// capi_run.hip — the host pass loop (the C++ counterpart of J/opencl/OpenClPathTracingRenderer.java).
#include "capi_internal.hpp"

extern "C" int chunky_render_run_ex(chunky_render* r, double* sample_buffer, int32_t* scene_spp, int32_t target_spp,
                                    int32_t merge_interval, const chunky_run_callbacks* callbacks) {
    if (!r || !r->ctx) return fail(CHUNKY_E_INVALID, "NULL render");
    if (!sample_buffer || !scene_spp) return fail(CHUNKY_E_INVALID, "render_run: NULL buffer");
    if (merge_interval < 1) merge_interval = 1024;  // OpenClPathTracingRenderer.java:158
    // the caller's struct may be older (shorter) than this library's: copy what it holds, the rest stays NULL
    chunky_run_callbacks cb{};
    if (callbacks) {
        const size_t have = callbacks->struct_size;
        if (have % sizeof(void*) != 0 || !take_versioned(callbacks, have, offsetof(chunky_run_callbacks, progress), &cb))
            return fail(CHUNKY_E_INVALID, "render_run_ex: callbacks->struct_size %zu (set it to sizeof(chunky_run_callbacks))", have);
    }
    const int64_t n = (int64_t)r->width * r->height * 3;
    std::vector<float> pass_buffer((size_t)n);
    JavaRandom rnd(0);                 // :95
    int logical_spp = *scene_spp;      // :91
    int samp_spp = *scene_spp;         // sceneSpp[0], :92
    auto last_callback = std::chrono::steady_clock::now();
    if (int rc = chunky_render_reset(r)) return rc;  // new float[] passBuffer uploaded with the buffer, :61,71
    // The launches below grow to what fits 95 ms.  Once the climb has shown where it is heading (a launch of 8 passes or more is
    // next), the staging array is sized ONCE for the launch size it will settle at instead of being regrown at every step; a
    // heavy scene that settles at a few passes never reserves anything.  The hint is dropped when the loop ends, however it ends.
    struct Reserve {
        chunky_render* r;
        void set(int passes) {
            std::lock_guard<std::recursive_mutex> g(r->ctx->mu);
            if (r->parts.empty()) r->reserve_passes = passes;
            for (chunky_render* part : r->parts) part->reserve_passes = passes;
        }
        ~Reserve() { set(0); }
    } reserve{r};
    int launch_passes = 1;             // adapts to ~95 ms per launch (below), so postRender is polled often enough
    while (logical_spp < target_spp) { // :102
        int buffer_spp = 0;            // bufferSppReal
        int until_merge = target_spp - logical_spp < merge_interval ? target_spp - logical_spp : merge_interval;
        bool stop = false, save = false, save_poll = false;
        while (buffer_spp < until_merge && !save) {
            int m = until_merge - buffer_spp < launch_passes ? until_merge - buffer_spp : launch_passes;
            if (cb.save_event)  // a snapshot / dump due inside the next launch, or a buffer to finalize, ends it there (:150)
                for (int k = 1; k <= m; k++)
                    if (const int ev = cb.save_event(cb.user, logical_spp + buffer_spp + k)) {
                        m = k;
                        save = true;
                        save_poll = ev != 2;  // a real save event is followed by one more poll (:179-182); shouldFinalizeBuffer alone is not
                        break;
                    }
            std::vector<int32_t> seeds((size_t)m);
            for (int k = 0; k < m; k++) seeds[(size_t)k] = rnd.next_int();  // :107
            auto t0 = std::chrono::steady_clock::now();
            if (int rc = chunky_render_passes(r, seeds.data(), m, buffer_spp)) return rc;
            if (int rc = chunky_render_sync(r)) return rc;                  // clWaitForEvents, :141
            auto t1 = std::chrono::steady_clock::now();
            buffer_spp += m;
            *scene_spp += m;                                                 // :144
            if (cb.progress) cb.progress(cb.user, *scene_spp);
            if (cb.regenerate_camera) cb.regenerate_camera(cb.user);         // :146-148
            double ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
            // passes per launch: as many as fit ~95 ms at the rate just measured (postRender is polled between launches, at least
            // every 100 ms where a launch allows it), at most eight times the last launch — a launch of few passes overstates
            // the time per pass (its fixed costs), so the sequence climbs 1, 8, 64, ... and settles; it comes down the same way
            {
                const double per_pass = ms / (double)m;
                int want = per_pass > 0.0 ? (int)(95.0 / per_pass) : kMaxPassesPerLaunch;  // a launch stays under the 100 ms of :153
                if (want > launch_passes * 8) want = launch_passes * 8;
                if (want > kMaxPassesPerLaunch) want = kMaxPassesPerLaunch;
                if (want < 1) want = 1;
                if (want > launch_passes || ms > 90.0) launch_passes = want;
                // where the climb is heading: the rate just measured says how many passes fit 95 ms
                // (a quarter more than the rate says: the next estimate differs by a few passes, and a launch larger than the array by ONE pass
                // regrows it — 4.4 GB and 240 ms of hipMalloc in the middle of a warm render, seen on configs[1])
                if (launch_passes >= 8) reserve.set(per_pass > 0.0 && 119.0 / per_pass < (double)merge_interval ? (int)(119.0 / per_pass) + 1 : merge_interval);
            }
            if (!save && cb.post_render && std::chrono::duration<double, std::milli>(t1 - last_callback).count() > 100.0 &&
                (!cb.poll_gate || cb.poll_gate(cb.user))) {  // :153-157; the gate is `!manager.shouldFinalize()` (:154)
                last_callback = t1;
                if (cb.post_render(cb.user)) {
                    stop = true;
                    break;
                }
            }
        }
        if (!stop && cb.post_render && cb.post_render(cb.user)) stop = true;  // :163
        if (stop && buffer_spp == 0) return fail(CHUNKY_E_ABORTED, "stopped by postRender");
        if (int rc = chunky_render_read(r, pass_buffer.data(), n)) return rc;  // :164-166
        const double sinv = 1.0 / (samp_spp + buffer_spp);                   // :169
        const double a = samp_spp, b = buffer_spp;
        {   // :172-177: the reference merges on Chunky's common worker threads; here a few host threads, each its own range
            auto merge = [&](int64_t lo, int64_t hi) {
                for (int64_t i = lo; i < hi; i++)                             // :173
                    sample_buffer[i] = (sample_buffer[i] * a + (double)pass_buffer[(size_t)i] * b) * sinv;
            };
            unsigned workers = std::thread::hardware_concurrency();
            workers = workers > 16 ? 16 : (workers < 1 ? 1 : workers);
            if (n < (int64_t)1 << 18) workers = 1;
            std::vector<std::thread> pool;
            const int64_t chunk = (n + workers - 1) / workers;
            for (unsigned w = 1; w < workers; w++) pool.emplace_back(merge, (int64_t)w * chunk < n ? (int64_t)w * chunk : n, (int64_t)(w + 1) * chunk < n ? (int64_t)(w + 1) * chunk : n);
            merge(0, chunk < n ? chunk : n);
            for (auto& t : pool) t.join();
        }
        samp_spp += buffer_spp;
        logical_spp += buffer_spp;                                            // :178
        if (cb.merged) cb.merged(cb.user, samp_spp);                          // :174-176
        if (stop) return fail(CHUNKY_E_ABORTED, "stopped by postRender");
        if (save_poll && cb.post_render && cb.post_render(cb.user)) return fail(CHUNKY_E_ABORTED, "stopped by postRender");  // :179-182
        // bufferSppReal = 0 (:170): the next pass runs with spp = 0, i.e. (mean*0 + c)/1 — no reset needed
    }
    return CHUNKY_OK;
}

extern "C" int chunky_render_run(chunky_render* r, double* sample_buffer, int32_t* scene_spp, int32_t target_spp,
                                 int32_t merge_interval, chunky_post_render_fn post_render, void* user) {
    const chunky_run_callbacks cb{sizeof(chunky_run_callbacks), post_render, nullptr, nullptr, nullptr, nullptr, user, nullptr};
    return chunky_render_run_ex(r, sample_buffer, scene_spp, target_spp, merge_interval, &cb);
}
