// adaptive_host.cpp — adaptive sampling on the host: the specification loops (adaptive_spec.h) and the checks of a caller's params
// and state.  Plain C++: no device code, no HIP type.
#include "adaptive_host.hpp"

#include <cmath>
#include <cstring>
#include <vector>

#include "adaptive_spec.h"
#include "capi_error.hpp"

// The threshold is an UNMEASURED PLACEHOLDER: tools/adaptive_bench.py, which is to choose it, has not been run on a device yet
// 
constexpr float kAdaptiveThreshold = 0.05f, kAdaptiveFloor = 0.01f;
constexpr int kAdaptiveMinSpp = 16, kAdaptiveInterval = 16;

extern "C" int chunky_adaptive_default_params(chunky_adaptive_params* p) {
    if (!p) return fail(CHUNKY_E_INVALID, "adaptive_default_params: NULL params");
    p->size = sizeof(chunky_adaptive_params);
    p->threshold = kAdaptiveThreshold;
    p->floor = kAdaptiveFloor;
    p->min_spp = kAdaptiveMinSpp;
    p->check_interval = kAdaptiveInterval;
    p->flags = 0;
    p->reserved = 0;
    return CHUNKY_OK;
}

int adaptive_params(const char* who, const chunky_adaptive_params* params, int max_spp, chunky_adaptive_params* p) {
    if (!params) return fail(CHUNKY_E_INVALID, "%s: NULL params", who);
    constexpr size_t kFirst = offsetof(chunky_adaptive_params, flags) + sizeof(uint32_t);  // the first version of the struct
    if (!take_versioned(params, params->size, kFirst, p)) return fail(CHUNKY_E_INVALID, "%s: params.size %zu is smaller than the struct (%zu)", who, params->size, kFirst);
    if (!std::isfinite(p->threshold) || p->threshold < 0.0f) return fail(CHUNKY_E_INVALID, "%s: threshold must be finite and >= 0, got %g", who, (double)p->threshold);
    if (!std::isfinite(p->floor) || !(p->floor > 0.0f)) return fail(CHUNKY_E_INVALID, "%s: floor must be finite and > 0, got %g", who, (double)p->floor);
    if (p->min_spp < 2) return fail(CHUNKY_E_INVALID, "%s: min_spp %d < 2", who, p->min_spp);
    if (p->check_interval < 1) return fail(CHUNKY_E_INVALID, "%s: check_interval %d < 1", who, p->check_interval);
    if (p->flags) return fail(CHUNKY_E_INVALID, "%s: unknown flags 0x%x", who, p->flags);
    if (max_spp < p->min_spp) return fail(CHUNKY_E_INVALID, "%s: %d passes are fewer than min_spp %d", who, max_spp, p->min_spp);
    return CHUNKY_OK;
}

extern "C" int chunky_adaptive_host(int width, int height, const float* samples, int n, const chunky_adaptive_params* params,
                                    int32_t* count_out, float* mean_out, float* stat_out) {
    chunky_adaptive_params p;
    if (int rc = adaptive_params("adaptive_host", params, n, &p)) return rc;
    if (width <= 0 || height <= 0 || (int64_t)width * height > INT32_MAX / 16) return fail(CHUNKY_E_INVALID, "adaptive_host: bad size %dx%d", width, height);
    if (!samples) return fail(CHUNKY_E_INVALID, "adaptive_host: NULL samples");
    const size_t np = (size_t)width * height;
    const float t2 = p.threshold * p.threshold;
    std::vector<float> mean(3 * np, 0.0f), stat(2 * np, 0.0f);
    std::vector<int32_t> count(np, 0);
    std::vector<unsigned char> active(np, 1), unconv(np, 0);
    size_t n_active = np;
    int done = 0;
    while (done < n && n_active > 0) {
        const float* s = samples + 3 * np * (size_t)done;
        for (size_t i = 0; i < np; i++) {
            if (!active[i]) continue;
            for (int c = 0; c < 3; c++) mean[3 * i + c] = ad_mean(mean[3 * i + c], s[3 * i + c], done);
            ad_welford(ad_luma(s[3 * i], s[3 * i + 1], s[3 * i + 2]), done, &stat[2 * i], &stat[2 * i + 1]);
        }
        done += 1;
        if (!ad_check_due(done, p.min_spp, p.check_interval, n)) continue;
        for (size_t i = 0; i < np; i++) unconv[i] = (unsigned char)(active[i] && ad_unconverged(stat[2 * i], stat[2 * i + 1], done, t2, p.floor));
        for (int y = 0; y < height; y++)
            for (int x = 0; x < width; x++) {
                const size_t i = (size_t)y * width + x;
                if (!active[i]) continue;
                int any = 0;
                for (int yy = y > 0 ? y - 1 : y; yy <= (y < height - 1 ? y + 1 : y); yy++)
                    for (int xx = x > 0 ? x - 1 : x; xx <= (x < width - 1 ? x + 1 : x); xx++) any |= unconv[(size_t)yy * width + xx];
                if (!any) {
                    active[i] = 0;
                    count[i] = done;
                    n_active -= 1;
                }
            }
    }
    for (size_t i = 0; i < np; i++)
        if (active[i]) count[i] = done;
    if (count_out) memcpy(count_out, count.data(), np * sizeof(int32_t));
    if (mean_out) memcpy(mean_out, mean.data(), 3 * np * sizeof(float));
    if (stat_out) memcpy(stat_out, stat.data(), 2 * np * sizeof(float));
    return CHUNKY_OK;
}

int adaptive_callbacks(const char* who, const chunky_adaptive_callbacks* callbacks, chunky_adaptive_callbacks* cb) {
    memset(cb, 0, sizeof *cb);
    if (!callbacks) return CHUNKY_OK;
    const size_t have = callbacks->struct_size;
    if (have % sizeof(void*) != 0 || !take_versioned(callbacks, have, offsetof(chunky_adaptive_callbacks, round_done), cb))
        return fail(CHUNKY_E_INVALID, "%s: callbacks->struct_size %zu (set it to sizeof(chunky_adaptive_callbacks))", who, have);
    return CHUNKY_OK;
}

bool same_adaptive_params(const chunky_adaptive_params& a, const chunky_adaptive_params& b) {
    return a.threshold == b.threshold && a.floor == b.floor && a.min_spp == b.min_spp && a.check_interval == b.check_interval;
}

// ---- the state of a run and its continuation on the host (include/chunky_hip.h, "adaptive sampling that stops and continues")
void adaptive_empty_state(int width, int height, const chunky_adaptive_params& p, chunky_adaptive_state* s) {
    memset(s, 0, sizeof *s);
    s->size = sizeof *s;
    s->width = width;
    s->height = height;
    s->active = width * height;
    s->params = p;
}

int adaptive_dims(const char* who, int width, int height) {
    if (width <= 0 || height <= 0 || (int64_t)width * height > INT32_MAX / 16) return fail(CHUNKY_E_INVALID, "%s: bad size %dx%d", who, width, height);
    return CHUNKY_OK;
}

int adaptive_state_valid(const char* who, const chunky_adaptive_state* st, const int32_t* count, const uint8_t* active, chunky_adaptive_state* s) {
    if (!st || !count || !active) return fail(CHUNKY_E_INVALID, "%s: NULL argument", who);
    if (!take_versioned(st, st->size, kAdaptiveStateFirst, s)) return fail(CHUNKY_E_INVALID, "%s: state.size %zu is smaller than the struct (%zu)", who, st->size, kAdaptiveStateFirst);
    if (int rc = adaptive_dims(who, s->width, s->height)) return rc;
    chunky_adaptive_params p;
    if (int rc = adaptive_params(who, &s->params, INT32_MAX, &p)) return rc;
    s->params = p;
    if (s->passes < 0) return fail(CHUNKY_E_INVALID, "%s: %d passes", who, s->passes);
    const int g = ad_grid_floor(s->passes, p.min_spp, p.check_interval);
    const int before = g == s->passes ? ad_grid_before(g, p.min_spp, p.check_interval) : g;  // (no grid point <= passes: g = 0 = before)
    if (s->last_check != g && s->last_check != before)
        return fail(CHUNKY_E_INVALID, "%s: last_check %d after %d passes (min_spp %d, check_interval %d: %d%s%d)", who, s->last_check, s->passes, p.min_spp,
                    p.check_interval, g, g == before ? " = " : " or ", before);
    const size_t np = (size_t)s->width * s->height;
    int64_t ones = 0, samples = 0;
    for (size_t i = 0; i < np; i++) {
        if (active[i] > 1) return fail(CHUNKY_E_INVALID, "%s: active[%zu] is %d, not 0 or 1", who, i, (int)active[i]);
        if (active[i]) {
            if (count[i] != s->passes) return fail(CHUNKY_E_INVALID, "%s: pixel %zu is active with count %d after %d passes", who, i, count[i], s->passes);
            ones += 1;
        } else if (!ad_on_grid(count[i], p.min_spp, p.check_interval) || count[i] > s->last_check) {
            return fail(CHUNKY_E_INVALID, "%s: pixel %zu is inactive with count %d, which is no check point up to the last check (%d)", who, i, count[i], s->last_check);
        }
        samples += count[i];
    }
    if (ones != s->active) return fail(CHUNKY_E_INVALID, "%s: state.active is %d, the map holds %lld active pixels", who, s->active, (long long)ones);
    // (a round has at least one pass and a check its own grid point: the continuation indexes summary.active with checks and counts both up)
    if (s->summary.rounds < 0 || s->summary.rounds > s->passes || s->summary.checks < 0 || s->summary.checks > s->passes)
        return fail(CHUNKY_E_INVALID, "%s: summary.rounds %d, summary.checks %d after %d passes", who, s->summary.rounds, s->summary.checks, s->passes);
    if (s->summary.passes != s->passes) return fail(CHUNKY_E_INVALID, "%s: summary.passes %d, passes %d", who, s->summary.passes, s->passes);
    if (s->summary.samples != samples) return fail(CHUNKY_E_INVALID, "%s: summary.samples %lld, the counts add up to %lld", who, (long long)s->summary.samples, (long long)samples);
    return CHUNKY_OK;
}

extern "C" int chunky_adaptive_state_check(const chunky_adaptive_state* st, const int32_t* count, const uint8_t* active) {
    chunky_adaptive_state s;
    return adaptive_state_valid("adaptive_state_check", st, count, active, &s);
}

extern "C" int chunky_adaptive_host_begin(int width, int height, const chunky_adaptive_params* params, chunky_adaptive_state* st, int32_t* count,
                                          float* mean, float* stat, uint8_t* active) {
    chunky_adaptive_params p;
    if (int rc = adaptive_params("adaptive_host_begin", params, INT32_MAX, &p)) return rc;
    if (int rc = adaptive_dims("adaptive_host_begin", width, height)) return rc;
    if (!st || !count || !mean || !stat || !active) return fail(CHUNKY_E_INVALID, "adaptive_host_begin: NULL argument");
    if (st->size < kAdaptiveStateFirst)
        return fail(CHUNKY_E_INVALID, "adaptive_host_begin: st->size %zu is smaller than the struct (%zu): set it to sizeof(chunky_adaptive_state)", st->size, kAdaptiveStateFirst);
    const size_t np = (size_t)width * height;
    chunky_adaptive_state s;
    adaptive_empty_state(width, height, p, &s);
    give_versioned(s, st);
    memset(count, 0, np * sizeof(int32_t));
    memset(mean, 0, 3 * np * sizeof(float));
    memset(stat, 0, 2 * np * sizeof(float));
    memset(active, 1, np);
    return CHUNKY_OK;
}

extern "C" int chunky_adaptive_host_resume(chunky_adaptive_state* st, const float* samples, int n, int32_t* count, float* mean, float* stat,
                                           uint8_t* active) {
    chunky_adaptive_state s;
    if (int rc = adaptive_state_valid("adaptive_host_resume", st, count, active, &s)) return rc;
    if (!mean || !stat) return fail(CHUNKY_E_INVALID, "adaptive_host_resume: NULL argument");
    if (n < 0 || (n > 0 && !samples) || n > INT32_MAX - s.passes) return fail(CHUNKY_E_INVALID, "adaptive_host_resume: %d more passes after %d", n, s.passes);
    const chunky_adaptive_params& p = s.params;
    const int width = s.width, height = s.height, first = s.passes, max_spp = s.passes + n;
    const size_t np = (size_t)width * height;
    const float t2 = p.threshold * p.threshold;
    std::vector<unsigned char> unconv(np, 0);
    while (s.passes < max_spp && s.active > 0) {
        const ad_step_t step = ad_step(s.passes, s.last_check, p.min_spp, p.check_interval, max_spp);
        // (The fold and the check below are written out a second time on purpose: chunky_adaptive_host above stays as it was, the
        // independent single run that P1 and P2 hold this loop to.)
        for (int k = 0; k < step.round; k++) {  // (no pass when the step is the check the earlier run did not make)
            const int spp = s.passes + k;
            const float* c = samples + 3 * np * (size_t)(spp - first);
            for (size_t i = 0; i < np; i++) {
                if (!active[i]) continue;
                for (int ch = 0; ch < 3; ch++) mean[3 * i + ch] = ad_mean(mean[3 * i + ch], c[3 * i + ch], spp);
                ad_welford(ad_luma(c[3 * i], c[3 * i + 1], c[3 * i + 2]), spp, &stat[2 * i], &stat[2 * i + 1]);
            }
        }
        s.summary.samples += (int64_t)s.active * step.round;
        s.passes += step.round;
        if (step.round > 0) s.summary.rounds += 1;
        if (!step.check_first && !ad_check_due(s.passes, p.min_spp, p.check_interval, max_spp)) continue;
        for (size_t i = 0; i < np; i++) unconv[i] = (unsigned char)(active[i] && ad_unconverged(stat[2 * i], stat[2 * i + 1], s.passes, t2, p.floor));
        for (int y = 0; y < height; y++)
            for (int x = 0; x < width; x++) {
                const size_t i = (size_t)y * width + x;
                if (!active[i]) continue;
                int any = 0;
                for (int yy = y > 0 ? y - 1 : y; yy <= (y < height - 1 ? y + 1 : y); yy++)
                    for (int xx = x > 0 ? x - 1 : x; xx <= (x < width - 1 ? x + 1 : x); xx++) any |= unconv[(size_t)yy * width + xx];
                if (!any) {
                    active[i] = 0;
                    count[i] = s.passes;
                    s.active -= 1;
                }
            }
        s.last_check = s.passes;
        if (s.summary.checks < CHUNKY_ADAPTIVE_MAX_CHECKS) s.summary.active[s.summary.checks] = s.active;
        s.summary.checks += 1;
    }
    for (size_t i = 0; i < np; i++)
        if (active[i]) count[i] = s.passes;
    s.summary.passes = s.passes;
    give_versioned(s, st);
    return CHUNKY_OK;
}
