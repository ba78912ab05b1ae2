// matte_host.cpp — the ID mattes on the host: the fold, the ranks and the extract of the specification (matte_spec.h) over the
// plane-major state, and the check of a caller's state.  Plain C++: no device code, no HIP type.
#include "matte_host.hpp"

#include <algorithm>

#include "capi_error.hpp"
#include "matte_spec.h"

static_assert(MATTE_SLOTS == CHUNKY_MATTE_SLOTS && MATTE_SKY == CHUNKY_MATTE_SKY && MATTE_WORLD_ENTITY == CHUNKY_MATTE_WORLD_ENTITY &&
                  MATTE_ACTOR_ENTITY == CHUNKY_MATTE_ACTOR_ENTITY && MATTE_EMPTY == CHUNKY_MATTE_EMPTY,
              "matte_spec.h and include/chunky_hip.h name the same values");

// slot s of pixel i is at [s * n + i]
static matte_px_t load_px(const int32_t* ids, const int32_t* counts, int32_t other, size_t n, size_t i) {
    matte_px_t p;
    p.id0 = ids[i], p.id1 = ids[n + i], p.id2 = ids[2 * n + i], p.id3 = ids[3 * n + i], p.id4 = ids[4 * n + i], p.id5 = ids[5 * n + i];
    p.c0 = counts[i], p.c1 = counts[n + i], p.c2 = counts[2 * n + i], p.c3 = counts[3 * n + i], p.c4 = counts[4 * n + i], p.c5 = counts[5 * n + i];
    p.other = other;
    return p;
}

// counts >= 0 and no more than `most` samples in the slots of any pixel: what the twins below need to stay inside int32
static int counts_within(const char* who, const int32_t* counts, size_t n, int64_t most) {
    for (size_t i = 0; i < n; i++) {
        int64_t sum = 0;
        for (int s = 0; s < MATTE_SLOTS; s++) {
            const int32_t c = counts[(size_t)s * n + i];
            if (c < 0) return fail(CHUNKY_E_INVALID, "%s: pixel %zu slot %d has count %d", who, i, s, c);
            sum += c;
        }
        if (sum > most) return fail(CHUNKY_E_INVALID, "%s: pixel %zu holds %lld samples, more than %lld", who, i, (long long)sum, (long long)most);
    }
    return CHUNKY_OK;
}

extern "C" int chunky_matte_host_fold(const int32_t* sample_ids, int n_passes, int64_t n_pixels, int32_t* ids, int32_t* counts, int32_t* other) {
    if (n_passes < 0 || n_pixels <= 0 || !ids || !counts || !other || (n_passes > 0 && !sample_ids)) return fail(CHUNKY_E_INVALID, "matte_host_fold: bad arguments");
    const size_t n = (size_t)n_pixels;
    for (size_t i = 0; i < n; i++)
        if (other[i] < 0 || other[i] > INT32_MAX - n_passes) return fail(CHUNKY_E_INVALID, "matte_host_fold: pixel %zu has other = %d before %d passes", i, other[i], n_passes);
    if (int rc = counts_within("matte_host_fold", counts, n, (int64_t)INT32_MAX - n_passes)) return rc;
    for (size_t i = 0; i < n * (size_t)n_passes; i++)
        if (sample_ids[i] == MATTE_EMPTY) return fail(CHUNKY_E_INVALID, "matte_host_fold: sample %zu is CHUNKY_MATTE_EMPTY, which is no id", i);
    for (size_t i = 0; i < n; i++) {
        matte_px_t p = load_px(ids, counts, other[i], n, i);
        for (int k = 0; k < n_passes; k++) matte_update(&p, sample_ids[(size_t)k * n + i]);
        ids[i] = p.id0, ids[n + i] = p.id1, ids[2 * n + i] = p.id2, ids[3 * n + i] = p.id3, ids[4 * n + i] = p.id4, ids[5 * n + i] = p.id5;
        counts[i] = p.c0, counts[n + i] = p.c1, counts[2 * n + i] = p.c2, counts[3 * n + i] = p.c3, counts[4 * n + i] = p.c4, counts[5 * n + i] = p.c5;
        other[i] = p.other;
    }
    return CHUNKY_OK;
}

extern "C" int chunky_matte_host_ranks(const int32_t* ids, const int32_t* counts, int64_t n_pixels, int32_t passes, int32_t* out_ids, float* out_coverage) {
    if (n_pixels <= 0 || !ids || !counts || !out_ids || !out_coverage) return fail(CHUNKY_E_INVALID, "matte_host_ranks: bad arguments");
    if (passes <= 0) return fail(CHUNKY_E_INVALID, "matte_host_ranks: %d passes", passes);
    const size_t n = (size_t)n_pixels;
    if (int rc = counts_within("matte_host_ranks", counts, n, passes)) return rc;
    for (size_t i = 0; i < n; i++) {
        const matte_px_t p = load_px(ids, counts, 0, n, i);
        const matte_rank_t r = matte_ranks(&p);
        const int rank[MATTE_SLOTS] = {r.r0, r.r1, r.r2, r.r3, r.r4, r.r5};
        const int32_t id[MATTE_SLOTS] = {p.id0, p.id1, p.id2, p.id3, p.id4, p.id5}, c[MATTE_SLOTS] = {p.c0, p.c1, p.c2, p.c3, p.c4, p.c5};
        for (int s = 0; s < MATTE_SLOTS; s++) {
            out_ids[(size_t)rank[s] * n + i] = matte_rank_id(id[s], c[s]);
            out_coverage[(size_t)rank[s] * n + i] = matte_coverage(c[s], passes);
        }
    }
    return CHUNKY_OK;
}

int matte_sorted_set(const char* who, const int32_t* set, int n_set, std::vector<int32_t>* sorted) {
    if (n_set < 0 || (n_set > 0 && !set)) return fail(CHUNKY_E_INVALID, "%s: a set of %d ids%s", who, n_set, n_set > 0 ? " at NULL" : "");
    sorted->assign(set, set + n_set);
    std::sort(sorted->begin(), sorted->end());
    sorted->erase(std::unique(sorted->begin(), sorted->end()), sorted->end());
    if (!sorted->empty() && sorted->front() == MATTE_EMPTY) return fail(CHUNKY_E_INVALID, "%s: CHUNKY_MATTE_EMPTY in the set: it is no id", who);
    return CHUNKY_OK;
}

extern "C" int chunky_matte_host_extract(const int32_t* ids, const int32_t* counts, int64_t n_pixels, int32_t passes, const int32_t* set, int n_set, float* out) {
    if (n_pixels <= 0 || !ids || !counts || !out) return fail(CHUNKY_E_INVALID, "matte_host_extract: bad arguments");
    if (passes <= 0) return fail(CHUNKY_E_INVALID, "matte_host_extract: %d passes", passes);
    std::vector<int32_t> sorted;
    if (int rc = matte_sorted_set("matte_host_extract", set, n_set, &sorted)) return rc;
    const size_t n = (size_t)n_pixels;
    if (int rc = counts_within("matte_host_extract", counts, n, passes)) return rc;
    for (size_t i = 0; i < n; i++) {
        const matte_px_t p = load_px(ids, counts, 0, n, i);
        out[i] = matte_mask(matte_masked_sum(&p, sorted.data(), (int)sorted.size()), passes);
    }
    return CHUNKY_OK;
}

int matte_state_valid(const char* who, const int32_t* ids, const int32_t* counts, const int32_t* other, int64_t n_pixels, int32_t passes) {
    if (n_pixels <= 0 || !ids || !counts || !other) return fail(CHUNKY_E_INVALID, "%s: bad arguments", who);
    if (passes < 0) return fail(CHUNKY_E_INVALID, "%s: %d passes", who, passes);
    const size_t n = (size_t)n_pixels;
    for (size_t i = 0; i < n; i++) {
        if (other[i] < 0) return fail(CHUNKY_E_INVALID, "%s: pixel %zu has other = %d", who, i, other[i]);
        int64_t sum = other[i];
        bool empty_seen = false;
        for (int s = 0; s < MATTE_SLOTS; s++) {
            const int32_t c = counts[(size_t)s * n + i], id = ids[(size_t)s * n + i];
            if (c < 0) return fail(CHUNKY_E_INVALID, "%s: pixel %zu slot %d has count %d", who, i, s, c);
            if (c == 0) {
                empty_seen = true;
                continue;
            }
            if (empty_seen) return fail(CHUNKY_E_INVALID, "%s: pixel %zu slot %d is occupied behind an empty slot", who, i, s);
            if (id == MATTE_EMPTY) return fail(CHUNKY_E_INVALID, "%s: pixel %zu slot %d holds CHUNKY_MATTE_EMPTY, which is no id", who, i, s);
            for (int t = 0; t < s; t++)  // (the slots before s are all occupied)
                if (ids[(size_t)t * n + i] == id) return fail(CHUNKY_E_INVALID, "%s: pixel %zu holds id %d in slots %d and %d", who, i, id, t, s);
            sum += c;
        }
        if (sum != 0 && sum != passes) return fail(CHUNKY_E_INVALID, "%s: pixel %zu holds %lld samples after %d passes", who, i, (long long)sum, passes);
    }
    return CHUNKY_OK;
}

extern "C" int chunky_matte_state_check(const int32_t* ids, const int32_t* counts, const int32_t* other, int64_t n_pixels, int32_t passes) {
    return matte_state_valid("matte_state_check", ids, counts, other, n_pixels, passes);
}
