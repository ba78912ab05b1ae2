/* matte_spec.h — the arithmetic of the antialiased ID mattes (include/chunky_hip.h, "ID mattes"), compiled by
 * the kernels (matte.hip) and by the host (matte_host.cpp) from this one text: the id of a sample given which part of
 * closestIntersect won, the update of a pixel's slots, the rank order and the masked sum.
 *
 * Counts are integers; the only float operations are the two int -> float conversions (round to nearest) and the one division of a
 * coverage, each exactly rounded on both sides.  A pixel's state is six named (id, count) pairs and a word, never an array: device
 * code keeps it in registers, and an array indexed at run time would go to scratch memory. */
#pragma once
#include <stdint.h>

#include "rt_math.h"

#define MATTE_SLOTS 6
#define MATTE_SKY (-1)
#define MATTE_WORLD_ENTITY (-2)
#define MATTE_ACTOR_ENTITY (-3)
#define MATTE_EMPTY INT32_MIN

/* The id of a sample.  closestIntersect runs the octree, then the world BVH, then the actor BVH, and each later part wins only with
 * a strictly smaller distance: the id names the last part that won.  octree_hit: the octree part hit a block, whose leaf value is
 * `material`; world_won / actor_won: that BVH's walk accepted a triangle. */
RT_FN int32_t matte_id(int octree_hit, int32_t material, int world_won, int actor_won) {
    if (actor_won) return MATTE_ACTOR_ENTITY;
    if (world_won) return MATTE_WORLD_ENTITY;
    return octree_hit ? material : MATTE_SKY;
}

typedef struct matte_px_t {
    int32_t id0, id1, id2, id3, id4, id5;
    int32_t c0, c1, c2, c3, c4, c5;
    int32_t other;
} matte_px_t;

/* One sample with id v: the first occupied slot that holds v counts it, else the first empty slot takes it, else `other` does.
 * (The slot found gets id = v and count + 1 either way: a match already holds v, an empty slot goes from 0 to 1.) */
RT_FN void matte_update(matte_px_t* p, int32_t v) {
    int s = -1;
    /* the first empty slot ... */
    s = p->c5 == 0 ? 5 : s;
    s = p->c4 == 0 ? 4 : s;
    s = p->c3 == 0 ? 3 : s;
    s = p->c2 == 0 ? 2 : s;
    s = p->c1 == 0 ? 1 : s;
    s = p->c0 == 0 ? 0 : s;
    /* ... unless an occupied slot holds v: the first of those */
    int m = -1;
    m = (p->c5 > 0 && p->id5 == v) ? 5 : m;
    m = (p->c4 > 0 && p->id4 == v) ? 4 : m;
    m = (p->c3 > 0 && p->id3 == v) ? 3 : m;
    m = (p->c2 > 0 && p->id2 == v) ? 2 : m;
    m = (p->c1 > 0 && p->id1 == v) ? 1 : m;
    m = (p->c0 > 0 && p->id0 == v) ? 0 : m;
    s = m >= 0 ? m : s;
    p->id0 = s == 0 ? v : p->id0;
    p->id1 = s == 1 ? v : p->id1;
    p->id2 = s == 2 ? v : p->id2;
    p->id3 = s == 3 ? v : p->id3;
    p->id4 = s == 4 ? v : p->id4;
    p->id5 = s == 5 ? v : p->id5;
    p->c0 += s == 0;
    p->c1 += s == 1;
    p->c2 += s == 2;
    p->c3 += s == 3;
    p->c4 += s == 4;
    p->c5 += s == 5;
    p->other += s < 0;
}

/* The rank of every slot: slots by count descending, ties by the lower slot index (a stable order), so empty slots come last.  For
 * each pair i < j exactly one of the two moves down a rank: i when slot j's count is strictly greater, else j. */
typedef struct matte_rank_t {
    int r0, r1, r2, r3, r4, r5;
} matte_rank_t;

#define MATTE_PAIR(i, j)                 \
    {                                    \
        const int gt = p->c##j > p->c##i; \
        r.r##i += gt;                    \
        r.r##j += !gt;                   \
    }
RT_FN matte_rank_t matte_ranks(const matte_px_t* p) {
    matte_rank_t r;
    r.r0 = r.r1 = r.r2 = r.r3 = r.r4 = r.r5 = 0;
    MATTE_PAIR(0, 1) MATTE_PAIR(0, 2) MATTE_PAIR(0, 3) MATTE_PAIR(0, 4) MATTE_PAIR(0, 5)
    MATTE_PAIR(1, 2) MATTE_PAIR(1, 3) MATTE_PAIR(1, 4) MATTE_PAIR(1, 5)
    MATTE_PAIR(2, 3) MATTE_PAIR(2, 4) MATTE_PAIR(2, 5)
    MATTE_PAIR(3, 4) MATTE_PAIR(3, 5)
    MATTE_PAIR(4, 5)
    return r;
}
#undef MATTE_PAIR

/* what a rank reports for a slot: the id (MATTE_EMPTY for an empty slot) and the share of the passes that saw it */
RT_FN int32_t matte_rank_id(int32_t id, int32_t count) { return count > 0 ? id : MATTE_EMPTY; }
RT_FN float matte_coverage(int32_t count, int32_t passes) { return count > 0 ? (float)count / (float)passes : 0.0f; }

/* 1 when v is in sorted[0 .. n): ascending, no value twice */
RT_FN int matte_in_set(const int32_t* sorted, int n, int32_t v) {
    int lo = 0, hi = n; /* the first element >= v lies in [lo, hi] */
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (sorted[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo < n && sorted[lo] == v;
}

/* the samples of a pixel that the set names: the counts of its occupied slots whose id is in the set (`other` belongs to no id) */
RT_FN int32_t matte_masked_sum(const matte_px_t* p, const int32_t* sorted, int n) {
    int32_t sum = 0;
    sum += (p->c0 > 0 && matte_in_set(sorted, n, p->id0)) ? p->c0 : 0;
    sum += (p->c1 > 0 && matte_in_set(sorted, n, p->id1)) ? p->c1 : 0;
    sum += (p->c2 > 0 && matte_in_set(sorted, n, p->id2)) ? p->c2 : 0;
    sum += (p->c3 > 0 && matte_in_set(sorted, n, p->id3)) ? p->c3 : 0;
    sum += (p->c4 > 0 && matte_in_set(sorted, n, p->id4)) ? p->c4 : 0;
    sum += (p->c5 > 0 && matte_in_set(sorted, n, p->id5)) ? p->c5 : 0;
    return sum;
}
RT_FN float matte_mask(int32_t sum, int32_t passes) { return (float)sum / (float)passes; }
