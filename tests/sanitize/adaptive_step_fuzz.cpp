// adaptive_step_fuzz — the step function of adaptive continuation (csrc/adaptive_spec.h ad_step, ad_grid_floor, ad_grid_before,
// ad_on_grid) on its own, under AddressSanitizer + UBSan: hand-written cases, every (passes, last_check) a run can leave for a grid of
// small parameters against the loop of a single run written out here, and the extremes of what an int holds.
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../chunkyclplugin_amd/csrc/adaptive_spec.h"

static long long failures = 0;
#define EXPECT(cond)                                                       \
    do {                                                                   \
        if (!(cond)) {                                                     \
            if (failures++ < 20) fprintf(stderr, "line %d: %s\n", __LINE__, #cond); \
        }                                                                  \
    } while (0)

struct Trace {
    std::vector<int> round_ends, checks;  // pass counts at which rounds ended and checks ran
    int passes, last_check;
};

// continues (passes, last_check) to max_spp with ad_step, as the host and the device loops do (no pixel ever leaves here)
static void walk(Trace* t, int mn, int ci, int max_spp) {
    for (int guard = 0; t->passes < max_spp; guard++) {
        if (guard > 1000000) { EXPECT(!"the loop ends"); return; }
        const ad_step_t s = ad_step(t->passes, t->last_check, mn, ci, max_spp);
        if (s.check_first) {
            EXPECT(s.round == 0);
            t->checks.push_back(t->passes);
            t->last_check = t->passes;
            continue;
        }
        EXPECT(s.round > 0 && s.round <= max_spp - t->passes);
        t->passes += s.round;
        t->round_ends.push_back(t->passes);
        if (ad_check_due(t->passes, mn, ci, max_spp)) {
            t->checks.push_back(t->passes);
            t->last_check = t->passes;
        }
    }
}

// the loop of a single run as chunky_render_adaptive had it before it could continue: min_spp passes, then check_interval or what is left
static void single(Trace* t, int mn, int ci, int max_spp) {
    int done = 0;
    while (done < max_spp) {
        const int left = max_spp - done;
        const int n = done == 0 ? (mn < left ? mn : left) : (ci < left ? ci : left);
        done += n;
        t->round_ends.push_back(done);
        if (done >= mn && done < max_spp && (done - mn) % ci == 0) {
            t->checks.push_back(done);
            t->last_check = done;
        }
    }
    t->passes = done;
}

static void step_is(int passes, int last_check, int mn, int ci, int max_spp, int check_first, int round) {
    const ad_step_t s = ad_step(passes, last_check, mn, ci, max_spp);
    if (s.check_first != check_first || s.round != round) {
        if (failures++ < 20)
            fprintf(stderr, "ad_step(%d, %d, %d, %d, %d) = (%d, %d), expected (%d, %d)\n", passes, last_check, mn, ci, max_spp, s.check_first, s.round,
                    check_first, round);
    }
}

int main() {
    // hand-written: min_spp 8, check_interval 4 (grid 8, 12, 16, ...)
    step_is(12, 8, 8, 4, 20, 1, 0);   // on the grid, its check not run: the check first
    step_is(12, 8, 8, 4, 12, 0, 0);   // ... but not when max_spp is reached there (no check at max_spp, nothing to render)
    step_is(12, 12, 8, 4, 20, 0, 4);  // on the grid, checked: a whole round
    step_is(12, 12, 8, 4, 14, 0, 2);  // ... cut by max_spp
    step_is(13, 12, 8, 4, 40, 0, 3);  // off the grid: a short round to the next grid point
    step_is(15, 12, 8, 4, 40, 0, 1);
    step_is(13, 12, 8, 4, 14, 0, 1);  // ... or to max_spp when that comes first
    step_is(3, 0, 8, 4, 40, 0, 5);    // below min_spp: to min_spp
    step_is(3, 0, 8, 4, 5, 0, 2);     // ... or to max_spp
    step_is(0, 0, 8, 4, 40, 0, 8);    // the empty state: min_spp passes
    step_is(8, 0, 8, 4, 40, 1, 0);    // the first grid point, unchecked
    step_is(8, 8, 8, 4, 40, 0, 4);
    step_is(39, 36, 8, 4, 40, 0, 1);  // one pass left
    step_is(36, 32, 8, 4, 37, 1, 0);  // one pass left after the check that is now due
    step_is(36, 36, 8, 4, 37, 0, 1);
    step_is(40, 36, 8, 4, 40, 0, 0);  // nothing left
    step_is(41, 40, 8, 4, 40, 0, 0);  // (max_spp below passes: the callers refuse it; the step is empty)
    // extremes: no sum may pass INT_MAX
    step_is(5, 4, 4, INT_MAX, 9, 0, 4);
    step_is(4, 0, 4, INT_MAX, INT_MAX, 1, 0);
    step_is(4, 4, 4, INT_MAX, INT_MAX, 0, INT_MAX - 4);
    step_is(0, 0, INT_MAX, 1, INT_MAX, 0, INT_MAX);
    step_is(INT_MAX - 1, INT_MAX - 2, 2, 1, INT_MAX, 1, 0);
    step_is(INT_MAX - 1, INT_MAX - 1, 2, 1, INT_MAX, 0, 1);
    step_is(7, 5, 2, 3, INT_MAX, 0, 1);
    EXPECT(ad_grid_floor(INT_MAX, 2, INT_MAX) == 2 && ad_grid_floor(1, 2, 1) == 0 && ad_grid_floor(13, 8, 4) == 12 && ad_grid_floor(12, 8, 4) == 12);
    EXPECT(ad_grid_before(8, 8, 4) == 0 && ad_grid_before(12, 8, 4) == 8 && ad_grid_before(2, 2, INT_MAX) == 0);
    EXPECT(ad_on_grid(8, 8, 4) && ad_on_grid(16, 8, 4) && !ad_on_grid(0, 8, 4) && !ad_on_grid(4, 8, 4) && !ad_on_grid(13, 8, 4) && ad_on_grid(INT_MAX, INT_MAX, 7));

    long long walks = 0, splits = 0;
    for (int mn = 2; mn <= 9; mn++)
        for (int ci = 1; ci <= 7; ci++)
            for (int B = 1; B <= 40; B++) {
                Trace one{{}, {}, 0, 0}, ref{{}, {}, 0, 0};
                walk(&one, mn, ci, B);
                single(&ref, mn, ci, B);
                walks++;
                // from the empty state ad_step is the single run's loop, round for round
                EXPECT(one.round_ends == ref.round_ends && one.checks == ref.checks && one.passes == B && one.last_check == ref.last_check);
                // and a run cut at any d, continued to B, makes the single run's checks, each once and in order; every round ends on a
                // grid point, on d or on B, and none is longer than the single run's
                for (int d = 1; d < B; d++) {
                    Trace t{{}, {}, 0, 0};
                    walk(&t, mn, ci, d);
                    // what chunky_adaptive_state_check allows after d passes
                    const int g = ad_grid_floor(d, mn, ci);
                    EXPECT(t.last_check == g || (g == d && t.last_check == ad_grid_before(g, mn, ci)));
                    walk(&t, mn, ci, B);
                    splits++;
                    EXPECT(t.checks == ref.checks && t.passes == B && t.last_check == ref.last_check);
                    int prev = 0;
                    for (int e : t.round_ends) {
                        EXPECT(e > prev && (e == d || e == B || ad_on_grid(e, mn, ci)));
                        EXPECT(prev == 0 || prev == d || e - prev <= ci);
                        EXPECT(prev != 0 || e == (mn < d ? mn : d));  // the first round
                        prev = e;
                    }
                    // no round is split needlessly: the run cut at d has the single run's rounds plus at most one (the one d cut)
                    EXPECT(t.round_ends.size() <= ref.round_ends.size() + 1);
                }
            }
    printf("{\"walks\": %lld, \"splits\": %lld, \"failures\": %lld}\n", walks, splits, failures);
    return failures != 0;
}
