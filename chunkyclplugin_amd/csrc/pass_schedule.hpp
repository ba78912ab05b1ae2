// pass_schedule.hpp — how the n passes of a call become launches, decided in one place: how many passes one launch may carry
// (launch_pass_cap), how large the staging array must be and what happens when the device cannot hold it (stage_passes), and how
// seeds[0 .. n) is cut into the PassSeeds of the launches (for_each_launch).  Every call of the C API that renders passes —
// chunky_render_passes, the adaptive rounds, the robust passes, the first-hit passes — goes through these.  Plain C++17 over ints, no
// HIP type and no device call: tests/sanitize/pass_schedule_fuzz.cpp runs them under AddressSanitizer + UBSan with an allocator that
// refuses above a limit (tests/test_pass_schedule_cpu.py).  DESIGN.md section 5, "how passes become launches".
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "launch_plan.hpp"  // kMaxPassesPerLaunch, kSampleTile, pool_tiles

namespace chunky {

// Seeds of the passes one launch runs, passed by value in the kernel-argument segment (wave-uniform
// scalar loads, no per-launch host->device copy): pass k uses seed[k] and bufferSpp first_spp + k
// (OpenClPathTracingRenderer.java:106-109).
// (kMaxPassesPerLaunch, and render_pool's kMaxPoolPasses: launch_plan.hpp)
struct PassSeeds {
    int n, first_spp;
    int seed[kMaxPassesPerLaunch];
};

// staging floats render_pool needs for a launch of n passes over this rank's tiles
inline size_t staging_floats(const ShardView& T, int width, int height, int n_passes) {
    return 3 * (size_t)pool_tiles(T, width, height) * kSampleTile * (size_t)n_passes;
}

// The most passes one launch over the pixel slots of T carries: render_pool stages every sample of a launch (12 bytes each) — at
// most `budget` bytes of it, fewer than 2^31 samples, at most `most` passes (kMaxPassesPerLaunch: the seeds fit the kernel-argument
// segment; kMaxPoolPasses for render_pool, which reads longer launches' seeds from device memory — a share of the image on several
// GPUs then pays the end-of-launch tail once per 1024 passes instead of four times).  Below 1 when not even one pass fits.
inline int launch_pass_cap(const ShardView& T, int width, int height, size_t budget, int most) {
    const int64_t n_slots = (int64_t)(staging_floats(T, width, height, 1) / 3);  // padded tiles
    if (n_slots <= 0) return most;
    int64_t cap = (int64_t)(budget / 12) / n_slots;
    const int64_t cap31 = ((int64_t)1 << 31) / n_slots - 1;
    if (cap > cap31) cap = cap31;
    return (int)(cap > most ? most : cap);
}

// The cut: seeds[0 .. n) in launches of at most `cap` (>= 1) passes, in order.  fn(P, launch_seeds) is called once per launch with
// P.n and P.first_spp = first_spp + the launch's offset, and launch_seeds = seeds + that offset; P.seed holds the launch's seeds
// when they fit the kernel-argument segment (P.n <= kMaxPassesPerLaunch) — a longer launch's travel by device memory, from
// launch_seeds.  The first code fn returns that is not 0 ends the cut and is returned.
template <class Fn>
int for_each_launch(const int32_t* seeds, int n, int first_spp, int cap, Fn fn) {
    for (int done = 0; done < n;) {
        PassSeeds P;
        P.n = n - done < cap ? n - done : cap;
        P.first_spp = first_spp + done;
        if (P.n <= kMaxPassesPerLaunch) memcpy(P.seed, seeds + done, (size_t)P.n * 4);
        if (int rc = fn(P, seeds + done)) return rc;
        done += P.n;
    }
    return 0;
}

// The staging rule.  `held` bytes are allocated now; the call's first launch — its longest: every later one is at most as long, so
// sizing once here equals sizing before each launch — carries `launch` passes of at most `cap` per launch over shard T.
//   * It grows only: an array that holds the launch stays as it is, and try_alloc is not called.
//   * Otherwise try_alloc(bytes) -> bool allocates a new array (the caller has released the old one).  A reserve hint (`reserve`
//     passes, 0: none; chunky_render_run_ex climbs 1, 8, 64 ... passes per launch: one allocation for where it is going, not four)
//     is tried first — ahead = min(reserve, cap, kMaxPassesPerLaunch) passes, when that exceeds the launch and is at most half of
//     `free_bytes` (other targets and members live on the device too); if it is not taken, the launch's own bytes are asked for.
//   * When that fails memory is short: shorter launches instead of a failed render.  The launch is halved, (n + 1) / 2, until
//     try_alloc succeeds — the cap of every later launch is then the launch that fitted — or one pass does not fit.
// Returns the bytes held afterwards and the passes per launch (0: not even one pass could be allocated, nothing is held).
struct StagedLaunch {
    size_t bytes;
    int passes;
};
template <class TryAlloc>
StagedLaunch stage_passes(size_t held, const ShardView& T, int width, int height, int launch, int cap, int reserve, size_t free_bytes,
                          TryAlloc try_alloc) {
    size_t need = staging_floats(T, width, height, launch) * sizeof(float);
    if (held >= need) return StagedLaunch{held, launch};
    int ahead = reserve < cap ? reserve : cap;
    if (ahead > kMaxPassesPerLaunch) ahead = kMaxPassesPerLaunch;  // (the pass loop's own launches stop there)
    if (ahead > launch) {
        const size_t want = staging_floats(T, width, height, ahead) * sizeof(float);
        if (want <= free_bytes / 2 && try_alloc(want)) return StagedLaunch{want, launch};
    }
    while (!try_alloc(need)) {
        if (launch <= 1) return StagedLaunch{0, 0};
        launch = (launch + 1) / 2;
        need = staging_floats(T, width, height, launch) * sizeof(float);
    }
    return StagedLaunch{need, launch};
}

}  // namespace chunky
