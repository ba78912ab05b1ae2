"""The AOV specification (include/chunky_hip.h chunky_render_aov_passes) restated on the oracles: for each pass the sample of a
pixel is record 0 of the reference's sample — the first closestIntersect of the camera ray — folded with the reference's running
mean.  A plain helper module for the AOV tests (not a conftest)."""
import numpy as np

from oracle import binding


def expected_aov(tracer, sc, seeds, gids, first_spp=0, init=None):
    """(albedo, normal), each (len(gids), 3) float32, after the passes `seeds` with bufferSpp first_spp, first_spp + 1, ...

    `tracer` is binding.ref() or binding.port(); `sc` a scene or a binding.SceneHandle (made once here otherwise: converting a
    1080p scene per call is slow).  A hit contributes record.color.xyz and record.normal; a miss the sample's radiance (the sky
    of intersectSky with record.emittance = 1) and (0, 0, 0).  `init` = (albedo, normal) to continue from."""
    h = sc if isinstance(sc, binding.SceneHandle) else binding.SceneHandle(sc)
    gids = np.asarray(gids, np.int64).reshape(-1)
    if init is None:
        albedo = np.zeros((len(gids), 3), np.float32)
        normal = np.zeros((len(gids), 3), np.float32)
    else:
        albedo = np.array(init[0], np.float32).reshape(len(gids), 3)
        normal = np.array(init[1], np.float32).reshape(len(gids), 3)
    for k, seed in enumerate(np.asarray(seeds, np.int32).reshape(-1)):
        a = np.zeros((len(gids), 3), np.float32)
        n = np.zeros((len(gids), 3), np.float32)
        for i, gid in enumerate(gids):
            recs, rad = tracer.trace_records(h, int(seed), int(gid))
            if recs[0]["hit"]:
                a[i] = recs[0]["color"][:3]
                n[i] = recs[0]["normal"]
            else:
                a[i] = rad
        spp = np.float32(first_spp + k)
        spp1 = np.float32(first_spp + k + 1)
        # float32 throughout, one rounding per operation (no fused multiply-add): K/rayTracer.cl:109-112
        albedo = (albedo * spp + a) / spp1
        normal = (normal * spp + n) / spp1
    return albedo, normal
