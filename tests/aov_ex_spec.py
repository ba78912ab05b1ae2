"""The specification of chunky_render_aov_passes_ex (include/chunky_hip.h) restated on the oracles, the way
aov_spec.py restates the AOV: the sample of a pass at a pixel is record 0 of the reference's sample — the first closestIntersect
of the camera ray — and seven images are folded from it.  Also the alpha byte of chunky_filter_frame_alpha as a numpy formula.
A plain helper module for the tests (not a conftest)."""
import numpy as np

from oracle import binding

from chunkyclplugin_amd import native

FLOAT_IMAGES = ("albedo", "normal", "alpha", "depth", "position", "emittance")
IMAGES = FLOAT_IMAGES + ("block",)
WHICH = {"albedo": native.AOV_ALBEDO, "normal": native.AOV_NORMAL, "alpha": native.AOV_ALPHA, "depth": native.AOV_DEPTH,
         "position": native.AOV_POSITION, "emittance": native.AOV_EMITTANCE, "block": native.AOV_BLOCK}
WORDS = {"albedo": 3, "normal": 3, "alpha": 1, "depth": 1, "position": 3, "emittance": 1, "block": 1}


def zero_images(n):
    out = {k: np.zeros((n, WORDS[k]), np.float32) for k in FLOAT_IMAGES}
    out["block"] = np.zeros((n, 1), np.int32)
    return out


def expected_aov_ex(tracer, sc, seeds, gids, first_spp=0, init=None):
    """{image name: (len(gids), words per pixel)} after the passes `seeds` with bufferSpp first_spp, first_spp + 1, ...; float32, the
    block id int32.  `tracer` is binding.ref() or binding.port(); `sc` a scene or a binding.SceneHandle; `init` such a dict to
    continue from.  Hit: albedo = color.xyz, normal, alpha 1, depth = distance, position = point, emittance, block = material.  Miss:
    albedo = the sample's radiance (the sky), block -1, everything else 0.  The float images are folded in float32 with one rounding
    per operation, (img * spp + v) / (spp + 1) (K/rayTracer.cl:109-112); the block id is overwritten by every pass."""
    h = sc if isinstance(sc, binding.SceneHandle) else binding.SceneHandle(sc)
    gids = np.asarray(gids, np.int64).reshape(-1)
    n = len(gids)
    if init is None:
        img = zero_images(n)
    else:
        img = {k: np.array(init[k], np.int32 if k == "block" else np.float32).reshape(n, WORDS[k]) for k in IMAGES}
    for k, seed in enumerate(np.asarray(seeds, np.int32).reshape(-1)):
        v = zero_images(n)
        for i, gid in enumerate(gids):
            recs, rad = tracer.trace_records(h, int(seed), int(gid))
            rec = recs[0]
            if rec["hit"]:
                v["albedo"][i] = rec["color"][:3]
                v["normal"][i] = rec["normal"]
                v["alpha"][i] = 1.0
                v["depth"][i] = rec["distance"]
                v["position"][i] = rec["point"]
                v["emittance"][i] = rec["emittance"]
                v["block"][i] = rec["material"]
            else:
                v["albedo"][i] = rad
                v["block"][i] = -1
        spp = np.float32(first_spp + k)
        spp1 = np.float32(first_spp + k + 1)
        for name in FLOAT_IMAGES:
            img[name] = (img[name] * spp + v[name]) / spp1
        img["block"] = v["block"]
    return img


def alpha_byte(alpha):
    """min(255, (uint)(clamp(alpha, 0, 1) * 255.0f + 0.5f)) in float32, one rounding per operation; a NaN gives 0."""
    a = np.asarray(alpha, np.float32)
    c = np.where(np.isnan(a), np.float32(0), np.clip(a, np.float32(0), np.float32(1))).astype(np.float32)
    v = c * np.float32(255.0) + np.float32(0.5)
    return np.minimum(255, v.astype(np.uint32)).astype(np.uint32)   # truncation, as the C cast
