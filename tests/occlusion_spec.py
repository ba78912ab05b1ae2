"""The specification of chunky_render_occlusion_passes (include/chunky_hip.h) restated on the oracles, the way
aov_ex_spec.py restates the first-hit images: the sample of a pass at a pixel is the reference's sample cut off after its first bounce
trace — records 0 to 2 of trace_records — and two images are folded from it.  The records are gathered once (occlusion_records) and
folded for any radius (fold_occlusion); expected_occlusion is the two in a row.  A plain helper module for the tests (not a conftest)."""
import numpy as np

from oracle import binding

from chunkyclplugin_amd import native

IMAGES = ("ao", "sun")
WHICH = {"ao": native.AOV_AO, "sun": native.AOV_SUN}


def handle_and_sun(sc):
    """(binding.SceneHandle, bit 0 of the PackedSun flags — word 0) of a scene or a SceneHandle"""
    h = sc if isinstance(sc, binding.SceneHandle) else binding.SceneHandle(sc)
    return h, bool(int(h.keep["sun"].reshape(-1)[0]) & 1)


def occlusion_records(tracer, sc, seeds, gids):
    """What the two images are made of, per (pass, pixel): "hit" rec[0].hit; "sun_hit" rec[1].hit where the scene's sun flag is set
    (else False); "b_hit", "b_distance", "b_normal" of the bounce record rec[sun ? 2 : 1] (False, 0, 0 where the first trace misses);
    and "sun", the flag.  `tracer` is binding.ref() or binding.port() with its default options: records 0 to 2 always exist within
    CHUNKY_MAX_TRACES at the default max depth 5."""
    h, sun = handle_and_sun(sc)
    gids = np.asarray(gids, np.int64).reshape(-1)
    seeds = np.asarray(seeds, np.int32).reshape(-1)
    shape = (len(seeds), len(gids))
    out = {"sun": sun, "hit": np.zeros(shape, bool), "sun_hit": np.zeros(shape, bool), "b_hit": np.zeros(shape, bool),
           "b_distance": np.zeros(shape, np.float32), "b_normal": np.zeros(shape + (3,), np.float32)}
    for k, seed in enumerate(seeds):
        for i, gid in enumerate(gids):
            recs, _ = tracer.trace_records(h, int(seed), int(gid))
            if not recs[0]["hit"]:
                continue
            out["hit"][k, i] = True
            if sun:
                out["sun_hit"][k, i] = bool(recs[1]["hit"])
            b = recs[2 if sun else 1]
            out["b_hit"][k, i] = bool(b["hit"])
            out["b_distance"][k, i] = b["distance"]
            out["b_normal"][k, i] = b["normal"]
    return out


def sample_values(rec, ao_distance):
    """(ao, sun) samples, (passes, pixels) float32 each, exactly as the table of section 16 says."""
    with np.errstate(invalid="ignore"):
        near = rec["b_distance"] < np.float32(ao_distance)   # one strict float compare: a NaN distance is not near, a negative one is
    v_ao = np.where(rec["hit"] & rec["b_hit"] & near, np.float32(0), np.float32(1)).astype(np.float32)
    if rec["sun"]:
        v_sun = np.where(rec["hit"] & rec["sun_hit"], np.float32(0), np.float32(1)).astype(np.float32)
    else:
        v_sun = np.where(rec["hit"], np.float32(0), np.float32(1)).astype(np.float32)
    return v_ao, v_sun


def fold_occlusion(rec, ao_distance, first_spp=0, init=None):
    """{"ao", "sun"}: (pixels,) float32 each after the passes of `rec` with bufferSpp first_spp, first_spp + 1, ...; `init` such a dict
    to continue from.  Folded in float32 with one rounding per operation, (img * spp + v) / (spp + 1) (K/rayTracer.cl:109-112)."""
    n = rec["hit"].shape[1]
    img = {k: np.zeros(n, np.float32) if init is None else np.array(init[k], np.float32).reshape(n) for k in IMAGES}
    v_ao, v_sun = sample_values(rec, ao_distance)
    for k in range(rec["hit"].shape[0]):
        spp, spp1 = np.float32(first_spp + k), np.float32(first_spp + k + 1)
        img["ao"] = (img["ao"] * spp + v_ao[k]) / spp1
        img["sun"] = (img["sun"] * spp + v_sun[k]) / spp1
    return img


def expected_occlusion(tracer, sc, seeds, gids, ao_distance, first_spp=0, init=None):
    """The two images of `gids` after the passes `seeds`; `sc` a scene or a binding.SceneHandle.  A first trace that misses folds 1
    into both."""
    return fold_occlusion(occlusion_records(tracer, sc, seeds, gids), ao_distance, first_spp, init)
