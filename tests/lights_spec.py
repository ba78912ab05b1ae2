"""The specification of chunky_render_light_passes (include/chunky_hip.h) on the oracle: a group image IS the
oracle's own image of the scene with the other two scalars set to zero — sky_intensity, the sun's intensity (PackedSun word 3) and the
emitter scale.  Four port.render_passes calls and nothing else: the oracle is the specification.  A plain helper module for the tests
(not a conftest)."""
import dataclasses

import numpy as np

from oracle import binding

from chunkyclplugin_amd import native

IMAGES = ("sky", "sun", "emitters", "all")
WHICH = {"sky": native.LIGHT_SKY, "sun": native.LIGHT_SUN, "emitters": native.LIGHT_EMITTERS, "all": native.LIGHT_ALL}
ZERO_BITS = 0   # the bits of 0.0f


def group_scene(sc, group, emitter_scale):
    """(scene, emitter scale) of `group`: the triple of the table in section 17"""
    sun = np.array(sc.sun, np.int32)
    if group not in ("sun", "all"):
        sun[3] = ZERO_BITS
    sky = sc.sky_intensity if group in ("sky", "all") else 0.0
    return dataclasses.replace(sc, sky_intensity=sky, sun=sun), (emitter_scale if group in ("emitters", "all") else 0.0)


def expected_lights(port, sc, seeds, first_spp=0, emitter_scale=13.0, max_depth=5, draw_depth=256, cull=False, init=None, groups=IMAGES):
    """{"sky", "sun", "emitters", "all"}: (3 * W * H,) float32 each after the passes `seeds`; `init` such a dict to continue from."""
    out = {}
    for g in groups:
        scene, scale = group_scene(sc, g, emitter_scale)
        res = None if init is None else np.array(init[g], np.float32).reshape(-1)
        with binding.PortOptions(port, draw_depth, max_depth, scale), binding.PortCull(port, cull):
            out[g] = port.render_passes(scene, seeds, first_spp=first_spp, res=res)
    return out
