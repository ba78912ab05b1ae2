"""Worlds for the tests of render_pool's march cap (tests/test_march_cap_cpu.py, tests/test_gpu_march_cap.py): a small outdoor scene's
palettes, atlas, sky and sun round an octree built here, whose highest leaf that can be hit sits where the case says.

Every world (edge S = 2^depth) has a floor of full cubes at y = 0 (except "air" and "floor", which is the floor alone) and, above
whatever tops it, things that cannot be hit: an invisible block (palette type 0) and an ANY_TYPE cell.  `expected` is 1 + the highest
y of a cell that can be hit — what the library's hit_top must be."""
import dataclasses
import functools

import numpy as np

from chunkyclplugin_amd import scenes

KINDS = ("floor", "middle", "last_row", "big_leaf", "column", "air")


@functools.lru_cache(maxsize=None)
def base():
    """palettes, atlas, sky, sun: the small outdoor world's (one chunk), with one invisible block appended to the block palette"""
    sc = scenes.outdoor_world(chunks=1, height=32, width=64, img_height=48, sun_flag=True, aabb_frac=0.10, quad_frac=0.06)
    bp = np.asarray(sc.block_palette, np.int32)
    types = bp[0::2]
    cube = int(np.flatnonzero(types == 1)[0])
    model = int(np.flatnonzero((types == 2) | (types == 3))[0])
    ghost = len(types)
    return dataclasses.replace(sc, block_palette=np.concatenate([bp, np.array([0, 0], np.int32)])), cube, model, ghost


def cells(kind, depth):
    """the dense [x, y, z] array of block-palette indices, and the expected hit_top"""
    _sc, cube, model, ghost = base()
    S = 1 << depth
    t = np.zeros((S, S, S), np.int32)
    if kind == "air":
        t[1, S - 2, 1] = ghost
        t[2, S - 1, 2] = scenes.ANY_TYPE
        return t, 0
    t[:, 0, :] = cube
    top = 1
    if kind == "middle":  # a pillar with a model block on top, below the middle
        h = S // 2 - 3
        t[S // 2, 1:h - 1, S // 2] = cube
        t[S // 2, h - 1, S // 2] = model
        top = h
    elif kind == "last_row":  # one cube in the world's last row: nothing is capped
        t[3, S - 1, S - 3] = cube
        top = S
    elif kind == "big_leaf":  # an aligned 4^3 block of one cube type: a leaf of level 2
        t[4:8, S // 2:S // 2 + 4, 8:12] = cube
        top = S // 2 + 4
    elif kind == "column":  # a full column: hit_top is the world's edge
        t[5, :, 6] = cube
        top = S
    else:
        assert kind == "floor", kind
    if top < S:  # what cannot be hit, above everything that can
        t[1, min(top + 2, S - 1), 1] = ghost
        t[S - 2, S - 1, S - 2] = scenes.ANY_TYPE
        t[2:4, S - 2:S, 2:4] = ghost  # (a leaf of level 1)
    return t, top


@functools.lru_cache(maxsize=None)
def world(kind, depth, sun="on"):
    """-> (scene, expected hit_top); sun: "on" (the base's), "horizon" (altitude 0: shadow rays with d.y about 0), "below", "off" """
    sc, _cube, _model, _ghost = base()
    t, top = cells(kind, depth)
    s = np.asarray(sc.sun, np.int32).copy()
    if sun == "horizon":
        s[4] = scenes.f2i(0.0)
    elif sun == "below":
        s[4] = scenes.f2i(-0.4)
    elif sun == "off":
        s[0] = 0
    else:
        assert sun == "on", sun
    return dataclasses.replace(sc, octree=scenes.build_octree(t, depth), octree_depth=depth, sun=s, name=f"cap_{kind}_{depth}_{sun}"), top


def view(sc, where, top, width, height):
    """the pinhole camera: "below" the cap looking across, "inside" the capped region looking across, "down" from above the world,
    "up" from above the floor into the sky"""
    S = float(1 << sc.octree_depth)
    mid = S / 2
    y_in = min(max(top, 1) + 2.5, S - 0.5)
    cam = {"below": scenes.look_at_camera((2.5, min(max(top, 1) - 0.5, 2.5) if top <= 3 else top - 1.5, 3.5), (mid, max(top, 1) * 0.6, mid)),
           "inside": scenes.look_at_camera((2.5, y_in, 3.5), (mid + 3, y_in - 1.0, mid)),
           "down": scenes.look_at_camera((mid * 0.3, S + 9.0, mid * 0.4), (mid, 0.0, mid)),
           "up": scenes.look_at_camera((mid, 1.5, mid), (mid + 4, S, mid + 3))}[where]
    return sc.with_view(width, height, camera=cam, projector_type=0)
