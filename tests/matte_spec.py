"""The specification of the antialiased ID mattes (include/chunky_hip.h "ID mattes") restated in numpy on the
oracles: the id of a sample from record 0 of trace_records on three versions of the scene, the slot update, the ranks and the
extract.  A plain helper module for the tests (not a conftest)."""
import dataclasses

import numpy as np

from oracle import binding

from chunkyclplugin_amd import native, scenes

SLOTS = native.MATTE_SLOTS
SKY, WORLD, ACTOR, EMPTY = native.MATTE_SKY, native.MATTE_WORLD_ENTITY, native.MATTE_ACTOR_ENTITY, native.MATTE_EMPTY


def _has_bvh(a):
    return not np.array_equal(np.asarray(a, np.int32).reshape(-1), scenes.empty_bvh())


def expected_ids(tracer, sc, seeds, gids):
    """(len(seeds), len(gids)) int32: the id of the sample of every pass at every pixel.  `tracer` is binding.ref() or binding.port(),
    `sc` a scenes.PackedScene.  closestIntersect runs the octree, then the world BVH, then the actor BVH, and a later part wins only
    with a strictly smaller distance; so with d_octree, d_world, d_full the distances of record 0 on the scene without BVHs, without
    the actor BVH and whole (a miss: +inf), the sample is an actor hit iff d_full < d_world, else a world hit iff d_world < d_octree,
    else the octree's block (rec.material) or the sky."""
    seeds = np.asarray(seeds, np.int32).reshape(-1)
    gids = np.asarray(gids, np.int64).reshape(-1)
    no_actor = dataclasses.replace(sc, actor_bvh=scenes.empty_bvh())
    octree_only = dataclasses.replace(no_actor, world_bvh=scenes.empty_bvh())
    h_full, h_world, h_octree = binding.SceneHandle(sc), binding.SceneHandle(no_actor), binding.SceneHandle(octree_only)
    actor, world = _has_bvh(sc.actor_bvh), _has_bvh(sc.world_bvh)   # (a part that is not there never wins: its trace is the one before)

    def first(h, seed, gid):
        rec = tracer.trace_records(h, int(seed), int(gid))[0][0]
        return (np.float32(rec["distance"]) if rec["hit"] else np.float32(np.inf)), int(rec["material"]), bool(rec["hit"])

    out = np.zeros((len(seeds), len(gids)), np.int32)
    for k, seed in enumerate(seeds):
        for i, gid in enumerate(gids):
            d_octree, material, hit = first(h_octree, seed, gid)
            d_world = first(h_world, seed, gid)[0] if world else d_octree
            d_full = first(h_full, seed, gid)[0] if actor else d_world
            if d_full < d_world:
                out[k, i] = ACTOR
            elif d_world < d_octree:
                out[k, i] = WORLD
            else:
                out[k, i] = material if hit else SKY
    return out


def empty_state(n):
    return np.zeros((SLOTS, n), np.int32), np.zeros((SLOTS, n), np.int32), np.zeros(n, np.int32)


def fold(sample_ids, state=None):
    """The state (ids (6, n), counts (6, n), other (n,)) after the samples (n_passes, n), continued from `state`: per sample the first
    occupied slot that holds the id counts it, else the first empty slot takes it, else `other` does."""
    s = np.asarray(sample_ids, np.int32)
    n = s.shape[1]
    ids, counts, other = empty_state(n) if state is None else tuple(np.array(a, np.int32) for a in state)
    for row in s:
        for i, v in enumerate(row):
            match = np.flatnonzero((counts[:, i] > 0) & (ids[:, i] == v))
            free = np.flatnonzero(counts[:, i] == 0)
            if len(match):
                counts[match[0], i] += 1
            elif len(free):
                ids[free[0], i] = v
                counts[free[0], i] = 1
            else:
                other[i] += 1
    return ids, counts, other


def ranks(ids, counts, passes):
    """(ids (6, n) int32, coverage (6, n) float32): slots by count descending, ties by the lower slot; empty slots last as (EMPTY, 0)."""
    ids, counts = np.asarray(ids, np.int32), np.asarray(counts, np.int32)
    order = np.argsort(-counts.astype(np.int64), axis=0, kind="stable")
    c = np.take_along_axis(counts, order, axis=0)
    i = np.take_along_axis(ids, order, axis=0)
    cov = c.astype(np.float32) / np.float32(passes)   # int -> float rounds to nearest; one float32 division
    return np.where(c > 0, i, EMPTY).astype(np.int32), np.where(c > 0, cov, np.float32(0)).astype(np.float32)


def extract(ids, counts, passes, id_set):
    """(n,) float32: (float)(the counts of the occupied slots whose id is in the set, added as integers) / (float)passes."""
    ids, counts = np.asarray(ids, np.int32), np.asarray(counts, np.int32)
    member = np.isin(ids, np.asarray(list(id_set), np.int64).astype(np.int32)) & (counts > 0)
    total = np.where(member, counts, 0).astype(np.int64).sum(axis=0)
    return total.astype(np.int32).astype(np.float32) / np.float32(passes)
