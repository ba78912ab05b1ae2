"""The antialiased ID mattes without a device: the host twins (csrc/matte_host.cpp, the arithmetic of csrc/matte_spec.h) against the
numpy restatement in matte_spec.py on random id streams, the state check, the extract's corner cases, the id derivation on the C
restatement against the reference build, and the ABI's symbols."""
import re

import numpy as np
import pytest

from oracle import binding

import golden_scenes as gs
import matte_spec as ms
from chunkyclplugin_amd import native

FUNCTIONS = ["chunky_render_matte_passes", "chunky_render_matte_reset", "chunky_render_matte_read", "chunky_render_matte_restore",
             "chunky_render_matte_ranks", "chunky_render_matte_extract", "chunky_render_matte_kernel_time", "chunky_render_matte_kernel_info",
             "chunky_matte_host_fold", "chunky_matte_host_ranks", "chunky_matte_host_extract", "chunky_matte_state_check"]
PASSES, PIXELS = 300, 24


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def stream(alphabet, seed):
    """(PASSES, PIXELS) ids drawn from `alphabet` values per pixel: blocks, the sky and the two entity ids among them.  Pixel 0 sees
    six ids and then, from pass 200 on, a seventh (an id that first arrives after the slots are full)."""
    rng = np.random.default_rng(seed)
    pool = np.concatenate([[ms.SKY, ms.WORLD, ms.ACTOR], rng.choice(5000, alphabet, replace=False)]).astype(np.int32)[:alphabet]
    s = pool[rng.integers(0, alphabet, (PASSES, PIXELS))]
    if alphabet > 6:
        s[:200, 0] = pool[rng.integers(0, 6, 200)]
        s[:6, 0] = pool[:6]
        s[200:, 0] = pool[6]
    return np.ascontiguousarray(s, np.int32)


def same_state(got, want):
    for g, w, name in zip(got, want, ("ids", "counts", "other")):
        np.testing.assert_array_equal(g, w, err_msg=name)


def test_header_declares_and_library_exports_the_entry_points():
    text = open(native.HEADER).read()
    for name, value in (("SLOTS", "6"), ("SKY", r"\(-1\)"), ("WORLD_ENTITY", r"\(-2\)"), ("ACTOR_ENTITY", r"\(-3\)"), ("EMPTY", "INT32_MIN")):
        assert re.search(rf"#define\s+CHUNKY_MATTE_{name}\s+{value}", text), name
    assert (native.MATTE_SLOTS, native.MATTE_SKY, native.MATTE_WORLD_ENTITY, native.MATTE_ACTOR_ENTITY, native.MATTE_EMPTY) == (6, -1, -2, -3, -2 ** 31)
    declared = native.declared_symbols()
    L = native.lib()
    for name in FUNCTIONS:
        assert name in declared, name
        assert hasattr(L, name), name
        assert getattr(L, name).argtypes is not None, name   # native.py gives it a prototype
    for src in ("matte.hip", "capi_matte.hip", "matte_host.cpp"):
        assert src in native.SOURCES


def test_null_handles_are_errors():
    L = native.lib()
    seeds = np.zeros(2, np.int32)
    a = np.zeros(12, np.int32)
    assert L.chunky_render_matte_passes(None, seeds.ctypes.data, 2) == native.E_INVALID
    assert L.chunky_render_matte_passes(None, seeds.ctypes.data, -1) == native.E_INVALID
    assert L.chunky_render_matte_reset(None) == native.E_INVALID
    assert L.chunky_render_matte_ranks(None, a.ctypes.data, a.ctypes.data, 2) == native.E_INVALID
    assert L.chunky_render_matte_extract(None, None, 0, a.ctypes.data, 2) == native.E_INVALID
    assert L.chunky_render_matte_kernel_info(None, a.ctypes.data) == native.E_INVALID
    assert b"NULL" in L.chunky_last_error()


@pytest.mark.parametrize("alphabet", [3, 40])
def test_host_fold_ranks_extract_on_random_streams(alphabet):
    s = stream(alphabet, alphabet)
    want = ms.fold(s)
    got = native.matte_host_fold(s)
    same_state(got, want)
    ids, counts, other = got
    assert (counts.sum(axis=0) + other == PASSES).all()
    if alphabet == 3:
        assert not other.any() and (counts[3:] == 0).all() and (counts[:3] > 0).all()
    else:
        assert (other > 0).all() and (counts > 0).all()                     # every pixel overflows: rule 3
        assert other[0] == 100 and s[200, 0] not in ids[:, 0]               # the late id found no slot
        assert native.matte_state_check(ids, counts, other, PASSES) == 0
    # split in two: the same state
    half = native.matte_host_fold(s[137:], native.matte_host_fold(s[:137]))
    same_state(half, want)
    same_state(native.matte_host_fold(s[:0], want), want)                   # and no pass changes nothing
    # ranks: ids and coverage bits
    r_ids, r_cov = native.matte_host_ranks(ids, counts, PASSES)
    w_ids, w_cov = ms.ranks(ids, counts, PASSES)
    np.testing.assert_array_equal(r_ids, w_ids)
    np.testing.assert_array_equal(bits(r_cov), bits(w_cov))
    assert (np.diff(r_cov, axis=0) <= 0).all()
    # extract
    for id_set in ([ms.SKY], [ms.WORLD, ms.ACTOR], list(np.unique(s)[::2]) * 2, []):
        np.testing.assert_array_equal(bits(native.matte_host_extract(ids, counts, PASSES, id_set)), bits(ms.extract(ids, counts, PASSES, id_set)), err_msg=str(id_set)[:40])
    everything = native.matte_host_extract(ids, counts, PASSES, np.unique(s))
    np.testing.assert_array_equal(bits(everything), bits((PASSES - other).astype(np.float32) / np.float32(PASSES)))   # `other` belongs to no id


def test_rank_ties_and_rounding():
    """Equal counts keep their slot order, empty slots come last, and counts above 2^24 round in the conversion."""
    ids = np.array([[7, 7, 7], [5, 5, 5], [9, 9, 9], [3, 3, 0], [11, 0, 0], [2, 0, 0]], np.int32)
    counts = np.array([[4, 1, 2 ** 24 + 1], [4, 5, 2 ** 24 + 3], [9, 5, 1], [4, 1, 0], [1, 0, 0], [4, 0, 0]], np.int32)
    passes = int(counts.sum(axis=0).max())
    r_ids, r_cov = native.matte_host_ranks(ids, counts, passes)
    assert r_ids[:, 0].tolist() == [9, 7, 5, 3, 2, 11]
    assert r_ids[:, 1].tolist() == [5, 9, 7, 3, ms.EMPTY, ms.EMPTY] and r_cov[4:, 1].tolist() == [0, 0]
    assert r_ids[:, 2].tolist() == [5, 7, 9, ms.EMPTY, ms.EMPTY, ms.EMPTY]
    w_ids, w_cov = ms.ranks(ids, counts, passes)
    np.testing.assert_array_equal(r_ids, w_ids)
    np.testing.assert_array_equal(bits(r_cov), bits(w_cov))
    assert np.float32(2 ** 24 + 1) == np.float32(2 ** 24)   # (the conversion does round here)
    np.testing.assert_array_equal(bits(native.matte_host_extract(ids, counts, passes, [5, 7])), bits(ms.extract(ids, counts, passes, [5, 7])))


def folded():
    s = stream(40, 9)
    return native.matte_host_fold(s)


def test_state_check():
    ids, counts, other = folded()
    assert native.matte_state_check(ids, counts, other, PASSES) == 0
    empty = ms.empty_state(PIXELS)
    assert native.matte_state_check(*empty, 0) == 0 and native.matte_state_check(*empty, 17) == 0   # a shard's foreign pixels
    L = native.lib()

    def refused(change, passes=PASSES, word=None):
        i, c, o = ids.copy(), counts.copy(), other.copy()
        change(i, c, o)
        assert native.matte_state_check(i, c, o, passes) == native.E_INVALID
        if word:
            assert word in L.chunky_last_error(), L.chunky_last_error()

    def negative_count(i, c, o):
        c[2, 3] = -1

    def negative_other(i, c, o):
        o[5] = -1

    def hole(i, c, o):
        o[4] += c[1, 4]
        c[1, 4] = 0

    def twice(i, c, o):
        i[4, 6] = i[1, 6]

    def empty_id(i, c, o):
        i[5, 7] = ms.EMPTY

    def wrong_sum(i, c, o):
        c[0, 8] += 1

    refused(negative_count, word=b"count -1")
    refused(negative_other, word=b"other = -1")
    refused(hole, word=b"behind an empty slot")
    refused(twice, word=b"in slots 1 and 4")
    refused(empty_id, word=b"CHUNKY_MATTE_EMPTY")
    refused(wrong_sum, word=b"samples after")
    refused(lambda i, c, o: None, passes=PASSES + 1)
    refused(lambda i, c, o: None, passes=-1)
    assert L.chunky_matte_state_check(None, counts.ctypes.data, other.ctypes.data, PIXELS, PASSES) == native.E_INVALID
    assert L.chunky_matte_state_check(ids.ctypes.data, counts.ctypes.data, other.ctypes.data, 0, PASSES) == native.E_INVALID
    # an id of an empty slot is not looked at
    i = ids.copy()
    c, o = ms.empty_state(PIXELS)[1:]
    i[:] = ms.EMPTY
    assert native.matte_state_check(i, c, o, 0) == 0


def test_extract_corner_cases():
    ids, counts, other = folded()
    L = native.lib()
    out = np.full(PIXELS, 7, np.float32)
    dup = native.matte_host_extract(ids, counts, PASSES, [ms.SKY, ms.SKY, ids[0, 0], ms.SKY, ids[0, 0]])
    np.testing.assert_array_equal(bits(dup), bits(native.matte_host_extract(ids, counts, PASSES, [ids[0, 0], ms.SKY])))   # duplicates count once
    assert dup[0] > 0
    assert not bits(native.matte_host_extract(ids, counts, PASSES, [])).any()                                             # the empty set: all +0
    bad = np.array([3, ms.EMPTY], np.int32)
    args = (ids.ctypes.data, counts.ctypes.data, PIXELS)
    assert L.chunky_matte_host_extract(*args, PASSES, bad.ctypes.data, 2, out.ctypes.data) == native.E_INVALID
    assert b"CHUNKY_MATTE_EMPTY" in L.chunky_last_error()
    assert L.chunky_matte_host_extract(*args, 0, bad.ctypes.data, 1, out.ctypes.data) == native.E_INVALID                 # no pass: nothing to divide by
    assert L.chunky_matte_host_extract(*args, PASSES, bad.ctypes.data, -1, out.ctypes.data) == native.E_INVALID
    assert L.chunky_matte_host_extract(*args, PASSES, None, 1, out.ctypes.data) == native.E_INVALID
    assert L.chunky_matte_host_extract(*args, 5, bad.ctypes.data, 1, out.ctypes.data) == native.E_INVALID        # more samples than passes
    assert L.chunky_matte_host_ranks(*args, 0, ids.ctypes.data, out.ctypes.data) == native.E_INVALID
    assert (out == 7).all()                                                                                               # nothing was written
    assert L.chunky_matte_host_extract(*args, PASSES, None, 0, out.ctypes.data) == 0 and not bits(out).any()
    # the fold refuses CHUNKY_MATTE_EMPTY as a sample and states it would push past 2^31 - 1, and changes nothing
    s = np.array([[1] * PIXELS, [ms.EMPTY] + [1] * (PIXELS - 1)], np.int32)
    i, c, o = ids.copy(), counts.copy(), other.copy()
    assert L.chunky_matte_host_fold(s.ctypes.data, 2, PIXELS, i.ctypes.data, c.ctypes.data, o.ctypes.data) == native.E_INVALID
    s[0, 0] = i[0, 0]   # (pixel 0's next sample goes to its slot 0)
    c[0, 0] = 2 ** 31 - 1 - c[1:, 0].sum() - 1
    assert L.chunky_matte_host_fold(s.ctypes.data, 1, PIXELS, i.ctypes.data, c.ctypes.data, o.ctypes.data) == 0
    assert L.chunky_matte_host_fold(s.ctypes.data, 1, PIXELS, i.ctypes.data, c.ctypes.data, o.ctypes.data) == native.E_INVALID


@pytest.mark.parametrize("name", ["entities", "outdoor"])
def test_port_ids_are_the_reference_ids(name):
    ref = binding.ref()
    if ref is None:
        pytest.skip("oracle/_ref not built (needs the reference sources)")
    sc = gs.make(name)
    seeds = native.java_random_ints(gs.N_PASSES)
    on_port = ms.expected_ids(binding.port(), sc, seeds, gs.RECORD_GIDS)
    on_ref = ms.expected_ids(ref, sc, seeds, gs.RECORD_GIDS)
    np.testing.assert_array_equal(on_port, on_ref)
    kinds = {"block": (on_port >= 0).any(), "sky": (on_port == ms.SKY).any(), "world": (on_port == ms.WORLD).any(), "actor": (on_port == ms.ACTOR).any()}
    if name == "entities":
        assert all(kinds.values()), kinds
    else:
        assert kinds["block"] and kinds["sky"] and not kinds["world"] and not kinds["actor"], kinds
