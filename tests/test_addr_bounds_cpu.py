"""The host's decision which scene arrays kernels may read as a scalar base + a 32-bit unsigned byte offset (csrc/scene_records.cpp
addr32_word through chunky_addr32_word; csrc/addr32.h has the bits), at its edges.  No device.

  atlas    width, height and layers * height are 24-bit factors of v_mad_u32_u24; the texel's byte offset has to fit 32 bits
  sky      a row's pitch, width * 16, is a 24-bit factor, the height too; the sky has to be below 2^32 bytes
  records  aabb_rec and quad_rec each below 2^32 bytes, and the library's own (indices_checked)"""
import pytest

from chunkyclplugin_amd import native
from chunkyclplugin_amd.native import ADDR32_ATLAS, ADDR32_RECORDS, ADDR32_SKY

K24, K32 = 1 << 24, 1 << 32


def word(**kw):
    return native.addr32_word(**kw)


def test_a_usual_scene_has_every_bit():
    assert word(atlas=(4096, 4096, 8), sky=(2048, 1024), record_bytes=(1 << 20, 1 << 16)) == ADDR32_ATLAS | ADDR32_SKY | ADDR32_RECORDS
    assert word(atlas=(1, 1, 1), sky=(1, 1), record_bytes=(0, 0)) == ADDR32_ATLAS | ADDR32_SKY | ADDR32_RECORDS   # (no model blocks: empty records)


@pytest.mark.parametrize("atlas,ok", [
    ((K24 - 1, 1, 1), True), ((K24, 1, 1), False),                       # width: 2^24 - 1 against 2^24
    ((1, K24 - 1, 1), True), ((1, K24, 1), False),                       # height
    ((1, 4096, 4095), True), ((1, 4096, 4096), False),                   # layers * height just under and just at 2^24
    ((1, 1, K24 - 1), True), ((1, 1, K24), False),                       # (one row per layer: the layers alone)
    ((2, 4097, 4095), True), ((2, 4097, 4096), False),                   # 4097 * 4095 = 2^24 - 1 rows, 4097 * 4096 = 2^24 + 4096
    ((0, 16, 1), False), ((16, -1, 1), False), ((16, 16, 0), False),     # no atlas
])
def test_atlas_edges(atlas, ok):
    assert bool(word(atlas=atlas) & ADDR32_ATLAS) == ok
    assert word(atlas=atlas) & (ADDR32_SKY | ADDR32_RECORDS) == ADDR32_SKY | ADDR32_RECORDS   # the other arrays do not care


def test_atlas_byte_limit():
    rows = K24 - 1                                # layers * height, a 24-bit factor
    assert rows * 64 * 4 < K32 <= rows * 65 * 4   # 64 columns: just under 2^32 bytes; 65: over
    assert word(atlas=(64, rows, 1)) & ADDR32_ATLAS
    assert not word(atlas=(65, rows, 1)) & ADDR32_ATLAS
    assert word(atlas=(16384, 16384, 3)) & ADDR32_ATLAS and not word(atlas=(16384, 16384, 4)) & ADDR32_ATLAS   # 3 GiB, 4 GiB


@pytest.mark.parametrize("sky,ok", [
    (((K24 >> 4) - 1, 1), True), ((K24 >> 4, 1), False),     # the pitch width * 16: 2^24 - 16 against 2^24
    ((1, K24 - 1), True), ((1, K24), False),                 # height
    ((16, K24 - 1), True), ((17, K24 - 1), False),           # bytes: 16 * (2^24 - 1) * 16 just under 2^32, 17 columns over
    ((16384, 16383), True), ((16384, 16384), False),         # ... and just at 2^32
    ((0, 4), False), ((4, 0), False),
])
def test_sky_edges(sky, ok):
    assert bool(word(sky=sky) & ADDR32_SKY) == ok
    assert word(sky=sky) & ADDR32_ATLAS


@pytest.mark.parametrize("which", [0, 1])
def test_record_array_sizes(which):
    sizes = [4096, 4096]
    sizes[which] = K32 - 16                       # just under 2^32 bytes (whole 16-byte words)
    assert word(record_bytes=tuple(sizes)) & ADDR32_RECORDS
    sizes[which] = K32                            # just at
    assert not word(record_bytes=tuple(sizes)) & ADDR32_RECORDS
    assert word(record_bytes=tuple(sizes)) & (ADDR32_ATLAS | ADDR32_SKY) == ADDR32_ATLAS | ADDR32_SKY


def test_unchecked_indices_say_no():
    assert not word(record_bytes=(4096, 4096), indices_checked=False) & ADDR32_RECORDS
    assert word(record_bytes=(4096, 4096), indices_checked=False) == ADDR32_ATLAS | ADDR32_SKY
