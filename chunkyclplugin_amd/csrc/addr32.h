// addr32.h — which scene arrays kernels may read as "kernel-argument base + 32-bit unsigned byte offset" (SceneView::addr32).
// Plain C++: scene_records.cpp (addr32_word) sets the bits at upload, rt_device.hpp names with them the arrays a translation unit's
// kernels read that way (CHUNKY_ADDR32_FORMS), and launch_render starts such kernels only for a scene whose word has those bits.
//
// A bit is set only where the offset cannot wrap and cannot come from an index nobody bounded: an unsigned offset made from a negative
// index is 4 GB away from where the signed 64-bit form would have read.
#pragma once

namespace chunky {

enum : unsigned {
    // atlas_texel: atlas_w, atlas_h and atlas_layers * atlas_h < 2^24 (the factors of two v_mad_u32_u24), the atlas < 2^32 bytes.
    // x, y and the layer are clamped in the kernel, whatever the material says.
    kAddr32Atlas = 1,
    // sky_fetch: sky_w * 16 (a row's pitch, a 24-bit factor) and sky_h < 2^24, the sky < 2^32 bytes.  rt_mirror_linear clamps both indices.
    kAddr32Sky = 2,
    // aabb_rec and quad_rec each < 2^32 bytes.  The index is a record number, 24 bits of block_info word 7, plus a count of 8 bits —
    // bounded by their width even where a hostile (odd) block pointer makes the kernel read that word from the wrong place; the offsets
    // are then the very addresses the 64-bit form computes.  mat8 is NOT in this set: its index is read out of a record (see
    // material_sample8); block_info neither (an unsigned index already; rt_device.hpp block_hit says why it stays).
    kAddr32Records = 4,
};

}  // namespace chunky
