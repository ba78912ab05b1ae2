// scene_records.hpp — everything a scene upload derives on the host from caller-supplied ints (palettes, entity BVHs, the octree):
// plain C++17 over vectors and scalars, no device call.  This is the part hostile scene data reaches first, so
// tests/sanitize/scene_records_fuzz.cpp runs it under AddressSanitizer + UBSan; capi_scene.hip uploads what it returns.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

#include "addr32.h"

namespace chunky {

inline float bits_to_float(int32_t i) {
    float f;
    memcpy(&f, &i, 4);
    return f;
}

// How common model blocks are in a world: octree leaves whose block is an AABB or quad model (types 2, 3), per thousand leaves that
// can be hit at all.  render_pool tests full cubes and model blocks in phases of their own where that pays: the model tests cost
// three times the cube test and a wave runs them whenever ONE lane of a block test has a model block, but a class more costs every
// iteration of every wave 1 % in bookkeeping.  Measured: the benchmark city (110 per thousand; 58 % of the block tests on its saved
// view) +2.3 ... +2.8 %, the synthetic outdoor world (10) +0.1 ... +0.5 %, the same world 16 times larger -1.5 %, the indoor room
// (0.3) -1 %: sorted from 30 per thousand on.  (CHUNKY_OPT_KERNEL bits 8 / 9 force it on / off.)
constexpr int kSortBlocksPermille = 30;
int model_leaf_permille(const std::vector<int32_t>& octree, const std::vector<int32_t>& blocks);

// Everything the kernels read that is derived from the four palettes (rt_device.hpp has the layouts):
//   block_info  per block {type, pointer, 5 material words of a full cube, model record}
//   mat8        materials at a 32-byte stride (two 16-byte reads instead of five unaligned dwords)
//   aabb_rec    AABB-model boxes as three 16-byte words each, materials as mat8 indices
//   quad_rec    quad-model quads as six 16-byte words each (the material's five words inline), with the ray-independent values of K/primitives.h:262-276
//               (unit normal, its dot with the origin, |xv|^2, |yv|^2) evaluated here with the kernel's own rt_math.h
// A block whose model cannot be re-laid out (pointer outside its palette, more than 255 primitives, a material pointer
// that is not a whole material) keeps model record 0 and takes the path that reads the packed palettes as they are.
struct DerivedRecords {
    std::vector<int32_t> info, mat8, aabb_rec, quad_rec;
};
void derive_records(const std::vector<int32_t>& blocks, const std::vector<int32_t>& materials, const std::vector<int32_t>& aabbs,
                    const std::vector<int32_t>& quads, DerivedRecords* out);

// SceneView::addr32 (addr32.h): which arrays the kernels may address as a scalar base + a 32-bit unsigned byte offset.  Sizes are what
// the scene holds (the record arrays in bytes); `indices_checked` says that the record arrays are the ones derive_records built from the
// palettes as they are now (the record numbers in block_info are its own), and not a stale or foreign copy.
struct AddrBounds {
    int64_t atlas_w = 0, atlas_h = 0, atlas_layers = 0, sky_w = 0, sky_h = 0;
    uint64_t aabb_rec_bytes = 0, quad_rec_bytes = 0;
    bool indices_checked = false;
};
unsigned addr32_word(const AddrBounds& b);

// quad_aux (rt_device.hpp), for the quads that kept the packed path; false = no table
bool build_quad_aux(const std::vector<int32_t>& blocks, const std::vector<int32_t>& quads, std::vector<float>* out);

// Child links of a packed entity BVH (7 ints per node, first child at +7, second at node[0]): false when one leaves the array, the
// links form a cycle, or the tree is deeper than the reference's 64-entry to-visit stack (K/bvh.h:38); else *height = its inner levels.
bool bvh_links_height(const std::vector<int32_t>& nodes, int* height);

// Every leaf inside the triangle palette, every triangle's material inside the material palette (links: bvh_links_height)
bool bvh_leaves_sound(const std::vector<int32_t>& nodes, bool empty, const std::vector<int32_t>& trigs, const std::vector<int32_t>& materials);

// Both entity BVHs as 64-byte inner records and 80-byte triangle records, placed as a breadth-first top of `top` records over
// treelets of `treelet` (treelet <= 1: plain depth-first order); false = something does not fit, the packed arrays are walked
bool build_bvh_records(const std::vector<int32_t>& world_nodes, bool world_empty, const std::vector<int32_t>& actor_nodes, bool actor_empty,
                       const std::vector<int32_t>& trigs, const std::vector<int32_t>& materials, int top, int treelet,
                       std::vector<int32_t>* bvh_rec, std::vector<int32_t>* tri_rec, int* world_root, int* actor_root);

// The emitter leaves of the octree as {x, y, z, level << 25 | block pointer}, in pre-order
void list_emitters(const std::vector<int32_t>& octree, int depth, const std::vector<int32_t>& blocks, const std::vector<int32_t>& materials,
                   std::vector<int32_t>* out);

}  // namespace chunky
