// route_pin — which route scene_records.cpp picks for every block and for the entity BVHs of one scene (tests/test_routes_cpu.py).
// Links csrc/scene_records.cpp alone, built with AddressSanitizer + UBSan like the fuzzers beside it.
// Input file: seven arrays (block, material, AABB and quad palettes, world and actor BVH nodes, triangles), each an int64 length
// followed by that many int32, then two int32: world BVH empty, actor BVH empty.
// Output: one JSON line {"word7": [block_info word 7 per block], "type": [block_info word 0 per block], "quad_aux": table built,
// "bvh_records": what build_bvh_records returned, "tri_records": .., "bvh_inner_records": ..}.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../chunkyclplugin_amd/csrc/scene_records.hpp"

static bool read_array(FILE* f, std::vector<int32_t>* out) {
    int64_t n = 0;
    if (fread(&n, sizeof n, 1, f) != 1 || n < 0 || n > (int64_t)1 << 28) return false;
    out->resize((size_t)n);
    return n == 0 || fread(out->data(), 4, (size_t)n, f) == (size_t)n;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<int32_t> B, M, A, Q, WN, AN, T;
    int32_t empty[2] = {1, 1};
    const bool ok = read_array(f, &B) && read_array(f, &M) && read_array(f, &A) && read_array(f, &Q) && read_array(f, &WN) &&
                    read_array(f, &AN) && read_array(f, &T) && fread(empty, 4, 2, f) == 2;
    fclose(f);
    if (!ok) return 3;
    chunky::DerivedRecords d;
    chunky::derive_records(B, M, A, Q, &d);
    std::vector<float> aux;
    const bool have_aux = chunky::build_quad_aux(B, Q, &aux);
    std::vector<int32_t> bvh_rec, tri_rec;
    int world_root = 0, actor_root = 0;
    const bool bvh = chunky::build_bvh_records(WN, empty[0] != 0, AN, empty[1] != 0, T, M, 5, 3, &bvh_rec, &tri_rec, &world_root, &actor_root);
    printf("{\"word7\": [");
    for (size_t k = 0; k < B.size() / 2; k++) printf("%s%d", k ? ", " : "", (int)d.info[k * 8 + 7]);
    printf("], \"type\": [");
    for (size_t k = 0; k < B.size() / 2; k++) printf("%s%d", k ? ", " : "", (int)d.info[k * 8]);
    printf("], \"quad_aux\": %s, \"bvh_records\": %s, \"tri_records\": %zu, \"bvh_inner_records\": %zu}\n", have_aux ? "true" : "false",
           bvh ? "true" : "false", tri_rec.size() / 20, bvh_rec.size() / 16);
    return 0;
}
