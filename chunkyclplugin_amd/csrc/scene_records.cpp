// scene_records.cpp — the host-only derivation of scene_records.hpp.  No <hip/hip_runtime.h>: the arithmetic is rt_math.h's, the
// same expressions the kernels evaluate, so a stored float is the one a kernel would compute.
#include "scene_records.hpp"

#include <algorithm>
#include <cstddef>
#include <utility>

#include "rt_math.h"

namespace chunky {

// quad_aux (rt_device.hpp): for every quad of every quad model the block palette points at, the
// ray-independent values of K/primitives.h:262-276 — normalize(cross(xv, yv)), dot(n, origin), dot(xv, xv),
// dot(yv, yv) — written at the quad's own int offset.  Same rt_math.h expressions as the kernel, so
// the stored floats are the ones the kernel would compute.  Returns false (no table) when two
// models overlap in a way that would make entries collide, or a pointer leaves the array.
bool build_quad_aux(const std::vector<int32_t>& B, const std::vector<int32_t>& Q, std::vector<float>* out) {
    out->assign(Q.size(), 0.0f);
    std::vector<int64_t> owner(Q.size(), -1);
    bool any = false;
    for (size_t k = 0; k + 1 < B.size(); k += 2) {
        if (B[k] != 3) continue;
        const int64_t ptr = B[k + 1];
        if (ptr < 0 || (size_t)ptr >= Q.size()) return false;
        const int64_t count = Q[(size_t)ptr];
        if (count < 0 || (size_t)(ptr + 1 + 15 * count) > Q.size()) return false;
        for (int64_t i = 0; i < count; i++) {
            const int64_t q = ptr + 1 + 15 * i;
            for (int w = 0; w < 6; w++) {
                if (owner[(size_t)(q + w)] >= 0 && owner[(size_t)(q + w)] != q) return false;
                owner[(size_t)(q + w)] = q;
            }
            float f[9];
            memcpy(f, &Q[(size_t)q], sizeof f);
            const float cx = rt_cross_c(f[4], f[8], f[5], f[7]), cy = rt_cross_c(f[5], f[6], f[3], f[8]),
                        cz = rt_cross_c(f[3], f[7], f[4], f[6]);
            const float rl = rt_rlen3(cx, cy, cz);
            const float nx = cx * rl, ny = cy * rl, nz = cz * rl;
            float* a = out->data() + q;
            a[0] = nx;
            a[1] = ny;
            a[2] = nz;
            a[3] = rt_dot3(nx, ny, nz, f[0], f[1], f[2]);
            a[4] = rt_dot3(f[3], f[4], f[5], f[3], f[4], f[5]);
            a[5] = rt_dot3(f[6], f[7], f[8], f[6], f[7], f[8]);
            any = true;
        }
    }
    return any;
}

int model_leaf_permille(const std::vector<int32_t>& T, const std::vector<int32_t>& B) {
    int64_t cubes = 0, models = 0;
    for (const int32_t v : T) {
        if (v > 0) continue;  // a branch
        const int64_t ptr = -(int64_t)v;
        if (ptr == 0 || ptr + 1 >= (int64_t)B.size()) continue;  // air, ANY_TYPE, a pointer beyond the palette
        const int32_t type = B[(size_t)ptr];
        cubes += type == 1;
        models += type == 2 || type == 3;
    }
    return cubes + models > 0 ? (int)(models * 1000 / (cubes + models)) : 0;
}

unsigned addr32_word(const AddrBounds& b) {
    constexpr int64_t k24 = (int64_t)1 << 24;
    constexpr uint64_t k32 = (uint64_t)1 << 32;
    unsigned word = 0;
    // (dimensions below 2^24 and a product below 2^32 bytes: nothing here overflows 64 bits)
    if (b.atlas_w > 0 && b.atlas_h > 0 && b.atlas_layers > 0 && b.atlas_w < k24 && b.atlas_h < k24 && b.atlas_layers < k24 &&
        b.atlas_layers * b.atlas_h < k24 && (uint64_t)(b.atlas_layers * b.atlas_h) * (uint64_t)b.atlas_w * 4 < k32)
        word |= kAddr32Atlas;
    if (b.sky_w > 0 && b.sky_h > 0 && b.sky_w * 16 < k24 && b.sky_h < k24 && (uint64_t)b.sky_w * (uint64_t)b.sky_h * 16 < k32) word |= kAddr32Sky;
    if (b.indices_checked && b.aabb_rec_bytes < k32 && b.quad_rec_bytes < k32) word |= kAddr32Records;
    return word;
}

void derive_records(const std::vector<int32_t>& B, const std::vector<int32_t>& M, const std::vector<int32_t>& A, const std::vector<int32_t>& Q,
                    DerivedRecords* out) {
    const size_t n_blocks = B.size() / 2, n_mats = M.size() / 6;
    std::vector<int32_t>&mat8 = out->mat8, &info = out->info, &aabb_rec = out->aabb_rec, &quad_rec = out->quad_rec;
    mat8.assign(n_mats * 8, 0);
    for (size_t m = 0; m < n_mats; m++)
        for (int w = 0; w < 6; w++) mat8[m * 8 + w] = M[m * 6 + w];  // word 5 (spec | metal | rough) rides in the second word
    auto mat_index = [&](int32_t ptr, int32_t* out) {  // packed material pointer -> index of its first 16-byte word in mat8
        if (ptr < 0 || ptr % 6 != 0 || (size_t)ptr / 6 >= n_mats) return false;
        *out = (ptr / 6) * 2;
        return true;
    };
    info.assign(n_blocks * 8, 0);
    aabb_rec.clear();
    quad_rec.clear();
    std::vector<int64_t> aabb_at(A.size(), -1), quad_at(Q.size(), -1);  // model pointer -> first record (models are shared between blocks)
    for (size_t k = 0; k < n_blocks; k++) {
        int32_t* e = &info[k * 8];
        const int32_t type = B[2 * k], ptr = B[2 * k + 1];
        e[0] = type;
        e[1] = ptr;
        if (type == 1) {
            if (ptr >= 0 && (size_t)ptr + 5 <= M.size()) {
                for (int w = 0; w < 5; w++) e[2 + w] = M[(size_t)ptr + w];
                if ((size_t)ptr + 6 <= M.size()) e[7] = M[(size_t)ptr + 5];  // material word 5 (extensions)
            } else {
                e[0] = 0x7FFFFFFF;  // malformed cube: an unknown model type never hits (K/block.h:44-47)
            }
        } else if (type == 2 || type == 3) {
            // A model whose pointer, primitive count or material pointers leave their palettes would make the kernels read outside
            // device memory (the reference has no such check: its behaviour there is undefined).  Such a block never hits, like
            // an unknown model type (K/block.h:44-47); every well-formed block is untouched by this.
            const std::vector<int32_t>& P = type == 2 ? A : Q;
            const int64_t stride = type == 2 ? 13 : 15;
            bool sound = ptr >= 0 && (size_t)ptr < P.size();
            if (sound) {
                const int64_t count = P[(size_t)ptr];
                sound = count >= 0 && (size_t)(ptr + 1 + stride * count) <= P.size();
                for (int64_t i = 0; sound && i < count; i++) {
                    const int32_t* prim = &P[(size_t)(ptr + 1 + stride * i)];
                    if (type == 2) {
                        for (int w = 1; w < 6 && sound; w++) sound = prim[7 + w] >= 0 && (size_t)prim[7 + w] + 6 <= M.size();  // E, S, W, T, B: the ones that are read
                    } else {
                        sound = prim[13] >= 0 && (size_t)prim[13] + 6 <= M.size();
                    }
                }
            }
            if (!sound) e[0] = 0x7FFFFFFF;
        }
        if (e[0] == 2) {
            const int64_t count = A[(size_t)ptr];
            if (count < 1 || count > 255) continue;
            if (aabb_at[(size_t)ptr] < 0) {
                const int64_t first = (int64_t)aabb_rec.size() / 12;
                bool ok = true;
                std::vector<int32_t> rec((size_t)count * 12);
                for (int64_t i = 0; i < count && ok; i++) {
                    const int32_t* b = &A[(size_t)(ptr + 1 + 13 * i)];
                    int32_t* r = &rec[(size_t)i * 12];
                    for (int w = 0; w < 7; w++) r[w] = b[w];  // six bounds, flags
                    for (int w = 0; w < 5 && ok; w++) ok = mat_index(b[8 + w], &r[7 + w]);  // E, S, W, T, B (N is never read: K/primitives.h:209-234)
                }
                if (!ok) {
                    aabb_at[(size_t)ptr] = -2;
                } else {
                    aabb_at[(size_t)ptr] = first;
                    aabb_rec.insert(aabb_rec.end(), rec.begin(), rec.end());
                }
            }
            if (aabb_at[(size_t)ptr] >= 0 && aabb_at[(size_t)ptr] < (1 << 22)) e[7] = (int32_t)((aabb_at[(size_t)ptr] << 8) | count);
        } else if (e[0] == 3) {
            const int64_t count = Q[(size_t)ptr];
            if (count < 1 || count > 255) continue;
            if (quad_at[(size_t)ptr] < 0) {
                const int64_t first = (int64_t)quad_rec.size() / 24;
                bool ok = true;
                std::vector<int32_t> rec((size_t)count * 24);
                for (int64_t i = 0; i < count && ok; i++) {
                    const int32_t* q = &Q[(size_t)(ptr + 1 + 15 * i)];
                    float f[9];
                    memcpy(f, q, sizeof f);
                    const float cx = rt_cross_c(f[4], f[8], f[5], f[7]), cy = rt_cross_c(f[5], f[6], f[3], f[8]),
                                cz = rt_cross_c(f[3], f[7], f[4], f[6]);
                    const float rl = rt_rlen3(cx, cy, cz);
                    const float nx = cx * rl, ny = cy * rl, nz = cz * rl;
                    const float aux[6] = {nx, ny, nz, rt_dot3(nx, ny, nz, f[0], f[1], f[2]), rt_dot3(f[3], f[4], f[5], f[3], f[4], f[5]),
                                          rt_dot3(f[6], f[7], f[8], f[6], f[7], f[8])};
                    int32_t a[6];
                    memcpy(a, aux, sizeof a);
                    int32_t* r = &rec[(size_t)i * 24];
                    r[0] = q[0]; r[1] = q[1]; r[2] = q[2]; r[3] = a[3];      // origin, dot(n, origin)
                    r[4] = q[3]; r[5] = q[4]; r[6] = q[5]; r[7] = a[4];      // xv, |xv|^2
                    r[8] = q[6]; r[9] = q[7]; r[10] = q[8]; r[11] = a[5];    // yv, |yv|^2
                    r[12] = q[9]; r[13] = q[10]; r[14] = q[11]; r[15] = q[12];  // uv
                    r[16] = a[0]; r[17] = a[1]; r[18] = a[2];                // unit normal
                    int32_t m8 = 0;
                    ok = mat_index(q[13], &m8);                              // the quad's material, inline: one dependent read less
                    if (ok && (M[(size_t)q[13]] & 2)) ok = false;          // an emittance texture needs the full word: packed path
                    if (ok) {
                        const int32_t* m = &M[(size_t)q[13]];
                        r[19] = (m[4] & 0xFF) | (int32_t)((uint32_t)m[5] << 8);
                        r[20] = m[0]; r[21] = m[1]; r[22] = m[2]; r[23] = m[3];
                    }
                }
                if (!ok) {
                    quad_at[(size_t)ptr] = -2;
                } else {
                    quad_at[(size_t)ptr] = first;
                    quad_rec.insert(quad_rec.end(), rec.begin(), rec.end());
                }
            }
            if (quad_at[(size_t)ptr] >= 0 && quad_at[(size_t)ptr] < (1 << 22)) e[7] = (int32_t)((quad_at[(size_t)ptr] << 8) | count);
        }
    }
}

// The two entity BVHs re-laid out for aligned 16-byte reads (rt_device.hpp has the layouts): every inner node becomes a
// 64-byte record holding BOTH children (their references and boxes — what one visit of K/bvh.h:72-85 reads), every
// triangle an 80-byte record with its material as a mat8 index.  A reference is the index of an inner record, or
// -1 - (first triangle record << 6 | count) for a leaf.  The walk order, the tests and the arithmetic stay the reference's.
// Returns false (no records: the packed arrays are walked as they are) when something does not fit: a leaf of more than
// 63 triangles, a triangle pointer outside the palette, a material pointer that is not a whole material.
// Placement of the inner records of one BVH (records [lo, hi) of bvh_rec, root reference *root): the first `top` records
// breadth-first from the root (the levels every walk crosses, contiguous), then every subtree below that cut as depth-first
// TREELETS of at most `treelet` records, each treelet breadth-first from its own root — a walker that enters a treelet finds
// its next few visits in the same 1–2 KB.  References are renumbered; nothing else changes.
static void relayout_bvh_records(std::vector<int32_t>* bvh_rec, size_t lo, size_t hi, int* root, int top, int treelet) {
    if (hi <= lo || *root < 0) return;
    const size_t n = hi - lo;
    std::vector<int32_t> order;  // order[k] = old index of the record that moves to lo + k
    order.reserve(n);
    auto rec = [&](int32_t idx) { return &(*bvh_rec)[(size_t)idx * 16]; };
    std::vector<int32_t> frontier{*root};
    {   // the top, breadth-first
        size_t head = 0;
        while (head < frontier.size() && order.size() < (size_t)top) {
            const int32_t at = frontier[head++];
            order.push_back(at);
            for (int c = 0; c < 2; c++)
                if (rec(at)[c] >= 0) frontier.push_back(rec(at)[c]);
        }
        frontier.erase(frontier.begin(), frontier.begin() + (ptrdiff_t)head);
    }
    // below the cut: treelets, depth-first (a stack of treelet roots; the first child's treelet follows its parent's)
    std::vector<int32_t> roots(frontier.rbegin(), frontier.rend()), members, next;
    while (!roots.empty()) {
        members.assign(1, roots.back());
        roots.pop_back();
        next.clear();
        for (size_t head = 0; head < members.size(); head++) {
            const int32_t at = members[head];
            order.push_back(at);
            for (int c = 0; c < 2; c++) {
                const int32_t r = rec(at)[c];
                if (r < 0) continue;
                if (members.size() < (size_t)treelet) members.push_back(r); else next.push_back(r);
            }
        }
        roots.insert(roots.end(), next.rbegin(), next.rend());
    }
    if (order.size() != n) return;  // (cannot happen: every record of the range hangs under the root exactly once)
    std::vector<int32_t> where(n), moved(n * 16);
    for (size_t k = 0; k < n; k++) where[(size_t)order[k] - lo] = (int32_t)(lo + k);
    for (size_t k = 0; k < n; k++) {
        const int32_t* from = rec(order[k]);
        int32_t* to = &moved[k * 16];
        std::copy(from, from + 16, to);
        for (int c = 0; c < 2; c++)
            if (to[c] >= 0) to[c] = where[(size_t)to[c] - lo];
    }
    std::copy(moved.begin(), moved.end(), bvh_rec->begin() + (ptrdiff_t)(lo * 16));
    *root = where[(size_t)*root - lo];
}

// Triangle records in the order in which the inner records (as placed) refer to their leaves, so that the leaves under one
// treelet lie together.  A leaf shared by several references moves once.
static void reorder_triangles(std::vector<int32_t>* bvh_rec, std::vector<int32_t>* tri_rec, int* world_root, int* actor_root) {
    const size_t n_tri = tri_rec->size() / 20;
    std::vector<int32_t> moved;
    moved.reserve(tri_rec->size());
    std::vector<int32_t> first_at(n_tri + 1, -1);  // old first triangle of a leaf -> new
    auto move_leaf = [&](int32_t* ref) {
        if (*ref >= 0) return;
        const int32_t l = -1 - *ref, first = l >> 6, count = l & 63;
        if (count == 0 || (size_t)first + (size_t)count > n_tri) return;
        if (first_at[(size_t)first] < 0) {
            first_at[(size_t)first] = (int32_t)(moved.size() / 20);
            moved.insert(moved.end(), tri_rec->begin() + (ptrdiff_t)first * 20, tri_rec->begin() + (ptrdiff_t)(first + count) * 20);
        }
        *ref = -1 - ((first_at[(size_t)first] << 6) | count);
    };
    move_leaf(world_root);
    move_leaf(actor_root);
    for (size_t k = 0; k < bvh_rec->size() / 16; k++) {
        move_leaf(&(*bvh_rec)[k * 16]);
        move_leaf(&(*bvh_rec)[k * 16 + 1]);
    }
    tri_rec->swap(moved);  // every reference now points into `moved`
}

bool build_bvh_records(const std::vector<int32_t>& world_nodes, bool world_empty, const std::vector<int32_t>& actor_nodes, bool actor_empty,
                       const std::vector<int32_t>& T, const std::vector<int32_t>& M, int top, int treelet, std::vector<int32_t>* bvh_rec,
                       std::vector<int32_t>* tri_rec, int* world_root, int* actor_root) {
    const size_t n_mats = M.size() / 6;
    std::vector<int64_t> leaf_at(T.size(), -1);  // triangle pointer -> its leaf reference (leaves may be shared)
    auto leaf_ref = [&](int64_t prim, int32_t* ref) {
        if (prim < 0 || (size_t)prim >= T.size()) return false;
        if (leaf_at[(size_t)prim] >= 0) {
            *ref = (int32_t)(-1 - leaf_at[(size_t)prim]);
            return true;
        }
        const int64_t count = T[(size_t)prim];
        if (count < 0 || count > 63 || (size_t)(prim + 1 + 20 * count) > T.size()) return false;
        const int64_t first = (int64_t)tri_rec->size() / 20;
        if (first >= (1 << 24)) return false;
        for (int64_t i = 0; i < count; i++) {
            const int32_t* t = &T[(size_t)(prim + 1 + 20 * i)];
            const int32_t mp = t[19];
            if (mp < 0 || mp % 6 != 0 || (size_t)mp / 6 >= n_mats) return false;
            const int32_t r[20] = {t[1], t[2], t[3], t[0],             // e1, flags
                                   t[4], t[5], t[6], (mp / 6) * 2,     // e2, material (mat8 index)
                                   t[7], t[8], t[9], t[13],            // o, t1.u
                                   t[10], t[11], t[12], t[14],         // n, t1.v
                                   t[15], t[16], t[17], t[18]};        // t2.u, t2.v, t3.u, t3.v
            tri_rec->insert(tri_rec->end(), r, r + 20);
        }
        leaf_at[(size_t)prim] = (first << 6) | count;
        *ref = (int32_t)(-1 - leaf_at[(size_t)prim]);
        return true;
    };
    auto build = [&](const std::vector<int32_t>& N, bool empty, int* root) {
        *root = 0;
        if (empty || N.size() < 7) return true;
        // reference of the node at int offset `at`: inner nodes get records in visiting (depth-first) order
        std::vector<std::pair<int64_t, int64_t>> todo;  // (node offset, index of the int in bvh_rec that receives its reference)
        int32_t root_ref = 0;
        // iterative: slot index -1 means the root reference
        todo.emplace_back(0, -1);
        int64_t guard = 0;
        while (!todo.empty()) {
            auto [at, slot] = todo.back();
            todo.pop_back();
            if (at < 0 || (size_t)at + 7 > N.size() || ++guard > (int64_t)N.size()) return false;
            const int32_t head = N[(size_t)at];
            int32_t ref;
            if (head <= 0) {
                if (!leaf_ref(-(int64_t)head, &ref)) return false;
            } else {
                const int64_t a = at + 7, b = head;
                if ((size_t)a + 7 > N.size() || b < 0 || (size_t)b + 7 > N.size()) return false;
                const int64_t idx = (int64_t)bvh_rec->size() / 16;
                if (idx >= (1 << 24)) return false;  // (with at most 2^24 triangles: every record within 32-bit byte offsets)
                ref = (int32_t)idx;
                bvh_rec->resize(bvh_rec->size() + 16, 0);
                int32_t* r = &(*bvh_rec)[(size_t)idx * 16];
                for (int w = 0; w < 6; w++) {
                    r[4 + w] = N[(size_t)a + 1 + w];    // first child's box  (words 1, 2.xy)
                    r[10 + w] = N[(size_t)b + 1 + w];   // second child's box (words 2.zw, 3)
                }
                todo.emplace_back(b, idx * 16 + 1);
                todo.emplace_back(a, idx * 16 + 0);
            }
            if (slot < 0) root_ref = ref; else (*bvh_rec)[(size_t)slot] = ref;
        }
        *root = root_ref;
        return true;
    };
    bvh_rec->clear();
    tri_rec->clear();
    if (!build(world_nodes, world_empty, world_root)) return false;
    const size_t world_records = bvh_rec->size() / 16;
    if (!build(actor_nodes, actor_empty, actor_root)) return false;
    // where the records sit (addresses only: the walk's order, tests and arithmetic do not see it)
    if (treelet > 1) {
        relayout_bvh_records(bvh_rec, 0, world_records, world_root, top, treelet);
        relayout_bvh_records(bvh_rec, world_records, bvh_rec->size() / 16, actor_root, top, treelet);
        reorder_triangles(bvh_rec, tri_rec, world_root, actor_root);
    }
    return true;
}

// Height of the tree = most entries the to-visit stack can hold; also rejects child links that leave the array or form a cycle (a
// malformed BVH would hang the traversal)
bool bvh_links_height(const std::vector<int32_t>& N, int* height) {
    const int64_t n = (int64_t)N.size();
    *height = 0;
    std::vector<std::pair<int64_t, int>> todo;
    todo.emplace_back(0, 0);
    int64_t visited = 0;
    while (!todo.empty()) {
        auto [at, d] = todo.back();
        todo.pop_back();
        if (at < 0 || at + 7 > n || ++visited > n) return false;
        if (d > *height) *height = d;
        const int32_t head = N[(size_t)at];
        if (head > 0) {
            todo.emplace_back(at + 7, d + 1);
            todo.emplace_back((int64_t)head, d + 1);
        }
    }
    return *height <= 63;
}

// Every leaf of an entity BVH has to lie inside the triangle palette, every triangle's material inside the material palette: the
// kernels follow these ints as they are (the reference does too — with hostile data its reads are undefined; here the render call
// is refused instead).  Node links were checked by chunky_scene_set_bvh (bvh_links_height).
bool bvh_leaves_sound(const std::vector<int32_t>& N, bool empty, const std::vector<int32_t>& T, const std::vector<int32_t>& M) {
    if (empty || N.size() < 7) return true;
    std::vector<int64_t> todo{0};  // the nodes the walk can reach (first child at +7, second at node[0]: K/bvh.h:72-85)
    size_t visited = 0;
    while (!todo.empty()) {
        const int64_t at = todo.back();
        todo.pop_back();
        if (at < 0 || (size_t)at + 7 > N.size() || ++visited > N.size()) return false;
        const int32_t head = N[(size_t)at];
        if (head > 0) {
            todo.push_back(at + 7);
            todo.push_back((int64_t)head);
            continue;
        }
        const int64_t prim = -(int64_t)head;
        if ((size_t)prim >= T.size()) return false;
        const int64_t count = T[(size_t)prim];
        if (count < 0 || (size_t)(prim + 1 + 20 * count) > T.size()) return false;
        for (int64_t i = 0; i < count; i++) {
            const int32_t mp = T[(size_t)(prim + 20 + 20 * i)];  // word 19 of the triangle
            if (mp < 0 || (size_t)mp + 6 > M.size()) return false;
        }
    }
    return true;
}

// The emitter list of the next-event-estimation extension (same rule and order as oracle/port.c
// port_list_emitters): every octree leaf whose block is a full cube with a non-zero emittance byte and no emittance
// texture, in pre-order (children in index order), as {x, y, z, level << 25 | block pointer}.
void list_emitters(const std::vector<int32_t>& T, int depth, const std::vector<int32_t>& B, const std::vector<int32_t>& M, std::vector<int32_t>* out) {
    out->clear();
    if (T.empty() || depth < 0 || depth > 15) return;
    struct Item { int64_t node; int x, y, z, level; };
    std::vector<Item> todo{{0, 0, 0, 0, depth}};
    // chunky_scene_set_octree only checks that branch values stay inside the array: a tree with a cycle, or with branches
    // below level 0, must not make this walk run or allocate without end — the kernels' walk is bounded by the depth, so
    // here a node at level 0 is a leaf whatever it holds, and no more nodes are visited than the array has
    size_t visited = 0;
    while (!todo.empty()) {
        const Item it = todo.back();
        todo.pop_back();
        if (++visited > T.size()) break;
        const int32_t v = T[(size_t)it.node];
        if (v > 0 && it.level > 0) {
            const int h = 1 << (it.level - 1);
            for (int c = 7; c >= 0; c--)  // pushed in reverse: popped in index order
                todo.push_back({(int64_t)v + c, it.x + ((c >> 2) & 1) * h, it.y + ((c >> 1) & 1) * h, it.z + (c & 1) * h, it.level - 1});
            continue;
        }
        if (v > 0) continue;  // a branch below level 0: not a leaf the kernels can reach
        const int64_t block = -(int64_t)v;
        if (block == 0 || block == 0x7FFFFFFE || block + 1 >= (int64_t)B.size() || block >= (1 << 25)) continue;
        if (B[(size_t)block] != 1) continue;
        const int64_t mp = B[(size_t)block + 1];
        if (mp < 0 || (size_t)mp + 6 > M.size()) continue;
        if ((M[(size_t)mp] & 2) || (M[(size_t)mp + 4] & 0xFF) == 0) continue;
        const int32_t rec[4] = {it.x, it.y, it.z, (int32_t)((it.level << 25) | (int32_t)block)};
        out->insert(out->end(), rec, rec + 4);
    }
}

}  // namespace chunky
