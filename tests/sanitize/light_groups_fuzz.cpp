// light_groups_fuzz — the device-free half of the emitter light groups (csrc/lights_host.cpp: light_group_table, light_group_of) in a
// stand-alone program under AddressSanitizer + UBSan.  Links lights_host.cpp and capi_error.cpp and nothing else.  Every array lives
// in a heap block of exactly its size, so a read past the caller's ids or a write past the table is caught.  Driven with: every
// refusal the header names, one by one, each leaving the table it was given untouched; accepted sets against a map written out here;
// palettes of 0, 1, 2 and 3 words; 4000 random sets of hostile ids (odd, negative, INT32_MIN / INT32_MAX, just past the palette,
// duplicates); lookups of ids far beyond a table built for a longer palette.  Prints one JSON line of counts.
#include <climits>
#include <cstdint>
#include <cstdio>
#include <map>
#include <vector>

#include "../../chunkyclplugin_amd/csrc/lights_host.hpp"

static long long failures = 0;
#define EXPECT(cond)                                                       \
    do {                                                                   \
        if (!(cond)) {                                                     \
            if (failures++ < 20) fprintf(stderr, "line %d: %s\n", __LINE__, #cond); \
        }                                                                  \
    } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 16);
}

static const int32_t WORLD = CHUNKY_MATTE_WORLD_ENTITY, ACTOR = CHUNKY_MATTE_ACTOR_ENTITY;
static long long accepted = 0, refused = 0, refusal_kinds = 0, lookups = 0;

// a table that no call below may change when it refuses
static LightGroupTable marked() {
    LightGroupTable t;
    t.n_groups = 5;
    t.of_block = {4, 3, 2, 1};
    t.world = 2, t.actor = 3;
    return t;
}
static bool is_marked(const LightGroupTable& t) {
    return t.n_groups == 5 && t.of_block == std::vector<uint8_t>{4, 3, 2, 1} && t.world == 2 && t.actor == 3;
}

// the call on exact-size heap copies of the caller's arrays
static int build(int n_groups, const std::vector<int32_t>& ids, const std::vector<uint8_t>& groups, int64_t palette_words, LightGroupTable* t) {
    std::vector<int32_t> i(ids);
    std::vector<uint8_t> g(groups);
    i.shrink_to_fit(), g.shrink_to_fit();
    return light_group_table("fuzz", n_groups, i.empty() ? nullptr : i.data(), g.empty() ? nullptr : g.data(), (int)i.size(), palette_words, t);
}

static void refuses(int n_groups, const std::vector<int32_t>& ids, const std::vector<uint8_t>& groups, int64_t palette_words) {
    LightGroupTable t = marked();
    EXPECT(build(n_groups, ids, groups, palette_words, &t) == CHUNKY_E_INVALID);
    EXPECT(is_marked(t));
    refused++, refusal_kinds++;
}

// what the rules say, written with a map: 0 accepted, else refused
static int plain(int n_groups, const std::vector<int32_t>& ids, const std::vector<uint8_t>& groups, int64_t palette_words, std::map<int32_t, int>* out) {
    if (n_groups < 0 || n_groups > CHUNKY_LIGHT_MAX_EMITTER_GROUPS) return 1;
    if (n_groups == 0 && !ids.empty()) return 1;
    out->clear();
    for (size_t k = 0; k < ids.size(); k++) {
        const int64_t id = ids[k];
        if (groups[k] >= n_groups) return 1;
        const bool entity = id == WORLD || id == ACTOR;
        if (!entity && (id < 0 || id % 2 != 0 || id + 1 >= palette_words)) return 1;
        if (out->count((int32_t)id)) return 1;
        (*out)[(int32_t)id] = groups[k];
    }
    return 0;
}

int main() {
    // ---- every refusal of the header, each alone
    refuses(-1, {}, {}, 64);                                  // groups below 0
    refuses(CHUNKY_LIGHT_MAX_EMITTER_GROUPS + 1, {}, {}, 64); // more than the maximum
    refuses(0, {8}, {0}, 64);                                 // ids and no group
    refuses(2, {9}, {1}, 64);                                 // an odd pointer
    refuses(2, {64}, {1}, 64);                                // a pointer beyond the palette
    refuses(2, {62}, {1}, 63);                                // ... whose second word is beyond it
    refuses(2, {-1}, {1}, 64);                                // the sky's id
    refuses(2, {-4}, {1}, 64);                                // a negative id that is no entity
    refuses(2, {INT32_MIN}, {1}, 64);
    refuses(2, {INT32_MAX}, {1}, 64);
    refuses(2, {INT32_MAX - 1}, {1}, 64);                     // even, and id + 1 must not overflow on the way to the answer
    {
        LightGroupTable t;
        EXPECT(build(2, {6}, {1}, 8, &t) == CHUNKY_OK);       // the last block of a palette of four
        EXPECT(t.of_block.size() == 4 && t.of_block[3] == 1);
    }
    refuses(3, {8, 10, 8}, {1, 2, 1}, 64);                    // a block pointer twice
    refuses(3, {WORLD, 8, WORLD}, {1, 2, 2}, 64);             // an entity id twice
    refuses(3, {ACTOR, ACTOR}, {0, 0}, 64);
    refuses(3, {8}, {3}, 64);                                 // a group out of range
    refuses(1, {WORLD}, {1}, 64);
    refuses(8, {8}, {255}, 64);
    {   // NULL arrays with ids announced, a negative count, a NULL table
        LightGroupTable t = marked();
        const int32_t id = 8;
        const uint8_t g = 0;
        EXPECT(light_group_table("fuzz", 2, nullptr, &g, 1, 64, &t) == CHUNKY_E_INVALID && is_marked(t));
        EXPECT(light_group_table("fuzz", 2, &id, nullptr, 1, 64, &t) == CHUNKY_E_INVALID && is_marked(t));
        EXPECT(light_group_table("fuzz", 2, nullptr, nullptr, 1, 64, &t) == CHUNKY_E_INVALID && is_marked(t));
        EXPECT(light_group_table("fuzz", 2, &id, &g, -1, 64, &t) == CHUNKY_E_INVALID && is_marked(t));
        EXPECT(light_group_table("fuzz", 2, &id, &g, 1, 64, nullptr) == CHUNKY_E_INVALID);
        refused += 5, refusal_kinds += 5;
    }
    // ---- accepted: no ids at all, groups without ids, palettes too short to hold a block, a negative palette size
    for (int64_t words : {(int64_t)-5, (int64_t)0, (int64_t)1, (int64_t)2, (int64_t)3}) {
        LightGroupTable t = marked();
        EXPECT(build(0, {}, {}, words, &t) == CHUNKY_OK);
        EXPECT(t.n_groups == 0 && t.of_block.size() == (size_t)(words > 0 ? words / 2 : 0) && t.world == 0 && t.actor == 0);
        EXPECT(build(8, {WORLD, ACTOR}, {7, 6}, words, &t) == CHUNKY_OK);
        EXPECT(t.n_groups == 8 && t.world == 7 && t.actor == 6);
        EXPECT(light_group_of(t, WORLD) == 7 && light_group_of(t, ACTOR) == 6 && light_group_of(t, 0) == 0 && light_group_of(t, -1) == 0);
        if (words < 2) refuses(1, {0}, {0}, words);
        accepted += 2;
    }
    // ---- random sets against the map
    for (int round = 0; round < 4000; round++) {
        const int64_t words = rnd() % 5 == 0 ? (int64_t)(rnd() % 4) : (int64_t)(rnd() % 200);
        const int n_groups = (int)(rnd() % 10) - (rnd() % 16 == 0 ? 1 : 0);
        const int n = (int)(rnd() % 12);
        std::vector<int32_t> ids;
        std::vector<uint8_t> groups;
        for (int k = 0; k < n; k++) {
            const uint32_t kind = rnd() % 16;
            int32_t id = (int32_t)(2 * (rnd() % (uint32_t)(words / 2 + 1)));  // mostly even and near the palette
            if (kind == 0) id = WORLD;
            if (kind == 1) id = ACTOR;
            if (kind == 2) id += 1;
            if (kind == 3) id = -(int32_t)(rnd() % 6);
            if (kind == 4) id = rnd() % 2 ? INT32_MIN : INT32_MAX;
            if (kind == 5) id = (int32_t)words;
            ids.push_back(id);
            groups.push_back((uint8_t)(rnd() % 32 == 0 ? rnd() % 256 : rnd() % (uint32_t)(n_groups > 0 ? n_groups : 1)));
        }
        std::map<int32_t, int> want;
        const int bad = plain(n_groups, ids, groups, words, &want);
        LightGroupTable t = marked();
        const int rc = build(n_groups, ids, groups, words, &t);
        EXPECT((rc == CHUNKY_OK) == (bad == 0));
        EXPECT(rc == CHUNKY_OK || rc == CHUNKY_E_INVALID);
        if (rc != CHUNKY_OK) {
            EXPECT(is_marked(t));
            refused++;
            continue;
        }
        accepted++;
        EXPECT(t.n_groups == n_groups && t.of_block.size() == (size_t)(words / 2));
        for (int32_t id = -6; id < (int32_t)words + 6; id++) {
            if (id > 0 && id % 2 != 0) continue;  // (no hit has an odd block pointer)
            const int g = light_group_of(t, id);
            EXPECT(g == (want.count(id) ? want[id] : 0));
            EXPECT(g >= 0 && g < (n_groups > 0 ? n_groups : 1));
            lookups++;
        }
        // ids the kernel may meet after the palette grew or shrank: far beyond the table, never out of it
        for (int32_t id : {INT32_MAX, INT32_MAX - 1, INT32_MIN, (int32_t)(2 * t.of_block.size()), (int32_t)(2 * t.of_block.size() + 2)}) {
            EXPECT(light_group_of(t, id) == 0);
            lookups++;
        }
    }
    printf("{\"failures\": %lld, \"accepted\": %lld, \"refused\": %lld, \"refusal_kinds\": %lld, \"lookups\": %lld}\n", failures, accepted, refused,
           refusal_kinds, lookups);
    return failures ? 1 : 0;
}
