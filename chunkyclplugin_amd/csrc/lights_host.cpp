// lights_host.cpp — the device-free half of the emitter light groups (lights_host.hpp).  Plain C++: compiled by g++ alone in
// tests/sanitize/light_groups_fuzz.cpp's build.
#include "lights_host.hpp"

#include "capi_error.hpp"

int light_group_table(const char* who, int n_groups, const int32_t* ids, const uint8_t* group_of, int n_ids, int64_t palette_words,
                      LightGroupTable* table) {
    if (!table) return fail(CHUNKY_E_INVALID, "%s: NULL table", who);
    if (n_groups < 0 || n_groups > CHUNKY_LIGHT_MAX_EMITTER_GROUPS)
        return fail(CHUNKY_E_INVALID, "%s: %d groups (0 .. %d)", who, n_groups, CHUNKY_LIGHT_MAX_EMITTER_GROUPS);
    if (n_ids < 0 || (n_ids > 0 && (!ids || !group_of))) return fail(CHUNKY_E_INVALID, "%s: %d ids need both arrays", who, n_ids);
    if (n_groups == 0 && n_ids > 0) return fail(CHUNKY_E_INVALID, "%s: %d ids and no group to put them in", who, n_ids);
    if (palette_words < 0) palette_words = 0;
    LightGroupTable t;
    t.n_groups = n_groups;
    t.of_block.assign((size_t)(palette_words / 2), 0);
    std::vector<bool> seen(t.of_block.size(), false);
    bool seen_world = false, seen_actor = false;
    for (int i = 0; i < n_ids; i++) {
        const int32_t id = ids[i];
        if (group_of[i] >= n_groups) return fail(CHUNKY_E_INVALID, "%s: id %d in group %d of %d", who, (int)id, (int)group_of[i], n_groups);
        if (id == CHUNKY_MATTE_WORLD_ENTITY || id == CHUNKY_MATTE_ACTOR_ENTITY) {
            bool& seen_it = id == CHUNKY_MATTE_WORLD_ENTITY ? seen_world : seen_actor;
            if (seen_it) return fail(CHUNKY_E_INVALID, "%s: entity id %d listed twice", who, (int)id);
            seen_it = true;
            (id == CHUNKY_MATTE_WORLD_ENTITY ? t.world : t.actor) = group_of[i];
            continue;
        }
        if (id < 0 || (id & 1) || (int64_t)id + 1 >= palette_words)  // a block takes the words id and id + 1
            return fail(CHUNKY_E_INVALID, "%s: id %d is neither an entity id nor an even pointer into a block palette of %lld words", who, (int)id,
                        (long long)palette_words);
        const size_t k = (size_t)(id >> 1);
        if (seen[k]) return fail(CHUNKY_E_INVALID, "%s: block pointer %d listed twice", who, (int)id);
        seen[k] = true;
        t.of_block[k] = group_of[i];
    }
    *table = std::move(t);
    return CHUNKY_OK;
}

int light_group_of(const LightGroupTable& table, int32_t id) {
    if (id == CHUNKY_MATTE_WORLD_ENTITY) return table.world;
    if (id == CHUNKY_MATTE_ACTOR_ENTITY) return table.actor;
    if (id < 0) return 0;
    const size_t k = (size_t)(id >> 1);
    return k < table.of_block.size() ? table.of_block[k] : 0;
}
