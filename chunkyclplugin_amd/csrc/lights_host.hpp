// lights_host.hpp — the device-free half of the emitter light groups (chunky_render_light_set_emitter_groups):
// the checks of the caller's ids and the table the kernel reads.  Plain C++: no HIP type.
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/chunky_hip.h"

#pragma GCC visibility push(hidden)  // internal to the library

// Which group every id belongs to.  of_block[pointer >> 1] for a block pointer (one byte per block of the palette the table was built
// against), world / actor for the two entity ids; whatever the caller did not list is group 0.
struct LightGroupTable {
    int n_groups = 0;
    std::vector<uint8_t> of_block;
    uint8_t world = 0, actor = 0;
};

// The caller's (id, group) pairs as a table over a block palette of `palette_words` int32 (two words per block).  CHUNKY_E_INVALID,
// with *table untouched, for n_groups outside 0 .. CHUNKY_LIGHT_MAX_EMITTER_GROUPS, n_ids < 0, a null array with n_ids > 0, ids with
// n_groups == 0, an id that is neither an entity id nor an even pointer inside the palette, an id listed twice, or a group >= n_groups.
int light_group_table(const char* who, int n_groups, const int32_t* ids, const uint8_t* group_of, int n_ids, int64_t palette_words,
                      LightGroupTable* table);
// The group of a hit's id as the kernel decides it: a pointer beyond the table (a palette shortened since) is group 0.
int light_group_of(const LightGroupTable& table, int32_t id);

#pragma GCC visibility pop
