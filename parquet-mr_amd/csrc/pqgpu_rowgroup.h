// pqgpu_rowgroup.h — the row-group dictionary filter (include/pqgpu.h, "row-group dictionary filter"),
// shared by its host half (pqgpu_rowgroup_host.cpp: the binding of a call's tables, the flag rules, the
// work list, pqg_chunk_has_non_dictionary_pages; plain C++) and its device half (pqgpu_rowgroup.hip).
#pragma once
#include <stdint.h>

#include <vector>

#include "pqgpu_filter.h"

namespace pqg {

constexpr uint32_t RG_TILE = PQG_RG_TILE_ENTRIES;  // entries of one work item: RG_TILE / 64 steps of a wave
static_assert(RG_TILE % 64 == 0, "a wave steps 64 entries at a time");
// RgColDev::flags beside PQG_RG_*: the dictionary can decide (not MISSING / NO_DICTIONARY / NON_DICT_PAGES,
// and a type expandDictionary decodes)
constexpr uint32_t RG_USABLE = 0x100;

// One (row group, slot) of the device table: entry [g * n_slots + s]; a slot is the s-th distinct column the
// program reads.
struct RgColDev {
  const void* values;     // the dictionary in the decoder's layout (null unless usable with entries)
  const uint8_t* binary;
  uint32_t n_entries;
  uint32_t flags;         // PQG_RG_* | RG_USABLE
};
// One wave's work in k_rg_any: every leaf of `slot` without a null literal on entries
// [tile * RG_TILE, min(n_entries, (tile + 1) * RG_TILE)) of row group `group`.
struct RgItem {
  uint32_t group;
  uint32_t slot_tile;  // slot << 24 | tile
};
static_assert(sizeof(RgColDev) == 24 && sizeof(RgItem) == 8, "row-group device tables");
static_assert((0xFFFFFFFFull + RG_TILE - 1) / RG_TILE <= (1u << 24), "a dictionary's tiles fit RgItem::tile");

constexpr uint64_t RG_MAX_GROUPS = 0x7FFFFFFFull;  // error_group is an int32
constexpr uint64_t RG_MAX_ITEMS = 1ull << 26;      // 512 MiB of work list; k_rg_any's grid is items / 4 workgroups

struct RgPlan {
  uint32_t n_slots = 0, n_nodes = 0;
  std::vector<RgColDev> cols;  // n_row_groups * n_slots
  std::vector<RgItem> items;
};

// Every refusal pqg_filter_row_groups makes before a launch, the device table and the work list. No device calls.
int rowgroup_bind(const pqg_filter* filter, const pqg_rowgroup_column* cols, int n_cols, uint64_t n_row_groups,
                  RgPlan* plan);

// Device words (u64) of the scratch: the (row group, node) hit flags (u32 each, zeroed before k_rg_any), then
// the kept count of every bitmap word.
inline uint64_t rowgroup_hit_words(uint64_t n_row_groups, uint32_t n_nodes) { return (n_row_groups * n_nodes + 1) / 2; }
inline uint64_t rowgroup_scratch_words(uint64_t n_row_groups, uint32_t n_nodes) {
  return rowgroup_hit_words(n_row_groups, n_nodes) + (n_row_groups + 63) / 64;
}

}  // namespace pqg
