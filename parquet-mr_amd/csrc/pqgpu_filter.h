// pqgpu_filter.h — the compiled form of a filter2 predicate, shared by its host half
// (pqgpu_filter_host.cpp: validation, LogicalInverseRewriter, comparator keys; plain C++) and its
// device half (pqgpu_filter.hip: the five launches of pqg_filter_run, and those of contains()).
#pragma once
#include <stdint.h>

#include <vector>

#include "../../include/pqgpu.h"

namespace pqg {

// One node of the device program (16 bytes). Leaves name a slot: the s-th distinct column the
// program reads. Literal cells hold comparator keys (int64, compared signed) for the fixed-width
// types and offset | length << 32 into the literal bytes for BYTE_ARRAY.
struct FilterDevNode {
  uint8_t op;     // pqg_filter_op, never NOT
  uint8_t flags;  // PQG_FILTER_*
  uint8_t slot;   // leaves
  uint8_t type;   // leaves: pqg_physical_type of the column
  uint8_t left;   // AND / OR
  uint8_t right;
  uint16_t n_lit;
  uint32_t lit_begin;
  uint32_t pad;
};

// Header of the device image: FilterDevHeader, nodes[n_nodes], order[PQG_FILTER_MAX_NODES] (u8: the
// leaves grouped by slot, then nothing), cells[n_cells] (8 bytes each), bytes[n_bytes] padded to 8 + 8.
struct FilterDevHeader {
  uint32_t n_nodes, n_leaves, n_slots, n_cells, n_bytes, cells_off, bytes_off, image_bytes;
};

constexpr uint32_t FILTER_IN_LINEAR = 8;  // sets up to this size are probed linearly, larger ones by binary search

// The columns the program reads (its slots), passed to the kernels by value; null_slot lists the
// slots that have definition levels (the columns k_filter_rank counts).
struct FilterColDev {
  const void* values;    // dense values, or the uint32 ids of a column that has a dictionary (FilterDictSlot)
  const uint8_t* binary;
  const uint8_t* dl;     // null: required (max_def == 0) or missing (max_def > 0)
  uint64_t n_values;
  int32_t type;
  int32_t max_def;
  int32_t column;        // the caller's column index (error_column)
  int32_t null_idx;      // position in null_slot, -1 without definition levels
};
struct FilterCols {
  uint32_t n_slots, n_nullable;
  uint8_t null_slot[PQG_FILTER_MAX_NODES];
  FilterColDev c[PQG_FILTER_MAX_NODES];
};

// pqg_filter_run_dict: what the kernels need beyond FilterCols, read from a small device table (FilterCols
// with these fields in it would pass the 4 KiB of kernel arguments).
struct FilterDictSlot {
  const void* values;     // the slot's dictionary in the decoder's layout; its ids are FilterColDev::values
  const uint8_t* binary;
  uint32_t n_entries;
  uint32_t is_dict;       // 0: the slot holds values
};
constexpr uint64_t FILTER_NO_TABLE = ~0ull;
struct FilterDictTab {
  uint32_t n_tables;      // leaves with a verdict table of at least one word (k_filter_dict's grid.y)
  uint32_t in_lds;        // the tables are staged in LDS behind the image (table_words * 8 <= PQG_FILTER_DICT_LDS_BYTES)
  uint64_t table_words;   // u64 words of all tables: ceil(n_entries / 64) per table
  uint64_t max_words;     // the largest table (k_filter_dict's grid.x covers it)
  uint64_t leaf_off[PQG_FILTER_MAX_NODES];   // node -> first word of its table, FILTER_NO_TABLE without one
  uint8_t table_leaf[PQG_FILTER_MAX_NODES];  // t-th table -> node
  FilterDictSlot slot[PQG_FILTER_MAX_NODES];
};
// image + staged tables stay inside the 64 KiB a workgroup may allocate
static_assert(sizeof(FilterDevHeader) + PQG_FILTER_MAX_NODES * (sizeof(FilterDevNode) + 1) + 8 * PQG_FILTER_MAX_LITERALS +
                      PQG_FILTER_MAX_LITERAL_BYTES + 16 + PQG_FILTER_DICT_LDS_BYTES <= 65536,
              "filter image + dictionary tables exceed a workgroup's LDS");

// ---- pqg_filter_run_records -----------------------------------------------------------------------
// Device-node flag (never in pqg_filter_node.flags): the leaf is the child of a CONTAINS node. The
// evaluation kernel skips it; k_filter_contains evaluates it per slot.
constexpr uint8_t FILTER_DEV_CONTAINED = 0x80;
// FilterColDev::null_idx of a repeated slot (its levels are per slot, not per row: never ranked over rows)
constexpr int32_t FILTER_NULL_IDX_REPEATED = -2;
constexpr uint8_t FILTER_NO_LEAF = 0xFF;
constexpr uint32_t FILTER_CONTAINS_GROUP = 4;  // contains leaves of one column a wave evaluates on one load of the value

// The record facts of a run, read by the kernels from a small device table beside FilterDictTab.
// Repeated columns the predicate names are numbered 0 .. n_rep - 1 (rep_slot), contains leaves
// 0 .. n_leaves - 1 in program order (leaf_node: the CONTAINS node's child). A missing column has no
// entry in rep_slot: the record bitmaps of its contains leaves stay zero. The contains leaves of a repeated
// column are dealt to groups of up to FILTER_CONTAINS_GROUP (k_filter_contains: one wave per group and tile).
struct FilterRecTab {
  uint32_t n_rep;         // repeated, present slots with a contains leaf
  uint32_t n_leaves;      // contains leaves (record bitmaps)
  uint32_t n_groups;      // groups of contains leaves (k_filter_contains' grid.y)
  uint32_t pad;
  uint64_t bitmap_words;  // u64 words of one record bitmap: filter_tiles(n_rows) * 64
  uint64_t max_slots;     // the largest n_slots of rep_slot's columns
  uint8_t rep_slot[PQG_FILTER_MAX_NODES];     // repeated column -> program slot
  uint8_t leaf_node[PQG_FILTER_MAX_NODES];    // contains leaf -> its leaf node
  uint8_t leaf_rep[PQG_FILTER_MAX_NODES];     // contains leaf -> repeated column, FILTER_NO_LEAF: missing column
  uint8_t node_leaf[PQG_FILTER_MAX_NODES];    // CONTAINS node -> contains leaf, FILTER_NO_LEAF otherwise
  uint8_t group_rep[PQG_FILTER_MAX_NODES];    // group -> repeated column
  uint8_t group_n[PQG_FILTER_MAX_NODES];      // group -> its leaves, 1 .. FILTER_CONTAINS_GROUP
  uint8_t group_leaf[PQG_FILTER_MAX_NODES][FILTER_CONTAINS_GROUP];  // group -> contains leaves (unused: 0)
  const uint8_t* rl[PQG_FILTER_MAX_NODES];    // per repeated column: repetition bytes
  uint64_t n_slots[PQG_FILTER_MAX_NODES];     // per repeated column
  uint64_t* bitmaps;      // device: the record bitmaps, bitmap_words each (set at launch, inside the scratch)
};
// What goes to the device for a run with contains leaves (k_filter_contains, k_filter_eval_records).
struct FilterRecDev {
  FilterDictTab dt;
  FilterRecTab rt;
};

// Binds the caller's columns (and dictionaries, or null) to the program's slots: every refusal
// pqg_filter_run / pqg_filter_run_dict make before a launch, the FilterCols the kernels take and, with
// dictionaries, the FilterDictTab (`dt` may be null without them). No device calls.
int filter_bind(const pqg_filter* filter, const pqg_filter_column* cols, const pqg_filter_dictionary* dicts, int n_cols,
                uint64_t n_rows, FilterCols* fc, FilterDictTab* dt, bool* any_dict);

// The same for pqg_filter_run_records: every refusal it makes before a launch, the FilterCols (a repeated
// slot has null_idx == FILTER_NULL_IDX_REPEATED and is not in null_slot), the FilterDictTab (`dt` is
// required: it is filled whether or not a dictionary is given) and the FilterRecTab. No device calls.
int filter_bind_records(const pqg_filter* filter, const pqg_filter_record_column* cols, const pqg_filter_dictionary* dicts,
                        int n_cols, uint64_t n_rows, FilterCols* fc, FilterDictTab* dt, bool* any_dict, FilterRecTab* rt);

}  // namespace pqg

struct pqg_filter {
  uint64_t serial = 0;                  // unique per created filter (the ctx caches the uploaded image by it)
  std::vector<pqg_filter_node> program; // rewritten, NOT-free, post-order; literal_begin into `cells`
  std::vector<int32_t> column_types;
  std::vector<uint64_t> cells;          // raw literal cells, one private range per leaf (sets > 8 sorted)
  std::vector<uint8_t> bytes;           // BYTE_ARRAY literal bytes
  std::vector<int32_t> slot_column;     // slot -> column index
  std::vector<uint8_t> image;           // device image (FilterDevHeader ...)
  bool has_contains = false;            // a CONTAINS node: pqg_filter_run_records only
};

namespace pqg {
// Comparator key of a raw literal / value cell of a fixed-width type: signed int64 order of the keys
// is the PrimitiveComparator's order of the values.
#ifdef __HIPCC__
#define PQG_FILTER_HD __host__ __device__
#else
#define PQG_FILTER_HD
#endif
PQG_FILTER_HD inline int64_t filter_key(int type, bool is_unsigned, uint64_t raw) {
  switch (type) {
    case PQG_BOOLEAN: return (raw & 0xFFu) != 0;
    case PQG_INT32: return is_unsigned ? (int64_t)(uint32_t)raw : (int64_t)(int32_t)(uint32_t)raw;
    case PQG_INT64: return (int64_t)(is_unsigned ? raw ^ 0x8000000000000000ull : raw);
    case PQG_FLOAT: {
      uint32_t b = (uint32_t)raw;
      if ((b & 0x7FFFFFFFu) > 0x7F800000u) b = 0x7FC00000u;  // Float.floatToIntBits: one NaN
      const uint32_t k = b ^ ((b >> 31) ? 0x7FFFFFFFu : 0u);
      return (int64_t)(int32_t)k;
    }
    case PQG_DOUBLE: {
      uint64_t b = raw;
      if ((b & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull) b = 0x7FF8000000000000ull;
      return (int64_t)(b ^ ((b >> 63) ? 0x7FFFFFFFFFFFFFFFull : 0ull));
    }
    default: return 0;
  }
}
}  // namespace pqg
