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
// types and offset | length << 32 into the literal bytes for BYTE_ARRAY. The binary types (BYTE_ARRAY,
// FIXED_LEN_BYTE_ARRAY, INT96) carry their comparator in the flags: none = unsigned bytes;
// FILTER_DEV_FLOAT16: cells hold keys as for the fixed-width types; FILTER_DEV_SIGNED: big-endian two's
// complement, and with FILTER_DEV_KEY128 every literal takes three cells: its BYTE_ARRAY cell, then the
// high (signed) and low (unsigned) half of its sign-extended 128-bit value.
struct FilterDevNode {
  uint8_t op;     // pqg_filter_op, never NOT
  uint8_t flags;  // PQG_FILTER_*
  uint8_t slot;   // leaves
  uint8_t type;   // leaves: pqg_physical_type of the column
  uint8_t left;   // AND / OR
  uint8_t right;
  uint16_t n_lit;
  uint32_t lit_begin;
  uint32_t width;  // leaves on INT96 / FIXED_LEN_BYTE_ARRAY: bytes per element; otherwise 0
};
constexpr uint8_t FILTER_DEV_SIGNED = 0x04;   // PQG_FILTER_ORDER_SIGNED_INTEGER
constexpr uint8_t FILTER_DEV_FLOAT16 = 0x08;  // PQG_FILTER_ORDER_FLOAT16
constexpr uint8_t FILTER_DEV_KEY128 = 0x10;   // with FILTER_DEV_SIGNED: literals carry 128-bit keys
constexpr uint32_t FILTER_KEY128_BYTES = 16;  // the widest value the 128-bit keys compare
// pqg_filter::rg_image only (the row-group form of the program): a notIn whose set is exactly {null}
constexpr uint8_t FILTER_DEV_NULL_ONLY = 0x20;

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
  std::vector<pqg_filter_column_type> columns;  // as declared (pqg_filter_create: width and order 0)
  bool binary_paths = false;            // a leaf on INT96 / FLBA or with an order of its own: the kernels' BIN form
  std::vector<uint64_t> cells;          // raw literal cells, one private range per leaf (sets > 8 sorted)
  std::vector<uint8_t> bytes;           // BYTE_ARRAY literal bytes
  std::vector<int32_t> slot_column;     // slot -> column index
  std::vector<uint8_t> image;           // device image (FilterDevHeader ...)
  // pqg_filter_row_groups: the image with the equality leaves (eq, notEq, in, notIn) of binary columns keyed by
  // their unsigned bytes, whatever the column's order (HashSet.contains is equals(), not the comparator), their
  // sets of more than 8 members sorted that way, and FILTER_DEV_NULL_ONLY
  std::vector<uint8_t> rg_image;
  std::vector<uint8_t> null_only;       // per program node: in / notIn whose set is exactly {null}
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

// Float16.compare (schema/Float16.java:108-134) as a key: every NaN is 0x7e00, above +Infinity (0x7c00);
// a negative value of magnitude m is -m - 1, so -0.0 (-1) stands below +0.0 (0).
PQG_FILTER_HD inline int64_t filter_key_float16(uint32_t bits) {
  const uint32_t m = bits & 0x7FFFu;
  if (m > 0x7C00u) return 0x7E00;
  return (bits & 0x8000u) ? -(int64_t)m - 1 : (int64_t)m;
}

// The value of n big-endian two's-complement bytes as a sign-extended 128-bit integer (hi signed, lo
// unsigned); an empty value is 0. Leading bytes that only repeat the sign are dropped first, which changes
// no comparison of BINARY_AS_SIGNED_INTEGER_COMPARATOR (it pads the shorter side with exactly those bytes).
// false: more than 16 bytes remain.
inline bool filter_key128(const uint8_t* p, uint32_t n, int64_t* hi, uint64_t* lo) {
  const bool neg = n > 0 && (p[0] & 0x80u);
  const uint8_t pad = neg ? 0xFFu : 0u;
  while (n > 1 && p[0] == pad && ((p[1] & 0x80u) != 0) == neg) p++, n--;
  if (n > FILTER_KEY128_BYTES) return false;
  uint64_t h = neg ? ~0ull : 0ull, l = h;
  for (uint32_t i = 0; i < n; i++) {
    h = (h << 8) | (l >> 56);
    l = (l << 8) | p[i];
  }
  *hi = (int64_t)h;
  *lo = l;
  return true;
}
}  // namespace pqg
