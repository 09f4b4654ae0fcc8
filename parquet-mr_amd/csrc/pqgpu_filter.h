// pqgpu_filter.h — the compiled form of a filter2 predicate, shared by its host half
// (pqgpu_filter_host.cpp: validation, LogicalInverseRewriter, comparator keys; plain C++) and its
// device half (pqgpu_filter.hip: the five launches of pqg_filter_run).
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

}  // namespace pqg

struct pqg_filter {
  uint64_t serial = 0;                  // unique per created filter (the ctx caches the uploaded image by it)
  std::vector<pqg_filter_node> program; // rewritten, NOT-free, post-order; literal_begin into `cells`
  std::vector<int32_t> column_types;
  std::vector<uint64_t> cells;          // raw literal cells, one private range per leaf (sets > 8 sorted)
  std::vector<uint8_t> bytes;           // BYTE_ARRAY literal bytes
  std::vector<int32_t> slot_column;     // slot -> column index
  std::vector<uint8_t> image;           // device image (FilterDevHeader ...)
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
