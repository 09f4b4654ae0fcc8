// pqgpu_take.h — pqg_take (include/pqgpu.h, "row selection"): the per-column record the kernels read,
// shared by the host half (pqgpu_take_host.cpp: validation; plain C++) and the device half
// (pqgpu_take.hip).
#pragma once
#include <stdint.h>

#include "../../include/pqgpu.h"

namespace pqg {

enum TakeKind : int32_t {
  TAKE_MISSING = 0,  // every row null: nothing is read or written
  TAKE_W1 = 1,       // 1-byte elements (BOOLEAN)
  TAKE_W4 = 2,       // INT32, FLOAT, dictionary ids
  TAKE_W8 = 3,       // INT64, DOUBLE
  TAKE_GENERIC = 4,  // INT96, FIXED_LEN_BYTE_ARRAY: `width` bytes per element
  TAKE_BINARY = 5    // BYTE_ARRAY: int64 offsets + bytes
};

// One column of a pqg_take call as the kernels see it (the table is uploaded once per call).
struct TakeColDev {
  const void* values;
  const uint8_t* binary;
  const uint8_t* dl;  // null: a required column (or a missing one)
  void* out_values;
  uint8_t* out_binary;
  uint8_t* out_dl;    // null: no level bytes are written
  uint64_t n_values, cap_values, cap_bytes;
  int32_t kind;       // TakeKind
  int32_t max_def;
  uint32_t width;     // bytes per element (TAKE_BINARY: 8, the offsets)
  uint32_t pad;
};
static_assert(sizeof(TakeColDev) == 88, "TakeColDev layout");

// The host-side refusals of pqg_take; on PQG_OK tab[0, n_cols) is filled in.
int take_validate(bool have_ctx, const uint64_t* d_bitmap, uint64_t n_rows, const pqg_take_column* cols, int n_cols,
                  uint64_t out_rows_capacity, const pqg_take_counts* d_counts, const pqg_take_result* d_result,
                  TakeColDev* tab);

}  // namespace pqg
