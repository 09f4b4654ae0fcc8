// pqgpu_take.h — pqg_take and pqg_take_records (include/pqgpu.h, "row selection", "record selection on
// repeated columns"): the per-column records the kernels read,
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

// One internal column of a pqg_take_records call ("record selection on repeated columns"): the column
// as the shared gather sees it, plus the bitmap its rows are kept by. A flat column keeps rows of the
// caller's record bitmap; a repeated column keeps slots of its own slot bitmap, which k_rec_expand
// writes into the scratch; its repetition bytes travel as a second record (a required 1-byte column on
// the same slot bitmap) behind the n_cols records of the caller's columns.
struct TakeRecDev {
  TakeColDev c;
  const uint64_t* bitmap;  // flat: the caller's; otherwise set by the launcher from slot_off
  uint64_t n;              // rows the bitmap covers: n_rows (flat) or n_slots
  const uint8_t* rl;       // repetition bytes of a repeated column's own record, null otherwise
  uint64_t cap_levels;     // level bytes the column may write: out_rows_capacity (flat), out_slots_capacity
  uint64_t slot_off;       // u64 words from the start of the slot bitmaps (own_bitmap only)
  uint32_t keep_col;       // the caller's column whose per-tile kept rows are this record's output rows
  uint32_t own_bitmap;     // 1: the slot bitmap at slot_off
};
static_assert(sizeof(TakeRecDev) == 136, "TakeRecDev layout");

constexpr int TAKE_REC_MAX_RECORDS = 2 * PQG_TAKE_MAX_COLUMNS;

// What take_records_validate learned about the call besides the table.
struct TakeRecPlan {
  uint32_t n_records;   // entries of tab: n_cols, then one per repeated column that is not missing
  uint64_t max_rows;    // largest `n` of any record and of n_rows: the grid covers its tiles
  uint64_t slot_words;  // u64 words of all slot bitmaps (whole tiles per column)
  bool any_repeated, any_nullable, any_binary;
};

// The host-side refusals of pqg_take_records; on PQG_OK tab[0, plan->n_records) is filled in
// (tab holds TAKE_REC_MAX_RECORDS entries).
int take_records_validate(bool have_ctx, const uint64_t* d_bitmap, uint64_t n_rows, const pqg_take_record_column* cols,
                          int n_cols, uint64_t out_rows_capacity, const pqg_take_record_counts* d_counts,
                          const pqg_take_result* d_result, TakeRecDev* tab, TakeRecPlan* plan);

}  // namespace pqg
