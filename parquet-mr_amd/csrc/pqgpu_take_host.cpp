// pqgpu_take_host.cpp — host half of pqg_take and pqg_take_records (include/pqgpu.h, "row selection",
// "record selection on repeated columns"): the refusals made before any launch and the per-column table
// for the kernels. Plain C++ with no HIP in it, so that it also builds alone under the sanitizers
// (tests/c/take_sanitize.cpp, tests/c/take_records_sanitize.cpp). No pointer is dereferenced except
// `cols`.
#include "pqgpu_take.h"

namespace pqg {

static bool aligned(const void* p, uint32_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

int take_validate(bool have_ctx, const uint64_t* d_bitmap, uint64_t n_rows, const pqg_take_column* cols, int n_cols,
                  uint64_t out_rows_capacity, const pqg_take_counts* d_counts, const pqg_take_result* d_result,
                  TakeColDev* tab) {
  if (!have_ctx || !d_result || !d_counts || n_cols < 0 || (n_cols > 0 && !cols)) return PQG_ERR_INVALID_ARG;
  if (n_rows && !d_bitmap) return PQG_ERR_INVALID_ARG;
  if (!aligned(d_bitmap, 8) || !aligned(d_counts, 8) || !aligned(d_result, 8)) return PQG_ERR_INVALID_ARG;
  if (n_cols > PQG_TAKE_MAX_COLUMNS) return PQG_ERR_UNSUPPORTED;
  for (int i = 0; i < n_cols; i++) {
    const pqg_take_column& c = cols[i];
    TakeColDev d{};
    if (c.physical_type < PQG_BOOLEAN || c.physical_type > PQG_FIXED_LEN_BYTE_ARRAY) return PQG_ERR_INVALID_ARG;
    if (c.max_def < 0 || c.max_def > 254 || (c.flags & ~PQG_COLUMN_DICTIONARY_IDS)) return PQG_ERR_INVALID_ARG;
    if (c.physical_type == PQG_FIXED_LEN_BYTE_ARRAY && c.type_length <= 0) return PQG_ERR_INVALID_ARG;
    d.max_def = c.max_def;
    if (c.max_def > 0 && !c.def_levels) {  // a column the file does not have
      d.kind = TAKE_MISSING;
      tab[i] = d;
      continue;
    }
    uint32_t align = 1;
    if (c.flags & PQG_COLUMN_DICTIONARY_IDS) {
      d.kind = TAKE_W4, d.width = 4, align = 4;
    } else {
      switch (c.physical_type) {
        case PQG_BOOLEAN: d.kind = TAKE_W1, d.width = 1; break;
        case PQG_INT32: case PQG_FLOAT: d.kind = TAKE_W4, d.width = 4, align = 4; break;
        case PQG_INT64: case PQG_DOUBLE: d.kind = TAKE_W8, d.width = 8, align = 8; break;
        case PQG_INT96: d.kind = TAKE_GENERIC, d.width = 12, align = 4; break;
        case PQG_BYTE_ARRAY: d.kind = TAKE_BINARY, d.width = 8, align = 8; break;
        default: d.kind = TAKE_GENERIC, d.width = (uint32_t)c.type_length; break;
      }
    }
    const bool binary = d.kind == TAKE_BINARY;
    // the pointer rules of pqg_filter_run, on the inputs and on the outputs the column needs
    if (!c.values && (c.n_values || binary)) return PQG_ERR_INVALID_ARG;
    if (binary && (!c.binary_data || !c.out_binary_data)) return PQG_ERR_INVALID_ARG;
    if (c.max_def == 0 && c.n_values < n_rows) return PQG_ERR_INVALID_ARG;  // a required column has a value per row
    if (!c.out_values && (c.out_values_capacity || binary)) return PQG_ERR_INVALID_ARG;
    if (c.max_def > 0 && !c.out_def_levels && out_rows_capacity) return PQG_ERR_INVALID_ARG;
    if (!aligned(c.values, align) || !aligned(c.out_values, align)) return PQG_ERR_INVALID_ARG;
    // capacities whose byte size does not fit 64 bits cannot be real
    if (c.out_values_capacity > (UINT64_MAX >> 1) / (d.width ? d.width : 1)) return PQG_ERR_INVALID_ARG;
    d.values = c.values;
    d.binary = binary ? c.binary_data : nullptr;
    d.dl = c.max_def > 0 ? c.def_levels : nullptr;
    d.out_values = c.out_values;
    d.out_binary = binary ? c.out_binary_data : nullptr;
    d.out_dl = c.max_def > 0 ? c.out_def_levels : nullptr;
    d.n_values = c.n_values;
    d.cap_values = c.out_values_capacity;
    d.cap_bytes = binary ? c.out_binary_capacity : 0;
    tab[i] = d;
  }
  return PQG_OK;
}

int take_records_validate(bool have_ctx, const uint64_t* d_bitmap, uint64_t n_rows, const pqg_take_record_column* cols,
                          int n_cols, uint64_t out_rows_capacity, const pqg_take_record_counts* d_counts,
                          const pqg_take_result* d_result, TakeRecDev* tab, TakeRecPlan* plan) {
  if (!have_ctx || !d_result || !d_counts || !plan || n_cols < 0 || (n_cols > 0 && !cols)) return PQG_ERR_INVALID_ARG;
  if (n_rows && !d_bitmap) return PQG_ERR_INVALID_ARG;
  if (!aligned(d_bitmap, 8) || !aligned(d_counts, 8) || !aligned(d_result, 8)) return PQG_ERR_INVALID_ARG;
  if (n_cols > PQG_TAKE_MAX_COLUMNS) return PQG_ERR_UNSUPPORTED;
  TakeRecPlan p{};
  p.n_records = (uint32_t)n_cols;
  p.max_rows = n_rows;
  constexpr uint64_t tile = PQG_FILTER_TILE_ROWS;
  for (int i = 0; i < n_cols; i++) {
    const pqg_take_record_column& rc = cols[i];
    const bool missing = rc.col.max_def > 0 && !rc.col.def_levels;
    if (rc.max_rep < 0 || rc.max_rep > 254 || rc.reserved != 0) return PQG_ERR_INVALID_ARG;
    // take_validate on `col`; the level bytes of a repeated column are bounded by its own capacity
    const uint64_t n = rc.max_rep > 0 ? rc.n_slots : n_rows;
    const uint64_t level_cap = rc.max_rep > 0 ? rc.out_slots_capacity : out_rows_capacity;
    TakeRecDev d{};
    const int e = take_validate(true, d_bitmap, n_rows, &rc.col, 1, level_cap, (const pqg_take_counts*)d_counts, d_result,
                                &d.c);
    if (e != PQG_OK) return e;
    if (rc.max_rep > 0) {
      if (rc.col.max_def == 0) return PQG_ERR_INVALID_ARG;  // a repeated node always adds a definition level
      if (!missing) {
        if (!rc.rep_levels) return PQG_ERR_INVALID_ARG;
        if (rc.out_slots_capacity && (!rc.out_rep_levels || !rc.col.out_def_levels)) return PQG_ERR_INVALID_ARG;
        if (rc.n_slots > UINT64_MAX - tile) return PQG_ERR_INVALID_ARG;  // its tiles cannot be counted
      }
    } else {
      if (rc.rep_levels || rc.n_slots != n_rows) return PQG_ERR_INVALID_ARG;
    }
    if (!missing && rc.n_slots < n_rows) return PQG_ERR_INVALID_ARG;  // a record has at least one slot
    d.keep_col = (uint32_t)i;
    d.cap_levels = level_cap;
    d.n = missing ? 0 : n;
    d.bitmap = d_bitmap;
    if (!missing) {
      p.any_nullable |= d.c.dl != nullptr;
      p.any_binary |= d.c.kind == TAKE_BINARY;
      if (d.n > p.max_rows) p.max_rows = d.n;
    }
    if (rc.max_rep > 0 && !missing) {
      d.rl = rc.rep_levels;
      d.bitmap = nullptr;
      d.own_bitmap = 1;
      d.slot_off = p.slot_words;
      p.slot_words += (rc.n_slots + tile - 1) / tile * (tile / 64);
      p.any_repeated = true;
      // the repetition bytes: a required 1-byte column over the same slots
      TakeRecDev r{};
      r.c.kind = TAKE_W1;
      r.c.width = 1;
      r.c.values = rc.rep_levels;
      r.c.n_values = rc.n_slots;
      r.c.out_values = rc.out_rep_levels;
      r.c.cap_values = rc.out_rep_levels ? rc.out_slots_capacity : 0;
      r.n = rc.n_slots;
      r.cap_levels = 0;
      r.own_bitmap = 1;
      r.slot_off = d.slot_off;
      r.keep_col = (uint32_t)i;
      tab[p.n_records++] = r;
    }
    tab[i] = d;
  }
  *plan = p;
  return PQG_OK;
}

}  // namespace pqg
