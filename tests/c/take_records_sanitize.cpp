/*
 * take_records_sanitize.cpp — the host half of pqg_take_records (csrc/pqgpu_take_host.cpp,
 * take_records_validate: the refusals made before any launch, the per-record table, the plan) under
 * AddressSanitizer + UndefinedBehaviorSanitizer, without HIP. Built by
 * tests/test_take_records_sanitize.py with -fsanitize=address,undefined -fno-sanitize-recover=all, so
 * any finding aborts the run.
 *
 * usage: take_records_sanitize <mutations per base table>
 * Valid column tables (flat, repeated and missing columns of every physical type, 0 to
 * PQG_TAKE_MAX_COLUMNS columns) must be accepted and come back as the records the kernels read; every
 * refusal the header lists must be made; deterministic mutations (flipped bits in any field, column
 * counts from negative to far past the limit, random row counts and capacities) must be accepted or
 * refused with PQG_ERR_INVALID_ARG / PQG_ERR_UNSUPPORTED. The column table is an exactly-sized heap
 * allocation and the record table holds exactly the records the call may write, so an access past
 * either is caught; the "device" pointers are made-up addresses and never dereferenced.
 * Prints: cases=<n> ok=<n> invalid=<n> unsupported=<n>; exit status 1 on any other outcome.
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../parquet-mr_amd/csrc/pqgpu_take.h"

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {  // xorshift64*
  g_state ^= g_state >> 12;
  g_state ^= g_state << 25;
  g_state ^= g_state >> 27;
  return g_state * 0x2545F4914F6CDD1Dull;
}

// made-up, suitably aligned device addresses
static void* dev(uint64_t k) { return (void*)(uintptr_t)(0x7000000000ull + k * 4096); }

// max_rep > 0: a repeated leaf of n_rows + extra slots; missing: a column the file does not have
static pqg_take_record_column column(int type, int max_def, int max_rep, bool missing, uint64_t n_rows, uint64_t extra,
                                     uint64_t k) {
  pqg_take_record_column r{};
  pqg_take_column& c = r.col;
  const uint64_t n_slots = max_rep ? n_rows + extra : n_rows;
  c.physical_type = type;
  c.max_def = max_def;
  c.type_length = type == PQG_FIXED_LEN_BYTE_ARRAY ? 1 + (int)(k % 20) : 0;
  c.flags = (type == PQG_BYTE_ARRAY && k % 3 == 0) ? PQG_COLUMN_DICTIONARY_IDS : 0;
  r.max_rep = max_rep;
  r.n_slots = n_slots;
  if (missing) return r;
  c.values = dev(16 * k);
  c.binary_data = (const uint8_t*)dev(16 * k + 1);
  c.def_levels = max_def ? (const uint8_t*)dev(16 * k + 2) : nullptr;
  c.n_values = n_slots;
  c.out_values = dev(16 * k + 3);
  c.out_binary_data = (uint8_t*)dev(16 * k + 4);
  c.out_def_levels = max_def ? (uint8_t*)dev(16 * k + 5) : nullptr;
  c.out_values_capacity = n_slots;
  c.out_binary_capacity = 1000;
  if (max_rep) {
    r.rep_levels = (const uint8_t*)dev(16 * k + 6);
    r.out_rep_levels = (uint8_t*)dev(16 * k + 7);
    r.out_slots_capacity = n_slots;
  }
  return r;
}

struct Tally {
  long cases = 0, ok = 0, invalid = 0, unsupported = 0, other = 0;
};

static int run(Tally& t, bool ctx, const uint64_t* bitmap, uint64_t n_rows, const std::vector<pqg_take_record_column>& cols,
               int n_cols, uint64_t rows_cap, const pqg_take_record_counts* counts, const pqg_take_result* result) {
  // exactly-sized heap copies: the columns in; out, the records n_cols columns can need at the most
  pqg_take_record_column* in =
      cols.empty() ? nullptr : (pqg_take_record_column*)malloc(sizeof(pqg_take_record_column) * cols.size());
  if (in) memcpy(in, cols.data(), sizeof(pqg_take_record_column) * cols.size());
  const size_t n_in = n_cols > 0 && n_cols <= PQG_TAKE_MAX_COLUMNS ? (size_t)n_cols : 0;
  pqg::TakeRecDev* out = (pqg::TakeRecDev*)malloc(sizeof(pqg::TakeRecDev) * (n_in ? 2 * n_in : 1));
  pqg::TakeRecPlan plan{};
  const int rc = pqg::take_records_validate(ctx, bitmap, n_rows, in, n_cols, rows_cap, counts, result, out, &plan);
  t.cases++;
  if (rc == PQG_OK) {
    t.ok++;
    size_t n_rep = 0;
    uint64_t max_rows = n_rows, slot_words = 0;
    for (size_t i = 0; i < n_in; i++) {  // the records are fully written and consistent with their columns
      const pqg_take_record_column& r = cols[i];
      const pqg_take_column& c = r.col;
      const pqg::TakeRecDev& d = out[i];
      const bool missing = c.max_def > 0 && !c.def_levels;
      if (missing != (d.c.kind == pqg::TAKE_MISSING) || d.c.max_def != c.max_def || d.keep_col != i) t.other++;
      if (missing) continue;
      if (d.c.values != c.values || d.c.out_values != c.out_values || d.c.n_values != c.n_values || d.c.width == 0 ||
          d.c.cap_values != c.out_values_capacity || (d.c.dl != nullptr) != (c.max_def > 0))
        t.other++;
      const uint64_t n = r.max_rep > 0 ? r.n_slots : n_rows;
      if (d.n != n || (d.rl != nullptr) != (r.max_rep > 0) || d.own_bitmap != (r.max_rep > 0 ? 1u : 0u)) t.other++;
      if (n > max_rows) max_rows = n;
      if (r.max_rep == 0) {
        if (d.bitmap != bitmap || d.cap_levels != rows_cap) t.other++;
        continue;
      }
      // a repeated column: its slot bitmap, and a second record for its repetition bytes on the same bitmap
      const pqg::TakeRecDev& q = out[n_in + n_rep];
      if (d.rl != r.rep_levels || d.cap_levels != r.out_slots_capacity || d.slot_off != slot_words) t.other++;
      if (q.c.kind != pqg::TAKE_W1 || q.c.values != r.rep_levels || q.c.out_values != r.out_rep_levels || q.c.dl || q.rl ||
          q.c.n_values != r.n_slots || q.c.cap_values != (r.out_rep_levels ? r.out_slots_capacity : 0) || q.n != r.n_slots ||
          q.own_bitmap != 1 || q.slot_off != d.slot_off || q.keep_col != i)
        t.other++;
      slot_words += (r.n_slots + PQG_FILTER_TILE_ROWS - 1) / PQG_FILTER_TILE_ROWS * (PQG_FILTER_TILE_ROWS / 64);
      n_rep++;
    }
    if (plan.n_records != n_in + n_rep || plan.max_rows != max_rows || plan.slot_words != slot_words ||
        plan.any_repeated != (n_rep > 0))
      t.other++;
  } else if (rc == PQG_ERR_INVALID_ARG) {
    t.invalid++;
  } else if (rc == PQG_ERR_UNSUPPORTED) {
    t.unsupported++;
  } else {
    t.other++;
  }
  free(in);
  free(out);
  return rc;
}

int main(int argc, char** argv) {
  const long n_mut = argc > 1 ? atol(argv[1]) : 1000;
  Tally t;
  const uint64_t* bitmap = (const uint64_t*)dev(1000001);
  const pqg_take_record_counts* counts = (const pqg_take_record_counts*)dev(1000002);
  const pqg_take_result* result = (const pqg_take_result*)dev(1000003);
  const uint64_t n_rows = 100000;
  typedef pqg_take_record_column Col;

  // valid tables of every size: every type in turn; flat required / flat nullable / repeated / missing
  std::vector<std::vector<Col>> bases;
  for (int n : {0, 1, 2, 7, 8, 33, PQG_TAKE_MAX_COLUMNS}) {
    std::vector<Col> cols;
    for (int i = 0; i < n; i++) {
      const int shape = (i / 8) % 4;  // 0 required, 1 nullable, 2 repeated, 3 missing (flat or repeated)
      const int max_def = shape == 0 ? 0 : (i % 4) + 1;
      const int max_rep = shape == 2 || (shape == 3 && i % 2) ? 1 + i % 3 : 0;
      cols.push_back(column(i % 8, max_def, max_rep, shape == 3, n_rows, (uint64_t)i * 1000, (uint64_t)i));
    }
    if (run(t, true, bitmap, n_rows, cols, n, n_rows, counts, result) != PQG_OK) {
      fprintf(stderr, "a valid table of %d columns was refused\n", n);
      return 1;
    }
    bases.push_back(cols);
  }
  // the refusals the header lists
  {
    std::vector<Col> flat = {column(PQG_INT64, 1, 0, false, n_rows, 0, 1)};
    std::vector<Col> list = {column(PQG_INT64, 2, 1, false, n_rows, 500, 2)};
    std::vector<Col> many(PQG_TAKE_MAX_COLUMNS + 1, list[0]);
    int bad = 0;
    for (const auto& one : {flat, list}) {
      bad += run(t, true, bitmap, n_rows, one, 1, n_rows, counts, result) != PQG_OK;
      bad += run(t, false, bitmap, n_rows, one, 1, n_rows, counts, result) != PQG_ERR_INVALID_ARG;
      bad += run(t, true, nullptr, n_rows, one, 1, n_rows, counts, result) != PQG_ERR_INVALID_ARG;
      bad += run(t, true, bitmap, n_rows, one, 1, n_rows, nullptr, result) != PQG_ERR_INVALID_ARG;
      bad += run(t, true, bitmap, n_rows, one, 1, n_rows, counts, nullptr) != PQG_ERR_INVALID_ARG;
      bad += run(t, true, bitmap, n_rows, one, -1, n_rows, counts, result) != PQG_ERR_INVALID_ARG;
    }
    bad += run(t, true, nullptr, 0, {column(PQG_INT64, 1, 0, false, 0, 0, 1)}, 1, 0, counts, result) != PQG_OK;  // no rows
    bad += run(t, true, bitmap, n_rows, {}, 1, n_rows, counts, result) != PQG_ERR_INVALID_ARG;
    bad += run(t, true, bitmap, n_rows, {}, 0, n_rows, counts, result) != PQG_OK;
    bad += run(t, true, bitmap, n_rows, many, PQG_TAKE_MAX_COLUMNS + 1, n_rows, counts, result) != PQG_ERR_UNSUPPORTED;
    auto with = [&](const std::vector<Col>& base, auto&& edit) {
      std::vector<Col> c = base;
      edit(c[0]);
      return run(t, true, bitmap, n_rows, c, 1, n_rows, counts, result);
    };
    // what take_validate refuses for `col`, on a flat and on a repeated column
    for (const auto& one : {flat, list}) {
      bad += with(one, [](Col& c) { c.col.max_def = 255; }) != PQG_ERR_INVALID_ARG;
      bad += with(one, [](Col& c) { c.col.max_def = -1; }) != PQG_ERR_INVALID_ARG;
      bad += with(one, [](Col& c) { c.col.physical_type = 8; }) != PQG_ERR_INVALID_ARG;
      bad += with(one, [](Col& c) { c.col.physical_type = PQG_FIXED_LEN_BYTE_ARRAY; c.col.type_length = 0; }) != PQG_ERR_INVALID_ARG;
      bad += with(one, [](Col& c) { c.col.values = nullptr; }) != PQG_ERR_INVALID_ARG;
      bad += with(one, [](Col& c) { c.col.out_values = nullptr; }) != PQG_ERR_INVALID_ARG;
      bad += with(one, [](Col& c) { c.col.out_def_levels = nullptr; }) != PQG_ERR_INVALID_ARG;
      bad += with(one, [](Col& c) { c.col.values = (const uint8_t*)c.col.values + 4; }) != PQG_ERR_INVALID_ARG;
      bad += with(one, [](Col& c) { c.col.physical_type = PQG_BYTE_ARRAY; c.col.binary_data = nullptr; }) != PQG_ERR_INVALID_ARG;
      bad += with(one, [](Col& c) { c.col.physical_type = PQG_BYTE_ARRAY; c.col.out_binary_data = nullptr; }) != PQG_ERR_INVALID_ARG;
      bad += with(one, [](Col& c) { c.max_rep = 255; }) != PQG_ERR_INVALID_ARG;
      bad += with(one, [](Col& c) { c.max_rep = -1; }) != PQG_ERR_INVALID_ARG;
      bad += with(one, [](Col& c) { c.reserved = 1; }) != PQG_ERR_INVALID_ARG;
      bad += with(one, [&](Col& c) { c.n_slots = n_rows - 1; }) != PQG_ERR_INVALID_ARG;
    }
    bad += with(flat, [&](Col& c) { c.col.max_def = 0; c.col.n_values = n_rows - 1; }) != PQG_ERR_INVALID_ARG;
    bad += with(flat, [](Col& c) { c.rep_levels = (const uint8_t*)dev(77); }) != PQG_ERR_INVALID_ARG;
    bad += with(flat, [&](Col& c) { c.n_slots = n_rows + 1; }) != PQG_ERR_INVALID_ARG;
    bad += with(flat, [](Col& c) { c.out_rep_levels = (uint8_t*)dev(78); c.out_slots_capacity = 5; }) != PQG_OK;  // unused
    bad += with(list, [](Col& c) { c.max_rep = 254; }) != PQG_OK;
    bad += with(list, [](Col& c) { c.col.max_def = 0; c.col.def_levels = nullptr; c.col.out_def_levels = nullptr; }) != PQG_ERR_INVALID_ARG;
    bad += with(list, [](Col& c) { c.rep_levels = nullptr; }) != PQG_ERR_INVALID_ARG;
    bad += with(list, [](Col& c) { c.out_rep_levels = nullptr; }) != PQG_ERR_INVALID_ARG;
    bad += with(list, [](Col& c) { c.out_rep_levels = nullptr; c.col.out_def_levels = nullptr; c.out_slots_capacity = 0; }) != PQG_OK;
    bad += with(list, [&](Col& c) { c.n_slots = n_rows; c.col.n_values = 3; }) != PQG_OK;  // one slot per record
    // missing columns: no levels, so no slots either; a repeated one needs no rep_levels
    bad += with(list, [](Col& c) { c.col.def_levels = nullptr; c.col.values = nullptr; c.col.out_values = nullptr; c.rep_levels = nullptr; c.n_slots = 0; }) != PQG_OK;
    bad += with(flat, [](Col& c) { c.col.def_levels = nullptr; c.col.values = nullptr; c.col.out_values = nullptr; }) != PQG_OK;
    if (bad) {
      fprintf(stderr, "%d listed refusals came out differently\n", bad);
      return 1;
    }
  }
  // mutations: bit flips anywhere in one column, and of the call's own arguments
  for (const auto& base : bases) {
    for (long m = 0; m < n_mut; m++) {
      std::vector<Col> cols = base;
      int n_cols = (int)cols.size();
      uint64_t rows = n_rows, cap = n_rows;
      const uint64_t r = rnd();
      if (!cols.empty()) {
        uint8_t* raw = (uint8_t*)cols.data();
        const size_t bytes = sizeof(Col) * cols.size();
        for (int k = 0; k < 1 + (int)(r % 3); k++) raw[rnd() % bytes] ^= (uint8_t)(1u << (rnd() % 8));
      }
      switch ((r >> 8) % 8) {
        case 0: n_cols = (int)(rnd() % 200) - 50; break;
        case 1: rows = rnd(); break;
        case 2: cap = rnd(); break;
        default: break;
      }
      if (n_cols > (int)cols.size()) cols.resize((size_t)n_cols, column(PQG_INT32, 0, 0, false, n_rows, 0, 5));
      run(t, true, bitmap, rows, cols, n_cols, cap, counts, result);
    }
  }
  printf("cases=%ld ok=%ld invalid=%ld unsupported=%ld\n", t.cases, t.ok, t.invalid, t.unsupported);
  return t.other ? 1 : 0;
}
