/*
 * take_sanitize.cpp — the host half of pqg_take (csrc/pqgpu_take_host.cpp: the refusals made before
 * any launch, the per-column table) under AddressSanitizer + UndefinedBehaviorSanitizer, without HIP.
 * Built by tests/test_take_sanitize.py with -fsanitize=address,undefined -fno-sanitize-recover=all,
 * so any finding aborts the run.
 *
 * usage: take_sanitize <mutations per base table>
 * Valid column tables (every physical type, required / nullable / missing, dictionary ids, 0 to
 * PQG_TAKE_MAX_COLUMNS columns) must be accepted and come back as the table the kernels read;
 * deterministic mutations (flipped bits in any field, misaligned and NULL pointers, huge capacities,
 * negative and oversized column counts) must be accepted or refused with PQG_ERR_INVALID_ARG /
 * PQG_ERR_UNSUPPORTED. The column table and the output table are exactly-sized heap allocations, so an
 * access one entry past either is caught; the "device" pointers are never dereferenced (they are
 * made-up addresses here, so a dereference would fault).
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

static pqg_take_column column(int type, int max_def, bool missing, uint64_t n_rows, uint64_t k) {
  pqg_take_column c{};
  c.physical_type = type;
  c.max_def = max_def;
  c.type_length = type == PQG_FIXED_LEN_BYTE_ARRAY ? 1 + (int)(k % 20) : 0;
  c.flags = (type == PQG_BYTE_ARRAY && k % 3 == 0) ? PQG_COLUMN_DICTIONARY_IDS : 0;
  if (missing) return c;
  c.values = dev(8 * k);
  c.binary_data = (const uint8_t*)dev(8 * k + 1);
  c.def_levels = max_def ? (const uint8_t*)dev(8 * k + 2) : nullptr;
  c.n_values = n_rows;
  c.out_values = dev(8 * k + 3);
  c.out_binary_data = (uint8_t*)dev(8 * k + 4);
  c.out_def_levels = max_def ? (uint8_t*)dev(8 * k + 5) : nullptr;
  c.out_values_capacity = n_rows;
  c.out_binary_capacity = 1000;
  return c;
}

struct Tally {
  long cases = 0, ok = 0, invalid = 0, unsupported = 0, other = 0;
};

static int run(Tally& t, bool ctx, const uint64_t* bitmap, uint64_t n_rows, const std::vector<pqg_take_column>& cols,
               int n_cols, uint64_t rows_cap, const pqg_take_counts* counts, const pqg_take_result* result) {
  // exactly-sized heap copies: n_cols entries in, at most PQG_TAKE_MAX_COLUMNS entries out
  pqg_take_column* in = cols.empty() ? nullptr : (pqg_take_column*)malloc(sizeof(pqg_take_column) * cols.size());
  if (in) memcpy(in, cols.data(), sizeof(pqg_take_column) * cols.size());
  const size_t n_out = n_cols > 0 && n_cols <= PQG_TAKE_MAX_COLUMNS ? (size_t)n_cols : 0;
  pqg::TakeColDev* out = (pqg::TakeColDev*)malloc(sizeof(pqg::TakeColDev) * (n_out ? n_out : 1));
  const int rc = pqg::take_validate(ctx, bitmap, n_rows, in, n_cols, rows_cap, counts, result, out);
  t.cases++;
  if (rc == PQG_OK) {
    t.ok++;
    for (size_t i = 0; i < n_out; i++) {  // the table is fully written and consistent with its column
      const pqg_take_column& c = cols[i];
      const pqg::TakeColDev& d = out[i];
      const bool missing = c.max_def > 0 && !c.def_levels;
      if (missing != (d.kind == pqg::TAKE_MISSING) || d.max_def != c.max_def) t.other++;
      if (!missing && (d.values != c.values || d.out_values != c.out_values || d.n_values != c.n_values || d.width == 0 ||
                       d.cap_values != c.out_values_capacity || (d.dl != nullptr) != (c.max_def > 0)))
        t.other++;
    }
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
  const pqg_take_counts* counts = (const pqg_take_counts*)dev(1000002);
  const pqg_take_result* result = (const pqg_take_result*)dev(1000003);
  const uint64_t n_rows = 100000;

  // valid tables of every size, every type in turn, required / nullable / missing
  std::vector<std::vector<pqg_take_column>> bases;
  for (int n : {0, 1, 2, 7, 8, 33, PQG_TAKE_MAX_COLUMNS}) {
    std::vector<pqg_take_column> cols;
    for (int i = 0; i < n; i++) cols.push_back(column(i % 8, (i / 8) % 3 == 0 ? 0 : (i % 4) + 1, (i / 8) % 3 == 2, n_rows, (uint64_t)i));
    if (run(t, true, bitmap, n_rows, cols, n, n_rows, counts, result) != PQG_OK) {
      fprintf(stderr, "a valid table of %d columns was refused\n", n);
      return 1;
    }
    bases.push_back(cols);
  }
  // the refusals the header lists
  {
    std::vector<pqg_take_column> one = {column(PQG_INT64, 1, false, n_rows, 1)};
    std::vector<pqg_take_column> many(PQG_TAKE_MAX_COLUMNS + 1, one[0]);
    int bad = 0;
    bad += run(t, false, bitmap, n_rows, one, 1, n_rows, counts, result) != PQG_ERR_INVALID_ARG;
    bad += run(t, true, nullptr, n_rows, one, 1, n_rows, counts, result) != PQG_ERR_INVALID_ARG;
    bad += run(t, true, nullptr, 0, one, 1, n_rows, counts, result) != PQG_OK;  // no rows: no bitmap needed
    bad += run(t, true, bitmap, n_rows, one, 1, n_rows, nullptr, result) != PQG_ERR_INVALID_ARG;
    bad += run(t, true, bitmap, n_rows, one, 1, n_rows, counts, nullptr) != PQG_ERR_INVALID_ARG;
    bad += run(t, true, bitmap, n_rows, one, -1, n_rows, counts, result) != PQG_ERR_INVALID_ARG;
    bad += run(t, true, bitmap, n_rows, {}, 1, n_rows, counts, result) != PQG_ERR_INVALID_ARG;
    bad += run(t, true, bitmap, n_rows, many, PQG_TAKE_MAX_COLUMNS + 1, n_rows, counts, result) != PQG_ERR_UNSUPPORTED;
    auto with = [&](auto&& edit) {
      std::vector<pqg_take_column> c = one;
      edit(c[0]);
      return run(t, true, bitmap, n_rows, c, 1, n_rows, counts, result);
    };
    bad += with([](pqg_take_column& c) { c.max_def = 255; }) != PQG_ERR_INVALID_ARG;
    bad += with([](pqg_take_column& c) { c.max_def = -1; }) != PQG_ERR_INVALID_ARG;
    bad += with([](pqg_take_column& c) { c.physical_type = 8; }) != PQG_ERR_INVALID_ARG;
    bad += with([](pqg_take_column& c) { c.physical_type = PQG_FIXED_LEN_BYTE_ARRAY; c.type_length = 0; }) != PQG_ERR_INVALID_ARG;
    bad += with([](pqg_take_column& c) { c.values = nullptr; }) != PQG_ERR_INVALID_ARG;
    bad += with([](pqg_take_column& c) { c.out_values = nullptr; }) != PQG_ERR_INVALID_ARG;
    bad += with([](pqg_take_column& c) { c.out_def_levels = nullptr; }) != PQG_ERR_INVALID_ARG;
    bad += with([](pqg_take_column& c) { c.values = (const uint8_t*)c.values + 4; }) != PQG_ERR_INVALID_ARG;
    bad += with([](pqg_take_column& c) { c.physical_type = PQG_BYTE_ARRAY; c.binary_data = nullptr; }) != PQG_ERR_INVALID_ARG;
    bad += with([](pqg_take_column& c) { c.physical_type = PQG_BYTE_ARRAY; c.out_binary_data = nullptr; }) != PQG_ERR_INVALID_ARG;
    bad += with([&](pqg_take_column& c) { c.max_def = 0; c.n_values = n_rows - 1; }) != PQG_ERR_INVALID_ARG;
    bad += with([](pqg_take_column& c) { c.def_levels = nullptr; c.values = nullptr; c.out_values = nullptr; }) != PQG_OK;  // missing
    bad += with([](pqg_take_column& c) { c.physical_type = PQG_FIXED_LEN_BYTE_ARRAY; c.type_length = 5; c.values = (const uint8_t*)c.values + 3; }) != PQG_OK;
    if (bad) {
      fprintf(stderr, "%d listed refusals came out differently\n", bad);
      return 1;
    }
  }
  // mutations: bit flips anywhere in one column, and of the call's own arguments
  for (const auto& base : bases) {
    for (long m = 0; m < n_mut; m++) {
      std::vector<pqg_take_column> cols = base;
      int n_cols = (int)cols.size();
      uint64_t rows = n_rows, cap = n_rows;
      const uint64_t r = rnd();
      if (!cols.empty()) {
        uint8_t* raw = (uint8_t*)cols.data();
        const size_t bytes = sizeof(pqg_take_column) * cols.size();
        for (int k = 0; k < 1 + (int)(r % 3); k++) raw[rnd() % bytes] ^= (uint8_t)(1u << (rnd() % 8));
      }
      switch ((r >> 8) % 8) {
        case 0: n_cols = (int)(rnd() % 200) - 50; break;
        case 1: rows = rnd(); break;
        case 2: cap = rnd(); break;
        default: break;
      }
      if (n_cols > (int)cols.size()) cols.resize((size_t)n_cols, column(PQG_INT32, 0, false, n_rows, 5));
      run(t, true, bitmap, rows, cols, n_cols, cap, counts, result);
    }
  }
  printf("cases=%ld ok=%ld invalid=%ld unsupported=%ld\n", t.cases, t.ok, t.invalid, t.unsupported);
  return t.other ? 1 : 0;
}
