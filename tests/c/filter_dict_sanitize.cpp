/*
 * filter_dict_sanitize.cpp — the host binding of pqg_filter_run / pqg_filter_run_dict
 * (csrc/pqgpu_filter_host.cpp: pqg::filter_bind, the refusals made before any launch, the slot table and
 * the dictionary table with the leaves' verdict-table offsets) under AddressSanitizer +
 * UndefinedBehaviorSanitizer, without HIP. Built by tests/test_filter_dict_sanitize.py with
 * -fsanitize=address,undefined -fno-sanitize-recover=all, so any finding aborts the run.
 *
 * usage: filter_dict_sanitize <mutations per base case>
 * Valid bindings (value columns, id columns with dictionaries of 0, 1, 64, 65, 1,000 and 2^32 - 1 entries,
 * the largest program a tree admits: 32 leaves on 32 columns, every one with a table) must be accepted and
 * come back consistent; the refusals the header lists must come back as PQG_ERR_INVALID_ARG; deterministic
 * mutations (bit flips in any field of the column and dictionary tables, wrong column counts) must be
 * accepted or refused, never crashed on. The column and dictionary tables are exactly-sized heap blocks,
 * so an access one entry past either is caught; the "device" pointers are made-up addresses that are never
 * dereferenced.
 * Prints: cases=<n> ok=<n> invalid=<n>; exit status 1 on any other outcome.
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../parquet-mr_amd/csrc/pqgpu_filter.h"

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {  // xorshift64*
  g_state ^= g_state >> 12;
  g_state ^= g_state << 25;
  g_state ^= g_state >> 27;
  return g_state * 0x2545F4914F6CDD1Dull;
}

static void* dev(uint64_t k) { return (void*)(uintptr_t)(0x7000000000ull + k * 4096); }

static const int TYPES[6] = {PQG_BOOLEAN, PQG_INT32, PQG_INT64, PQG_FLOAT, PQG_DOUBLE, PQG_BYTE_ARRAY};

struct Case {
  pqg_filter* filter = nullptr;
  std::vector<pqg_filter_column> cols;
  std::vector<pqg_filter_dictionary> dicts;
  uint64_t n_rows = 0;
};

// n_leaves leaves (eq, or eq null on every third when with_null), leaf i on column i, and-ed in a chain
static Case make_case(int n_leaves, uint64_t n_rows, const std::vector<uint32_t>& entries, bool with_null) {
  Case c;
  c.n_rows = n_rows;
  std::vector<pqg_filter_node> nodes;
  std::vector<int32_t> types;
  std::vector<uint64_t> lits;
  const uint8_t bytes[4] = {'a', 'b', 'c', 'd'};
  for (int i = 0; i < n_leaves; i++) {
    const int t = TYPES[i % 6];
    types.push_back(t);
    pqg_filter_node nd{};
    nd.op = PQG_FILTER_EQ;
    nd.column = i;
    nd.left = nd.right = -1;
    if (with_null && i % 3 == 2) {
      nd.flags = PQG_FILTER_NULL_LITERAL;
    } else {
      nd.literal_begin = (uint32_t)lits.size();
      nd.n_literals = 1;
      lits.push_back(t == PQG_BYTE_ARRAY ? (3ull << 32) : (uint64_t)i);
    }
    nodes.push_back(nd);
  }
  for (int i = 1; i < n_leaves; i++) {
    pqg_filter_node nd{};
    nd.op = PQG_FILTER_AND;
    nd.column = -1;
    nd.left = i == 1 ? 0 : n_leaves + i - 2;
    nd.right = i;
    nodes.push_back(nd);
  }
  pqg_status st;
  if (pqg_filter_create(nodes.data(), (int)nodes.size(), types.data(), n_leaves, lits.data(), (int)lits.size(), bytes, 4,
                        &c.filter, &st) != PQG_OK) {
    fprintf(stderr, "pqg_filter_create: %s\n", st.message);
    exit(1);
  }
  for (int i = 0; i < n_leaves; i++) {
    pqg_filter_column fc{};
    fc.physical_type = types[(size_t)i];
    fc.max_def = i % 2;
    fc.values = dev(8 * (uint64_t)i);
    fc.binary_data = (const uint8_t*)dev(8 * (uint64_t)i + 1);
    fc.def_levels = fc.max_def ? (const uint8_t*)dev(8 * (uint64_t)i + 2) : nullptr;
    fc.n_values = n_rows;
    c.cols.push_back(fc);
    pqg_filter_dictionary d{};
    if (!entries.empty()) {
      d.values = dev(8 * (uint64_t)i + 3);
      d.binary_data = (const uint8_t*)dev(8 * (uint64_t)i + 4);
      d.n_entries = entries[(size_t)i % entries.size()];
    }
    c.dicts.push_back(d);
  }
  return c;
}

struct Tally {
  long cases = 0, ok = 0, invalid = 0, other = 0;
};

// one binding through exactly-sized heap copies of both tables; an accepted one is checked for consistency
static int run(Tally& t, const pqg_filter* filter, const std::vector<pqg_filter_column>& cols,
               const std::vector<pqg_filter_dictionary>* dicts, int n_cols, uint64_t n_rows) {
  pqg_filter_column* in = cols.empty() ? nullptr : (pqg_filter_column*)malloc(sizeof(pqg_filter_column) * cols.size());
  if (in) memcpy(in, cols.data(), sizeof(pqg_filter_column) * cols.size());
  pqg_filter_dictionary* din = nullptr;
  if (dicts && !dicts->empty()) {
    din = (pqg_filter_dictionary*)malloc(sizeof(pqg_filter_dictionary) * dicts->size());
    memcpy(din, dicts->data(), sizeof(pqg_filter_dictionary) * dicts->size());
  }
  pqg::FilterCols* fc = (pqg::FilterCols*)malloc(sizeof(pqg::FilterCols));
  pqg::FilterDictTab* dt = (pqg::FilterDictTab*)malloc(sizeof(pqg::FilterDictTab));
  bool any = false;
  const int rc = pqg::filter_bind(filter, in, din, n_cols, n_rows, fc, din ? dt : nullptr, &any);
  t.cases++;
  if (rc == PQG_OK) {
    t.ok++;
    if (fc->n_slots != filter->slot_column.size() || fc->n_nullable > fc->n_slots) t.other++;
    uint64_t words = 0, largest = 0;
    uint32_t tables = 0;
    if (any) {
      for (size_t i = 0; i < filter->program.size(); i++) {
        const pqg_filter_node& nd = filter->program[i];
        const bool leaf = nd.op <= PQG_FILTER_NOTIN;
        uint32_t s = 0;
        while (leaf && filter->slot_column[s] != nd.column) s++;
        const bool table = leaf && !(nd.flags & PQG_FILTER_NULL_LITERAL) && dt->slot[s].is_dict;
        if (!table) {
          if (dt->leaf_off[i] != pqg::FILTER_NO_TABLE) t.other++;
          continue;
        }
        const pqg_filter_dictionary& d = (*dicts)[(size_t)nd.column];
        const uint64_t w = ((uint64_t)d.n_entries + 63) / 64;
        if (dt->leaf_off[i] != words || dt->slot[s].n_entries != d.n_entries || dt->slot[s].values != d.values ||
            fc->c[s].values != cols[(size_t)nd.column].values)
          t.other++;
        if (w && (tables >= PQG_FILTER_MAX_NODES || dt->table_leaf[tables++] != i)) t.other++;
        words += w;
        largest = w > largest ? w : largest;
      }
      if (dt->table_words != words || dt->n_tables != tables || dt->max_words != largest ||
          (dt->in_lds != 0) != (words > 0 && words * 8 <= PQG_FILTER_DICT_LDS_BYTES))
        t.other++;
    }
  } else if (rc == PQG_ERR_INVALID_ARG) {
    t.invalid++;
  } else {
    t.other++;
  }
  free(in);
  free(din);
  free(fc);
  free(dt);
  return rc;
}

int main(int argc, char** argv) {
  const long n_mut = argc > 1 ? atol(argv[1]) : 1000;
  Tally t;
  const uint64_t n_rows = 100000;
  std::vector<Case> bases;
  bases.push_back(make_case(1, n_rows, {}, false));                                // values only
  bases.push_back(make_case(6, n_rows, {7}, true));                                // every type, null literals
  bases.push_back(make_case(12, n_rows, {0u, 1u, 64u, 65u, 1000u, 0xFFFFFFFFu}, false));  // n_entries 0 ... 2^32 - 1
  bases.push_back(make_case(32, n_rows, {1000u}, false));  // the largest tree: 32 leaves + 31 ands, 32 slots with tables
  bases.push_back(make_case(32, n_rows, {0xFFFFFFFFu}, false));
  bases.push_back(make_case(8, n_rows, {8192u}, false));   // 8 tables of 1 KiB: exactly PQG_FILTER_DICT_LDS_BYTES
  bases.push_back(make_case(8, n_rows, {8193u}, false));   // one word each over it
  int bad = 0;
  for (const Case& c : bases) {
    bad += run(t, c.filter, c.cols, &c.dicts, (int)c.cols.size(), c.n_rows) != PQG_OK;
    bad += run(t, c.filter, c.cols, nullptr, (int)c.cols.size(), c.n_rows) != PQG_OK;  // as pqg_filter_run binds them
  }
  if (bad) {
    fprintf(stderr, "%d valid bindings were refused\n", bad);
    return 1;
  }
  {  // the refusals the header lists, each on the six-column case
    const Case& b = bases[1];
    auto with = [&](auto&& edit) {
      Case c;
      c.cols = b.cols;
      c.dicts = b.dicts;
      edit(c);
      return run(t, b.filter, c.cols, &c.dicts, (int)c.cols.size(), b.n_rows);
    };
    bad += with([](Case& c) { c.cols[2].physical_type = PQG_INT32; }) != PQG_ERR_INVALID_ARG;         // wrong type
    bad += with([](Case& c) { c.cols[1].def_levels = nullptr; }) != PQG_ERR_INVALID_ARG;              // missing column with a dictionary
    bad += with([](Case& c) { c.cols[1].def_levels = nullptr; c.dicts[1].values = nullptr; }) != PQG_OK;  // ... without: a missing column
    bad += with([](Case& c) { c.dicts[5].binary_data = nullptr; }) != PQG_ERR_INVALID_ARG;            // BYTE_ARRAY dictionary without bytes
    bad += with([](Case& c) { c.cols[5].binary_data = nullptr; }) != PQG_OK;                          // the id column needs none
    bad += with([](Case& c) { c.cols[0].values = (const uint8_t*)c.cols[0].values + 2; }) != PQG_ERR_INVALID_ARG;  // misaligned ids
    bad += with([](Case& c) { c.dicts[3].reserved = 1; }) != PQG_ERR_INVALID_ARG;
    bad += with([](Case& c) { c.cols[4].max_def = 255; }) != PQG_ERR_INVALID_ARG;
    bad += with([](Case& c) { c.cols[0].n_values = 99999; }) != PQG_ERR_INVALID_ARG;                  // required: a value per row
    bad += with([](Case& c) { c.cols[0].values = nullptr; }) != PQG_ERR_INVALID_ARG;
    bad += with([](Case& c) { c.dicts[0].n_entries = 0; }) != PQG_OK;
    bad += with([](Case& c) { c.dicts[0].n_entries = 0xFFFFFFFFu; }) != PQG_OK;
    bad += run(t, b.filter, b.cols, &b.dicts, 5, b.n_rows) != PQG_ERR_INVALID_ARG;                    // not the filter's column count
    bad += run(t, nullptr, b.cols, &b.dicts, 6, b.n_rows) != PQG_ERR_INVALID_ARG;
    if (bad) {
      fprintf(stderr, "%d listed refusals came out differently\n", bad);
      return 1;
    }
  }
  for (const Case& base : bases) {
    for (long m = 0; m < n_mut; m++) {
      std::vector<pqg_filter_column> cols = base.cols;
      std::vector<pqg_filter_dictionary> dicts = base.dicts;
      const uint64_t r = rnd();
      uint8_t* raw = (r & 1) ? (uint8_t*)cols.data() : (uint8_t*)dicts.data();
      const size_t bytes = (r & 1) ? sizeof(pqg_filter_column) * cols.size() : sizeof(pqg_filter_dictionary) * dicts.size();
      for (int k = 0; k < 1 + (int)((r >> 1) % 3); k++) raw[rnd() % bytes] ^= (uint8_t)(1u << (rnd() % 8));
      const uint64_t rows = (r >> 8) % 8 == 0 ? rnd() : base.n_rows;
      run(t, base.filter, cols, &dicts, (int)cols.size(), rows);
    }
  }
  for (Case& c : bases) pqg_filter_destroy(c.filter);
  printf("cases=%ld ok=%ld invalid=%ld\n", t.cases, t.ok, t.invalid);
  return t.other ? 1 : 0;
}
