/*
 * rowgroup_sanitize.cpp — the host half of pqg_filter_row_groups (csrc/pqgpu_rowgroup_host.cpp:
 * pqg::rowgroup_bind, the refusals made before any launch, the (row group, slot) table with the "usable" rule
 * and the flat work list; pqg_chunk_has_non_dictionary_pages) and the row-group form of the program image
 * (csrc/pqgpu_filter_host.cpp: pqg_filter::rg_image, the equality leaves of binary columns keyed by their
 * bytes) under AddressSanitizer + UndefinedBehaviorSanitizer, without HIP. Built by
 * tests/test_rowgroup_sanitize.py with -fsanitize=address,undefined -fno-sanitize-recover=all, so any
 * finding aborts the run.
 *
 * usage: rowgroup_sanitize <mutations per base case>
 * Valid tables (0 to 130 row groups; dictionaries of 0, 1, 1,024, 1,025 and 2^32 - 1 entries; every flag
 * combination; every physical type; 32 leaves on 32 columns) must be accepted and come back consistent:
 * one table entry per (row group, slot), an item per tile of every usable dictionary a comparing leaf
 * stands on, in row-group order, every item inside its dictionary. The refusals the header lists must come
 * back as PQG_ERR_INVALID_ARG. Deterministic mutations (bit flips in any field of the table, wrong column
 * and row-group counts) must be accepted or refused, never crashed on. The table is an exactly-sized heap
 * block, so an access one entry past it is caught; the "device" pointers are made-up addresses that are
 * never dereferenced.
 * Prints: cases=<n> ok=<n> invalid=<n>; exit status 1 on any other outcome.
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../parquet-mr_amd/csrc/pqgpu_rowgroup.h"

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {  // xorshift64*
  g_state ^= g_state >> 12;
  g_state ^= g_state << 25;
  g_state ^= g_state >> 27;
  return g_state * 0x2545F4914F6CDD1Dull;
}

static void* dev(uint64_t k) { return (void*)(uintptr_t)(0x7000000000ull + k * 4096); }

static const int TYPES[8] = {PQG_BOOLEAN, PQG_INT32, PQG_INT64, PQG_INT96, PQG_FLOAT, PQG_DOUBLE, PQG_BYTE_ARRAY,
                             PQG_FIXED_LEN_BYTE_ARRAY};

struct Case {
  pqg_filter* filter = nullptr;
  std::vector<pqg_rowgroup_column> cols;
  int n_cols = 0;
  uint64_t n_groups = 0;
};

// n_leaves leaves, leaf i on column i of type TYPES[i % 8] (eq; eq null on every fifth; in of 12 on every
// seventh), and-ed in a chain
static pqg_filter* make_filter(int n_leaves) {
  std::vector<pqg_filter_node> nodes;
  std::vector<pqg_filter_column_type> types;
  std::vector<uint64_t> lits;
  std::vector<uint8_t> bytes;
  for (int k = 0; k < 12; k++) {  // twelve literals of 12 bytes: 00 .. 00 k
    for (int b = 0; b < 11; b++) bytes.push_back(0);
    bytes.push_back((uint8_t)(11 - k));
  }
  for (int i = 0; i < n_leaves; i++) {
    const int t = TYPES[i % 8];
    pqg_filter_column_type ct{};
    ct.physical_type = t;
    ct.type_length = t == PQG_FIXED_LEN_BYTE_ARRAY ? 12 : 0;
    ct.binary_order = t == PQG_INT96 || t == PQG_FIXED_LEN_BYTE_ARRAY ? PQG_FILTER_ORDER_SIGNED_INTEGER : 0;
    types.push_back(ct);
    const bool binary = t == PQG_BYTE_ARRAY || t == PQG_INT96 || t == PQG_FIXED_LEN_BYTE_ARRAY;
    pqg_filter_node nd{};
    nd.op = PQG_FILTER_EQ;
    nd.column = i;
    nd.left = nd.right = -1;
    if (i % 5 == 4) {
      nd.flags = PQG_FILTER_NULL_LITERAL;
    } else {
      nd.literal_begin = (uint32_t)lits.size();
      nd.n_literals = 1;
      if (i % 7 == 6) {
        nd.op = PQG_FILTER_IN;
        nd.n_literals = 12;
      }
      for (uint32_t k = 0; k < nd.n_literals; k++) lits.push_back(binary ? (12ull << 32) | (12u * k) : (uint64_t)(i + k));
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
  pqg_filter* f = nullptr;
  pqg_status st;
  if (pqg_filter_create_typed(nodes.data(), (int)nodes.size(), types.data(), n_leaves, lits.data(), (int)lits.size(),
                              bytes.data(), bytes.size(), &f, &st) != PQG_OK) {
    fprintf(stderr, "pqg_filter_create_typed: %s\n", st.message);
    exit(1);
  }
  return f;
}

static Case make_case(int n_leaves, uint64_t n_groups, const std::vector<uint32_t>& entries) {
  Case c;
  c.filter = make_filter(n_leaves);
  c.n_cols = n_leaves;
  c.n_groups = n_groups;
  for (uint64_t g = 0; g < n_groups; g++)
    for (int i = 0; i < n_leaves; i++) {
      pqg_rowgroup_column rc{};
      rc.dict.values = dev(16 * g + 2 * (uint64_t)i);
      rc.dict.binary_data = (const uint8_t*)dev(16 * g + 2 * (uint64_t)i + 1);
      rc.dict.n_entries = entries[(size_t)((g + (uint64_t)i) % entries.size())];
      rc.flags = (uint32_t)((g * 7 + (uint64_t)i) % 16);  // every combination of the four flags
      c.cols.push_back(rc);
    }
  return c;
}

struct Tally {
  long cases = 0, ok = 0, invalid = 0, other = 0;
};

static bool decodable(int t) { return t != PQG_BOOLEAN && t != PQG_INT96; }

// one binding through an exactly-sized heap copy of the table; an accepted one is checked for consistency
static int run(Tally& t, const pqg_filter* filter, const std::vector<pqg_rowgroup_column>& cols, int n_cols,
               uint64_t n_groups) {
  pqg_rowgroup_column* in = cols.empty() ? nullptr : (pqg_rowgroup_column*)malloc(sizeof(pqg_rowgroup_column) * cols.size());
  if (in) memcpy(in, cols.data(), sizeof(pqg_rowgroup_column) * cols.size());
  pqg::RgPlan plan;
  const int rc = pqg::rowgroup_bind(filter, in, n_cols, n_groups, &plan);
  t.cases++;
  if (rc == PQG_OK) {
    t.ok++;
    const uint32_t n_slots = (uint32_t)filter->slot_column.size();
    if (plan.n_slots != n_slots || plan.n_nodes != filter->program.size() || plan.cols.size() != n_groups * n_slots) t.other++;
    size_t it = 0;
    for (uint64_t g = 0; g < n_groups && !t.other; g++)
      for (uint32_t s = 0; s < n_slots; s++) {
        const int col = filter->slot_column[s];
        const pqg_rowgroup_column& c = cols[(size_t)(g * (uint64_t)n_cols + (uint64_t)col)];
        const pqg::RgColDev& d = plan.cols[(size_t)(g * n_slots + s)];
        const bool usable = !(c.flags & 7u) && decodable(filter->column_types[(size_t)col]);
        if (((d.flags & pqg::RG_USABLE) != 0) != usable || (d.flags & 15u) != c.flags) t.other++;
        if (d.n_entries != (usable ? c.dict.n_entries : 0u)) t.other++;
        if ((d.values != nullptr) != (usable && c.dict.n_entries > 0)) t.other++;
        bool compares = false;
        for (const pqg_filter_node& nd : filter->program)
          compares |= nd.op <= PQG_FILTER_NOTIN && nd.column == col && !(nd.flags & PQG_FILTER_NULL_LITERAL);
        if (!usable || !compares) continue;
        const uint64_t tiles = ((uint64_t)d.n_entries + pqg::RG_TILE - 1) / pqg::RG_TILE;
        for (uint64_t k = 0; k < tiles; k++, it++) {
          if (it >= plan.items.size()) {
            t.other++;
            break;
          }
          const pqg::RgItem& q = plan.items[it];
          if (q.group != g || (q.slot_tile >> 24) != s || (q.slot_tile & 0xFFFFFFu) != k ||
              (uint64_t)(q.slot_tile & 0xFFFFFFu) * pqg::RG_TILE >= d.n_entries)
            t.other++;
        }
      }
    if (it != plan.items.size()) t.other++;
  } else if (rc == PQG_ERR_INVALID_ARG) {
    t.invalid++;
  } else {
    t.other++;
  }
  free(in);
  return rc;
}

// the row-group image of `f` beside its own: the same shape, equality leaves of binary columns with raw cells
// (sets of more than 8 ascending by bytes), everything else untouched
static int check_images(const pqg_filter* f) {
  int bad = 0;
  const auto& a = f->image;
  const auto& b = f->rg_image;
  pqg::FilterDevHeader ha, hb;
  if (a.size() < sizeof(ha) || b.size() < sizeof(hb)) return 1;
  memcpy(&ha, a.data(), sizeof(ha));
  memcpy(&hb, b.data(), sizeof(hb));
  bad += ha.image_bytes != a.size() || hb.image_bytes != b.size() || hb.image_bytes % 8;
  bad += ha.n_nodes != hb.n_nodes || ha.n_leaves != hb.n_leaves || ha.n_slots != hb.n_slots || ha.n_bytes != hb.n_bytes;
  bad += hb.bytes_off != hb.cells_off + 8u * hb.n_cells || hb.bytes_off + hb.n_bytes > hb.image_bytes;
  if (bad) return bad;
  const uint8_t* lb = b.data() + hb.bytes_off;
  for (uint32_t i = 0; i < hb.n_nodes; i++) {
    pqg::FilterDevNode na, nb;
    memcpy(&na, a.data() + sizeof(ha) + i * sizeof(na), sizeof(na));
    memcpy(&nb, b.data() + sizeof(hb) + i * sizeof(nb), sizeof(nb));
    bad += na.op != nb.op || na.slot != nb.slot || na.type != nb.type || na.n_lit != nb.n_lit || na.width != nb.width;
    if (nb.op > PQG_FILTER_NOTIN) continue;
    bad += (uint64_t)nb.lit_begin + nb.n_lit > hb.n_cells;
    const bool binary = nb.type == PQG_BYTE_ARRAY || nb.type == PQG_INT96 || nb.type == PQG_FIXED_LEN_BYTE_ARRAY;
    const bool equality = nb.op == PQG_FILTER_EQ || nb.op == PQG_FILTER_NOTEQ || nb.op == PQG_FILTER_IN || nb.op == PQG_FILTER_NOTIN;
    if (!binary || !equality) {
      bad += (na.flags & ~pqg::FILTER_DEV_NULL_ONLY) != (nb.flags & ~pqg::FILTER_DEV_NULL_ONLY);
      continue;
    }
    bad += (nb.flags & (pqg::FILTER_DEV_SIGNED | pqg::FILTER_DEV_FLOAT16 | pqg::FILTER_DEV_KEY128)) != 0;
    std::vector<uint64_t> cells(nb.n_lit);
    if (nb.n_lit) memcpy(cells.data(), b.data() + hb.cells_off + 8u * nb.lit_begin, 8u * nb.n_lit);
    for (uint32_t k = 0; k < nb.n_lit; k++) {
      const uint64_t off = (uint32_t)cells[k], len = cells[k] >> 32;
      bad += off + len > hb.n_bytes;
      if (bad || !k || nb.n_lit <= pqg::FILTER_IN_LINEAR) continue;
      const uint64_t poff = (uint32_t)cells[k - 1], plen = cells[k - 1] >> 32;
      const size_t n = (size_t)(len < plen ? len : plen);
      const int c = n ? memcmp(lb + poff, lb + off, n) : 0;
      bad += c > 0 || (c == 0 && plen > len);  // ascending by unsigned bytes, then length
    }
  }
  return bad;
}

int main(int argc, char** argv) {
  const long n_mut = argc > 1 ? atol(argv[1]) : 1000;
  Tally t;
  std::vector<Case> bases;
  bases.push_back(make_case(1, 0, {7}));                                           // no row groups
  bases.push_back(make_case(8, 1, {7}));                                           // every type
  bases.push_back(make_case(8, 65, {0u, 1u, 1024u, 1025u, 4097u}));                 // tile seams, every flag combination
  bases.push_back(make_case(16, 130, {1000u}));
  bases.push_back(make_case(32, 3, {5u, 64u, 1000u, 0u, 0xFFFFFFFFu, 3u, 1u, 70000u, 9u, 2u, 11u}));  // the largest tree; 2^22 tiles in a dictionary
  int bad = 0;
  for (const Case& c : bases) {
    bad += run(t, c.filter, c.cols, c.n_cols, c.n_groups) != PQG_OK;
    bad += check_images(c.filter);
  }
  if (bad) {
    fprintf(stderr, "%d valid cases came out wrong\n", bad);
    return 1;
  }
  {  // the refusals the header lists, on the every-type case (columns 1, 2, 6: INT32, INT64, BYTE_ARRAY)
    const Case& b = bases[1];
    auto with = [&](auto&& edit) {
      std::vector<pqg_rowgroup_column> cols = b.cols;
      for (auto& c : cols) c.flags = 0;
      edit(cols);
      return run(t, b.filter, cols, b.n_cols, b.n_groups);
    };
    bad += with([](auto&) {}) != PQG_OK;
    bad += with([](auto& c) { c[2].reserved = 1; }) != PQG_ERR_INVALID_ARG;
    bad += with([](auto& c) { c[2].dict.reserved = 1; }) != PQG_ERR_INVALID_ARG;
    bad += with([](auto& c) { c[1].flags = 16; }) != PQG_ERR_INVALID_ARG;                        // unknown flag
    bad += with([](auto& c) { c[6].dict.binary_data = nullptr; }) != PQG_ERR_INVALID_ARG;       // BYTE_ARRAY without bytes
    bad += with([](auto& c) { c[6].dict.binary_data = nullptr; c[6].flags = PQG_RG_NO_DICTIONARY; }) != PQG_OK;
    bad += with([](auto& c) { c[6].dict.binary_data = nullptr; c[6].dict.n_entries = 0; }) != PQG_OK;
    bad += with([](auto& c) { c[1].dict.values = nullptr; }) != PQG_ERR_INVALID_ARG;
    bad += with([](auto& c) { c[1].dict.values = nullptr; c[1].flags = PQG_RG_MISSING; }) != PQG_OK;
    bad += with([](auto& c) { c[0].dict.values = nullptr; c[3].dict.values = nullptr; }) != PQG_OK;  // BOOLEAN, INT96: never read
    bad += with([](auto& c) { c[1].dict.n_entries = 0xFFFFFFFFu; }) != PQG_OK;
    bad += run(t, b.filter, b.cols, b.n_cols - 1, b.n_groups) != PQG_ERR_INVALID_ARG;          // not the filter's column count
    bad += run(t, b.filter, b.cols, b.n_cols + 1, b.n_groups) != PQG_ERR_INVALID_ARG;
    bad += run(t, nullptr, b.cols, b.n_cols, b.n_groups) != PQG_ERR_INVALID_ARG;
    bad += run(t, b.filter, {}, b.n_cols, b.n_groups) != PQG_ERR_INVALID_ARG;                  // row groups without a table
    bad += run(t, b.filter, {}, b.n_cols, 0) != PQG_OK;
    bad += run(t, b.filter, b.cols, b.n_cols, 0x80000000ull) != PQG_ERR_INVALID_ARG;           // tables that overflow
    bad += run(t, b.filter, b.cols, b.n_cols, ~0ull) != PQG_ERR_INVALID_ARG;
    // more work items than a call takes: 17 usable dictionaries of 2^32 - 1 entries on comparing leaves
    Case big = make_case(32, 1, {0xFFFFFFFFu});
    for (auto& c : big.cols) c.flags = 0;
    bad += run(t, big.filter, big.cols, big.n_cols, 1) != PQG_ERR_INVALID_ARG;
    pqg_filter_destroy(big.filter);
    if (bad) {
      fprintf(stderr, "%d listed refusals came out differently\n", bad);
      return 1;
    }
  }
  {  // pqg_chunk_has_non_dictionary_pages on exactly-sized tables
    for (int n = 0; n <= 4; n++) {
      pqg_page_encoding_stat* st = (pqg_page_encoding_stat*)malloc(sizeof(pqg_page_encoding_stat) * (size_t)(n ? n : 1));
      int32_t* enc = (int32_t*)malloc(sizeof(int32_t) * (size_t)(n ? n : 1));
      for (int i = 0; i < n; i++) {
        st[i] = pqg_page_encoding_stat{(int32_t)(rnd() % 4), (int32_t)(rnd() % 10), (int32_t)(rnd() % 3)};
        enc[i] = (int32_t)(rnd() % 10);
      }
      const int a = pqg_chunk_has_non_dictionary_pages(n ? st : nullptr, n, n ? enc : nullptr, n);
      const int b = pqg_chunk_has_non_dictionary_pages(nullptr, -1, n ? enc : nullptr, n);
      bad += (a != 0 && a != 1) || (b != 0 && b != 1);
      free(st);
      free(enc);
    }
    if (bad) return 1;
  }
  for (const Case& base : bases) {
    if (base.cols.empty()) continue;
    // the large tables and the work lists of millions of items cost more per binding
    const long muts = base.n_cols == 32 ? n_mut / 50 : base.cols.size() > 500 ? n_mut / 10 : n_mut;
    for (long m = 0; m < muts; m++) {
      std::vector<pqg_rowgroup_column> cols = base.cols;
      const uint64_t r = rnd();
      uint8_t* raw = (uint8_t*)cols.data();
      const size_t bytes = sizeof(pqg_rowgroup_column) * cols.size();
      for (int k = 0; k < 1 + (int)((r >> 1) % 3); k++) raw[rnd() % bytes] ^= (uint8_t)(1u << (rnd() % 8));
      uint64_t groups = base.n_groups;
      if ((r >> 8) % 8 == 0) groups = rnd() % (base.n_groups + 1);  // fewer row groups than the table holds
      run(t, base.filter, cols, base.n_cols, groups);
    }
  }
  for (Case& c : bases) pqg_filter_destroy(c.filter);
  printf("cases=%ld ok=%ld invalid=%ld\n", t.cases, t.ok, t.invalid);
  return t.other ? 1 : 0;
}
