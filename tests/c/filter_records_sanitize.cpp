/*
 * filter_records_sanitize.cpp — the host half of contains() (csrc/pqgpu_filter_host.cpp: the validation of
 * PQG_FILTER_CONTAINS nodes and the refusals of LogicalInverter and ContainsRewriter in pqg_filter_create,
 * and pqg::filter_bind_records with the FilterRecTab it fills) under AddressSanitizer +
 * UndefinedBehaviorSanitizer, without HIP. Built by tests/test_filter_records_sanitize.py with
 * -fsanitize=address,undefined -fno-sanitize-recover=all, so any finding aborts the run.
 *
 * usage: filter_records_sanitize <mutations per base case>
 * Part 1, creation: valid node tables with contains nodes must be accepted, every listed refusal must come
 * back with its code and node, and deterministic mutations of the node table (bit flips in any field, in
 * an exactly-sized heap block) must be accepted or refused, never crashed on.
 * Part 2, binding: valid record-column tables (flat, repeated and missing columns, dictionaries) must be
 * accepted and come back consistent, every refusal the header lists must be PQG_ERR_INVALID_ARG, and bit
 * flips in the column and dictionary tables must be accepted or refused. The "device" pointers are made-up
 * addresses that are never dereferenced.
 * Prints: cases=<n> ok=<n> invalid=<n> unsupported=<n>; exit status 1 on any other outcome.
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

struct Tally {
  long cases = 0, ok = 0, invalid = 0, unsupported = 0, other = 0;
  void count(int rc) {
    cases++;
    if (rc == PQG_OK) ok++;
    else if (rc == PQG_ERR_INVALID_ARG) invalid++;
    else if (rc == PQG_ERR_UNSUPPORTED) unsupported++;
    else other++;
  }
};

// columns 0, 1: repeated INT64 / BYTE_ARRAY; 2: flat INT32; 3: flat DOUBLE
static const int32_t TYPES[4] = {PQG_INT64, PQG_BYTE_ARRAY, PQG_INT32, PQG_DOUBLE};
static const uint64_t LITS[4] = {5, 3ull << 32, 7, 0x4000000000000000ull};
static const uint8_t BYTES[4] = {'a', 'b', 'c', 'd'};

struct Tree {
  std::vector<pqg_filter_node> n;
  int leaf(int op, int col, uint32_t flags = 0) {
    pqg_filter_node nd{};
    nd.op = op;
    nd.column = col;
    nd.left = nd.right = -1;
    nd.flags = flags;
    nd.literal_begin = (uint32_t)col;
    nd.n_literals = (flags & PQG_FILTER_NULL_LITERAL) ? 0 : 1;
    n.push_back(nd);
    return (int)n.size() - 1;
  }
  int node(int op, int l, int r = -1) {
    pqg_filter_node nd{};
    nd.op = op;
    nd.column = -1;
    nd.left = l;
    nd.right = r;
    n.push_back(nd);
    return (int)n.size() - 1;
  }
  int contains(int col, int op = PQG_FILTER_EQ) { return node(PQG_FILTER_CONTAINS, leaf(op, col)); }
};

// pqg_filter_create over an exactly-sized heap copy of the node table
static int create(Tally& t, const std::vector<pqg_filter_node>& nodes, int* node = nullptr, pqg_filter** keep = nullptr) {
  pqg_filter_node* in = (pqg_filter_node*)malloc(sizeof(pqg_filter_node) * (nodes.empty() ? 1 : nodes.size()));
  if (!nodes.empty()) memcpy(in, nodes.data(), sizeof(pqg_filter_node) * nodes.size());
  int32_t* types = (int32_t*)malloc(sizeof(TYPES));
  memcpy(types, TYPES, sizeof(TYPES));
  uint64_t* lits = (uint64_t*)malloc(sizeof(LITS));
  memcpy(lits, LITS, sizeof(LITS));
  uint8_t* bytes = (uint8_t*)malloc(4);
  memcpy(bytes, BYTES, 4);
  pqg_filter* f = nullptr;
  pqg_status st;
  const int rc = pqg_filter_create(in, (int)nodes.size(), types, 4, lits, 4, bytes, 4, &f, &st);
  t.count(rc);
  if ((rc == PQG_OK) != (f != nullptr) || st.code != rc) t.other++;
  if (rc == PQG_OK) {
    pqg_filter_node out[PQG_FILTER_MAX_NODES];
    const int n = pqg_filter_program(f, out, PQG_FILTER_MAX_NODES);
    if (n <= 0 || n > PQG_FILTER_MAX_NODES) t.other++;
    for (int i = 0; i < n && i < PQG_FILTER_MAX_NODES; i++)
      if (out[i].op == PQG_FILTER_NOT || (out[i].op == PQG_FILTER_CONTAINS && (out[i].left < 0 || out[i].left >= i || out[i].right != -1)))
        t.other++;
  }
  if (node) *node = st.value_index;
  if (keep) *keep = f;
  else if (f) pqg_filter_destroy(f);
  free(in);
  free(types);
  free(lits);
  free(bytes);
  return rc;
}

struct Bound {
  std::vector<pqg_filter_record_column> cols;
  std::vector<pqg_filter_dictionary> dicts;
  uint64_t n_rows = 1000;
};

static Bound make_columns(bool with_dicts) {
  Bound b;
  for (int i = 0; i < 4; i++) {
    pqg_filter_record_column c{};
    const bool rep = i < 2;
    c.col.physical_type = TYPES[i];
    c.col.max_def = rep ? 2 + i : i - 2;
    c.col.values = dev(8 * (uint64_t)i);
    c.col.binary_data = (const uint8_t*)dev(8 * (uint64_t)i + 1);
    c.col.def_levels = c.col.max_def ? (const uint8_t*)dev(8 * (uint64_t)i + 2) : nullptr;
    c.col.n_values = rep ? 2500 : b.n_rows;
    c.max_rep = rep ? 1 + i : 0;
    c.rep_levels = rep ? (const uint8_t*)dev(8 * (uint64_t)i + 3) : nullptr;
    c.n_slots = rep ? 3000 + 5000 * (uint64_t)i : b.n_rows;
    b.cols.push_back(c);
    pqg_filter_dictionary d{};
    if (with_dicts && i != 3) {
      d.values = dev(8 * (uint64_t)i + 4);
      d.binary_data = (const uint8_t*)dev(8 * (uint64_t)i + 5);
      d.n_entries = 100u * (uint32_t)(i + 1);
    }
    b.dicts.push_back(d);
  }
  return b;
}

// filter_bind_records through exactly-sized heap copies of both tables; an accepted one is checked for consistency
static int bind(Tally& t, const pqg_filter* filter, const Bound& b, bool with_dicts, int n_cols) {
  pqg_filter_record_column* in = (pqg_filter_record_column*)malloc(sizeof(pqg_filter_record_column) * b.cols.size());
  memcpy(in, b.cols.data(), sizeof(pqg_filter_record_column) * b.cols.size());
  pqg_filter_dictionary* din = nullptr;
  if (with_dicts) {
    din = (pqg_filter_dictionary*)malloc(sizeof(pqg_filter_dictionary) * b.dicts.size());
    memcpy(din, b.dicts.data(), sizeof(pqg_filter_dictionary) * b.dicts.size());
  }
  pqg::FilterCols* fc = (pqg::FilterCols*)malloc(sizeof(pqg::FilterCols));
  pqg::FilterRecDev* rd = (pqg::FilterRecDev*)malloc(sizeof(pqg::FilterRecDev));
  bool any = false;
  const int rc = pqg::filter_bind_records(filter, in, din, n_cols, b.n_rows, fc, &rd->dt, &any, &rd->rt);
  t.count(rc);
  if (rc == PQG_OK) {
    const pqg::FilterRecTab& rt = rd->rt;
    uint32_t n_contains = 0;
    for (const pqg_filter_node& nd : filter->program) n_contains += nd.op == PQG_FILTER_CONTAINS;
    if (fc->n_slots != filter->slot_column.size() || rt.n_leaves != n_contains || rt.n_rep > fc->n_slots ||
        rt.bitmap_words != (b.n_rows + 4095) / 4096 * 64)
      t.other++;
    uint64_t largest = 0;
    for (uint32_t ri = 0; ri < rt.n_rep; ri++) {
      const uint32_t s = rt.rep_slot[ri];
      if (s >= fc->n_slots) { t.other++; continue; }
      const pqg_filter_record_column& c = b.cols[(size_t)fc->c[s].column];
      if (fc->c[s].null_idx != pqg::FILTER_NULL_IDX_REPEATED || rt.rl[ri] != c.rep_levels || rt.n_slots[ri] != c.n_slots ||
          c.max_rep <= 0)
        t.other++;
      largest = c.n_slots > largest ? c.n_slots : largest;
    }
    if (rt.max_slots != largest) t.other++;
    for (uint32_t ni = 0; ni < fc->n_nullable; ni++)
      if (fc->null_slot[ni] >= fc->n_slots || fc->c[fc->null_slot[ni]].null_idx != (int32_t)ni) t.other++;
    for (uint32_t li = 0; li < rt.n_leaves; li++) {
      const uint32_t leaf = rt.leaf_node[li];
      if (leaf >= filter->program.size() || filter->program[leaf].op > PQG_FILTER_NOTIN) { t.other++; continue; }
      if (rt.leaf_rep[li] != pqg::FILTER_NO_LEAF &&
          (rt.leaf_rep[li] >= rt.n_rep || fc->c[rt.rep_slot[rt.leaf_rep[li]]].column != filter->program[leaf].column))
        t.other++;
    }
    // every contains leaf of a present column stands in exactly one group, with leaves of its column only
    uint32_t grouped[PQG_FILTER_MAX_NODES] = {};
    if (rt.n_groups > rt.n_leaves) t.other++;
    for (uint32_t g = 0; g < rt.n_groups && g < PQG_FILTER_MAX_NODES; g++) {
      if (rt.group_n[g] < 1 || rt.group_n[g] > pqg::FILTER_CONTAINS_GROUP || rt.group_rep[g] >= rt.n_rep) { t.other++; continue; }
      for (uint32_t k = 0; k < rt.group_n[g]; k++) {
        const uint32_t li = rt.group_leaf[g][k];
        if (li >= rt.n_leaves || rt.leaf_rep[li] != rt.group_rep[g]) t.other++;
        else grouped[li]++;
      }
    }
    for (uint32_t li = 0; li < rt.n_leaves; li++)
      if (grouped[li] != (rt.leaf_rep[li] != pqg::FILTER_NO_LEAF ? 1u : 0u)) t.other++;
    for (size_t i = 0; i < filter->program.size(); i++) {
      const bool is_contains = filter->program[i].op == PQG_FILTER_CONTAINS;
      if ((rt.node_leaf[i] != pqg::FILTER_NO_LEAF) != is_contains) t.other++;
      if (is_contains && rt.leaf_node[rt.node_leaf[i]] != (uint8_t)filter->program[i].left) t.other++;
    }
  } else if (rc != PQG_ERR_INVALID_ARG) {
    t.other++;
  }
  free(in);
  free(din);
  free(fc);
  free(rd);
  return rc;
}

int main(int argc, char** argv) {
  const long n_mut = argc > 1 ? atol(argv[1]) : 1000;
  Tally t;
  int bad = 0, node = -1;

  // ---- part 1: pqg_filter_create -----------------------------------------------------------------------
  std::vector<Tree> valid(6);
  valid[0].contains(0);
  { Tree& g = valid[1]; g.node(PQG_FILTER_AND, g.contains(0), g.contains(0, PQG_FILTER_NOTIN)); }
  { Tree& g = valid[2]; g.node(PQG_FILTER_OR, g.leaf(PQG_FILTER_EQ, 2), g.contains(1, PQG_FILTER_LT)); }
  { Tree& g = valid[3]; const int a = g.node(PQG_FILTER_AND, g.leaf(PQG_FILTER_GT, 3), g.contains(0)); g.node(PQG_FILTER_AND, a, g.contains(1)); }
  { Tree& g = valid[4]; const int a = g.node(PQG_FILTER_NOT, g.leaf(PQG_FILTER_LT, 2)); g.node(PQG_FILTER_OR, a, g.contains(0)); }
  {  // the largest tree: 21 contains on one column or-ed in a chain (62 nodes)
    Tree& g = valid[5];
    int acc = g.contains(0);
    for (int i = 1; i < 21; i++) acc = g.node(PQG_FILTER_OR, acc, g.contains(0, i % 8));
  }
  for (const Tree& g : valid) bad += create(t, g.n) != PQG_OK;
  if (bad) {
    fprintf(stderr, "%d valid predicates were refused\n", bad);
    return 1;
  }
  {  // the listed refusals, with the node each names
    auto expect = [&](const Tree& g, int code, int at) {
      int where = -2;
      const int rc = create(t, g.n, &where);
      if (rc != code || where != at) {
        fprintf(stderr, "refusal %ld: code %d node %d, expected %d at %d\n", t.cases, rc, where, code, at);
        bad++;
      }
    };
    { Tree g; g.node(PQG_FILTER_CONTAINS, -1); expect(g, PQG_ERR_INVALID_ARG, 0); }
    { Tree g; const int a = g.leaf(PQG_FILTER_EQ, 0), b = g.leaf(PQG_FILTER_EQ, 0); g.node(PQG_FILTER_CONTAINS, a, b); expect(g, PQG_ERR_INVALID_ARG, 2); }
    { Tree g; g.contains(0); g.n[1].flags = PQG_FILTER_UNSIGNED; expect(g, PQG_ERR_INVALID_ARG, 1); }
    { Tree g; g.contains(0); g.n[1].n_literals = 1; expect(g, PQG_ERR_INVALID_ARG, 1); }
    { Tree g; g.node(PQG_FILTER_CONTAINS, g.node(PQG_FILTER_AND, g.leaf(PQG_FILTER_EQ, 0), g.leaf(PQG_FILTER_EQ, 0))); expect(g, PQG_ERR_INVALID_ARG, 3); }
    { Tree g; g.node(PQG_FILTER_CONTAINS, g.contains(0)); expect(g, PQG_ERR_INVALID_ARG, 2); }
    { Tree g; g.node(PQG_FILTER_CONTAINS, g.leaf(PQG_FILTER_EQ, 0, PQG_FILTER_NULL_LITERAL)); expect(g, PQG_ERR_INVALID_ARG, 1); }
    { Tree g; g.node(PQG_FILTER_CONTAINS, g.leaf(PQG_FILTER_NOTIN, 0, PQG_FILTER_NULL_LITERAL)); expect(g, PQG_ERR_INVALID_ARG, 1); }
    { Tree g; g.node(PQG_FILTER_NOT, g.contains(0)); expect(g, PQG_ERR_UNSUPPORTED, 1); }
    { Tree g; g.node(PQG_FILTER_NOT, g.node(PQG_FILTER_NOT, g.contains(0))); expect(g, PQG_ERR_UNSUPPORTED, 1); }
    { Tree g; const int c1 = g.contains(0); const int inner = g.node(PQG_FILTER_NOT, g.contains(0)); g.node(PQG_FILTER_NOT, g.node(PQG_FILTER_AND, c1, inner)); expect(g, PQG_ERR_UNSUPPORTED, 3); }
    { Tree g; const int c = g.contains(0); g.node(PQG_FILTER_AND, c, g.node(PQG_FILTER_AND, g.leaf(PQG_FILTER_EQ, 2), g.leaf(PQG_FILTER_EQ, 3))); expect(g, PQG_ERR_UNSUPPORTED, 5); }
    { Tree g; const int a = g.node(PQG_FILTER_AND, g.leaf(PQG_FILTER_EQ, 2), g.leaf(PQG_FILTER_EQ, 3)); g.node(PQG_FILTER_AND, a, g.contains(0)); expect(g, PQG_OK, -1); }
    { Tree g; g.node(PQG_FILTER_OR, g.contains(0), g.contains(1)); expect(g, PQG_ERR_INVALID_ARG, 4); }
    {  // the early return: a leaf on the left leaves the refusal on the right unexamined
      Tree g;
      const int l = g.leaf(PQG_FILTER_EQ, 2);
      g.node(PQG_FILTER_AND, l, g.node(PQG_FILTER_OR, g.contains(0), g.contains(1)));
      expect(g, PQG_OK, -1);
    }
    {  // 4096 nested not() above a contains: the deepest walk the node limit admits
      Tree g;
      int acc = g.contains(0);
      for (int i = 0; i < 4094; i++) acc = g.node(PQG_FILTER_NOT, acc);
      expect(g, PQG_ERR_UNSUPPORTED, 1);
    }
    if (bad) {
      fprintf(stderr, "%d listed creation refusals came out differently\n", bad);
      return 1;
    }
  }
  for (const Tree& base : valid)
    for (long m = 0; m < n_mut; m++) {
      std::vector<pqg_filter_node> nodes = base.n;
      const uint64_t r = rnd();
      uint8_t* raw = (uint8_t*)nodes.data();
      const size_t bytes = sizeof(pqg_filter_node) * nodes.size();
      if (r % 4 == 0) {  // a field set to a small value: ops, children and columns near their valid ranges
        int32_t* f = (int32_t*)raw + rnd() % (bytes / 4);
        *f = (int32_t)(rnd() % 16) - 2;
      } else {
        for (int k = 0; k < 1 + (int)((r >> 2) % 3); k++) raw[rnd() % bytes] ^= (uint8_t)(1u << (rnd() % 8));
      }
      if ((r >> 16) % 8 == 0) {  // and a not() above the root: LogicalInverter meets the contains nodes
        Tree top;
        top.node(PQG_FILTER_NOT, (int)nodes.size() - 1);
        nodes.push_back(top.n[0]);
      }
      create(t, nodes);
    }

  // ---- part 2: filter_bind_records ---------------------------------------------------------------------
  std::vector<pqg_filter*> filters;
  for (size_t i = 0; i < 5; i++) {
    pqg_filter* f = nullptr;
    create(t, valid[i].n, nullptr, &f);
    filters.push_back(f);
  }
  {  // a plain flat predicate: filter_bind_records is filter_bind
    Tree g;
    g.node(PQG_FILTER_AND, g.leaf(PQG_FILTER_EQ, 2), g.leaf(PQG_FILTER_LT, 3));
    pqg_filter* f = nullptr;
    create(t, g.n, nullptr, &f);
    filters.push_back(f);
  }
  const Bound plain = make_columns(false), with_dicts = make_columns(true);
  for (pqg_filter* f : filters) {
    bad += bind(t, f, plain, false, 4) != PQG_OK;
    bad += bind(t, f, with_dicts, true, 4) != PQG_OK;
  }
  {  // filter_bind refuses a filter with a contains node
    pqg::FilterCols fc;
    std::vector<pqg_filter_column> flat(4);
    for (int i = 0; i < 4; i++) flat[(size_t)i] = plain.cols[(size_t)i].col;
    bad += pqg::filter_bind(filters[0], flat.data(), nullptr, 4, plain.n_rows, &fc, nullptr, nullptr) != PQG_ERR_INVALID_ARG;
    bad += pqg::filter_bind(filters[5], flat.data(), nullptr, 4, plain.n_rows, &fc, nullptr, nullptr) != PQG_OK;
  }
  if (bad) {
    fprintf(stderr, "%d valid bindings came out differently\n", bad);
    return 1;
  }
  {  // the refusals the header lists; filters[3] names columns 3 (flat), 0 and 1 (contains)
    pqg_filter* f = filters[3];
    auto with = [&](auto&& edit, bool dicts = false) {
      Bound b = dicts ? with_dicts : plain;
      edit(b);
      return bind(t, f, b, dicts, 4);
    };
    const int inv = PQG_ERR_INVALID_ARG;
    bad += with([](Bound& b) { b.cols[0].max_rep = 0; b.cols[0].rep_levels = nullptr; b.cols[0].n_slots = b.n_rows; }) != inv;  // contains on a flat column
    bad += with([](Bound& b) { b.cols[3].max_rep = 1; b.cols[3].col.max_def = 2; b.cols[3].rep_levels = (const uint8_t*)dev(99); b.cols[3].col.def_levels = (const uint8_t*)dev(98); }) != inv;  // a plain leaf on a repeated column
    bad += with([](Bound& b) { b.cols[0].max_rep = 255; }) != inv;
    bad += with([](Bound& b) { b.cols[0].max_rep = -1; }) != inv;
    bad += with([](Bound& b) { b.cols[1].reserved = 1; }) != inv;
    bad += with([](Bound& b) { b.cols[3].reserved = 1; }) != inv;
    bad += with([](Bound& b) { b.cols[0].col.max_def = 0; }) != inv;  // a repeated node adds a definition level
    bad += with([](Bound& b) { b.cols[0].rep_levels = nullptr; }) != inv;
    bad += with([](Bound& b) { b.cols[0].n_slots = b.n_rows - 1; }) != inv;
    bad += with([](Bound& b) { b.cols[3].rep_levels = (const uint8_t*)dev(99); }) != inv;
    bad += with([](Bound& b) { b.cols[3].n_slots = b.n_rows + 1; }) != inv;
    bad += with([](Bound& b) { b.cols[0].col.physical_type = PQG_INT32; }) != inv;
    bad += with([](Bound& b) { b.cols[0].col.max_def = 255; }) != inv;
    bad += with([](Bound& b) { b.cols[0].col.values = nullptr; }) != inv;
    bad += with([](Bound& b) { b.cols[1].col.binary_data = nullptr; }) != inv;
    bad += with([](Bound& b) { b.cols[3].col.max_def = 0; b.cols[3].col.def_levels = nullptr; }) != PQG_OK;
    bad += with([](Bound& b) { b.cols[3].col.max_def = 0; b.cols[3].col.def_levels = nullptr; b.cols[3].col.n_values = b.n_rows - 1; }) != inv;  // required: a value per row
    bad += with([](Bound& b) { b.dicts[0].reserved = 1; }, true) != inv;
    bad += with([](Bound& b) { b.cols[0].col.values = (const uint8_t*)b.cols[0].col.values + 2; }, true) != inv;  // misaligned ids
    bad += with([](Bound& b) { b.dicts[1].binary_data = nullptr; }, true) != inv;
    bad += with([](Bound& b) { b.cols[0].col.def_levels = nullptr; }, true) != inv;  // a dictionary on a missing column
    // a missing column is exempt from the structural rules and the leaf rules
    bad += with([](Bound& b) { b.cols[0].col.def_levels = nullptr; b.cols[0].rep_levels = nullptr; b.cols[0].n_slots = 0; b.cols[0].reserved = 9; b.cols[0].max_rep = 300; }) != PQG_OK;
    bad += with([](Bound& b) { b.cols[1].col.def_levels = nullptr; b.cols[1].max_rep = 0; }) != PQG_OK;
    // a column the predicate does not name is not looked at
    bad += with([](Bound& b) { b.cols[2].max_rep = 300; b.cols[2].reserved = 1; b.cols[2].col.physical_type = 77; }) != PQG_OK;
    bad += bind(t, f, plain, false, 3) != inv;  // not the filter's column count
    bad += bind(t, nullptr, plain, false, 4) != inv;
    if (bad) {
      fprintf(stderr, "%d listed binding refusals came out differently\n", bad);
      return 1;
    }
  }
  for (pqg_filter* f : filters)
    for (long m = 0; m < n_mut; m++) {
      Bound b = with_dicts;
      const uint64_t r = rnd();
      uint8_t* raw = (r & 1) ? (uint8_t*)b.cols.data() : (uint8_t*)b.dicts.data();
      const size_t bytes = (r & 1) ? sizeof(pqg_filter_record_column) * b.cols.size() : sizeof(pqg_filter_dictionary) * b.dicts.size();
      for (int k = 0; k < 1 + (int)((r >> 1) % 3); k++) raw[rnd() % bytes] ^= (uint8_t)(1u << (rnd() % 8));
      if ((r >> 8) % 8 == 0) b.n_rows = rnd() >> (rnd() % 64);
      bind(t, f, b, (r >> 12) % 4 != 0, 4);
    }
  for (pqg_filter* f : filters) pqg_filter_destroy(f);
  printf("cases=%ld ok=%ld invalid=%ld unsupported=%ld\n", t.cases, t.ok, t.invalid, t.unsupported);
  return t.other ? 1 : 0;
}
