/*
 * filter_sanitize.cpp — the record filter's host half (csrc/pqgpu_filter_host.cpp: validation of a
 * predicate table, LogicalInverseRewriter, literal keys, the device image) under AddressSanitizer +
 * UndefinedBehaviorSanitizer, without HIP. Built by tests/test_filter_sanitize.py with
 * -fsanitize=address,undefined -fno-sanitize-recover=all, so any finding aborts the run.
 *
 * usage: filter_sanitize <mutations per base table>
 * Valid tables (every op and type, sets above and below the binary-search size, BYTE_ARRAY literals,
 * nested not()) must be accepted; deterministic mutations of them (flipped bits, negative indices,
 * huge counts, zeroed fields, other column types, truncated tables, literal cells that point past
 * the bytes) must be accepted or refused with PQG_ERR_INVALID_ARG / PQG_ERR_UNSUPPORTED. Every table
 * handed to the library is an exactly-sized heap allocation, so a read one byte past it is caught.
 * Prints: cases=<n> ok=<n> invalid=<n> unsupported=<n>; exit status 1 on any other outcome.
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pqgpu.h"

struct Table {
  std::vector<pqg_filter_node> nodes;
  std::vector<int32_t> types;
  std::vector<uint64_t> literals;
  std::vector<uint8_t> bytes;
};

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {  // xorshift64*
  g_state ^= g_state >> 12;
  g_state ^= g_state << 25;
  g_state ^= g_state >> 27;
  return g_state * 0x2545F4914F6CDD1Dull;
}

static int leaf(Table& t, int op, int column, std::vector<uint64_t> lits, uint32_t flags = 0) {
  pqg_filter_node n{};
  n.op = op;
  n.column = column;
  n.left = n.right = -1;
  n.flags = flags;
  n.literal_begin = (uint32_t)t.literals.size();
  n.n_literals = (uint32_t)lits.size();
  t.literals.insert(t.literals.end(), lits.begin(), lits.end());
  t.nodes.push_back(n);
  return (int)t.nodes.size() - 1;
}
static int inner(Table& t, int op, int l, int r = -1) {
  pqg_filter_node n{};
  n.op = op;
  n.column = -1;
  n.left = l;
  n.right = r;
  t.nodes.push_back(n);
  return (int)t.nodes.size() - 1;
}
static uint64_t str(Table& t, const char* s, size_t len) {
  const uint64_t cell = (uint64_t)t.bytes.size() | ((uint64_t)len << 32);
  t.bytes.insert(t.bytes.end(), (const uint8_t*)s, (const uint8_t*)s + len);
  return cell;
}

static const int32_t kTypes[] = {PQG_BOOLEAN, PQG_INT32, PQG_INT64, PQG_FLOAT, PQG_DOUBLE, PQG_BYTE_ARRAY};

static std::vector<Table> base_tables() {
  std::vector<Table> out;
  {  // every comparison on every fixed-width type, joined by and / or / not
    Table t;
    t.types.assign(kTypes, kTypes + 6);
    int root = -1;
    for (int c = 0; c < 5; c++)
      for (int op = PQG_FILTER_EQ; op <= PQG_FILTER_GTEQ; op++) {
        if (c == 0 && op >= PQG_FILTER_LT) continue;
        int l = leaf(t, op, c, {0xFFFFFFFF80000000ull + (uint64_t)op}, (c == 1 || c == 2) && (op & 1) ? PQG_FILTER_UNSIGNED : 0);
        if (op == PQG_FILTER_GT) l = inner(t, PQG_FILTER_NOT, l);
        root = root < 0 ? l : inner(t, (op & 1) ? PQG_FILTER_AND : PQG_FILTER_OR, root, l);
      }
    root = inner(t, PQG_FILTER_NOT, inner(t, PQG_FILTER_NOT, inner(t, PQG_FILTER_NOT, root)));
    out.push_back(t);
  }
  {  // sets: 1, 8, 9 and 300 members, a null member, doubles with NaNs and both zeros
    Table t;
    t.types.assign(kTypes, kTypes + 6);
    std::vector<uint64_t> big;
    for (int i = 0; i < 300; i++) big.push_back(rnd());
    const int a = leaf(t, PQG_FILTER_IN, 2, big, PQG_FILTER_UNSIGNED);
    const int b = leaf(t, PQG_FILTER_NOTIN, 4, {0ull, 0x8000000000000000ull, 0x7FF8000000000000ull, 0xFFF8000000000123ull,
                                                0x7FF0000000000000ull, 0xFFF0000000000000ull, 1ull, 2ull, 3ull});
    const int c = leaf(t, PQG_FILTER_IN, 1, {7, 8, 9, 10, 11, 12, 13, 14});
    const int d = leaf(t, PQG_FILTER_NOTIN, 3, {0x7FC00000u}, PQG_FILTER_NULL_LITERAL);
    const int e = leaf(t, PQG_FILTER_EQ, 0, {}, PQG_FILTER_NULL_LITERAL);
    inner(t, PQG_FILTER_OR, inner(t, PQG_FILTER_AND, a, inner(t, PQG_FILTER_NOT, b)), inner(t, PQG_FILTER_AND, c, inner(t, PQG_FILTER_OR, d, e)));
    out.push_back(t);
  }
  {  // BYTE_ARRAY: comparisons and sets, empty strings, prefixes, high bytes
    Table t;
    t.types.assign(kTypes, kTypes + 6);
    std::vector<uint64_t> set;
    const char* words[] = {"", "a", "ab", "abc", "ab\x80", "\x80", "\xff\xff", "b", "abcdefgh", "abcdefghi", "zz", "z"};
    for (const char* w : words) set.push_back(str(t, w, strlen(w)));
    const int a = leaf(t, PQG_FILTER_IN, 5, set);
    const int b = leaf(t, PQG_FILTER_LT, 5, {str(t, "ab", 2)});
    const int c = leaf(t, PQG_FILTER_NOTEQ, 5, {str(t, "", 0)});
    const int d = leaf(t, PQG_FILTER_NOTIN, 5, {set[1], set[4]});
    inner(t, PQG_FILTER_NOT, inner(t, PQG_FILTER_AND, inner(t, PQG_FILTER_OR, a, b), inner(t, PQG_FILTER_OR, c, d)));
    out.push_back(t);
  }
  return out;
}

// Hand the table to the library in exactly-sized heap blocks.
static int run(const Table& t, int n_nodes, int n_cols, int n_literals, uint64_t n_bytes, int counts[3]) {
  // malloc(0) is a valid pointer no byte of which may be touched
  pqg_filter_node* nodes = (pqg_filter_node*)malloc(t.nodes.size() * sizeof(pqg_filter_node));
  int32_t* types = (int32_t*)malloc(t.types.size() * sizeof(int32_t));
  uint64_t* lits = (uint64_t*)malloc(t.literals.size() * sizeof(uint64_t));
  uint8_t* bytes = (uint8_t*)malloc(t.bytes.size());
  if (!t.nodes.empty()) memcpy(nodes, t.nodes.data(), t.nodes.size() * sizeof(pqg_filter_node));
  if (!t.types.empty()) memcpy(types, t.types.data(), t.types.size() * sizeof(int32_t));
  if (!t.literals.empty()) memcpy(lits, t.literals.data(), t.literals.size() * sizeof(uint64_t));
  if (!t.bytes.empty()) memcpy(bytes, t.bytes.data(), t.bytes.size());
  pqg_filter* f = nullptr;
  pqg_status st;
  const int rc = pqg_filter_create(nodes, n_nodes, types, n_cols, lits, n_literals, bytes, n_bytes, &f, &st);
  free(nodes);
  free(types);
  free(lits);
  free(bytes);  // the filter keeps its own copies: it must not touch the caller's tables from here on
  int bad = 0;
  if (rc == PQG_OK) {
    counts[0]++;
    if (!f) bad = 1;
    const int n = pqg_filter_program(f, nullptr, 0);
    if (n <= 0 || n > PQG_FILTER_MAX_NODES) bad = 1;
    for (int cap : {0, 1, n, PQG_FILTER_MAX_NODES}) {
      pqg_filter_node* out = (pqg_filter_node*)malloc((size_t)cap * sizeof(pqg_filter_node));
      if (pqg_filter_program(f, out, cap) != n) bad = 1;
      for (int i = 0; i < cap && i < n; i++)
        if (out[i].op == PQG_FILTER_NOT || out[i].left >= i || out[i].right >= i) bad = 1;
      free(out);
    }
    pqg_filter_destroy(f);
  } else if (rc == PQG_ERR_INVALID_ARG || rc == PQG_ERR_UNSUPPORTED) {
    counts[rc]++;
    if (f || st.code != rc) bad = 1;
  } else {
    bad = 1;
  }
  if (bad) fprintf(stderr, "unexpected outcome: rc=%d\n", rc);
  return bad;
}

static uint64_t weird() {
  static const uint64_t v[] = {0, 1, 0xFFFFFFFFull, 0x7FFFFFFFull, 0x80000000ull, 0xFFFFFFFFFFFFFFFFull,
                               0x8000000000000000ull, 64, 65, 4096, 4097, 16384, 16385};
  return v[rnd() % (sizeof(v) / sizeof(v[0]))];
}

int main(int argc, char** argv) {
  const int per_base = argc > 1 ? atoi(argv[1]) : 2000;
  int counts[3] = {0, 0, 0}, cases = 0, bad = 0;
  for (const Table& base : base_tables()) {
    int before = counts[0];
    bad |= run(base, (int)base.nodes.size(), (int)base.types.size(), (int)base.literals.size(), base.bytes.size(), counts);
    cases++;
    if (counts[0] != before + 1) {
      fprintf(stderr, "a valid table was refused\n");
      bad = 1;
    }
    for (int m = 0; m < per_base; m++, cases++) {
      Table t = base;
      int n_nodes = (int)t.nodes.size(), n_cols = (int)t.types.size(), n_lit = (int)t.literals.size();
      uint64_t n_bytes = t.bytes.size();
      for (int k = (int)(rnd() % 3); k >= 0; k--) {
        const int kind = (int)(rnd() % 9);
        if (kind <= 3) {  // a node field: flipped bit, weird value
          uint32_t* w = (uint32_t*)&t.nodes[rnd() % t.nodes.size()];
          uint32_t& field = w[rnd() % 8];
          if (kind == 0) field ^= 1u << (rnd() % 32);
          else if (kind == 1) field = (uint32_t)weird();
          else if (kind == 2) field = (uint32_t)-(int32_t)(rnd() % 5);
          else field = (uint32_t)(rnd() % (2 * t.nodes.size()));
        } else if (kind == 4 && !t.types.empty()) {  // another column type (8 and -1 are not types)
          t.types[rnd() % t.types.size()] = (int32_t)(rnd() % 10) - 1;
        } else if (kind == 5 && !t.literals.empty()) {  // a literal cell: BYTE_ARRAY cells now point anywhere
          uint64_t& c = t.literals[rnd() % t.literals.size()];
          c = (rnd() & 1) ? weird() | (weird() << 32) : c ^ (1ull << (rnd() % 64));
        } else if (kind == 6) {  // truncated tables (the sizes told to the library shrink with them)
          switch (rnd() % 4) {
            case 0: n_nodes = (int)(rnd() % (t.nodes.size() + 1)); t.nodes.resize((size_t)n_nodes); break;
            case 1: n_lit = (int)(rnd() % (t.literals.size() + 1)); t.literals.resize((size_t)n_lit); break;
            case 2: n_bytes = rnd() % (t.bytes.size() + 1); t.bytes.resize((size_t)n_bytes); break;
            default: n_cols = (int)(rnd() % (t.types.size() + 1)); t.types.resize((size_t)n_cols); break;
          }
          if (t.nodes.empty()) break;
        } else if (kind == 7) {  // negative table sizes
          switch (rnd() % 3) {
            case 0: n_nodes = -(int)(rnd() % 3); break;
            case 1: n_lit = -1 - (int)(rnd() % 3); break;
            default: n_cols = -1 - (int)(rnd() % 3); break;
          }
        } else {  // many literals / literal bytes, inside and over the limits
          const size_t grow = (size_t)weird() & 0x7FFF;
          if (rnd() & 1) {
            t.literals.resize(t.literals.size() + grow, 5);
            n_lit = (int)t.literals.size();
          } else {
            t.bytes.resize(t.bytes.size() + grow, 'x');
            n_bytes = t.bytes.size();
          }
        }
      }
      bad |= run(t, n_nodes, n_cols, n_lit, n_bytes, counts);
    }
  }
  printf("cases=%d ok=%d invalid=%d unsupported=%d\n", cases, counts[0], counts[1], counts[2]);
  return bad ? 1 : 0;
}
