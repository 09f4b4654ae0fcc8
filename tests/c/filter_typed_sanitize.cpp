/*
 * filter_typed_sanitize.cpp — pqg_filter_create_typed (csrc/pqgpu_filter_host.cpp: the validation of column
 * widths and binary orders, the literal keys of the signed-integer and FLOAT16 comparators, the sorting of
 * large sets and the device image) under AddressSanitizer + UndefinedBehaviorSanitizer, without HIP. Built by
 * tests/test_filter_typed_sanitize.py with -fsanitize=address,undefined -fno-sanitize-recover=all, so any
 * finding aborts the run.
 *
 * usage: filter_typed_sanitize <mutations per base case> <random literal pairs>
 * Valid typed tables (FLBA of widths 1 .. 40, INT96, BYTE_ARRAY; the three orders; all eight ops; literals of
 * 0 .. 40 bytes; sets of 3 and of 12 with comparator-equal members) must be accepted, every refusal the header
 * lists must come back as PQG_ERR_INVALID_ARG, and deterministic bit flips in the node, column-type and
 * literal tables must be accepted or refused, never crashed on. Every table is an exactly-sized heap block.
 * The host's literal keys are checked against a plain byte-loop comparator (restated here from
 * PrimitiveComparator.java:214-279 and Float16.java:108-134) on random pairs: the keys the image holds must
 * order every pair as the byte loops do, a literal without keys must not fit 16 bytes, and a large set must
 * come out sorted. Accepted typed filters are also bound to columns (pqg::filter_bind).
 * Prints: cases=<n> ok=<n> invalid=<n> pairs=<n>; exit status 1 on any other outcome.
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

// ---- the byte loops -------------------------------------------------------------------------------
static int with_padding(int length, const uint8_t* b, int p, int padding) {
  for (int i = p, n = p + length; i < n; ++i) {
    const int r = (int)b[i] - padding;
    if (r != 0) return r;
  }
  return 0;
}
static int ref_signed(const uint8_t* b1, int l1, const uint8_t* b2, int l2) {
  int p1 = 0, p2 = 0;
  const bool neg1 = l1 > 0 && (int8_t)b1[0] < 0, neg2 = l2 > 0 && (int8_t)b2[0] < 0;
  if (neg1 != neg2) return neg1 ? -1 : 1;
  int result = 0;
  if (l1 < l2) {
    const int d = l2 - l1;
    result = -with_padding(d, b2, p2, neg1 ? 0xFF : 0);
    p2 += d;
  } else if (l1 > l2) {
    const int d = l1 - l2;
    result = with_padding(d, b1, p1, neg2 ? 0xFF : 0);
    p1 += d;
  }
  if (result == 0)
    for (int i = 0; i < (l1 < l2 ? l1 : l2); ++i) {
      result = (int)b1[p1 + i] - (int)b2[p2 + i];
      if (result != 0) break;
    }
  return result < 0 ? -1 : (result > 0 ? 1 : 0);
}
static int ref_float16(const uint8_t* a, const uint8_t* b) {
  const int16_t x = (int16_t)(a[0] | (a[1] << 8)), y = (int16_t)(b[0] | (b[1] << 8));
  const bool xn = (x & 0x7fff) > 0x7c00, yn = (y & 0x7fff) > 0x7c00;
  if (!xn && !yn) {
    const int first = (x & 0x8000) != 0 ? 0x8000 - (x & 0xffff) : x & 0xffff;
    const int second = (y & 0x8000) != 0 ? 0x8000 - (y & 0xffff) : y & 0xffff;
    if (first < second) return -1;
    if (first > second) return 1;
  }
  const int16_t xb = xn ? (int16_t)0x7e00 : x, yb = yn ? (int16_t)0x7e00 : y;
  return xb == yb ? 0 : (xb < yb ? -1 : 1);
}

// ---- one creation through exactly-sized heap copies -------------------------------------------------
struct Tally {
  long cases = 0, ok = 0, invalid = 0, other = 0, pairs = 0;
};
static Tally T;

template <class V>
static V* heap(const std::vector<V>& v) {
  if (v.empty()) return nullptr;
  V* p = (V*)malloc(sizeof(V) * v.size());
  memcpy(p, v.data(), sizeof(V) * v.size());
  return p;
}

struct Tables {
  std::vector<pqg_filter_node> nodes;
  std::vector<pqg_filter_column_type> cols;
  std::vector<uint64_t> lits;
  std::vector<uint8_t> bytes;
};

static int create(const Tables& t, pqg_filter** out) {
  pqg_filter_node* n = heap(t.nodes);
  pqg_filter_column_type* c = heap(t.cols);
  uint64_t* l = heap(t.lits);
  uint8_t* b = heap(t.bytes);
  pqg_status st;
  pqg_filter* f = nullptr;
  const int rc = pqg_filter_create_typed(n, (int)t.nodes.size(), c, (int)t.cols.size(), l, (int)t.lits.size(), b,
                                         t.bytes.size(), &f, &st);
  free(n);
  free(c);
  free(l);
  free(b);
  T.cases++;
  if (rc == PQG_OK && f) {
    T.ok++;
    const pqg::FilterDevHeader* h = (const pqg::FilterDevHeader*)f->image.data();
    if (f->image.size() != h->image_bytes || h->bytes_off + h->n_bytes > h->image_bytes ||
        h->cells_off + 8ull * h->n_cells > h->bytes_off ||
        8ull * h->n_cells + h->n_bytes > 8ull * PQG_FILTER_MAX_LITERALS + PQG_FILTER_MAX_LITERAL_BYTES)
      T.other++;
  } else if ((rc == PQG_ERR_INVALID_ARG || rc == PQG_ERR_UNSUPPORTED) && !f) {
    T.invalid++;
  } else {
    T.other++;
  }
  if (out) *out = f;
  else pqg_filter_destroy(f);
  return rc;
}

static pqg_filter_node leaf(int op, int column, uint32_t begin, uint32_t n, uint32_t flags = 0) {
  pqg_filter_node nd{};
  nd.op = op;
  nd.column = column;
  nd.left = nd.right = -1;
  nd.flags = flags;
  nd.literal_begin = begin;
  nd.n_literals = n;
  return nd;
}

// a leaf `op` on column 0 of the given type with the literals `lits` (byte strings)
static Tables one_leaf(pqg_filter_column_type ct, int op, const std::vector<std::vector<uint8_t>>& lits) {
  Tables t;
  t.cols.push_back(ct);
  for (const auto& l : lits) {
    t.lits.push_back((uint64_t)t.bytes.size() | ((uint64_t)l.size() << 32));
    t.bytes.insert(t.bytes.end(), l.begin(), l.end());
  }
  t.nodes.push_back(leaf(op, 0, 0, (uint32_t)lits.size()));
  return t;
}

static std::vector<uint8_t> random_bytes(uint32_t n) {
  std::vector<uint8_t> v(n);
  for (uint8_t& b : v) b = (uint8_t)rnd();
  // sign padding in front of about half of them, so that lengths differ while values collide
  if (n > 2 && (rnd() & 1)) {
    const uint32_t k = 1 + (uint32_t)(rnd() % (n - 1));
    const uint8_t pad = (rnd() & 1) ? 0xFF : 0;
    for (uint32_t i = 0; i < k; i++) v[i] = pad;
  }
  return v;
}

// the device node and cells of program node 0
static const pqg::FilterDevNode* dev_node(const pqg_filter* f) {
  return (const pqg::FilterDevNode*)(f->image.data() + sizeof(pqg::FilterDevHeader));
}
static const uint64_t* dev_cells(const pqg_filter* f) {
  return (const uint64_t*)(f->image.data() + ((const pqg::FilterDevHeader*)f->image.data())->cells_off);
}

int main(int argc, char** argv) {
  const long n_mut = argc > 1 ? atol(argv[1]) : 1000;
  const long n_pairs = argc > 2 ? atol(argv[2]) : 2000;
  const int U = PQG_FILTER_ORDER_UNSIGNED_BYTES, S = PQG_FILTER_ORDER_SIGNED_INTEGER, H = PQG_FILTER_ORDER_FLOAT16;
  const int FLBA = PQG_FIXED_LEN_BYTE_ARRAY;
  int bad = 0;

  // ---- valid tables: widths, orders, ops, literal lengths 0 .. 40 ----
  std::vector<Tables> bases;
  for (int width : {1, 2, 3, 5, 12, 16, 17, 20, 40})
    for (int order : {U, S})
      for (int op = PQG_FILTER_EQ; op <= PQG_FILTER_NOTIN; op++) {
        std::vector<std::vector<uint8_t>> lits;
        const int n = op >= PQG_FILTER_IN ? (width % 2 ? 3 : 12) : 1;
        for (int k = 0; k < n; k++) lits.push_back(random_bytes((uint32_t)((width + op + 7 * k) % 41)));
        if (n > 1) lits[1] = lits[0];  // comparator-equal members
        bases.push_back(one_leaf({FLBA, width, order, 0}, op, lits));
      }
  for (uint32_t len = 0; len <= 40; len++) {
    bases.push_back(one_leaf({PQG_INT96, (int)(len % 2) * 12, S, 0}, PQG_FILTER_LT, {random_bytes(len)}));
    bases.push_back(one_leaf({PQG_BYTE_ARRAY, 0, S, 0}, PQG_FILTER_GTEQ, {random_bytes(len)}));
    bases.push_back(one_leaf({FLBA, 16, S, 0}, PQG_FILTER_IN, {random_bytes(len), random_bytes(40 - len), {}}));
  }
  bases.push_back(one_leaf({FLBA, 2, H, 0}, PQG_FILTER_LT, {{0x00, 0x7c}}));
  {
    std::vector<std::vector<uint8_t>> lits;
    for (int k = 0; k < 12; k++) lits.push_back({(uint8_t)rnd(), (uint8_t)rnd()});
    bases.push_back(one_leaf({FLBA, 2, H, 0}, PQG_FILTER_NOTIN, lits));
  }
  for (const Tables& t : bases) bad += create(t, nullptr) != PQG_OK;
  if (bad) {
    fprintf(stderr, "%d valid typed tables were refused\n", bad);
    return 1;
  }

  // ---- the refusals the header lists ----
  {
    const std::vector<uint8_t> two = {1, 2};
    auto rc_of = [&](pqg_filter_column_type ct, uint32_t flags = 0, std::vector<uint8_t> lit = {1, 2}) {
      Tables t = one_leaf(ct, PQG_FILTER_EQ, {lit});
      t.nodes[0].flags = flags;
      return create(t, nullptr);
    };
    const int I = PQG_ERR_INVALID_ARG;
    bad += rc_of({FLBA, 4, U, 1}) != I;                      // reserved
    bad += rc_of({PQG_INT32, 4, 0, 0}) != I;                 // type_length on a non-binary type
    bad += rc_of({PQG_INT64, 0, S, 0}) != I;                 // order on a non-binary type
    bad += rc_of({PQG_BYTE_ARRAY, 1, U, 0}) != I;
    bad += rc_of({FLBA, 0, U, 0}) != I;
    bad += rc_of({FLBA, -5, S, 0}) != I;
    bad += rc_of({PQG_INT96, 8, S, 0}) != I;
    bad += rc_of({PQG_INT96, 0, U, 0}) != I;
    bad += rc_of({PQG_INT96, 12, H, 0}) != I;
    bad += rc_of({FLBA, 4, H, 0}) != I;
    bad += rc_of({PQG_BYTE_ARRAY, 0, H, 0}) != I;
    bad += rc_of({FLBA, 2, H, 0}, 0, {1}) != I;              // a FLOAT16 literal of 1 byte
    bad += rc_of({FLBA, 2, H, 0}, 0, {1, 2, 3}) != I;
    bad += rc_of({FLBA, 2, H, 0}, 0, {}) != I;
    bad += rc_of({FLBA, 4, U, 0}, PQG_FILTER_UNSIGNED) != I;
    bad += rc_of({PQG_INT96, 0, S, 0}, PQG_FILTER_UNSIGNED) != I;
    bad += rc_of({PQG_BYTE_ARRAY, 0, S, 0}, PQG_FILTER_UNSIGNED) != I;
    bad += rc_of({FLBA, 4, 3, 0}) != I;
    bad += rc_of({FLBA, 4, -1, 0}) != I;
    bad += rc_of({FLBA, 2, H, 0}) != PQG_OK;
    bad += rc_of({FLBA, 0x7FFFFFFF, S, 0}) != PQG_OK;
    {  // the bare form keeps its refusal
      Tables t = one_leaf({FLBA, 0, 0, 0}, PQG_FILTER_EQ, {two});
      const int32_t type = FLBA;
      pqg_filter* f = nullptr;
      pqg_status st;
      bad += pqg_filter_create(t.nodes.data(), 1, &type, 1, t.lits.data(), 1, t.bytes.data(), 2, &f, &st) != PQG_ERR_UNSUPPORTED;
    }
    if (bad) {
      fprintf(stderr, "%d listed refusals came out differently\n", bad);
      return 1;
    }
  }

  // ---- the host's keys against the byte loops ----
  for (long i = 0; i < n_pairs; i++) {
    const uint32_t la = (uint32_t)(rnd() % 41), lb = (rnd() & 3) ? (uint32_t)(rnd() % 41) : la;
    std::vector<uint8_t> a = random_bytes(la), b = random_bytes(lb);
    if (la == lb && la && (rnd() & 1)) {  // near neighbours: equal but for one late byte
      b = a;
      b[la - 1 - (uint32_t)(rnd() % (la < 3 ? la : 3))] ^= (uint8_t)(1u << (rnd() % 8));
    }
    pqg_filter* f = nullptr;
    if (create(one_leaf({PQG_BYTE_ARRAY, 0, S, 0}, PQG_FILTER_IN, {a, b}), &f) != PQG_OK) return 1;
    const pqg::FilterDevNode nd = dev_node(f)[0];
    const uint64_t* c = dev_cells(f) + nd.lit_begin;
    const int want = ref_signed(a.data(), (int)la, b.data(), (int)lb);
    int64_t ha, hb;
    uint64_t loa, lob;
    const bool fa = pqg::filter_key128(a.data(), la, &ha, &loa), fb = pqg::filter_key128(b.data(), lb, &hb, &lob);
    if (!(nd.flags & pqg::FILTER_DEV_SIGNED) || ((nd.flags & pqg::FILTER_DEV_KEY128) != 0) != (fa && fb)) T.other++;
    if (nd.flags & pqg::FILTER_DEV_KEY128) {
      const int64_t h0 = (int64_t)c[1], h1 = (int64_t)c[4];
      const int got = h0 != h1 ? (h0 < h1 ? -1 : 1) : (c[2] > c[5]) - (c[2] < c[5]);
      if (got != want || c[0] != f->cells[0] || c[3] != f->cells[1]) T.other++;
    } else {
      // a side without a key holds more than 16 significant bytes: it lies outside every 16-byte value
      const std::vector<uint8_t>& w = fa ? b : a;
      const uint8_t lo[16] = {0x80}, hi[16] = {0x7F, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF};
      if (ref_signed(w.data(), (int)w.size(), lo, 16) >= 0 && ref_signed(w.data(), (int)w.size(), hi, 16) <= 0) T.other++;
    }
    pqg_filter_destroy(f);
    // FLOAT16
    const uint8_t x[2] = {(uint8_t)rnd(), (uint8_t)rnd()}, y[2] = {(uint8_t)rnd(), (uint8_t)((rnd() & 1) ? x[1] : rnd())};
    if (create(one_leaf({FLBA, 2, H, 0}, PQG_FILTER_IN, {{x[0], x[1]}, {y[0], y[1]}}), &f) != PQG_OK) return 1;
    const uint64_t* k = dev_cells(f) + dev_node(f)[0].lit_begin;
    const int64_t kx = (int64_t)k[0], ky = (int64_t)k[1];
    if (!(dev_node(f)[0].flags & pqg::FILTER_DEV_FLOAT16) || ((kx > ky) - (kx < ky)) != ref_float16(x, y)) T.other++;
    pqg_filter_destroy(f);
    T.pairs++;
  }
  // ---- large sets come out sorted by the leaf's comparator ----
  for (int round = 0; round < 50; round++) {
    std::vector<std::vector<uint8_t>> lits;
    const int n = 9 + (int)(rnd() % 30);
    for (int k = 0; k < n; k++) lits.push_back(random_bytes((uint32_t)(rnd() % 25)));
    lits[3] = lits[7];
    pqg_filter* f = nullptr;
    if (create(one_leaf({FLBA, round % 2 ? 16 : 20, S, 0}, PQG_FILTER_IN, lits), &f) != PQG_OK) return 1;
    const uint8_t* lb = f->bytes.data();
    for (int k = 0; k + 1 < n; k++) {
      const uint64_t p = f->cells[(size_t)k], q = f->cells[(size_t)k + 1];
      if (ref_signed(lb + (uint32_t)p, (int)(p >> 32), lb + (uint32_t)q, (int)(q >> 32)) > 0) T.other++;
    }
    // and the columns bind: the declared type only
    pqg_filter_column col{};
    col.physical_type = FLBA;
    col.values = (const void*)(uintptr_t)0x7000000001ull;  // any alignment
    col.n_values = 1000;
    pqg::FilterCols* fc = (pqg::FilterCols*)malloc(sizeof(pqg::FilterCols));
    if (pqg::filter_bind(f, &col, nullptr, 1, 1000, fc, nullptr, nullptr) != PQG_OK) T.other++;
    col.physical_type = PQG_BYTE_ARRAY;
    if (pqg::filter_bind(f, &col, nullptr, 1, 1000, fc, nullptr, nullptr) != PQG_ERR_INVALID_ARG) T.other++;
    free(fc);
    pqg_filter_destroy(f);
  }

  // ---- deterministic bit flips in the three tables ----
  for (size_t bi = 0; bi < bases.size(); bi += 7) {
    for (long m = 0; m < n_mut; m++) {
      Tables t = bases[bi];
      const uint64_t r = rnd();
      uint8_t* raw;
      size_t bytes;
      switch (r % 3) {
        case 0: raw = (uint8_t*)t.nodes.data(), bytes = sizeof(pqg_filter_node) * t.nodes.size(); break;
        case 1: raw = (uint8_t*)t.cols.data(), bytes = sizeof(pqg_filter_column_type) * t.cols.size(); break;
        default: raw = (uint8_t*)t.lits.data(), bytes = 8 * t.lits.size(); break;
      }
      for (int k = 0; k < 1 + (int)((r >> 2) % 3); k++) raw[rnd() % bytes] ^= (uint8_t)(1u << (rnd() % 8));
      create(t, nullptr);
    }
  }
  printf("cases=%ld ok=%ld invalid=%ld pairs=%ld\n", T.cases, T.ok, T.invalid, T.pairs);
  return T.other ? 1 : 0;
}
