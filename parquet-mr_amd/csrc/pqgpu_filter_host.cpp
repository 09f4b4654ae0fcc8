// pqgpu_filter_host.cpp — host half of the record filter (include/pqgpu.h, "record filter"):
// validation of a predicate table, LogicalInverseRewriter and ContainsRewriter's refusals, literal keys
// and the device image, and the binding of a run's columns and dictionaries to the program's slots
// (pqg::filter_bind, pqg::filter_bind_records).
// Plain C++ with no HIP in it, so that it also builds alone under the sanitizers
// (tests/c/filter_sanitize.cpp, tests/c/filter_dict_sanitize.cpp, tests/c/filter_records_sanitize.cpp,
// tests/c/filter_typed_sanitize.cpp).
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <new>

#include "pqgpu_filter.h"

namespace {

constexpr int kMaxInputNodes = 4096;  // nodes before the rewrite (NOT nodes disappear in it)

int fail(pqg_status* st, int code, int node, const char* msg) {
  if (st) {
    st->code = code;
    st->page = -1;
    st->value_index = node;
    snprintf(st->message, sizeof(st->message), "%s", msg);
  }
  return code;
}

bool is_leaf(int op) { return op >= PQG_FILTER_EQ && op <= PQG_FILTER_NOTIN; }

int inverse(int op) {
  switch (op) {
    case PQG_FILTER_EQ: return PQG_FILTER_NOTEQ;
    case PQG_FILTER_NOTEQ: return PQG_FILTER_EQ;
    case PQG_FILTER_LT: return PQG_FILTER_GTEQ;
    case PQG_FILTER_GTEQ: return PQG_FILTER_LT;
    case PQG_FILTER_LTEQ: return PQG_FILTER_GT;
    case PQG_FILTER_GT: return PQG_FILTER_LTEQ;
    case PQG_FILTER_IN: return PQG_FILTER_NOTIN;
    case PQG_FILTER_NOTIN: return PQG_FILTER_IN;
    case PQG_FILTER_AND: return PQG_FILTER_OR;
    case PQG_FILTER_OR: return PQG_FILTER_AND;
    default: return op;
  }
}

// Binary.lexicographicCompare (PrimitiveComparator.java:196-207): unsigned bytes, then length.
int compare_bytes(const uint8_t* a, uint32_t na, const uint8_t* b, uint32_t nb) {
  const uint32_t n = na < nb ? na : nb;
  const int c = n ? memcmp(a, b, n) : 0;
  if (c) return c < 0 ? -1 : 1;
  return na < nb ? -1 : (na > nb ? 1 : 0);
}

// BINARY_AS_SIGNED_INTEGER_COMPARATOR (PrimitiveComparator.java:214-279): the signs (of the first byte; an
// empty value is non-negative), the longer side's extra leading bytes against the shorter side's sign
// padding, then the common tail as unsigned bytes.
int compare_signed(const uint8_t* a, uint32_t na, const uint8_t* b, uint32_t nb) {
  const bool neg_a = na > 0 && (a[0] & 0x80u), neg_b = nb > 0 && (b[0] & 0x80u);
  if (neg_a != neg_b) return neg_a ? -1 : 1;
  const int pad = neg_a ? 0xFF : 0;
  if (na < nb) {
    for (uint32_t i = 0; i < nb - na; i++)
      if (b[i] != pad) return b[i] > pad ? -1 : 1;
    b += nb - na;
  } else if (na > nb) {
    for (uint32_t i = 0; i < na - nb; i++)
      if (a[i] != pad) return a[i] > pad ? 1 : -1;
    a += na - nb;
  }
  const uint32_t n = na < nb ? na : nb;
  const int c = n ? memcmp(a, b, n) : 0;
  return c < 0 ? -1 : (c > 0 ? 1 : 0);
}

bool is_binary(int type) { return type == PQG_BYTE_ARRAY || type == PQG_INT96 || type == PQG_FIXED_LEN_BYTE_ARRAY; }

// Float16 key of a literal cell (two little-endian bytes; the length was checked)
int64_t float16_key(const uint8_t* lb, uint64_t cell) {
  const uint8_t* p = lb + (uint32_t)cell;
  return pqg::filter_key_float16((uint32_t)p[0] | ((uint32_t)p[1] << 8));
}

std::atomic<uint64_t> g_serial{1};

bool is_logical(int op) { return op == PQG_FILTER_AND || op == PQG_FILTER_OR; }

// The leftmost CONTAINS of the subtree at `i` in visiting order (left before right), -1 without one.
int first_contains(const pqg_filter_node* n, int i) {
  const int op = n[i].op;
  if (op == PQG_FILTER_CONTAINS) return i;
  if (is_leaf(op)) return -1;
  const int l = first_contains(n, n[i].left);
  if (l >= 0 || op == PQG_FILTER_NOT) return l;
  return first_contains(n, n[i].right);
}

// LogicalInverseRewriter on a tree with contains: not(p) is LogicalInverter.invert(rewrite(p)), and
// LogicalInverter.visit(Contains) throws (LogicalInverter.java:97-99). The walk is the rewriter's:
// operands first, left before right, so the innermost not() above a contains throws, at the first
// contains its inversion meets. Returns that node, -1 when nothing is refused.
int inverse_refusal(const pqg_filter_node* n, int i) {
  const int op = n[i].op;
  if (is_leaf(op) || op == PQG_FILTER_CONTAINS) return -1;
  const int l = inverse_refusal(n, n[i].left);
  if (l >= 0) return l;
  if (op == PQG_FILTER_NOT) return first_contains(n, n[i].left);
  return inverse_refusal(n, n[i].right);
}

// ContainsRewriter.visit(And) / visit(Or) (ContainsRewriter.java:100-168) on the NOT-free program, restated
// with its quirks: a side that is neither and / or nor a Contains returns the node as it is at once; the
// sides are visited left first; a left side that became a Contains needs a Contains on the right
// (UnsupportedOperationException), on the same column (ContainsComposedPredicate, IllegalArgumentException).
// Returns the column of the Contains node `i` rewrites to, -1 when it stays an and / or. *code != PQG_OK:
// refused at program node *bad.
int contains_rewrite(const std::vector<pqg_filter_node>& p, int i, int* code, int* bad) {
  int col[2] = {-1, -1};
  for (int k = 0; k < 2; k++) {
    const int c = k ? p[(size_t)i].right : p[(size_t)i].left;
    const int op = p[(size_t)c].op;
    if (is_logical(op)) {
      col[k] = contains_rewrite(p, c, code, bad);
      if (*code != PQG_OK) return -1;
    } else if (op == PQG_FILTER_CONTAINS) {
      col[k] = p[(size_t)p[(size_t)c].left].column;
    } else {
      return -1;
    }
  }
  if (col[0] < 0) return -1;
  if (col[1] < 0 || col[0] != col[1]) {
    *code = col[1] < 0 ? PQG_ERR_UNSUPPORTED : PQG_ERR_INVALID_ARG;
    *bad = i;
    return -1;
  }
  return col[0];
}

// The device image of the created filter `f` (FilterDevHeader ...). equals = false: the filter's own, every
// leaf under its column's comparator. equals = true: pqg_filter::rg_image, the form pqg_filter_row_groups runs.
void build_image(const pqg_filter* f, bool equals, std::vector<uint8_t>* out) {
  const uint8_t* lb = f->bytes.data();
  // the image's cells, leaf by leaf: one per literal, or three under FILTER_DEV_KEY128 (every literal of the
  // leaf fits 16 bytes once its redundant sign bytes are gone, and so does every value it can meet below the
  // byte-wise path) while cells and bytes together stay inside what the limits give an image
  std::vector<uint64_t> img_cells;
  std::vector<uint32_t> img_begin(f->program.size(), 0);
  std::vector<uint8_t> dev_flags(f->program.size(), 0);
  size_t spare = (8u * PQG_FILTER_MAX_LITERALS + PQG_FILTER_MAX_LITERAL_BYTES - 8u * f->cells.size() - f->bytes.size()) / 16u;
  std::vector<uint64_t> by_bytes;
  for (size_t i = 0; i < f->program.size(); i++) {
    const pqg_filter_node& nd = f->program[i];
    if (!is_leaf(nd.op)) continue;
    const pqg_filter_column_type& ct = f->columns[(size_t)nd.column];
    const int type = ct.physical_type;
    const uint64_t* raw = f->cells.data() + nd.literal_begin;
    img_begin[i] = (uint32_t)img_cells.size();
    if (equals && nd.op == PQG_FILTER_NOTIN && f->null_only[i]) dev_flags[i] |= pqg::FILTER_DEV_NULL_ONLY;
    const bool equality = nd.op == PQG_FILTER_EQ || nd.op == PQG_FILTER_NOTEQ || nd.op == PQG_FILTER_IN || nd.op == PQG_FILTER_NOTIN;
    if (equals && equality && is_binary(type) && ct.binary_order != PQG_FILTER_ORDER_UNSIGNED_BYTES) {
      // Binary.equals: the bytes and the length, under every comparator; the set was sorted by the comparator
      by_bytes.assign(raw, raw + nd.n_literals);
      if (nd.n_literals > pqg::FILTER_IN_LINEAR)
        std::sort(by_bytes.begin(), by_bytes.end(), [lb](uint64_t x, uint64_t y) {
          return compare_bytes(lb + (uint32_t)x, (uint32_t)(x >> 32), lb + (uint32_t)y, (uint32_t)(y >> 32)) < 0;
        });
      img_cells.insert(img_cells.end(), by_bytes.begin(), by_bytes.end());
    } else if (ct.binary_order == PQG_FILTER_ORDER_FLOAT16) {
      dev_flags[i] |= pqg::FILTER_DEV_FLOAT16;
      for (uint32_t k = 0; k < nd.n_literals; k++) img_cells.push_back((uint64_t)float16_key(lb, raw[k]));
    } else if (ct.binary_order == PQG_FILTER_ORDER_SIGNED_INTEGER) {
      dev_flags[i] |= pqg::FILTER_DEV_SIGNED;
      const uint32_t width = type == PQG_INT96 ? 12u : (uint32_t)ct.type_length;
      bool keys = nd.n_literals <= spare && (type == PQG_BYTE_ARRAY || width <= pqg::FILTER_KEY128_BYTES);
      int64_t hi;
      uint64_t lo;
      for (uint32_t k = 0; keys && k < nd.n_literals; k++)
        keys = pqg::filter_key128(lb + (uint32_t)raw[k], (uint32_t)(raw[k] >> 32), &hi, &lo);
      if (keys) {
        dev_flags[i] |= pqg::FILTER_DEV_KEY128;
        spare -= nd.n_literals;
      }
      for (uint32_t k = 0; k < nd.n_literals; k++) {
        img_cells.push_back(raw[k]);
        if (!keys) continue;
        (void)pqg::filter_key128(lb + (uint32_t)raw[k], (uint32_t)(raw[k] >> 32), &hi, &lo);
        img_cells.push_back((uint64_t)hi);
        img_cells.push_back(lo);
      }
    } else {
      for (uint32_t k = 0; k < nd.n_literals; k++)
        img_cells.push_back(is_binary(type) ? raw[k]
                                            : (uint64_t)pqg::filter_key(type, (nd.flags & PQG_FILTER_UNSIGNED) != 0, raw[k]));
    }
  }
  pqg::FilterDevHeader h{};
  h.n_nodes = (uint32_t)f->program.size();
  h.n_slots = (uint32_t)f->slot_column.size();
  h.n_cells = (uint32_t)img_cells.size();
  h.n_bytes = (uint32_t)f->bytes.size();
  h.cells_off = (uint32_t)(sizeof(h) + h.n_nodes * sizeof(pqg::FilterDevNode) + PQG_FILTER_MAX_NODES);
  h.bytes_off = h.cells_off + 8u * h.n_cells;
  h.image_bytes = h.bytes_off + (h.n_bytes + 7u) / 8u * 8u + 8u;
  out->assign(h.image_bytes, 0);
  uint8_t* img = out->data();
  uint8_t* order = img + sizeof(h) + h.n_nodes * sizeof(pqg::FilterDevNode);
  for (uint32_t s = 0; s < h.n_slots; s++)
    for (uint32_t i = 0; i < h.n_nodes; i++) {
      const pqg_filter_node& nd = f->program[i];
      if (is_leaf(nd.op) && nd.column == f->slot_column[s]) order[h.n_leaves++] = (uint8_t)i;
    }
  std::vector<char> contained(h.n_nodes, 0);
  for (const pqg_filter_node& nd : f->program)
    if (nd.op == PQG_FILTER_CONTAINS) contained[(size_t)nd.left] = 1;
  for (uint32_t i = 0; i < h.n_nodes; i++) {
    const pqg_filter_node& nd = f->program[i];
    pqg::FilterDevNode d{};
    d.op = (uint8_t)nd.op;
    d.flags = (uint8_t)(nd.flags | dev_flags[i] | (contained[i] ? pqg::FILTER_DEV_CONTAINED : 0u));
    if (is_leaf(nd.op)) {
      const pqg_filter_column_type& ct = f->columns[(size_t)nd.column];
      d.type = (uint8_t)ct.physical_type;
      d.slot = (uint8_t)(std::find(f->slot_column.begin(), f->slot_column.end(), nd.column) - f->slot_column.begin());
      d.n_lit = (uint16_t)nd.n_literals;
      d.lit_begin = img_begin[i];
      d.width = ct.physical_type == PQG_INT96 ? 12u : ct.physical_type == PQG_FIXED_LEN_BYTE_ARRAY ? (uint32_t)ct.type_length : 0u;
    } else {
      d.left = (uint8_t)nd.left;
      d.right = (uint8_t)(nd.right < 0 ? 0 : nd.right);
    }
    memcpy(img + sizeof(h) + i * sizeof(d), &d, sizeof(d));
  }
  if (h.n_cells) memcpy(img + h.cells_off, img_cells.data(), 8u * h.n_cells);
  if (h.n_bytes) memcpy(img + h.bytes_off, lb, h.n_bytes);
  memcpy(img, &h, sizeof(h));
}

// pqg_filter_create (`bare`: the columns came as plain physical types, INT96 / FLBA are refused) and
// pqg_filter_create_typed: one validation path.
int create_filter(const pqg_filter_node* nodes, int n_nodes, const pqg_filter_column_type* columns, int n_cols, bool bare,
                  const uint64_t* literals, int n_literals, const uint8_t* literal_bytes, uint64_t n_literal_bytes,
                  pqg_filter** out, pqg_status* st) {
  if (!nodes || n_nodes <= 0) return fail(st, PQG_ERR_INVALID_ARG, -1, "filter: no nodes");
  if (n_literals < 0 || (n_literals > 0 && !literals)) return fail(st, PQG_ERR_INVALID_ARG, -1, "filter: no literal table");
  if (n_literal_bytes > 0 && !literal_bytes) return fail(st, PQG_ERR_INVALID_ARG, -1, "filter: no literal bytes");
  if (n_nodes > kMaxInputNodes) return fail(st, PQG_ERR_UNSUPPORTED, -1, "filter: more than 4096 nodes");
  if (n_literals > PQG_FILTER_MAX_LITERALS) return fail(st, PQG_ERR_UNSUPPORTED, -1, "filter: more than 4096 literal cells");
  if (n_literal_bytes > PQG_FILTER_MAX_LITERAL_BYTES)
    return fail(st, PQG_ERR_UNSUPPORTED, -1, "filter: more than 16 KiB of literal bytes");

  // ---- validation -----------------------------------------------------------------
  std::vector<int> uses((size_t)n_nodes, 0);
  for (int i = 0; i < n_nodes; i++) {
    const pqg_filter_node& nd = nodes[i];
    if (nd.op < PQG_FILTER_EQ || nd.op > PQG_FILTER_CONTAINS) return fail(st, PQG_ERR_INVALID_ARG, i, "filter: unknown op");
    if (nd.flags & ~(uint32_t)(PQG_FILTER_NULL_LITERAL | PQG_FILTER_UNSIGNED))
      return fail(st, PQG_ERR_INVALID_ARG, i, "filter: unknown flags");
    if (!is_leaf(nd.op)) {
      const bool two = is_logical(nd.op);
      if (nd.left < 0 || nd.left >= i) return fail(st, PQG_ERR_INVALID_ARG, i, "filter: child index not below its parent");
      if (two ? (nd.right < 0 || nd.right >= i || nd.right == nd.left) : nd.right != -1)
        return fail(st, PQG_ERR_INVALID_ARG, i, "filter: child index not below its parent");
      uses[(size_t)nd.left]++;
      if (two) uses[(size_t)nd.right]++;
      if (nd.op == PQG_FILTER_CONTAINS) {
        // FilterApi.contains takes a SingleColumnFilterPredicate, without null among its values
        if (nd.flags || nd.n_literals) return fail(st, PQG_ERR_INVALID_ARG, i, "filter: contains with flags or literals of its own");
        if (!is_leaf(nodes[nd.left].op)) return fail(st, PQG_ERR_INVALID_ARG, i, "filter: contains of a node that is not a leaf");
        if (nodes[nd.left].flags & PQG_FILTER_NULL_LITERAL)
          return fail(st, PQG_ERR_INVALID_ARG, i, "filter: contains does not support null element values");
      }
      continue;
    }
    if (nd.left != -1 || nd.right != -1) return fail(st, PQG_ERR_INVALID_ARG, i, "filter: a leaf has children");
    if (nd.column < 0 || nd.column >= n_cols) return fail(st, PQG_ERR_INVALID_ARG, i, "filter: column out of range");
    const pqg_filter_column_type& ct = columns[nd.column];
    const int type = ct.physical_type;
    if (type < PQG_BOOLEAN || type > PQG_FIXED_LEN_BYTE_ARRAY) return fail(st, PQG_ERR_INVALID_ARG, i, "filter: unknown column type");
    if (bare && (type == PQG_INT96 || type == PQG_FIXED_LEN_BYTE_ARRAY))
      return fail(st, PQG_ERR_UNSUPPORTED, i, "filter: INT96 / FIXED_LEN_BYTE_ARRAY columns are not supported");
    const int order = ct.binary_order;
    if (order < PQG_FILTER_ORDER_UNSIGNED_BYTES || order > PQG_FILTER_ORDER_FLOAT16)
      return fail(st, PQG_ERR_INVALID_ARG, i, "filter: unknown binary order");
    if (!is_binary(type) && (ct.type_length || order))
      return fail(st, PQG_ERR_INVALID_ARG, i, "filter: type_length or binary_order on a column that is not binary");
    if (type == PQG_BYTE_ARRAY && ct.type_length) return fail(st, PQG_ERR_INVALID_ARG, i, "filter: type_length on a BYTE_ARRAY column");
    if (type == PQG_FIXED_LEN_BYTE_ARRAY && ct.type_length < 1)
      return fail(st, PQG_ERR_INVALID_ARG, i, "filter: FIXED_LEN_BYTE_ARRAY column without a type_length");
    if (type == PQG_INT96 && ct.type_length != 0 && ct.type_length != 12)
      return fail(st, PQG_ERR_INVALID_ARG, i, "filter: INT96 column with a type_length other than 12");
    if (type == PQG_INT96 && order != PQG_FILTER_ORDER_SIGNED_INTEGER)
      return fail(st, PQG_ERR_INVALID_ARG, i, "filter: INT96 compares as a signed integer only");
    if (order == PQG_FILTER_ORDER_FLOAT16 && (type != PQG_FIXED_LEN_BYTE_ARRAY || ct.type_length != 2))
      return fail(st, PQG_ERR_INVALID_ARG, i, "filter: FLOAT16 order on a column that is not FIXED_LEN_BYTE_ARRAY(2)");
    if ((nd.flags & PQG_FILTER_UNSIGNED) && type != PQG_INT32 && type != PQG_INT64)
      return fail(st, PQG_ERR_INVALID_ARG, i, "filter: unsigned order on a column that is not INT32 / INT64");
    if ((uint64_t)nd.literal_begin + nd.n_literals > (uint64_t)n_literals)
      return fail(st, PQG_ERR_INVALID_ARG, i, "filter: literal range past the table");
    const bool null_lit = (nd.flags & PQG_FILTER_NULL_LITERAL) != 0;
    const bool set = nd.op == PQG_FILTER_IN || nd.op == PQG_FILTER_NOTIN;
    const bool ineq = nd.op >= PQG_FILTER_LT && nd.op <= PQG_FILTER_GTEQ;
    if (ineq && type == PQG_BOOLEAN) return fail(st, PQG_ERR_INVALID_ARG, i, "filter: lt / ltEq / gt / gtEq on a BOOLEAN column");
    if (ineq && null_lit) return fail(st, PQG_ERR_INVALID_ARG, i, "filter: lt / ltEq / gt / gtEq against null");
    if (set ? (nd.n_literals == 0 && !null_lit) : nd.n_literals != (null_lit ? 0u : 1u))
      return fail(st, PQG_ERR_INVALID_ARG, i, "filter: wrong number of literals");
    if (is_binary(type))
      for (uint32_t k = 0; k < nd.n_literals; k++) {
        const uint64_t cell = literals[nd.literal_begin + k];
        if ((cell & 0xFFFFFFFFull) + (cell >> 32) > n_literal_bytes)
          return fail(st, PQG_ERR_INVALID_ARG, i, "filter: BYTE_ARRAY literal past the literal bytes");
        if (order == PQG_FILTER_ORDER_FLOAT16 && (cell >> 32) != 2)
          return fail(st, PQG_ERR_INVALID_ARG, i, "filter: FLOAT16 literal that is not 2 bytes long");
      }
  }
  for (int i = 0; i < n_nodes; i++)
    if (uses[(size_t)i] != (i == n_nodes - 1 ? 0 : 1))
      return fail(st, PQG_ERR_INVALID_ARG, i, "filter: not a tree with its root last");

  // ---- LogicalInverseRewriter -------------------------------------------------------
  // not(p) is invert(rewrite(p)); inverting twice is the identity on every node kind here, so a node
  // ends up inverted when an odd number of NOTs stand above it. A contains cannot be inverted at all.
  {
    const int bad = inverse_refusal(nodes, n_nodes - 1);
    if (bad >= 0) return fail(st, PQG_ERR_UNSUPPORTED, bad, "filter: not() above a contains (Contains not supported yet)");
  }
  std::vector<char> inv((size_t)n_nodes, 0);
  std::vector<int> remap((size_t)n_nodes, -1);
  for (int i = n_nodes - 1; i >= 0; i--) {
    const pqg_filter_node& nd = nodes[i];
    if (nd.op == PQG_FILTER_NOT) {
      inv[(size_t)nd.left] = !inv[(size_t)i];
    } else if (is_logical(nd.op)) {
      inv[(size_t)nd.left] = inv[(size_t)nd.right] = inv[(size_t)i];
    }
  }
  pqg_filter* f = new (std::nothrow) pqg_filter();
  if (!f) return fail(st, PQG_ERR_INVALID_ARG, -1, "filter: out of memory");
  f->serial = g_serial.fetch_add(1);
  f->columns.assign(columns, columns + n_cols);
  for (int c = 0; c < n_cols; c++) f->column_types.push_back(columns[c].physical_type);
  if (n_literal_bytes) f->bytes.assign(literal_bytes, literal_bytes + n_literal_bytes);
  std::vector<int> orig;  // program node -> input node
  for (int i = 0; i < n_nodes; i++) {
    pqg_filter_node nd = nodes[i];
    if (nd.op == PQG_FILTER_NOT) {
      remap[(size_t)i] = remap[(size_t)nd.left];
      continue;
    }
    orig.push_back(i);
    if (inv[(size_t)i]) nd.op = inverse(nd.op);
    nd.reserved = 0;
    f->null_only.push_back(is_leaf(nd.op) && (nd.flags & PQG_FILTER_NULL_LITERAL) && nd.n_literals == 0);
    if (is_leaf(nd.op)) {
      const uint32_t begin = (uint32_t)f->cells.size();
      for (uint32_t k = 0; k < nd.n_literals; k++) f->cells.push_back(literals[nd.literal_begin + k]);
      nd.literal_begin = begin;
      if (nd.flags & PQG_FILTER_NULL_LITERAL) {  // the set's other members are ignored
        f->cells.resize(begin);
        nd.n_literals = 0;
      }
    } else {
      nd.left = remap[(size_t)nd.left];
      nd.right = is_logical(nd.op) ? remap[(size_t)nd.right] : -1;
      nd.column = -1;
      if (nd.op == PQG_FILTER_CONTAINS) f->has_contains = true;
      nd.literal_begin = nd.n_literals = 0;
    }
    remap[(size_t)i] = (int)f->program.size();
    f->program.push_back(nd);
  }
  if (f->program.size() > PQG_FILTER_MAX_NODES || f->cells.size() > PQG_FILTER_MAX_LITERALS) {
    delete f;
    return fail(st, PQG_ERR_UNSUPPORTED, -1, "filter: more than 64 nodes or 4096 literal cells after the rewrite");
  }

  // ---- ContainsRewriter's refusals (its merging is an optimisation: and / or stay as they are) ----
  if (f->has_contains && is_logical(f->program.back().op)) {
    int code = PQG_OK, bad = -1;
    (void)contains_rewrite(f->program, (int)f->program.size() - 1, &code, &bad);
    if (code != PQG_OK) {
      const int node = orig[(size_t)bad];
      delete f;
      return fail(st, code, node,
                  code == PQG_ERR_UNSUPPORTED ? "filter: Contains predicates cannot be composed with non-Contains predicates"
                                              : "filter: composed Contains predicates must reference the same column");
    }
  }

  // ---- sets for the binary search, slots, device image ----------------------------------
  const uint8_t* lb = f->bytes.data();
  for (pqg_filter_node& nd : f->program) {
    if (!is_leaf(nd.op)) continue;
    const int type = f->column_types[(size_t)nd.column];
    const int order = f->columns[(size_t)nd.column].binary_order;
    if (order || type == PQG_INT96 || type == PQG_FIXED_LEN_BYTE_ARRAY) f->binary_paths = true;
    if (nd.n_literals > pqg::FILTER_IN_LINEAR) {
      uint64_t* b = f->cells.data() + nd.literal_begin;
      const bool uns = (nd.flags & PQG_FILTER_UNSIGNED) != 0;
      if (order == PQG_FILTER_ORDER_SIGNED_INTEGER)
        std::sort(b, b + nd.n_literals, [lb](uint64_t x, uint64_t y) {
          return compare_signed(lb + (uint32_t)x, (uint32_t)(x >> 32), lb + (uint32_t)y, (uint32_t)(y >> 32)) < 0;
        });
      else if (order == PQG_FILTER_ORDER_FLOAT16)
        std::sort(b, b + nd.n_literals, [lb](uint64_t x, uint64_t y) { return float16_key(lb, x) < float16_key(lb, y); });
      else if (is_binary(type))
        std::sort(b, b + nd.n_literals, [lb](uint64_t x, uint64_t y) {
          return compare_bytes(lb + (uint32_t)x, (uint32_t)(x >> 32), lb + (uint32_t)y, (uint32_t)(y >> 32)) < 0;
        });
      else
        std::sort(b, b + nd.n_literals, [type, uns](uint64_t x, uint64_t y) {
          return pqg::filter_key(type, uns, x) < pqg::filter_key(type, uns, y);
        });
    }
    if (std::find(f->slot_column.begin(), f->slot_column.end(), nd.column) == f->slot_column.end())
      f->slot_column.push_back(nd.column);
  }
  build_image(f, false, &f->image);
  build_image(f, true, &f->rg_image);
  *out = f;
  if (st) fail(st, PQG_OK, -1, "");
  return PQG_OK;
}

}  // namespace

extern "C" {

int pqg_filter_create(const pqg_filter_node* nodes, int n_nodes, const int32_t* column_types, int n_cols,
                      const uint64_t* literals, int n_literals, const uint8_t* literal_bytes,
                      uint64_t n_literal_bytes, pqg_filter** out, pqg_status* st) {
  if (!out) return fail(st, PQG_ERR_INVALID_ARG, -1, "filter: out is null");
  *out = nullptr;
  if (n_cols < 0 || (n_cols > 0 && !column_types)) return fail(st, PQG_ERR_INVALID_ARG, -1, "filter: no column types");
  std::vector<pqg_filter_column_type> columns((size_t)n_cols);
  for (int c = 0; c < n_cols; c++) columns[(size_t)c] = pqg_filter_column_type{column_types[c], 0, 0, 0};
  return create_filter(nodes, n_nodes, columns.data(), n_cols, true, literals, n_literals, literal_bytes, n_literal_bytes,
                       out, st);
}

int pqg_filter_create_typed(const pqg_filter_node* nodes, int n_nodes, const pqg_filter_column_type* columns, int n_cols,
                            const uint64_t* literals, int n_literals, const uint8_t* literal_bytes,
                            uint64_t n_literal_bytes, pqg_filter** out, pqg_status* st) {
  if (!out) return fail(st, PQG_ERR_INVALID_ARG, -1, "filter: out is null");
  *out = nullptr;
  if (n_cols < 0 || (n_cols > 0 && !columns)) return fail(st, PQG_ERR_INVALID_ARG, -1, "filter: no column types");
  for (int c = 0; c < n_cols; c++)
    if (columns[c].reserved) return fail(st, PQG_ERR_INVALID_ARG, c, "filter: reserved field of a column type is not 0");
  return create_filter(nodes, n_nodes, columns, n_cols, false, literals, n_literals, literal_bytes, n_literal_bytes, out, st);
}

int pqg_filter_program(const pqg_filter* filter, pqg_filter_node* out, int cap) {
  if (!filter) return -1;
  const int n = (int)filter->program.size();
  if (out)
    for (int i = 0; i < n && i < cap; i++) out[i] = filter->program[(size_t)i];
  return n;
}

int pqg_filter_destroy(pqg_filter* filter) {
  delete filter;
  return PQG_OK;
}

}  // extern "C"

namespace pqg {

// filter_bind and filter_bind_records: column `col` is at cols + col * stride (a pqg_filter_column, or the one
// that begins a pqg_filter_record_column); repeated[col] != 0 (records only): a present repeated column.
static int bind_slots(const pqg_filter* filter, const uint8_t* cols_base, size_t stride, const uint8_t* repeated,
                      const pqg_filter_dictionary* dicts, uint64_t n_rows, FilterCols* fc, FilterDictTab* dt,
                      bool* any_dict) {
  if (any_dict) *any_dict = false;
  memset(fc, 0, sizeof(*fc));
  if (dt) {
    memset(dt, 0, sizeof(*dt));
    for (uint64_t& o : dt->leaf_off) o = FILTER_NO_TABLE;
  }
  bool any = false;
  fc->n_slots = (uint32_t)filter->slot_column.size();
  for (uint32_t s = 0; s < fc->n_slots; s++) {
    const int col = filter->slot_column[s];
    const pqg_filter_column& c = *(const pqg_filter_column*)(cols_base + (size_t)col * stride);
    if (c.physical_type != filter->column_types[(size_t)col] || c.max_def < 0 || c.max_def > 254) return PQG_ERR_INVALID_ARG;
    const bool missing = c.max_def > 0 && !c.def_levels;
    const pqg_filter_dictionary* dc = dicts && dicts[col].values ? &dicts[col] : nullptr;
    if (dicts && dicts[col].reserved) return PQG_ERR_INVALID_ARG;
    if (dc) {
      // the column holds uint32 ids; its values are the dictionary's
      if (missing) return PQG_ERR_INVALID_ARG;
      if (c.physical_type == PQG_BYTE_ARRAY && !dc->binary_data) return PQG_ERR_INVALID_ARG;
      if (((uintptr_t)c.values & 3u) || (!c.values && c.n_values)) return PQG_ERR_INVALID_ARG;
      if (c.max_def == 0 && c.n_values < n_rows) return PQG_ERR_INVALID_ARG;
      FilterDictSlot& ds = dt->slot[s];
      ds.values = dc->values;
      ds.binary = dc->binary_data;
      ds.n_entries = dc->n_entries;
      ds.is_dict = 1;
      any = true;
    } else if (!missing) {
      if (!c.values && (c.n_values || c.physical_type == PQG_BYTE_ARRAY)) return PQG_ERR_INVALID_ARG;
      if (c.physical_type == PQG_BYTE_ARRAY && !c.binary_data) return PQG_ERR_INVALID_ARG;
      if (c.max_def == 0 && c.n_values < n_rows) return PQG_ERR_INVALID_ARG;  // a required column has a value per row
    }
    FilterColDev& d = fc->c[s];
    d.values = c.values;
    d.binary = dc ? nullptr : c.binary_data;
    d.dl = c.max_def > 0 ? c.def_levels : nullptr;
    d.n_values = c.n_values;
    d.type = c.physical_type;
    d.max_def = c.max_def;
    d.column = col;
    d.null_idx = -1;
    if (repeated && repeated[col]) {
      d.null_idx = FILTER_NULL_IDX_REPEATED;
    } else if (d.dl) {
      d.null_idx = (int32_t)fc->n_nullable;
      fc->null_slot[fc->n_nullable++] = (uint8_t)s;
    }
  }
  if (any) {
    // a leaf without a null literal on a dictionary slot: one bit per entry, whole words (a null-literal leaf
    // depends on validity only)
    for (size_t i = 0; i < filter->program.size(); i++) {
      const pqg_filter_node& nd = filter->program[i];
      if (!is_leaf(nd.op) || (nd.flags & PQG_FILTER_NULL_LITERAL)) continue;
      const size_t s = (size_t)(std::find(filter->slot_column.begin(), filter->slot_column.end(), nd.column) -
                                filter->slot_column.begin());
      if (s >= fc->n_slots || !dt->slot[s].is_dict) continue;
      const uint64_t words = ((uint64_t)dt->slot[s].n_entries + 63) / 64;
      dt->leaf_off[i] = dt->table_words;
      dt->table_words += words;
      if (words) dt->table_leaf[dt->n_tables++] = (uint8_t)i;
      if (words > dt->max_words) dt->max_words = words;
    }
    dt->in_lds = dt->table_words && dt->table_words * 8 <= PQG_FILTER_DICT_LDS_BYTES;
  }
  if (any_dict) *any_dict = any;
  return PQG_OK;
}

int filter_bind(const pqg_filter* filter, const pqg_filter_column* cols, const pqg_filter_dictionary* dicts, int n_cols,
                uint64_t n_rows, FilterCols* fc, FilterDictTab* dt, bool* any_dict) {
  if (any_dict) *any_dict = false;
  if (!filter || !fc || n_cols != (int)filter->column_types.size() || (n_cols > 0 && !cols)) return PQG_ERR_INVALID_ARG;
  if (dicts && !dt) return PQG_ERR_INVALID_ARG;
  // no repetition levels here: the reference refuses contains on a column with maxRepetitionLevel == 0
  if (filter->has_contains) return PQG_ERR_INVALID_ARG;
  return bind_slots(filter, (const uint8_t*)cols, sizeof(pqg_filter_column), nullptr, dicts, n_rows, fc, dt, any_dict);
}

int filter_bind_records(const pqg_filter* filter, const pqg_filter_record_column* cols, const pqg_filter_dictionary* dicts,
                        int n_cols, uint64_t n_rows, FilterCols* fc, FilterDictTab* dt, bool* any_dict, FilterRecTab* rt) {
  if (any_dict) *any_dict = false;
  if (!filter || !fc || !dt || !rt || n_cols != (int)filter->column_types.size() || (n_cols > 0 && !cols))
    return PQG_ERR_INVALID_ARG;
  memset(rt, 0, sizeof(*rt));
  memset(rt->leaf_rep, FILTER_NO_LEAF, sizeof(rt->leaf_rep));
  memset(rt->node_leaf, FILTER_NO_LEAF, sizeof(rt->node_leaf));
  // the structural rules of pqg_take_record_column, on the columns the predicate names (the others are not
  // read); a missing column is exempt
  std::vector<uint8_t> repeated((size_t)n_cols, 0), missing((size_t)n_cols, 0);
  for (const int col : filter->slot_column) {
    const pqg_filter_record_column& r = cols[col];
    if (r.col.max_def > 0 && !r.col.def_levels) {
      missing[(size_t)col] = 1;
      continue;
    }
    if (r.max_rep < 0 || r.max_rep > 254 || r.reserved) return PQG_ERR_INVALID_ARG;
    if (r.max_rep > 0) {
      // a repeated node always adds a definition level
      if (r.col.max_def == 0 || !r.rep_levels || r.n_slots < n_rows) return PQG_ERR_INVALID_ARG;
      repeated[(size_t)col] = 1;
    } else if (r.rep_levels || r.n_slots != n_rows) {
      return PQG_ERR_INVALID_ARG;
    }
  }
  // contains needs maxRepetitionLevel > 0, every other predicate a flat column
  // (SchemaCompatibilityValidator.java:177-214)
  std::vector<char> contained(filter->program.size(), 0);
  for (const pqg_filter_node& nd : filter->program)
    if (nd.op == PQG_FILTER_CONTAINS) contained[(size_t)nd.left] = 1;
  for (size_t i = 0; i < filter->program.size(); i++) {
    const pqg_filter_node& nd = filter->program[i];
    if (!is_leaf(nd.op) || missing[(size_t)nd.column]) continue;
    if ((contained[i] != 0) != (repeated[(size_t)nd.column] != 0)) return PQG_ERR_INVALID_ARG;
  }
  const int rc = bind_slots(filter, (const uint8_t*)cols, sizeof(pqg_filter_record_column), repeated.data(), dicts, n_rows,
                            fc, dt, any_dict);
  if (rc != PQG_OK) return rc;
  rt->bitmap_words = (n_rows + PQG_FILTER_TILE_ROWS - 1) / PQG_FILTER_TILE_ROWS * (PQG_FILTER_TILE_ROWS / 64);
  uint8_t slot_rep[PQG_FILTER_MAX_NODES];
  for (uint32_t s = 0; s < fc->n_slots; s++) {
    const int col = filter->slot_column[s];
    slot_rep[s] = FILTER_NO_LEAF;
    if (!repeated[(size_t)col]) continue;
    slot_rep[s] = (uint8_t)rt->n_rep;
    rt->rep_slot[rt->n_rep] = (uint8_t)s;
    rt->rl[rt->n_rep] = cols[col].rep_levels;
    rt->n_slots[rt->n_rep] = cols[col].n_slots;
    if (cols[col].n_slots > rt->max_slots) rt->max_slots = cols[col].n_slots;
    rt->n_rep++;
  }
  for (size_t i = 0; i < filter->program.size(); i++) {
    const pqg_filter_node& nd = filter->program[i];
    if (nd.op != PQG_FILTER_CONTAINS) continue;
    const int col = filter->program[(size_t)nd.left].column;
    const size_t s = (size_t)(std::find(filter->slot_column.begin(), filter->slot_column.end(), col) - filter->slot_column.begin());
    rt->node_leaf[i] = (uint8_t)rt->n_leaves;
    rt->leaf_node[rt->n_leaves] = (uint8_t)nd.left;
    rt->leaf_rep[rt->n_leaves] = slot_rep[s];
    rt->n_leaves++;
  }
  // a column's contains leaves share its loads: groups of up to FILTER_CONTAINS_GROUP
  for (uint32_t ri = 0; ri < rt->n_rep; ri++) {
    uint32_t in_group = FILTER_CONTAINS_GROUP;  // the next leaf opens a group
    for (uint32_t li = 0; li < rt->n_leaves; li++) {
      if (rt->leaf_rep[li] != ri) continue;
      if (in_group == FILTER_CONTAINS_GROUP) {
        rt->group_rep[rt->n_groups] = (uint8_t)ri;
        rt->n_groups++;
        in_group = 0;
      }
      rt->group_leaf[rt->n_groups - 1][in_group++] = (uint8_t)li;
      rt->group_n[rt->n_groups - 1] = (uint8_t)in_group;
    }
  }
  return PQG_OK;
}

}  // namespace pqg
