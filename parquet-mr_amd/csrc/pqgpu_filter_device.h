// pqgpu_filter_device.h — device functions shared by the kernels that evaluate a filter program's leaves:
// pqgpu_filter.hip (rows, dictionary ids, list elements) and pqgpu_rowgroup.hip (the entries of many
// dictionaries). A lane's value of a column (load_value), the comparators of PrimitiveComparator over it
// (compare_cell), one leaf on one value (leaf_eval) and the staging of the program image in LDS.
#pragma once
#include "pqgpu_device.h"
#include "pqgpu_filter.h"

namespace pqg {

constexpr uint32_t FT_ROWS = PQG_FILTER_TILE_ROWS;
constexpr uint32_t FT_STEPS = FT_ROWS / 64;
static_assert(FT_STEPS == 64, "lane k keeps the word of step k: 64 steps per tile");
constexpr int FT_WPB = 4;       // tiles (waves) per workgroup
constexpr int FS_PER = 4;       // k_filter_scan: tiles per thread per round (1,024 per round)

__device__ __forceinline__ uint32_t lanes_below(uint64_t m) {  // set bits of m in lanes below this one
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}
__device__ __forceinline__ uint64_t rdl64(uint64_t v, uint32_t l) {
  return ((uint64_t)rdl((uint32_t)(v >> 32), l) << 32) | rdl((uint32_t)v, l);
}

// A lane's value of the column being evaluated: the comparator key of a fixed-width value, or where a
// BYTE_ARRAY value's bytes are.
struct LaneValue {
  int64_t key;
  uint64_t lo;           // FILTER_DEV_KEY128: the value is key (high, signed) : lo
  rsrc_t rs;             // binary types: the data from the wave's first value on (range-checked)
  uint32_t rel, len;     // the value's bytes are [rel, rel + len) of rs
  const uint8_t* slow;   // non-null: the value's bytes start here and do not fit rs (over 4 GiB away): plain loads
};

// 4 bytes of the value at byte p (p < len), little endian; bytes past the value are unspecified.
__device__ __forceinline__ uint32_t value_dword(const LaneValue& v, uint32_t p) {
  if (!v.slow) return ld4_any(v.rs, v.rel + p);
  uint32_t w = 0;
  for (uint32_t b = 0; b < 4 && p + b < v.len; b++) w |= (uint32_t)v.slow[p + b] << (8u * b);
  return w;
}

// Binary.lexicographicCompare of the lane's value with the literal at lit[0, llen) in LDS: unsigned bytes
// over min(len, llen), then the lengths.
__device__ __forceinline__ int compare_bytes(const LaneValue& v, const uint8_t* lit, uint32_t llen) {
  const uint32_t n = v.len < llen ? v.len : llen;
  for (uint32_t p = 0; p < n; p += 4) {
    uint32_t a = value_dword(v, p);
    uint32_t b = (uint32_t)lit[p] | ((uint32_t)lit[p + 1] << 8) | ((uint32_t)lit[p + 2] << 16) | ((uint32_t)lit[p + 3] << 24);
    const uint32_t rem = n - p;
    const uint32_t m = rem >= 4 ? 0xFFFFFFFFu : (1u << (8u * rem)) - 1u;
    a &= m;
    b &= m;
    if (a != b) return __builtin_bswap32(a) < __builtin_bswap32(b) ? -1 : 1;
  }
  return v.len < llen ? -1 : (v.len > llen ? 1 : 0);
}

__device__ __forceinline__ uint32_t lds_dword(const uint8_t* p) {  // any alignment; the image is padded behind its bytes
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

// Unsigned order of the value's bytes [pv, pv + n) against n bytes of the other side, of which other(p) gives
// 4 at p (little endian; bytes past n unspecified).
template <class F>
__device__ __forceinline__ int compare_span(const LaneValue& v, uint32_t pv, uint32_t n, F other) {
  for (uint32_t p = 0; p < n; p += 4) {
    uint32_t a = value_dword(v, pv + p), b = other(p);
    const uint32_t rem = n - p;
    const uint32_t m = rem >= 4 ? 0xFFFFFFFFu : (1u << (8u * rem)) - 1u;
    a &= m;
    b &= m;
    if (a != b) return __builtin_bswap32(a) < __builtin_bswap32(b) ? -1 : 1;
  }
  return 0;
}

// BINARY_AS_SIGNED_INTEGER_COMPARATOR (PrimitiveComparator.java:214-279) of the lane's value with the literal
// at lit[0, llen), byte-wise for any lengths: the signs (first bytes; an empty side is non-negative), the
// longer side's extra leading bytes against the shorter side's sign padding, the common tail unsigned.
__device__ __forceinline__ int compare_signed_bytes(const LaneValue& v, const uint8_t* lit, uint32_t llen) {
  const bool neg_v = v.len != 0 && (value_dword(v, 0) & 0x80u) != 0;
  const bool neg_l = llen != 0 && (lit[0] & 0x80u) != 0;
  if (neg_v != neg_l) return neg_v ? -1 : 1;
  const uint32_t pad = neg_v ? 0xFFFFFFFFu : 0u;
  uint32_t pv = 0;
  if (v.len < llen) {
    const uint32_t d = llen - v.len;
    for (uint32_t p = 0; p < d; p += 4) {
      const uint32_t m = d - p >= 4 ? 0xFFFFFFFFu : (1u << (8u * (d - p))) - 1u;
      const uint32_t a = pad & m, b = lds_dword(lit + p) & m;
      if (a != b) return __builtin_bswap32(a) < __builtin_bswap32(b) ? -1 : 1;
    }
    lit += d;
    llen = v.len;
  } else if (v.len > llen) {
    pv = v.len - llen;
    const int c = compare_span(v, 0, pv, [pad](uint32_t) { return pad; });
    if (c) return c;
  }
  return compare_span(v, pv, llen, [lit](uint32_t p) { return lds_dword(lit + p); });
}

// The lane's value of at most FILTER_KEY128_BYTES big-endian two's-complement bytes as a sign-extended
// 128-bit integer: up to four dwords, byte-swapped into one 128-bit word whose top bytes are the value,
// shifted down arithmetically (what was loaded past the value leaves with the shift). Empty: 0.
// A value inside the wave's buffer takes the five aligned dwords that cover any 16 bytes and v_alignbyte
// (value_dword would fetch eight); a dword past the buffer reads 0.
__device__ __forceinline__ void value_key128(const LaneValue& v, int64_t* hi, uint64_t* lo) {
  uint32_t c[4];
  if (!v.slow) {
    const uint32_t a = v.rel & ~3u, sb = v.rel & 3u;
    uint32_t w[5];
#pragma unroll
    for (uint32_t k = 0; k < 5; k++) w[k] = ld32(v.rs, a + 4u * k);
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) c[k] = __builtin_bswap32(__builtin_amdgcn_alignbyte(w[k + 1], w[k], sb));
  } else {
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) c[k] = 4u * k < v.len ? __builtin_bswap32(value_dword(v, 4u * k)) : 0u;
  }
  int64_t h = (int64_t)(((uint64_t)c[0] << 32) | c[1]);
  uint64_t l = ((uint64_t)c[2] << 32) | c[3];
  const uint32_t sh = 8u * (FILTER_KEY128_BYTES - v.len);
  if (sh >= 128u) {
    h = 0;
    l = 0;
  } else if (sh >= 64u) {
    l = (uint64_t)(h >> (sh - 64u));
    h >>= 63;
  } else if (sh) {
    l = (l >> sh) | ((uint64_t)h << (64u - sh));
    h >>= sh;
  }
  *hi = h;
  *lo = l;
}

__device__ __forceinline__ bool binary_type(int32_t type) {
  return type == PQG_BYTE_ARRAY || type == PQG_INT96 || type == PQG_FIXED_LEN_BYTE_ARRAY;
}

// compare(value, literal j of the leaf whose cells begin at `b`) of the column's PrimitiveComparator.
template <bool BIN>
__device__ __forceinline__ int compare_cell(const LaneValue& v, bool binary, uint32_t flags, const uint64_t* cells,
                                            const uint8_t* lbytes, uint32_t b, uint32_t j) {
  if (BIN && (flags & FILTER_DEV_SIGNED)) {
    const bool keys = (flags & FILTER_DEV_KEY128) != 0;
    const uint64_t* c = cells + b + (keys ? 3u * j : j);
    if (keys && v.len <= FILTER_KEY128_BYTES) {  // leaf_value made the value's key
      const int64_t hi = (int64_t)c[1];
      const uint64_t lo = c[2];
      if (v.key != hi) return v.key < hi ? -1 : 1;
      return (v.lo > lo) - (v.lo < lo);
    }
    return compare_signed_bytes(v, lbytes + (uint32_t)c[0], (uint32_t)(c[0] >> 32));
  }
  const uint64_t cell = cells[b + j];
  if (!binary) {
    const int64_t k = (int64_t)cell;
    return (v.key > k) - (v.key < k);
  }
  return compare_bytes(v, lbytes + (uint32_t)cell, (uint32_t)(cell >> 32));
}

// The value a leaf compares, from the column's loaded value: the comparator key of a fixed-width value
// (the unsigned flag is the leaf's), of a FLOAT16, or of a signed integer that the 128-bit keys cover.
template <bool BIN>
__device__ __forceinline__ LaneValue leaf_value(const FilterDevNode& nd, int32_t type, bool valid, const LaneValue& v) {
  LaneValue lv = v;
  if (BIN && binary_type(type)) {
    if (nd.flags & FILTER_DEV_FLOAT16)
      lv.key = valid ? filter_key_float16(value_dword(v, 0) & 0xFFFFu) : 0;
    else if ((nd.flags & FILTER_DEV_KEY128) && valid && v.len <= FILTER_KEY128_BYTES)
      value_key128(v, &lv.key, &lv.lo);
    return lv;
  }
  if (type != PQG_BYTE_ARRAY) lv.key = filter_key(type, (nd.flags & PQG_FILTER_UNSIGNED) != 0, (uint64_t)v.key);
  return lv;
}

// One leaf on one row (the generated ValueInspectors): `valid` = the row has a value.
template <bool BIN>
__device__ __forceinline__ bool leaf_eval(const FilterDevNode& nd, bool valid, const LaneValue& v, const uint64_t* cells,
                                          const uint8_t* lbytes) {
  const bool null_lit = (nd.flags & PQG_FILTER_NULL_LITERAL) != 0;
  const bool binary = BIN ? binary_type(nd.type) && !(nd.flags & FILTER_DEV_FLOAT16) : nd.type == PQG_BYTE_ARRAY;
  const uint32_t fl = nd.flags;
  const uint32_t b = nd.lit_begin, n = nd.n_lit;
  if (null_lit)  // eq(c, null) / in(c, {null, ...}): null rows; notEq / notIn: the others
    return (nd.op == PQG_FILTER_EQ || nd.op == PQG_FILTER_IN) ? !valid : valid;
  if (nd.op == PQG_FILTER_IN || nd.op == PQG_FILTER_NOTIN) {
    bool found = false;
    if (valid) {
      if (n <= FILTER_IN_LINEAR) {
        for (uint32_t j = 0; j < n; j++) found |= compare_cell<BIN>(v, binary, fl, cells, lbytes, b, j) == 0;
      } else {  // the set is sorted by comparator order
        uint32_t lo = 0, hi = n;
        while (lo < hi) {
          const uint32_t mid = (lo + hi) >> 1;
          const int c = compare_cell<BIN>(v, binary, fl, cells, lbytes, b, mid);
          if (c == 0) {
            found = true;
            break;
          }
          if (c > 0) lo = mid + 1; else hi = mid;
        }
      }
    }
    return nd.op == PQG_FILTER_IN ? found : !found;
  }
  const int c = valid ? compare_cell<BIN>(v, binary, fl, cells, lbytes, b, 0) : 0;
  switch (nd.op) {
    case PQG_FILTER_EQ: return valid && c == 0;
    case PQG_FILTER_NOTEQ: return !valid || c != 0;
    case PQG_FILTER_LT: return valid && c < 0;
    case PQG_FILTER_LTEQ: return valid && c <= 0;
    case PQG_FILTER_GT: return valid && c > 0;
    default: return valid && c >= 0;  // GTEQ
  }
}

// The lane's value `idx` of a column (`valid` lanes only; the whole wave calls): the raw bits of a fixed-width
// value (the key is per leaf), or where a BYTE_ARRAY value's bytes are. ENTRY: the column is a dictionary of
// n_values entries, whose offsets are clamped into [offsets[0], offsets[n_values]] (n_values > 0).
// BIN: an INT96 / FIXED_LEN_BYTE_ARRAY value is the `width` bytes at idx * width of `values`, found like a
// BYTE_ARRAY value's (idx < n_values: inside the column).
template <bool ENTRY, bool BIN>
__device__ __forceinline__ LaneValue load_value(int32_t type, uint32_t width, const void* values, const uint8_t* binary,
                                                bool valid, uint64_t idx, uint64_t n_values) {
  LaneValue v;
  v.key = 0;
  v.lo = 0;
  v.rel = v.len = 0;
  v.slow = nullptr;
  const bool fixed = BIN && (type == PQG_INT96 || type == PQG_FIXED_LEN_BYTE_ARRAY);
  if (type == PQG_BYTE_ARRAY || fixed) {
    // the value's bytes are [a0, a1) (addresses), as its two offsets say
    uint64_t a0 = 0, a1 = 0;
    if (fixed) {
      binary = (const uint8_t*)values;
      if (valid) {
        a0 = (uint64_t)(uintptr_t)values + idx * (uint64_t)width;
        a1 = a0 + width;
      }
    } else if (valid) {
      int64_t a = ((const int64_t*)values)[idx], b = ((const int64_t*)values)[idx + 1];
      if (ENTRY) {
        int64_t lo = ((const int64_t*)values)[0], hi = ((const int64_t*)values)[n_values];
        lo = lo < 0 ? 0 : lo;
        hi = hi < lo ? lo : hi;
        a = a < lo ? lo : (a > hi ? hi : a);
        b = b > hi ? hi : b;
      }
      a0 = (uint64_t)(uintptr_t)binary + (uint64_t)(a < 0 ? 0 : a);
      a1 = (uint64_t)(uintptr_t)binary + (uint64_t)(b < a || b < 0 ? (a < 0 ? 0 : a) : b);
    }
    const uint64_t vm = __ballot(valid);
    // the wave's buffer spans its first value's start to its last value's end (offsets ascend), cut to
    // whole dwords: a buffer load is range-checked per dword, so one that straddles the end reads 0. A
    // value that reaches into the cut tail, lies outside the buffer or more than 4 GiB into it is read
    // with plain byte loads inside its own bytes
    uint64_t first = vm ? rdl64(a0, (uint32_t)__builtin_ctzll(vm)) & ~3ull : 0;
    if (first < (uint64_t)(uintptr_t)binary)  // fixed: the first whole dword inside the column (a value before it: byte loads)
      first = fixed ? ((uint64_t)(uintptr_t)binary + 3u) & ~3ull : (uint64_t)(uintptr_t)binary;
    const uint64_t last = vm ? rdl64(a1, 63u - (uint32_t)__builtin_clzll(vm)) : 0;
    const uint64_t whole = last > first ? (last - first) & ~3ull : 0;
    v.rs = make_rsrc((const uint8_t*)(uintptr_t)first, whole);
    const uint64_t len = a1 - a0;
    v.len = len > 0x7FFFFFFFull ? 0x7FFFFFFFu : (uint32_t)len;
    if (a0 < first || a0 - first + v.len > (whole < 0xFFFFFFF0ull ? whole : 0xFFFFFFF0ull))
      v.slow = (const uint8_t*)(uintptr_t)a0;
    v.rel = (uint32_t)(a0 - first);
  } else if (valid) {
    uint64_t raw;
    if (type == PQG_BOOLEAN) raw = ((const uint8_t*)values)[idx];
    else if (type == PQG_INT32 || type == PQG_FLOAT) raw = ((const uint32_t*)values)[idx];
    else raw = ((const uint64_t*)values)[idx];
    v.key = (int64_t)raw;  // the raw bits; the key is per leaf (the unsigned flag is the leaf's)
  }
  return v;
}

// the program, literal cells and literal bytes: staged once per workgroup (the caller synchronises)
__device__ __forceinline__ void stage_image(uint8_t* lds, const uint8_t* __restrict__ image, uint32_t image_bytes) {
  for (uint32_t i = threadIdx.x * 8u; i < image_bytes; i += 64u * FT_WPB * 8u)
    *(uint64_t*)(lds + i) = *(const uint64_t*)(image + i);
}

}  // namespace pqg
