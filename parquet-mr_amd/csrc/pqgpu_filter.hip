// pqgpu_filter.hip — record-level filter2 predicates over decoded columns (pqg_filter_run,
// pqg_filter_run_dict).
//
// Five launches on the context's stream, none of which waits on another workgroup (every
// cross-tile dependency is a launch boundary):
//   k_filter_rank  per nullable column and tile: rows with dl == max_def
//   k_filter_scan  one workgroup per column: exclusive scan of those counts (a tile's first dense
//                  value index), the total checked against the column's n_values
//   k_filter_eval  one wave per tile of PQG_FILTER_TILE_ROWS rows, 64 rows per step, lane = row
//   k_filter_scan  the tiles' selected counts -> first row id slot per tile, n_selected, the result
//   k_filter_emit  bitmap words -> ascending row ids, bounded by the capacity
// A tile is one wave's work: 64 steps of 64 rows, lane k keeping the bitmap word of step k, so the
// tile's 64 words leave as one 512-byte store.
// With dictionary-id columns (pqg_filter_run_dict) one launch goes first when a leaf has a verdict table:
//   k_filter_dict  one wave per 64 entries of a leaf's dictionary: the leaf on every entry, one bit each
// and k_filter_eval<true> takes a leaf's verdict on such a column as bit `id` of its table.
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

// ---- k_filter_rank ---------------------------------------------------------------------------
__global__ __launch_bounds__(64 * FT_WPB) void k_filter_rank(const FilterCols cols, uint64_t n_rows, uint64_t n_tiles,
                                                             uint64_t* __restrict__ rank) {
  const uint64_t tile = (uint64_t)blockIdx.x * FT_WPB + wave_id();
  if (tile >= n_tiles) return;
  const uint32_t ni = blockIdx.y;
  const FilterColDev& c = cols.c[cols.null_slot[ni]];
  const uint8_t* __restrict__ dl = c.dl;
  const uint32_t md = (uint32_t)c.max_def;
  const uint32_t lane = lane_id();
  const uint64_t row0 = tile * FT_ROWS;
  uint32_t cnt = 0;
  if (((uintptr_t)dl & 3u) == 0) {
#pragma unroll 4
    for (uint32_t k = 0; k < FT_ROWS / 256; k++) {
      const uint64_t r = row0 + 4ull * (k * 64u + lane);
      if (r + 4 <= n_rows) {
        const uint32_t w = *(const uint32_t*)(dl + r);
        cnt += ((w & 0xFFu) == md) + (((w >> 8) & 0xFFu) == md) + (((w >> 16) & 0xFFu) == md) + ((w >> 24) == md);
      } else {
        for (uint32_t b = 0; b < 4; b++)
          if (r + b < n_rows) cnt += dl[r + b] == md;
      }
    }
  } else {
    for (uint32_t s = 0; s < FT_STEPS; s++) {
      const uint64_t r = row0 + s * 64u + lane;
      if (r < n_rows) cnt += dl[r] == md;
    }
  }
  uint32_t total;
  (void)wave_excl_scan_u32(cnt, &total);
  if (lane == 0) gst(&rank[(uint64_t)ni * n_tiles + tile], (uint64_t)total);
}

// ---- k_filter_scan ---------------------------------------------------------------------------
// One workgroup per row of `arr` (n_tiles words each): exclusive scan in place, FS_PER tiles per thread
// per round. FINAL = false (the rank counts of nullable column blockIdx.x): the total goes to
// totals[blockIdx.x] and bad[blockIdx.x] says whether it differs from the column's n_values.
// FINAL = true (the selected counts, one row): writes the result, with the first bad column; DICT: when
// the counts are right, the lowest column with an id outside its dictionary (dict_bad, per slot).
template <bool FINAL, bool DICT = false>
__global__ __launch_bounds__(256) void k_filter_scan(uint64_t* __restrict__ arr, uint64_t n_tiles, const FilterCols cols,
                                                     uint64_t* __restrict__ totals, uint64_t* __restrict__ bad,
                                                     pqg_filter_result* __restrict__ result,
                                                     const uint64_t* __restrict__ dict_bad) {
  const uint64_t carry = block_excl_scan_u64<FS_PER>(arr + (uint64_t)blockIdx.x * n_tiles, n_tiles);
  if (threadIdx.x != 0) return;
  if (!FINAL) {
    gst(&totals[blockIdx.x], carry);
    gst(&bad[blockIdx.x], (uint64_t)(carry != cols.c[cols.null_slot[blockIdx.x]].n_values));
  } else {
    int32_t err_col = -1;
    for (uint32_t ni = 0; ni < cols.n_nullable; ni++) {
      const int32_t col = cols.c[cols.null_slot[ni]].column;
      if (bad[ni] && (err_col < 0 || col < err_col)) err_col = col;
    }
    int32_t err = err_col >= 0 ? PQG_ERR_INVALID_ARG : PQG_OK;
    if (DICT && err_col < 0) {
      for (uint32_t s = 0; s < cols.n_slots; s++) {
        const int32_t col = cols.c[s].column;
        if (dict_bad[s] && (err_col < 0 || col < err_col)) err_col = col;
      }
      if (err_col >= 0) err = PQG_ERR_DICT_ID;
    }
    result->n_selected = carry;
    result->error = err;
    result->error_column = err_col;
  }
}

// ---- k_filter_eval ---------------------------------------------------------------------------
// A lane's value of the column being evaluated: the comparator key of a fixed-width value, or where a
// BYTE_ARRAY value's bytes are.
struct LaneValue {
  int64_t key;
  rsrc_t rs;             // BYTE_ARRAY: the binary data from the wave's first value on (range-checked)
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

// compare(value, literal cell j) of the column's PrimitiveComparator.
__device__ __forceinline__ int compare_cell(const LaneValue& v, bool binary, const uint64_t* cells, const uint8_t* lbytes,
                                            uint32_t j) {
  const uint64_t cell = cells[j];
  if (!binary) {
    const int64_t k = (int64_t)cell;
    return (v.key > k) - (v.key < k);
  }
  return compare_bytes(v, lbytes + (uint32_t)cell, (uint32_t)(cell >> 32));
}

// One leaf on one row (the generated ValueInspectors): `valid` = the row has a value.
__device__ __forceinline__ bool leaf_eval(const FilterDevNode& nd, bool valid, const LaneValue& v, const uint64_t* cells,
                                          const uint8_t* lbytes) {
  const bool null_lit = (nd.flags & PQG_FILTER_NULL_LITERAL) != 0;
  const bool binary = nd.type == PQG_BYTE_ARRAY;
  const uint32_t b = nd.lit_begin, n = nd.n_lit;
  if (null_lit)  // eq(c, null) / in(c, {null, ...}): null rows; notEq / notIn: the others
    return (nd.op == PQG_FILTER_EQ || nd.op == PQG_FILTER_IN) ? !valid : valid;
  if (nd.op == PQG_FILTER_IN || nd.op == PQG_FILTER_NOTIN) {
    bool found = false;
    if (valid) {
      if (n <= FILTER_IN_LINEAR) {
        for (uint32_t j = 0; j < n; j++) found |= compare_cell(v, binary, cells, lbytes, b + j) == 0;
      } else {  // the set is sorted by comparator order
        uint32_t lo = 0, hi = n;
        while (lo < hi) {
          const uint32_t mid = (lo + hi) >> 1;
          const int c = compare_cell(v, binary, cells, lbytes, b + mid);
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
  const int c = valid ? compare_cell(v, binary, cells, lbytes, b) : 0;
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
template <bool ENTRY>
__device__ __forceinline__ LaneValue load_value(int32_t type, const void* values, const uint8_t* binary, bool valid,
                                                uint64_t idx, uint64_t n_values) {
  LaneValue v;
  v.key = 0;
  v.rel = v.len = 0;
  v.slow = nullptr;
  if (type == PQG_BYTE_ARRAY) {
    // the value's bytes are [a0, a1) (addresses), as its two offsets say
    uint64_t a0 = 0, a1 = 0;
    if (valid) {
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
    if (first < (uint64_t)(uintptr_t)binary) first = (uint64_t)(uintptr_t)binary;
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

// ---- k_filter_dict ---------------------------------------------------------------------------
// Grid (64-entry words / FT_WPB, table leaves): a wave evaluates its leaf on 64 entries of the leaf's
// dictionary, lane = entry, and stores the ballot as one word of the leaf's table. Entries past n_entries: 0.
__global__ __launch_bounds__(64 * FT_WPB) void k_filter_dict(const uint8_t* __restrict__ image, uint32_t image_bytes,
                                                             const FilterDictTab* __restrict__ dt,
                                                             uint64_t* __restrict__ tables) {
  extern __shared__ __align__(16) uint8_t lds[];
  stage_image(lds, image, image_bytes);
  __syncthreads();
  const FilterDevHeader& h = *(const FilterDevHeader*)lds;
  const FilterDevNode* nodes = (const FilterDevNode*)(lds + sizeof(FilterDevHeader));
  const uint64_t* cells = (const uint64_t*)(lds + uni(h.cells_off));
  const uint8_t* lbytes = lds + uni(h.bytes_off);
  const uint32_t ni = uni(dt->table_leaf[blockIdx.y]);
  const FilterDevNode nd = nodes[ni];
  const FilterDictSlot ds = dt->slot[uni(nd.slot)];
  const uint32_t n = uni(ds.n_entries);
  const uint64_t word = (uint64_t)blockIdx.x * FT_WPB + wave_id();
  if (word >= ((uint64_t)n + 63) / 64) return;
  const uint32_t type = uni(nd.type);
  const uint64_t e = word * 64 + lane_id();
  const bool valid = e < n;
  LaneValue v = load_value<true>((int32_t)type, ds.values, ds.binary, valid, e, n);
  if (type != PQG_BYTE_ARRAY) v.key = filter_key((int)type, (nd.flags & PQG_FILTER_UNSIGNED) != 0, (uint64_t)v.key);
  const uint64_t m = __ballot(valid && leaf_eval(nd, valid, v, cells, lbytes));
  if (lane_id() == 0) gst(&tables[uni64(dt->leaf_off[ni]) + word], m);
}

// ---- k_filter_eval ---------------------------------------------------------------------------
// DICT = false is pqg_filter_run's kernel. DICT = true: slots with a dictionary (dt->slot[s].is_dict) hold
// uint32 ids; a leaf's verdict on a row is bit `id` of the leaf's table (staged in LDS behind the image when
// dt->in_lds, else read from `tables`), a row without a value takes the leaf's verdict on null, and an id
// outside the dictionary sets the slot's word of dict_bad (every writer stores 1) and matches nothing.
template <bool DICT>
__global__ __launch_bounds__(64 * FT_WPB) void k_filter_eval(const uint8_t* __restrict__ image, uint32_t image_bytes,
                                                             const FilterCols cols, uint64_t n_rows, uint64_t n_tiles,
                                                             const uint64_t* __restrict__ rank, uint64_t* __restrict__ bitmap,
                                                             uint64_t* __restrict__ sel,
                                                             const FilterDictTab* __restrict__ dt,
                                                             const uint64_t* __restrict__ tables,
                                                             uint64_t* __restrict__ dict_bad) {
  extern __shared__ __align__(16) uint8_t lds[];
  stage_image(lds, image, image_bytes);
  const uint64_t* lds_tables = (const uint64_t*)(lds + image_bytes);  // image_bytes is a multiple of 8
  bool in_lds = false;
  if (DICT) {
    in_lds = uni(dt->in_lds) != 0;
    if (in_lds) {
      const uint32_t words = (uint32_t)uni64(dt->table_words);
      for (uint32_t i = threadIdx.x; i < words; i += 64u * FT_WPB) ((uint64_t*)(lds + image_bytes))[i] = tables[i];
    }
  }
  __syncthreads();
  const uint64_t tile = (uint64_t)blockIdx.x * FT_WPB + wave_id();
  if (tile >= n_tiles) return;
  const FilterDevHeader& h = *(const FilterDevHeader*)lds;
  const FilterDevNode* nodes = (const FilterDevNode*)(lds + sizeof(FilterDevHeader));
  const uint32_t n_nodes = uni(h.n_nodes), n_leaves = uni(h.n_leaves), n_slots = uni(h.n_slots);
  const uint8_t* order = (const uint8_t*)(nodes + n_nodes);
  const uint64_t* cells = (const uint64_t*)(lds + uni(h.cells_off));
  const uint8_t* lbytes = lds + uni(h.bytes_off);

  const uint32_t lane = lane_id();
  const uint64_t row0 = tile * FT_ROWS;
  const uint64_t n_words = (n_rows + 63) / 64;
  const uint32_t steps = n_words - tile * FT_STEPS < FT_STEPS ? (uint32_t)(n_words - tile * FT_STEPS) : FT_STEPS;

  // lane s holds slot s's state: the dense index of the tile's next non-null row
  uint64_t next_idx = 0;
  if (lane < n_slots) {
    const FilterColDev& c = cols.c[lane];
    if (c.null_idx >= 0) next_idx = rank[(uint64_t)c.null_idx * n_tiles + tile];
  }
  uint64_t node_mask = 0;  // lane i holds the 64-row mask of node i in the current step
  uint64_t my_word = 0;    // lane k keeps the bitmap word of step k
  uint32_t n_sel = 0;

  for (uint32_t s = 0; s < steps; s++) {
    const uint64_t row = row0 + s * 64u + lane;
    const bool in = row < n_rows;
    uint32_t li = 0;
    for (uint32_t sl = 0; sl < n_slots; sl++) {
      const FilterColDev& c = cols.c[sl];
      const int32_t type = c.type;
      bool valid;
      uint64_t idx;
      if (c.max_def == 0) {
        valid = in;
        idx = row;
      } else if (!c.dl) {
        valid = false;
        idx = 0;
      } else {
        valid = in && c.dl[row] == (uint8_t)c.max_def;
        const uint64_t vb = __ballot(valid);
        const uint64_t base = rdl64(next_idx, sl);
        idx = base + lanes_below(vb);
        if (lane == sl) next_idx = base + (uint32_t)__popcll(vb);
      }
      valid = valid && idx < c.n_values;  // every value load stays inside the column
      if (DICT && uni(dt->slot[sl].is_dict)) {
        const uint32_t n_entries = uni(dt->slot[sl].n_entries);
        const uint32_t id = valid ? ((const uint32_t*)c.values)[idx] : 0u;
        const bool ok = valid && id < n_entries;  // every table read stays inside the table
        if (valid && !ok) gst(&dict_bad[sl], (uint64_t)1);
        while (li < n_leaves) {
          const uint32_t ni = uni(order[li]);
          const FilterDevNode nd = nodes[ni];
          if (uni(nd.slot) != sl) break;
          bool verdict;
          if (nd.flags & PQG_FILTER_NULL_LITERAL) {
            verdict = (nd.op == PQG_FILTER_EQ || nd.op == PQG_FILTER_IN) ? !valid : valid;
          } else {
            uint64_t w = 0;
            if (ok) {
              const uint64_t o = uni64(dt->leaf_off[ni]) + (id >> 6);
              w = in_lds ? lds_tables[o] : tables[o];
            }
            // a null row: what leaf_eval gives without a value
            verdict = valid ? ((w >> (id & 63u)) & 1u) != 0 : (nd.op == PQG_FILTER_NOTEQ || nd.op == PQG_FILTER_NOTIN);
          }
          const uint64_t m = __ballot(verdict);
          if (lane == ni) node_mask = m;
          li++;
        }
        continue;
      }
      const LaneValue v = load_value<false>(type, c.values, c.binary, valid, idx, 0);
      // every leaf on this column (the column is loaded once per step)
      while (li < n_leaves) {
        const uint32_t ni = uni(order[li]);
        const FilterDevNode nd = nodes[ni];
        if (uni(nd.slot) != sl) break;
        LaneValue lv = v;
        if (type != PQG_BYTE_ARRAY) lv.key = filter_key(type, (nd.flags & PQG_FILTER_UNSIGNED) != 0, (uint64_t)v.key);
        const uint64_t m = __ballot(leaf_eval(nd, valid, lv, cells, lbytes));
        if (lane == ni) node_mask = m;
        li++;
      }
    }
    // and / or on wave-uniform 64-row masks (children have smaller indices)
    for (uint32_t i = 0; i < n_nodes; i++) {
      const uint32_t op = uni(nodes[i].op);
      if (op != PQG_FILTER_AND && op != PQG_FILTER_OR) continue;
      const uint64_t a = rdl64(node_mask, uni(nodes[i].left)), b = rdl64(node_mask, uni(nodes[i].right));
      const uint64_t m = op == PQG_FILTER_AND ? (a & b) : (a | b);
      if (lane == i) node_mask = m;
    }
    const uint64_t word = rdl64(node_mask, n_nodes - 1) & __ballot(in);  // rows past n_rows: 0
    if (lane == s) my_word = word;
    n_sel += (uint32_t)__popcll(word);
  }
  if (lane < steps) gst_nt(&bitmap[tile * FT_STEPS + lane], my_word);
  if (lane == 0) gst(&sel[tile], (uint64_t)n_sel);
}

// ---- k_filter_emit ---------------------------------------------------------------------------
// Row ids of a tile: its first output slot is sel[tile] (scanned), lane k expands word k.
__global__ __launch_bounds__(64 * FT_WPB) void k_filter_emit(const uint64_t* __restrict__ bitmap, uint64_t n_rows,
                                                             uint64_t n_tiles, const uint64_t* __restrict__ sel,
                                                             int64_t* __restrict__ row_ids, uint64_t capacity) {
  const uint64_t tile = (uint64_t)blockIdx.x * FT_WPB + wave_id();
  if (tile >= n_tiles) return;
  const uint32_t lane = lane_id();
  const uint64_t n_words = (n_rows + 63) / 64;
  const uint64_t wi = tile * FT_STEPS + lane;
  uint64_t w = wi < n_words ? bitmap[wi] : 0;
  uint32_t total;
  const uint32_t before = wave_excl_scan_u32((uint32_t)__popcll(w), &total);
  uint64_t pos = sel[tile] + before;
  const int64_t base = (int64_t)(wi * 64);
  while (w && pos < capacity) {
    gst(&row_ids[pos], base + (int64_t)__builtin_ctzll(w));
    w &= w - 1;
    pos++;
  }
}

// ---- launch ----------------------------------------------------------------------------------
hipError_t launch_filter(hipStream_t st, const uint8_t* d_image, uint32_t image_bytes, const FilterCols& cols,
                         uint64_t n_rows, uint64_t* scratch, uint64_t* bitmap, int64_t* row_ids, uint64_t row_ids_capacity,
                         pqg_filter_result* result, const FilterDictTab* d_dict, const FilterDictTab* h_dict) {
  const uint64_t n_tiles = filter_tiles(n_rows);
  uint64_t* rank = scratch;
  uint64_t* sel = rank + (uint64_t)cols.n_nullable * n_tiles;
  uint64_t* totals = sel + n_tiles;
  uint64_t* bad = totals + PQG_FILTER_MAX_NODES;
  uint64_t* dict_bad = bad + PQG_FILTER_MAX_NODES;      // with dictionaries only
  uint64_t* tables = dict_bad + PQG_FILTER_MAX_NODES;
  const uint32_t wgs = (uint32_t)((n_tiles + FT_WPB - 1) / FT_WPB);
  if (d_dict) {
    if (hipMemsetAsync(dict_bad, 0, 8 * PQG_FILTER_MAX_NODES, st) != hipSuccess) return hipGetLastError();
    if (h_dict->n_tables)
      hipLaunchKernelGGL(k_filter_dict, dim3((uint32_t)((h_dict->max_words + FT_WPB - 1) / FT_WPB), h_dict->n_tables),
                         dim3(64 * FT_WPB), image_bytes, st, d_image, image_bytes, d_dict, tables);
  }
  if (cols.n_nullable) {
    if (n_tiles)
      hipLaunchKernelGGL(k_filter_rank, dim3(wgs, cols.n_nullable), dim3(64 * FT_WPB), 0, st, cols, n_rows, n_tiles, rank);
    hipLaunchKernelGGL(k_filter_scan<false>, dim3(cols.n_nullable), dim3(256), 0, st, rank, n_tiles, cols, totals, bad,
                       result, (const uint64_t*)nullptr);
  }
  if (!d_dict) {
    if (n_tiles)
      hipLaunchKernelGGL(k_filter_eval<false>, dim3(wgs), dim3(64 * FT_WPB), image_bytes, st, d_image, image_bytes, cols,
                         n_rows, n_tiles, rank, bitmap, sel, (const FilterDictTab*)nullptr, (const uint64_t*)nullptr,
                         (uint64_t*)nullptr);
    hipLaunchKernelGGL(k_filter_scan<true>, dim3(1), dim3(256), 0, st, sel, n_tiles, cols, totals, bad, result,
                       (const uint64_t*)nullptr);
  } else {
    const uint32_t lds_bytes = image_bytes + (h_dict->in_lds ? (uint32_t)h_dict->table_words * 8u : 0u);
    if (n_tiles)
      hipLaunchKernelGGL(k_filter_eval<true>, dim3(wgs), dim3(64 * FT_WPB), lds_bytes, st, d_image, image_bytes, cols,
                         n_rows, n_tiles, rank, bitmap, sel, d_dict, tables, dict_bad);
    hipLaunchKernelGGL((k_filter_scan<true, true>), dim3(1), dim3(256), 0, st, sel, n_tiles, cols, totals, bad, result,
                       dict_bad);
  }
  if (n_tiles && row_ids && row_ids_capacity)
    hipLaunchKernelGGL(k_filter_emit, dim3(wgs), dim3(64 * FT_WPB), 0, st, bitmap, n_rows, n_tiles, sel, row_ids,
                       row_ids_capacity);
  return hipGetLastError();
}

}  // namespace pqg
