// pqgpu_take.hip — the rows a selection bitmap keeps, gathered into compact columns (pqg_take), and the
// records it keeps of columns with repetition levels (pqg_take_records, second half of this file).
//
// Launches on the context's stream, none of which waits on another workgroup (every cross-tile
// dependency is a launch boundary) and whose number does not depend on the number of columns (the
// column is grid.y):
//   k_take_count   per (column, tile): rows with dl == max_def (the tile's source rank), kept rows
//                  with dl == max_def; column 0's waves also count the tile's kept rows (from its words)
//   k_take_scan    one workgroup per counted array: exclusive scan in place, the total aside
//   k_take_bytes   BYTE_ARRAY columns only, per (column, tile): bytes of the kept values (needs the
//                  scanned ranks: a value's offsets sit at its dense index)
//   k_take_scan    those byte counts
//   k_take_finish  one wave, lane = column: d_counts, the n_values and capacity verdicts, d_result,
//                  the closing BYTE_ARRAY offsets
//   k_take_gather  one wave per (column, tile), 64 rows per step, lane = row: the source index is the
//                  tile's rank + mbcnt(valid), the destinations the tile's output bases + mbcnt(valid &
//                  keep) and + mbcnt(keep). Every load is checked against n_values and every store
//                  against the capacities. The loads of 8 steps are issued together.
// A tile is PQG_FILTER_TILE_ROWS rows: its 64 bitmap words are one 512-byte load, lane k holding the
// word of step k. The output of a tile is contiguous, so kept elements go through a small LDS ring per
// wave and leave as aligned full-wave stores (STAGED; the direct variant, one store per kept lane, is
// kept for the A/B: PQG_DISPATCH_TAKE_STAGED).
#include "pqgpu_device.h"
#include "pqgpu_take.h"

namespace pqg {

constexpr uint32_t TT_ROWS = PQG_FILTER_TILE_ROWS;
constexpr uint32_t TT_STEPS = TT_ROWS / 64;
static_assert(TT_STEPS == 64, "lane k holds the bitmap word of step k: 64 steps per tile");
constexpr int TT_WPB = 4;  // tiles (waves) per workgroup
constexpr int TS_PER = 4;  // k_take_scan: tiles per thread per round

__device__ __forceinline__ uint32_t take_lanes_below(uint64_t m) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}
__device__ __forceinline__ uint64_t take_rdl64(uint64_t v, uint32_t l) {
  return ((uint64_t)rdl((uint32_t)(v >> 32), l) << 32) | rdl((uint32_t)v, l);
}

// scratch layout (see take_scratch_words)
struct TakeScratch {
  uint64_t *keep, *rank, *kept, *bytes, *totals;
  uint64_t n_tiles;
  uint32_t n_cols;
};
__host__ __device__ inline TakeScratch take_scratch(uint64_t* s, uint64_t n_tiles, uint32_t n_cols) {
  TakeScratch t;
  t.n_tiles = n_tiles;
  t.n_cols = n_cols;
  t.keep = s;
  t.rank = t.keep + n_tiles;
  t.kept = t.rank + (uint64_t)n_cols * n_tiles;
  t.bytes = t.kept + (uint64_t)n_cols * n_tiles;
  t.totals = t.bytes + (uint64_t)n_cols * n_tiles;  // [0] kept rows, [1 + c] rank, [1 + C + c] kept values, [1 + 2C + c] bytes
  return t;
}

// The tile's bitmap word of step `lane`, rows past n_rows cleared.
__device__ __forceinline__ uint64_t tile_word(const uint64_t* __restrict__ bitmap, uint64_t n_rows, uint64_t tile) {
  const uint64_t n_words = (n_rows + 63) / 64;
  const uint64_t wi = tile * TT_STEPS + lane_id();
  uint64_t w = wi < n_words ? bitmap[wi] : 0;
  if (wi == n_words - 1 && (n_rows & 63u)) w &= (1ull << (n_rows & 63u)) - 1ull;
  return w;
}

// ---- k_take_count ----------------------------------------------------------------------------
// One wave's counts over a tile: rows with dl == md, kept rows with dl == md (both 0 without dl), kept rows.
__device__ __forceinline__ void take_count_tile(const uint64_t* __restrict__ bitmap, uint64_t n_rows, uint64_t tile,
                                                const uint8_t* __restrict__ dl, uint32_t md, uint32_t& t_valid,
                                                uint32_t& t_kept, uint32_t& t_keep) {
  const uint32_t lane = lane_id();
  const uint64_t row0 = tile * TT_ROWS;
  const uint8_t* __restrict__ bm = (const uint8_t*)bitmap;
  const bool dl_words = ((uintptr_t)dl & 3u) == 0;
  uint32_t n_valid = 0, n_kept = 0;
  const uint32_t n_keep = (uint32_t)__popcll(tile_word(bitmap, n_rows, tile));  // lane k: the rows step k keeps
  // a lane takes 4 rows at a time: their keep bits are a nibble of the bitmap, their levels one dword
  if (dl) {
#pragma unroll 4
    for (uint32_t k = 0; k < TT_ROWS / 256; k++) {
      const uint64_t r = row0 + 4ull * (k * 64u + lane);
      if (r >= n_rows) continue;
      const uint32_t in = r + 4 <= n_rows ? 0xFu : (1u << (uint32_t)(n_rows - r)) - 1u;
      const uint32_t keep = ((uint32_t)bm[r >> 3] >> (uint32_t)(r & 4u)) & in;
      uint32_t valid = 0;
      if (dl_words && in == 0xFu) {
        const uint32_t w = *(const uint32_t*)(dl + r);
        valid = ((w & 0xFFu) == md) | ((((w >> 8) & 0xFFu) == md) << 1) | ((((w >> 16) & 0xFFu) == md) << 2) |
                (((w >> 24) == md) << 3);
      } else {
        for (uint32_t b = 0; b < 4; b++)
          if ((in >> b) & 1u) valid |= (uint32_t)(dl[r + b] == md) << b;
      }
      n_valid += (uint32_t)__popc(valid);
      n_kept += (uint32_t)__popc(valid & keep);
    }
  }
  (void)wave_excl_scan_u32(n_valid, &t_valid);
  (void)wave_excl_scan_u32(n_kept, &t_kept);
  (void)wave_excl_scan_u32(n_keep, &t_keep);
}

__global__ __launch_bounds__(64 * TT_WPB) void k_take_count(const uint64_t* __restrict__ bitmap, uint64_t n_rows,
                                                            const TakeColDev* __restrict__ cols, uint32_t n_cols,
                                                            uint64_t* __restrict__ scratch) {
  const TakeScratch S = take_scratch(scratch, (n_rows + TT_ROWS - 1) / TT_ROWS, n_cols);
  const uint64_t tile = (uint64_t)blockIdx.x * TT_WPB + wave_id();
  if (tile >= S.n_tiles) return;
  const uint32_t ci = blockIdx.y;
  const uint8_t* __restrict__ dl = ci < n_cols ? cols[ci].dl : nullptr;
  if (ci != 0 && !dl) return;  // nothing to count: a required column's rank is the row, its kept values the kept rows
  const uint32_t md = dl ? (uint32_t)cols[ci].max_def : 0;
  uint32_t t_valid, t_kept, t_keep;
  take_count_tile(bitmap, n_rows, tile, dl, md, t_valid, t_kept, t_keep);
  if (lane_id() == 0) {
    if (ci == 0) gst(&S.keep[tile], (uint64_t)t_keep);
    if (dl) {
      gst(&S.rank[(uint64_t)ci * S.n_tiles + tile], (uint64_t)t_valid);
      gst(&S.kept[(uint64_t)ci * S.n_tiles + tile], (uint64_t)t_kept);
    }
  }
}

// ---- k_take_scan -----------------------------------------------------------------------------
// Workgroup b scans array first + b of the scratch: 0 the kept rows, 1 + c / 1 + C + c the ranks / kept
// values of nullable column c, 1 + 2C + c the kept bytes of BYTE_ARRAY column c. Arrays nothing was
// counted into are left alone.
__global__ __launch_bounds__(256) void k_take_scan(uint64_t* __restrict__ scratch, uint64_t n_tiles,
                                                   const TakeColDev* __restrict__ cols, uint32_t n_cols, uint32_t first) {
  const TakeScratch S = take_scratch(scratch, n_tiles, n_cols);
  const uint32_t a = first + blockIdx.x;
  if (a > 0) {
    const uint32_t ci = (a - 1) % n_cols, which = (a - 1) / n_cols;
    if (which < 2 ? cols[ci].dl == nullptr : cols[ci].kind != TAKE_BINARY) return;
  }
  const uint64_t total = block_excl_scan_u64<TS_PER>(S.keep + (uint64_t)a * n_tiles, n_tiles);
  if (threadIdx.x == 0) gst(&S.totals[a], total);
}

// ---- BYTE_ARRAY helpers ----------------------------------------------------------------------
// The bytes of dense value idx (idx < n_values) as [a, a + len) of binary_data, held inside the
// column's own bytes [lo, hi) = [offsets[0], offsets[n_values]).
__device__ __forceinline__ void binary_span(const int64_t* __restrict__ off, uint64_t idx, int64_t lo, int64_t hi,
                                            uint64_t& a, uint64_t& len) {
  int64_t x = off[idx], y = off[idx + 1];
  x = x < lo ? lo : (x > hi ? hi : x);
  y = y < x ? x : (y > hi ? hi : y);
  a = (uint64_t)x;
  len = (uint64_t)(y - x);
}

// ---- k_take_bytes ----------------------------------------------------------------------------
// The bytes of the values a tile keeps of BYTE_ARRAY column c (in lane 63), rank0 the tile's source rank.
__device__ __forceinline__ uint64_t take_bytes_tile(const uint64_t* __restrict__ bitmap, uint64_t n_rows, uint64_t tile,
                                                    const TakeColDev c, uint64_t rank0) {
  const uint32_t lane = lane_id();
  const uint64_t row0 = tile * TT_ROWS;
  const uint64_t my_word = tile_word(bitmap, n_rows, tile);
  const int64_t* __restrict__ off = (const int64_t*)c.values;
  const int64_t lo = c.n_values ? off[0] : 0, hi = c.n_values ? off[c.n_values] : 0;
  uint64_t next = rank0;
  uint64_t sum = 0;
  constexpr uint32_t G = 8;  // steps whose loads are issued together
  for (uint32_t g = 0; g < TT_STEPS; g += G) {
    const uint64_t r0 = row0 + g * 64u;
    if (r0 >= n_rows) break;
    uint8_t d[G];
    uint64_t idx[G];
    uint32_t has = 0;
#pragma unroll
    for (uint32_t i = 0; i < G; i++) {
      const uint64_t row = r0 + i * 64u + lane;
      d[i] = c.dl && row < n_rows ? c.dl[row] : 0;
    }
#pragma unroll
    for (uint32_t i = 0; i < G; i++) {
      const bool in = r0 + i * 64u + lane < n_rows;
      const uint64_t vb = __ballot(in && (!c.dl || d[i] == (uint8_t)c.max_def));
      idx[i] = next + take_lanes_below(vb);
      next += (uint32_t)__popcll(vb);
      has |= (uint32_t)((((vb & take_rdl64(my_word, g + i)) >> lane) & 1ull) && idx[i] < c.n_values) << i;
    }
#pragma unroll
    for (uint32_t i = 0; i < G; i++) {
      if (!((has >> i) & 1u)) continue;
      uint64_t a, len;
      binary_span(off, idx[i], lo, hi, a, len);
      sum += len;
    }
  }
  return wave_incl_scan_u64(sum);
}

__global__ __launch_bounds__(64 * TT_WPB) void k_take_bytes(const uint64_t* __restrict__ bitmap, uint64_t n_rows,
                                                            const TakeColDev* __restrict__ cols, uint32_t n_cols,
                                                            uint64_t* __restrict__ scratch) {
  const TakeScratch S = take_scratch(scratch, (n_rows + TT_ROWS - 1) / TT_ROWS, n_cols);
  const uint64_t tile = (uint64_t)blockIdx.x * TT_WPB + wave_id();
  if (tile >= S.n_tiles) return;
  const uint32_t ci = blockIdx.y;
  if (cols[ci].kind != TAKE_BINARY) return;
  const TakeColDev c = cols[ci];
  const uint64_t sum = take_bytes_tile(bitmap, n_rows, tile, c, c.dl ? S.rank[(uint64_t)ci * S.n_tiles + tile] : tile * TT_ROWS);
  if (lane_id() == 63) gst(&S.bytes[(uint64_t)ci * S.n_tiles + tile], sum);
}

// ---- k_take_finish ---------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_take_finish(const TakeColDev* __restrict__ cols, uint32_t n_cols, uint64_t n_rows,
                                                    uint64_t rows_capacity, uint64_t* __restrict__ scratch,
                                                    pqg_take_counts* __restrict__ counts,
                                                    pqg_take_result* __restrict__ result) {
  const TakeScratch S = take_scratch(scratch, (n_rows + TT_ROWS - 1) / TT_ROWS, n_cols);
  const uint32_t ci = threadIdx.x;
  const uint64_t n_keep = S.totals[0];
  bool bad = false;
  if (ci < n_cols) {
    const TakeColDev c = cols[ci];
    uint64_t n_out = 0, n_bytes = 0;
    if (c.kind != TAKE_MISSING) {
      n_out = c.dl ? S.totals[1 + n_cols + ci] : n_keep;
      if (c.dl && S.totals[1 + ci] != c.n_values) bad = true;  // rows with a value differ from n_values
      if (c.kind == TAKE_BINARY) n_bytes = S.totals[1 + 2 * n_cols + ci];
      if (n_out > c.cap_values || n_bytes > c.cap_bytes) bad = true;
      // the closing offset (out_values holds capacity + 1 of them)
      if (c.kind == TAKE_BINARY && n_out <= c.cap_values) gst((int64_t*)c.out_values + n_out, (int64_t)n_bytes);
    }
    if (n_keep > rows_capacity) bad = true;  // the kept rows do not fit: counts against every column
    counts[ci].n_values = n_out;
    counts[ci].n_bytes = n_bytes;
  }
  const uint64_t bad_cols = __ballot(bad);
  if (threadIdx.x == 0) {
    result->n_rows = n_keep;
    const bool err = bad_cols != 0 || n_keep > rows_capacity;
    result->error = err ? PQG_ERR_INVALID_ARG : PQG_OK;
    result->error_column = bad_cols ? (int32_t)__builtin_ctzll(bad_cols) : -1;
  }
}

// ---- the output ring -------------------------------------------------------------------------
// A wave's contiguous output of E-byte elements (E = 1, 4, 8; dst naturally aligned), from element
// `first` on, never at or past element `cap`. STAGED: elements collect in an LDS ring of two granules
// (a granule = 64 lanes x U bytes, U = 4 or 8) indexed by their destination address, and a granule
// leaves as one aligned full-wave store once it is complete; the ends of the run leave by bytes.
// Not STAGED: every element is stored by its own lane at once.
template <uint32_t E, bool STAGED>
struct OutRing {
  static constexpr uint32_t U = E == 8 ? 8 : 4, G = 64 * U, SZ = 2 * G;
  uint8_t* lds;
  uint64_t begin, end;  // destination addresses: the run's first byte, the first byte never to write
  uint64_t head, tail;  // staged bytes are [max(head, begin), tail); head is a multiple of G

  __device__ __forceinline__ void init(uint8_t* ring, void* dst, uint64_t first, uint64_t cap) {
    lds = ring;
    begin = (uint64_t)(uintptr_t)dst + first * E;
    end = (uint64_t)(uintptr_t)dst + (cap > first ? cap : first) * E;
    tail = begin;
    head = begin & ~(uint64_t)(G - 1);
  }
  // Granule [head, head + G) or what of it lies below `lim`.
  __device__ __forceinline__ void emit(uint64_t lim) {
    wave_sync();
    const uint64_t a = head + (uint64_t)U * lane_id();
    const uint64_t stop = lim < end ? lim : end;
    const uint8_t* src = lds + (a & (SZ - 1));
    if (a >= begin && a + U <= stop) {
      if (U == 8) gst_nt((uint64_t*)(uintptr_t)a, *(const uint64_t*)src);
      else gst_nt((uint32_t*)(uintptr_t)a, *(const uint32_t*)src);
    } else {
      for (uint32_t b = 0; b < U; b += E) {
        if (a + b < begin || a + b + E > stop) continue;
        if (E == 1) gst((uint8_t*)(uintptr_t)(a + b), src[b]);
        else if (E == 4) gst((uint32_t*)(uintptr_t)(a + b), *(const uint32_t*)(src + b));
        else gst((uint64_t*)(uintptr_t)(a + b), *(const uint64_t*)(src + b));
      }
    }
    wave_sync();
  }
  // The wave appends the elements of the lanes with `on`, in lane order: pos = set lanes below, n = set lanes.
  template <class T>
  __device__ __forceinline__ void push(bool on, uint32_t pos, uint32_t n, T v) {
    static_assert(sizeof(T) == E, "element width");
    const uint64_t a = tail + (uint64_t)pos * E;
    if (!STAGED) {
      if (on && a + E <= end) gst((T*)(uintptr_t)a, v);
      tail += (uint64_t)n * E;
      return;
    }
    if (on) *(T*)(lds + (a & (SZ - 1))) = v;
    tail += (uint64_t)n * E;
    if (tail - head >= G) {  // at most one granule completes per push (64 elements)
      emit(head + G);
      head += G;
    }
  }
  __device__ __forceinline__ void finish() {
    if (STAGED && tail > head) emit(tail);
  }
};

// LDS per wave: the value ring (2 x 512 bytes for 8-byte elements), the level ring (2 x 256) and a
// BYTE_ARRAY step's inclusive lengths and source addresses (2 x 512)
constexpr uint32_t TG_VAL_RING = 1024, TG_DL_RING = 512, TG_BIN = 1024;
constexpr uint32_t TG_LDS_WAVE = TG_VAL_RING + TG_DL_RING + TG_BIN;

struct TakeTile {
  uint64_t row0, n_rows, my_word;
  uint64_t rank0, val0, row_out0, byte0;  // the tile's source rank and output bases
  uint64_t rows_capacity;
};

// The loads of TG_GROUP steps are issued together (a step at a time leaves a wave waiting for one
// load after the other: 64 memory latencies per tile).
constexpr uint32_t TG_GROUP = 8;
static_assert(TT_STEPS % TG_GROUP == 0, "whole groups per tile");

// A group's lane state: per step, is the row kept, has it a value, where the value sits.
struct TakeGroup {
  uint64_t keep[TG_GROUP], kv[TG_GROUP];  // kept rows, kept rows with a value (wave-uniform masks)
  uint64_t src[TG_GROUP];                 // dense source index of this lane's value
  uint8_t level[TG_GROUP];
  uint32_t has;  // bit i: this lane's row of step i is kept, has a value, and src < n_values
};

template <bool STAGED>
struct TakeWalk {
  const TakeColDev& c;
  const TakeTile& t;
  OutRing<1, STAGED> levels;
  uint64_t next;  // dense index of the next row with a value
  uint32_t g = 0;

  __device__ __forceinline__ TakeWalk(const TakeColDev& col, const TakeTile& tile, uint8_t* lds) : c(col), t(tile) {
    next = t.rank0;
    const uint64_t cap = t.rows_capacity < t.n_rows ? t.rows_capacity : t.n_rows;
    levels.init(lds + TG_VAL_RING, c.out_dl, t.row_out0, c.out_dl ? cap : 0);
  }
  // The next group of steps that keeps a row; false when the tile is done.
  __device__ __forceinline__ bool group(TakeGroup& q) {
    const uint32_t lane = lane_id();
    for (; g < TT_STEPS; g += TG_GROUP) {
      const uint64_t r0 = t.row0 + g * 64u;
      if (r0 >= t.n_rows) break;
      uint64_t any = 0;
#pragma unroll
      for (uint32_t i = 0; i < TG_GROUP; i++) {
        q.keep[i] = take_rdl64(t.my_word, g + i);
        any |= q.keep[i];
      }
      if (!c.dl) {  // a required column: row r is value r
        if (!any) continue;
#pragma unroll
        for (uint32_t i = 0; i < TG_GROUP; i++) {
          q.kv[i] = q.keep[i];
          q.src[i] = r0 + i * 64u + lane;
          q.level[i] = 0;
        }
      } else {
#pragma unroll
        for (uint32_t i = 0; i < TG_GROUP; i++) {
          const uint64_t row = r0 + i * 64u + lane;
          q.level[i] = row < t.n_rows ? c.dl[row] : 0;
        }
#pragma unroll
        for (uint32_t i = 0; i < TG_GROUP; i++) {
          const bool in = r0 + i * 64u + lane < t.n_rows;
          const uint64_t vb = __ballot(in && q.level[i] == (uint8_t)c.max_def);
          q.src[i] = next + take_lanes_below(vb);
          next += (uint32_t)__popcll(vb);
          q.kv[i] = vb & q.keep[i];
        }
        if (!any) continue;
      }
      q.has = 0;
#pragma unroll
      for (uint32_t i = 0; i < TG_GROUP; i++)  // every value load stays inside the column
        q.has |= (uint32_t)(((q.kv[i] >> lane) & 1ull) && q.src[i] < c.n_values) << i;
      g += TG_GROUP;
      return true;
    }
    levels.finish();
    return false;
  }
  __device__ __forceinline__ void push_levels(const TakeGroup& q, uint32_t i) {
    if (c.out_dl) levels.push((q.keep[i] >> lane_id()) & 1ull, take_lanes_below(q.keep[i]), (uint32_t)__popcll(q.keep[i]), q.level[i]);
  }
};

template <class T, bool STAGED>
__device__ __forceinline__ void gather_fixed(const TakeColDev& c, const TakeTile& t, uint8_t* lds) {
  TakeWalk<STAGED> walk(c, t, lds);
  OutRing<sizeof(T), STAGED> out;
  out.init(lds, c.out_values, t.val0, c.cap_values);
  const T* __restrict__ values = (const T*)c.values;
  TakeGroup q;
  while (walk.group(q)) {
    T v[TG_GROUP];
#pragma unroll
    for (uint32_t i = 0; i < TG_GROUP; i++) v[i] = (q.has >> i) & 1u ? values[q.src[i]] : (T)0;
#pragma unroll
    for (uint32_t i = 0; i < TG_GROUP; i++) {
      if (!q.keep[i]) continue;
      walk.push_levels(q, i);
      out.push((q.kv[i] >> lane_id()) & 1ull, take_lanes_below(q.kv[i]), (uint32_t)__popcll(q.kv[i]), v[i]);
    }
  }
  out.finish();
}

// INT96 and FIXED_LEN_BYTE_ARRAY: every lane copies its own element, by dwords when both sides allow.
template <bool STAGED>
__device__ __forceinline__ void gather_generic(const TakeColDev& c, const TakeTile& t, uint8_t* lds) {
  TakeWalk<STAGED> walk(c, t, lds);
  const uint32_t w = c.width;
  const bool dwords = (w & 3u) == 0 && (((uintptr_t)c.values | (uintptr_t)c.out_values) & 3u) == 0;
  uint64_t out = t.val0;
  TakeGroup q;
  while (walk.group(q)) {
#pragma unroll
    for (uint32_t i = 0; i < TG_GROUP; i++) {
      if (!q.keep[i]) continue;
      walk.push_levels(q, i);
      const uint64_t dst = out + take_lanes_below(q.kv[i]);
      out += (uint32_t)__popcll(q.kv[i]);
      if (!((q.has >> i) & 1u) || dst >= c.cap_values) continue;
      const uint8_t* __restrict__ p = (const uint8_t*)c.values + q.src[i] * w;
      uint8_t* __restrict__ d = (uint8_t*)c.out_values + dst * w;
      if (dwords) {
        for (uint32_t b = 0; b < w; b += 4) gst((uint32_t*)(d + b), *(const uint32_t*)(p + b));
      } else {
        for (uint32_t b = 0; b < w; b++) gst(d + b, p[b]);
      }
    }
  }
}

// BYTE_ARRAY: the offsets go through the ring; a step's kept bytes are contiguous in the output, so the
// whole wave copies them, lane j taking output bytes j, j + 64, ... of the step and finding each one's
// value in the step's inclusive scan of the kept lengths (a long value is thus copied by all 64 lanes,
// and so is a run of short ones).
template <bool STAGED>
__device__ __forceinline__ void gather_binary(const TakeColDev& c, const TakeTile& t, uint8_t* lds) {
  TakeWalk<STAGED> walk(c, t, lds);
  OutRing<8, STAGED> offs;
  offs.init(lds, c.out_values, t.val0, c.cap_values);
  uint64_t* __restrict__ s_inc = (uint64_t*)(lds + TG_VAL_RING + TG_DL_RING);  // inclusive scan of the lengths
  uint64_t* __restrict__ s_src = s_inc + 64;                                   // source offset of the lane's value
  const int64_t* __restrict__ off = (const int64_t*)c.values;
  const int64_t lo = c.n_values ? off[0] : 0, hi = c.n_values ? off[c.n_values] : 0;
  const uint32_t lane = lane_id();
  uint64_t byte_pos = t.byte0;
  TakeGroup q;
  while (walk.group(q)) {
    uint64_t a[TG_GROUP], len[TG_GROUP];
#pragma unroll
    for (uint32_t i = 0; i < TG_GROUP; i++) {
      a[i] = len[i] = 0;
      if ((q.has >> i) & 1u) binary_span(off, q.src[i], lo, hi, a[i], len[i]);
    }
#pragma unroll
    for (uint32_t i = 0; i < TG_GROUP; i++) {
      if (!q.keep[i]) continue;
      walk.push_levels(q, i);
      const uint64_t inc = wave_incl_scan_u64(len[i]);
      const uint64_t total = take_rdl64(inc, 63);
      offs.push((q.kv[i] >> lane) & 1ull, take_lanes_below(q.kv[i]), (uint32_t)__popcll(q.kv[i]),
                (int64_t)(byte_pos + inc - len[i]));
      if (total) {
        s_inc[lane] = inc;
        s_src[lane] = a[i];
        wave_sync();
        for (uint64_t j0 = 0; j0 < total; j0 += 64) {
          const uint64_t j = j0 + lane;
          if (j >= total) continue;
          uint32_t l = 0, h = 63;  // the first lane whose inclusive sum is above j
          while (l < h) {
            const uint32_t m = (l + h) >> 1;
            if (s_inc[m] > j) h = m; else l = m + 1;
          }
          const uint64_t before = l ? s_inc[l - 1] : 0;
          const uint64_t d = byte_pos + j;
          if (d < c.cap_bytes) gst(c.out_binary + d, c.binary[s_src[l] + (j - before)]);
        }
        wave_sync();
      }
      byte_pos += total;
    }
  }
  offs.finish();
}

// ---- k_take_gather ---------------------------------------------------------------------------
template <bool STAGED>
__global__ __launch_bounds__(64 * TT_WPB) void k_take_gather(const uint64_t* __restrict__ bitmap, uint64_t n_rows,
                                                             const TakeColDev* __restrict__ cols, uint32_t n_cols,
                                                             uint64_t rows_capacity, const uint64_t* __restrict__ scratch) {
  __shared__ __align__(16) uint8_t lds_all[TT_WPB * TG_LDS_WAVE];
  const TakeScratch S = take_scratch(const_cast<uint64_t*>(scratch), (n_rows + TT_ROWS - 1) / TT_ROWS, n_cols);
  const uint64_t tile = (uint64_t)blockIdx.x * TT_WPB + wave_id();
  if (tile >= S.n_tiles) return;
  const uint32_t ci = blockIdx.y;
  if (cols[ci].kind == TAKE_MISSING) return;
  const TakeColDev c = cols[ci];
  uint8_t* lds = lds_all + wave_id() * TG_LDS_WAVE;
  TakeTile t;
  t.row0 = tile * TT_ROWS;
  t.n_rows = n_rows;
  t.my_word = tile_word(bitmap, n_rows, tile);
  if (__ballot(t.my_word != 0) == 0) return;  // the tile keeps nothing
  t.rows_capacity = rows_capacity;
  t.row_out0 = S.keep[tile];
  t.rank0 = c.dl ? S.rank[(uint64_t)ci * S.n_tiles + tile] : t.row0;
  t.val0 = c.dl ? S.kept[(uint64_t)ci * S.n_tiles + tile] : t.row_out0;
  t.byte0 = c.kind == TAKE_BINARY ? S.bytes[(uint64_t)ci * S.n_tiles + tile] : 0;
  switch (c.kind) {
    case TAKE_W1: gather_fixed<uint8_t, STAGED>(c, t, lds); break;
    case TAKE_W4: gather_fixed<uint32_t, STAGED>(c, t, lds); break;
    case TAKE_W8: gather_fixed<uint64_t, STAGED>(c, t, lds); break;
    case TAKE_GENERIC: gather_generic<STAGED>(c, t, lds); break;
    default: gather_binary<STAGED>(c, t, lds); break;
  }
}

// ---- launch ----------------------------------------------------------------------------------
hipError_t launch_take(hipStream_t st, const uint64_t* bitmap, uint64_t n_rows, const TakeColDev* d_cols, uint32_t n_cols,
                       bool any_nullable, bool any_binary, uint64_t rows_capacity, uint64_t* scratch,
                       pqg_take_counts* counts, pqg_take_result* result, bool staged) {
  const uint64_t n_tiles = filter_tiles(n_rows);
  const uint32_t wgs = (uint32_t)((n_tiles + TT_WPB - 1) / TT_WPB);
  if (n_tiles)
    hipLaunchKernelGGL(k_take_count, dim3(wgs, any_nullable ? n_cols : 1), dim3(64 * TT_WPB), 0, st, bitmap, n_rows, d_cols,
                       n_cols, scratch);
  hipLaunchKernelGGL(k_take_scan, dim3(any_nullable ? 1 + 2 * n_cols : 1), dim3(256), 0, st, scratch, n_tiles, d_cols, n_cols,
                     0u);
  if (any_binary) {
    if (n_tiles)
      hipLaunchKernelGGL(k_take_bytes, dim3(wgs, n_cols), dim3(64 * TT_WPB), 0, st, bitmap, n_rows, d_cols, n_cols, scratch);
    hipLaunchKernelGGL(k_take_scan, dim3(n_cols), dim3(256), 0, st, scratch, n_tiles, d_cols, n_cols, 1 + 2 * n_cols);
  }
  hipLaunchKernelGGL(k_take_finish, dim3(1), dim3(64), 0, st, d_cols, n_cols, n_rows, rows_capacity, scratch, counts, result);
  if (n_tiles && n_cols) {
    if (staged)
      hipLaunchKernelGGL(k_take_gather<true>, dim3(wgs, n_cols), dim3(64 * TT_WPB), 0, st, bitmap, n_rows, d_cols, n_cols,
                         rows_capacity, scratch);
    else
      hipLaunchKernelGGL(k_take_gather<false>, dim3(wgs, n_cols), dim3(64 * TT_WPB), 0, st, bitmap, n_rows, d_cols, n_cols,
                         rows_capacity, scratch);
  }
  return hipGetLastError();
}

// ==== record selection on repeated columns (pqg_take_records) ====================================
// The record bitmap is expanded into one slot bitmap per repeated column, and then the take above runs
// with every record of the table on its own bitmap and row count (TakeRecDev): a flat column on the
// caller's bitmap, a repeated column on its slot bitmap, its repetition bytes as a required 1-byte
// column on the same slot bitmap. The gathers (TakeWalk, OutRing, gather_*) are the ones above.
//   k_rec_count    per (repeated column, tile of slots): slots with rep == 0; tile 0 also the verdict
//                  on slot 0
//   k_rtake_scan   those counts: each tile's first record index, the column's record starts
//   k_rec_expand   per (repeated column, tile): 64 steps of 64 slots, lane = slot: the slot's record
//                  is the tile's base + the starts up to and including it - 1, its keep bit the
//                  record's bit; lane k keeps the word of step k and the tile's words leave as one
//                  512-byte store
//   k_rtake_count / k_rtake_scan / k_rtake_bytes / k_rtake_scan / k_rtake_finish / k_rtake_gather
// scratch (u64 words), C = n_cols, T = tiles of the largest record: five arrays of [C + 1][T] per-tile
// counts scanned in place (kept rows, rank, kept values, bytes, record starts; row C of the first is
// the caller's bitmap itself: the kept records), their totals [5][C + 1], the slot-0 flags [C], the
// slot bitmaps (whole tiles per repeated column).
enum : uint32_t { RA_KEEP = 0, RA_RANK = 1, RA_KEPT = 2, RA_BYTES = 3, RA_RECS = 4, RA_ARRAYS = 5 };

struct RecScratch {
  uint64_t *arr, *totals, *flags, *slots;
  uint64_t n_tiles;
  uint32_t n_cols;
  __host__ __device__ uint64_t* tiles(uint32_t which, uint32_t ci) const {
    return arr + ((uint64_t)which * (n_cols + 1) + ci) * n_tiles;
  }
  __host__ __device__ uint64_t* total(uint32_t which, uint32_t ci) const { return totals + which * (n_cols + 1) + ci; }
};
__host__ __device__ inline RecScratch rec_scratch(uint64_t* s, uint64_t n_tiles, uint32_t n_cols) {
  RecScratch r;
  r.n_tiles = n_tiles;
  r.n_cols = n_cols;
  r.arr = s;
  r.totals = r.arr + (uint64_t)RA_ARRAYS * (n_cols + 1) * n_tiles;
  r.flags = r.totals + RA_ARRAYS * (n_cols + 1);
  r.slots = r.flags + n_cols;
  return r;
}
uint64_t take_records_scratch_words(uint64_t max_rows, uint32_t n_cols, uint64_t slot_words) {
  return (uint64_t)RA_ARRAYS * (n_cols + 1) * (filter_tiles(max_rows) + 1) + n_cols + slot_words;
}

__device__ __forceinline__ const uint64_t* rec_bitmap(const TakeRecDev& r, const RecScratch& S) {
  return r.own_bitmap ? S.slots + r.slot_off : r.bitmap;
}

// ---- k_rec_count -----------------------------------------------------------------------------
__global__ __launch_bounds__(64 * TT_WPB) void k_rec_count(const TakeRecDev* __restrict__ recs, uint32_t n_cols,
                                                           uint64_t n_tiles, uint64_t* __restrict__ scratch) {
  const RecScratch S = rec_scratch(scratch, n_tiles, n_cols);
  const uint32_t ci = blockIdx.y;
  const uint8_t* __restrict__ rl = recs[ci].rl;
  if (!rl) return;
  const uint64_t n = recs[ci].n;
  const uint64_t tile = (uint64_t)blockIdx.x * TT_WPB + wave_id();
  if (tile * TT_ROWS >= n) return;
  const uint32_t lane = lane_id();
  const uint64_t row0 = tile * TT_ROWS;
  const bool words = ((uintptr_t)rl & 3u) == 0;
  uint32_t starts = 0;
  // a lane takes 4 slots at a time: their repetition bytes are one dword
#pragma unroll 4
  for (uint32_t k = 0; k < TT_ROWS / 256; k++) {
    const uint64_t r = row0 + 4ull * (k * 64u + lane);
    if (r >= n) continue;
    if (words && r + 4 <= n) {
      const uint32_t w = *(const uint32_t*)(rl + r);
      starts += ((w & 0xFFu) == 0) + (((w >> 8) & 0xFFu) == 0) + (((w >> 16) & 0xFFu) == 0) + ((w >> 24) == 0);
    } else {
      for (uint32_t b = 0; b < 4 && r + b < n; b++) starts += rl[r + b] == 0;
    }
  }
  uint32_t total;
  (void)wave_excl_scan_u32(starts, &total);
  if (lane == 0) {
    gst(&S.tiles(RA_RECS, ci)[tile], (uint64_t)total);
    if (tile == 0) gst(&S.flags[ci], (uint64_t)(rl[0] != 0));  // a column does not begin inside a record
  }
}

// ---- k_rtake_scan ----------------------------------------------------------------------------
// Workgroup (c, w) scans array first + w of record c over the record's own tiles. Arrays nothing was
// counted into are left alone. Record n_cols of RA_KEEP is the caller's bitmap over n_rows.
__global__ __launch_bounds__(256) void k_rtake_scan(uint64_t* __restrict__ scratch, uint64_t n_tiles,
                                                    const TakeRecDev* __restrict__ recs, uint32_t n_cols, uint64_t n_rows,
                                                    uint32_t first) {
  const RecScratch S = rec_scratch(scratch, n_tiles, n_cols);
  const uint32_t ci = blockIdx.x, which = first + blockIdx.y;
  uint64_t n = n_rows;
  if (ci < n_cols) {
    const TakeRecDev& r = recs[ci];
    if (r.c.kind == TAKE_MISSING) return;
    if ((which == RA_RANK || which == RA_KEPT) && !r.c.dl) return;
    if (which == RA_BYTES && r.c.kind != TAKE_BINARY) return;
    if (which == RA_RECS && !r.rl) return;
    n = r.n;
  } else if (which != RA_KEEP) {
    return;
  }
  const uint64_t total = block_excl_scan_u64<TS_PER>(S.tiles(which, ci), (n + TT_ROWS - 1) / TT_ROWS);
  if (threadIdx.x == 0) gst(S.total(which, ci), total);
}

// ---- k_rec_expand ----------------------------------------------------------------------------
__global__ __launch_bounds__(64 * TT_WPB) void k_rec_expand(const uint64_t* __restrict__ bitmap, uint64_t n_rows,
                                                            const TakeRecDev* __restrict__ recs, uint32_t n_cols,
                                                            uint64_t n_tiles, uint64_t* __restrict__ scratch) {
  const RecScratch S = rec_scratch(scratch, n_tiles, n_cols);
  const uint32_t ci = blockIdx.y;
  const uint8_t* __restrict__ rl = recs[ci].rl;
  if (!rl) return;
  const uint64_t n = recs[ci].n;
  const uint64_t tile = (uint64_t)blockIdx.x * TT_WPB + wave_id();
  if (tile * TT_ROWS >= n) return;
  const uint32_t lane = lane_id();
  const uint64_t row0 = tile * TT_ROWS;
  uint64_t run = S.tiles(RA_RECS, ci)[tile];  // record starts before the step
  uint64_t my_word = 0;
  constexpr uint32_t G = TG_GROUP;  // steps whose loads are issued together
  for (uint32_t g = 0; g < TT_STEPS; g += G) {
    const uint64_t r0 = row0 + g * 64u;
    if (r0 >= n) break;
    uint8_t rep[G];
    uint64_t word[G];
    uint32_t sh[G];
#pragma unroll
    for (uint32_t i = 0; i < G; i++) {
      const uint64_t slot = r0 + i * 64u + lane;
      rep[i] = slot < n ? rl[slot] : 1;
    }
#pragma unroll
    for (uint32_t i = 0; i < G; i++) {
      const bool in = r0 + i * 64u + lane < n;
      const uint64_t start = __ballot(in && rep[i] == 0);
      // starts up to and including this slot, minus 1: before the column's first start it wraps to
      // 2^64 - 1, which no n_rows exceeds
      const uint64_t rec = run + take_lanes_below(start) + ((start >> lane) & 1ull) - 1ull;
      run += (uint32_t)__popcll(start);
      const bool ok = in && rec < n_rows;
      word[i] = ok ? bitmap[rec >> 6] : 0;
      sh[i] = (uint32_t)(rec & 63u);
    }
#pragma unroll
    for (uint32_t i = 0; i < G; i++) {
      const uint64_t keep = __ballot((word[i] >> sh[i]) & 1ull);
      if (lane == g + i) my_word = keep;
    }
  }
  gst(&S.slots[recs[ci].slot_off + tile * TT_STEPS + lane], my_word);
}

// ---- k_rtake_count ---------------------------------------------------------------------------
__global__ __launch_bounds__(64 * TT_WPB) void k_rtake_count(const uint64_t* __restrict__ bitmap, uint64_t n_rows,
                                                             const TakeRecDev* __restrict__ recs, uint32_t n_cols,
                                                             uint64_t n_tiles, uint64_t* __restrict__ scratch) {
  const RecScratch S = rec_scratch(scratch, n_tiles, n_cols);
  const uint64_t tile = (uint64_t)blockIdx.x * TT_WPB + wave_id();
  const uint32_t ci = blockIdx.y;
  const uint64_t* bm = bitmap;
  uint64_t n = n_rows;
  const uint8_t* __restrict__ dl = nullptr;
  uint32_t md = 0;
  if (ci < n_cols) {
    if (recs[ci].c.kind == TAKE_MISSING) return;
    bm = rec_bitmap(recs[ci], S);
    n = recs[ci].n;
    dl = recs[ci].c.dl;
    md = (uint32_t)recs[ci].c.max_def;
  }
  if (tile * TT_ROWS >= n) return;
  uint32_t t_valid, t_kept, t_keep;
  take_count_tile(bm, n, tile, dl, md, t_valid, t_kept, t_keep);
  if (lane_id() == 0) {
    gst(&S.tiles(RA_KEEP, ci)[tile], (uint64_t)t_keep);
    if (dl) {
      gst(&S.tiles(RA_RANK, ci)[tile], (uint64_t)t_valid);
      gst(&S.tiles(RA_KEPT, ci)[tile], (uint64_t)t_kept);
    }
  }
}

// ---- k_rtake_bytes ---------------------------------------------------------------------------
__global__ __launch_bounds__(64 * TT_WPB) void k_rtake_bytes(const TakeRecDev* __restrict__ recs, uint32_t n_cols,
                                                             uint64_t n_tiles, uint64_t* __restrict__ scratch) {
  const RecScratch S = rec_scratch(scratch, n_tiles, n_cols);
  const uint64_t tile = (uint64_t)blockIdx.x * TT_WPB + wave_id();
  const uint32_t ci = blockIdx.y;
  if (recs[ci].c.kind != TAKE_BINARY) return;
  const uint64_t n = recs[ci].n;
  if (tile * TT_ROWS >= n) return;
  const TakeColDev c = recs[ci].c;
  const uint64_t sum =
      take_bytes_tile(rec_bitmap(recs[ci], S), n, tile, c, c.dl ? S.tiles(RA_RANK, ci)[tile] : tile * TT_ROWS);
  if (lane_id() == 63) gst(&S.tiles(RA_BYTES, ci)[tile], sum);
}

// ---- k_rtake_finish --------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_rtake_finish(const TakeRecDev* __restrict__ recs, uint32_t n_cols, uint64_t n_rows,
                                                     uint64_t rows_capacity, uint64_t n_tiles, uint64_t* __restrict__ scratch,
                                                     pqg_take_record_counts* __restrict__ counts,
                                                     pqg_take_result* __restrict__ result) {
  const RecScratch S = rec_scratch(scratch, n_tiles, n_cols);
  const uint32_t ci = threadIdx.x;
  const uint64_t n_keep = *S.total(RA_KEEP, n_cols);  // kept records
  bool bad = false;
  if (ci < n_cols) {
    const TakeRecDev& r = recs[ci];
    const TakeColDev& c = r.c;
    uint64_t n_records = 0, n_slots = 0, n_out = 0, n_bytes = 0;
    if (c.kind != TAKE_MISSING) {
      n_slots = *S.total(RA_KEEP, ci);
      n_out = c.dl ? *S.total(RA_KEPT, ci) : n_slots;
      if (c.dl && *S.total(RA_RANK, ci) != c.n_values) bad = true;  // slots with a value differ from n_values
      if (c.kind == TAKE_BINARY) n_bytes = *S.total(RA_BYTES, ci);
      if (n_out > c.cap_values || n_bytes > c.cap_bytes) bad = true;
      if (c.kind == TAKE_BINARY && n_out <= c.cap_values) gst((int64_t*)c.out_values + n_out, (int64_t)n_bytes);
      if (r.rl) {
        n_records = *S.total(RA_RECS, ci);
        if (n_records != n_rows) bad = true;             // the column's records are not the bitmap's
        if (r.n && S.flags[ci]) bad = true;              // slot 0 continues a record
        if (n_slots > r.cap_levels) bad = true;          // the kept slots do not fit
      } else {
        n_records = n_rows;
      }
    }
    if (n_keep > rows_capacity) bad = true;  // the kept records do not fit: counts against every column
    counts[ci].n_records = n_records;
    counts[ci].n_slots = n_slots;
    counts[ci].n_values = n_out;
    counts[ci].n_bytes = n_bytes;
  }
  const uint64_t bad_cols = __ballot(bad);
  if (threadIdx.x == 0) {
    result->n_rows = n_keep;
    const bool err = bad_cols != 0 || n_keep > rows_capacity;
    result->error = err ? PQG_ERR_INVALID_ARG : PQG_OK;
    result->error_column = bad_cols ? (int32_t)__builtin_ctzll(bad_cols) : -1;
  }
}

// ---- k_rtake_gather --------------------------------------------------------------------------
template <bool STAGED>
__global__ __launch_bounds__(64 * TT_WPB) void k_rtake_gather(const TakeRecDev* __restrict__ recs, uint32_t n_cols,
                                                              uint64_t n_tiles, const uint64_t* __restrict__ scratch) {
  __shared__ __align__(16) uint8_t lds_all[TT_WPB * TG_LDS_WAVE];
  const RecScratch S = rec_scratch(const_cast<uint64_t*>(scratch), n_tiles, n_cols);
  const uint64_t tile = (uint64_t)blockIdx.x * TT_WPB + wave_id();
  const uint32_t ri = blockIdx.y;  // n_cols columns, then the repetition bytes of the repeated ones
  if (recs[ri].c.kind == TAKE_MISSING) return;
  const uint64_t n = recs[ri].n;
  if (tile * TT_ROWS >= n) return;
  const TakeColDev c = recs[ri].c;
  const uint32_t kc = recs[ri].keep_col;
  uint8_t* lds = lds_all + wave_id() * TG_LDS_WAVE;
  TakeTile t;
  t.row0 = tile * TT_ROWS;
  t.n_rows = n;
  t.my_word = tile_word(rec_bitmap(recs[ri], S), n, tile);
  if (__ballot(t.my_word != 0) == 0) return;  // the tile keeps nothing
  t.rows_capacity = recs[ri].cap_levels;
  t.row_out0 = S.tiles(RA_KEEP, kc)[tile];
  t.rank0 = c.dl ? S.tiles(RA_RANK, ri)[tile] : t.row0;
  t.val0 = c.dl ? S.tiles(RA_KEPT, ri)[tile] : t.row_out0;
  t.byte0 = c.kind == TAKE_BINARY ? S.tiles(RA_BYTES, ri)[tile] : 0;
  switch (c.kind) {
    case TAKE_W1: gather_fixed<uint8_t, STAGED>(c, t, lds); break;
    case TAKE_W4: gather_fixed<uint32_t, STAGED>(c, t, lds); break;
    case TAKE_W8: gather_fixed<uint64_t, STAGED>(c, t, lds); break;
    case TAKE_GENERIC: gather_generic<STAGED>(c, t, lds); break;
    default: gather_binary<STAGED>(c, t, lds); break;
  }
}

// ---- launch ----------------------------------------------------------------------------------
hipError_t launch_take_records(hipStream_t st, const uint64_t* bitmap, uint64_t n_rows, const TakeRecDev* d_recs,
                               uint32_t n_cols, const TakeRecPlan& plan, uint64_t rows_capacity, uint64_t* scratch,
                               pqg_take_record_counts* counts, pqg_take_result* result, bool staged) {
  const uint64_t n_tiles = filter_tiles(plan.max_rows);
  const uint32_t wgs = (uint32_t)((n_tiles + TT_WPB - 1) / TT_WPB);
  const dim3 wg(64 * TT_WPB);
  if (plan.any_repeated) {
    if (n_tiles) hipLaunchKernelGGL(k_rec_count, dim3(wgs, n_cols), wg, 0, st, d_recs, n_cols, n_tiles, scratch);
    hipLaunchKernelGGL(k_rtake_scan, dim3(n_cols, 1), dim3(256), 0, st, scratch, n_tiles, d_recs, n_cols, n_rows,
                       (uint32_t)RA_RECS);
    if (n_tiles)
      hipLaunchKernelGGL(k_rec_expand, dim3(wgs, n_cols), wg, 0, st, bitmap, n_rows, d_recs, n_cols, n_tiles, scratch);
  }
  if (n_tiles)
    hipLaunchKernelGGL(k_rtake_count, dim3(wgs, n_cols + 1), wg, 0, st, bitmap, n_rows, d_recs, n_cols, n_tiles, scratch);
  hipLaunchKernelGGL(k_rtake_scan, dim3(n_cols + 1, plan.any_nullable ? 3 : 1), dim3(256), 0, st, scratch, n_tiles, d_recs,
                     n_cols, n_rows, (uint32_t)RA_KEEP);
  if (plan.any_binary) {
    if (n_tiles) hipLaunchKernelGGL(k_rtake_bytes, dim3(wgs, n_cols), wg, 0, st, d_recs, n_cols, n_tiles, scratch);
    hipLaunchKernelGGL(k_rtake_scan, dim3(n_cols, 1), dim3(256), 0, st, scratch, n_tiles, d_recs, n_cols, n_rows,
                       (uint32_t)RA_BYTES);
  }
  hipLaunchKernelGGL(k_rtake_finish, dim3(1), dim3(64), 0, st, d_recs, n_cols, n_rows, rows_capacity, n_tiles, scratch, counts,
                     result);
  if (n_tiles && plan.n_records) {
    if (staged)
      hipLaunchKernelGGL(k_rtake_gather<true>, dim3(wgs, plan.n_records), wg, 0, st, d_recs, n_cols, n_tiles, scratch);
    else
      hipLaunchKernelGGL(k_rtake_gather<false>, dim3(wgs, plan.n_records), wg, 0, st, d_recs, n_cols, n_tiles, scratch);
  }
  return hipGetLastError();
}

}  // namespace pqg
