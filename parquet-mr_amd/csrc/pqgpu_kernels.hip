// pqgpu_kernels.hip — CDNA4 (gfx950) kernels of the MI355X Parquet page decoder that have no file of
// their own yet: the definition / repetition levels (with BOOLEAN values of encoding RLE, which run the
// level decoder) and DELTA_BINARY_PACKED. All integer / byte work, one 64-lane wave per page: no MFMA.
//
// Semantics follow the reference reader value for value:
//   RunLengthBitPackingHybridDecoder.readInt/readNext (rle/…Decoder.java:61-109),
//   DeltaBinaryPackingValuesReader (delta/DeltaBinaryPackingValuesReader.java:59-172),
//   ColumnReaderBase.readPageV1/V2 + levels (impl/ColumnReaderBase.java:650-789).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "pqgpu_device.h"
#include "pqgpu_hybrid.h"

namespace pqg {

// ---------------------------------------------------------------------------
// Levels (def/rep) of nullable columns: ColumnReaderBase.readPageV1/readPageV2,
// RunLengthBitPackingHybridValuesReader.initFromPage (4-byte length prefix),
// newRLEIterator (V2, no prefix). Writes u8 levels, the page's non-null count
// and the data section start; value kernels run afterwards.

// BIT_PACKED (big-endian) level section [beg, end): level i = bits [i*w, (i+1)*w) MSB first
// (Packer.BIG_ENDIAN, ByteBasedBitPackingGenerator getShift msbFirst :153-159); bytes past the
// section read as 0 (ByteBitPackingValuesReader.readMore :49-57). 16 slots per lane, no errors.
__device__ uint32_t decode_levels_be(rsrc_t rs, uint32_t beg, uint32_t end, int w, uint32_t N, uint8_t* out,
                                     uint32_t max_def, bool count_nonnull, uint32_t* nonnull, int* err_code) {
  const uint32_t lane = lane_id();
  uint32_t cnt = 0;
  const uint32_t mask = (1u << w) - 1u;  // w <= 8 (max level <= 254)
  for (uint32_t s0 = 16u * lane; s0 < N; s0 += 16u * WAVE) {
    uint64_t wlo = 0, whi = 0;
    for (uint32_t j = 0; j < 16 && s0 + j < N; j++) {
      const uint64_t bit = (uint64_t)(s0 + j) * (uint32_t)w;
      const uint32_t a = beg + (uint32_t)(bit >> 3);
      uint32_t x = 0;  // bytes a .. a+3, big endian, 0 past the section
#pragma unroll
      for (uint32_t q = 0; q < 4; q++) {
        const uint32_t bq = a + q < end ? (ld32(rs, (a + q) & ~3u) >> (((a + q) & 3u) * 8u)) & 0xFFu : 0u;
        x = (x << 8) | bq;
      }
      const uint32_t v = (x >> (32u - (uint32_t)(bit & 7u) - (uint32_t)w)) & mask;
      if (count_nonnull && v == max_def) cnt++;
      if (j < 8) wlo |= (uint64_t)v << (8 * j);
      else whi |= (uint64_t)v << (8 * (j - 8));
    }
    if (out)
      for (uint32_t j = 0; j < 16 && s0 + j < N; j++)
        gst(out + s0 + j, (uint8_t)((j < 8 ? wlo >> (8 * j) : whi >> (8 * (j - 8))) & 0xFFu));
  }
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
  if (nonnull) *nonnull = cnt;
  *err_code = 0;
  return N;
}

// Per-wave LDS of the level decoder: the page segment, the binary-lifting tables of one 256-byte
// window's header chain, the window's pre-decoded headers, and the window's run table.
// A run of a level section takes at least 2 bytes (w >= 1: header + value byte, or header + >= 1
// group byte), so a window's chain holds at most 128 runs.
constexpr uint32_t LV_RUNS = 128;
struct LevelWaveLds {
  uint8_t seg[SEG_BYTES];     // page bytes [seg_lo, seg_lo + SEG_BYTES)
  uint8_t J[6][256];          // J[r][p]: window offset of the 2^r-th header after p; 0: the chain stops first
  uint32_t ecnt[256];         // position p as a header: run count | packed << 31
  uint16_t eval[256];         // RLE: value (saturated to 255); PACKED: data start - window start
  uint32_t r_start[LV_RUNS];  // first slot of run k of the window
  uint32_t r_pay[LV_RUNS];    // RLE: value (saturated to 255); PACKED: 0x80000000 | data byte position
  uint32_t r_end[LV_RUNS];    // PACKED: end of the bytes read for the run (truncated final group)
  // the partial 16-slot tile a window's expansion ended on (more windows follow): its levels wait
  // here for the next window's part instead of going out as byte stores (expand_level_tiles)
  uint32_t carry[4];
  int32_t carry_s0;       // tile start (slot index relative to the output base)
  uint32_t carry_j;       // valid bytes [carry_j & 255, carry_j >> 8); 0: none
};

// Levels of the runs rs[0 .. n_run) covering slots [s_lo, s_hi) -> out (u8), 16 slots per lane
// with 16-byte stores where the tile is inside [s_lo, s_hi); counts slots == max_def.
// Packed bytes come from the wave's LDS segment of the page when it holds them (a global load
// here would wait for the tile stores before it: vmcnt counts stores).
// Byte mask of bytes [jb, je) (clamped to the tile) in dword i of a 16-byte tile.
__device__ __forceinline__ uint32_t tile_byte_mask(int32_t jb, int32_t je, int32_t i) {
  const int32_t lo = jb - 4 * i < 0 ? 0 : (jb - 4 * i > 4 ? 4 : jb - 4 * i);
  const int32_t hi = je - 4 * i < 0 ? 0 : (je - 4 * i > 4 ? 4 : je - 4 * i);
  const uint32_t mh = hi >= 4 ? 0xFFFFFFFFu : (1u << (8 * hi)) - 1u;
  const uint32_t ml = lo >= 4 ? 0xFFFFFFFFu : (1u << (8 * lo)) - 1u;
  return mh & ~ml;
}

// Run holding slot lo_s: the largest a < n_run (<= 256) with r_start[a] <= lo_s (r_start ascending,
// r_start[0] <= lo_s). Eight fixed steps with unconditional LDS reads instead of this divergent
// bisection loop (whose exec bookkeeping runs on the scalar unit) measured C3 10.01 -> 10.10 ms,
// C5 2.17 -> 2.19 ms (profiles/r02/lv_ab) and were removed.
// Store one tile's levels [j0, j1) (out + s0 is 16-byte aligned): the first tile of a window range merges
// the carried part of the same tile (the previous window ended inside it, so carry_j's end is j0); a tile
// the range ends inside, with more windows to come, becomes the carry; whole tiles go out as one
// 16-byte store, the tiles at the page's edges byte by byte (other pages own the rest).
__device__ __forceinline__ void level_tile_out(LevelWaveLds& L, uint8_t* out, int64_t s0, uint32_t (&acc)[4], int32_t j0,
                                               int32_t j1, uint32_t s_lo, uint32_t s_hi, bool more) {
  if (s0 + j0 == (int64_t)s_lo && j0 > 0) {
    const uint32_t cj = L.carry_j;
    if (cj && L.carry_s0 == (int32_t)s0 && (int32_t)(cj >> 8) == j0) {
#pragma unroll
      for (int32_t c = 0; c < 4; c++) {
        const uint32_t mk = tile_byte_mask(j0, 16, c);
        acc[c] = (acc[c] & mk) | (L.carry[c] & ~mk);
      }
      j0 = (int32_t)(cj & 255u);
      L.carry_j = 0;
    }
  }
  if (more && j1 < 16 && s0 + j1 == (int64_t)s_hi) {
#pragma unroll
    for (int32_t c = 0; c < 4; c++) L.carry[c] = acc[c];
    L.carry_s0 = (int32_t)s0;
    L.carry_j = (uint32_t)j0 | ((uint32_t)j1 << 8);
    return;
  }
  uint8_t* o = out + s0;
  if (j0 == 0 && j1 == 16) {
    gst((u32x4*)o, u32x4{acc[0], acc[1], acc[2], acc[3]});
  } else {
#pragma unroll
    for (int32_t j = 0; j < 16; j++)
      if (j >= j0 && j < j1) gst(o + j, (uint8_t)(acc[j >> 2] >> (8 * (j & 3))));
  }
}

// A carry left when the section's decode stopped early (an error): its levels go out byte by byte.
__device__ __forceinline__ void level_carry_flush(LevelWaveLds& L, uint8_t* out) {
  wave_sync();
  const uint32_t cj = L.carry_j;
  if (cj && out && lane_id() < 16u) {
    const uint32_t j = lane_id();
    if (j >= (cj & 255u) && j < (cj >> 8)) gst(out + L.carry_s0 + (int32_t)j, (uint8_t)(L.carry[j >> 2] >> (8u * (j & 3u))));
  }
  wave_sync();
  if (lane_id() == 0) L.carry_j = 0;
  wave_sync();
}

__device__ __forceinline__ uint32_t level_run_of(const LevelWaveLds& L, uint32_t n_run, uint32_t lo_s) {
  uint32_t a = 0, b = n_run;
  while (b - a > 1) {
    const uint32_t mid = (a + b) >> 1;
    if (L.r_start[mid] <= lo_s) a = mid;
    else b = mid;
  }
  return a;
}

// Bit width WB (1..8) specialisation of expand_level_runs: per tile piece (the part of one run
// inside the lane's 16 slots) the 16 levels are formed without a per-slot loop: an RLE piece is
// its value replicated, a packed piece is 24 bytes at the piece's bit offset, shifted once, then
// 16 bit fields at compile-time positions; a byte mask merges the piece into the tile.
template <int WB>
__device__ __forceinline__ void expand_level_tiles(LevelWaveLds& L, const PreWin& win, uint32_t n_run,
                                                   uint32_t s_lo, uint32_t s_hi, uint8_t* out, uint32_t max_def,
                                                   bool count_nonnull, uint32_t& cnt, bool more) {
  const rsrc_t rs = win.rs;
  const uint32_t lane = lane_id();
  const int64_t mis = out ? (int64_t)((uintptr_t)out & 15u) : 0;
  // width 1 with every RLE value 0 or 1 (the usual flat optional column): the tile's 16 levels
  // are built as a 16-bit mask (3 operations per piece) and spread to bytes once per tile
  bool bits_ok = false;
  if constexpr (WB == 1) {
    bool bad = false;
    for (uint32_t i = lane; i < n_run; i += WAVE) {
      const uint32_t p = L.r_pay[i];
      bad |= !(p & 0x80000000u) && p > 1u;
    }
    bits_ok = !__ballot(bad);
  }
  for (int64_t t = (((int64_t)s_lo + mis) & ~(int64_t)15) - mis; t < (int64_t)s_hi; t += 16 * WAVE) {
    const int64_t s0 = t + 16 * (int64_t)lane;
    if (s0 + 16 <= (int64_t)s_lo || s0 >= (int64_t)s_hi) continue;
    const uint32_t lo_s = (uint32_t)(s0 > (int64_t)s_lo ? s0 : (int64_t)s_lo);
    const uint32_t hi_s = (uint32_t)(s0 + 16 < (int64_t)s_hi ? s0 + 16 : (int64_t)s_hi);
    const uint32_t a = level_run_of(L, n_run, lo_s);
    uint32_t acc[4] = {0u, 0u, 0u, 0u};
    uint32_t cur = lo_s, k = a;
    if (WB == 1 && bits_ok) {
      uint32_t m = 0;  // bit j: level of tile slot j
      while (cur < hi_s) {
        const uint32_t st = L.r_start[k], pay = L.r_pay[k];
        const uint32_t re = k + 1 < n_run ? L.r_start[k + 1] : s_hi;
        const uint32_t stop = hi_s < re ? hi_s : re;
        const uint32_t jb = cur - (uint32_t)s0, je = stop - (uint32_t)s0;
        const uint32_t pm = ((1u << je) - 1u) & ~((1u << jb) - 1u);
        uint32_t bits;
        if (!(pay & 0x80000000u)) {
          bits = pay ? 0xFFFFu : 0u;
        } else {
          // 32 bits of the run's data from slot cur on (bytes at or past the read end are 0)
          const uint32_t rlo = pay & 0x7FFFFFFFu, rhi = L.r_end[k];
          const uint32_t bp = cur - st, byte0 = rlo + (bp >> 3), a4 = byte0 & ~3u;
          uint32_t y0, y1;
          if (seg_has(win, a4, 8u)) {
            y0 = seg32(win, a4);
            y1 = seg32(win, a4 + 4u);
          } else {
            y0 = ld32(rs, a4);
            y1 = ld32(rs, a4 + 4u);
          }
          const int32_t k0 = (int32_t)rhi - (int32_t)a4, k1 = k0 - 4;
          y0 &= k0 >= 4 ? 0xFFFFFFFFu : (k0 <= 0 ? 0u : (1u << (8 * k0)) - 1u);
          y1 &= k1 >= 4 ? 0xFFFFFFFFu : (k1 <= 0 ? 0u : (1u << (8 * k1)) - 1u);
          const uint32_t z = __builtin_amdgcn_alignbyte(y1, y0, byte0 & 3u);
          bits = (z >> (bp & 7u)) << jb;
        }
        m = (m & ~pm) | (bits & pm);
        cur = stop;
        k++;
      }
#pragma unroll
      for (uint32_t c = 0; c < 4; c++) acc[c] = (((m >> (4u * c)) & 0xFu) * 0x204081u) & 0x01010101u;
      const uint32_t j0 = lo_s - (uint32_t)s0, j1 = hi_s - (uint32_t)s0;
      const uint32_t jm = ((1u << j1) - 1u) & ~((1u << j0) - 1u);
      if (count_nonnull) cnt += max_def == 1 ? __builtin_popcount(m & jm) : max_def == 0 ? __builtin_popcount(~m & jm) : 0;
      if (out) level_tile_out(L, out, s0, acc, (int32_t)j0, (int32_t)j1, s_lo, s_hi, more);
      continue;
    }
    while (cur < hi_s) {
      const uint32_t st = L.r_start[k], pay = L.r_pay[k];
      const uint32_t re = k + 1 < n_run ? L.r_start[k + 1] : s_hi;
      const uint32_t stop = hi_s < re ? hi_s : re;
      const int32_t jb = (int32_t)(cur - (uint32_t)s0), je = (int32_t)(stop - (uint32_t)s0);
      uint32_t v[4];
      if (!(pay & 0x80000000u)) {
        const uint32_t rep = pay * 0x01010101u;  // pay <= 255 (saturated)
        v[0] = v[1] = v[2] = v[3] = rep;
      } else {
        // bit offset of tile slot 0 from the run's data start (negative when the run starts
        // inside the tile: those slots are masked off below)
        const uint32_t rlo = pay & 0x7FFFFFFFu, rhi = L.r_end[k];
        const int64_t base = ((int64_t)cur - (int64_t)st - (int64_t)jb) * WB;
        const int64_t byte0 = (int64_t)rlo + (base >> 3);
        const uint32_t bsh = (uint32_t)(base & 7);
        const int64_t a4 = byte0 & ~(int64_t)3;  // may be < 0 near the page start (masked slots only)
        const uint32_t sb = (uint32_t)(byte0 & 3);
        uint32_t y[6];
        if (a4 >= 0 && seg_has(win, (uint32_t)a4, 24u)) {
#pragma unroll
          for (uint32_t c = 0; c < 6; c++) y[c] = seg32(win, (uint32_t)a4 + 4u * c);
        } else {
#pragma unroll
          for (uint32_t c = 0; c < 6; c++) y[c] = a4 + 4 * (int64_t)c >= 0 ? ld32(rs, (uint32_t)(a4 + 4 * (int64_t)c)) : 0u;
        }
        // bytes at or past the run's read end are 0 (readNext :96-99: truncated final group)
#pragma unroll
        for (uint32_t c = 0; c < 6; c++) {
          const int64_t kp = (int64_t)rhi - (a4 + 4 * (int64_t)c);
          y[c] &= kp >= 4 ? 0xFFFFFFFFu : (kp <= 0 ? 0u : (1u << (8 * kp)) - 1u);
        }
        uint32_t z[5], D[5];
#pragma unroll
        for (uint32_t c = 0; c < 5; c++) z[c] = __builtin_amdgcn_alignbyte(y[c + 1], y[c], sb);
#pragma unroll
        for (uint32_t c = 0; c < 4; c++) D[c] = __builtin_amdgcn_alignbit(z[c + 1], z[c], bsh);
        D[4] = z[4] >> bsh;
        v[0] = v[1] = v[2] = v[3] = 0u;
#pragma unroll
        for (uint32_t q = 0; q < 16; q++) {
          constexpr uint32_t M = (1u << WB) - 1u;
          const uint32_t bp = q * WB, wi = bp >> 5, bo = bp & 31u;
          const uint32_t f = (bo + WB <= 32u ? (D[wi] >> bo) : __builtin_amdgcn_alignbit(D[wi + 1], D[wi], bo)) & M;
          v[q >> 2] |= f << (8u * (q & 3u));
        }
      }
#pragma unroll
      for (int32_t c = 0; c < 4; c++) {
        const uint32_t m = tile_byte_mask(jb, je, c);
        acc[c] = (acc[c] & ~m) | (v[c] & m);
      }
      cur = stop;
      k++;
    }
    const int32_t j0 = (int32_t)(lo_s - (uint32_t)s0), j1 = (int32_t)(hi_s - (uint32_t)s0);
    if (count_nonnull) {
      // bytes == max_def inside [j0, j1): zero bytes of acc ^ max_def (per-byte test, no carries)
      const uint32_t rep = max_def * 0x01010101u;
#pragma unroll
      for (int32_t c = 0; c < 4; c++) {
        const uint32_t y = acc[c] ^ rep;
        const uint32_t nz = ((y & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | y;  // bit 7 of a byte: byte != 0
        cnt += (uint32_t)__builtin_popcount(~nz & 0x80808080u & tile_byte_mask(j0, j1, c));
      }
    }
    if (out) level_tile_out(L, out, s0, acc, j0, j1, s_lo, s_hi, more);
  }
}

__device__ __forceinline__ void expand_level_runs_generic(const LevelWaveLds& L, const PreWin& win, uint32_t n_run,
                                                          uint32_t s_lo, uint32_t s_hi, int w, uint8_t* out,
                                                          uint32_t max_def, bool count_nonnull, uint32_t& cnt);

// WB = 1..4: the specialised tile expansion; WB = 0: any width. (A level image in LDS written one run
// per lane, then read 16 slots per lane, measured no faster on C3: 0.990 vs 0.981 ms, profiles/r05/lv_image.)
template <int WB>
__device__ __forceinline__ void expand_level_runs(LevelWaveLds& L, const PreWin& win, uint32_t n_run,
                                                  uint32_t s_lo, uint32_t s_hi, int w, uint8_t* out,
                                                  uint32_t max_def, bool count_nonnull, uint32_t& cnt, bool more) {
  if constexpr (WB > 0) expand_level_tiles<WB>(L, win, n_run, s_lo, s_hi, out, max_def, count_nonnull, cnt, more);
  else expand_level_runs_generic(L, win, n_run, s_lo, s_hi, w, out, max_def, count_nonnull, cnt);
}

__device__ __forceinline__ void expand_level_runs_generic(const LevelWaveLds& L, const PreWin& win, uint32_t n_run,
                                                          uint32_t s_lo, uint32_t s_hi, int w, uint8_t* out,
                                                          uint32_t max_def, bool count_nonnull, uint32_t& cnt) {
  const rsrc_t rs = win.rs;
  const uint32_t lane = lane_id();
  const int64_t mis = out ? (int64_t)((uintptr_t)out & 15u) : 0;
  const uint32_t wmask = w >= 32 ? 0xFFFFFFFFu : (1u << w) - 1u;
  for (int64_t t = (((int64_t)s_lo + mis) & ~(int64_t)15) - mis; t < (int64_t)s_hi; t += 16 * WAVE) {
    const int64_t s0 = t + 16 * (int64_t)lane;
    if (s0 + 16 <= (int64_t)s_lo || s0 >= (int64_t)s_hi) continue;
    const uint32_t lo_s = (uint32_t)(s0 > (int64_t)s_lo ? s0 : (int64_t)s_lo);
    const uint32_t hi_s = (uint32_t)(s0 + 16 < (int64_t)s_hi ? s0 + 16 : (int64_t)s_hi);
    // run holding lo_s: last k with r_start[k] <= lo_s
    const uint32_t a = level_run_of(L, n_run, lo_s);
    uint64_t wlo = 0, whi = 0;
    uint32_t cur = lo_s, k = a;
    while (cur < hi_s) {
      const uint32_t st = L.r_start[k], pay = L.r_pay[k];
      const uint32_t re = k + 1 < n_run ? L.r_start[k + 1] : s_hi;
      const uint32_t stop = hi_s < re ? hi_s : re;
      if (!(pay & 0x80000000u)) {
        for (uint32_t q = cur; q < stop; q++) {
          const uint32_t j = q - (uint32_t)s0;
          if (j < 8) wlo |= (uint64_t)pay << (8 * j);
          else whi |= (uint64_t)pay << (8 * (j - 8));
        }
      } else if (w > 0) {
        const uint32_t rlo = pay & 0x7FFFFFFFu, rhi = L.r_end[k];
        const uint64_t bit0 = (uint64_t)(cur - st) * (uint32_t)w;
        const uint32_t a0 = rlo + (uint32_t)(bit0 >> 3);
        uint64_t x[3];
        const bool in_seg = seg_has(win, a0 & ~3u, 28u);
        uint32_t dw[7];
        if (in_seg) {
#pragma unroll
          for (uint32_t c = 0; c < 7; c++) dw[c] = seg32(win, (a0 & ~3u) + 4u * c);
        }
#pragma unroll
        for (uint32_t c = 0; c < 3; c++) {
          const uint32_t ac = a0 + 8u * c;
          const uint32_t sb = a0 & 3u;
          const uint64_t v = in_seg ? ((uint64_t)__builtin_amdgcn_alignbyte(dw[2 * c + 1], dw[2 * c], sb) |
                                       ((uint64_t)__builtin_amdgcn_alignbyte(dw[2 * c + 2], dw[2 * c + 1], sb) << 32))
                                    : ld8_any(rs, ac);
          const int64_t keep = (int64_t)rhi - (int64_t)ac;  // bytes past the run's read end are 0 (:96-99)
          x[c] = keep >= 8 ? v : (keep <= 0 ? 0 : (v & ((1ull << (8 * keep)) - 1ull)));
        }
        for (uint32_t q = cur; q < stop; q++) {
          const uint32_t sh = (uint32_t)(bit0 & 7u) + (q - cur) * (uint32_t)w;
          const uint32_t c = sh >> 6, o = sh & 63u;
          const uint64_t lo64 = c == 0 ? x[0] : (c == 1 ? x[1] : x[2]);
          const uint64_t hi64 = c == 0 ? x[1] : (c == 1 ? x[2] : 0ull);
          const uint64_t f = o ? ((lo64 >> o) | (hi64 << (64u - o))) : lo64;
          uint32_t v = (uint32_t)f & wmask;
          v = v > 255u ? 255u : v;
          const uint32_t j = q - (uint32_t)s0;
          if (j < 8) wlo |= (uint64_t)v << (8 * j);
          else whi |= (uint64_t)v << (8 * (j - 8));
        }
      }
      cur = stop;
      k++;
    }
    const uint32_t j0 = lo_s - (uint32_t)s0, j1 = hi_s - (uint32_t)s0;
    if (count_nonnull)
      for (uint32_t j = j0; j < j1; j++)
        cnt += (uint32_t)((j < 8 ? wlo >> (8 * j) : whi >> (8 * (j - 8))) & 0xFFu) == max_def ? 1u : 0u;
    if (out) {
      uint8_t* o = out + s0;
      if (j0 == 0 && j1 == 16) {
        typedef uint64_t v2 __attribute__((ext_vector_type(2)));
        gst((v2*)o, v2{wlo, whi});
      } else {
        for (uint32_t j = j0; j < j1; j++) gst(o + j, (uint8_t)((j < 8 ? wlo >> (8 * j) : whi >> (8 * (j - 8))) & 0xFFu));
      }
    }
  }
}

// RLE / bit-packed level section [beg, end) (RunLengthBitPackingHybridDecoder over the section)
// -> out[0 .. N), one 256-byte window at a time:
//   1. pre-decode: every lane parses a run header at each of its 4 byte positions as if one started
//      there (count, value / data start, successor position; branch-free up to 4-byte varints);
//   2. binary lifting: J[0][p] = the successor of p inside the window (0: the chain leaves the window
//      or p is not a fast-path header), J[r+1] = J[r] o J[r] — built only until the chain from the
//      window's entry position ends (J[r][entry] == 0), at most 5 rounds of 4 LDS byte gathers per lane;
//   3. lane t takes the chain's t-th header directly, c_t = J^t(entry), from the bits of t (one LDS
//      gather per bit): no per-position marks, no compaction; a chain of more than 64 headers is taken
//      64 at a time;
//   4. lane t reads its header's pre-decoded count / payload, a saturating DPP scan gives the runs'
//      first slots, lane t writes run t of the window's run table, and the tile expansion writes
//      the slots the window's runs cover.
// Replaced (round 4) the pointer doubling over all 256 positions with a scatter of chain marks per
// round and a ballot compaction of the marked headers (C3: ~15 VALU + 7 SALU per run, 1.05 ms).
// Returns the slots decoded before an error (N when none) and sets *err_code.
template <int WB>
__device__ __forceinline__ uint32_t decode_levels_bl(LevelWaveLds& L, rsrc_t rs, uint32_t beg, uint32_t end, int w,
                                                     uint32_t N, uint8_t* out, uint32_t max_def, bool count_nonnull,
                                                     uint32_t* nonnull, int* err_code, uint64_t* diag = nullptr) {
  const uint32_t lane = lane_id();
  typedef uint32_t __attribute__((may_alias)) u32a;
#ifdef PQG_DIAG
  uint64_t dt[5] = {0, 0, 0, 0, 0}, dm = __builtin_amdgcn_s_memtime();
#define LV_TICK(k) do { if (diag) { const uint64_t t_ = __builtin_amdgcn_s_memtime(); dt[k] += t_ - dm; dm = t_; } } while (0)
#else
#define LV_TICK(k) do { } while (0)
#endif
  PreWin win;
  win.rs = rs;
  win.seg = L.seg;
  win.seg_lo = 0xFFFFF000u;  // nothing staged yet
  uint32_t pos = beg, produced = 0, cnt = 0;
  int code = 0;
  if (lane == 0) L.carry_j = 0;
  wave_sync();
  while (true) {
    pos = uni(pos);
    produced = uni(produced);
    if (produced >= N) break;
    if (pos >= end) { code = PQG_ERR_RLE_PAST_END; break; }  // readNext :81
    const uint32_t B = pos & ~3u;
    predecode(win, B, w);  // stages [B, B + 264) in the segment when needed
    uint32_t js = 0, nn[4], slowm = 0, inm = 0, ec[4], ev[4];
#pragma unroll
    for (uint32_t b = 0; b < 4; b++) {
      const uint32_t p = B + 4u * lane + b;
      const uint32_t f = (win.flg >> (8u * b)) & 0xFFu;
      const uint32_t hl = f >> 2;
      const uint32_t nx = win.nxt[b];
      const bool in = p < end;
      const bool slow = in && ((f & 2u) || p + hl > end || (!(f & 1u) && nx > end));
      nn[b] = (f & 1u) ? (nx < end ? nx : end) : nx;  // packed: readFully of what is left
      const uint32_t j = (!in || slow || nn[b] - B >= 256u) ? 0u : nn[b] - B;
      js |= j << (8u * b);
      slowm |= (slow ? 1u : 0u) << b;
      inm |= (in ? 1u : 0u) << b;
      ec[b] = win.cnt[b] | ((f & 1u) << 31);
      ev[b] = (f & 1u) ? ((win.val[b] - B) & 0xFFFFu) : (win.val[b] > 255u ? 255u : win.val[b]);
    }
    wave_sync();  // the previous window's chain / expansion reads are done
    ((u32a*)L.J[0])[lane] = js;
    LV_TICK(0);
    *(u32x4*)(L.ecnt + 4u * lane) = u32x4{ec[0], ec[1], ec[2], ec[3]};
    ((u32a*)L.eval)[2u * lane] = ev[0] | (ev[1] << 16);
    ((u32a*)L.eval)[2u * lane + 1u] = ev[2] | (ev[3] << 16);
    wave_sync();
    // J[r + 1] = J[r] o J[r] until the 2^r-th successor of the entry is missing (chain <= 2^r)
    uint32_t s = pos - B;  // chain entry (window offset)
    uint32_t nt = 1;       // tables built
    {
      uint32_t cur = js;
#pragma unroll 1
      for (uint32_t r = 0; r < 5u; r++) {
        if (uni((uint32_t)L.J[r][s]) == 0u) break;
        uint32_t nx2 = 0;
#pragma unroll
        for (uint32_t b = 0; b < 4; b++) {
          const uint32_t j = (cur >> (8u * b)) & 0xFFu;
          const uint32_t jj = L.J[r][j];
          nx2 |= (j ? jj : 0u) << (8u * b);
        }
        ((u32a*)L.J[r + 1])[lane] = nx2;
        cur = nx2;
        nt = r + 2;
        wave_sync();
      }
    }
    nt = uni(nt);
    LV_TICK(1);
    const uint32_t w0 = produced;
    uint32_t n_runs = 0, q = s;
    while (true) {  // batches of at most 64 chain headers
      // lane t: c_t = J^t(s)
      uint32_t c = s;
      bool ok = true;
#pragma unroll 1
      for (uint32_t r = 0; r < nt; r++) {
        const uint32_t x = L.J[r][c];
        const bool take = (lane >> r) & 1u;
        ok = ok && (!take || x != 0u);
        c = take ? x : c;
      }
      ok = ok && lane < (1u << nt);  // nt == 6: every lane
      const uint64_t vm = __ballot(ok);
      const uint32_t n = uni((uint32_t)__builtin_popcountll(vm));  // a prefix of the lanes
      q = uni(rdl(c, n - 1u));
      const uint32_t nq = uni((uint32_t)L.J[0][q]);
      // the batch's last header q: a run unless the chain stops at it (slow / past the section)
      const uint32_t ql = q >> 2, qb = q & 3u;
      const bool last_run = nq != 0u || (!((rdl(slowm, ql) >> qb) & 1u) && ((rdl(inm, ql) >> qb) & 1u));
      const uint32_t n_v = last_run ? n : n - 1u;
      const uint32_t cap = N - produced;
      uint32_t cc = 0, payload = 0, rend = 0;
      if (lane < n_v) {
        const uint32_t e = L.ecnt[c], v = L.eval[c];
        const bool pk = e >> 31;
        const uint32_t raw = e & 0x7FFFFFFFu;
        cc = (!pk && raw == 0u) ? cap : raw;  // Java: currentCount goes negative, the value repeats forever
        cc = cc < cap ? cc : cap;
        if (pk) {
          const uint32_t d = B + v;  // data start
          const uint64_t e2 = (uint64_t)d + (uint64_t)(raw >> 3) * (uint32_t)w;
          rend = e2 < (uint64_t)end ? (uint32_t)e2 : end;
          payload = 0x80000000u | d;
        } else {
          payload = v;
        }
      }
      const uint32_t inc = wave_incl_scan_sat(cc, cap);
      uint32_t st = __shfl_up(inc, 1);
      if (lane == 0) st = 0;
      const uint32_t total = uni(rdl(inc, WAVE - 1));
      const bool em = cc > 0u && st < cap;
      const uint32_t n_em = uni((uint32_t)__builtin_popcountll(__ballot(em)));
      if (em) {
        const uint32_t k = n_runs + lane;
        L.r_start[k] = produced + st;
        L.r_pay[k] = payload;
        L.r_end[k] = rend;
      }
      n_runs = uni(n_runs + n_em);
      produced = uni(produced + total);
      if (produced >= N || nq == 0u) break;
      s = nq;  // the chain goes on inside this window: next batch
    }
    wave_sync();
    LV_TICK(2);
    if (n_runs) expand_level_runs<WB>(L, win, n_runs, w0, produced, w, out, max_def, count_nonnull, cnt, produced < N);
    LV_TICK(3);
#ifdef PQG_DIAG
    dt[4] += 1;
#endif
    if (produced >= N) break;
    // continue after the window's last chain header q
    const uint32_t ql = q >> 2, qb = q & 3u;
    const uint32_t q_slow = (rdl(slowm, ql) >> qb) & 1u;
    const uint32_t q_in = (rdl(inm, ql) >> qb) & 1u;
    if (!q_in) {
      pos = B + q;  // at or past the section end: RLE_PAST_END next
    } else if (!q_slow) {
      pos = pick4(nn, qb, ql);  // leaves the window
    } else {
      // scalar re-decode of the header at q (readNext :80-109)
      pos = B + q;
      uint32_t hl, m, nxs, vv;
      uint64_t cnt64;
      code = slow_header_g([&](uint32_t p) { return wbyte(win, p); }, pos, end, w, hl, m, cnt64, vv, nxs);
      if (code) break;
      if (m == 0 && nxs > end) { code = PQG_ERR_EOF; break; }
      uint64_t c64 = cnt64;
      const uint32_t left = N - produced;
      if (m == 0 && c64 == 0) c64 = left;
      const uint32_t take = c64 < left ? (uint32_t)c64 : left;
      const uint32_t rd_end = m ? (nxs < end ? nxs : end) : nxs;
      wave_sync();
      if (lane == 0) {
        L.r_start[0] = produced;
        L.r_pay[0] = m ? (0x80000000u | vv) : (vv > 255u ? 255u : vv);
        L.r_end[0] = rd_end;
      }
      wave_sync();
      expand_level_runs<WB>(L, win, 1, produced, produced + take, w, out, max_def, count_nonnull, cnt, produced + take < N);
      produced += take;
      pos = rd_end;
    }
  }
  if (WB > 0) level_carry_flush(L, out);
#ifdef PQG_DIAG
  if (diag && lane == 0)
    for (int k = 0; k < 5; k++) diag[k] = dt[k];
#endif
#undef LV_TICK
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
  if (nonnull) *nonnull = cnt;
  *err_code = code;
  return code ? produced : N;
}

// decode_levels_bl with the tile expansion specialised for the section's bit width.
__device__ __forceinline__ uint32_t decode_levels_w(LevelWaveLds& L, rsrc_t rs, uint32_t beg, uint32_t end, int w,
                                                    uint32_t N, uint8_t* out, uint32_t max_def, bool count_nonnull,
                                                    uint32_t* nonnull, int* err_code, uint64_t* diag = nullptr) {
  switch (w) {
    case 1: return decode_levels_bl<1>(L, rs, beg, end, w, N, out, max_def, count_nonnull, nonnull, err_code, diag);
    case 2: return decode_levels_bl<2>(L, rs, beg, end, w, N, out, max_def, count_nonnull, nonnull, err_code, diag);
    case 3: return decode_levels_bl<3>(L, rs, beg, end, w, N, out, max_def, count_nonnull, nonnull, err_code, diag);
    case 4: return decode_levels_bl<4>(L, rs, beg, end, w, N, out, max_def, count_nonnull, nonnull, err_code, diag);
    default: return decode_levels_bl<0>(L, rs, beg, end, w, N, out, max_def, count_nonnull, nonnull, err_code, diag);
  }
}

// 5 waves per SIMD (LDS 6.9 KiB per wave, <= 102 VGPRs): 40,000 C3 pages in 8 rounds instead of 10
__global__ __launch_bounds__(64 * WPB) __attribute__((amdgpu_waves_per_eu(5))) void k_levels(const uint8_t* __restrict__ bytes, uint64_t n_bytes,
                                                PageWork* __restrict__ work, const ColumnDev* __restrict__ cols,
                                                const int32_t* __restrict__ list, int n_list, uint64_t* err,
                                                ErrCount err_count, uint32_t* hint_bad) {
  // hint_bad != nullptr: the plan runs on the V2 header null counts (PQG_PAGE_NULL_COUNT), which the
  // host already put in n_values / data_begin / out_offset and the value kernels are reading beside this
  // kernel; nothing of the page's work entry is written here, the true count is only compared, and a
  // mismatch or any level error raises hint_bad (err_count's epoch): pqg_sync then re-runs level-first
  __shared__ __attribute__((aligned(16))) LevelWaveLds lvl_lds[WPB];
  const int page = wave_page(list, n_list);
  if (page < 0) return;
  LevelWaveLds& LL = lvl_lds[wave_id()];
  PageWork pw = work[page];
  const ColumnDev cd = cols[pw.column];
  const uint32_t lane = lane_id();
  Window win;
  win.rs = make_rsrc(bytes + pw.base, n_bytes - pw.base);
  const uint32_t size = uni(pw.size);
  const uint32_t nslots = uni(pw.num_slots);
  const int wr = cd.max_rep ? 32 - __builtin_clz((uint32_t)cd.max_rep) : 0;
  const int wd = cd.max_def ? 32 - __builtin_clz((uint32_t)cd.max_def) : 0;
  uint32_t rl_beg = 0, rl_end = 0, dl_beg = 0, dl_end = 0, data_beg = 0;
  bool rl_be = false, dl_be = false;  // V1 BIT_PACKED (big-endian) level sections
  int init_err = 0, init_phase = 0;
  if (pw.version == 2) {
    rl_beg = 0;
    rl_end = pw.rl_len;
    dl_beg = rl_end;
    dl_end = rl_end + pw.dl_len;
    data_beg = dl_end;
    if ((uint64_t)pw.rl_len + pw.dl_len > size) { init_err = PQG_ERR_CORRUPT; init_phase = 0; }
  } else {
    uint32_t p = 0;
    win.seek(0);
    // rl section (RunLengthBitPackingHybridValuesReader.initFromPage :40-46) when max_rep > 0
    for (int which = 0; which < 2 && !init_err; which++) {
      int maxl = which == 0 ? cd.max_rep : cd.max_def;
      int enc = which == 0 ? pw.rl_encoding : pw.dl_encoding;
      uint32_t b = p, e = p;
      if (maxl > 0 && enc == PQG_BIT_PACKED) {
        // deprecated BIT_PACKED levels (ByteBitPackingValuesReader(maxLevel, BIG_ENDIAN).initFromPage
        // :77-88): min(ceil(num_values * w / 8), available) bytes, no length prefix
        const uint32_t wl = 32 - __builtin_clz((uint32_t)maxl);
        const uint64_t want = ((uint64_t)nslots * wl + 7u) / 8u;
        const uint32_t len = (uint32_t)(want < (uint64_t)(size - p) ? want : (uint64_t)(size - p));
        b = p;
        e = p + len;
        p = e;
        if (which == 0) rl_be = true;
        else dl_be = true;
      } else if (maxl > 0) {
        if (enc != PQG_RLE) { init_err = PQG_ERR_UNSUPPORTED; init_phase = which; break; }
        if (p + 4u > size) { init_err = PQG_ERR_EOF; init_phase = which; break; }
        int32_t len = (int32_t)(uint32_t)win.read8(p);
        if (len < 0) { init_err = PQG_ERR_CORRUPT; init_phase = which; break; }
        if ((uint64_t)p + 4u + (uint32_t)len > size) { init_err = PQG_ERR_EOF; init_phase = which; break; }
        b = p + 4u;
        e = b + (uint32_t)len;
        p = e;
      } else if (enc != PQG_RLE && enc != PQG_BIT_PACKED) {
        init_err = PQG_ERR_UNSUPPORTED;
        init_phase = which;
        break;
      }
      if (which == 0) { rl_beg = b; rl_end = e; } else { dl_beg = b; dl_end = e; }
    }
    data_beg = p;
  }
  if (init_err) {
    if (lane == 0) {
      report(err, err_count, page, 0, (uint64_t)init_phase, init_err);
      if (hint_bad) {
        sst(hint_bad, err_count.epoch);
      } else {
        work[page].n_values = 0;
        work[page].data_begin = size;
      }
    }
    return;
  }
  // repetition levels first (ColumnReaderBase.checkRead reads rl then dl per slot)
  uint32_t limit = nslots;
  int code = 0;
  uint8_t* rep_out = cd.rep_levels ? cd.rep_levels + pw.slot_offset : nullptr;
  uint8_t* def_out = cd.def_levels ? cd.def_levels + pw.slot_offset : nullptr;
  uint64_t lvl_err_key = ~0ull;
  if (wr > 0) {
    uint32_t done = rl_be ? decode_levels_be(win.rs, rl_beg, rl_end, wr, nslots, rep_out, 0, false, nullptr, &code)
                          : decode_levels_w(LL, win.rs, rl_beg, rl_end, wr, nslots, rep_out, 0, false, nullptr, &code);
    if (code) {
      limit = done;
      lvl_err_key = ((uint64_t)done << 1) << 8 | (uint64_t)code;
    }
  } else if (rep_out) {
    for (uint32_t i = lane; i < nslots; i += WAVE) gst(rep_out + i, (uint8_t)0);
  }
  uint32_t nonnull = 0;
  if (wd > 0) {
    int code2 = 0;
    uint32_t done = dl_be ? decode_levels_be(win.rs, dl_beg, dl_end, wd, limit, def_out, (uint32_t)cd.max_def, true,
                                             &nonnull, &code2)
                          : decode_levels_w(LL, win.rs, dl_beg, dl_end, wd, limit, def_out, (uint32_t)cd.max_def, true,
                                             &nonnull, &code2,
#ifdef PQG_DIAG
                                            pqg_diag_wph ? pqg_diag_wph + 8 * (uint64_t)page : nullptr
#else
                                            nullptr
#endif
                                             );
    if (code2) {
      uint64_t key = (((uint64_t)done << 1) | 1ull) << 8 | (uint64_t)code2;
      if (key < lvl_err_key) lvl_err_key = key;
    }
  } else {
    nonnull = limit;  // max_def == 0: every slot holds a value
    if (def_out)
      for (uint32_t i = lane; i < limit; i += WAVE) gst(def_out + i, (uint8_t)0);
  }
  if (lane == 0) {
    if (lvl_err_key != ~0ull) {
      // level error key: slot << 1 | (0 = rl, 1 = dl) — host decodes it
      report_key(&err[3 * (uint64_t)page + 1], err_count, lvl_err_key);
    }
    if (hint_bad) {
      if (lvl_err_key != ~0ull || nonnull != pw.n_values || data_beg != pw.data_begin) sst(hint_bad, err_count.epoch);
    } else {
      work[page].n_values = nonnull;
      work[page].data_begin = data_beg;
    }
  }
}

// Exclusive scan of non-null counts per column (one workgroup per column).
__global__ __launch_bounds__(256) void k_scan_offsets(PageWork* __restrict__ work, const int32_t* __restrict__ col_pages,
                                                      const int32_t* __restrict__ col_page_start, int n_cols) {
  // thread t takes SO_PER consecutive pages per round, all loads issued first (two dependent round
  // trips per round instead of per 256 pages), one workgroup scan of the threads' totals
  constexpr int SO_PER = 16;
  const int c = blockIdx.x;
  const int b = col_page_start[c], e = col_page_start[c + 1];
  __shared__ uint64_t warp_sums[4];
  uint64_t carry = 0;
  for (int r0 = b; r0 < e; r0 += 256 * SO_PER) {
    const int i0 = r0 + (int)threadIdx.x * SO_PER;
    int pg[SO_PER];
#pragma unroll
    for (int q = 0; q < SO_PER; q++) pg[q] = i0 + q < e ? col_pages[i0 + q] : -1;
    uint64_t v[SO_PER], own = 0;
#pragma unroll
    for (int q = 0; q < SO_PER; q++) {
      v[q] = pg[q] >= 0 ? work[pg[q]].n_values : 0;
      own += v[q];
    }
    uint64_t x = own;
    for (int o = 1; o < 64; o <<= 1) {
      const uint64_t y = __shfl_up(x, o);
      if ((int)lane_id() >= o) x += y;
    }
    if (lane_id() == 63) warp_sums[threadIdx.x >> 6] = x;
    __syncthreads();
    uint64_t pre = carry + x - own, tot = 0;
    for (int wv = 0; wv < 4; wv++) {
      pre += wv < (int)(threadIdx.x >> 6) ? warp_sums[wv] : 0;
      tot += warp_sums[wv];
    }
#pragma unroll
    for (int q = 0; q < SO_PER; q++) {
      if (pg[q] >= 0) gst(&work[pg[q]].out_offset, pre);
      pre += v[q];
    }
    carry += tot;
    __syncthreads();
  }
}

// BOOLEAN values with encoding RLE (Encoding.RLE.getValuesReader :116-124, getMaxLevel :255-271:
// width 1 for BOOLEAN values; parquet-mr's V2 writer, DefaultV2ValuesWriterFactory
// .getBooleanValuesWriter :77-84): RunLengthBitPackingHybridValuesReader.initFromPage :40-46 reads
// a 4-byte LE length and slices the stream; readBoolean :58-60 = readInteger() != 0. The width-1
// hybrid stream is decoded by the level-section decoder (same decoder class in the reference),
// then an RLE run's unmasked repeated byte is folded to 0 / 1.
__global__ __launch_bounds__(64 * WPB) void k_rle_bool(const uint8_t* __restrict__ bytes, uint64_t n_bytes,
                                                 const PageWork* __restrict__ work, const ColumnDev* __restrict__ cols,
                                                 const int32_t* __restrict__ list, int n_list, uint64_t* err,
                                                 ErrCount err_count) {
  __shared__ __attribute__((aligned(16))) LevelWaveLds lvl_lds[WPB];
  const int page = wave_page(list, n_list);
  if (page < 0) return;
  const PageWork pw = work[page];
  const ColumnDev cd = cols[pw.column];
  const uint32_t lane = lane_id();
  const uint32_t beg = uni(pw.data_begin), size = uni(pw.size), n = uni(pw.n_values);
  const rsrc_t rs = make_rsrc(bytes + pw.base, n_bytes - pw.base);
  int code = 0;
  uint32_t b = 0, e = 0;
  if ((uint64_t)beg + 4u > size) {
    code = PQG_ERR_EOF;  // readIntLittleEndian
  } else {
    const int32_t len = (int32_t)uni(ld4_any(rs, beg));
    if (len < 0) code = PQG_ERR_CORRUPT;  // sliceStream(negative)
    else if ((uint64_t)beg + 4u + (uint32_t)len > size) code = PQG_ERR_EOF;
    b = beg + 4u;
    e = b + (uint32_t)len;
  }
  if (code) {
    if (lane == 0) report(err, err_count, page, 0, 2, code);
    return;
  }
  uint8_t* out = (uint8_t*)cd.values + pw.out_offset;
  int c2 = 0;
  const uint32_t done = decode_levels_w(lvl_lds[wave_id()], rs, b, e, 1, n, out, 1u, false, nullptr, &c2);
  if (c2 && lane == 0) report(err, err_count, page, 2, done, c2);
  __builtin_amdgcn_s_waitcnt(0);  // this wave's stores are visible to its loads
  for (uint32_t i = lane; i < done; i += WAVE) {
    const uint8_t v = *(const volatile uint8_t*)(out + i);
    if (v > 1u) gst(out + i, (uint8_t)1);
  }
}

// ---------------------------------------------------------------------------
// DELTA_BINARY_PACKED (DeltaBinaryPackingValuesReader.initFromPage :59-77, eager):
// the wave walks block headers (min delta, miniblock widths) into registers
// (block b -> lane b % 64), then per block each lane unpacks its deltas, a
// wave-wide inclusive scan (wrapping int64) turns them into values. INT32 =
// (int) of the long (readInteger :103-107).
//
// LDS segment of the page bytes for the delta decoder: the serial header chain and the
// miniblocks are read from LDS, and the segment is refilled (one coalesced 8 KiB load) only
// every few dozen blocks. Reading the page with global loads between the blocks' stores costs
// a full store drain per block (vmcnt counts stores on CDNA).
constexpr uint32_t DSEG = 8192;
// segment expansion (delta_expand_seg) for miniblocks of a multiple of 16 deltas
// block headers parsed by the vector unit (delta_hdr_v)

struct DSeg {
  rsrc_t rs;
  uint8_t* seg;
  uint32_t lo;  // segment = page bytes [lo, lo + DSEG), lo 16-aligned (uniform)

  __device__ __forceinline__ void fill(uint32_t p) {
    lo = uni(p & ~15u);
#pragma unroll
    for (uint32_t i = 0; i < DSEG; i += 16u * WAVE) {
      const uint32_t o = i + 16u * lane_id();
      *(u32x4*)(seg + o) = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)(lo + o), 0, 0);
    }
    wave_sync();
  }
  __device__ __forceinline__ bool has(uint32_t a, uint32_t n) const {
    return a >= lo && (uint64_t)a + n <= (uint64_t)lo + DSEG;
  }
  __device__ __forceinline__ uint32_t w32(uint32_t a4) const { return *(const u32_alias*)(seg + (a4 - lo)); }
  // 8 bytes at uniform p (refills the segment when they are not staged)
  __device__ __forceinline__ uint64_t read8u(uint32_t p) {
    const uint32_t a = p & ~3u, sb = p & 3u;
    if (!has(a, 12)) fill(p);
    const uint32_t x0 = w32(a), x1 = w32(a + 4), x2 = w32(a + 8);
    return (uint64_t)__builtin_amdgcn_alignbyte(x1, x0, sb) |
           ((uint64_t)__builtin_amdgcn_alignbyte(x2, x1, sb) << 32);
  }
};

// readUnsignedVarInt / readUnsignedVarLong (BytesUtils.java:202-211, 260-269) at uniform p with
// Java shift masking; a varint not terminated within `lim` bytes gets len = lim + 1.
template <bool INT>
__device__ __forceinline__ uint64_t seg_uvar(DSeg& S, uint32_t p, uint32_t lim, uint32_t& len) {
  uint64_t value = 0, x = S.read8u(p);
  uint32_t i = 0, k = 0, b;
  for (;;) {
    b = (k < 8u) ? (uint32_t)(x >> (8u * k)) & 0xFFu : (uint32_t)S.read8u(p + k) & 0xFFu;
    if (!(b & 0x80u)) break;
    value |= (uint64_t)(b & 0x7Fu) << (i & (INT ? 31u : 63u));
    i += 7;
    k++;
    if (k >= lim) break;
  }
  len = k + 1;
  if (INT) return (uint32_t)value | (b << (i & 31u));
  return value | ((uint64_t)b << (i & 63u));
}

// Expansion of nb walked blocks (block b's facts in lane b of b_*): lane l unpacks deltas
// [l*E, l*E + E) of every block, all in one miniblock m (the lane's miniblock index and its
// position in it are the same for every block): unpacked + minDelta (wrapping, as
// loadNewBlockToBuffer :139-142), a DPP scan of the lanes' sums. The value after delta j has
// index blk_first + b*block + j; lane l STORES the E values ending one delta earlier
// (indices blk_first - 1 + b*block + l*E + q, the first taken from lane l - 1 / the carry), so
// that every lane's run is E-aligned and goes out as wide stores. The value after a stream's
// last full block is written by the caller (delta_stream).
template <class T, uint32_t E>
__device__ __forceinline__ void store_run(T* p, const T (&u)[E]) {
  constexpr uint32_t BYTES = E * sizeof(T);
  if constexpr (BYTES >= 16) {
#pragma unroll
    for (uint32_t i = 0; i < BYTES / 16; i++) {
      u32x4 v;
      __builtin_memcpy(&v, (const uint8_t*)u + 16 * i, 16);
      gst((u32x4*)p + i, v);
    }
  } else if constexpr (BYTES == 8) {
    uint64_t v;
    __builtin_memcpy(&v, u, 8);
    gst((uint64_t*)p, v);
  } else {
#pragma unroll
    for (uint32_t q = 0; q < E; q++) gst(p + q, u[q]);
  }
}

template <int W, bool NEG, uint32_t E>
__device__ __forceinline__ void delta_expand(const DSeg& S, uint32_t nb, uint32_t b_data, uint32_t b_wpos,
                                             uint32_t b_lo, uint32_t b_hi, uint32_t b_nmb, uint32_t blk_first,
                                             uint32_t block, uint32_t mbs, uint32_t n_out, uint64_t& carry,
                                             typename DictVal<W>::T* out, int page, uint64_t* err,
                                             ErrCount err_count) {
  typedef typename DictVal<W>::T T;
  const uint32_t lane = lane_id();
  const uint32_t j0 = lane * E;
  const bool lane_in = j0 < block;
  const uint32_t m = lane_in ? j0 / mbs : 0u;
  // (a lane past the block, when the block is shorter than 64 * E, reads as delta 0 of miniblock 0: its
  // own index would address up to 64 * E * 8 bytes from the block's data, past the staged bytes)
  const uint32_t jm = lane_in ? j0 - m * mbs : 0u;
  const uint32_t mb_bytes = mbs / 8u;  // bytes per bit of width
  // wide stores need the run's first value E*W-aligned (runs start at multiples of E from `out`)
  constexpr uint32_t RUN = E * (uint32_t)sizeof(T);
  const bool wide = RUN >= 8 && (((uintptr_t)out + ((uint64_t)(blk_first - 1) * sizeof(T))) % (RUN >= 16 ? 16 : 8)) == 0 &&
                    ((uint64_t)block * sizeof(T)) % (RUN >= 16 ? 16 : 8) == 0;
  for (uint32_t b = 0; b < nb; b++) {
    const uint32_t data = rdl(b_data, b), wpos = rdl(b_wpos, b), nmb = rdl(b_nmb, b);
    const uint64_t mind = ((uint64_t)rdl(b_hi, b) << 32) | rdl(b_lo, b);
    // the block's miniblock widths (<= 8 bytes at wpos)
    const uint32_t wa = wpos & ~3u, sb = wpos & 3u;
    const uint32_t y0 = S.w32(wa), y1 = S.w32(wa + 4), y2 = S.w32(wa + 8);
    const uint32_t wlo = __builtin_amdgcn_alignbyte(y1, y0, sb), whi = __builtin_amdgcn_alignbyte(y2, y1, sb);
    // width of the lane's miniblock and the byte offset of its data (sum of the widths before it)
    const uint32_t wl = m < nmb ? ((m < 4u ? wlo >> (8u * m) : whi >> (8u * (m - 4u))) & 0xFFu) : 0u;
    const uint32_t blo = m >= 4u ? wlo : (m ? wlo & ((1u << (8u * m)) - 1u) : 0u);
    const uint32_t bhi = m <= 4u ? 0u : whi & ((1u << (8u * (m - 4u))) - 1u);
    const uint32_t off = (__builtin_amdgcn_sad_u8(blo, 0u, 0u) + __builtin_amdgcn_sad_u8(bhi, 0u, 0u)) * mb_bytes;
    const uint64_t mask = wl == 64 ? ~0ull : ((1ull << wl) - 1ull);
    uint64_t loc[E];
    uint64_t sum = 0;
#pragma unroll
    for (uint32_t q = 0; q < E; q++) {
      uint64_t d = 0;
      if (wl) {
        const uint32_t bit = (jm + q) * wl;
        const uint32_t byte = data + off + (bit >> 3);
        const uint32_t a = byte & ~3u;
        const uint32_t x0 = S.w32(a), x1 = S.w32(a + 4), x2 = S.w32(a + 8);
        const uint32_t sh = (byte - a) * 8u + (bit & 7u);  // < 32
        const uint64_t lo64 = (uint64_t)x0 | ((uint64_t)x1 << 32);
        const uint64_t v = sh == 0 ? lo64 : ((lo64 >> sh) | ((uint64_t)x2 << (64u - sh)));
        d = v & mask;
      }
      sum += lane_in ? d + mind : 0ull;
      loc[q] = sum;
    }
    const uint64_t x = wave_incl_scan_u64(sum);
    const uint64_t base_v = carry + (x - sum);
    // value before this lane's first delta: the previous lane's last value (lane 0: the carry)
    const uint64_t last = base_v + loc[E - 1];
    const uint32_t plo = (uint32_t)__shfl_up((int)(uint32_t)last, 1), phi = (uint32_t)__shfl_up((int)(uint32_t)(last >> 32), 1);
    const uint64_t prev = lane == 0 ? carry : (((uint64_t)phi << 32) | plo);
    const uint64_t k0 = (uint64_t)blk_first - 1u + (uint64_t)b * block + j0;  // index of the run's first value
    T u[E];
#pragma unroll
    for (uint32_t q = 0; q < E; q++) u[q] = (T)(q == 0 ? prev : base_v + loc[q - 1]);
    if (lane_in) {
      if (!NEG && wide && k0 + E <= n_out) {
        store_run<T, E>(out + k0, u);
      } else {
#pragma unroll
        for (uint32_t q = 0; q < E; q++) {
          const uint64_t k = k0 + q;
          if (k < n_out) {
            T v = u[q];
            if (NEG && k > 0 && (int32_t)(uint32_t)v < 0) {
              report(err, err_count, page, 2, k, PQG_ERR_CORRUPT);
              v = 0;
            }
            if (!NEG || k > 0) gst(out + k, v);
          }
        }
      }
    }
    carry += (uint64_t)rdl((uint32_t)x, 63) | ((uint64_t)rdl((uint32_t)(x >> 32), 63) << 32);
  }
}

// Segment expansion of nb walked blocks whose miniblocks hold a multiple of 16 deltas (parquet-mr
// and Arrow write 128 / 4, i.e. 32 per miniblock): lane l of a step takes segment g = 64 * step + l
// of the batch — L = 8 consecutive deltas of one miniblock of block g / (block / L) — unpacks them
// from the LDS segment at its own bit position, keeps their running sums in registers, and one
// 64-bit DPP scan of the 64 segment sums gives every segment its base: 512 deltas per scan and
// per carry step instead of one block (delta_expand: 64 * E). Values, the minDelta addition
// (loadNewBlockToBuffer :139-142, also for the unread miniblocks of a last block, whose values lie
// past the count and are not stored) and the store layout are those of delta_expand: lane l stores
// the L values ending one delta earlier (the first from lane l - 1 / the carry), as wide stores
// when the run is aligned. NEG streams (DELTA_LENGTH lengths) check every value of a step that holds a
// negative one on the per-lane stores.
// In-place inclusive prefix of a lane's deltas in two independent halves joined at the end (half the
// dependent adds of one running sum).
template <class U, uint32_t N>
__device__ __forceinline__ void delta_local_prefix(U (&v)[N]) {
  constexpr uint32_t H = N / 2;
#pragma unroll
  for (uint32_t q = 1; q < H; q++) v[q] += v[q - 1];
#pragma unroll
  for (uint32_t q = H + 1; q < N; q++) v[q] += v[q - 1];
#pragma unroll
  for (uint32_t q = H; q < N; q++) v[q] += v[H - 1];
}

// NEG (DELTA_LENGTH_BYTE_ARRAY lengths): a negative (int) value is reported as CORRUPT at its index and stored
// as 0; a step holding one takes the per-lane stores, which check every value.
template <int W, bool NEG = false>
__device__ __forceinline__ void delta_expand_seg(const DSeg& S, uint32_t nb, uint32_t b_data, uint32_t b_wpos,
                                                 uint32_t b_lo, uint32_t b_hi, uint32_t b_nmb, uint32_t blk_first,
                                                 uint32_t block, uint32_t mbs, uint32_t n_out, uint64_t& carry,
                                                 typename DictVal<W>::T* out, int page = 0, uint64_t* err = nullptr,
                                                 ErrCount err_count = ErrCount{}) {
  typedef typename DictVal<W>::T T;
  // 8 deltas per lane-step (16 measured slower: its 115 VGPRs left 4 waves per SIMD, and 5,000 pages of
  // delta_i64 took 1.2 rounds of them; at 98 VGPRs the LDS segments' 5 waves per SIMD hold every page at
  // once: delta_i64 0.370 -> 0.336 ms, C3 6.68 -> 6.61 ms, C4 10.26 -> 10.12 ms, profiles/r06/delta_l8)
  constexpr uint32_t L = 8;
  const uint32_t lane = lane_id();
  const uint32_t SB = block / L;  // segments per block
  const uint32_t n_seg = nb * SB;
  const uint32_t mb_bytes = mbs / 8u;  // bytes per bit of width
  // Runs are stored shifted by `sft` values so that every lane's L stored values start 16-byte
  // aligned whatever the page's output offset (pages of nullable columns start at any value): lane l
  // stores values [k0 + sft, k0 + sft + L), the last sft of them the first values of lane l + 1's
  // run (its u[1], u[2]: one shuffle each; u[L] is the lane's own last value). The batch's last lane
  // stores only its own values, lane 0 also the sft values before its wide run.
  constexpr uint32_t VPC = 16u / sizeof(T);  // values per 16 bytes
  const uint32_t mis = (uint32_t)((((uintptr_t)out + (uint64_t)(blk_first - 1) * sizeof(T)) % 16u) / sizeof(T));
  const uint32_t sft = mis ? VPC - mis : 0u;
  const bool wide = ((uintptr_t)out % sizeof(T)) == 0 && ((uint64_t)block * sizeof(T)) % 16 == 0;
  for (uint32_t g0 = 0; g0 < n_seg; g0 += WAVE) {
    const uint32_t g = g0 + lane;
    const bool lane_in = g < n_seg;
    const uint32_t bb = lane_in ? g / SB : 0u;
    // (a lane past the batch's segments reads as segment 0 of block 0, staged, and stores nothing)
    const uint32_t j0 = lane_in ? (g - bb * SB) * L : 0u;  // the segment's first delta in its block
    const uint32_t m = j0 / mbs, jm = j0 - m * mbs;
    const uint32_t data = (uint32_t)__shfl((int)b_data, (int)bb), wpos = (uint32_t)__shfl((int)b_wpos, (int)bb);
    const uint32_t nmb = (uint32_t)__shfl((int)b_nmb, (int)bb);
    const uint64_t mind = ((uint64_t)(uint32_t)__shfl((int)b_hi, (int)bb) << 32) | (uint32_t)__shfl((int)b_lo, (int)bb);
    // the block's miniblock widths (<= 8 bytes at wpos), the lane's width and data offset
    const uint32_t wa = wpos & ~3u, sb = wpos & 3u;
    const uint32_t y0 = S.w32(wa), y1 = S.w32(wa + 4), y2 = S.w32(wa + 8);
    // only the nmb used width bytes count: the reader never looks at the width of an unread miniblock of a
    // last block (any byte value), so such a lane gets width 0 and the position after the used miniblocks'
    // data, inside the staged bytes (the walk staged dbytes + 12), not a sum over arbitrary bytes
    const uint32_t uml = nmb >= 4u ? 0xFFFFFFFFu : (1u << (8u * nmb)) - 1u;
    const uint32_t umh = nmb <= 4u ? 0u : (nmb >= 8u ? 0xFFFFFFFFu : (1u << (8u * (nmb - 4u))) - 1u);
    const uint32_t wlo = __builtin_amdgcn_alignbyte(y1, y0, sb) & uml, whi = __builtin_amdgcn_alignbyte(y2, y1, sb) & umh;
    const uint32_t wl = (m < 4u ? wlo >> (8u * m) : whi >> (8u * (m - 4u))) & 0xFFu;
    const uint32_t blo = m >= 4u ? wlo : (m ? wlo & ((1u << (8u * m)) - 1u) : 0u);
    const uint32_t bhi = m <= 4u ? 0u : whi & ((1u << (8u * (m - 4u))) - 1u);
    const uint32_t dbase = data + (__builtin_amdgcn_sad_u8(blo, 0u, 0u) + __builtin_amdgcn_sad_u8(bhi, 0u, 0u)) * mb_bytes;
    T u[L + 3];
    uint64_t x;  // the wave scan of the lanes' sums (its last lane: the batch's total)
    if constexpr (W == 4) {
      // 4-byte values: the reader keeps long sums and casts them to int, whose low 32 bits depend on
      // the low 32 bits of every delta and of minDelta only: 32-bit unpack (one v_alignbit from the
      // dword pair holding the delta's first bit), sums and scan
      const uint32_t mask = wl >= 32u ? 0xFFFFFFFFu : (1u << wl) - 1u;
      const uint32_t mind32 = (uint32_t)mind;
      uint32_t loc[L];
      uint32_t sum = 0;
      // bit position relative to the dword holding the miniblock data's first byte (a page-absolute
      // bit position would wrap for data 512 MiB or more into a page)
      const uint32_t abase = dbase & ~3u;
      const uint32_t ab0 = (dbase & 3u) * 8u + jm * wl;
      // every dword pair is read unconditionally (a zero width reads the miniblock's first dword, inside
      // the staged segment, and masks it to 0): a branch per delta put an LDS round trip and its wait
      // between the deltas, 8 serial trips per step instead of one
      uint32_t x0[L], x1[L];
#pragma unroll
      for (uint32_t q = 0; q < L; q++) {
        const uint32_t a = abase + (((ab0 + q * wl) >> 5) << 2);
        x0[q] = S.w32(a);
        x1[q] = S.w32(a + 4);
      }
#pragma unroll
      for (uint32_t q = 0; q < L; q++) {
        const uint32_t d = __builtin_amdgcn_alignbit(x1[q], x0[q], (ab0 + q * wl) & 31u) & mask;
        loc[q] = lane_in ? d + mind32 : 0u;
      }
      delta_local_prefix(loc);
      sum = loc[L - 1];
      const uint32_t x32 = wave_incl_scan_u32_dpp(sum);
      // the value before the lane's first delta: the carry plus every earlier lane's sum (= lane l - 1's last)
      const uint32_t base_v = (uint32_t)carry + (x32 - sum);
#pragma unroll
      for (uint32_t q = 0; q < L + 1; q++) u[q] = (T)(q == 0 ? base_v : base_v + loc[q - 1]);
      x = x32;
    } else {
      const uint64_t mask = wl == 64 ? ~0ull : ((1ull << wl) - 1ull);
      const bool narrow = !__ballot(lane_in && wl > 32u);  // every width <= 32: two dwords per delta
      uint64_t loc[L];
      uint64_t sum = 0;
      // all reads of the step first, no branch per delta (see the 4-byte path): a zero width reads the
      // miniblock's first dwords and masks them to 0
      const uint32_t bit0 = (dbase & 3u) * 8u + jm * wl;  // relative to the dword holding dbase
      const uint32_t abase = dbase & ~3u;
      uint32_t x0[L], x1[L], x2[L];
      auto unpack = [&](auto wide_tag) {
        constexpr bool WIDE = decltype(wide_tag)::value;
#pragma unroll
        for (uint32_t q = 0; q < L; q++) {
          const uint32_t a = abase + (((bit0 + q * wl) >> 5) << 2);
          x0[q] = S.w32(a);
          x1[q] = S.w32(a + 4);
          if (WIDE) x2[q] = S.w32(a + 8);
        }
#pragma unroll
        for (uint32_t q = 0; q < L; q++) {
          const uint32_t sh = (bit0 + q * wl) & 31u;
          const uint64_t lo64 = (uint64_t)x0[q] | ((uint64_t)x1[q] << 32);
          const uint64_t d = (WIDE ? (sh == 0 ? lo64 : ((lo64 >> sh) | ((uint64_t)x2[q] << (64u - sh)))) : (lo64 >> sh)) & mask;
          loc[q] = lane_in ? d + mind : 0ull;
        }
      };
      if (narrow) unpack(std::false_type{});
      else unpack(std::true_type{});
      delta_local_prefix(loc);
      sum = loc[L - 1];
      x = wave_incl_scan_u64(sum);
      // the value before the lane's first delta: the carry plus every earlier lane's sum (= lane l - 1's last)
      const uint64_t base_v = carry + (x - sum);
#pragma unroll
      for (uint32_t q = 0; q < L + 1; q++) u[q] = (T)(q == 0 ? base_v : base_v + loc[q - 1]);
    }
    const uint64_t k0 = (uint64_t)blk_first - 1u + (uint64_t)bb * block + j0;  // index of the run's first value
    // values L + 1, L + 2 of the lane's window: lane l + 1's u[1], u[2] (only for 4-byte values: sft <= 3)
    if constexpr (VPC > 2) {
      u[L + 1] = (T)(uint32_t)__shfl_down((int)(uint32_t)u[1], 1);
      u[L + 2] = (T)(uint32_t)__shfl_down((int)(uint32_t)u[2], 1);
    } else {
      u[L + 1] = u[L + 2] = 0;
    }
    // A full step (64 lanes, its 16-byte rows inside the output): the rows are exchanged between lanes so
    // that every store instruction writes 1 KiB contiguous (lane_rows_to_tiles). Lane-contiguous runs (each
    // lane 64 bytes, four 16-byte stores 64 bytes apart) store at ~3.6 TB/s (profiles/r02/store_patterns.txt
    // 'lane-contig'); the same step with 1 KiB per instruction took delta_i64 0.335 -> 0.245 ms
    // (profiles/r06/delta_tstore). Row r of the step holds values [K + sft + VPC r, + VPC); lane l's run is
    // rows NR l .. NR l + NR - 1; store i of lane m writes row 64 i + m.
    const uint64_t K = (uint64_t)blk_first - 1u + (uint64_t)L * g0;  // value index of lane 0's u[0]
    bool neg_any = false;
    if constexpr (NEG) {
      bool ln = false;
#pragma unroll
      for (uint32_t q = 0; q < L + VPC - 1u; q++) ln |= (int32_t)(uint32_t)u[q] < 0;
      neg_any = __ballot(lane_in && ln) != 0;
    }
    if (wide && (!NEG || !neg_any) && g0 + WAVE <= n_seg && K + sft + (uint64_t)WAVE * L <= n_out) {
      if (lane == 0)  // the sft values before the first row
        for (uint32_t q = 0; q < VPC - 1u; q++)
          if (q < sft) gst(out + K + q, u[q]);
      auto tput = [&](auto s_tag) {
        constexpr uint32_t SF = decltype(s_tag)::value;
        constexpr uint32_t NR = L / VPC;  // rows per lane (4 for 8-byte values, 2 for 4-byte)
        u32x4 row[NR];
#pragma unroll
        for (uint32_t j = 0; j < NR; j++) {
          T v[VPC];
#pragma unroll
          for (uint32_t q = 0; q < VPC; q++) v[q] = u[SF + VPC * j + q];
          __builtin_memcpy(&row[j], v, 16);
        }
        u32x4 st[NR];
        lane_rows_to_tiles<NR>(row, st);
        u32x4* const base = (u32x4*)(out + K + SF);
#pragma unroll
        for (uint32_t i = 0; i < NR; i++) {
          // with 4-byte values and SF >= 2 the step's last row reaches past index K + 64 L (lane 63's last
          // value): only its values up to there go out here, the rest are the next step's head
          if (W == 4 && SF >= 2 && i == NR - 1 && lane == WAVE - 1) {
            const uint32_t* sp = (const uint32_t*)&st[i];
#pragma unroll
            for (uint32_t q = 0; q < 5u - SF; q++) gst((uint32_t*)(base + WAVE * i + lane) + q, sp[q]);
          } else {
            gst(base + WAVE * i + lane, st[i]);
          }
        }
      };
      if (sft == 0) tput(std::integral_constant<uint32_t, 0>{});
      else if (sft == 1) tput(std::integral_constant<uint32_t, 1>{});
      else if constexpr (VPC > 2) {
        if (sft == 2) tput(std::integral_constant<uint32_t, 2>{});
        else tput(std::integral_constant<uint32_t, 3>{});
      }
      if constexpr (W == 4) carry += rdl((uint32_t)x, 63);
      else carry += (uint64_t)rdl((uint32_t)x, 63) | ((uint64_t)rdl((uint32_t)(x >> 32), 63) << 32);
      continue;
    }
    if (lane_in) {
      const bool last_lane = g + 1u >= n_seg || lane == WAVE - 1u;
      // a checked store (NEG: a negative length is CORRUPT at its index and written as 0)
      // (value 0, the stream's first value, was checked and stored by delta_stream: never rewritten here)
      auto put1 = [&](uint64_t k, T v) {
        if constexpr (NEG) {
          if (k == 0) return;
          if ((int32_t)(uint32_t)v < 0) {
            report(err, err_count, page, 2, k, PQG_ERR_CORRUPT);
            v = 0;
          }
        }
        gst(out + k, v);
      };
      if (lane == 0)  // the sft values before lane 0's shifted run
        for (uint32_t q = 0; q < VPC - 1u; q++)
          if (q < sft && k0 + q < n_out) {
            if constexpr (NEG) put1(k0 + q, u[q]);
            else gst(out + k0 + q, u[q]);
          }
      const uint64_t a = k0 + sft;
      if (wide && (!NEG || !neg_any) && !last_lane && a + L <= n_out) {
        // v[q] = u[sft + q]: sft is uniform, so a branch per value of it picks the registers statically
        auto put = [&](auto s_tag) {
          constexpr uint32_t SF = decltype(s_tag)::value;
          T v[L];
#pragma unroll
          for (uint32_t q = 0; q < L; q++) v[q] = u[q + SF];
          store_run<T, L>(out + a, v);
        };
        if (sft == 0) put(std::integral_constant<uint32_t, 0>{});
        else if (sft == 1) put(std::integral_constant<uint32_t, 1>{});
        else if constexpr (VPC > 2) {
          if (sft == 2) put(std::integral_constant<uint32_t, 2>{});
          else put(std::integral_constant<uint32_t, 3>{});
        }
      } else {
        const uint64_t e = last_lane ? k0 + L : a + L;  // the last lane: its own values only
#pragma unroll
        for (uint32_t q = 0; q < L + VPC - 1u; q++) {
          const uint64_t k = k0 + q;
          if (k >= a && k < e && k < n_out) {
            if constexpr (NEG) put1(k, u[q]);
            else gst(out + k, u[q]);
          }
        }
      }
    }
    if constexpr (W == 4) carry += rdl((uint32_t)x, 63);  // (only its low 32 bits are ever stored)
    else carry += (uint64_t)rdl((uint32_t)x, 63) | ((uint64_t)rdl((uint32_t)(x >> 32), 63) << 32);
  }
}

// Any other DeltaBinaryPackingConfig the reference accepts (blocks of more than 512 values or more
// than 8 miniblocks; DuckDB writes 2048 / 8): block by block, miniblock by miniblock, 64 deltas
// per step, page bytes read with buffer loads. Same checks, in the same order, as the batched walk
// below (loadNewBlockToBuffer :118-143): widths of the used miniblocks (> 64: CORRUPT), then
// their bytes (EOF). p = position after the header; the first value is already stored.
// Every byte comes from the wave's LDS segment (refilled when a header or a 64-delta step leaves
// it): a global load between the steps' stores would wait for all of them (vmcnt counts stores),
// one drain per 64 values; with the segment it is one drain per 8 KiB of page bytes.
template <int W, bool NEG>
__device__ int delta_generic(DSeg& S, uint32_t p, uint32_t end, uint32_t block, uint32_t mbn, uint32_t mbs,
                             uint32_t total, uint32_t n_out, uint64_t carry, typename DictVal<W>::T* out, int page,
                             uint64_t* err, ErrCount err_count, uint32_t* p_end, uint32_t buffered0 = 1) {
  typedef typename DictVal<W>::T T;
  const uint32_t lane = lane_id();
  auto byte_at = [&](uint32_t a) -> uint32_t {
    if (!S.has(a & ~3u, 4)) S.fill(a);
    return uni((S.w32(a & ~3u) >> (8u * (a & 3u))) & 0xFFu);
  };
  // (buffered0 > 1: resumed at a block boundary by the batched path, values before it stored)
  uint32_t buffered = buffered0;
  uint64_t k_next = buffered0;  // value index after the next delta
  while (true) {
    p = uni(p);
    buffered = uni(buffered);
    if (buffered >= total) break;
    if (p >= end) return PQG_ERR_EOF;
    // min delta (readZigZagVarLong, Java shift masking)
    uint64_t mraw = 0;
    uint32_t i = 0, k = 0, b;
    for (;;) {
      b = byte_at(p + k);
      if (!(b & 0x80u)) break;
      mraw |= (uint64_t)(b & 0x7Fu) << (i & 63u);
      i += 7;
      k++;
      if (k >= end - p) break;
    }
    mraw |= (uint64_t)b << (i & 63u);
    if ((uint64_t)p + k + 1u > end) return PQG_ERR_EOF;
    const uint64_t mind = (uint64_t)zigzag64(mraw);
    const uint32_t wpos = p + k + 1u;
    if ((uint64_t)wpos + mbn > end) return PQG_ERR_EOF;  // readBitWidthsForMiniBlocks
    uint32_t used = 0, bufd = buffered;
    uint64_t dbytes = 0;
    for (uint32_t m = 0; m < mbn && bufd < total; m++) {
      const uint32_t wm = byte_at(wpos + m);
      if (wm > 64u) return PQG_ERR_CORRUPT;
      dbytes += (uint64_t)wm * (mbs / 8u);
      bufd += mbs;
      used++;
    }
    const uint32_t dpos = wpos + mbn;
    if ((uint64_t)dpos + dbytes > end) return PQG_ERR_EOF;  // in.slice EOF
    uint32_t mo = dpos;  // data of miniblock m
    for (uint32_t m = 0; m < used; m++) {
      const uint32_t w = byte_at(wpos + m);
      const uint64_t mask = w == 64u ? ~0ull : ((1ull << w) - 1ull);
      for (uint32_t c = 0; c < mbs; c += WAVE) {
        const uint32_t q = c + lane;
        const bool in = q < mbs;
        // the step's bytes [mo + c*w/8, mo + (c+64)*w/8 + 12) staged (<= 524 bytes)
        const uint32_t s_lo = (mo + ((c * w) >> 3)) & ~3u, s_hi = mo + (((c + WAVE) * w + 7u) >> 3) + 12u;
        if (w && !S.has(s_lo, s_hi - s_lo)) S.fill(s_lo);
        uint64_t d = 0;
        if (in && w) {
          const uint32_t bit = q * w, byte = mo + (bit >> 3), a = byte & ~3u;
          const uint32_t x0 = S.w32(a), x1 = S.w32(a + 4), x2 = S.w32(a + 8);
          const uint32_t sh = (byte - a) * 8u + (bit & 7u);
          const uint64_t lo64 = (uint64_t)x0 | ((uint64_t)x1 << 32);
          d = (sh == 0 ? lo64 : ((lo64 >> sh) | ((uint64_t)x2 << (64u - sh)))) & mask;
        }
        const uint64_t x = wave_incl_scan_u64(in ? d + mind : 0ull);
        const uint64_t kk = k_next + q;
        if (in && kk < n_out) {
          T v = (T)(carry + x);
          if (NEG && (int32_t)(uint32_t)v < 0) {
            report(err, err_count, page, 2, kk, PQG_ERR_CORRUPT);
            v = 0;
          }
          gst(out + kk, v);
        }
        carry += (uint64_t)rdl((uint32_t)x, 63) | ((uint64_t)rdl((uint32_t)(x >> 32), 63) << 32);
      }
      k_next += mbs;
      mo += w * (mbs / 8u);
    }
    p = dpos + (uint32_t)dbytes;
    buffered = bufd;
  }
  (void)block;
  *p_end = p;
  return 0;
}

// Block header chain step (loadNewBlockToBuffer :118-143: zigzag varlong min delta,
// readBitWidthsForMiniBlocks, the used miniblocks' byte count) on the VECTOR unit at uniform p:
// every lane computes the same values from its LDS copy of 20 bytes (laundered into VGPRs so the
// compiler keeps the arithmetic off the scalar unit, which the CU's four SIMDs share: the scalar
// walk issued ~230 SALU instructions per 128-value block and made k_delta scalar-issue bound).
// Only what the NEXT header's position needs is on this serial path — the varint's length (stop-bit
// mask + ctz), the used widths' byte sum (v_sad_u8) — the min delta's value is decoded afterwards
// by the block's own lane (delta_mind_v), all blocks of a batch at once. Covers the common case —
// a min delta of at most 8 varint bytes, every used width <= 64, header and data inside the
// section — and returns false otherwise, so the scalar walk raises the reference's error.
struct DeltaHdr {
  uint32_t len, wpos, dpos, next, used, dbytes;
};
// (per lane: p need not be uniform; `used` miniblocks are read)
__device__ __forceinline__ bool delta_hdr_parse(const DSeg& S, uint32_t p, uint32_t end, uint32_t mbn, uint32_t mbs,
                                                uint32_t used, DeltaHdr& h) {
  const uint32_t a = p & ~3u, sb = p & 3u;
  if (!S.has(a, 20)) return false;
  uint32_t d[5];
#pragma unroll
  for (int i = 0; i < 5; i++) d[i] = S.w32(a + 4u * i);
  asm volatile("" : "+v"(d[0]), "+v"(d[1]), "+v"(d[2]), "+v"(d[3]), "+v"(d[4]));
  uint32_t x[4];
#pragma unroll
  for (int i = 0; i < 4; i++) x[i] = __builtin_amdgcn_alignbyte(d[i + 1], d[i], sb);  // bytes p + 4i ..
  const uint64_t lo = (uint64_t)x[0] | ((uint64_t)x[1] << 32);
  const uint64_t stop = ~lo & 0x8080808080808080ull;  // the varint's last byte has bit 7 clear
  const uint32_t len = stop ? ((uint32_t)__builtin_ctzll(stop) >> 3) + 1u : 9u;
  h.len = len;
  h.wpos = p + len;
  // the <= 8 width bytes: bytes [len, len + 8) of x (len == 8: x[2], x[3])
  const uint32_t q = len >> 2, r = len & 3u;
  const uint32_t xa = q == 0 ? x[0] : (q == 1 ? x[1] : x[2]);
  const uint32_t xb = q == 0 ? x[1] : (q == 1 ? x[2] : x[3]);
  const uint32_t xc = q == 0 ? x[2] : x[3];
  uint32_t wl = __builtin_amdgcn_alignbyte(xb, xa, r), wh = __builtin_amdgcn_alignbyte(xc, xb, r);
  wl &= used >= 4u ? 0xFFFFFFFFu : (1u << (8u * used)) - 1u;
  wh &= used <= 4u ? 0u : (used == 8u ? 0xFFFFFFFFu : (1u << (8u * (used - 4u))) - 1u);
  // a used width > 64 (bit 7 set, or low 7 bits >= 65): the scalar walk reports CORRUPT
  const uint32_t bad = (((wl & 0x7F7F7F7Fu) + 0x3F3F3F3Fu) | wl | ((wh & 0x7F7F7F7Fu) + 0x3F3F3F3Fu) | wh) & 0x80808080u;
  h.used = used;
  h.dbytes = (__builtin_amdgcn_sad_u8(wl, 0u, 0u) + __builtin_amdgcn_sad_u8(wh, 0u, 0u)) * (mbs / 8u);
  h.dpos = h.wpos + mbn;
  h.next = h.dpos + h.dbytes;
  return len <= 8u && !bad && (uint64_t)h.dpos + h.dbytes <= end;  // (implies p + len, wpos + mbn <= end)
}
__device__ __forceinline__ bool delta_hdr_v(const DSeg& S, uint32_t p, uint32_t end, uint32_t mbn, uint32_t mbs,
                                            uint32_t buffered, uint32_t total, DeltaHdr& h) {
  // miniblocks unpacked while buffered < total (:131-135)
  const uint32_t rem = total - buffered;  // > 0
  const uint32_t used = rem >= mbn * mbs ? mbn : (rem + mbs - 1u) / mbs;  // a page's last block only
  const bool ok = delta_hdr_parse(S, p, end, mbn, mbs, used, h);
  return uni(ok ? 1u : 0u) != 0u;
}

// The min delta of a block whose header delta_hdr_v walked: zigzag varlong of `len` (<= 8) bytes at
// hp (readZigZagVarLong), decoded by the block's lane from the LDS segment.
__device__ __forceinline__ uint64_t delta_mind_v(const DSeg& S, uint32_t hp, uint32_t len) {
  const uint32_t a = hp & ~3u, sb = hp & 3u;
  const uint32_t d0 = S.w32(a), d1 = S.w32(a + 4), d2 = S.w32(a + 8);
  const uint64_t lo = (uint64_t)__builtin_amdgcn_alignbyte(d1, d0, sb) | ((uint64_t)__builtin_amdgcn_alignbyte(d2, d1, sb) << 32);
  const uint64_t v = len >= 8u ? lo : lo & ((1ull << (8u * len)) - 1ull);
  const uint64_t raw = (v & 0x7Full) | ((v >> 1) & (0x7Full << 7)) | ((v >> 2) & (0x7Full << 14)) |
                       ((v >> 3) & (0x7Full << 21)) | ((v >> 4) & (0x7Full << 28)) | ((v >> 5) & (0x7Full << 35)) |
                       ((v >> 6) & (0x7Full << 42)) | ((v >> 7) & (0x7Full << 49));
  return (raw >> 1) ^ (0ull - (raw & 1ull));  // zigzag
}

// One stream [p, end) -> out[0 .. min(want, total)). Returns 0 or the init error code (the
// reader decodes eagerly in initFromPage); *p_end = stream position after the used miniblocks,
// *total_out = the header's value count. NEG: a negative (int) value is reported as CORRUPT at
// its index and written as 0 (DELTA_LENGTH_BYTE_ARRAY lengths: in.slice(negative)).
template <int W, bool NEG>
__device__ int delta_stream(DSeg& S, uint32_t p, uint32_t end, uint32_t want, typename DictVal<W>::T* out,
                            int page, uint64_t* err, ErrCount err_count, uint32_t* p_end, uint32_t* total_out) {
  typedef typename DictVal<W>::T T;
  const uint32_t lane = lane_id();
  uint32_t len;
  p = uni(p);
  // header (DeltaBinaryPackingConfig.readConfig :43-45, totalValueCount, first value)
  if (p >= end) return PQG_ERR_EOF;
  const uint32_t block = (uint32_t)seg_uvar<true>(S, p, end - p, len);
  if ((uint64_t)p + len > end) return PQG_ERR_EOF;
  p += len;
  if (p >= end) return PQG_ERR_EOF;
  const uint32_t mbn = (uint32_t)seg_uvar<true>(S, p, end - p, len);
  if ((uint64_t)p + len > end) return PQG_ERR_EOF;
  p += len;
  // DeltaBinaryPackingConfig ctor :34-41: (double) block / mbn % 8 == 0 on Java ints, i.e. block is a
  // multiple of 8 * mbn whatever the signs (the quotient of two ints is never rounded to an integer);
  // the precondition comes first, a negative count of miniblocks or block size is refused after it
  if (mbn == 0) return PQG_ERR_DELTA_CONFIG;
  if ((int64_t)(int32_t)block % (8 * (int64_t)(int32_t)mbn) != 0) return PQG_ERR_DELTA_CONFIG;
  if ((int32_t)mbn < 0 || (int32_t)block < 0) return PQG_ERR_CORRUPT;
  const uint32_t mbs = block / mbn;
  if (mbs == 0) return PQG_ERR_CORRUPT;
  if (p >= end) return PQG_ERR_EOF;
  uint32_t total = (uint32_t)seg_uvar<true>(S, p, end - p, len);
  if ((uint64_t)p + len > end) return PQG_ERR_EOF;
  p += len;
  // allocateValuesBuffer :83-87 takes ceil(count / mbs) miniblocks: a count of at most -mbs is a negative
  // array size, one in (-mbs, 0) rounds to no miniblock and the page reads as an empty one
  if ((int32_t)total < 0) {
    if ((int64_t)(int32_t)total <= -(int64_t)mbs) return PQG_ERR_CORRUPT;
    total = 0;
  }
  if (p >= end) return PQG_ERR_EOF;
  const uint64_t fraw = seg_uvar<false>(S, p, end - p, len);
  if ((uint64_t)p + len > end) return PQG_ERR_EOF;
  p += len;
  const int64_t first = zigzag64(fraw);
  *total_out = total;
  // values to emit: min(want, total); want > total -> "no more value to read" at index total (caller)
  const uint32_t n_out = want > total ? total : want;
  // Value index k (0-based) of the page: k = 0 is `first`; block b covers
  // k in [1 + b*block, 1 + (b+1)*block).
  uint64_t carry = (uint64_t)first;
  if (lane == 0 && n_out > 0) {
    if (NEG && (int32_t)(uint32_t)carry < 0) {
      report(err, err_count, page, 2, 0, PQG_ERR_CORRUPT);
      gst(out, (T)0);
    } else {
      gst(out, (T)carry);
    }
  }
  // register budget of the batched expansion: block <= 512 values, <= 8 miniblocks (parquet-mr
  // and Arrow write 128 / 4); other configurations take the block-by-block path
  // (blocks of up to 2,048 values in at most 8 miniblocks of a multiple of 16 deltas — DuckDB writes 2048 / 8 —
  // take the batched walk and the segment expansion too, whose per-lane work does not depend on the block)
  const bool seg_big = block <= 2048u && mbn <= 8u && (mbs % 16u) == 0 && ((uint64_t)block * W) % 16u == 0;
  if ((block > 512u || mbn > 8u) && !seg_big)
    return delta_generic<W, NEG>(S, p, end, block, mbn, mbs, total, n_out, carry, out, page, err, err_count, p_end);
  uint32_t buffered = 1;  // Java valuesBuffered (includes the first value)
  uint32_t n_blocks = 0;
  // deltas per lane per block: the power of two >= block / 64 (it divides the block, a multiple
  // of 8, so a lane's deltas never straddle a miniblock)
  const uint32_t E = block <= 64u ? 1u : block <= 128u ? 2u : block <= 256u ? 4u : 8u;
  // bytes a block header may touch: varint (<= 10) + widths (<= 8) + read slack
  constexpr uint32_t HDR_SPAN = 40;
  while (true) {
    buffered = uni(buffered);
    p = uni(p);
    if (buffered >= total) break;
    // a batch starts with its first block fully staged (a block is <= 4126 bytes)
    if (!S.has(p, DSEG / 2 + 64)) S.fill(p);
    // ---- walk up to 64 blocks whose bytes lie in the segment (headers + data offsets)
    uint32_t b_data = 0, b_wpos = 0, b_lo = 0, b_hi = 0, b_nmb = 0, b_mv = 0;
    uint32_t nb = 0;
    const uint32_t blk_first = buffered;
    // Fast chain over the batch's full blocks (every miniblock read): on the serial path only what the
    // next header's position needs — the min delta varint's length (stop-bit mask), the width bytes' sum —
    // while lane b keeps block b's header position; then every check of delta_hdr_v and the staged-data
    // test, one lane per block, all at once. The batch is cut at the first block that fails them (its
    // successor, computed from a bad header, is never used): the loop below takes that block (slow
    // header, error, refill) and the page's last, partial block.
    {
      const uint32_t full = mbn * mbs;                   // values of a full block (<= 512)
      const uint32_t nfull = uni((total - buffered) / full);
      const uint32_t lim = nfull < 64u ? nfull : 64u;
      const uint32_t mb8 = mbs / 8u;
      const uint32_t wml = mbn >= 4u ? 0xFFFFFFFFu : (1u << (8u * mbn)) - 1u;
      const uint32_t wmh = mbn <= 4u ? 0u : (mbn == 8u ? 0xFFFFFFFFu : (1u << (8u * (mbn - 4u))) - 1u);
      uint32_t pc = p, b_p = 0, n_c = 0;
      while (n_c < lim && S.has(pc, HDR_SPAN)) {
        const uint32_t a = pc & ~3u, sb = pc & 3u;
        uint32_t d[5];
#pragma unroll
        for (int i = 0; i < 5; i++) d[i] = S.w32(a + 4u * i);
        uint32_t x[4];
#pragma unroll
        for (int i = 0; i < 4; i++) x[i] = __builtin_amdgcn_alignbyte(d[i + 1], d[i], sb);
        const uint64_t lo = (uint64_t)x[0] | ((uint64_t)x[1] << 32);
        const uint64_t stop = ~lo & 0x8080808080808080ull;
        const uint32_t len = stop ? ((uint32_t)__builtin_ctzll(stop) >> 3) + 1u : 9u;
        const uint32_t q = len >> 2, r = len & 3u;
        const uint32_t xa = q == 0 ? x[0] : (q == 1 ? x[1] : x[2]);
        const uint32_t xb = q == 0 ? x[1] : (q == 1 ? x[2] : x[3]);
        const uint32_t xc = q == 0 ? x[2] : x[3];
        const uint32_t wl = __builtin_amdgcn_alignbyte(xb, xa, r) & wml, wh = __builtin_amdgcn_alignbyte(xc, xb, r) & wmh;
        b_p = lane == n_c ? pc : b_p;
        pc = uni(pc + len + mbn + (__builtin_amdgcn_sad_u8(wl, 0u, 0u) + __builtin_amdgcn_sad_u8(wh, 0u, 0u)) * mb8);
        n_c = uni(n_c + 1u);
      }
      if (n_c) {
        DeltaHdr h{};
        bool ok = false;
        if (lane < n_c)
          ok = delta_hdr_parse(S, b_p, end, mbn, mbs, mbn, h) && S.has(h.dpos, h.dbytes + 12u);
        const uint64_t badm = __ballot(lane < n_c && !ok);
        const uint32_t nk = uni(badm ? (uint32_t)__builtin_ctzll(badm) : n_c);  // blocks kept
        const bool keep = lane < nk;
        b_data = keep ? h.dpos : 0u;
        b_wpos = keep ? h.wpos : 0u;
        b_lo = keep ? b_p : 0u;  // header position and varint length: the min delta follows below
        b_hi = keep ? h.len : 0u;
        b_mv = keep ? 1u : 0u;
        b_nmb = keep ? mbn : 0u;
        if (nk) {
          p = uni(rdl(h.next, nk - 1u));
          buffered = uni(buffered + nk * full);
        }
        nb = nk;
      }
    }
    while (true) {
      nb = uni(nb);
      p = uni(p);
      buffered = uni(buffered);
      if (nb >= 64u || buffered >= total) break;
      if (p >= end) return PQG_ERR_EOF;
      if (!S.has(p, HDR_SPAN)) break;  // nb > 0 here: the batch ends, the next one refills
      {
        DeltaHdr h;
        if (delta_hdr_v(S, p, end, mbn, mbs, buffered, total, h)) {
          // the block's data (+ read slack) must be staged, else the block starts the next batch
          if (!S.has(uni(h.dpos), uni(h.dbytes) + 12u)) break;
          const bool me = lane == nb;
          b_data = me ? h.dpos : b_data;
          b_wpos = me ? h.wpos : b_wpos;
          b_lo = me ? p : b_lo;  // header position and varint length: the min delta follows below
          b_hi = me ? h.len : b_hi;
          b_mv = me ? 1u : b_mv;
          b_nmb = me ? h.used : b_nmb;
          p = uni(h.next);
          buffered = uni(buffered + h.used * mbs);
          nb++;
          continue;
        }
      }
      const uint64_t mraw = seg_uvar<false>(S, p, end - p, len);  // loadNewBlockToBuffer :122-126
      if ((uint64_t)p + len > end) return PQG_ERR_EOF;
      const int64_t mind = zigzag64(mraw);
      const uint32_t wpos = p + len;
      if ((uint64_t)wpos + mbn > end) return PQG_ERR_EOF;  // readBitWidthsForMiniBlocks
      // miniblocks unpacked while buffered < total (:131-135)
      uint32_t used = 0, bufd = buffered;
      uint64_t dbytes = 0;
      const uint64_t wbytes = S.read8u(wpos);  // the <= 8 width bytes
      for (uint32_t m = 0; m < mbn && bufd < total; m++) {
        const uint32_t wm = (uint32_t)(wbytes >> (8u * m)) & 0xFFu;
        if (wm > 64u) return PQG_ERR_CORRUPT;
        dbytes += (uint64_t)wm * (mbs / 8u);
        bufd += mbs;
        used++;
      }
      const uint32_t dpos = wpos + mbn;
      if ((uint64_t)dpos + dbytes > end) return PQG_ERR_EOF;  // in.slice EOF
      // the block's data (+ read slack) must be staged, else the block starts the next batch
      if (!S.has(dpos, (uint32_t)dbytes + 12u)) break;
      const bool me = lane == nb;
      b_data = me ? dpos : b_data;
      b_wpos = me ? wpos : b_wpos;
      b_lo = me ? (uint32_t)(uint64_t)mind : b_lo;
      b_hi = me ? (uint32_t)((uint64_t)mind >> 32) : b_hi;
      b_nmb = me ? used : b_nmb;
      p = dpos + (uint32_t)dbytes;
      buffered = bufd;
      nb++;
    }
    if (nb == 0) {
      // a block whose data does not fit the segment (only blocks over 512 values: > 4 KiB of deltas): the rest of
      // the stream block by block, from this block boundary (the values before it are stored)
      if (block > 512u) {
        if (S.lo != uni(p & ~15u)) {  // a fresh segment from the block on, then the batch again
          S.fill(p);
          continue;
        }
        const uint64_t k = (uint64_t)n_blocks * block;
        if (n_blocks && k < n_out && lane == 0) {  // the value before this block
          T v = (T)carry;
          if (NEG && (int32_t)(uint32_t)v < 0) {
            report(err, err_count, page, 2, k, PQG_ERR_CORRUPT);
            v = 0;
          }
          gst(out + k, v);
        }
        return delta_generic<W, NEG>(S, p, end, block, mbn, mbs, total, n_out, carry, out, page, err, err_count, p_end,
                                     buffered);
      }
      return PQG_ERR_CORRUPT;  // unreachable: a block of at most 512 values always fits
    }
    // min deltas of the blocks delta_hdr_v walked, one lane per block (the segment holds them: it is
    // refilled only at a batch start)
    if (b_mv) {
      const uint64_t md = delta_mind_v(S, b_lo, b_hi);
      b_lo = (uint32_t)md;
      b_hi = (uint32_t)(md >> 32);
    }
    // ---- expand the walked blocks (every read from the LDS segment)
    // (the segment path stores 16-value runs per lane, shifted to 16-byte alignment: pages of
    // nullable columns, which start at any value offset, take it too)
    if ((mbs % 16u) == 0 && ((uint64_t)block * W) % 16u == 0)
      {
        if constexpr (NEG)
          delta_expand_seg<W, NEG>(S, nb, b_data, b_wpos, b_lo, b_hi, b_nmb, blk_first, block, mbs, n_out, carry, out, page,
                                   err, err_count);
        else
          delta_expand_seg<W>(S, nb, b_data, b_wpos, b_lo, b_hi, b_nmb, blk_first, block, mbs, n_out, carry, out);
      }
    else if (E == 1)
      delta_expand<W, NEG, 1>(S, nb, b_data, b_wpos, b_lo, b_hi, b_nmb, blk_first, block, mbs, n_out, carry, out, page, err, err_count);
    else if (E == 2) delta_expand<W, NEG, 2>(S, nb, b_data, b_wpos, b_lo, b_hi, b_nmb, blk_first, block, mbs, n_out, carry, out, page, err, err_count);
    else if (E == 4) delta_expand<W, NEG, 4>(S, nb, b_data, b_wpos, b_lo, b_hi, b_nmb, blk_first, block, mbs, n_out, carry, out, page, err, err_count);
    else delta_expand<W, NEG, 8>(S, nb, b_data, b_wpos, b_lo, b_hi, b_nmb, blk_first, block, mbs, n_out, carry, out, page, err, err_count);
    n_blocks += nb;
  }
  // the value after the last delta of the last block (the expansion stores values up to the one
  // before each block's last delta); only needed when that block was full
  {
    const uint64_t k = (uint64_t)n_blocks * block;
    if (n_blocks && k < n_out && lane == 0) {
      T v = (T)carry;
      if (NEG && (int32_t)(uint32_t)v < 0) {
        report(err, err_count, page, 2, k, PQG_ERR_CORRUPT);
        v = 0;
      }
      gst(out + k, v);
    }
  }
  *p_end = p;
  return 0;
}

// MODE 0: DELTA_BINARY_PACKED values. MODE 1 (DLBA): the lengths of DELTA_LENGTH_BYTE_ARRAY
// pages (DeltaLengthByteArrayValuesReader.initFromPage :44-48 reads them with this reader, then
// takes the remaining stream as the value bytes) -> ColumnDev::blen, value bytes start ->
// PageWork::aux. MODE 2 (DBA): DELTA_BYTE_ARRAY pages (DeltaByteArrayReader.initFromPage :45-48):
// prefix lengths -> bsrc, suffix lengths -> blen, suffix bytes start -> aux; then per value the
// checks of readBytes :57-79 in the reference's order and blen <- prefix + suffix length.
template <int W, int MODE = 0>
__global__ __launch_bounds__(64 * WPB) void k_delta(const uint8_t* __restrict__ bytes, uint64_t n_bytes,
                                              PageWork* __restrict__ work, const ColumnDev* __restrict__ cols,
                                              const int32_t* __restrict__ list, int n_list, uint64_t* err,
                                              ErrCount err_count, uint32_t* __restrict__ dba_meta = nullptr) {
  typedef typename DictVal<W>::T T;
  __shared__ __attribute__((aligned(16))) uint8_t dseg_all[WPB][DSEG];
  const int page = wave_page(list, n_list);
  if (page < 0) return;
  const PageWork pw = work[page];
  const ColumnDev cd = cols[pw.column];
  const uint32_t lane = lane_id();
  const uint32_t beg = uni(pw.data_begin), end = uni(pw.size);
  const uint32_t want = uni(pw.n_values);
  DSeg S;
  S.rs = make_rsrc(bytes + pw.base, n_bytes - pw.base);
  S.seg = dseg_all[wave_id()];
  S.lo = 0x80000000u;  // nothing staged yet (pages are < 2 GiB)
  uint32_t p_end = beg, total = 0;
  T* out = (MODE == 0 ? (T*)cd.values : MODE == 1 ? (T*)cd.blen : (T*)cd.bsrc) + pw.out_offset;
  int code = delta_stream<W, MODE == 1>(S, beg, end, want, out, page, err, err_count, &p_end, &total);
  if (code) {
    if (lane == 0) report(err, err_count, page, 0, 2, code);
    return;
  }
  uint32_t past_end = want > total ? total : 0xFFFFFFFFu;  // first index with no value
  if constexpr (MODE == 2) {
    uint32_t total2 = 0, p2 = p_end;
    code = delta_stream<4, false>(S, p_end, end, want, cd.blen + pw.out_offset, page, err, err_count, &p2, &total2);
    if (code) {
      if (lane == 0) report(err, err_count, page, 0, 2, code);
      return;
    }
    p_end = p2;
    if (want > total2 && total2 < past_end) past_end = total2;
    // readBytes checks per value i, in order: prefix / suffix length past the streams
    // (DELTA_PAST_END), suffix length < 0 (slice(negative)), suffix bytes past the page (EOF),
    // then for prefix != 0: new byte[prefix + suffix] < 0, arraycopy(previous, 0, out, 0, prefix)
    // with prefix < 0 or > previous.length. blen becomes the value length (0 past an error).
    const uint32_t n_chk = want < past_end ? want : past_end;
    const uint32_t avail = end > p_end ? end - p_end : 0;
    uint32_t* pl = cd.bsrc + pw.out_offset;
    uint32_t* sl = cd.blen + pw.out_offset;
    uint64_t s_carry = 0;
    uint32_t prev_len = 0;  // previous value of the page (empty before the first, :41)
    // PQG_PAGE_DBA_CARRY (PARQUET-246, setPreviousReader :89-95): the first value's previous is the
    // column's value out_offset - 1, known only after the earlier pages: its prefix check is made by
    // k_dba_carry, which copies the page in page order
    const bool carry = (uni(pw.pflags) & PQG_PAGE_DBA_CARRY) != 0;
    // FIXED_LEN_BYTE_ARRAY (Encoding.java :219-222): every value must be type_length bytes to fit the
    // fixed-width output
    const int32_t fixw = cd.physical_type == PQG_FIXED_LEN_BYTE_ARRAY ? cd.type_length : 0;
    uint32_t first_bad = 0xFFFFFFFFu;
    // per BIN_CHUNK-value chunk of the page, for the chunk-parallel value copy (k_dba_tail /
    // k_dba_chain / k_dba_chunks): suffix bytes before the chunk, smallest prefix length in it
    uint32_t* meta = dba_meta + 2u * (uint64_t)pw.chunk_base;
    uint32_t lmax = 0;
    // the lengths were just stored by this wave: wait for them, then read past the L1 (a line
    // shared with a neighbouring page may sit in this CU's L1 from before those stores)
    __builtin_amdgcn_s_waitcnt(0);
    // Rounds of DG chunks (BIN_CHUNK = 256 values: lane l holds values 4 l .. 4 l + 3 of a chunk): every
    // length of a round is loaded before the stores of any of it (a load issued after stores waits for
    // them), and a chunk costs one wave scan, min, max and ballot for 256 values (the lane's 4 values
    // are chained in registers), where one per 64 values left the check at half of the kernel.
    static_assert(BIN_CHUNK == 4 * WAVE, "a chunk is 4 values per lane");
    constexpr uint32_t DG = 4;
    for (uint32_t g0 = 0; g0 < n_chk; g0 += DG * BIN_CHUNK) {
    int32_t pre_g[DG][4], suf_g[DG][4];
#pragma unroll
    for (uint32_t d = 0; d < DG; d++)
#pragma unroll
      for (uint32_t q = 0; q < 4; q++) {
        const uint32_t i = g0 + d * BIN_CHUNK + 4u * lane + q;
        pre_g[d][q] = i < n_chk ? (int32_t)sld(pl + i) : 0;
        suf_g[d][q] = i < n_chk ? (int32_t)sld(sl + i) : 0;
      }
    __builtin_amdgcn_s_waitcnt(0);
#pragma unroll
    for (uint32_t d = 0; d < DG; d++) {
      const uint32_t c0 = g0 + d * BIN_CHUNK;  // the chunk's first value
      if (c0 >= n_chk) break;
      const uint32_t ib = c0 + 4u * lane;       // the lane's first value
      uint64_t sv_sum = 0;
#pragma unroll
      for (uint32_t q = 0; q < 4; q++) sv_sum += suf_g[d][q] > 0 ? (uint64_t)suf_g[d][q] : 0;
      const uint64_t incl_l = wave_incl_scan_u64(sv_sum);
      uint64_t run = s_carry + incl_l - sv_sum;  // suffix bytes before the lane's first value
      // previous value's length (clamped at 0) for the lane's first value: the last of lane - 1
      const int32_t f3 = (int32_t)((uint32_t)pre_g[d][3] + (uint32_t)suf_g[d][3]);
      const uint32_t up = __shfl_up((uint32_t)(f3 < 0 ? 0 : f3), 1);
      uint32_t prev = lane == 0 ? prev_len : up;
      uint32_t bad_i = 0xFFFFFFFFu;
      int bad_c = 0;
      int32_t full[4];
#pragma unroll
      for (uint32_t q = 0; q < 4; q++) {
        const uint32_t i = ib + q;
        const int32_t pre = pre_g[d][q], suf = suf_g[d][q];
        full[q] = (int32_t)((uint32_t)pre + (uint32_t)suf);
        run += suf > 0 ? (uint64_t)suf : 0;
        int c = 0;
        if (i < n_chk) {
          if (suf < 0) c = PQG_ERR_CORRUPT;
          else if (run > avail) c = PQG_ERR_EOF;
          else if (pre != 0 && (full[q] < 0 || pre < 0 || ((uint32_t)pre > prev && !(carry && i == 0)))) c = PQG_ERR_CORRUPT;
          else if (fixw && full[q] != fixw) c = PQG_ERR_CORRUPT;
        }
        if (c && bad_i == 0xFFFFFFFFu) {
          bad_i = i;
          bad_c = c;
        }
        prev = full[q] < 0 ? 0u : (uint32_t)full[q];
      }
      // the page's first invalid value (the reference throws there): reported once, every value from
      // it on gets length 0
      const uint32_t wb = uni(wave_min_u32(bad_i));
      if (wb != 0xFFFFFFFFu && first_bad == 0xFFFFFFFFu) {
        first_bad = wb;
        if (bad_i == wb) report(err, err_count, page, 2, wb, bad_c);
      }
      const uint32_t fb = uni(first_bad);
      uint32_t pmn = 0xFFFFFFFFu, lmx = 0;
#pragma unroll
      for (uint32_t q = 0; q < 4; q++) {
        const uint32_t i = ib + q;
        if (i >= n_chk) break;
        const uint32_t Lf = i >= fb ? 0u : (uint32_t)full[q];
        gst(sl + i, Lf);
        const uint32_t pf = Lf ? (uint32_t)pre_g[d][q] : 0u;  // the copy's prefix: min(prefix, length)
        pmn = pf < pmn ? pf : pmn;
        lmx = Lf > lmx ? Lf : lmx;
      }
      const uint32_t cmin = wave_min_u32(pmn), mx = wave_max_u32(lmx);
      lmax = mx > lmax ? mx : lmax;
      if (lane == 0) {
        gst(meta + 2u * (c0 / BIN_CHUNK), (uint32_t)s_carry);
        gst(meta + 2u * (c0 / BIN_CHUNK) + 1u, cmin);
      }
      prev_len = rdl(prev, WAVE - 1);
      s_carry += rdl((uint32_t)incl_l, WAVE - 1) | ((uint64_t)rdl((uint32_t)(incl_l >> 32), WAVE - 1) << 32);
    }
    }
    // chunks past the checked values hold no bytes
    const uint32_t nch = (uint32_t)(((uint64_t)pw.num_slots + BIN_CHUNK - 1) / BIN_CHUNK);
    for (uint32_t j = (n_chk + BIN_CHUNK - 1) / BIN_CHUNK + lane; j < nch; j += WAVE) {
      gst(meta + 2u * j, (uint32_t)s_carry);
      gst(meta + 2u * j + 1u, 0u);
    }
    // a value longer than the LDS value buffers sends the page to the serial copy
    if (lane == 0) work[page].reserved = carry ? 2u : lmax > DBA_VB ? 1u : 0u;
    // values past an error or past the streams hold length 0 (blen was cleared before the launch)
  }
  if (past_end != 0xFFFFFFFFu && lane == 0) report(err, err_count, page, 2, past_end, PQG_ERR_DELTA_PAST_END);
  if (MODE != 0 && lane == 0) work[page].aux = p_end;
}

// ---------------------------------------------------------------------------
// Launchers (host side of this translation unit)

#define PQG_LAUNCH_ARGS bytes, n_bytes, work, cols, list, n, err, err_count

hipError_t launch_levels(hipStream_t st, const uint8_t* bytes, uint64_t n_bytes, PageWork* work, const ColumnDev* cols,
                         const int32_t* list, int n, uint64_t* err, ErrCount err_count, uint32_t* hint_bad) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_levels, dim3((n + WPB - 1) / WPB), dim3(64 * WPB), 0, st, PQG_LAUNCH_ARGS, hint_bad);
  return hipGetLastError();
}

hipError_t launch_scan(hipStream_t st, PageWork* work, const int32_t* col_pages, const int32_t* col_page_start,
                       int n_cols) {
  if (n_cols <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_scan_offsets, dim3(n_cols), dim3(256), 0, st, work, col_pages, col_page_start, n_cols);
  return hipGetLastError();
}

hipError_t launch_rle_bool(hipStream_t st, const uint8_t* bytes, uint64_t n_bytes, PageWork* work,
                           const ColumnDev* cols, const int32_t* list, int n, uint64_t* err, ErrCount err_count) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_rle_bool, dim3((n + WPB - 1) / WPB), dim3(64 * WPB), 0, st, PQG_LAUNCH_ARGS);
  return hipGetLastError();
}

hipError_t launch_delta(int width, hipStream_t st, const uint8_t* bytes, uint64_t n_bytes, PageWork* work,
                        const ColumnDev* cols, const int32_t* list, int n, uint64_t* err, ErrCount err_count) {
  if (n <= 0) return hipSuccess;
  if (width == 8) hipLaunchKernelGGL(k_delta<8>, dim3((n + WPB - 1) / WPB), dim3(64 * WPB), 0, st, PQG_LAUNCH_ARGS);
  else hipLaunchKernelGGL(k_delta<4>, dim3((n + WPB - 1) / WPB), dim3(64 * WPB), 0, st, PQG_LAUNCH_ARGS);
  return hipGetLastError();
}

hipError_t launch_dlba_lengths(hipStream_t st, const uint8_t* bytes, uint64_t n_bytes, PageWork* work,
                               const ColumnDev* cols, const int32_t* list, int n, uint64_t* err, ErrCount err_count) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL((k_delta<4, 1>), dim3((n + WPB - 1) / WPB), dim3(64 * WPB), 0, st, PQG_LAUNCH_ARGS);
  return hipGetLastError();
}

hipError_t launch_dba_lengths(hipStream_t st, const uint8_t* bytes, uint64_t n_bytes, PageWork* work,
                              const ColumnDev* cols, const int32_t* list, int n, uint64_t* err, ErrCount err_count,
                              uint32_t* dba_meta) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL((k_delta<4, 2>), dim3((n + WPB - 1) / WPB), dim3(64 * WPB), 0, st, PQG_LAUNCH_ARGS, dba_meta);
  return hipGetLastError();
}

#ifdef PQG_DIAG
int diag_nostore_kernels(int v) {
  return hipMemcpyToSymbol(HIP_SYMBOL(pqg_diag_nostore), &v, sizeof(v)) == hipSuccess ? 0 : 3;
}
int diag_wph_kernels(void* p) {
  return hipMemcpyToSymbol(HIP_SYMBOL(pqg_diag_wph), &p, sizeof(p)) == hipSuccess ? 0 : 3;
}
#endif

}  // namespace pqg
