// pqgpu_dict_strings.hip — CDNA4 (gfx950) kernels of the dictionary-direct BYTE_ARRAY columns
// (ColumnDev::dict_direct), which run after the id expansion of pqgpu_dict.hip (k_dict_fused_dd): the
// per-column scan of the chunks' byte sums (k_dd_bases), offsets and value bytes from a dictionary page
// staged in LDS (k_dd_str), and the same for dictionaries too large to stage (k_dd_gsums, k_dd_gstr).
// Semantics follow the reference reader value for value:
//   DictionaryValuesReader.readBytes (dictionary/DictionaryValuesReader.java:75-82),
//   PlainBinaryDictionary (dictionary/PlainValuesDictionary.java:58-134).
#include <hip/hip_runtime.h>

#include "pqgpu_device.h"

namespace pqg {

// One workgroup per dictionary-direct column: its chunks are sums[start[2i] .. start[2i + 1]) in page order.
// Exclusive scan in one pass over the column: thread t takes DDB_PER consecutive sums per round (a
// register scan), a workgroup scan of the threads' totals, then each thread writes its bases. (The
// previous 256-sum rounds with two barriers each took 15 us for str_dict's 4,883 chunks.)
constexpr uint32_t DDB_PER = 16;
__global__ __launch_bounds__(256) void k_dd_bases(const PageWork* __restrict__ work, const ColumnDev* __restrict__ cols,
                                                  const uint64_t* __restrict__ chunks, const int32_t* __restrict__ dd_cols,
                                                  const int32_t* __restrict__ start, uint64_t* sums) {
  __shared__ uint64_t wsum[4];
  const ColumnDev& cd = cols[dd_cols[blockIdx.x]];
  const uint32_t b = (uint32_t)start[2 * blockIdx.x], e = (uint32_t)start[2 * blockIdx.x + 1];
  uint64_t carry = 0;
  for (uint32_t c0 = b; c0 < e; c0 += 256u * DDB_PER) {
    const uint32_t i0 = c0 + threadIdx.x * DDB_PER;
    uint64_t v[DDB_PER], own = 0;
#pragma unroll
    for (uint32_t j = 0; j < DDB_PER; j++) {
      v[j] = i0 + j < e ? sums[i0 + j] : 0;
      own += v[j];
    }
    uint64_t x = own;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint64_t y = __shfl_up(x, o);
      if ((int)lane_id() >= o) x += y;
    }
    if (lane_id() == 63) wsum[threadIdx.x >> 6] = x;
    __syncthreads();
    uint64_t pre = carry + x - own, tot = 0;
#pragma unroll
    for (uint32_t w = 0; w < 4; w++) {
      pre += w < (threadIdx.x >> 6) ? wsum[w] : 0;
      tot += wsum[w];
    }
#pragma unroll
    for (uint32_t j = 0; j < DDB_PER; j++) {
      if (i0 + j < e) sums[i0 + j] = pre;
      pre += v[j];
    }
    carry += tot;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    *cd.bin_total = carry;
    // offsets[n]: n = the column's values = the end of its last page's (the last chunk's page: the host
    // pads before a column's first chunk, never after its last; slots for a required column, the non-null
    // count of a nullable one)
    uint64_t n = cd.n_slots;
    if (e > b) {
      const PageWork& lp = work[(uint32_t)chunks[e - 1]];
      n = lp.out_offset + lp.n_values;
    }
    gst((int64_t*)cd.values + n, (int64_t)carry);
  }
}

// Value bytes of the lane's E values (entry e: ln[e] bytes at LDS dd_lds + sr[e]), bytes [q0, q0 + 4 MD)
// of each: all MD dwords of every value and its tail dword are read first, then the stores (whole
// dwords, then a 2- and a 1-byte store for the last 1-3 bytes inside the range). Reads past an entry
// stay inside the workgroup's LDS or return 0; no store leaves the value's own bytes.
template <uint32_t MD>
__device__ __forceinline__ void dd_put(uint8_t* dst, const uint64_t (&o)[4], const uint32_t (&ln)[4],
                                       const uint32_t (&sr)[4], const uint8_t* dd_lds, uint32_t q0 = 0) {
  typedef uint32_t __attribute__((aligned(1), may_alias)) u32u;
  typedef uint32_t __attribute__((aligned(1), may_alias, address_space(1))) g32u;
  typedef uint16_t __attribute__((aligned(1), may_alias, address_space(1))) g16u;
  uint32_t x[4][MD], tl[4];
#pragma unroll
  for (uint32_t e = 0; e < 4; e++) {
#pragma unroll
    for (uint32_t k = 0; k < MD; k++) x[e][k] = *(const u32u*)(dd_lds + sr[e] + q0 + 4u * k);
    tl[e] = *(const u32u*)(dd_lds + sr[e] + (ln[e] & ~3u));
  }
#pragma unroll
  for (uint32_t e = 0; e < 4; e++) {
    uint8_t* ob = dst + o[e];
#pragma unroll
    for (uint32_t k = 0; k < MD; k++)
      if (q0 + 4u * k + 4u <= ln[e]) *(g32u*)(ob + q0 + 4u * k) = x[e][k];
    const uint32_t q = ln[e] & ~3u, r = ln[e] & 3u;
    if (r && q >= q0 && q < q0 + 4u * MD) {
      if (r & 2u) *(g16u*)(ob + q) = (uint16_t)tl[e];
      if (r & 1u) gst(ob + q + (r & 2u), (uint8_t)(tl[e] >> (8u * (r & 2u))));
    }
  }
}

// Block gather of k_dd_str (entries of 2 .. DDG_MD_MAX bytes): per tile, each wave writes its values'
// tile-relative starts and entries to LDS and, for every 16-byte output block, the value holding the
// block's first byte (each value marks the blocks whose first byte it holds); then every lane composes
// whole blocks from the staged dictionary page (a 16-byte unaligned LDS read per value piece, masked and
// shifted into the block) and stores them as one aligned 16-byte store: 64 KB of value bytes per 4,096
// store instructions, where storing each value's own bytes (dd_put) scattered dword / short / byte stores
// at lane strides (C4: 24.7 M store instructions per launch, the kernel's bound).
constexpr uint32_t DDG_MD_MAX = 32;
constexpr uint32_t DD_SPLIT_MAX_CHUNKS = 16384;  // k_dd_str: a workgroup per chunk up to this many chunks
constexpr uint32_t DDG_FV = (WAVE * 4u * DDG_MD_MAX) / 16u + 2u;
struct DdgLds {
  uint32_t vo[WAVE * 4];  // tile-relative first byte of value v
  uint32_t ve[WAVE * 4];  // entry: source << 16 | length (0: empty / out of range)
  uint16_t fv[DDG_FV];    // block b: the value holding its first byte
};
constexpr uint32_t DDG_WAVE_BYTES = (sizeof(DdgLds) + 15u) & ~15u;

// One wave per output chunk of k_dict_fused_dd (chunks of one column per workgroup: the plan pads the
// chunk list). The chunk's ids are loaded first, all of them (one dword per tile per lane for u8 ids,
// two for u16: no load after the first store, whose wait would drain the stores), then per 256-value
// tile: the entries from the staged table, a wave scan of the lanes' byte counts, the offsets as two
// 16-byte stores per lane, and each value's bytes from the staged dictionary page as unaligned dword
// stores plus a 2- and a 1-byte store for its last 1-3 bytes (no store leaves the value's own bytes).
// Slots of a page past a walk error (pstat) are empty values. dd_region: LDS bytes of the staged page
// (16-byte rounded) + its u32 entry table (source << 16 | length).
template <uint32_t TPW>
__global__ __launch_bounds__(64 * WPB) void k_dd_str(const uint8_t* __restrict__ bytes, uint64_t n_bytes,
                                                     const PageWork* __restrict__ work,
                                                     const ColumnDev* __restrict__ cols,
                                                     const uint64_t* __restrict__ chunks, uint32_t n_chunks,
                                                     const uint64_t* pstat, const uint64_t* __restrict__ bases,
                                                     uint64_t* err, ErrCount err_count, uint32_t dd_region) {
  typedef uint32_t __attribute__((aligned(1), may_alias, address_space(1))) g32u;
  typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
  typedef int64_t i64x2 __attribute__((ext_vector_type(2)));
  constexpr uint32_t E = 4, TV = WAVE * E, CH = CH_TILES * TV;
  // the staged dictionary page at dd_raw + 16 (16 bytes of slack before it for the block gather's reads)
  extern __shared__ __attribute__((aligned(16))) uint8_t dd_raw[];
  uint8_t* const dd_lds = dd_raw + 16;
  __shared__ int wg_col[WPB];
  // block gather: v_perm selectors taking bytes k .. 15 of a block from the source, the rest from the
  // accumulated block (dd_sel[k], dword d: byte j <- source when 4 d + j >= k)
  __shared__ u32x4 dd_sel[16];
  if (threadIdx.x < 64u) {
    const uint32_t k = threadIdx.x >> 2, d = threadIdx.x & 3u;
    uint32_t sel = 0;
#pragma unroll
    for (uint32_t jb = 0; jb < 4; jb++) sel |= (4u * d + jb >= k ? 4u + jb : jb) << (8u * jb);
    ((uint32_t*)dd_sel)[threadIdx.x] = sel;
  }
  const uint32_t lane = lane_id();
  // TPW = CH_TILES: one chunk per wave. TPW = CH_TILES / WPB: one workgroup per chunk, wave w takes tiles
  // [T0, T1) of it (4x the workgroups: str_dict's 4,883 chunks filled 1.2 rounds of the chip's workgroup
  // slots, the second one a fifth: 0.321 -> 0.274 ms; C4's 122 k chunks keep a chunk per wave, 10.50 vs
  // 10.63 ms; profiles/r05/dd_split)
  static_assert(TPW == CH_TILES || TPW * WPB == CH_TILES, "a chunk per wave or per workgroup");
  constexpr bool SPLIT = TPW < CH_TILES;
  const uint32_t c = SPLIT ? blockIdx.x : blockIdx.x * WPB + wave_id();
  const uint32_t T0 = SPLIT ? wave_id() * TPW : 0u, T1 = T0 + TPW;
  __shared__ uint32_t wsum[WPB];
  const int page = c < n_chunks ? (int)(uint32_t)chunks[c] : -1;
  if (lane == 0) wg_col[wave_id()] = page >= 0 ? work[page].column : -1;
  __syncthreads();
  int c0 = -1;
  bool same = true;
#pragma unroll
  for (int q = 0; q < WPB; q++) {
    const int cq = wg_col[q];
    if (cq >= 0) {
      if (c0 < 0) c0 = cq;
      else if (cq != c0) same = false;
    }
  }
  uint32_t ent_off = 0;
  bool staged = false;
  if (same && c0 >= 0) {  // the dictionary page, then the entry table
    const ColumnDev& cd0 = cols[c0];
    const uint32_t dn = uni(cd0.dict_n);
    ent_off = (uint32_t)((cd0.dict_bytes + 15u) & ~15ull);
    staged = dn <= DD_ENT_MAX && cd0.dict_bytes <= DD_DICT_MAX && ent_off + 4u * dn <= dd_region;
    if (staged) {
      uint32_t* ent = (uint32_t*)(dd_lds + ent_off);
      for (uint32_t i = threadIdx.x; i < dn; i += 64u * WPB) ent[i] = (cd0.dict_src[i] << 16) | cd0.dict_len[i];
      // (a resource over the rest of the batch: a 16-byte load crossing the end of its range would
      // return 0 as a whole; only entry bytes are ever read from the staged page)
      const rsrc_t d0 = make_rsrc(bytes + cd0.dict_offset, n_bytes - cd0.dict_offset);
      for (uint32_t o = 16u * threadIdx.x; o < ent_off; o += 16u * 64u * WPB)
        *(u32x4*)(dd_lds + o) = __builtin_amdgcn_raw_buffer_load_b128(d0, (int)o, 0, 0);
    }
  }
  __syncthreads();
  if (page < 0) return;
  const PageWork pw = work[page];
  const ColumnDev& cd = cols[pw.column];
  const uint32_t j = (uint32_t)(chunks[c] >> 32);
  if (!staged || pw.column != c0) {
    // (never with the plan's layout: whole workgroups per column, dictionaries within DD_DICT_MAX /
    // 2,048 entries and within the launch's dd_region)
    if (lane == 0) report(err, err_count, page, 2, 0, PQG_ERR_INVALID_ARG);
    return;
  }
  const uint32_t dict_n = uni(cd.dict_n), idw = uni(cd.dict_direct);
  // longest entry (its bytes decide the store shapes below) and whether every entry is 1 byte long
  uint32_t md = 0, mn = 0xFFFFu;
  for (uint32_t i = lane; i < dict_n; i += WAVE) {
    const uint32_t l = ((const uint32_t*)(dd_lds + ent_off))[i] & 0xFFFFu;
    md = l > md ? l : md;
    mn = l < mn ? l : mn;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const uint32_t a = (uint32_t)__shfl_xor((int)md, o), b = (uint32_t)__shfl_xor((int)mn, o);
    md = a > md ? a : md;
    mn = b < mn ? b : mn;
  }
  md = uni(md);
  const bool one = uni(mn) == 1u && md == 1u;
  const uint32_t NF = uni(pw.n_values);
  const uint32_t nok = uni((uint32_t)(sld(pstat + page) >> 32));  // values before a walk error
  const uint32_t sh = (uint32_t)(pw.out_offset % E);
  const uint32_t s_lo = j * CH > sh ? j * CH : sh;
  const uint32_t s_hi = (j + 1) * CH < NF + sh ? (j + 1) * CH : NF + sh;
  if (s_lo >= s_hi) return;
  const uint32_t ok_hi = (nok < NF ? nok : NF) + sh;  // slots [ok_hi, s_hi): empty values
  // the wave's ids: tile T0 + t -> lane's 4 ids (u8: dword t; u16: dwords 2t, 2t + 1)
  const uint8_t* idpag = (const uint8_t*)cd.blen + (pw.out_offset - sh) * (uint64_t)idw;
  uint32_t idr[2 * TPW];
#pragma unroll
  for (uint32_t t = 0; t < TPW; t++) {
    const uint32_t ts = j * CH + (T0 + t) * TV;
    const uint8_t* ip = idpag + (uint64_t)(ts + E * lane) * idw;
    const bool any = ts + E * lane < s_hi;  // (the id array is padded: the ids after a lane's first are readable)
    if (idw == 1u) {
      idr[2 * t] = any ? *(const __attribute__((address_space(1))) uint32_t*)ip : 0u;
      idr[2 * t + 1] = 0u;
    } else {
      const u32x2 x = any ? *(const __attribute__((address_space(1))) u32x2*)ip : u32x2{0u, 0u};
      idr[2 * t] = x.x;
      idr[2 * t + 1] = x.y;
    }
  }
  const uint32_t* ent = (const uint32_t*)(dd_lds + ent_off);
  uint8_t* const dst = cd.binary_data;
  const uint64_t cap = cd.binary_capacity;
  int64_t* const opag = (int64_t*)cd.values + (pw.out_offset - sh);  // offsets of the page's slot 0
  const bool o16 = ((uintptr_t)cd.values & 15u) == 0;
  // block gather: entries of 2 .. DDG_MD_MAX bytes into a 16-byte aligned value buffer
  const bool gather = !one && md <= DDG_MD_MAX && ((uintptr_t)dst & 15u) == 0;
  DdgLds& G = *(DdgLds*)(dd_lds + ((dd_region + 15u) & ~15u) + wave_id() * DDG_WAVE_BYTES);
  // a tile's partial last block, finished by the next tile (uniform): bytes [cb_lo, cb_hi) of the block
  // at cb_tal; cx / cxlo: the carrying lane's copy
  bool cb_on = false;
  uint32_t cb_w[4] = {0, 0, 0, 0}, cb_lo = 0, cb_hi = 0, cx[4] = {0, 0, 0, 0}, cxlo = 0;
  uint64_t cb_tal = 0;
  // the wave's first byte: the chunk's plus the bytes of the lower waves' tiles (SPLIT; the waves of a
  // workgroup then share its chunk, so none of them has returned above)
  if constexpr (SPLIT) {
    uint32_t ws = 0;
#pragma unroll
    for (uint32_t t = 0; t < TPW; t++) {
      const uint32_t ts = j * CH + (T0 + t) * TV;
#pragma unroll
      for (uint32_t e = 0; e < E; e++) {
        const uint32_t sl = ts + E * lane + e;
        const uint32_t id = idw == 1u ? (idr[2 * t] >> (8u * e)) & 0xFFu
                                      : (idr[2 * t + (e >> 1)] >> (16u * (e & 1u))) & 0xFFFFu;
        ws += sl >= s_lo && sl < ok_hi && id < dict_n ? ent[id] & 0xFFFFu : 0u;
      }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) ws += (uint32_t)__shfl_xor((int)ws, o);
    if (lane == 0) wsum[wave_id()] = ws;
    __syncthreads();
  }
  uint64_t run_base = uni64(bases[c]);
  if constexpr (SPLIT) {
    for (uint32_t w = 0; w < wave_id(); w++) run_base += wsum[w];
    run_base = uni64(run_base);
  }
#pragma unroll 1
  for (uint32_t t = T0; t < T1; t++) {
    const uint32_t ts = uni(j * CH + t * TV);
    if (ts >= s_hi) break;
    uint32_t ln[E], sr[E], ls = 0;
#pragma unroll
    for (uint32_t e = 0; e < E; e++) {
      const uint32_t sl = ts + E * lane + e;
      const uint32_t id = idw == 1u ? (idr[2 * (t - T0)] >> (8u * e)) & 0xFFu
                                    : (idr[2 * (t - T0) + (e >> 1)] >> (16u * (e & 1u))) & 0xFFFFu;
      const uint32_t en = sl >= s_lo && sl < ok_hi && id < dict_n ? ent[id] : 0u;
      ln[e] = en & 0xFFFFu;
      sr[e] = en >> 16;
      ls += ln[e];
    }
    const uint32_t inc = wave_incl_scan_u32_dpp(ls);
    const uint32_t tot = uni(rdl(inc, WAVE - 1));
    uint64_t o[E];
    o[0] = run_base + (inc - ls);
#pragma unroll
    for (uint32_t e = 1; e < E; e++) o[e] = o[e - 1] + ln[e - 1];
    int64_t* op = opag + ts + E * lane;
    if (o16 && ts >= s_lo && ts + TV <= s_hi) {
      gst_nt((i64x2*)op, i64x2{(int64_t)o[0], (int64_t)o[1]});
      gst_nt((i64x2*)(op + 2), i64x2{(int64_t)o[2], (int64_t)o[3]});
    } else {
#pragma unroll
      for (uint32_t e = 0; e < E; e++)
        if (ts + E * lane + e >= s_lo && ts + E * lane + e < s_hi) gst(op + e, (int64_t)o[e]);
    }
    const uint64_t tb = run_base;  // the tile's first byte
    run_base += tot;
    if (run_base <= cap && gather) {
      wave_sync();  // the previous tile's gather reads are done
      // positions relative to the tile's first 16-byte block (32-bit): bytes [rb, re)
      const uint64_t tal = tb & ~15ull;
      const uint32_t rb = (uint32_t)(tb - tal), re = rb + tot;
#pragma unroll
      for (uint32_t e = 0; e < E; e++) {
        G.vo[E * lane + e] = rb + (uint32_t)(o[e] - tb);
        G.ve[E * lane + e] = (sr[e] << 16) | ln[e];
      }
      const uint32_t nblk = (re + 15u) >> 4;
#pragma unroll
      for (uint32_t e = 0; e < E; e++) {
        if (!ln[e]) continue;
        // the blocks whose first byte (16 b, or rb for the tile's first block) this value holds
        const uint32_t g = rb + (uint32_t)(o[e] - tb);
        for (uint32_t b = g == rb ? (g >> 4) : ((g + 15u) >> 4); (b << 4) < g + ln[e]; b++) G.fv[b] = (uint16_t)(E * lane + e);
      }
      wave_sync();
      // the tile's last block, when partial, is finished by the next tile of the chunk (same wave)
      const bool next_tile = t + 1 < T1 && ts + TV < s_hi;
      for (uint32_t b = lane; b < nblk; b += WAVE) {
        const uint32_t gb = b << 4;
        uint32_t bs = gb > rb ? gb : rb;
        const uint32_t be = gb + 16u < re ? gb + 16u : re;
        uint32_t v = G.fv[b];
        uint32_t a0 = 0, a1 = 0, a2 = 0, a3 = 0;
        if (b == 0 && cb_on) {  // the previous tile's partial last block (uniform carry)
          a0 = cb_w[0]; a1 = cb_w[1]; a2 = cb_w[2]; a3 = cb_w[3];
          bs = cb_lo;
        }
        uint32_t pos = gb > rb ? gb : rb;
        while (pos < be) {
          const uint32_t g = G.vo[v], ev = G.ve[v];
          const uint32_t ge = g + (ev & 0xFFFFu);
          if (pos < ge) {  // (empty values hold no byte)
            const uint32_t n = (ge < be ? ge : be) - pos;  // bytes of this piece
            const uint32_t k = pos - gb;                    // their place in the block
            // the 16 page bytes that line up with the block: page offset (source of pos) - k, read
            // through the 16 bytes of slack before the staged page
            const uint32_t base = 16u + (ev >> 16) + (pos - g) - k;
            const uint32_t q = base & ~3u, r = base & 3u;
            const uint32_t* w = (const uint32_t*)(dd_raw + q);
            const uint32_t w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3], w4 = w[4];
            // block bytes k .. 15 from the source (a later piece overwrites from its own k on; bytes
            // past the block's end are not stored)
            const u32x4 sl = dd_sel[k];
            a0 = __builtin_amdgcn_perm(__builtin_amdgcn_alignbyte(w1, w0, r), a0, sl.x);
            a1 = __builtin_amdgcn_perm(__builtin_amdgcn_alignbyte(w2, w1, r), a1, sl.y);
            a2 = __builtin_amdgcn_perm(__builtin_amdgcn_alignbyte(w3, w2, r), a2, sl.z);
            a3 = __builtin_amdgcn_perm(__builtin_amdgcn_alignbyte(w4, w3, r), a3, sl.w);
            pos += n;
          }
          v++;
        }
        const uint32_t wd[4] = {a0, a1, a2, a3};
        if (b == nblk - 1u && be < gb + 16u && next_tile) {  // carried: the lane's values go to the next tile
          cx[0] = a0; cx[1] = a1; cx[2] = a2; cx[3] = a3;
          cxlo = bs - gb;
        } else {
          uint32_t have = 0;
#pragma unroll
          for (uint32_t d = 0; d < 4; d++) have |= (gb + 4u * d >= bs && gb + 4u * d + 4u <= be ? 1u : 0u) << d;
          store_block16(dst, tal + gb, tal + bs, tal + be, wd, have, true);
        }
      }
      // the partial last block of this tile (lane (nblk - 1) % 64) as uniform values for the next tile,
      // whose block 0 is the same 16 bytes (its first byte continues this tile's last)
      const bool carried = nblk && next_tile && (re & 15u) != 0u;
      if (carried) {
        const uint32_t cl = (nblk - 1u) & (WAVE - 1u);
#pragma unroll
        for (uint32_t d = 0; d < 4; d++) cb_w[d] = rdl(cx[d], cl);
        cb_lo = rdl(cxlo, cl);
      } else if (cb_on && nblk == 0) {  // (a tile without bytes: the carried block is stored as is)
        if (lane == 0) {
          uint32_t have = 0;
#pragma unroll
          for (uint32_t d = 0; d < 4; d++) have |= (4u * d >= cb_lo && 4u * d + 4u <= cb_hi ? 1u : 0u) << d;
          store_block16(dst, cb_tal, cb_tal + cb_lo, cb_tal + cb_hi, cb_w, have, true);
        }
      }
      cb_on = carried;
      cb_hi = re & 15u;
      cb_tal = tal + ((uint64_t)(nblk ? nblk - 1u : 0u) << 4);
    } else if (run_base <= cap) {
      if (one && ls == E) {  // 1-byte entries, the lane's 4 values in range: one dword
        uint32_t x = 0;
#pragma unroll
        for (uint32_t e = 0; e < E; e++) x |= (uint32_t)dd_lds[sr[e]] << (8u * e);
        *(g32u*)(dst + o[0]) = x;
      } else if (md <= 4u) {
        dd_put<1>(dst, o, ln, sr, dd_lds);
      } else if (md <= 8u) {
        dd_put<2>(dst, o, ln, sr, dd_lds);
      } else {
        // 16 bytes per value a round: every LDS read of a round before its stores (a read per store
        // waited for the LDS latency once per dword)
        for (uint32_t q0 = 0; q0 < md; q0 += 16u) dd_put<4>(dst, o, ln, sr, dd_lds, q0);
      }
    } else {  // past the capacity (reported at sync with the size needed): the bytes that fit
      if (cb_on) {  // the previous tile's carried partial block: its bytes below the capacity
        if (lane == 0) {
          const uint64_t hi = cb_tal + cb_hi < cap ? cb_tal + cb_hi : cap;
          store_block16(dst, cb_tal, cb_tal + cb_lo, hi, cb_w, 0u, true);
        }
        cb_on = false;
      }
#pragma unroll
      for (uint32_t e = 0; e < E; e++)
        for (uint32_t q = 0; q < ln[e]; q++)
          if (o[e] + q < cap) gst(dst + o[e] + q, dd_lds[sr[e] + q]);
    }
  }
}

// ---------------------------------------------------------------------------
// Dictionary-direct columns whose dictionary page is too large to stage in LDS (ColumnDev::dd_global: over
// DD_DICT_MAX bytes or 2,048 entries, at most 65,536 entries): the walk's expansion stores the u16 ids only
// (DD_IDS); the entries (PlainBinaryDictionary, PlainValuesDictionary.java:58-134: dict_len / dict_src from
// the dictionary walk) and the value bytes are gathered from HBM — a dictionary of a few hundred KB stays
// in L2 — by the two kernels below, with k_dd_bases between them. Ids past the dictionary and slots past a
// walk error are empty values (the walk reports the error), as k_dd_str writes them.

// Byte sum of every chunk: one wave per chunk, all its ids loaded first (two dwords per lane per tile),
// then the walked slots' entry lengths, summed over the wave (no stores but the sum).
__global__ __launch_bounds__(64 * WPB) void k_dd_gsums(const PageWork* __restrict__ work, const ColumnDev* __restrict__ cols,
                                                     const uint64_t* __restrict__ chunks, uint32_t n_chunks,
                                                     const uint64_t* pstat, uint64_t* sums) {
  typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
  constexpr uint32_t E = 4, TV = WAVE * E, CH = CH_TILES * TV;
  const uint32_t lane = lane_id();
  const uint32_t c = blockIdx.x * WPB + wave_id();
  if (c >= n_chunks) return;
  const uint64_t ce = chunks[c];
  if ((uint32_t)ce == 0xFFFFFFFFu) return;  // padding between columns (never summed)
  const int page = (int)(uint32_t)ce;
  const PageWork pw = work[page];
  const ColumnDev& cd = cols[pw.column];
  const uint32_t j = (uint32_t)(ce >> 32);
  const uint32_t dict_n = uni(cd.dict_n), NF = uni(pw.n_values);
  const uint32_t nok = uni((uint32_t)(sld(pstat + page) >> 32));  // values before a walk error
  const uint32_t sh = (uint32_t)(pw.out_offset % E);
  const uint32_t s_lo = j * CH > sh ? j * CH : sh;
  const uint32_t s_hi = (j + 1) * CH < NF + sh ? (j + 1) * CH : NF + sh;
  const uint32_t ok_hi = (nok < NF ? nok : NF) + sh;
  uint64_t acc = 0;
  if (s_lo < s_hi) {
    const uint16_t* idpag = (const uint16_t*)cd.blen + (pw.out_offset - sh);
    u32x2 idr[CH_TILES];
#pragma unroll
    for (uint32_t t = 0; t < CH_TILES; t++) {
      const uint32_t ts = j * CH + t * TV;
      idr[t] = ts + E * lane < s_hi ? *(const __attribute__((address_space(1))) u32x2*)(idpag + ts + E * lane)
                                     : u32x2{0u, 0u};
    }
#pragma unroll
    for (uint32_t t = 0; t < CH_TILES; t++) {
      const uint32_t ts = j * CH + t * TV;
#pragma unroll
      for (uint32_t e = 0; e < E; e++) {
        const uint32_t sl = ts + E * lane + e;
        const uint32_t id = ((e < 2 ? idr[t].x : idr[t].y) >> (16u * (e & 1u))) & 0xFFFFu;
        const bool ok = sl >= s_lo && sl < ok_hi && id < dict_n;
        acc += ok ? cd.dict_len[ok ? id : 0u] : 0u;
      }
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) acc += (uint64_t)__shfl_xor((long long)acc, o);
  if (lane == 0) gst(sums + c, acc);
}

// Offsets and value bytes: one workgroup per 4,096-value chunk, wave w its tiles [4 w, 4 w + 4). The
// wave's ids, then its values' entries (lane: 4 per tile), are loaded before the first store; per tile
// a wave scan of the lengths gives the offsets (two 16-byte stores per lane), and the value bytes of
// entries of at most 32 bytes go through LDS: each value's 32 source bytes (two 16-byte loads from the
// dictionary page, the next tile's requested before this tile's stores) into a staging slot, then every
// lane composes whole 16-byte output blocks from the slots (k_dd_str's block gather) and stores them
// aligned, a tile's edge blocks byte-masked. A tile with a longer entry copies bytes one by one.
constexpr uint32_t DDX_MD = 32;  // longest entry of the block path (= staging bytes per value)
// (16-bit offsets and 8-bit block owners: 39.4 KB per workgroup, 4 workgroups per CU instead of 3)
struct DdxLds {
  uint8_t pre[16];                               // slack before the staging (the gather reads base - k)
  uint32_t stg[WAVE * 4 * DDX_MD / 4 + 8];       // lane l's value e: 32 source bytes at 32 (64 e + l) (+ slack)
  uint16_t vo[WAVE * 4];                         // tile-relative first output byte of value v (< 8,208)
  uint16_t ve[WAVE * 4];                         // staging slot << 6 | length (<= 32)
  uint8_t fv[(WAVE * 4 * DDX_MD) / 16 + 2];      // output block b: the value (< 256) holding its first byte
};
__global__ __launch_bounds__(64 * WPB) void k_dd_gstr(const uint8_t* __restrict__ bytes, uint64_t n_bytes,
                                                    const PageWork* __restrict__ work, const ColumnDev* __restrict__ cols,
                                                    const uint64_t* __restrict__ chunks, uint32_t n_chunks,
                                                    const uint64_t* pstat, const uint64_t* __restrict__ bases,
                                                    uint64_t* err, ErrCount err_count) {
  typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
  typedef int64_t i64x2 __attribute__((ext_vector_type(2)));
  constexpr uint32_t E = 4, TV = WAVE * E, CH = CH_TILES * TV, TPW = CH_TILES / WPB;
  __shared__ __attribute__((aligned(16))) DdxLds lds_all[WPB];
  __shared__ u32x4 dd_sel[16];  // (k_dd_str's selectors: block bytes k .. 15 from the source)
  __shared__ uint32_t wsum[WPB];
  if (threadIdx.x < 64u) {
    const uint32_t k = threadIdx.x >> 2, d = threadIdx.x & 3u;
    uint32_t sel = 0;
#pragma unroll
    for (uint32_t jb = 0; jb < 4; jb++) sel |= (4u * d + jb >= k ? 4u + jb : jb) << (8u * jb);
    ((uint32_t*)dd_sel)[threadIdx.x] = sel;
  }
  __syncthreads();
  const uint32_t lane = lane_id();
  const uint32_t c = blockIdx.x;  // (the workgroup's waves share the chunk: uniform exits below)
  if (c >= n_chunks) return;
  const uint64_t ce = chunks[c];
  if ((uint32_t)ce == 0xFFFFFFFFu) return;
  const int page = (int)(uint32_t)ce;
  const PageWork pw = work[page];
  const ColumnDev& cd = cols[pw.column];
  const uint32_t j = (uint32_t)(ce >> 32);
  const uint32_t dict_n = uni(cd.dict_n), NF = uni(pw.n_values);
  const uint32_t nok = uni((uint32_t)(sld(pstat + page) >> 32));
  const uint32_t sh = (uint32_t)(pw.out_offset % E);
  const uint32_t s_lo = j * CH > sh ? j * CH : sh;
  const uint32_t s_hi = (j + 1) * CH < NF + sh ? (j + 1) * CH : NF + sh;
  if (s_lo >= s_hi) return;
  const uint32_t ok_hi = (nok < NF ? nok : NF) + sh;
  const uint32_t T0 = wave_id() * TPW;
  // ids, then entries (all loads before the first store)
  const uint16_t* idpag = (const uint16_t*)cd.blen + (pw.out_offset - sh);
  u32x2 idr[TPW];
#pragma unroll
  for (uint32_t t = 0; t < TPW; t++) {
    const uint32_t ts = j * CH + (T0 + t) * TV;
    idr[t] = ts + E * lane < s_hi ? *(const __attribute__((address_space(1))) u32x2*)(idpag + ts + E * lane)
                                   : u32x2{0u, 0u};
  }
  uint32_t ln[TPW][E], sr[TPW][E], ws = 0;
#pragma unroll
  for (uint32_t t = 0; t < TPW; t++) {
    const uint32_t ts = j * CH + (T0 + t) * TV;
#pragma unroll
    for (uint32_t e = 0; e < E; e++) {
      const uint32_t sl = ts + E * lane + e;
      const uint32_t id = ((e < 2 ? idr[t].x : idr[t].y) >> (16u * (e & 1u))) & 0xFFFFu;
      const bool ok = sl >= s_lo && sl < ok_hi && id < dict_n;
      const uint64_t en = cd.dict_ent[ok ? id : 0u];  // (branch-free: see ld8_any)
      ln[t][e] = ok ? (uint32_t)en : 0u;
      sr[t][e] = ok ? (uint32_t)(en >> 32) : 0u;
      ws += ln[t][e];
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) ws += (uint32_t)__shfl_xor((int)ws, o);
  if (lane == 0) wsum[wave_id()] = ws;
  __syncthreads();
  uint64_t run_base = uni64(bases[c]);
  for (uint32_t w = 0; w < wave_id(); w++) run_base += wsum[w];
  run_base = uni64(run_base);
  uint8_t* const dst = cd.binary_data;
  const uint64_t cap = cd.binary_capacity;
  int64_t* const opag = (int64_t*)cd.values + (pw.out_offset - sh);
  const bool o16 = ((uintptr_t)cd.values & 15u) == 0, d16 = ((uintptr_t)dst & 15u) == 0;
  // the dictionary page + the batch's readable slack after it: a load at DDX_OOB is out of range (no access)
  const rsrc_t drs = make_rsrc(bytes + cd.dict_offset, cd.dict_bytes + 64u);
  constexpr uint32_t DDX_OOB = 0x7FFFFFF0u;
  const rsrc_t brs = make_rsrc(bytes + cd.dict_offset, n_bytes - cd.dict_offset);  // (long entries, byte by byte)
  DdxLds& X = lds_all[wave_id()];
  const uint8_t* const xb = (const uint8_t*)&X;  // staged source s is at xb + 16 + s
  // the 32 source bytes of the lane's 4 values of tile t (entries over 32 bytes: the byte path)
  u32x4 pb[E][2];
  auto load_tile = [&](uint32_t t) {
#pragma unroll
    for (uint32_t e = 0; e < E; e++) {  // (out-of-range offsets for empty values / bytes 16.. of short ones)
      pb[e][0] = __builtin_amdgcn_raw_buffer_load_b128(drs, (int)(ln[t][e] ? sr[t][e] : DDX_OOB), 0, 0);
      pb[e][1] = __builtin_amdgcn_raw_buffer_load_b128(drs, (int)(ln[t][e] > 16u ? sr[t][e] + 16u : DDX_OOB), 0, 0);
    }
  };
  load_tile(0);
#pragma unroll
  for (uint32_t t = 0; t < TPW; t++) {
    const uint32_t ts = j * CH + (T0 + t) * TV;
    if (ts >= s_hi) break;  // (uniform)
    uint32_t ls = 0, mx = 0;
#pragma unroll
    for (uint32_t e = 0; e < E; e++) {
      ls += ln[t][e];
      mx = ln[t][e] > mx ? ln[t][e] : mx;
    }
    const uint32_t inc = wave_incl_scan_u32_dpp(ls);
    const uint32_t tot = uni(rdl(inc, WAVE - 1));
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const uint32_t y = (uint32_t)__shfl_xor((int)mx, o);
      mx = y > mx ? y : mx;
    }
    mx = uni(mx);
    uint64_t o[E];
    o[0] = run_base + (inc - ls);
#pragma unroll
    for (uint32_t e = 1; e < E; e++) o[e] = o[e - 1] + ln[t][e - 1];
    const uint64_t tb = run_base;
    run_base += tot;
    const bool gather = mx <= DDX_MD && d16 && run_base <= cap;
    const uint64_t tal = tb & ~15ull;
    const uint32_t rb = (uint32_t)(tb - tal), re = rb + tot;
    if (gather) {
      wave_sync();  // the previous tile's gather reads are done
#pragma unroll
      for (uint32_t e = 0; e < E; e++) {
        // slots 64 e + lane: consecutive lanes 32 bytes apart (slots 4 lane + e, 128 bytes apart, put a
        // 16-byte write of every lane on two bank groups)
        const uint32_t v = E * lane + e, slot = WAVE * e + lane;
        *(u32x4*)&X.stg[8u * slot] = pb[e][0];
        *(u32x4*)&X.stg[8u * slot + 4u] = pb[e][1];
        X.vo[v] = (uint16_t)(rb + (uint32_t)(o[e] - tb));
        X.ve[v] = (uint16_t)((slot << 6) | ln[t][e]);
      }
#pragma unroll
      for (uint32_t e = 0; e < E; e++) {
        if (!ln[t][e]) continue;
        // the blocks whose first byte (16 b, or rb for the tile's first block) this value holds
        const uint32_t g = rb + (uint32_t)(o[e] - tb);
        for (uint32_t b = g == rb ? (g >> 4) : ((g + 15u) >> 4); (b << 4) < g + ln[t][e]; b++)
          X.fv[b] = (uint8_t)(E * lane + e);
      }
    }
    // the next tile's source bytes, requested before this tile's stores
    if (t + 1 < TPW) load_tile(t + 1);
    int64_t* op = opag + ts + E * lane;
    if (o16 && ts >= s_lo && ts + TV <= s_hi) {
      gst_nt((i64x2*)op, i64x2{(int64_t)o[0], (int64_t)o[1]});
      gst_nt((i64x2*)(op + 2), i64x2{(int64_t)o[2], (int64_t)o[3]});
    } else {
#pragma unroll
      for (uint32_t e = 0; e < E; e++)
        if (ts + E * lane + e >= s_lo && ts + E * lane + e < s_hi) gst(op + e, (int64_t)o[e]);
    }
    if (gather) {
      wave_sync();
      const uint32_t nblk = (re + 15u) >> 4;
      for (uint32_t b = lane; b < nblk; b += WAVE) {
        const uint32_t gb = b << 4;
        const uint32_t bs = gb > rb ? gb : rb;
        const uint32_t be = gb + 16u < re ? gb + 16u : re;
        uint32_t v = X.fv[b];
        uint32_t a0 = 0, a1 = 0, a2 = 0, a3 = 0;
        uint32_t pos = bs;
        while (pos < be) {
          const uint32_t g = X.vo[v], ev = X.ve[v];
          const uint32_t ge = g + (ev & 63u);
          if (pos < ge) {  // (empty values hold no byte)
            const uint32_t n = (ge < be ? ge : be) - pos;
            const uint32_t k = pos - gb;
            const uint32_t base = 16u + DDX_MD * (ev >> 6) + (pos - g) - k;
            const uint32_t q = base & ~3u, r = base & 3u;
            const uint32_t* w = (const uint32_t*)(xb + q);
            const uint32_t w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3], w4 = w[4];
            const u32x4 sl = dd_sel[k];
            a0 = __builtin_amdgcn_perm(__builtin_amdgcn_alignbyte(w1, w0, r), a0, sl.x);
            a1 = __builtin_amdgcn_perm(__builtin_amdgcn_alignbyte(w2, w1, r), a1, sl.y);
            a2 = __builtin_amdgcn_perm(__builtin_amdgcn_alignbyte(w3, w2, r), a2, sl.z);
            a3 = __builtin_amdgcn_perm(__builtin_amdgcn_alignbyte(w4, w3, r), a3, sl.w);
            pos += n;
          }
          v++;
        }
        const uint32_t wd[4] = {a0, a1, a2, a3};
        uint32_t have = 0;
#pragma unroll
        for (uint32_t d = 0; d < 4; d++) have |= (gb + 4u * d >= bs && gb + 4u * d + 4u <= be ? 1u : 0u) << d;
        store_block16(dst, tal + gb, tal + bs, tal + be, wd, have, true);
      }
    } else {  // entries over 32 bytes, an unaligned value buffer, or past the capacity: the bytes that fit
#pragma unroll
      for (uint32_t e = 0; e < E; e++)
        for (uint32_t q = 0; q < ln[t][e]; q++)
          if (o[e] + q < cap) gst(dst + o[e] + q, (uint8_t)(ld32(brs, (sr[t][e] + q) & ~3u) >> (((sr[t][e] + q) & 3u) * 8u)));
    }
  }
  (void)err;
  (void)err_count;
}

// ---------------------------------------------------------------------------
// Launcher (host side of this translation unit): see pqgpu_internal.h

hipError_t launch_dd_strings(hipStream_t st, const uint8_t* bytes, uint64_t n_bytes, PageWork* work,
                             const ColumnDev* cols, const uint64_t* chunks, uint32_t n_chunks, const uint64_t* pstat,
                             uint64_t* err, ErrCount err_count, uint64_t* sums, const int32_t* dd_cols,
                             const int32_t* dd_start, int n_dd_cols, uint32_t dd_region, bool global,
                             hipEvent_t entries_ready) {
  const uint32_t n_tile = (n_chunks + WPB - 1) / WPB;
  const dim3 blk(64 * WPB);
  hipError_t e;
  // (the entries, walked on another queue: the ids never read them)
  if (entries_ready && hipStreamWaitEvent(st, entries_ready, 0) != hipSuccess) return hipErrorUnknown;
  if (global && n_tile) {  // the chunks' byte sums from the stored ids (entry lengths gathered from HBM)
    hipLaunchKernelGGL(k_dd_gsums, dim3(n_tile), blk, 0, st, work, cols, chunks, n_chunks, pstat, sums);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k_dd_bases, dim3(n_dd_cols), dim3(256), 0, st, work, cols, chunks, dd_cols, dd_start, sums);
  e = hipGetLastError();
  if (e != hipSuccess || !n_tile) return e;
  if (global) {  // a workgroup per chunk
    hipLaunchKernelGGL(k_dd_gstr, dim3(n_chunks), blk, 0, st, bytes, n_bytes, work, cols, chunks, n_chunks, pstat, sums,
                       err, err_count);
    return hipGetLastError();
  }
  const uint32_t dd_lds_bytes = 16u + ((dd_region + 15u) & ~15u) + WPB * DDG_WAVE_BYTES;
  if (n_chunks <= DD_SPLIT_MAX_CHUNKS)  // few chunks: a workgroup per chunk
    hipLaunchKernelGGL(k_dd_str<CH_TILES / WPB>, dim3(n_chunks), blk, dd_lds_bytes, st, bytes, n_bytes, work, cols, chunks,
                       n_chunks, pstat, sums, err, err_count, dd_region);
  else
    hipLaunchKernelGGL(k_dd_str<CH_TILES>, dim3(n_tile), blk, dd_lds_bytes, st, bytes, n_bytes, work, cols, chunks, n_chunks,
                       pstat, sums, err, err_count, dd_region);
  return hipGetLastError();
}

#ifdef PQG_DIAG
int diag_nostore_dict_strings(int v) {
  return hipMemcpyToSymbol(HIP_SYMBOL(pqg_diag_nostore), &v, sizeof(v)) == hipSuccess ? 0 : 3;
}
#endif

}  // namespace pqg
