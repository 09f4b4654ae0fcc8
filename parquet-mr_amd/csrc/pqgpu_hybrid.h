// pqgpu_hybrid.h — the RLE / bit-packed hybrid window helpers shared by the dictionary walk
// (pqgpu_dict.hip) and the level walk (pqgpu_kernels.hip): the pre-decoded 256-byte window over an LDS
// page segment, the branch-free header parsers, the scalar slow path and the saturating wave scan.
// Semantics: RunLengthBitPackingHybridDecoder.readInt/readNext (rle/…Decoder.java:61-109), value for value.
#pragma once
#include "pqgpu_device.h"

namespace pqg {

// ---------------------------------------------------------------------------
// RLE / bit-packed hybrid walker (RunLengthBitPackingHybridDecoder.readNext :80-109).
//
// Parallel pre-decode: a 256-byte window [B, B + 256) is held one dword per
// lane (plus the next two dwords), and every lane decodes a run header at each
// of its 4 byte positions as if a run started there (varint, count, RLE value or
// packed data start, next header position). The serial part — following the
// chain of headers from the section start — is then 4 v_readlane per run.

struct PreWin {
  rsrc_t rs;
  // Optional LDS copy of page bytes [seg_lo, seg_lo + SEG_BYTES): windows inside it are read
  // from LDS. (A global load issued after this wave's stores waits for all of them: vmcnt
  // counts stores on CDNA, so the bytes are staged before the first store.)
  uint8_t* seg;
  uint32_t seg_lo;
  uint32_t B;          // uniform: window start (4-aligned, page-relative)
  uint32_t nxt[4];     // per lane, byte b: next header position (0xFFFFFFFF: overflow)
  uint32_t cnt[4];     // run count (values)
  uint32_t val[4];     // RLE: raw value; PACKED: data start
  uint32_t flg;        // byte b: bit0 packed, bit1 slow path, bits 2..4 header length
};

constexpr uint32_t SEG_BYTES = 3072;   // LDS page segment per wave of k_dict_runs (5 workgroups per CU)

// Fill the wave's LDS segment with page bytes [lo, lo + SEG_BYTES) (lo 16-aligned).
__device__ __forceinline__ void seg_fill(PreWin& pw, uint32_t lo) {
  pw.seg_lo = lo;
#pragma unroll
  for (uint32_t i = 0; i < SEG_BYTES; i += 16u * WAVE) {
    const uint32_t o = i + 16u * lane_id();
    if (o < SEG_BYTES) {
      const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(pw.rs, (int)(lo + o), 0, 0);
      *(u32x4*)(pw.seg + o) = v;
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// True when bytes [a, a + n) of the page are in the segment.
__device__ __forceinline__ bool seg_has(const PreWin& pw, uint32_t a, uint32_t n) {
  return pw.seg && a >= pw.seg_lo && a + n <= pw.seg_lo + SEG_BYTES;
}

// LDS byte buffers are written as u32x4 and read as u32: may_alias keeps TBAA from
// reordering the two.
typedef uint32_t __attribute__((may_alias)) u32_alias;

__device__ __forceinline__ uint32_t seg32(const PreWin& pw, uint32_t a) {  // a 4-aligned, inside
  return *(const u32_alias*)(pw.seg + (a - pw.seg_lo));
}

// Headers of at most 4 bytes are parsed branch-free from the position's first dword; a 5-byte
// header (a count / group number of 2^27 or more) is marked slow and left to the scalar path, so
// an RLE value (<= 4 bytes) always lies inside the 8 bytes at the position. Stages [B, B + 264)
// in the segment when needed.
__device__ __forceinline__ void predecode(PreWin& pw, uint32_t B, int w) {
  pw.B = B;
  const uint32_t base = B + 4u * lane_id();
  if (pw.seg && !seg_has(pw, B, 264u)) seg_fill(pw, B & ~15u);
  uint32_t d0, d1, d2;
  if (pw.seg) {
    d0 = seg32(pw, base);
    d1 = seg32(pw, base + 4);
    d2 = seg32(pw, base + 8);
  } else {
    d0 = ld32(pw.rs, base);
    d1 = ld32(pw.rs, base + 4);
    d2 = ld32(pw.rs, base + 8);
  }
  const uint64_t lo = (uint64_t)d0 | ((uint64_t)d1 << 32);
  const uint32_t nb = ((uint32_t)w + 7u) >> 3;
  uint32_t flg = 0;
#pragma unroll
  for (uint32_t b = 0; b < 4; b++) {
    const uint32_t p = base + b;
    // bytes p .. p+7
    const uint64_t x = b ? ((lo >> (8 * b)) | ((uint64_t)d2 << (64 - 8 * b))) : lo;
    // readUnsignedVarInt, Java int semantics, up to 4 bytes here (longer: slow path). Open-coded: the
    // same parse through varint4 (below) costs k_levels and k_rle_bool a VGPR each.
    const uint32_t d = (uint32_t)x, stop = ~d & 0x80808080u;  // stop bit of each of 4 bytes
    uint32_t slow = stop == 0u;
    const uint32_t hl = stop ? ((uint32_t)__builtin_ctz(stop) >> 3) + 1u : 4u;
    const uint32_t dm = d & (0xFFFFFFFFu >> (32u - 8u * hl));
    const uint32_t v = (dm & 0x7Fu) | ((dm >> 1) & 0x3F80u) | ((dm >> 2) & 0x1FC000u) | ((dm >> 3) & 0xFE00000u);
    uint32_t nx, c, vv, pk;
    if ((v & 1u) == 0) {  // RLE: count, then ceil(w/8) little-endian bytes, not masked
      const uint64_t y = x >> (8u * hl);
      vv = nb == 4 ? (uint32_t)y : (uint32_t)y & ((1u << (8u * nb)) - 1u);
      c = v >> 1;
      nx = p + hl + nb;
      pk = 0;
    } else {              // PACKED: (header >>> 1) groups of 8 values, groups * w bytes
      const uint32_t groups = v >> 1;
      if (groups == 0 || groups >= (1u << 28)) slow = 1;
      c = groups * 8u;
      vv = p + hl;
      const uint64_t e = (uint64_t)p + hl + (uint64_t)groups * (uint32_t)w;
      nx = e > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)e;
      pk = 1;
    }
    pw.nxt[b] = nx;
    pw.cnt[b] = c;
    pw.val[b] = vv;
    flg |= (pk | (slow << 1) | (hl << 2)) << (8 * b);
  }
  pw.flg = flg;
}

// readUnsignedVarInt of a header of at most 4 bytes whose first dword is d: the header length
// (4 when no byte of d ends the varint: the caller treats that as slow) and the 7-bit groups
// compacted, branch-free.
__device__ __forceinline__ uint32_t varint4(uint32_t d, uint32_t& hl) {
  const uint32_t stop = ~d & 0x80808080u;  // stop bit of each of 4 bytes
  hl = ((uint32_t)__builtin_ctz(stop | 0x80000000u) >> 3) + 1u;
  const uint32_t dm = d & (0xFFFFFFFFu >> (32u - 8u * hl));
  return (dm & 0x7Fu) | ((dm >> 1) & 0x3F80u) | ((dm >> 2) & 0x1FC000u) | ((dm >> 3) & 0xFE00000u);
}

// Successor-only pre-decode of the window [B, B + 256) for the dictionary list walk: what the
// chain needs of a position is where the next header would be, nothing else. Lane l, byte b of
// js: window offset of the successor of position B + 4 l + b, 0 when the chain stops there (the
// successor leaves the window, the position is past the section end, or the header is one for the
// scalar path: a varint of 5 bytes or more, 0 groups, a header or RLE value crossing the section
// end). Bit b of slowm / inm: scalar-path header / position inside the section. Branch-free;
// counts and values are parsed later, only at the positions the chain visited (walk_header).
template <bool LDS_ONLY>
__device__ __forceinline__ void predecode_succ(PreWin& pw, uint32_t B, int w, uint32_t sec_end, uint32_t& js,
                                               uint32_t& slowm, uint32_t& inm) {
  pw.B = B;
  const uint32_t base = B + 4u * lane_id();
  if (!LDS_ONLY && !seg_has(pw, B, 264u)) seg_fill(pw, B & ~15u);
  const uint32_t d0 = seg32(pw, base), d1 = seg32(pw, base + 4);
  const uint32_t nb = ((uint32_t)w + 7u) >> 3;
  js = slowm = inm = 0;
#pragma unroll
  for (uint32_t b = 0; b < 4; b++) {
    const uint32_t p = base + b;
    const uint32_t d = b ? __builtin_amdgcn_alignbyte(d1, d0, b) : d0;  // bytes p .. p + 3
    uint32_t hl;
    const uint32_t v = varint4(d, hl);
    const uint32_t pk = d & 1u;
    const uint32_t groups = v >> 1;
    // 256 groups or more leave the window at any w > 0 (and add nothing at w = 0)
    const uint32_t adv = pk ? __umul24(groups < 256u ? groups : 256u, (uint32_t)w) : nb;
    const uint32_t nx = p + hl + adv;
    // (bitwise on 0 / 1 words: && and || would come out as exec-masked branches)
    const uint32_t in = p < sec_end;
    const uint32_t slow = in & ((uint32_t)((~d & 0x80808080u) == 0u) | (pk & (uint32_t)(groups == 0u)) |
                                (uint32_t)(p + hl > sec_end) | ((pk ^ 1u) & (uint32_t)(nx > sec_end)));
    const uint32_t nn = nx < sec_end ? nx : (pk ? sec_end : nx);  // packed: readFully of what is left
    const uint32_t j = (in & (slow ^ 1u) & (uint32_t)(nn - B < 256u)) ? nn - B : 0u;
    js |= j << (8u * b);
    slowm |= slow << b;
    inm |= in << b;
  }
}

// The header at window offset o of the pre-decoded window (a fast one: at most 4 bytes, inside
// the section), parsed by the lane that owns it in the batch: count (RLE 0 = "to the page end" is
// left to the caller), record payload (raw RLE value clamped to 2^31 - 1, or 0x80000000 | packed
// data start) and the next header position. Reads [B + o, B + o + 8) of the staged segment.
__device__ __forceinline__ void walk_header(const PreWin& pw, uint32_t o, int w, uint32_t sec_end, bool& pk,
                                            uint32_t& c, uint32_t& payload, uint32_t& nx) {
  const uint32_t p = pw.B + o, a = p & ~3u;
  const uint32_t d0 = seg32(pw, a), d1 = seg32(pw, a + 4), d2 = seg32(pw, a + 8);
  const uint32_t x0 = __builtin_amdgcn_alignbyte(d1, d0, p & 3u), x1 = __builtin_amdgcn_alignbyte(d2, d1, p & 3u);
  uint32_t hl;
  const uint32_t v = varint4(x0, hl);
  const uint32_t nb = ((uint32_t)w + 7u) >> 3;
  pk = x0 & 1u;
  if (pk) {  // (header >>> 1) groups of 8 values, groups * w bytes
    const uint32_t groups = v >> 1;  // < 2^27
    c = groups * 8u;
    payload = 0x80000000u | (p + hl);
    const uint64_t e = (uint64_t)p + hl + (uint64_t)groups * (uint32_t)w;
    nx = e < sec_end ? (uint32_t)e : sec_end;  // readFully of what is left
  } else {   // count, then ceil(w/8) little-endian bytes, not masked
    const uint32_t y = (uint32_t)((((uint64_t)x1 << 32) | x0) >> (8u * hl));
    const uint32_t vv = nb == 4 ? y : y & ((1u << (8u * nb)) - 1u);
    c = v >> 1;
    payload = vv > 0x7FFFFFFFu ? 0x7FFFFFFFu : vv;
    nx = p + hl + nb;
  }
}

// Scalar re-decode of one header at `pos` (rare: varints longer than 5 bytes,
// 0 or >= 2^28 groups). Bytes come through uniform buffer loads.
__device__ __forceinline__ uint32_t sbyte(rsrc_t rs, uint32_t p) {
  return uni((ld32(rs, p & ~3u) >> ((p & 3u) * 8u)) & 0xFFu);
}

template <class ByteAt>
__device__ int slow_header_g(ByteAt sbyte_at, uint32_t pos, uint32_t sec_end, int w, uint32_t& hl, uint32_t& m,
                             uint64_t& count, uint32_t& val, uint32_t& next) {
  uint32_t value = 0, i = 0, k = 0, bb;
  for (;;) {
    if (pos + k >= sec_end) return PQG_ERR_EOF;
    bb = sbyte_at(pos + k);
    if (!(bb & 0x80u)) break;
    value |= (bb & 0x7Fu) << (i & 31u);
    i += 7;
    k++;
  }
  const uint32_t header = value | (bb << (i & 31u));
  hl = k + 1;
  if ((header & 1u) == 0) {
    const uint32_t nb = ((uint32_t)w + 7u) >> 3;
    if ((uint64_t)pos + hl + nb > sec_end) return PQG_ERR_EOF;
    uint32_t v = 0;
    for (uint32_t j = 0; j < nb; j++) v |= sbyte_at(pos + hl + j) << (8u * j);
    m = 0;
    count = header >> 1;
    val = v;
    next = pos + hl + nb;
    return 0;
  }
  const uint32_t groups = header >> 1;
  if (groups == 0) return PQG_ERR_EMPTY_PACKED_RUN;
  if (groups >= (1u << 28)) return PQG_ERR_CORRUPT;
  m = 1;
  count = (uint64_t)groups * 8u;
  val = pos + hl;
  const uint64_t e = (uint64_t)pos + hl + (uint64_t)groups * (uint32_t)w;
  next = e > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)e;
  return 0;
}

__device__ __forceinline__ uint32_t wbyte(const PreWin& pw, uint32_t p) {
  if (seg_has(pw, p & ~3u, 4)) return uni((seg32(pw, p & ~3u) >> ((p & 3u) * 8u)) & 0xFFu);
  return sbyte(pw.rs, p);
}

__device__ __forceinline__ uint32_t pick4(const uint32_t (&a)[4], uint32_t b, uint32_t l) {
  switch (b) {
    case 0: return rdl(a[0], l);
    case 1: return rdl(a[1], l);
    case 2: return rdl(a[2], l);
    default: return rdl(a[3], l);
  }
}

// Saturating inclusive scan over the wave: lane l gets min(v_0 + ... + v_l, cap) (every v <= cap <
// 2^31). DPP row shifts and row broadcasts, no LDS round trip; call with all 64 lanes active.
__device__ __forceinline__ uint32_t wave_incl_scan_sat(uint32_t x, uint32_t cap) {
#define PQG_DPP_SAT(ctrl, rmask)                                                                \
  {                                                                                             \
    const uint32_t y_ = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, ctrl, rmask, 0xf, true); \
    x = x + y_ < cap ? x + y_ : cap;                                                            \
  }
  PQG_DPP_SAT(0x111, 0xf)  // row_shr:1
  PQG_DPP_SAT(0x112, 0xf)  // row_shr:2
  PQG_DPP_SAT(0x114, 0xf)  // row_shr:4
  PQG_DPP_SAT(0x118, 0xf)  // row_shr:8
  PQG_DPP_SAT(0x142, 0xa)  // row_bcast:15 -> rows 1, 3
  PQG_DPP_SAT(0x143, 0xc)  // row_bcast:31 -> rows 2, 3
#undef PQG_DPP_SAT
  return x;
}

}  // namespace pqg
