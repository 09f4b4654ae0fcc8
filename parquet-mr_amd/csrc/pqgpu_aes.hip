// pqgpu_aes.hip — pqg_decrypt_pages on the device (include/pqgpu.h, "encrypted pages"; the algebra and
// the tables: pqgpu_aes.h). Two launches, neither of which waits on another workgroup; no atomics.
//
// k_aes_tiles: one wave per (job, tile). The wave takes its tile in rows of AES_ROW bytes, one 16-byte
// block per lane: the lane loads its block's ciphertext (aligned dwords from the 4-byte boundary at or
// below the tile's first byte, range-checked against n_src rounded up to 4, shifted into place with
// v_alignbyte), encrypts nonce || counter with the key's schedule (te0 in LDS, 1 KiB per workgroup, filled
// once for all the tiles the workgroup takes), and XORs. Stores go out as 16-byte blocks of d_dst that
// start at the 4-byte boundary at or below the tile's first plaintext byte (4-byte, not 16-byte aligned):
// when the destination is not 4-byte aligned a lane takes the last bytes of its lower neighbour's block
// (the previous row's lane 63 for lane 0), so every lane still writes four whole dwords, consecutive lanes
// consecutive ones; only a destination that is 16-byte aligned (every codec source payload, every page of
// a batch) gets one 16-byte store per lane. The blocks at the tile's two ends are clipped to its byte
// range with byte stores, which is what keeps neighbouring tiles and jobs apart. GCM: the lane also runs Horner's rule over its blocks, which are 64 apart, with the
// key's 4-bit table of H^64 (8 KiB of LDS per wave, filled only by tiles of more than one row); after the
// last row a bit-serial product by H^(blocks after the lane's last one, 1..64) moves its sum to the tile's
// end and the wave XORs: the tile's partial.
// k_aes_fold: one wave per job. The AAD blocks go through Horner's rule with H; that value and the
// partials of all tiles but the last are items B blocks apart, which lane j sums for the items j, j + 64,
// ... (H^(64 B) between them) and moves by the items that follow its last one; the wave XORs, the result
// moves over the last tile's blocks and takes its partial, then the length block and one more H. Compared
// with E_K(nonce || 1) ^ tag.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pqgpu_aes.h"
#include "pqgpu_device.h"

namespace pqg {

namespace {

__device__ __forceinline__ uint32_t ror32(uint32_t v, uint32_t n) { return __builtin_amdgcn_alignbit(v, v, n); }

// FIPS-197 Cipher(): state and round keys as big-endian words; rk is wave-uniform.
__device__ __forceinline__ void aes_encrypt(const uint32_t* te, const uint32_t* __restrict__ rk, uint32_t rounds,
                                            uint32_t (&s)[4]) {
  uint32_t s0 = s[0] ^ rk[0], s1 = s[1] ^ rk[1], s2 = s[2] ^ rk[2], s3 = s[3] ^ rk[3];
  for (uint32_t r = 1; r < rounds; r++) {
    const uint32_t* k = rk + 4u * r;
    const uint32_t t0 = te[s0 >> 24] ^ ror32(te[(s1 >> 16) & 255u], 8) ^ ror32(te[(s2 >> 8) & 255u], 16) ^ ror32(te[s3 & 255u], 24) ^ k[0];
    const uint32_t t1 = te[s1 >> 24] ^ ror32(te[(s2 >> 16) & 255u], 8) ^ ror32(te[(s3 >> 8) & 255u], 16) ^ ror32(te[s0 & 255u], 24) ^ k[1];
    const uint32_t t2 = te[s2 >> 24] ^ ror32(te[(s3 >> 16) & 255u], 8) ^ ror32(te[(s0 >> 8) & 255u], 16) ^ ror32(te[s1 & 255u], 24) ^ k[2];
    const uint32_t t3 = te[s3 >> 24] ^ ror32(te[(s0 >> 16) & 255u], 8) ^ ror32(te[(s1 >> 8) & 255u], 16) ^ ror32(te[s2 & 255u], 24) ^ k[3];
    s0 = t0; s1 = t1; s2 = t2; s3 = t3;
  }
  // the last round has no MixColumns: S[x] is the second byte of te0[x]
  const uint32_t* k = rk + 4u * rounds;
#define PQG_SB(v) ((te[(v)] >> 8) & 255u)
  s[0] = (PQG_SB(s0 >> 24) << 24 | PQG_SB((s1 >> 16) & 255u) << 16 | PQG_SB((s2 >> 8) & 255u) << 8 | PQG_SB(s3 & 255u)) ^ k[0];
  s[1] = (PQG_SB(s1 >> 24) << 24 | PQG_SB((s2 >> 16) & 255u) << 16 | PQG_SB((s3 >> 8) & 255u) << 8 | PQG_SB(s0 & 255u)) ^ k[1];
  s[2] = (PQG_SB(s2 >> 24) << 24 | PQG_SB((s3 >> 16) & 255u) << 16 | PQG_SB((s0 >> 8) & 255u) << 8 | PQG_SB(s1 & 255u)) ^ k[2];
  s[3] = (PQG_SB(s3 >> 24) << 24 | PQG_SB((s0 >> 16) & 255u) << 16 | PQG_SB((s1 >> 8) & 255u) << 8 | PQG_SB(s2 & 255u)) ^ k[3];
#undef PQG_SB
}

// x * y in GF(2^128), "words" form (SP 800-38D algorithm 1), branch-free.
__device__ __forceinline__ void gf_mul_words(const uint32_t (&x)[4], const uint32_t (&y)[4], uint32_t (&z)[4]) {
  uint32_t z0 = 0, z1 = 0, z2 = 0, z3 = 0, v0 = y[0], v1 = y[1], v2 = y[2], v3 = y[3];
#pragma unroll
  for (int w = 0; w < 4; w++) {
    uint32_t xw = x[w];
#pragma unroll 4
    for (int b = 0; b < 32; b++) {
      const uint32_t m = 0u - (xw >> 31);
      xw <<= 1;
      z0 ^= v0 & m; z1 ^= v1 & m; z2 ^= v2 & m; z3 ^= v3 & m;
      const uint32_t red = 0xE1000000u & (0u - (v3 & 1u));
      v3 = __builtin_amdgcn_alignbit(v2, v3, 1);
      v2 = __builtin_amdgcn_alignbit(v1, v2, 1);
      v1 = __builtin_amdgcn_alignbit(v0, v1, 1);
      v0 = (v0 >> 1) ^ red;
    }
  }
  z[0] = z0; z[1] = z1; z[2] = z2; z[3] = z3;
}

__device__ __forceinline__ void ld_words(const uint32_t* __restrict__ p, uint32_t (&o)[4]) {
  const u32x4 v = *(const u32x4*)p;
  o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
}

// y * H^64, "bytes" form: the XOR of the 32 table entries of y's nibbles.
__device__ __forceinline__ u32x4 gf_mul_h64(const u32x4* tab, const u32x4 y) {
  u32x4 z = {0, 0, 0, 0};
  const uint32_t w[4] = {y.x, y.y, y.z, y.w};
#pragma unroll
  for (uint32_t q = 0; q < 4; q++)
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) {
      const uint32_t b = (w[q] >> (8u * k)) & 255u;
      const uint32_t pos = 2u * (4u * q + k);
      z ^= tab[16u * pos + (b >> 4)];
      z ^= tab[16u * (pos + 1u) + (b & 15u)];
    }
  return z;
}

__device__ __forceinline__ uint32_t wave_xor32(uint32_t v) {
#pragma unroll
  for (int m = 32; m; m >>= 1) v ^= (uint32_t)__shfl_xor((int)v, m, WAVE);
  return v;
}

// The dwords' bytes j < n (j counts from the dword's lowest address), n may be <= 0 or >= 4.
__device__ __forceinline__ uint32_t low_bytes(int32_t n) {
  return n <= 0 ? 0u : n >= 4 ? 0xFFFFFFFFu : (0xFFFFFFFFu >> (8 * (4 - n)));
}

// 16 bytes at byte `pos` (wave-uniform, any alignment) of src as four little-endian dwords: aligned loads,
// range-checked against n4 = the readable size rounded up to 4.
__device__ __forceinline__ void ld16_any(const uint8_t* __restrict__ src, uint64_t n4, uint64_t pos, uint32_t (&o)[4]) {
  const uint64_t base = pos & ~3ull;
  const uint32_t sb = (uint32_t)(pos & 3u);
  const uint64_t left = n4 - base;
  const rsrc_t rs = make_rsrc(src + base, left < 32u ? left : 32u);
  uint32_t w[5];
#pragma unroll
  for (uint32_t k = 0; k < 5; k++) w[k] = ld32(rs, 4u * k);
#pragma unroll
  for (uint32_t k = 0; k < 4; k++) o[k] = __builtin_amdgcn_alignbyte(w[k + 1], w[k], sb);
}

}  // namespace

__global__ __launch_bounds__(WAVE* WPB) void k_aes_tiles(const uint8_t* __restrict__ src, uint64_t n_src4,
                                                         uint8_t* __restrict__ dst, const AesTile* __restrict__ tiles,
                                                         uint32_t n_tiles, const AesJobDev* __restrict__ jobs,
                                                         const uint32_t* __restrict__ te0,
                                                         const uint32_t* __restrict__ keys, uint32_t key_words,
                                                         u32x4* __restrict__ partial) {
  __shared__ uint32_t te[256];
  __shared__ u32x4 h64_all[WPB][512];
  for (uint32_t i = threadIdx.x; i < 256u; i += WAVE * WPB) te[i] = te0[i];
  __syncthreads();
  const uint32_t lane = lane_id();
  u32x4* h64 = h64_all[wave_id()];
  for (uint32_t ti = blockIdx.x * WPB + wave_id(); ti < n_tiles; ti += gridDim.x * WPB) {
    const AesTile t = tiles[ti];
    const uint64_t t_src = uni64(t.src), t_dst = uni64(t.dst);
    const uint32_t size = uni(t.size), block0 = uni(t.block0);
    const AesJobDev* J = jobs + uni(t.job);
    const bool gcm = uni(J->mode) == (uint32_t)PQG_DECRYPT_GCM;
    const uint32_t* kw = keys + (uint64_t)uni(J->key) * key_words;
    const uint32_t rounds = uni(kw[AES_KEY_ROUNDS]);
    const uint32_t ctr0 = uni(J->ctr0) + block0;
    uint32_t nonce[4];
    ld16_any(src, n_src4, uni64(J->nonce_src), nonce);
    const uint32_t n0 = __builtin_bswap32(nonce[0]), n1 = __builtin_bswap32(nonce[1]), n2 = __builtin_bswap32(nonce[2]);
    const uint32_t nb = (size + 15u) / 16u;                     // blocks of the tile
    const uint32_t n_rows = (nb + AES_ROW_BLOCKS - 1) / AES_ROW_BLOCKS;
    if (gcm && n_rows > 1) {
      wave_sync();  // the previous tile's reads of the table
      const u32x4* g = (const u32x4*)(kw + AES_KEY_H64);
#pragma unroll
      for (uint32_t i = 0; i < 8; i++) h64[64u * i + lane] = g[64u * i + lane];
      wave_sync();
    }
    // loads: rows of aligned dwords from the 4-byte boundary at or below the first byte
    const uint64_t base = t_src & ~3ull;
    const uint32_t lead = (uint32_t)(t_src - base);             // 0..3
    const uint64_t left = n_src4 - base;
    const uint64_t want = (uint64_t)n_rows * AES_ROW + 16u;
    const uint32_t n_rec = (uint32_t)(left < want ? left : want);
    const rsrc_t rs = make_rsrc(src + base, n_rec);
    // stores: 16-byte blocks from the 4-byte boundary at or below the first plaintext byte
    const uint32_t s = (uint32_t)(t_dst & 3u);
    const uint64_t a0 = t_dst - s, o_hi = t_dst + size;
    const uint32_t nab = (s + size + 15u) / 16u;
    const uint32_t n_rows_out = (nab + AES_ROW_BLOCKS - 1) / AES_ROW_BLOCKS;
    u32x4 y = {0, 0, 0, 0};
    uint32_t carry = 0;  // the previous row's last plaintext dword
    for (uint32_t r = 0; r < n_rows_out; r++) {
      const uint32_t i = r * AES_ROW_BLOCKS + lane;
      uint32_t pt[4] = {0, 0, 0, 0};
      if (i < nb) {
        const uint32_t o = 16u * i;
        uint32_t w[5];
        if (o + 16u <= n_rec) {
          const u32x4 d = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)o, 0, 0);
          w[0] = d.x; w[1] = d.y; w[2] = d.z; w[3] = d.w;
        } else {
          w[0] = ld32(rs, o); w[1] = ld32(rs, o + 4); w[2] = ld32(rs, o + 8); w[3] = ld32(rs, o + 12);
        }
        w[4] = ld32(rs, o + 16u);
        uint32_t c[4];
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) c[k] = __builtin_amdgcn_alignbyte(w[k + 1], w[k], lead);
        const int32_t nbytes = (int32_t)(size - o);             // of this block: the last one may be short
        if (nbytes < 16) {
#pragma unroll
          for (int k = 0; k < 4; k++) c[k] &= low_bytes(nbytes - 4 * k);
        }
        uint32_t ks[4] = {n0, n1, n2, ctr0 + i};
        aes_encrypt(te, kw + AES_KEY_RK, rounds, ks);
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) pt[k] = c[k] ^ __builtin_bswap32(ks[k]);
        if (gcm) {
          if (r) y = gf_mul_h64(h64, y);
          y ^= u32x4{c[0], c[1], c[2], c[3]};
        }
      }
      // (all lanes) the lower neighbour's last dword
      uint32_t prev = (uint32_t)__shfl_up((int)pt[3], 1, WAVE);
      if (lane == 0) prev = carry;
      carry = rdl(pt[3], 63);
      if (i < nab) {
        uint32_t wd[4];
        if (s) {
          wd[0] = __builtin_amdgcn_alignbyte(pt[0], prev, 4u - s);
          wd[1] = __builtin_amdgcn_alignbyte(pt[1], pt[0], 4u - s);
          wd[2] = __builtin_amdgcn_alignbyte(pt[2], pt[1], 4u - s);
          wd[3] = __builtin_amdgcn_alignbyte(pt[3], pt[2], 4u - s);
        } else {
          wd[0] = pt[0]; wd[1] = pt[1]; wd[2] = pt[2]; wd[3] = pt[3];
        }
        const uint64_t a = a0 + 16ull * i;
        uint32_t have = 0;
#pragma unroll
        for (uint32_t q = 0; q < 4; q++)
          if (a + 4u * q >= t_dst && a + 4u * q + 4u <= o_hi) have |= 1u << q;
        store_block16(dst, a, t_dst, o_hi, wd, have, (((uint64_t)(uintptr_t)dst + a) & 15u) == 0);
      }
    }
    if (gcm) {
      // the lane's sum ends at its last block: move it to the tile's end, 1..64 blocks on
      uint32_t m[4] = {0, 0, 0, 0};
      if (lane < nb) {
        const uint32_t last = lane + AES_ROW_BLOCKS * ((nb - 1u - lane) / AES_ROW_BLOCKS);
        const uint32_t yw[4] = {__builtin_bswap32(y.x), __builtin_bswap32(y.y), __builtin_bswap32(y.z), __builtin_bswap32(y.w)};
        uint32_t p[4];
        ld_words(kw + AES_KEY_PW + 4u * (nb - last), p);
        gf_mul_words(yw, p, m);
      }
#pragma unroll
      for (int k = 0; k < 4; k++) m[k] = wave_xor32(m[k]);
      if (lane == 0) gst(partial + ti, u32x4{m[0], m[1], m[2], m[3]});
    }
  }
}

__global__ __launch_bounds__(WAVE* WPB) void k_aes_fold(const uint8_t* __restrict__ src, uint64_t n_src4,
                                                        const AesJobDev* __restrict__ jobs, uint32_t n_jobs,
                                                        const u32x4* __restrict__ partial,
                                                        const uint8_t* __restrict__ aad, const uint32_t* __restrict__ te0,
                                                        const uint32_t* __restrict__ keys, uint32_t key_words, uint32_t T,
                                                        int32_t* __restrict__ status) {
  __shared__ uint32_t te[256];
  for (uint32_t i = threadIdx.x; i < 256u; i += WAVE * WPB) te[i] = te0[i];
  __syncthreads();
  const uint32_t j = blockIdx.x * WPB + wave_id();
  if (j >= n_jobs) return;
  const uint32_t lane = lane_id();
  const AesJobDev* J = jobs + j;
  if (uni(J->mode) != (uint32_t)PQG_DECRYPT_GCM) {
    if (lane == 0) status[j] = PQG_OK;
    return;
  }
  const uint32_t* kw = keys + (uint64_t)uni(J->key) * key_words;
  const uint32_t* pw = kw + AES_KEY_PW;
  const uint32_t* xt = pw + 4u * (T / 16u + 1u);
  const uint32_t nt = uni(J->n_tiles), ct = uni(J->ct_size), n_aad = uni(J->aad_blocks), aad_len = uni(J->aad_length);
  const uint64_t tb = uni64(J->tile_begin);
  uint32_t H[4];
  ld_words(pw + 4, H);
  // the AAD blocks (zero-padded by the host), Horner with H: wave-uniform
  uint32_t ya[4] = {0, 0, 0, 0};
  const u32x4* ab = (const u32x4*)aad + uni(J->aad_block0);
  for (uint32_t b = 0; b < n_aad; b++) {
    const u32x4 v = ab[b];
    const uint32_t x[4] = {ya[0] ^ __builtin_bswap32(v.x), ya[1] ^ __builtin_bswap32(v.y), ya[2] ^ __builtin_bswap32(v.z),
                           ya[3] ^ __builtin_bswap32(v.w)};
    gf_mul_words(x, H, ya);
  }
  // items 0 .. nt - 1 (the AAD value, then the partials of the tiles 0 .. nt - 2), B blocks apart
  uint32_t acc[4] = {0, 0, 0, 0};
  if (lane < nt) {
    uint32_t x64[4];
    ld_words(xt + 4u * AES_FOLD_LANES, x64);
    uint32_t last = lane;
    for (uint32_t u = lane; u < nt; u += AES_FOLD_LANES) {
      if (u != lane) {
        const uint32_t a[4] = {acc[0], acc[1], acc[2], acc[3]};
        gf_mul_words(a, x64, acc);
      }
      if (u == 0) {
#pragma unroll
        for (int k = 0; k < 4; k++) acc[k] ^= ya[k];
      } else {
        const u32x4 p = partial[tb + u - 1u];
        acc[0] ^= p.x; acc[1] ^= p.y; acc[2] ^= p.z; acc[3] ^= p.w;
      }
      last = u;
    }
    uint32_t mv[4];
    ld_words(xt + 4u * (nt - 1u - last), mv);  // nt - 1 - last < 64
    const uint32_t a[4] = {acc[0], acc[1], acc[2], acc[3]};
    gf_mul_words(a, mv, acc);
  }
#pragma unroll
  for (int k = 0; k < 4; k++) acc[k] = wave_xor32(acc[k]);
  // over the last tile's blocks, its partial, the length block, one more H
  const uint32_t rem = (ct + 15u) / 16u - (nt - 1u) * (T / 16u);  // 1 .. T / 16
  uint32_t pr[4], sum[4];
  ld_words(pw + 4u * rem, pr);
  gf_mul_words(acc, pr, sum);
  const u32x4 pl = partial[tb + nt - 1u];
  const uint64_t abits = 8ull * aad_len, cbits = 8ull * ct;
  const uint32_t x[4] = {sum[0] ^ pl.x ^ (uint32_t)(abits >> 32), sum[1] ^ pl.y ^ (uint32_t)abits,
                         sum[2] ^ pl.z ^ (uint32_t)(cbits >> 32), sum[3] ^ pl.w ^ (uint32_t)cbits};
  gf_mul_words(x, H, sum);
  // E_K(J0) ^ tag
  uint32_t nonce[4], tag[4];
  ld16_any(src, n_src4, uni64(J->nonce_src), nonce);
  ld16_any(src, n_src4, uni64(J->tag_src), tag);
  uint32_t ek[4] = {__builtin_bswap32(nonce[0]), __builtin_bswap32(nonce[1]), __builtin_bswap32(nonce[2]), 1u};
  aes_encrypt(te, kw + AES_KEY_RK, uni(kw[AES_KEY_ROUNDS]), ek);
  uint32_t diff = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) diff |= sum[k] ^ ek[k] ^ __builtin_bswap32(tag[k]);
  if (lane == 0) status[j] = diff ? PQG_ERR_TAG : PQG_OK;
}

// pqg_copy_ranges: one wave per range, a byte per lane and step (the ranges are the level sections of V2 pages:
// tens of bytes at any alignment on both sides).
__global__ __launch_bounds__(WAVE* WPB) void k_copy_ranges(const uint8_t* __restrict__ src, uint64_t n_src,
                                                           uint8_t* __restrict__ dst, uint64_t n_dst,
                                                           const pqg_copy_range* __restrict__ ranges, uint32_t n) {
  const uint32_t j = blockIdx.x * WPB + wave_id();
  if (j >= n) return;
  const uint64_t so = uni64(ranges[j].src_offset), d0 = uni64(ranges[j].dst_offset);
  const uint32_t size = uni(ranges[j].size);
  if (uni(ranges[j].reserved) || so > n_src || size > n_src - so || d0 > n_dst || size > n_dst - d0) return;
  for (uint32_t i = lane_id(); i < size; i += WAVE) gst(dst + d0 + i, src[so + i]);
}

hipError_t launch_copy_ranges(hipStream_t st, const uint8_t* src, uint64_t n_src, uint8_t* dst, uint64_t n_dst,
                              const pqg_copy_range* ranges, uint32_t n) {
  hipLaunchKernelGGL(k_copy_ranges, dim3((n + WPB - 1) / WPB), dim3(WAVE * WPB), 0, st, src, n_src, dst, n_dst, ranges, n);
  return hipGetLastError();
}

hipError_t launch_decrypt(hipStream_t st, const uint8_t* src, uint64_t n_src, uint8_t* dst, const AesTile* tiles,
                          uint32_t n_tiles, const AesJobDev* jobs, uint32_t n_jobs, const uint8_t* aad,
                          const uint32_t* te0, const uint32_t* keys, uint32_t tile_bytes, void* partial,
                          int32_t* status) {
  const uint64_t n_src4 = (n_src + 3) & ~3ull;
  const uint32_t key_words = aes_key_words(tile_bytes);
  // several tiles per workgroup, so that the te0 fill is shared
  const uint32_t want = (n_tiles + WPB - 1) / WPB;
  const uint32_t grid = want < 8192u ? want : 8192u;
  hipLaunchKernelGGL(k_aes_tiles, dim3(grid), dim3(WAVE * WPB), 0, st, src, n_src4, dst, tiles, n_tiles, jobs, te0, keys,
                     key_words, (u32x4*)partial);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_aes_fold, dim3((n_jobs + WPB - 1) / WPB), dim3(WAVE * WPB), 0, st, src, n_src4, jobs, n_jobs,
                     (const u32x4*)partial, aad, te0, keys, key_words, tile_bytes, status);
  return hipGetLastError();
}

}  // namespace pqg
