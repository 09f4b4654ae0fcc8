// pqgpu_crc.hip — pqg_crc32_pages on the device (include/pqgpu.h, "page checksums"; the algebra and
// the tables: pqgpu_crc.h). Two launches, neither of which waits on another workgroup; no atomics.
//
// k_crc_tiles: one wave per (job, tile). The wave reads its tile in rows of CRC_ROW bytes, 16 per lane,
// from the 16-byte boundary at or below the tile's first byte (bytes before the first and after the
// last are masked to zero; loads are range-checked against n_bytes rounded up to 4). A lane keeps four
// states, one per dword of its 16 bytes, so every state sees one dword per row and one table serves
// all of them: s = (s ^ d) * x^(8 * CRC_ROW), four lookups in `row` that do not depend on each other
// across the four states. After the last row the four states sit 4 bytes apart (three steps through
// `step4` join them), the lanes' joined states 16 bytes apart: each lane moves its own to the tile's
// nominal end, start + T, with one constant of `xp8` and a bit-serial multiplication, and the wave XORs.
// k_crc_fold: one wave per job. Lane j runs Horner's rule over the partials of tiles j, j + 64, ...
// (x^(8 * 64 T) between them), moves its sum by the tiles that follow its last one, the wave XORs, and
// lane 0 moves the result from the last tile's nominal end back to the job's end and inverts it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pqgpu_crc.h"
#include "pqgpu_device.h"

namespace pqg {

namespace {

__device__ __forceinline__ uint32_t crc_mul(uint32_t a, uint32_t b) {  // a * b mod P, branch-free
  uint32_t p = 0;
#pragma unroll
  for (int i = 0; i < 32; i++) {
    p ^= b & (0u - (a >> 31));
    a <<= 1;
    b = (b >> 1) ^ (CRC_POLY & (0u - (b & 1u)));
  }
  return p;
}

__device__ __forceinline__ uint32_t crc_lookup4(const uint32_t* t, uint32_t v) {
  return t[v & 0xFFu] ^ t[256u + ((v >> 8) & 0xFFu)] ^ t[512u + ((v >> 16) & 0xFFu)] ^ t[768u + (v >> 24)];
}

// The bytes lo <= j < hi of a dword as a mask (j counts from the dword's lowest address).
__device__ __forceinline__ uint32_t crc_bytes(int32_t lo, int32_t hi) {
  lo = lo < 0 ? 0 : lo;
  hi = hi > 4 ? 4 : hi;
  if (hi <= lo) return 0u;
  return (0xFFFFFFFFu >> (8 * (4 - hi))) & (0xFFFFFFFFu << (8 * lo));
}

__device__ __forceinline__ uint32_t wave_xor(uint32_t v) {
#pragma unroll
  for (int m = 32; m; m >>= 1) v ^= (uint32_t)__shfl_xor((int)v, m, WAVE);
  return v;
}

}  // namespace

__global__ __launch_bounds__(WAVE* WPB) void k_crc_tiles(const uint8_t* __restrict__ bytes, uint64_t n_bytes4,
                                                         const CrcTile* __restrict__ tiles, uint32_t n_tiles,
                                                         const uint32_t* __restrict__ tab, uint32_t T,
                                                         uint32_t* __restrict__ partial) {
  __shared__ uint32_t lds[2048];  // step4, row
  for (uint32_t i = threadIdx.x; i < 2048u; i += WAVE * WPB) lds[i] = tab[i];
  __syncthreads();
  const uint32_t* step4 = lds + CRC_TAB_STEP4;
  const uint32_t* row = lds + CRC_TAB_ROW;
  const uint32_t* xp8 = tab + CRC_TAB_XP8;
  const uint32_t lane = lane_id();
  for (uint32_t ti = blockIdx.x * WPB + wave_id(); ti < n_tiles; ti += gridDim.x * WPB) {
    const CrcTile t = tiles[ti];
    const uint64_t start = uni64(t.start);
    const uint32_t size = uni(t.size), first = uni(t.flags) & CRC_TILE_FIRST;
    // the rows start at the 16-byte boundary at or below the first byte, but not before `bytes`
    const uint64_t pa = (uint64_t)(uintptr_t)bytes + start;
    uint64_t base = pa & ~15ull;
    if (base < (uint64_t)(uintptr_t)bytes) base = (uint64_t)(uintptr_t)bytes;
    const uint32_t lead = (uint32_t)(pa - base);                 // 0..15
    const uint32_t span = lead + size;                           // valid bytes are [lead, span) of the rows
    const uint32_t n_rows = (span + CRC_ROW - 1) / CRC_ROW;
    const uint64_t left = n_bytes4 - (base - (uint64_t)(uintptr_t)bytes);
    const uint32_t n_rec = left < (uint64_t)n_rows * CRC_ROW ? (uint32_t)left : n_rows * CRC_ROW;
    const rsrc_t rs = make_rsrc((const uint8_t*)(uintptr_t)base, n_rec);
    uint32_t s0 = 0, s1 = 0, s2 = 0, s3 = 0;
    for (uint32_t r = 0; r < n_rows; r++) {
      const uint32_t o = r * CRC_ROW + 16u * lane;
      u32x4 d = o + 16u <= n_rec ? __builtin_amdgcn_raw_buffer_load_b128(rs, (int)o, 0, 0)
                                 : u32x4{ld32(rs, o), ld32(rs, o + 4), ld32(rs, o + 8), ld32(rs, o + 12)};
      if (o < lead || o + 16u > span) {  // the tile's first and last bytes
        const int32_t lo = (int32_t)lead - (int32_t)o, hi = (int32_t)span - (int32_t)o;
        d.x &= crc_bytes(lo, hi);
        d.y &= crc_bytes(lo - 4, hi - 4);
        d.z &= crc_bytes(lo - 8, hi - 8);
        d.w &= crc_bytes(lo - 12, hi - 12);
      }
      if (first && r == 0 && lane < 2) {  // the start value: 0xFF on the job's first four byte positions
        const int32_t lo = (int32_t)lead - (int32_t)o;
        d.x ^= crc_bytes(lo, lo + 4);
        d.y ^= crc_bytes(lo - 4, lo);
        d.z ^= crc_bytes(lo - 8, lo - 4);
        d.w ^= crc_bytes(lo - 12, lo - 8);
      }
      s0 = crc_lookup4(row, s0 ^ d.x);
      s1 = crc_lookup4(row, s1 ^ d.y);
      s2 = crc_lookup4(row, s2 ^ d.z);
      s3 = crc_lookup4(row, s3 ^ d.w);
    }
    // the four states are 4 bytes apart: join them at the last one's position, 12 bytes into the lane's
    // 16 of the row after the last
    uint32_t c = crc_lookup4(step4, s0) ^ s1;
    c = crc_lookup4(step4, c) ^ s2;
    c = crc_lookup4(step4, c) ^ s3;
    // ... and move to the nominal end, start + T: by lead + T - n_rows * CRC_ROW - 16 lane - 12 bytes,
    // in [-2044, T - 1021]
    const int32_t mv = (int32_t)(lead + T) - (int32_t)(n_rows * CRC_ROW) - (int32_t)(16u * lane) - 12;
    c = wave_xor(crc_mul(c, xp8[(uint32_t)(mv + (int32_t)T)]));
    if (lane == 0) partial[ti] = c;
  }
}

__global__ __launch_bounds__(WAVE* WPB) void k_crc_fold(const CrcJobDev* __restrict__ jobs, uint32_t n_jobs,
                                                        const uint32_t* __restrict__ partial,
                                                        const uint32_t* __restrict__ tab, uint32_t T,
                                                        uint32_t* __restrict__ crc, int32_t* __restrict__ status) {
  const uint32_t j = blockIdx.x * WPB + wave_id();
  if (j >= n_jobs) return;
  const uint32_t* xp8 = tab + CRC_TAB_XP8;
  const uint32_t* xt = tab + CRC_TAB_XP8 + 2u * T;
  const uint32_t lane = lane_id();
  const CrcJobDev J = jobs[j];
  const uint32_t nt = uni(J.n_tiles), size = uni(J.size);
  const uint64_t tb = uni64(J.tile_begin);
  uint32_t v = 0;
  if (nt) {
    const uint32_t x64 = xt[CRC_FOLD_LANES];
    uint32_t acc = 0, last = lane;
    for (uint32_t t = lane; t < nt; t += CRC_FOLD_LANES) {
      acc = (t == lane ? 0u : crc_mul(acc, x64)) ^ partial[tb + t];
      last = t;
    }
    if (lane < nt) acc = crc_mul(acc, xt[nt - 1u - last]);  // nt - 1 - last < 64
    acc = wave_xor(acc);
    // from the last tile's nominal end back to the job's end: size - nt * T bytes, in (-T, 0]
    const int32_t rem = (int32_t)((int64_t)size - (int64_t)nt * (int64_t)T);
    v = ~crc_mul(acc, xp8[(uint32_t)(rem + (int32_t)T)]);
  }
  if (lane == 0) {
    if (crc) crc[j] = v;
    status[j] = ((uni(J.flags) & PQG_CRC_VERIFY) && v != uni(J.expected)) ? PQG_ERR_CRC : PQG_OK;
  }
}

hipError_t launch_crc(hipStream_t st, const uint8_t* bytes, uint64_t n_bytes, const CrcTile* tiles, uint32_t n_tiles,
                      const CrcJobDev* jobs, uint32_t n_jobs, const uint32_t* tab, uint32_t tile_bytes,
                      uint32_t* partial, uint32_t* crc, int32_t* status) {
  if (n_tiles) {
    // several tiles per workgroup, so that the 8 KiB table fill is shared
    const uint32_t want = (n_tiles + WPB - 1) / WPB;
    const uint32_t grid = want < 4096u ? want : 4096u;
    hipLaunchKernelGGL(k_crc_tiles, dim3(grid), dim3(WAVE * WPB), 0, st, bytes, (n_bytes + 3) & ~3ull, tiles, n_tiles, tab,
                       tile_bytes, partial);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k_crc_fold, dim3((n_jobs + WPB - 1) / WPB), dim3(WAVE * WPB), 0, st, jobs, n_jobs, partial, tab,
                     tile_bytes, crc, status);
  return hipGetLastError();
}

}  // namespace pqg
