// pqgpu_plain.hip — CDNA4 (gfx950) kernels of PLAIN fixed-width and PLAIN BOOLEAN pages, and the
// ParquetReadRouter batch unpack of bit-packed runs. Byte copies and bit extraction: no MFMA.
// Semantics: PlainValuesReader (plain/PlainValuesReader.java:32-138), value for value.
#include <hip/hip_runtime.h>

#include "pqgpu_device.h"

namespace pqg {

// ---------------------------------------------------------------------------
// PLAIN fixed width (PlainValuesReader / FixedLenByteArrayPlainValuesReader):
// byte copy of n_values * W bytes from the data section, EOF at the first
// value that does not fit.
// A workgroup per page, its WPB waves interleaved over the page's 1 KiB rows (wave w: rows w, w + WPB, ...):
// with one wave per page a page of 160 KB was one wave's serial copy (a load, its wait and a 1 KiB store per
// row), and C5's 14,224 pages took two uneven rounds of the resident waves.
__global__ __launch_bounds__(64 * WPB) void k_plain(const uint8_t* __restrict__ bytes, uint64_t n_bytes,
                                              const PageWork* __restrict__ work, const ColumnDev* __restrict__ cols,
                                              const int32_t* __restrict__ list, int n_list, uint64_t* err,
                                              ErrCount err_count) {
  const int page = (int)blockIdx.x < n_list ? list[blockIdx.x] : -1;
  if (page < 0) return;
  const uint32_t part = wave_id();
  const PageWork pw = work[page];
  const ColumnDev cd = cols[pw.column];
  const uint32_t lane = lane_id();
  const uint32_t W = uni((uint32_t)cd.elem_width);
  const uint32_t beg = uni(pw.data_begin), end = uni(pw.size);
  uint32_t n = uni(pw.n_values);
  const uint32_t avail = end > beg ? end - beg : 0;
  if ((uint64_t)n * W > avail) {
    uint32_t fit = avail / W;
    if (lane == 0 && part == 0) report(err, err_count, page, 2, fit, PQG_ERR_EOF);
    n = fit;
  }
  rsrc_t rs = make_rsrc(bytes + pw.base, n_bytes - pw.base);
  uint8_t* dst = (uint8_t*)cd.values + pw.out_offset * W;
  const uint64_t nb = (uint64_t)n * W;
  const uint32_t src0 = beg;
  // destination-aligned 16-byte chunks
  const uintptr_t d0 = (uintptr_t)dst, d1 = d0 + nb;
  const uintptr_t a0 = (d0 + 15u) & ~(uintptr_t)15u, a1 = d1 & ~(uintptr_t)15u;
  if (a0 >= a1) {  // tiny: bytewise
    if (part == 0)
      for (uint64_t i = lane; i < nb; i += WAVE) gst(dst + i, (uint8_t)(ld32(rs, (src0 + (uint32_t)i) & ~3u) >> (((src0 + (uint32_t)i) & 3u) * 8u)));
    return;
  }
  const uint32_t head = (uint32_t)(a0 - d0), tail = (uint32_t)(d1 - a1);
  if (part == 0 && lane < head) {
    uint32_t o = src0 + lane;
    gst(dst + lane, (uint8_t)(ld32(rs, o & ~3u) >> ((o & 3u) * 8u)));
  }
  if (part == 0 && lane < tail) {
    uint64_t i = (a1 - d0) + lane;
    uint32_t o = src0 + (uint32_t)i;
    gst(dst + i, (uint8_t)(ld32(rs, o & ~3u) >> ((o & 3u) * 8u)));
  }
  typedef uint32_t v4 __attribute__((ext_vector_type(4)));
  const uint64_t nchunks = (a1 - a0) >> 4;
  const uint32_t sbase = src0 + head;           // source offset of the first aligned chunk
  const uint32_t mis = sbase & 3u;
  for (uint64_t c = WAVE * part + lane; c < nchunks; c += WAVE * WPB) {
    uint32_t so = sbase + (uint32_t)(c << 4);
    v4 v;
    if (mis == 0) {
      v = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)so, 0, 0);
    } else {
      uint32_t a = so & ~3u, sh = mis * 8u;
      uint32_t x0 = ld32(rs, a), x1 = ld32(rs, a + 4), x2 = ld32(rs, a + 8), x3 = ld32(rs, a + 12), x4 = ld32(rs, a + 16);
      v.x = (x0 >> sh) | (x1 << (32u - sh));
      v.y = (x1 >> sh) | (x2 << (32u - sh));
      v.z = (x2 >> sh) | (x3 << (32u - sh));
      v.w = (x3 >> sh) | (x4 << (32u - sh));
    }
    gst_nt((v4*)(a0 + (c << 4)), v);
  }
}

// PLAIN BOOLEAN (BooleanPlainValuesReader -> ByteBitPackingValuesReader(1, LE)):
// bit i of the section (bytes past the section read as 0) -> one byte 0/1.
__global__ __launch_bounds__(64 * WPB) void k_plain_bool(const uint8_t* __restrict__ bytes, uint64_t n_bytes,
                                                   const PageWork* __restrict__ work, const ColumnDev* __restrict__ cols,
                                                   const int32_t* __restrict__ list, int n_list, uint64_t* err,
                                                   ErrCount err_count) {
  const int page = wave_page(list, n_list);
  if (page < 0) return;
  const PageWork pw = work[page];
  const ColumnDev cd = cols[pw.column];
  const uint32_t lane = lane_id();
  const uint32_t beg = uni(pw.data_begin), end = uni(pw.size);
  const uint32_t n = uni(pw.n_values);
  // ByteBitPackingValuesReader.initFromPage :77-88: min(ceil(num_values/8), available) bytes
  uint64_t want = ((uint64_t)pw.num_slots + 7u) / 8u;
  uint32_t avail = end > beg ? end - beg : 0;
  uint32_t lim = beg + (uint32_t)(want < avail ? want : avail);
  rsrc_t rs = make_rsrc(bytes + pw.base, n_bytes - pw.base);
  uint8_t* dst = (uint8_t*)cd.values + pw.out_offset;
  for (uint32_t i = lane; i < n; i += WAVE) {
    uint32_t o = beg + (i >> 3);
    uint32_t b = o < lim ? (ld32(rs, o & ~3u) >> ((o & 3u) * 8u)) & 0xFFu : 0u;
    gst(dst + i, (uint8_t)((b >> (i & 7u)) & 1u));
  }
}

// ---------------------------------------------------------------------------
// ParquetReadRouter batch: run r unpacks counts[r] LSB-first values of width w.
__global__ __launch_bounds__(256) void k_unpack_runs(int w, const uint8_t* __restrict__ in, uint64_t in_bytes,
                                                     const uint64_t* __restrict__ in_off, const uint32_t* __restrict__ counts,
                                                     const uint64_t* __restrict__ out_off, int32_t* __restrict__ out,
                                                     int n_runs) {
  const int r = blockIdx.y;
  if (r >= n_runs) return;
  const uint32_t cnt = counts[r];
  rsrc_t rs = make_rsrc(in + in_off[r], in_bytes - in_off[r]);
  int32_t* o = out + out_off[r];
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < cnt; i += gridDim.x * blockDim.x) {
    uint32_t v = 0;
    if (w) {
      uint64_t bit = (uint64_t)i * (uint32_t)w;
      uint32_t byte = (uint32_t)(bit >> 3), a = byte & ~3u;
      uint64_t x = (uint64_t)ld32(rs, a) | ((uint64_t)ld32(rs, a + 4) << 32);
      x >>= (byte - a) * 8u + (uint32_t)(bit & 7u);
      v = w == 32 ? (uint32_t)x : (uint32_t)x & ((1u << w) - 1u);
    }
    gst(o + i, (int32_t)v);
  }
}

// ---------------------------------------------------------------------------
// Launchers (host side of this translation unit)

hipError_t launch_plain(int kind, hipStream_t st, const uint8_t* bytes, uint64_t n_bytes, PageWork* work,
                        const ColumnDev* cols, const int32_t* list, int n, uint64_t* err, ErrCount err_count) {
  if (n <= 0) return hipSuccess;
  if (kind == 2) return launch_rle_bool(st, bytes, n_bytes, work, cols, list, n, err, err_count);
  if (kind == 1)
    hipLaunchKernelGGL(k_plain_bool, dim3((n + WPB - 1) / WPB), dim3(64 * WPB), 0, st, bytes, n_bytes, work, cols, list,
                       n, err, err_count);
  else  // a workgroup per page
    hipLaunchKernelGGL(k_plain, dim3(n), dim3(64 * WPB), 0, st, bytes, n_bytes, work, cols, list, n, err, err_count);
  return hipGetLastError();
}

hipError_t launch_unpack_runs(hipStream_t st, int w, const uint8_t* in, uint64_t in_bytes, const uint64_t* in_off,
                              const uint32_t* counts, const uint64_t* out_off, int32_t* out, int n_runs,
                              uint32_t max_count) {
  if (n_runs <= 0) return hipSuccess;
  uint32_t gx = (max_count + 255u) / 256u;
  if (gx == 0) gx = 1;
  if (gx > 64) gx = 64;
  hipLaunchKernelGGL(k_unpack_runs, dim3(gx, n_runs), dim3(256), 0, st, w, in, in_bytes, in_off, counts, out_off, out,
                     n_runs);
  return hipGetLastError();
}

#ifdef PQG_DIAG
int diag_nostore_plain(int v) {
  return hipMemcpyToSymbol(HIP_SYMBOL(pqg_diag_nostore), &v, sizeof(v)) == hipSuccess ? 0 : 3;
}
#endif

}  // namespace pqg
