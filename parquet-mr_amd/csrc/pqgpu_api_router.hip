// pqgpu_api_router.hip — the C ABI of ParquetReadRouter.read: bit-packed runs from host memory, unpacked on
// the device into host memory (pqg_router_read, _read_runs), and the page-wide variant that walks the
// hybrid stream once and serves the later reads from a cache (pqg_router_read_page, _cache_lookup,
// _cache_stats). The stream walk, the cache and the pinned image's layout are plain C++
// (pqgpu_api_host.cpp); here are the allocations, the copies and the launches.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "pqgpu_ctx.h"

extern "C" {

int pqg_router_read(pqg_ctx* ctx, int bit_width, const uint8_t* in, size_t in_len, int count, int32_t* out) {
  if (!ctx || bit_width < 0 || bit_width > 32 || count < 0 || (count && (!in || !out))) return PQG_ERR_INVALID_ARG;
  if (count % 8 != 0) return PQG_ERR_INVALID_ARG;  // currentCount of a bit-packed run is a multiple of 8
  const uint64_t need = (uint64_t)count * (uint64_t)bit_width / 8u;
  if (need > in_len) return PQG_ERR_EOF;  // in.slice(count * bitWidth / 8) -> EOFException
  if (count == 0) return PQG_OK;
  ctx->staged.clear();  // pin_in / pin_out are reused: an earlier staged decode's outputs are gone
  if (hipSetDevice(ctx->device) != hipSuccess) return PQG_ERR_HIP;
  hipStream_t s = ctx->stream;
  const uint64_t in_al = (need + 16 + 255) & ~uint64_t(255);
  const uint64_t tail = 32;  // [in_off, counts, out_off]
  if (ctx->host_runs.ensure(in_al + (uint64_t)count * 4 + 256 + tail) != hipSuccess ||
      ctx->pin_in.ensure(in_al + tail) != hipSuccess || ctx->pin_out.ensure((uint64_t)count * 4) != hipSuccess)
    return PQG_ERR_HIP;
  uint8_t* pin = (uint8_t*)ctx->pin_in.p;
  std::memcpy(pin, in, need);
  std::memset(pin + need, 0, in_al - need);
  uint64_t* meta = (uint64_t*)(pin + in_al);
  meta[0] = 0;                               // in offset
  ((uint32_t*)&meta[1])[0] = (uint32_t)count; // count
  meta[2] = 0;                               // out offset
  uint8_t* d = (uint8_t*)ctx->host_runs.p;
  int32_t* dout = (int32_t*)(d + in_al + tail + 256 - ((uintptr_t)(d + in_al + tail) & 255));
  if (hipMemcpyAsync(d, pin, in_al + tail, hipMemcpyHostToDevice, s) != hipSuccess) return PQG_ERR_HIP;
  hipError_t e = pqg::launch_unpack_runs(s, bit_width, d, need + 16, (const uint64_t*)(d + in_al),
                                         (const uint32_t*)(d + in_al + 8), (const uint64_t*)(d + in_al + 16), dout, 1,
                                         (uint32_t)count);
  if (e != hipSuccess) return PQG_ERR_HIP;
  if (hipMemcpyAsync(ctx->pin_out.p, dout, (size_t)count * 4, hipMemcpyDeviceToHost, s) != hipSuccess) return PQG_ERR_HIP;
  if (hipStreamSynchronize(s) != hipSuccess) return PQG_ERR_HIP;
  std::memcpy(out, ctx->pin_out.p, (size_t)count * 4);
  return PQG_OK;
}

int pqg_router_read_runs(pqg_ctx* ctx, int bit_width, const uint8_t* in, size_t in_len, const uint64_t* in_offsets,
                         const uint32_t* counts, int n_runs, int32_t* out) {
  if (!ctx || bit_width < 0 || bit_width > 32 || n_runs < 0) return PQG_ERR_INVALID_ARG;
  if (n_runs == 0) return PQG_OK;
  if (!in_offsets || !counts || !out) return PQG_ERR_INVALID_ARG;
  pqg::RouterRunsImage im;
  const int lrc = pqg::router_runs_layout(bit_width, in, in_len, in_offsets, counts, n_runs, &im);
  if (lrc != PQG_OK) return lrc;
  if (im.n_vals == 0) return PQG_OK;
  ctx->staged.clear();  // pin_in / pin_out are reused: an earlier staged decode's outputs are gone
  if (hipSetDevice(ctx->device) != hipSuccess) return PQG_ERR_HIP;
  hipStream_t s = ctx->stream;
  if (ctx->pin_in.ensure(im.img) != hipSuccess || ctx->pin_out.ensure(4 * im.n_vals) != hipSuccess ||
      ctx->host_runs.ensure(im.img + 4 * im.n_vals + 256) != hipSuccess)
    return PQG_ERR_HIP;
  uint8_t* pin = (uint8_t*)ctx->pin_in.p;
  pqg::router_runs_fill(im, bit_width, in, in_offsets, counts, n_runs, pin);
  uint8_t* d = (uint8_t*)ctx->host_runs.p;
  int32_t* dout = (int32_t*)(d + im.img);
  if (hipMemcpyAsync(d, pin, im.img, hipMemcpyHostToDevice, s) != hipSuccess) return PQG_ERR_HIP;
  for (int r0 = 0; r0 < n_runs; r0 += 65535) {  // grid.y holds the run index
    const int nr = std::min(n_runs - r0, 65535);
    const hipError_t e = pqg::launch_unpack_runs(s, bit_width, d, im.n_bytes + 16, (const uint64_t*)(d + im.o_in) + r0,
                                                 (const uint32_t*)(d + im.o_cnt) + r0, (const uint64_t*)(d + im.o_out) + r0,
                                                 dout, nr, im.max_count);
    if (e != hipSuccess) return PQG_ERR_HIP;
  }
  if (hipMemcpyAsync(ctx->pin_out.p, dout, (size_t)(4 * im.n_vals), hipMemcpyDeviceToHost, s) != hipSuccess) return PQG_ERR_HIP;
  if (hipStreamSynchronize(s) != hipSuccess) return PQG_ERR_HIP;
  std::memcpy(out, ctx->pin_out.p, (size_t)(4 * im.n_vals));
  return PQG_OK;
}

int pqg_router_cache_lookup(pqg_ctx* ctx, int bit_width, const uint8_t* run, size_t stream_left, int count,
                            int32_t* out, int* hit) {
  return pqg::router_cache_lookup(ctx ? &ctx->router : nullptr, bit_width, run, stream_left, count, out, hit);
}

int pqg_router_read_page(pqg_ctx* ctx, int bit_width, const uint8_t* in, size_t stream_left, int count, int32_t* out) {
  int hit = 0;
  const int lrc = pqg_router_cache_lookup(ctx, bit_width, in, stream_left, count, out, &hit);
  if (lrc != PQG_OK || hit) return lrc;
  if (!in) return PQG_ERR_INVALID_ARG;
  pqg::RouterCache& c = ctx->router;
  pqg::router_walk(c, bit_width, in, stream_left, count);
  const int rc = pqg_router_read_runs(ctx, bit_width, in, stream_left, c.off.data(), c.cnt.data(), (int)c.off.size(),
                                      c.vals.data());
  if (rc != PQG_OK) {
    c.off.clear();
    return rc;
  }
  c.w = bit_width;
  std::memcpy(out, c.vals.data(), (size_t)count * 4);
  return PQG_OK;
}

int pqg_router_cache_stats(pqg_ctx* ctx, uint64_t* hits, uint64_t* misses) {
  if (!ctx) return PQG_ERR_INVALID_ARG;
  if (hits) *hits = ctx->router.hits;
  if (misses) *misses = ctx->router.misses;
  return PQG_OK;
}

}  // extern "C"
