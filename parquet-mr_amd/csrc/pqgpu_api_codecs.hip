// pqgpu_api_codecs.hip — the C ABI's work on page bytes as they sit in the file: page checksums
// (pqg_crc32_pages), decryption (pqg_decrypt_pages) and
// the four decompressors (pqg_snappy_, pqg_lz4_raw_, pqg_gzip_, pqg_zstd_decompress), each with the
// *_sync call that waits for the jobs and reports the first that failed.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "pqgpu_ctx.h"

// The *_sync entry points: waits for the stream, reads the n_jobs status words and reports the first
// non-zero one as job `page` of `what_job` (a PQG_ERR_CRC as what_crc, a PQG_ERR_TAG as what_tag, where given).
static int job_status_sync(pqg_ctx* ctx, const int32_t* d_status, int n_jobs, pqg_status* st, const char* what,
                           const char* what_job, const char* what_crc = nullptr, const char* what_tag = nullptr) {
  if (!ctx || n_jobs < 0) return PQG_ERR_INVALID_ARG;
  if (hipStreamSynchronize(ctx->stream) != hipSuccess) return PQG_ERR_HIP;
  if (st) set_status(st, PQG_OK, -1, -1, what);
  if (!d_status || n_jobs == 0) return PQG_OK;
  std::vector<int32_t> h((size_t)n_jobs);
  if (hipMemcpy(h.data(), d_status, sizeof(int32_t) * (size_t)n_jobs, hipMemcpyDeviceToHost) != hipSuccess)
    return PQG_ERR_HIP;
  for (int j = 0; j < n_jobs; j++)
    if (h[(size_t)j]) {
      set_status(st, h[(size_t)j], j, -1,
                 h[(size_t)j] == PQG_ERR_CRC && what_crc ? what_crc : h[(size_t)j] == PQG_ERR_TAG && what_tag ? what_tag : what_job);
      return h[(size_t)j];
    }
  return PQG_OK;
}

extern "C" {

// ---- page checksums (pqgpu_crc_host.cpp validates and builds the tables, pqgpu_crc.hip runs) ---------
int pqg_crc32_pages(pqg_ctx* ctx, const uint8_t* d_bytes, uint64_t n_bytes, const pqg_crc_job* jobs, int n_jobs,
                    uint32_t* d_crc, int32_t* d_status) {
  uint64_t n_tiles = 0;
  const uint32_t T = ctx ? ctx->crc_tile : (uint32_t)PQG_CRC_TILE_BYTES;
  const int rc = pqg::crc_validate(ctx != nullptr, d_bytes, n_bytes, jobs, n_jobs, d_status, T, &n_tiles);
  if (rc != PQG_OK || n_jobs == 0) return rc;
  if (hipSetDevice(ctx->device) != hipSuccess) return PQG_ERR_HIP;
  if (ctx->crc_tab_tile != T) {  // the constants of this tile size (a pageable copy: done when it returns)
    std::vector<uint32_t> tab(pqg::crc_table_words(T));
    pqg::crc_build_tables(T, tab.data());
    if (hipStreamSynchronize(ctx->stream) != hipSuccess || ctx->crc_tab.ensure(4 * tab.size()) != hipSuccess ||
        hipMemcpy(ctx->crc_tab.p, tab.data(), 4 * tab.size(), hipMemcpyHostToDevice) != hipSuccess)
      return PQG_ERR_HIP;
    ctx->crc_tab_tile = T;
  }
  uint32_t slot;
  if (!ctx->crc_ring.acquire(&slot)) return PQG_ERR_HIP;  // (waits for the fold of this slot CRC_SLOTS calls ago)
  const size_t job_bytes = sizeof(pqg::CrcJobDev) * (size_t)n_jobs;  // a multiple of 8: the tiles follow
  const size_t bytes = job_bytes + sizeof(pqg::CrcTile) * (size_t)n_tiles;
  // grown by half again, so that a run of calls with rising page counts does not reallocate each time
  if (ctx->crc_pin[slot].cap < bytes && ctx->crc_pin[slot].ensure(bytes + bytes / 2) != hipSuccess) return PQG_ERR_HIP;
  if (ctx->crc_dev[slot].cap < bytes && ctx->crc_dev[slot].ensure(bytes + bytes / 2) != hipSuccess) return PQG_ERR_HIP;
  if (ctx->crc_partial[slot].cap < 4 * (size_t)n_tiles &&
      ctx->crc_partial[slot].ensure(6 * (size_t)n_tiles) != hipSuccess)
    return PQG_ERR_HIP;
  uint8_t* pin = (uint8_t*)ctx->crc_pin[slot].p;
  pqg::crc_build(jobs, n_jobs, T, (pqg::CrcJobDev*)pin, (pqg::CrcTile*)(pin + job_bytes));
  if (hipMemcpyAsync(ctx->crc_dev[slot].p, pin, bytes, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) return PQG_ERR_HIP;
  const uint8_t* dev = (const uint8_t*)ctx->crc_dev[slot].p;
  const hipError_t e = pqg::launch_crc(ctx->stream, d_bytes, n_bytes, (const pqg::CrcTile*)(dev + job_bytes), (uint32_t)n_tiles,
                                       (const pqg::CrcJobDev*)dev, (uint32_t)n_jobs, (const uint32_t*)ctx->crc_tab.p, T,
                                       (uint32_t*)ctx->crc_partial[slot].p, d_crc, d_status);
  if (e != hipSuccess || !ctx->crc_ring.publish(slot, ctx->stream)) return PQG_ERR_HIP;
  return PQG_OK;
}

int pqg_crc32_sync(pqg_ctx* ctx, const int32_t* d_status, int n_jobs, pqg_status* st) {
  return job_status_sync(ctx, d_status, n_jobs, st, "crc32", "crc32 job",
                         "could not verify page integrity, CRC checksum verification failed");
}

// ---- encrypted pages (pqgpu_aes_host.cpp validates and builds the tables, pqgpu_aes.hip runs) ---------
static_assert(sizeof(pqg_decrypt_job) == 40 && sizeof(pqg_aes_key) == 36, "decrypt job layout");

int pqg_decrypt_pages(pqg_ctx* ctx, const uint8_t* d_src, uint64_t n_src, uint8_t* d_dst, uint64_t n_dst,
                      const pqg_decrypt_job* jobs, int n_jobs, const pqg_aes_key* keys, int n_keys,
                      const uint8_t* aad, uint64_t aad_bytes, int32_t* d_status, pqg_status* st) {
  if (st) { std::memset(st, 0, sizeof(*st)); st->page = -1; }
  uint64_t n_tiles = 0, aad_blocks = 0;
  int bad = -1;
  const uint32_t T = ctx ? ctx->aes_tile : (uint32_t)PQG_AES_TILE_BYTES;
  const int rc = pqg::aes_validate(ctx != nullptr, d_src, n_src, d_dst, n_dst, jobs, n_jobs, keys, n_keys, aad, aad_bytes,
                                   d_status, T, &n_tiles, &aad_blocks, &bad);
  if (rc != PQG_OK) {
    set_status(st, rc, bad, -1, rc == PQG_ERR_CORRUPT ? "decrypt: Wrong input length" : "decrypt arguments");
    return rc;
  }
  if (n_jobs == 0) return PQG_OK;
  if (hipSetDevice(ctx->device) != hipSuccess) return PQG_ERR_HIP;
  if (!ctx->aes_te0.p) {  // (a pageable copy: done when it returns)
    uint32_t te[256];
    pqg::aes_te0(te);
    if (ctx->aes_te0.ensure(sizeof(te)) != hipSuccess ||
        hipMemcpy(ctx->aes_te0.p, te, sizeof(te), hipMemcpyHostToDevice) != hipSuccess) {
      ctx->aes_te0.release();
      return PQG_ERR_HIP;
    }
  }
  const size_t key_words = pqg::aes_key_words(T);
  const size_t keys_in = sizeof(pqg_aes_key) * (size_t)n_keys;
  if (ctx->aes_keys_tile != T || ctx->aes_keys_seen.size() != keys_in ||
      std::memcmp(ctx->aes_keys_seen.data(), keys, keys_in) != 0) {
    ctx->aes_wipe_keys(false);
    ctx->aes_keymat.assign(key_words * (size_t)n_keys, 0u);
    for (int k = 0; k < n_keys; k++)
      pqg::aes_build_key(keys[k].bytes, keys[k].size, T, ctx->aes_keymat.data() + key_words * (size_t)k);
    ctx->aes_keys_seen.assign((const uint8_t*)keys, (const uint8_t*)keys + keys_in);
    ctx->aes_keys_tile = T;
  }
  uint32_t slot;
  if (!ctx->aes_ring.acquire(&slot)) return PQG_ERR_HIP;  // (waits for the fold of this slot AES_SLOTS calls ago)
  // A failure below returns without publish(), as in pqg_crc32_pages: nothing that reads the slot was queued, so
  // its event stays as it was (never recorded, or recorded behind work that has since run) and the next
  // acquire() of the slot returns at once, which is right.
  // jobs (64 bytes each), tiles (32), AAD blocks (16), key material (a multiple of 16): each part 16-byte aligned
  const size_t job_bytes = sizeof(pqg::AesJobDev) * (size_t)n_jobs, tile_bytes = sizeof(pqg::AesTile) * (size_t)n_tiles;
  const size_t aad_off = job_bytes + tile_bytes, key_off = aad_off + 16 * (size_t)aad_blocks;
  const size_t bytes = key_off + 4 * key_words * (size_t)n_keys;
  if (ctx->aes_pin[slot].cap < bytes && ctx->aes_pin[slot].ensure(bytes + bytes / 2) != hipSuccess) return PQG_ERR_HIP;
  if (ctx->aes_dev[slot].cap < bytes && ctx->aes_dev[slot].ensure(bytes + bytes / 2) != hipSuccess) return PQG_ERR_HIP;
  if (ctx->aes_partial[slot].cap < 16 * (size_t)n_tiles && ctx->aes_partial[slot].ensure(24 * (size_t)n_tiles) != hipSuccess)
    return PQG_ERR_HIP;
  uint8_t* pin = (uint8_t*)ctx->aes_pin[slot].p;
  pqg::aes_build(jobs, n_jobs, aad, T, (pqg::AesJobDev*)pin, (pqg::AesTile*)(pin + job_bytes), pin + aad_off);
  std::memcpy(pin + key_off, ctx->aes_keymat.data(), 4 * key_words * (size_t)n_keys);
  if (hipMemcpyAsync(ctx->aes_dev[slot].p, pin, bytes, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) return PQG_ERR_HIP;
  const uint8_t* dev = (const uint8_t*)ctx->aes_dev[slot].p;
  const hipError_t e = pqg::launch_decrypt(ctx->stream, d_src, n_src, d_dst, (const pqg::AesTile*)(dev + job_bytes),
                                           (uint32_t)n_tiles, (const pqg::AesJobDev*)dev, (uint32_t)n_jobs, dev + aad_off,
                                           (const uint32_t*)ctx->aes_te0.p, (const uint32_t*)(dev + key_off), T,
                                           ctx->aes_partial[slot].p, d_status);
  if (e != hipSuccess || !ctx->aes_ring.publish(slot, ctx->stream)) return PQG_ERR_HIP;
  return PQG_OK;
}

int pqg_decrypt_sync(pqg_ctx* ctx, const int32_t* d_status, int n_jobs, pqg_status* st) {
  return job_status_sync(ctx, d_status, n_jobs, st, "decrypt", "decrypt job", nullptr, "GCM tag check failed");
}

static_assert(sizeof(pqg_copy_range) == 24, "pqg_copy_range layout");

int pqg_copy_ranges(pqg_ctx* ctx, const uint8_t* d_src, uint64_t n_src, uint8_t* d_dst, uint64_t n_dst,
                    const pqg_copy_range* d_ranges, int n) {
  if (!ctx || n < 0) return PQG_ERR_INVALID_ARG;
  if (n == 0) return PQG_OK;
  if (!d_src || !d_dst || !d_ranges) return PQG_ERR_INVALID_ARG;
  if (hipSetDevice(ctx->device) != hipSuccess) return PQG_ERR_HIP;
  const hipError_t e = pqg::launch_copy_ranges(ctx->stream, d_src, n_src, d_dst, n_dst, d_ranges, (uint32_t)n);
  return e == hipSuccess ? PQG_OK : PQG_ERR_HIP;
}

static_assert(sizeof(pqg_snappy_job) == 24, "pqg_snappy_job layout");

int pqg_snappy_decompress(pqg_ctx* ctx, const uint8_t* d_src, uint64_t src_bytes, uint8_t* d_dst, uint64_t dst_bytes,
                          const pqg_snappy_job* d_jobs, int n_jobs, int32_t* d_status) {
  if (!ctx || n_jobs < 0) return PQG_ERR_INVALID_ARG;
  if (n_jobs == 0) return PQG_OK;
  if (!d_src || !d_dst || !d_jobs) return PQG_ERR_INVALID_ARG;
  if (hipSetDevice(ctx->device) != hipSuccess) return PQG_ERR_HIP;
  const hipError_t e = pqg::launch_snappy(ctx->stream, d_src, src_bytes, d_dst, dst_bytes, d_jobs, n_jobs, d_status);
  return e == hipSuccess ? PQG_OK : PQG_ERR_HIP;
}

int pqg_snappy_sync(pqg_ctx* ctx, const int32_t* d_status, int n_jobs, pqg_status* st) {
  return job_status_sync(ctx, d_status, n_jobs, st, "snappy", "snappy block");
}

int pqg_lz4_raw_decompress(pqg_ctx* ctx, const uint8_t* d_src, uint64_t src_bytes, uint8_t* d_dst, uint64_t dst_bytes,
                           const pqg_lz4_job* d_jobs, int n_jobs, int32_t* d_status) {
  if (!ctx || n_jobs < 0) return PQG_ERR_INVALID_ARG;
  if (n_jobs == 0) return PQG_OK;
  if (!d_src || !d_dst || !d_jobs) return PQG_ERR_INVALID_ARG;
  if (hipSetDevice(ctx->device) != hipSuccess) return PQG_ERR_HIP;
  const hipError_t e = pqg::launch_lz4raw(ctx->stream, d_src, src_bytes, d_dst, dst_bytes, d_jobs, n_jobs, d_status);
  return e == hipSuccess ? PQG_OK : PQG_ERR_HIP;
}

int pqg_lz4_raw_sync(pqg_ctx* ctx, const int32_t* d_status, int n_jobs, pqg_status* st) {
  return job_status_sync(ctx, d_status, n_jobs, st, "lz4_raw", "lz4_raw block");
}

int pqg_gzip_decompress(pqg_ctx* ctx, const uint8_t* d_src, uint64_t src_bytes, uint8_t* d_dst, uint64_t dst_bytes,
                        const pqg_gzip_job* d_jobs, int n_jobs, int32_t* d_status) {
  if (!ctx || n_jobs < 0) return PQG_ERR_INVALID_ARG;
  if (n_jobs == 0) return PQG_OK;
  if (!d_src || !d_dst || !d_jobs) return PQG_ERR_INVALID_ARG;
  if (hipSetDevice(ctx->device) != hipSuccess) return PQG_ERR_HIP;
  // token pre-pass scratch: dst_bytes / 3 + 2 eight-byte records and one word per job; without it
  // every job takes the scalar decoder
  uint64_t* recs = nullptr;
  int32_t* mode = nullptr;
  {
    const size_t need_r = 8u * (size_t)(dst_bytes / 3u + 2u), need_m = 4u * (size_t)n_jobs;
    if (ctx->gzip_recs.cap < need_r || ctx->gzip_mode.cap < need_m) {
      if (hipStreamSynchronize(ctx->stream) != hipSuccess) return PQG_ERR_HIP;
      if (ctx->gzip_recs.ensure(need_r) != hipSuccess || ctx->gzip_mode.ensure(need_m) != hipSuccess) {
        (void)hipGetLastError();
        ctx->gzip_recs.release();
        ctx->gzip_mode.release();
      }
    }
    if (ctx->gzip_recs.cap >= need_r && ctx->gzip_mode.cap >= need_m) {
      recs = (uint64_t*)ctx->gzip_recs.p;
      mode = (int32_t*)ctx->gzip_mode.p;
    }
  }
  const hipError_t e = pqg::launch_gzip(ctx->stream, d_src, src_bytes, d_dst, dst_bytes, d_jobs, n_jobs, d_status,
                                        recs, mode, ctx->gz_prepass_min);
  return e == hipSuccess ? PQG_OK : PQG_ERR_HIP;
}

int pqg_gzip_sync(pqg_ctx* ctx, const int32_t* d_status, int n_jobs, pqg_status* st) {
  return job_status_sync(ctx, d_status, n_jobs, st, "gzip", "gzip block");
}

int pqg_zstd_decompress(pqg_ctx* ctx, const uint8_t* d_src, uint64_t src_bytes, uint8_t* d_dst, uint64_t dst_bytes,
                        const pqg_zstd_job* d_jobs, int n_jobs, int32_t* d_status) {
  if (!ctx || n_jobs < 0) return PQG_ERR_INVALID_ARG;
  if (n_jobs == 0) return PQG_OK;
  if (!d_src || !d_dst || !d_jobs) return PQG_ERR_INVALID_ARG;
  if (hipSetDevice(ctx->device) != hipSuccess) return PQG_ERR_HIP;
  // the scratch may be in use by a previous call still queued on the stream: grow only after it
  // one literal buffer per wave of the (bounded) grid, not per job
  const uint64_t slots = (uint64_t)std::min<int>(n_jobs, (int)pqg::ZSTD_GRID);
  if (ctx->zstd_scratch.cap < pqg::ZSTD_LIT_SCRATCH * slots) {
    if (hipStreamSynchronize(ctx->stream) != hipSuccess) return PQG_ERR_HIP;
    if (ctx->zstd_scratch.ensure(pqg::ZSTD_LIT_SCRATCH * slots) != hipSuccess) return PQG_ERR_HIP;
  }
  // sequence pre-pass scratch: dst_bytes / 5 + 1 eight-byte records (a job's records start at its
  // dst_offset / 5) and one mode word per job; without it every job takes the inline decoder
  // (PQG_DISPATCH_ZSTD_PREPASS 0 asks for exactly that)
  uint64_t* seqs = nullptr;
  int32_t* mode = nullptr;
  if (ctx->zstd_prepass) {
    const size_t need_s = 8u * (size_t)(dst_bytes / 5u + 2u), need_m = 4u * (size_t)n_jobs;
    if (ctx->zstd_seqs.cap < need_s || ctx->zstd_mode.cap < need_m) {
      if (hipStreamSynchronize(ctx->stream) != hipSuccess) return PQG_ERR_HIP;
      if (ctx->zstd_seqs.ensure(need_s) != hipSuccess || ctx->zstd_mode.ensure(need_m) != hipSuccess) {
        (void)hipGetLastError();
        ctx->zstd_seqs.release();
        ctx->zstd_mode.release();
      }
    }
    if (ctx->zstd_seqs.cap >= need_s && ctx->zstd_mode.cap >= need_m) {
      seqs = (uint64_t*)ctx->zstd_seqs.p;
      mode = (int32_t*)ctx->zstd_mode.p;
    }
  }
  const hipError_t e = pqg::launch_zstd(ctx->stream, d_src, src_bytes, d_dst, dst_bytes, d_jobs, n_jobs, d_status,
                                        (uint8_t*)ctx->zstd_scratch.p, seqs, mode);
  return e == hipSuccess ? PQG_OK : PQG_ERR_HIP;
}

int pqg_zstd_sync(pqg_ctx* ctx, const int32_t* d_status, int n_jobs, pqg_status* st) {
  return job_status_sync(ctx, d_status, n_jobs, st, "zstd", "zstd frame");
}

}  // extern "C"
