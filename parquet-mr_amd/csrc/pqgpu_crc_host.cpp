// pqgpu_crc_host.cpp — the host half of pqg_crc32_pages (include/pqgpu.h, "page checksums") in plain
// C++: the refusals, the tile table, the GF(2) helpers, the generated constants (pqgpu_crc.h), and the
// two host-only entry points pqg_crc32_combine and pqg_crc_jobs_from_headers. No HIP here: tests/c
// builds this file with a sanitizer.
#include <cstdio>
#include <cstring>

#include "pqgpu_crc.h"

namespace pqg {

uint32_t crc_mulmodp(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (uint32_t m = CRC_X0; m; m >>= 1) {
    if (a & m) p ^= b;
    b = (b & 1u) ? (b >> 1) ^ CRC_POLY : b >> 1;
  }
  return p;
}

namespace {

// x^(2^k) mod P, k = 0..31 (x^(2^32) = x: the order of x divides 2^32 - 1)
struct X2n {
  uint32_t t[32];
  X2n() {
    uint32_t p = CRC_X0 >> 1;  // x^1
    for (int k = 0; k < 32; k++) {
      t[k] = p;
      p = crc_mulmodp(p, p);
    }
  }
};
const X2n& x2n() {
  static const X2n tab;
  return tab;
}
constexpr uint64_t ORDER = 0xFFFFFFFFull;  // 2^32 - 1

void set_status(pqg_status* st, int code, int page, int64_t idx, const char* what) {
  if (!st) return;
  st->code = code;
  st->page = page;
  st->value_index = idx;
  std::snprintf(st->message, sizeof(st->message), "%s", what);
}

}  // namespace

uint32_t crc_x8n(uint64_t n) {
  n %= ORDER;
  uint32_t p = CRC_X0;
  for (int k = 3; n; n >>= 1, k++)
    if (n & 1u) p = crc_mulmodp(x2n().t[k & 31], p);
  return p;
}

uint32_t crc_x8n_back(uint64_t n) { return crc_x8n(ORDER - n % ORDER); }

void crc_build_tables(uint32_t tile, uint32_t* out) {
  const uint32_t x32 = crc_x8n(4), xrow = crc_x8n(CRC_ROW), x8 = crc_x8n(1);
  for (uint32_t k = 0; k < 4; k++)
    for (uint32_t b = 0; b < 256; b++) {
      out[CRC_TAB_STEP4 + 256 * k + b] = crc_mulmodp(b << (8 * k), x32);
      out[CRC_TAB_ROW + 256 * k + b] = crc_mulmodp(b << (8 * k), xrow);
    }
  uint32_t p = crc_x8n_back(tile);
  for (uint32_t i = 0; i < 2 * tile; i++) {
    out[CRC_TAB_XP8 + i] = p;
    p = crc_mulmodp(p, x8);
  }
  const uint32_t xtile = crc_x8n(tile);
  p = CRC_X0;
  for (uint32_t k = 0; k <= CRC_FOLD_LANES; k++) {
    out[crc_tab_xt(tile) + k] = p;
    p = crc_mulmodp(p, xtile);
  }
}

int crc_validate(bool have_ctx, const void* d_bytes, uint64_t n_bytes, const pqg_crc_job* jobs, int n_jobs,
                 const void* d_status, uint32_t tile, uint64_t* n_tiles) {
  if (n_tiles) *n_tiles = 0;
  if (!have_ctx || n_jobs < 0 || !crc_tile_ok(tile) || !n_tiles) return PQG_ERR_INVALID_ARG;
  if (n_jobs == 0) return PQG_OK;
  if (!jobs || !d_bytes || !d_status) return PQG_ERR_INVALID_ARG;
  uint64_t total = 0;
  for (int j = 0; j < n_jobs; j++) {
    const pqg_crc_job& J = jobs[j];
    if (J.reserved || (J.flags & ~(uint32_t)PQG_CRC_VERIFY)) return PQG_ERR_INVALID_ARG;
    if (J.offset > n_bytes || J.size > n_bytes - J.offset) return PQG_ERR_INVALID_ARG;
    total += ((uint64_t)J.size + tile - 1) / tile;
  }
  if (total > CRC_MAX_TILES) return PQG_ERR_UNSUPPORTED;
  *n_tiles = total;
  return PQG_OK;
}

void crc_build(const pqg_crc_job* jobs, int n_jobs, uint32_t tile, CrcJobDev* jd, CrcTile* tiles) {
  uint64_t at = 0;
  for (int j = 0; j < n_jobs; j++) {
    const pqg_crc_job& J = jobs[j];
    const uint32_t nt = (uint32_t)(((uint64_t)J.size + tile - 1) / tile);
    jd[j] = CrcJobDev{at, J.size, J.expected, J.flags, nt};
    for (uint32_t t = 0; t < nt; t++) {
      const uint64_t lo = (uint64_t)t * tile;
      const uint64_t left = (uint64_t)J.size - lo;
      tiles[at + t] = CrcTile{J.offset + lo, left < tile ? (uint32_t)left : tile, t == 0 ? CRC_TILE_FIRST : 0u};
    }
    at += nt;
  }
}

}  // namespace pqg

extern "C" {

uint32_t pqg_crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b) {
  return pqg::crc_mulmodp(pqg::crc_x8n(len_b), crc_a) ^ crc_b;
}

int pqg_crc_jobs_from_headers(const pqg_page_header* headers, int n_headers, uint64_t chunk_offset, pqg_crc_job* jobs,
                              int32_t* header_of_job, int capacity, int* n_jobs, pqg_status* st) {
  if (st) std::memset(st, 0, sizeof(*st));
  if (n_jobs) *n_jobs = 0;
  if (n_headers < 0 || (n_headers > 0 && !headers) || !n_jobs || capacity < 0 || (capacity > 0 && !jobs)) {
    pqg::set_status(st, PQG_ERR_INVALID_ARG, -1, -1, "pqg_crc_jobs_from_headers: bad arguments");
    return PQG_ERR_INVALID_ARG;
  }
  int n = 0;
  for (int i = 0; i < n_headers; i++) {
    const pqg_page_header& h = headers[i];
    if (!h.has_crc) continue;
    if (h.type != PQG_DICTIONARY_PAGE && h.type != PQG_DATA_PAGE && h.type != PQG_DATA_PAGE_V2) continue;
    if (h.compressed_page_size < 0) {
      pqg::set_status(st, PQG_ERR_INVALID_ARG, i, -1, "pqg_crc_jobs_from_headers: negative compressed_page_size");
      return PQG_ERR_INVALID_ARG;
    }
    if (n < capacity) {
      jobs[n] = pqg_crc_job{chunk_offset + h.body_offset, (uint32_t)h.compressed_page_size, h.crc, PQG_CRC_VERIFY, 0};
      if (header_of_job) header_of_job[n] = i;
    }
    n++;
  }
  *n_jobs = n;
  if (n > capacity) {
    pqg::set_status(st, PQG_ERR_INVALID_ARG, -1, n, "pqg_crc_jobs_from_headers: job capacity too small (value_index = needed)");
    return PQG_ERR_INVALID_ARG;
  }
  return PQG_OK;
}

}  // extern "C"
