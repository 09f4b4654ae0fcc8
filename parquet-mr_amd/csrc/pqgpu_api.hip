// pqgpu_api.hip — the C ABI of include/pqgpu.h.
//
// Host work here is descriptor bookkeeping only (page tables, class lists,
// prefix sums of header value counts, error resolution); every byte of page
// data is decoded by the kernels in pqgpu_kernels.hip. There is no CPU decode
// fallback: without a usable HIP device every entry point returns
// PQG_ERR_NO_DEVICE.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <new>
#include <atomic>
#include <thread>
#include <type_traits>
#include <vector>

#include "pqgpu_internal.h"
#include "pqgpu_filter.h"
#include "pqgpu_take.h"
#include "pqgpu_crc.h"

using pqg::ColumnDev;
using pqg::PageWork;
using pqg::HostErr;
using pqg::bin_out;
using pqg::elem_width;
using pqg::out_width;
// pqg::Cls
using pqg::C_DICT4; using pqg::C_DICT8; using pqg::C_IDS; using pqg::C_PLAIN; using pqg::C_BOOL; using pqg::C_DELTA4;
using pqg::C_DELTA8; using pqg::C_BSS; using pqg::C_BINP; using pqg::C_DLBA; using pqg::C_DBA; using pqg::C_RLEBOOL;
using pqg::C_DD; using pqg::C_DDG; using pqg::C_NCLS;

namespace {

const char* kNames[] = {"OK", "INVALID_ARG", "UNSUPPORTED", "HIP", "NO_DEVICE"};

void set_status(pqg_status* st, int code, int page, int64_t idx, const char* what) {
  if (!st) return;
  st->code = code;
  st->page = page;
  st->value_index = idx;
  std::snprintf(st->message, sizeof(st->message), "%s: %s (page %d, index %lld)", what, pqg_error_name(code), page,
                (long long)idx);
}

struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  hipError_t ensure(size_t n) {
    if (n <= cap) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    hipError_t e = hipMalloc(&p, n ? n : 16);
    if (e == hipSuccess) cap = n ? n : 16;
    return e;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
};

struct PinnedBuf {
  void* p = nullptr;
  size_t cap = 0;
  hipError_t ensure(size_t n) {
    if (n <= cap) return hipSuccess;
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
    hipError_t e = hipHostMalloc(&p, n ? n : 16, hipHostMallocDefault);
    if (e == hipSuccess) cap = n ? n : 16;
    return e;
  }
  void release() {
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
  }
};

// Error words: 3 per page + 3 per column (dictionary pages), padded to 16 bytes; the error
// counter follows them in the same allocation.
size_t err_region_bytes(int n_pages, int n_cols) {
  return (sizeof(uint64_t) * 3 * (size_t)(n_pages + std::max(n_cols, 1)) + 15) & ~(size_t)15;
}

// The device buffers of a plan.
enum PlanBuf {
  B_WORK, B_COLS, B_LISTS, B_COL_PAGES, B_COL_PAGE_START, B_ERR,
  // BYTE_ARRAY / fixed-width-dictionary scratch (PlanLayout::regions), dictionary walks, post-passes,
  // offset-scan blocks, copy chunks
  B_BSCRATCH, B_BIN_LISTS, B_BIN_BLOCKS, B_BIN_CHUNKS, B_DBA_CHUNKS,
  B_SEGS,        // PLAIN BYTE_ARRAY segments (k_bin_walk_seg)
  B_DENT_TILES,  // large dictionaries' tiles (launch_dict_entries)
  B_PSEGS, B_PSTATUS, B_PCOL_PAGES, B_PCOL_START,  // one-pass PLAIN: tiles; aggw + incw per tile; column page lists
  B_REC, B_CHUNK_RUN, B_CHUNKS,  // dictionary pages: run records, chunk -> record, chunk work list
  B_PSTAT, B_FLAGS,              // per page: {records, values} and ready epoch (fused dictionary kernel)
  B_COUNT
};

// One row per buffer: what plan creation allocates (`alloc` bytes, with the slack the kernels read past
// the tables' ends) and how it fills the first `bytes`: copied from `host`, or zeroed.
struct PlanBufInit {
  PlanBuf buf;
  const void* host;
  size_t bytes, alloc;
  bool zero;
};

template <class T>
PlanBufInit uploaded(PlanBuf b, const std::vector<T>& v, size_t min_elems) {
  return PlanBufInit{b, v.data(), sizeof(T) * v.size(), sizeof(T) * std::max(v.size(), min_elems), false};
}

}  // namespace

struct pqg_plan {
  pqg_ctx* ctx = nullptr;
  const uint8_t* d_bytes = nullptr;
  uint64_t n_bytes = 0;
  pqg::PlanLayout L;  // what the planner computed from the descriptors (pqgpu_plan.h)
  DevBuf buf[B_COUNT];
  uint32_t* dba_meta() const {
    return L.dba_meta_off == pqg::NO_REGION ? nullptr : (uint32_t*)((uint8_t*)buf[B_BSCRATCH].p + L.dba_meta_off);
  }
  // ---- launch-time state
  uint32_t epoch = 0;
  uint32_t err_epoch = pqg::ERR_EPOCH_MAX;  // error-word epoch of the last launch (first launch wraps: zeroes the region)
  uint32_t pseg_epoch = 0;                  // k_bin_plain tile words' epoch (1..255)
  bool dict_fused = true;
  // one-pass PLAIN columns (pqg_sync turns plain_fused off when a page's values do not fill its data section)
  bool plain_fused = false;
  // seg_walk false: the segmented PLAIN pages one wave per page instead (pqg_sync's re-run after a segment
  // wait timed out)
  bool seg_walk = true;
  // V2 header null counts in use; a mismatch makes pqg_sync re-run level-first, and the plan keeps that
  // order (null_hints false)
  bool null_hints = false;
  int kernels = 0;
  int timeout_fallbacks = 0;  // launches re-run in split mode after PQG_ERR_TIMEOUT (pqg_sync)
  int plain_fallbacks = 0;
  int hint_fallbacks = 0;
  uint32_t* d_counts = nullptr;  // pqg_decode's d_page_value_counts (refreshed after a re-run)
  std::vector<pqg_page_error> page_errs;  // per page, resolved by pqg_sync (pqg_page_errors)
};

// pqg_router_read_page: the bit-packed runs of a hybrid stream's tail, walked on the host at the first
// read of a page, unpacked on the device in one round trip and served from host memory by the later
// reads (ParquetReadRouter.read: the values are in the caller's buffer when the call returns).
struct RouterCache {
  int w = -1;
  uint64_t tail_len = 0;        // bytes from the walked tail's start to the stream's end
  std::vector<uint8_t> bytes;   // the tail (a cached run is served only when its bytes equal the request's)
  std::vector<uint64_t> off;    // run data start, relative to the tail start (ascending)
  std::vector<uint32_t> cnt;    // values of the run
  std::vector<uint64_t> vo;     // first value of the run in vals
  std::vector<int32_t> vals;
  uint64_t hits = 0, misses = 0;
};

struct pqg_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  pqg_plan* last = nullptr;          // plan of the most recent pqg_decode (owned)
  pqg_plan* last_launched = nullptr; // plan of the most recent launch (decode or plan_launch)
  std::vector<pqg_plan*> unsynced;   // plans launched since the last pqg_sync, in launch order
  std::vector<pqg_staged_output> staged;  // pqg_decode_staged: where each column's outputs are in pin_out
  pqg_column_desc* last_cols = nullptr;
  PinnedBuf pin_in, pin_out, pin_err;
  DevBuf host_bytes, host_out, host_counts, host_runs;
  DevBuf asm_scratch;                // pqg_assemble: block counts + totals
  hipStream_t copy_stream = nullptr; // pqg_decode_host: second D2H queue (odd output chunks)
  DevBuf zstd_scratch;               // pqg_zstd_decompress: literal buffers, ZSTD_LIT_SCRATCH per grid wave
  DevBuf zstd_seqs, zstd_mode;       // pqg_zstd_decompress: sequence records of the lane-per-page pre-pass, per-job mode
  DevBuf gzip_recs, gzip_mode;       // pqg_gzip_decompress: back-reference records of the token pre-pass, per-job count
  // pqg_plan_launch: the one-pass PLAIN BYTE_ARRAY kernel runs on a second queue beside the other
  // columns' kernels (forked after the levels, joined before the launch ends)
  hipStream_t side_stream = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  // ... and the BYTE_ARRAY kernels of the other columns (dictionary walk / ids / map, per-value walks,
  // offset scan, copies) on a third, beside the fixed-width columns' kernels
  hipStream_t bin_stream = nullptr;
  hipEvent_t ev_join_bin = nullptr;
  // ... and the fixed-width columns' kernels on a fourth. The three are created one after the other
  // with the context, so that HIP's round-robin puts them on different hardware queues; the caller's
  // stream only waits while they run (a queue shared with it costs nothing then).
  hipStream_t fix_stream = nullptr;
  hipEvent_t ev_join_fix = nullptr;
  // ... and the tile walk of large dictionaries beside the id walk of their dictionary-direct pages, whose
  // ids need no entries (C_DDG: the entries are first read by k_dd_gsums, which waits for ev_dent)
  hipStream_t dent_stream = nullptr;
  hipEvent_t ev_dent_fork = nullptr, ev_dent = nullptr;
  // pqg_ctx_set_dispatch: kernel-choice overrides for the plans created on this ctx
  int plain_mode = 2;       // PQG_DISPATCH_PLAIN_ONE_PASS
  bool dict_direct = true;  // PQG_DISPATCH_DICT_DIRECT
  bool dict_fused = true;   // PQG_DISPATCH_DICT_FUSED
  bool null_hints = true;   // PQG_DISPATCH_NULL_HINTS
  uint32_t gz_prepass_min = pqg::GZ_PREPASS_MIN;  // PQG_DISPATCH_GZIP_PREPASS_MIN
  bool zstd_prepass = true;  // PQG_DISPATCH_ZSTD_PREPASS
  RouterCache router;  // pqg_router_read_page
  // pqg_filter_run: per-tile counts, and the device image of the filter uploaded last (by its serial)
  DevBuf filter_scratch, filter_image;
  uint64_t filter_serial = 0;
  // pqg_filter_run_dict: the FilterDictTab on the device and its pinned slots (as take_cols / take_pin)
  DevBuf filter_dict;
  PinnedBuf filter_dict_pin;
  hipEvent_t filter_dict_ev[4] = {};
  uint32_t filter_dict_seq = 0;
  // pqg_decode_dictionary: the one-column batch it decodes (last_cols points at dict_desc until the next
  // decode) and the caller's descriptor that pqg_sync fills from it
  pqg_column_desc dict_desc = {};
  pqg_column_desc* dict_user = nullptr;
  // pqg_take: per-tile counts; the column table on the device and the pinned slots it is copied from
  // (a slot is reused once the copy out of it has run: its event)
  static constexpr int TAKE_SLOTS = 4;
  // one slot holds the table of either call (pqg_take: TakeColDev, pqg_take_records: TakeRecDev)
  static constexpr size_t TAKE_SLOT_BYTES = sizeof(pqg::TakeRecDev) * pqg::TAKE_REC_MAX_RECORDS;
  DevBuf take_scratch, take_cols;
  PinnedBuf take_pin;
  hipEvent_t take_ev[TAKE_SLOTS] = {};
  uint32_t take_seq = 0;
  bool take_staged = true;  // PQG_DISPATCH_TAKE_STAGED
  // pqg_crc32_pages: the constants of crc_tile on the device (built at the first call and when the tile
  // size changes), and per slot the job + tile tables in growable pinned memory, their device copy and
  // the tiles' partial values (a slot is reused once the fold that read it has run: its event)
  static constexpr int CRC_SLOTS = 2;
  uint32_t crc_tile = PQG_CRC_TILE_BYTES;  // PQG_DISPATCH_CRC_TILE_BYTES
  uint32_t crc_tab_tile = 0;
  DevBuf crc_tab;
  PinnedBuf crc_pin[CRC_SLOTS];
  DevBuf crc_dev[CRC_SLOTS], crc_partial[CRC_SLOTS];
  hipEvent_t crc_ev[CRC_SLOTS] = {};
  uint32_t crc_seq = 0;
};

extern "C" {

int pqg_abi_version(void) { return PQG_ABI_VERSION; }

const char* pqg_error_name(int code) {
  switch (code) {
    case PQG_OK: case PQG_ERR_INVALID_ARG: case PQG_ERR_UNSUPPORTED: case PQG_ERR_HIP: case PQG_ERR_NO_DEVICE:
      return kNames[code];
    case PQG_ERR_TIMEOUT: return "TIMEOUT";
    case PQG_ERR_EOF: return "EOF";
    case PQG_ERR_RLE_PAST_END: return "RLE_PAST_END";
    case PQG_ERR_BIT_WIDTH: return "BIT_WIDTH";
    case PQG_ERR_DICT_ID: return "DICT_ID";
    case PQG_ERR_EMPTY_PAGE: return "EMPTY_PAGE";
    case PQG_ERR_EMPTY_PACKED_RUN: return "EMPTY_PACKED_RUN";
    case PQG_ERR_DELTA_CONFIG: return "DELTA_CONFIG";
    case PQG_ERR_DELTA_PAST_END: return "DELTA_PAST_END";
    case PQG_ERR_CORRUPT: return "CORRUPT";
    case PQG_ERR_NO_DICTIONARY: return "NO_DICTIONARY";
    case PQG_ERR_DICT_ENCODING: return "DICT_ENCODING";
    case PQG_ERR_CRC: return "CRC";
    default: return "UNKNOWN";
  }
}

int pqg_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int pqg_ctx_create(int device, void* hip_stream, pqg_ctx** out) {
  if (!out) return PQG_ERR_INVALID_ARG;
  *out = nullptr;
  int n = pqg_device_count();
  if (n <= 0) return PQG_ERR_NO_DEVICE;
  if (device < 0 || device >= n) return PQG_ERR_INVALID_ARG;
  if (hipSetDevice(device) != hipSuccess) return PQG_ERR_HIP;
  pqg_ctx* c = new (std::nothrow) pqg_ctx();
  if (!c) return PQG_ERR_INVALID_ARG;
  c->device = device;
  if (hip_stream) {
    c->stream = (hipStream_t)hip_stream;
  } else {
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
      delete c;
      return PQG_ERR_HIP;
    }
    c->own_stream = true;
  }
  if (hipStreamCreateWithFlags(&c->side_stream, hipStreamNonBlocking) != hipSuccess) c->side_stream = nullptr;
  if (hipStreamCreateWithFlags(&c->bin_stream, hipStreamNonBlocking) != hipSuccess) c->bin_stream = nullptr;
  if (hipStreamCreateWithFlags(&c->fix_stream, hipStreamNonBlocking) != hipSuccess) c->fix_stream = nullptr;
  *out = c;
  return PQG_OK;
}

void* pqg_ctx_stream(pqg_ctx* ctx) { return ctx ? (void*)ctx->stream : nullptr; }

int pqg_ctx_set_dispatch(pqg_ctx* ctx, int key, int value) {
  if (!ctx) return PQG_ERR_INVALID_ARG;
  switch (key) {
    case PQG_DISPATCH_PLAIN_ONE_PASS:
      if (value < 0 || value > 3) return PQG_ERR_INVALID_ARG;
      ctx->plain_mode = value;
      return PQG_OK;
    case PQG_DISPATCH_DICT_DIRECT:
      if (value != 0 && value != 1) return PQG_ERR_INVALID_ARG;
      ctx->dict_direct = value != 0;
      return PQG_OK;
    case PQG_DISPATCH_GZIP_PREPASS_MIN:
      if (value < 0) return PQG_ERR_INVALID_ARG;
      ctx->gz_prepass_min = (uint32_t)value;
      return PQG_OK;
    case PQG_DISPATCH_DICT_FUSED:
      if (value != 0 && value != 1) return PQG_ERR_INVALID_ARG;
      ctx->dict_fused = value != 0;
      return PQG_OK;
    case PQG_DISPATCH_NULL_HINTS:
      if (value != 0 && value != 1) return PQG_ERR_INVALID_ARG;
      ctx->null_hints = value != 0;
      return PQG_OK;
    case PQG_DISPATCH_TAKE_STAGED:
      if (value != 0 && value != 1) return PQG_ERR_INVALID_ARG;
      ctx->take_staged = value != 0;
      return PQG_OK;
    case PQG_DISPATCH_ZSTD_PREPASS:
      if (value != 0 && value != 1) return PQG_ERR_INVALID_ARG;
      ctx->zstd_prepass = value != 0;
      return PQG_OK;
    case PQG_DISPATCH_CRC_TILE_BYTES:
      if (value < 0 || !pqg::crc_tile_ok((uint32_t)value)) return PQG_ERR_INVALID_ARG;
      ctx->crc_tile = (uint32_t)value;
      return PQG_OK;
    default: return PQG_ERR_INVALID_ARG;
  }
}

int pqg_plan_destroy(pqg_plan* p);

int pqg_ctx_destroy(pqg_ctx* c) {
  if (!c) return PQG_OK;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  if (c->last) pqg_plan_destroy(c->last);
  c->pin_in.release();
  c->pin_out.release();
  c->pin_err.release();
  c->host_bytes.release();
  c->host_out.release();
  c->host_counts.release();
  c->host_runs.release();
  c->asm_scratch.release();
  c->zstd_scratch.release();
  c->zstd_seqs.release();
  c->zstd_mode.release();
  c->gzip_recs.release();
  c->gzip_mode.release();
  c->filter_scratch.release();
  c->filter_image.release();
  c->filter_dict.release();
  c->filter_dict_pin.release();
  for (hipEvent_t& e : c->filter_dict_ev)
    if (e) (void)hipEventDestroy(e);
  c->take_scratch.release();
  c->take_cols.release();
  c->take_pin.release();
  for (hipEvent_t& e : c->take_ev)
    if (e) (void)hipEventDestroy(e);
  c->crc_tab.release();
  for (int i = 0; i < pqg_ctx::CRC_SLOTS; i++) {
    c->crc_pin[i].release();
    c->crc_dev[i].release();
    c->crc_partial[i].release();
    if (c->crc_ev[i]) (void)hipEventDestroy(c->crc_ev[i]);
  }
  if (c->copy_stream) {
    (void)hipStreamSynchronize(c->copy_stream);
    (void)hipStreamDestroy(c->copy_stream);
  }
  if (c->side_stream) {
    (void)hipStreamSynchronize(c->side_stream);
    (void)hipStreamDestroy(c->side_stream);
  }
  if (c->bin_stream) {
    (void)hipStreamSynchronize(c->bin_stream);
    (void)hipStreamDestroy(c->bin_stream);
  }
  if (c->ev_join_bin) (void)hipEventDestroy(c->ev_join_bin);
  if (c->fix_stream) {
    (void)hipStreamSynchronize(c->fix_stream);
    (void)hipStreamDestroy(c->fix_stream);
  }
  if (c->ev_join_fix) (void)hipEventDestroy(c->ev_join_fix);
  if (c->dent_stream) {
    (void)hipStreamSynchronize(c->dent_stream);
    (void)hipStreamDestroy(c->dent_stream);
  }
  if (c->ev_dent_fork) (void)hipEventDestroy(c->ev_dent_fork);
  if (c->ev_dent) (void)hipEventDestroy(c->ev_dent);
  if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
  if (c->ev_join) (void)hipEventDestroy(c->ev_join);
  if (c->own_stream) (void)hipStreamDestroy(c->stream);
  delete c;
  return PQG_OK;
}

// valid_bytes: the caller's data ends there (page and dictionary extents are checked against it); the
// kernels may read up to n_bytes (pqg_decode_host's zero padding past the caller's bytes)
// Kernels one launch of the plan runs (in its current modes).
static int plan_kernels(const pqg_plan* P) {
  return pqg::plan_kernel_count(P->L, P->plain_fused, P->dict_fused, P->null_hints);
}

static int plan_create_impl(pqg_ctx* ctx, const uint8_t* d_bytes, uint64_t n_bytes, uint64_t valid_bytes,
                            const pqg_column_desc* cols, int n_cols, const pqg_page_desc* pages, int n_pages,
                            pqg_plan** out, pqg_status* st) {
  if (st) { std::memset(st, 0, sizeof(*st)); st->page = -1; }
  if (!ctx || !out || n_cols < 0 || n_pages < 0 || (n_cols && !cols) || (n_pages && !pages) || (n_bytes && !d_bytes) ||
      ((uintptr_t)d_bytes & 3u)) {  // the batch buffer is read as dwords (scalar loads): 4-byte aligned
    set_status(st, PQG_ERR_INVALID_ARG, -1, -1, "plan arguments");
    return PQG_ERR_INVALID_ARG;
  }
  if (hipSetDevice(ctx->device) != hipSuccess) return PQG_ERR_HIP;
  pqg_plan* P = new (std::nothrow) pqg_plan();
  if (!P) return PQG_ERR_INVALID_ARG;
  P->ctx = ctx;
  P->d_bytes = d_bytes;
  P->n_bytes = n_bytes;
  pqg::PlanLayout& L = P->L;
  int bad_page = -1;
  if (pqg::plan_layout(n_bytes, valid_bytes, cols, n_cols, pages, n_pages,
                       pqg::PlanOptions{ctx->plain_mode, ctx->dict_direct, ctx->null_hints}, &L, &bad_page) != PQG_OK) {
    set_status(st, PQG_ERR_INVALID_ARG, bad_page, -1, "page descriptor");
    delete P;
    return PQG_ERR_INVALID_ARG;
  }
  P->dict_fused = ctx->dict_fused;
  P->plain_fused = L.n_pcp != 0;
  P->null_hints = L.null_hints;
  // ---- allocation. The minimum sizes and slack terms are what the kernels read past the tables' ends.
  const size_t pages1 = (size_t)std::max(n_pages, 1);
  const PlanBufInit init[B_COUNT] = {
      uploaded(B_WORK, L.h_work, 0),
      uploaded(B_COLS, L.cols, 0),
      uploaded(B_LISTS, L.flat, 1),
      uploaded(B_COL_PAGES, L.cp, 1),
      uploaded(B_COL_PAGE_START, L.cps, 0),
      {B_ERR, nullptr, 0, err_region_bytes(n_pages, n_cols) + 16, false},
      {B_BSCRATCH, nullptr, 0, (size_t)std::max<uint64_t>(L.scratch_bytes, 256), false},
      uploaded(B_BIN_LISTS, L.bl, 1),
      uploaded(B_BIN_BLOCKS, L.bin_blocks, 1),
      uploaded(B_BIN_CHUNKS, L.bin_chunks, 1),
      uploaded(B_DBA_CHUNKS, L.dba_chunks, 1),
      uploaded(B_SEGS, L.segs, 1),
      uploaded(B_DENT_TILES, L.dent_tiles, 1),
      uploaded(B_PSEGS, L.psegs, 1),
      {B_PSTATUS, nullptr, 2 * sizeof(uint64_t) * L.psegs.size(), 2 * sizeof(uint64_t) * std::max<size_t>(L.psegs.size(), 1), true},
      uploaded(B_PCOL_PAGES, L.pcp, 1),
      {B_PCOL_START, L.pcs.data(), L.pcp.empty() ? 0 : sizeof(int32_t) * L.pcs.size(), sizeof(int32_t) * L.pcs.size(), false},
      // the expansion prefetches a page's first 128 records
      {B_REC, nullptr, 0, sizeof(uint64_t) * (size_t)(L.rec_total + 2 * 64 + 16), false},
      {B_CHUNK_RUN, nullptr, 0, sizeof(uint32_t) * std::max<uint32_t>(L.chunk_total, 1), false},
      uploaded(B_CHUNKS, L.chunk_list, 1),
      {B_PSTAT, nullptr, 0, sizeof(uint64_t) * pages1, false},
      {B_FLAGS, nullptr, sizeof(uint32_t) * pages1, sizeof(uint32_t) * pages1, true},
  };
  hipStream_t s = ctx->stream;
  bool ok = true;
  for (const PlanBufInit& b : init) ok = ok && P->buf[b.buf].ensure(b.alloc) == hipSuccess;
  // ---- the columns' scratch pointers
  uint8_t* scb = (uint8_t*)P->buf[B_BSCRATCH].p;
  auto resolve = [&](auto*& ptr, uint64_t off) {
    if (off != pqg::NO_REGION) ptr = (std::remove_reference_t<decltype(ptr)>)(scb + off);
  };
  for (int i = 0; i < n_cols && ok; i++) {
    ColumnDev& d = L.cols[(size_t)i];
    resolve(d.blen, L.blen_off[(size_t)i]);  // (dictionary-id columns: the planner pointed it at `values`)
    resolve(d.bsrc, L.bsrc_off[(size_t)i]);
    resolve(d.dict_len, L.dlen_off[(size_t)i]);
    resolve(d.dict_src, L.dsrc_off[(size_t)i]);
    resolve(d.dict_ent, L.dent_off[(size_t)i]);
    resolve(d.block_sums, L.bsum_off[(size_t)i]);
    resolve(d.bin_total, L.bin_total_off[(size_t)i]);
  }
  // ---- upload
  for (const PlanBufInit& b : init) {
    if (!ok || !b.bytes) continue;
    ok = (b.zero ? hipMemsetAsync(P->buf[b.buf].p, 0, b.bytes, s)
                 : hipMemcpyAsync(P->buf[b.buf].p, b.host, b.bytes, hipMemcpyHostToDevice, s)) == hipSuccess;
  }
  // the epoch-tagged words of bscratch
  if (ok && L.n_pcp) ok = hipMemsetAsync(scb + L.pflag_off, 0, 8, s) == hipSuccess;
  if (ok && L.null_hints) ok = hipMemsetAsync(scb + L.hint_off, 0, 8, s) == hipSuccess;
  // the copies read the layout's host tables, which live as long as the plan; one wait all the same, so
  // that a failed copy is reported here
  ok = ok && hipStreamSynchronize(s) == hipSuccess;
  if (!ok) {
    set_status(st, PQG_ERR_HIP, -1, -1, "plan upload");
    pqg_plan_destroy(P);
    return PQG_ERR_HIP;
  }
  P->kernels = plan_kernels(P);
  *out = P;
  return PQG_OK;
}

int pqg_plan_kernel_count(pqg_plan* P) { return P ? P->kernels : 0; }

int pqg_plan_timeout_fallbacks(pqg_plan* P) { return P ? P->timeout_fallbacks : 0; }

int pqg_plan_plain_fallbacks(pqg_plan* P) { return P ? P->plain_fallbacks : 0; }

int pqg_plan_null_hint_fallbacks(pqg_plan* P) { return P ? P->hint_fallbacks : 0; }

int pqg_plan_launch(pqg_plan* P) {
  if (!P) return PQG_ERR_INVALID_ARG;
  pqg_ctx* ctx = P->ctx;
  hipStream_t s = ctx->stream;
  uint64_t* err = (uint64_t*)P->buf[B_ERR].p;
  // error words and the error counter share one allocation; both are tagged with the launch's
  // error epoch (pqg::ErrCount), so the region is zeroed only when the epoch wraps
  const size_t err_bytes = err_region_bytes(P->L.n_pages, P->L.n_cols);
  if (++P->err_epoch > pqg::ERR_EPOCH_MAX) {
    P->err_epoch = 1;
    if (hipMemsetAsync(P->buf[B_ERR].p, 0, err_bytes + 16, s) != hipSuccess) return PQG_ERR_HIP;
    if (P->L.n_pcp && hipMemsetAsync((uint8_t*)P->buf[B_BSCRATCH].p + P->L.pflag_off, 0, 8, s) != hipSuccess) return PQG_ERR_HIP;
    if (P->null_hints && hipMemsetAsync((uint8_t*)P->buf[B_BSCRATCH].p + P->L.hint_off, 0, 8, s) != hipSuccess) return PQG_ERR_HIP;
  }
  const pqg::ErrCount ecount{(uint32_t*)((uint8_t*)P->buf[B_ERR].p + err_bytes), P->err_epoch};
  PageWork* work = (PageWork*)P->buf[B_WORK].p;
  const ColumnDev* cols = (const ColumnDev*)P->buf[B_COLS].p;
  const int32_t* lists = (const int32_t*)P->buf[B_LISTS].p;
  const bool pf = P->plain_fused;
  const uint64_t clear = pf ? P->L.blen_bytes_nf : P->L.blen_bytes;
  if (clear && hipMemsetAsync(P->buf[B_BSCRATCH].p, 0, clear, s) != hipSuccess) return PQG_ERR_HIP;
  if (pf && ++P->pseg_epoch > 255u) {  // k_bin_plain tile words are tagged with 1..255
    P->pseg_epoch = 1;
    if (hipMemsetAsync(P->buf[B_PSTATUS].p, 0, 2 * sizeof(uint64_t) * P->L.n_psegs, s) != hipSuccess) return PQG_ERR_HIP;
  }
  for (void* v : P->L.empty_bin_values)
    if (hipMemsetAsync(v, 0, sizeof(int64_t), s) != hipSuccess) return PQG_ERR_HIP;
  // page ready flags compare against the launch epoch (even); a walker's early partial status is
  // flagged epoch - 1. Reset on wrap.
  P->epoch += 2;
  if (P->epoch == 0) {
    P->epoch = 2;
    if (hipMemsetAsync(P->buf[B_FLAGS].p, 0, sizeof(uint32_t) * (size_t)std::max(P->L.n_pages, 1), s) != hipSuccess)
      return PQG_ERR_HIP;
  }
  hipError_t e = hipSuccess;
  // level-first order: k_levels + k_scan_offsets give the nullable pages' counts and offsets before any
  // value kernel; with V2 header null counts (null_hints) the host has them and k_levels only verifies
  // them, on the caller's stream beside the forked value kernels (launched after the fork below)
  const bool hints = P->null_hints && P->L.levels_n;
  const int32_t* bl = (const int32_t*)P->buf[B_BIN_LISTS].p;
  auto launch_dent = [&](hipStream_t st) -> hipError_t {  // large dictionaries' entries, per 2 KiB tile
    uint8_t* scb = (uint8_t*)P->buf[B_BSCRATCH].p;
    return pqg::launch_dict_entries(st, P->d_bytes, P->n_bytes, cols, (const uint64_t*)P->buf[B_DENT_TILES].p, P->L.n_dent_tiles,
                                    bl + P->L.off_dent_cols, bl + P->L.off_dent_start, P->L.n_dent_cols,
                                    (uint64_t*)(scb + P->L.dent_rec_off), (uint16_t*)(scb + P->L.dent_scr_off),
                                    (uint64_t*)(scb + P->L.dent_tb_off), P->L.n_pages, err, ecount);
  };
  // every large dictionary's column dictionary-direct with HBM entries (C_DDG only): its tile walk runs
  // on a queue of its own from the start, beside the levels and the id walk (k_dict_fused_dd<DD_IDS>)
  bool dent_fork = false;
  if (e == hipSuccess && P->L.n_dent_tiles && P->L.cls_n[C_DDG] && !P->L.cls_n[C_DD] && !P->L.cls_n[C_IDS] && !P->L.n_bind) {
    dent_fork = (ctx->dent_stream || hipStreamCreateWithFlags(&ctx->dent_stream, hipStreamNonBlocking) == hipSuccess) &&
                (ctx->ev_dent_fork || hipEventCreateWithFlags(&ctx->ev_dent_fork, hipEventDisableTiming) == hipSuccess) &&
                (ctx->ev_dent || hipEventCreateWithFlags(&ctx->ev_dent, hipEventDisableTiming) == hipSuccess) &&
                hipEventRecord(ctx->ev_dent_fork, s) == hipSuccess &&
                hipStreamWaitEvent(ctx->dent_stream, ctx->ev_dent_fork, 0) == hipSuccess;
    if (dent_fork) {
      e = launch_dent(ctx->dent_stream);
      if (e == hipSuccess && hipEventRecord(ctx->ev_dent, ctx->dent_stream) != hipSuccess) e = hipErrorUnknown;
    }
  }
  auto launch_dict_walks = [&](hipStream_t st) -> hipError_t {
    hipError_t r = hipSuccess;
    if (P->L.n_dict_walk)  // BYTE_ARRAY dictionary entries (PlainBinaryDictionary ctor)
      r = pqg::launch_bin_walk(st, P->d_bytes, P->n_bytes, work, cols, bl + P->L.off_dict_walk, P->L.n_dict_walk, 1,
                               P->L.n_pages, err, ecount);
    if (r == hipSuccess && P->L.n_dent_tiles && !dent_fork) r = launch_dent(st);
    return r;
  };
  if (e == hipSuccess && P->L.levels_n && !hints) {
    e = pqg::launch_levels(s, P->d_bytes, P->n_bytes, work, cols, lists + P->L.levels_off, P->L.levels_n, err, ecount, nullptr);
    if (e == hipSuccess)
      e = pqg::launch_scan(s, work, (const int32_t*)P->buf[B_COL_PAGES].p, (const int32_t*)P->buf[B_COL_PAGE_START].p, P->L.n_scan_cols);
  }
  // The one-pass PLAIN BYTE_ARRAY kernel is latency / issue bound (~1 TB/s) and independent of the other
  // columns' kernels (most of them HBM bound): with other pages in the plan it runs on a second queue,
  // forked after the levels and joined at the end, so the two kinds share the chip.
  // The BYTE_ARRAY kernels of the other columns likewise go to a third queue when fixed-width columns'
  // kernels (HBM bound) are in the plan to share the chip with.
  bool fork = false, fork_bin = false, fork_fix = false;
  const bool has_fixed = P->L.cls_n[C_DICT4] || P->L.cls_n[C_DICT8] || P->L.cls_n[C_PLAIN] || P->L.cls_n[C_BOOL] ||
                         P->L.cls_n[C_RLEBOOL] || P->L.cls_n[C_DELTA4] || P->L.cls_n[C_DELTA8] || P->L.cls_n[C_BSS];
  const bool has_bin = P->L.n_dict_walk || P->L.n_dent_tiles || P->L.cls_n[C_IDS] || P->L.cls_n[C_DD] || P->L.cls_n[C_DDG] || P->L.cls_n[C_BINP] - P->L.n_binp_seg - (pf ? P->L.n_binp_fused : 0) > 0 ||
                       P->L.cls_n[C_DLBA] || P->L.cls_n[C_DBA] || P->L.n_segs;
  const bool want = e == hipSuccess && ((pf && (has_fixed || has_bin)) || (has_bin && has_fixed) ||
                                        (hints && (pf || has_bin || has_fixed)));
  const bool ev_ok = want && (ctx->ev_fork || hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming) == hipSuccess) &&
                     hipEventRecord(ctx->ev_fork, s) == hipSuccess;
  if (ev_ok && pf) {
    fork = (ctx->side_stream || hipStreamCreateWithFlags(&ctx->side_stream, hipStreamNonBlocking) == hipSuccess) &&
           (ctx->ev_join || hipEventCreateWithFlags(&ctx->ev_join, hipEventDisableTiming) == hipSuccess) &&
           hipStreamWaitEvent(ctx->side_stream, ctx->ev_fork, 0) == hipSuccess;
  }
  if (ev_ok && has_bin && (has_fixed || hints)) {
    fork_bin = (ctx->bin_stream || hipStreamCreateWithFlags(&ctx->bin_stream, hipStreamNonBlocking) == hipSuccess) &&
               (ctx->ev_join_bin || hipEventCreateWithFlags(&ctx->ev_join_bin, hipEventDisableTiming) == hipSuccess) &&
               hipStreamWaitEvent(ctx->bin_stream, ctx->ev_fork, 0) == hipSuccess;
  }
  if (ev_ok && (fork || fork_bin || hints) && has_fixed)
    fork_fix = (ctx->fix_stream || hipStreamCreateWithFlags(&ctx->fix_stream, hipStreamNonBlocking) == hipSuccess) &&
               (ctx->ev_join_fix || hipEventCreateWithFlags(&ctx->ev_join_fix, hipEventDisableTiming) == hipSuccess) &&
               hipStreamWaitEvent(ctx->fix_stream, ctx->ev_fork, 0) == hipSuccess;
  if (e == hipSuccess && hints)  // the level sections, verified against the header counts, beside the value kernels
    e = pqg::launch_levels(s, P->d_bytes, P->n_bytes, work, cols, lists + P->L.levels_off, P->L.levels_n, err, ecount,
                           (uint32_t*)((uint8_t*)P->buf[B_BSCRATCH].p + P->L.hint_off));
  if (e == hipSuccess && pf) {  // PLAIN-only BYTE_ARRAY columns: one pass (after the levels: n_values, out_offset)
    uint8_t* scb = (uint8_t*)P->buf[B_BSCRATCH].p;
    uint64_t* ps = (uint64_t*)P->buf[B_PSTATUS].p;
    e = pqg::launch_bin_plain(fork ? ctx->side_stream : s, P->d_bytes, P->n_bytes, work, cols, (const int32_t*)P->buf[B_PCOL_PAGES].p,
                              (const int32_t*)P->buf[B_PCOL_START].p, P->L.n_pcols, (const uint64_t*)P->buf[B_PSEGS].p, P->L.n_psegs, ps,
                              ps + P->L.n_psegs, (uint32_t*)(scb + P->L.pticket_off), P->pseg_epoch,
                              (uint32_t*)(scb + P->L.pflag_off), P->err_epoch, err, ecount, P->L.plain_pg, P->L.n_pcp);
    if (fork && hipEventRecord(ctx->ev_join, ctx->side_stream) != hipSuccess) e = hipErrorUnknown;
  }
  const hipStream_t sb = fork_bin ? ctx->bin_stream : s;  // BYTE_ARRAY kernels of the other columns
  const hipStream_t sf = fork_fix ? ctx->fix_stream : s;  // fixed-width columns
  if (e == hipSuccess) e = launch_dict_walks(sb);
  for (int k = 0; k < C_NCLS && e == hipSuccess; k++) {
    int n = P->L.cls_n[k] - (k == C_BINP ? P->L.n_binp_seg + (pf ? P->L.n_binp_fused : 0) : 0);
    if (!n) continue;
    const int32_t* l = lists + P->L.cls_off[k];
    switch (k) {
      case C_DICT4:
      case C_DICT8: {
        const int i = k - C_DICT4;
        e = pqg::launch_dict(k == C_DICT8 ? 8 : 4, sf, P->d_bytes, P->n_bytes, work, cols, l, n, (uint64_t*)P->buf[B_REC].p,
                             (uint32_t*)P->buf[B_CHUNK_RUN].p, (const uint64_t*)P->buf[B_CHUNKS].p + P->L.chunk_off[i], P->L.chunk_n[i],
                             (uint64_t*)P->buf[B_PSTAT].p, (uint32_t*)P->buf[B_FLAGS].p, P->epoch, P->dict_fused, err, ecount);
        break;
      }
      case C_IDS: {
        const int i = k - C_DICT4;
        e = pqg::launch_dict_ids(sb, P->d_bytes, P->n_bytes, work, cols, l, n, (uint64_t*)P->buf[B_REC].p,
                                 (uint32_t*)P->buf[B_CHUNK_RUN].p, (const uint64_t*)P->buf[B_CHUNKS].p + P->L.chunk_off[i],
                                 P->L.chunk_n[i], (uint64_t*)P->buf[B_PSTAT].p, (uint32_t*)P->buf[B_FLAGS].p, P->epoch, P->dict_fused, err, ecount);
        break;
      }
      case C_DD:
      case C_DDG: {
        const int g = k == C_DDG ? 1 : 0;
        e = pqg::launch_dict_dd(sb, P->d_bytes, P->n_bytes, work, cols, l, n, (uint64_t*)P->buf[B_REC].p,
                                (uint32_t*)P->buf[B_CHUNK_RUN].p, (const uint64_t*)P->buf[B_CHUNKS].p + P->L.dd_chunk_off[g],
                                P->L.dd_chunk_n[g], (uint64_t*)P->buf[B_PSTAT].p, (uint32_t*)P->buf[B_FLAGS].p, P->epoch, P->dict_fused,
                                err, ecount, (uint64_t*)((uint8_t*)P->buf[B_BSCRATCH].p + P->L.dd_sums_off[g]),
                                bl + P->L.off_dd_cols[g], bl + P->L.off_dd_start[g], P->L.n_dd_cols[g], P->L.dd_region, g == 1,
                                g == 1 && dent_fork ? ctx->ev_dent : nullptr);
        break;
      }
      case C_BSS: e = pqg::launch_bss(sf, P->d_bytes, P->n_bytes, work, cols, l, n, err, ecount); break;
      case C_BINP:
        e = pqg::launch_bin_walk(sb, P->d_bytes, P->n_bytes, work, cols, l, n, 0, P->L.n_pages, err, ecount);
        break;
      case C_DLBA: e = pqg::launch_dlba_lengths(sb, P->d_bytes, P->n_bytes, work, cols, l, n, err, ecount); break;
      case C_DBA:
        e = pqg::launch_dba_lengths(sb, P->d_bytes, P->n_bytes, work, cols, l, n, err, ecount, P->dba_meta());
        break;
      case C_PLAIN: e = pqg::launch_plain(0, sf, P->d_bytes, P->n_bytes, work, cols, l, n, err, ecount); break;
      case C_BOOL: e = pqg::launch_plain(1, sf, P->d_bytes, P->n_bytes, work, cols, l, n, err, ecount); break;
      case C_RLEBOOL: e = pqg::launch_plain(2, sf, P->d_bytes, P->n_bytes, work, cols, l, n, err, ecount); break;
      case C_DELTA4: e = pqg::launch_delta(4, sf, P->d_bytes, P->n_bytes, work, cols, l, n, err, ecount); break;
      case C_DELTA8: e = pqg::launch_delta(8, sf, P->d_bytes, P->n_bytes, work, cols, l, n, err, ecount); break;
    }
  }
  if (e == hipSuccess && P->L.n_segs && !P->seg_walk)  // the segmented pages one wave each (after a timeout)
    e = pqg::launch_bin_walk(sb, P->d_bytes, P->n_bytes, work, cols,
                             lists + P->L.cls_off[C_BINP] + (P->L.cls_n[C_BINP] - P->L.n_binp_seg), P->L.n_binp_seg, 0,
                             P->L.n_pages, err, ecount);
  if (e == hipSuccess && P->L.n_segs && P->seg_walk) {  // PLAIN BYTE_ARRAY pages in segments (status + ticket cleared above)
    uint8_t* scb = (uint8_t*)P->buf[B_BSCRATCH].p;
    e = pqg::launch_bin_walk_seg(sb, P->d_bytes, P->n_bytes, work, cols, (const uint64_t*)P->buf[B_SEGS].p, P->L.n_segs,
                                 (uint64_t*)(scb + P->L.seg_status_off), (uint32_t*)(scb + P->L.seg_status_off) + 2u * P->L.n_segs,
                                 (uint32_t*)(scb + P->L.seg_tmp_off), err, ecount);
  }
  // post-passes: dictionary ids -> BYTE_ARRAY entries / fixed-width entries; offsets; value bytes
  if (e == hipSuccess && P->L.n_bind) e = pqg::launch_bin_dict_map(sb, work, cols, bl + P->L.off_bind, P->L.n_bind);
  if (e == hipSuccess && P->L.n_fixd)
    e = pqg::launch_gather_fixed(sb, P->d_bytes, P->n_bytes, work, cols, bl + P->L.off_fixd, P->L.n_fixd);
  const uint32_t n_blocks = pf ? P->L.n_bin_blocks_nf : P->L.n_bin_blocks;
  if (e == hipSuccess && n_blocks)
    e = pqg::launch_bin_scan(sb, P->d_bytes, P->n_bytes, cols, bl + P->L.off_bin_cols, pf ? P->L.n_bin_cols_nf : P->L.n_bin_cols,
                             (const uint64_t*)P->buf[B_BIN_BLOCKS].p, n_blocks);
  const uint32_t n_chunks = pf ? P->L.n_bin_chunks_nf : P->L.n_bin_chunks;
  if (e == hipSuccess && n_chunks)
    e = pqg::launch_bin_copy(sb, P->d_bytes, P->n_bytes, work, cols, (const uint64_t*)P->buf[B_BIN_CHUNKS].p, n_chunks, err,
                             ecount);
  if (e == hipSuccess && P->L.cls_n[C_DBA])
    e = pqg::launch_dba_copy(sb, P->d_bytes, P->n_bytes, work, cols, lists + P->L.cls_off[C_DBA], P->L.cls_n[C_DBA],
                             (const uint64_t*)P->buf[B_DBA_CHUNKS].p, P->L.n_dba_chunks, P->dba_meta(), bl + P->L.off_carry,
                             P->L.n_carry, err, ecount);
  if (fork && hipStreamWaitEvent(s, ctx->ev_join, 0) != hipSuccess) e = hipErrorUnknown;
  if (fork_bin && (hipEventRecord(ctx->ev_join_bin, ctx->bin_stream) != hipSuccess ||
                   hipStreamWaitEvent(s, ctx->ev_join_bin, 0) != hipSuccess))
    e = hipErrorUnknown;
  if (fork_fix && (hipEventRecord(ctx->ev_join_fix, ctx->fix_stream) != hipSuccess ||
                   hipStreamWaitEvent(s, ctx->ev_join_fix, 0) != hipSuccess))
    e = hipErrorUnknown;
  ctx->last_launched = P;
  if (std::find(ctx->unsynced.begin(), ctx->unsynced.end(), P) == ctx->unsynced.end()) ctx->unsynced.push_back(P);
  return e == hipSuccess ? PQG_OK : PQG_ERR_HIP;
}

int pqg_plan_destroy(pqg_plan* P) {
  if (!P) return PQG_OK;
  if (P->ctx) {
    (void)hipStreamSynchronize(P->ctx->stream);
    if (P->ctx->last_launched == P) P->ctx->last_launched = nullptr;
    if (P->ctx->last == P) P->ctx->last = nullptr;
    auto& u = P->ctx->unsynced;
    u.erase(std::remove(u.begin(), u.end(), P), u.end());
  }
  for (DevBuf& b : P->buf) b.release();
  delete P;
  return PQG_OK;
}

}  // extern "C"

namespace {

int resolve_page_errors(pqg_plan* P, pqg_status* st, const std::vector<uint64_t>& errs);

// Resolve the first error of a launched plan in (page, value) order.
// Per page: init errors (rl init < dl init < data init) first; then value errors
// (values are decoded only for slots before a level error, so a value error is
// always earlier in the reference's read order); then level errors.
int resolve_errors(pqg_plan* P, pqg_status* st, std::vector<PageWork>* work_out) {
  pqg_ctx* ctx = P->ctx;
  hipStream_t s = ctx->stream;
  if (ctx->pin_err.ensure(16) != hipSuccess) return PQG_ERR_HIP;
  uint32_t* cnt = (uint32_t*)ctx->pin_err.p;
  if (hipMemcpyAsync(cnt, (uint8_t*)P->buf[B_ERR].p + err_region_bytes(P->L.n_pages, P->L.n_cols), sizeof(uint32_t),
                     hipMemcpyDeviceToHost, s) != hipSuccess)
    return PQG_ERR_HIP;
  bool need_work = false;
  for (auto v : P->L.col_nullable) need_work = need_work || v;
  if (need_work && work_out) {
    work_out->resize(P->L.h_work.size());
    if (hipMemcpyAsync(work_out->data(), P->buf[B_WORK].p, sizeof(PageWork) * P->L.h_work.size(), hipMemcpyDeviceToHost, s) != hipSuccess)
      return PQG_ERR_HIP;
  }
  if (hipStreamSynchronize(s) != hipSuccess) return PQG_ERR_HIP;
  std::vector<uint64_t> errs;
  if (*cnt == P->err_epoch) {  // a kernel of the last launch reported (see pqg::ErrCount)
    errs.resize(3 * (size_t)(P->L.n_pages + std::max(P->L.n_cols, 1)));
    if (hipMemcpy(errs.data(), P->buf[B_ERR].p, sizeof(uint64_t) * errs.size(), hipMemcpyDeviceToHost) != hipSuccess) return PQG_ERR_HIP;
    for (uint64_t& w : errs)  // words of earlier launches are stale: no error in this one
      w = (w >> 48) == P->err_epoch ? (~w & pqg::ERR_KEY_MASK) : ~0ull;
  }
  int rc = resolve_page_errors(P, st, errs);
  if (rc) return rc;
  // BYTE_ARRAY output capacity (API misuse, after the decode errors: values past a decode error
  // are not meaningful and may inflate the byte count)
  for (int i = 0; i < P->L.n_cols; i++) {
    if (P->L.bin_total_off[(size_t)i] == ~0ull) continue;
    uint64_t total = 0;
    if (hipMemcpy(&total, (uint8_t*)P->buf[B_BSCRATCH].p + P->L.bin_total_off[(size_t)i], sizeof(total), hipMemcpyDeviceToHost) !=
        hipSuccess)
      return PQG_ERR_HIP;
    if (total > P->L.bin_capacity[(size_t)i]) {
      if (st) {
        st->code = PQG_ERR_INVALID_ARG;
        st->page = -1;
        st->value_index = (int64_t)total;
        std::snprintf(st->message, sizeof(st->message),
                      "binary capacity: column %d needs %llu bytes of binary_data (capacity %llu)", i,
                      (unsigned long long)total, (unsigned long long)P->L.bin_capacity[(size_t)i]);
      }
      return PQG_ERR_INVALID_ARG;
    }
  }
  return PQG_OK;
}

int resolve_page_errors(pqg_plan* P, pqg_status* st, const std::vector<uint64_t>& errs) {
  // every page's own first error (pqg_page_errors), then the batch's first in page order (st)
  P->page_errs.assign((size_t)P->L.n_pages, pqg_page_error{PQG_OK, PQG_PHASE_NONE, -1});
  if (P->L.host_errs.empty() && errs.empty()) return PQG_OK;
  std::vector<const HostErr*> herr((size_t)std::max(P->L.n_pages, 1), nullptr);
  for (const HostErr& h : P->L.host_errs)
    if (!herr[(size_t)h.page]) herr[(size_t)h.page] = &h;
  int first = -1;
  for (int p = 0; p < P->L.n_pages; p++) {
    pqg_page_error& pe = P->page_errs[(size_t)p];
    const HostErr* h = herr[(size_t)p];
    // device-detected dictionary page errors (BYTE_ARRAY dictionary walk, pseudo page n_pages + column):
    // the ColumnReaderBase ctor reads the dictionary before the column's first page
    const int col = P->L.h_work[(size_t)p].column;
    const uint64_t d = (!errs.empty() && col >= 0 && col < P->L.n_cols && P->L.col_first_page[(size_t)col] == p)
                           ? errs[3 * (size_t)(P->L.n_pages + col)] : ~0ull;
    uint64_t init = errs.empty() ? ~0ull : errs[3 * (size_t)p];
    uint64_t lvl = errs.empty() ? ~0ull : errs[3 * (size_t)p + 1];
    uint64_t val = errs.empty() ? ~0ull : errs[3 * (size_t)p + 2];
    if (d != ~0ull) {
      pe = {(int32_t)(d & 0xFF), PQG_PHASE_DICTIONARY, -1};
    } else if (h && h->index == -1) {  // host-detected dictionary page error: before any page is read
      pe = {h->code, PQG_PHASE_DICTIONARY, -1};
    } else if (h || init != ~0ull) {   // init-phase errors: key = phase (0 rl, 1 dl, 2 data) << 8 | code
      const uint64_t hkey = h ? (((uint64_t)h->index << 8) | (uint64_t)h->code) : ~0ull;
      const uint64_t k = std::min(hkey, init);
      const int ph = (int)(k >> 8);
      pe = {(int32_t)(k & 0xFF), ph == 0 ? PQG_PHASE_RL_INIT : ph == 1 ? PQG_PHASE_DL_INIT : PQG_PHASE_DATA_INIT, -1};
    } else if (val != ~0ull) {
      // values are decoded only for slots before a level error: a value error comes first
      pe = {(int32_t)(val & 0xFF), PQG_PHASE_VALUE, (int64_t)(val >> 8)};
    } else if (lvl != ~0ull) {         // key = (slot << 1 | 0 rl / 1 dl) << 8 | code
      pe = {(int32_t)(lvl & 0xFF), ((lvl >> 8) & 1) ? PQG_PHASE_DL_READ : PQG_PHASE_RL_READ, (int64_t)(lvl >> 9)};
    }
    if (pe.code != PQG_OK && first < 0) first = p;
  }
  if (first < 0) return PQG_OK;
  const pqg_page_error& pe = P->page_errs[(size_t)first];
  switch (pe.phase) {
    case PQG_PHASE_DICTIONARY: set_status(st, pe.code, first, -1, "dictionary page"); break;
    case PQG_PHASE_DATA_INIT: set_status(st, pe.code, first, 0, "data init"); break;
    case PQG_PHASE_RL_INIT: case PQG_PHASE_DL_INIT: set_status(st, pe.code, first, 0, "level init"); break;
    case PQG_PHASE_VALUE: set_status(st, pe.code, first, pe.index, "value decode"); break;
    default: set_status(st, pe.code, first, pe.index, "level decode"); break;
  }
  return pe.code;
}

}  // namespace

namespace {

// pqg_sync for one launched plan: the PLAIN one-pass re-run, error resolution, the fused-kernel
// timeout re-run. `work` receives the plan's PageWork (nullable columns' value counts).
int sync_plan(pqg_plan* P, pqg_status* st, std::vector<PageWork>* work) {
  pqg_ctx* ctx = P->ctx;
  if (P->null_hints && P->L.levels_n) {
    // A V2 header null count that disagrees with the page's definition levels (or a level error on such
    // a page): the value kernels ran on wrong counts / offsets. The reference decodes by the levels
    // (ColumnReaderBase.java:650-676, 760-771), so the launch is re-run level-first, which rewrites every
    // output; the plan keeps that order.
    uint32_t flag = 0;
    if (hipMemcpy(&flag, (uint8_t*)P->buf[B_BSCRATCH].p + P->L.hint_off, sizeof(flag), hipMemcpyDeviceToHost) != hipSuccess)
      return PQG_ERR_HIP;
    if (flag == P->err_epoch) {
      P->null_hints = false;
      P->kernels = plan_kernels(P);
      P->hint_fallbacks++;
      const int lrc = pqg_plan_launch(P);
      if (lrc != PQG_OK) return lrc;
      if (P->d_counts &&  // pqg_decode's per-page counts, copied after the first launch
          hipMemcpy2DAsync(P->d_counts, sizeof(uint32_t), (const uint8_t*)P->buf[B_WORK].p + offsetof(PageWork, n_values),
                           sizeof(PageWork), sizeof(uint32_t), (size_t)P->L.n_pages, hipMemcpyDeviceToDevice,
                           ctx->stream) != hipSuccess)
        return PQG_ERR_HIP;
      if (hipStreamSynchronize(ctx->stream) != hipSuccess) return PQG_ERR_HIP;
    }
  }
  if (P->plain_fused) {
    // A PLAIN page whose values do not end at its section end (bytes the reader ignores after them)
    // breaks the one-pass path's byte bases: the launch is re-run on the per-value path (k_bin_walk,
    // offset scan, k_bin_copy), which reads exactly n_values values per page; the plan keeps that path.
    uint32_t flag = 0;
    if (hipMemcpy(&flag, (uint8_t*)P->buf[B_BSCRATCH].p + P->L.pflag_off, sizeof(flag), hipMemcpyDeviceToHost) != hipSuccess)
      return PQG_ERR_HIP;
    if (flag == P->err_epoch) {
      P->plain_fused = false;
      P->kernels = plan_kernels(P);
      P->plain_fallbacks++;
      const int lrc = pqg_plan_launch(P);
      if (lrc != PQG_OK) return lrc;
      if (hipStreamSynchronize(ctx->stream) != hipSuccess) return PQG_ERR_HIP;
    }
  }
  int rc = resolve_errors(P, st, work);
  // only a timeout of the fused dictionary kernel's hand-off is re-run in split mode (a PLAIN
  // BYTE_ARRAY segment walk that timed out waiting for its predecessor reaches the caller)
  const int tpage = st ? (int)st->page : -1;
  const int tcls = tpage >= 0 && tpage < P->L.n_pages ? P->L.page_cls[(size_t)tpage] : -1;
  if (rc == PQG_ERR_TIMEOUT && P->dict_fused && (tcls == C_DICT4 || tcls == C_DICT8 || tcls == C_IDS || tcls == C_DD || tcls == C_DDG)) {
    // The fused dictionary kernel's hand-off relies on the walker workgroups being dispatched before
    // the expansion workgroups that wait for them, which HIP does not promise. A launch in which an
    // expansion waited past SPIN_TIMEOUT_TICKS (it then stops and reports PQG_ERR_TIMEOUT; the walkers
    // still finish, so the grid drains) is re-run with the walk and the expansion as two launches,
    // which have no inter-workgroup waits; the plan keeps that mode. Every output of the re-run is
    // written again, so the result is the same bit for bit.
    P->dict_fused = false;
    P->kernels = plan_kernels(P);
    P->timeout_fallbacks++;
    rc = pqg_plan_launch(P);
    if (rc == PQG_OK) {
      if (st) { std::memset(st, 0, sizeof(*st)); st->page = -1; }
      work->clear();
      rc = resolve_errors(P, st, work);
    }
  }
  // likewise a segment of a segmented PLAIN BYTE_ARRAY page that waited past its bound for its
  // predecessor's publication (k_bin_walk_seg; the predecessor always holds an earlier ticket, so this
  // needs a starved wave): the plan re-runs with those pages one wave each and keeps that mode
  const int tpage2 = st ? (int)st->page : -1;
  const int tcls2 = tpage2 >= 0 && tpage2 < P->L.n_pages ? P->L.page_cls[(size_t)tpage2] : -1;
  if (rc == PQG_ERR_TIMEOUT && P->L.n_segs && P->seg_walk && tcls2 == C_BINP) {
    P->seg_walk = false;
    P->kernels = plan_kernels(P);
    P->timeout_fallbacks++;
    rc = pqg_plan_launch(P);
    if (rc == PQG_OK) {
      if (st) { std::memset(st, 0, sizeof(*st)); st->page = -1; }
      work->clear();
      rc = resolve_errors(P, st, work);
    }
  }
  return rc;
}

}  // namespace

extern "C" {

// pqg_decode_dictionary decodes a BYTE_ARRAY dictionary page as a PLAIN data page, where an entry that reaches
// past the page is an EOFException; PlainBinaryDictionary's slice of it is what pqg_decode reports as
// PQG_ERR_CORRUPT for a dictionary page. Error path only: the page's length prefixes, walked on the host.
static int dict_page_eof_code(const pqg_plan* P, const pqg_column_desc& user) {
  std::vector<uint8_t> page(user.dict_size);
  if (!page.empty() && hipMemcpy(page.data(), P->d_bytes + user.dict_offset, page.size(), hipMemcpyDeviceToHost) != hipSuccess)
    return PQG_ERR_HIP;
  uint64_t p = 0;
  for (uint32_t i = 0; i < user.dict_num_values; i++) {
    if (p + 4 > page.size()) return PQG_ERR_EOF;
    uint32_t len;
    std::memcpy(&len, page.data() + p, 4);
    if ((int32_t)len < 0 || p + 4 + len > page.size()) return PQG_ERR_CORRUPT;
    p += 4 + (uint64_t)len;
  }
  return PQG_ERR_EOF;
}

int pqg_sync(pqg_ctx* ctx, pqg_status* st) {
  if (st) { std::memset(st, 0, sizeof(*st)); st->page = -1; }
  if (!ctx) return PQG_ERR_INVALID_ARG;
  if (hipSetDevice(ctx->device) != hipSuccess) return PQG_ERR_HIP;
  if (hipStreamSynchronize(ctx->stream) != hipSuccess) {
    set_status(st, PQG_ERR_HIP, -1, -1, hipGetErrorString(hipGetLastError()));
    return PQG_ERR_HIP;
  }
  // every plan launched since the last sync, in launch order (re-runs inside sync_plan append the
  // plan again; the list is taken first and cleared at the end)
  std::vector<pqg_plan*> plans;
  plans.swap(ctx->unsynced);
  int rc = PQG_OK;
  for (pqg_plan* P : plans) {
    // sync_plan can return PQG_ERR_HIP before anything sets the status: start from "no error"
    pqg_status pst;
    std::memset(&pst, 0, sizeof(pst));
    pst.page = -1;
    std::vector<PageWork> work;
    int prc = sync_plan(P, &pst, &work);
    if (prc == PQG_ERR_EOF && P == ctx->last && ctx->dict_user && ctx->last_cols == &ctx->dict_desc &&
        ctx->dict_desc.physical_type == PQG_BYTE_ARRAY) {
      prc = dict_page_eof_code(P, *ctx->dict_user);
      set_status(&pst, prc, -1, pst.value_index, "dictionary page");
    }
    if (prc != PQG_OK && pst.code == 0 && pst.message[0] == '\0')
      set_status(&pst, prc, -1, -1, prc == PQG_ERR_HIP ? hipGetErrorString(hipGetLastError()) : "plan sync failed");
    if (prc != PQG_OK && rc == PQG_OK) {
      rc = prc;
      if (st) *st = pst;
    }
    if (prc == PQG_ERR_HIP) break;
    if (ctx->last_cols && P == ctx->last) {
      for (int i = 0; i < P->L.n_cols; i++) {
        uint64_t n = P->L.col_required_values[(size_t)i];
        if (P->L.col_nullable[(size_t)i] && !work.empty()) {
          n = 0;
          for (int p = 0; p < P->L.n_pages; p++)
            if (work[(size_t)p].column == i) n += work[(size_t)p].n_values;
        }
        ctx->last_cols[i].values_written = n;
      }
      if (ctx->dict_user && ctx->last_cols == &ctx->dict_desc) ctx->dict_user->values_written = ctx->dict_desc.values_written;
    }
  }
  ctx->unsynced.clear();
  return rc;
}

int pqg_plan_page_errors(pqg_plan* P, pqg_page_error* out, int n_pages) {
  if (!P || n_pages != P->L.n_pages || (n_pages && !out)) return PQG_ERR_INVALID_ARG;
  for (int p = 0; p < n_pages; p++)
    out[p] = (size_t)p < P->page_errs.size() ? P->page_errs[(size_t)p] : pqg_page_error{PQG_OK, PQG_PHASE_NONE, -1};
  return PQG_OK;
}

int pqg_page_errors(pqg_ctx* ctx, pqg_page_error* out, int n_pages) {
  if (!ctx || !ctx->last) return PQG_ERR_INVALID_ARG;
  return pqg_plan_page_errors(ctx->last, out, n_pages);
}

int pqg_plan_create(pqg_ctx* ctx, const uint8_t* d_bytes, uint64_t n_bytes, const pqg_column_desc* cols, int n_cols,
                    const pqg_page_desc* pages, int n_pages, pqg_plan** out, pqg_status* st) {
  return plan_create_impl(ctx, d_bytes, n_bytes, n_bytes, cols, n_cols, pages, n_pages, out, st);
}

static int decode_impl(pqg_ctx* ctx, const uint8_t* d_bytes, uint64_t n_bytes, uint64_t valid_bytes,
                       pqg_column_desc* cols, int n_cols, const pqg_page_desc* pages, int n_pages,
                       uint32_t* d_page_value_counts, pqg_status* st) {
  if (!ctx || n_cols < 0 || n_pages < 0 || (n_cols && !cols) || (n_pages && !pages)) return PQG_ERR_INVALID_ARG;
  // capacity checks (descriptor arithmetic)
  {
    std::vector<uint64_t> slots((size_t)std::max(n_cols, 1), 0);
    for (int p = 0; p < n_pages; p++)
      if (pages[p].column >= 0 && pages[p].column < n_cols) slots[(size_t)pages[p].column] += pages[p].num_values;
    for (int i = 0; i < n_cols; i++) {
      bool lv = cols[i].max_def > 0 || cols[i].max_rep > 0;
      const uint64_t need = slots[(size_t)i] + (bin_out(cols[i]) ? 1 : 0);  // offsets[n + 1]
      if (need > cols[i].values_capacity || (need && !cols[i].values) ||
          (lv && ((cols[i].max_def > 0 && cols[i].def_levels) || (cols[i].max_rep > 0 && cols[i].rep_levels)) &&
           slots[(size_t)i] > cols[i].levels_capacity)) {
        set_status(st, PQG_ERR_INVALID_ARG, -1, i, "output capacity");
        return PQG_ERR_INVALID_ARG;
      }
    }
  }
  ctx->dict_user = nullptr;
  if (ctx->last) {
    pqg_plan_destroy(ctx->last);
    ctx->last = nullptr;
  }
  pqg_plan* P = nullptr;
  int rc = plan_create_impl(ctx, d_bytes, n_bytes, valid_bytes, cols, n_cols, pages, n_pages, &P, st);
  if (rc) return rc;
  ctx->last = P;
  ctx->last_cols = cols;
  rc = pqg_plan_launch(P);
  P->d_counts = n_pages > 0 ? d_page_value_counts : nullptr;
  if (rc == PQG_OK && d_page_value_counts && n_pages > 0) {
    // n_values of every page (strided in PageWork) -> dense uint32 array
    rc = hipMemcpy2DAsync(d_page_value_counts, sizeof(uint32_t), (const uint8_t*)P->buf[B_WORK].p + offsetof(PageWork, n_values),
                          sizeof(PageWork), sizeof(uint32_t), (size_t)n_pages, hipMemcpyDeviceToDevice,
                          ctx->stream) == hipSuccess
             ? PQG_OK
             : PQG_ERR_HIP;
  }
  return rc;
}

int pqg_decode(pqg_ctx* ctx, const uint8_t* d_bytes, uint64_t n_bytes, pqg_column_desc* cols, int n_cols,
               const pqg_page_desc* pages, int n_pages, uint32_t* d_page_value_counts, pqg_status* st) {
  return decode_impl(ctx, d_bytes, n_bytes, n_bytes, cols, n_cols, pages, n_pages, d_page_value_counts, st);
}

// ---- host copies of the host path (pinned staging <-> caller arrays): one thread moves ~10 GB/s,
// so large copies are spread over up to 8 threads, and the D2H of the outputs is issued in chunks
// whose copies out of pinned memory start as each chunk lands.
namespace {
struct HostCopy {
  uint8_t* dst;
  uint64_t src;  // offset in the pinned buffer
  uint64_t len;
};
// D2H piece: each is copied out by one thread as soon as it lands, so the copy of the last piece is the
// tail after the link (32 MiB pieces: d2h+copy 21-24 ms for 800 MB against 14 ms of link, r05u)
constexpr uint64_t HOST_CHUNK = 8ull << 20;
inline int host_threads(uint64_t bytes) {
  const unsigned hw = std::thread::hardware_concurrency();
  const uint64_t want = bytes / (8ull << 20) + 1;
  // (16 threads measured 38.4 vs 36.9 GB/s for 8 on an 800 MB output: host memory bound, profiles/r05/e2e)
  return (int)std::min<uint64_t>({want, 8ull, hw ? (uint64_t)hw : 1ull});
}
// the parts of `jobs` inside [lo, hi) of the pinned buffer `base`
void copy_range(const std::vector<HostCopy>& jobs, const uint8_t* base, uint64_t lo, uint64_t hi) {
  for (const HostCopy& j : jobs) {
    const uint64_t a = std::max(lo, j.src), b = std::min(hi, j.src + j.len);
    if (a < b) std::memcpy(j.dst + (a - j.src), base + a, b - a);
  }
}
void par_memcpy(void* dst, const void* src, uint64_t n) {
  const int t = host_threads(n);
  if (t <= 1) { std::memcpy(dst, src, n); return; }
  std::vector<std::thread> th;
  const uint64_t per = (n / (uint64_t)t + 4095) & ~4095ull;
  for (int k = 0; k < t; k++) {
    const uint64_t a = std::min(n, per * (uint64_t)k), b = std::min(n, a + per);
    if (a < b) th.emplace_back([=] { std::memcpy((uint8_t*)dst + a, (const uint8_t*)src + a, b - a); });
  }
  for (auto& x : th) x.join();
}
}  // namespace

// The host path. h_bytes == nullptr: staged (pqg_decode_staged) — the bytes are already in ctx->pin_in,
// the outputs stay in ctx->pin_out and ctx->staged describes them; otherwise the caller's arrays.
static int host_path(pqg_ctx* ctx, const uint8_t* h_bytes, uint64_t n_bytes, pqg_column_desc* cols, int n_cols,
                     const pqg_page_desc* pages, int n_pages, uint32_t* h_page_value_counts, pqg_status* st) {
  if (st) { std::memset(st, 0, sizeof(*st)); st->page = -1; }
  const bool staged = h_bytes == nullptr;
  if (!ctx || n_cols < 0 || n_pages < 0 || (n_cols && !cols) || (n_pages && !pages)) return PQG_ERR_INVALID_ARG;
  if (staged && ctx->pin_in.cap < n_bytes + 1024) return PQG_ERR_INVALID_ARG;  // pqg_host_input first
  ctx->staged.clear();
  if (hipSetDevice(ctx->device) != hipSuccess) return PQG_ERR_HIP;
  hipStream_t s = ctx->stream;
  // PQG_HOST_TIMING=1: phase times of this call on stderr (diagnostics)
  static const bool timing = std::getenv("PQG_HOST_TIMING") != nullptr;
  auto t_last = std::chrono::steady_clock::now();
  auto phase = [&](const char* what) {
    if (!timing) return;
    const auto now = std::chrono::steady_clock::now();
    std::fprintf(stderr, "pqg_decode_host %-10s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(now - t_last).count());
    t_last = now;
  };
  const uint64_t pad = 1024;
  const size_t nc = (size_t)std::max(n_cols, 1);
  std::vector<uint64_t> slots(nc, 0), page_bytes(nc, 0);
  for (int p = 0; p < n_pages; p++)
    if (pages[p].column >= 0 && pages[p].column < n_cols) {
      slots[(size_t)pages[p].column] += pages[p].num_values;
      page_bytes[(size_t)pages[p].column] += pages[p].size;
    }
  // BYTE_ARRAY bytes on the device: PLAIN / DELTA_LENGTH values fit in their pages; dictionary
  // columns may expand, so the first attempt may come back short and is then re-run once at the
  // exact size the device counted
  std::vector<uint64_t> bin_cap(nc, 0);
  for (int i = 0; i < n_cols; i++)
    if (bin_out(cols[i]))
      bin_cap[(size_t)i] = page_bytes[(size_t)i] + (cols[i].dict_offset >= 0 ? 2 * (uint64_t)cols[i].dict_size : 0) + 64;
  if (ctx->host_bytes.ensure(n_bytes + pad) != hipSuccess || ctx->pin_in.ensure(n_bytes + pad) != hipSuccess ||
      ctx->host_counts.ensure(sizeof(uint32_t) * (size_t)std::max(n_pages, 1)) != hipSuccess) {
    set_status(st, PQG_ERR_HIP, -1, -1, "device buffers");
    return PQG_ERR_HIP;
  }
  // host -> pinned -> device (staged: the caller wrote the bytes into pin_in)
  if (!staged) par_memcpy(ctx->pin_in.p, h_bytes, n_bytes);
  std::memset((uint8_t*)ctx->pin_in.p + n_bytes, 0, pad);
  phase("stage-in");
  if (hipMemcpyAsync(ctx->host_bytes.p, ctx->pin_in.p, n_bytes + pad, hipMemcpyHostToDevice, s) != hipSuccess) return PQG_ERR_HIP;
  auto al = [](uint64_t x) { return (x + 255) & ~uint64_t(255); };
  std::vector<uint64_t> off_v(nc), off_d(nc), off_r(nc), off_b(nc);
  std::vector<pqg_column_desc> dcols(cols, cols + n_cols);
  // levels wanted: staged -> every column with a max level > 0; else where the caller gave an array
  std::vector<uint8_t> want_d(nc, 0), want_r(nc, 0);
  for (int i = 0; i < n_cols; i++) {
    want_d[(size_t)i] = cols[i].max_def > 0 && (staged || cols[i].def_levels);
    want_r[(size_t)i] = cols[i].max_rep > 0 && (staged || cols[i].rep_levels);
  }
  uint64_t total = 0;
  int rc = PQG_OK;
  pqg_status st2;
  for (int attempt = 0; attempt < 2; attempt++) {
    // device layout of outputs: per column values | def | rep | binary bytes, 256-B aligned
    total = 0;
    for (int i = 0; i < n_cols; i++) {
      const bool bin = bin_out(cols[i]);
      int w = out_width(cols[i]);
      if (w <= 0) w = 8;
      off_v[(size_t)i] = total;
      total = al(total + (slots[(size_t)i] + (bin ? 1 : 0)) * (uint64_t)w);
      off_d[(size_t)i] = total;
      if (want_d[(size_t)i]) total = al(total + slots[(size_t)i]);
      off_r[(size_t)i] = total;
      if (want_r[(size_t)i]) total = al(total + slots[(size_t)i]);
      off_b[(size_t)i] = total;
      if (bin) total = al(total + bin_cap[(size_t)i]);
    }
    if (ctx->host_out.ensure(total + 256) != hipSuccess || ctx->pin_out.ensure(total + 256) != hipSuccess) {
      set_status(st, PQG_ERR_HIP, -1, -1, "device buffers");
      return PQG_ERR_HIP;
    }
    uint8_t* dout = (uint8_t*)ctx->host_out.p;
    for (int i = 0; i < n_cols; i++) {
      const bool bin = bin_out(cols[i]);
      dcols[(size_t)i].values = dout + off_v[(size_t)i];
      dcols[(size_t)i].values_capacity = slots[(size_t)i] + (bin ? 1 : 0);
      dcols[(size_t)i].def_levels = want_d[(size_t)i] ? dout + off_d[(size_t)i] : nullptr;
      dcols[(size_t)i].rep_levels = want_r[(size_t)i] ? dout + off_r[(size_t)i] : nullptr;
      dcols[(size_t)i].levels_capacity = slots[(size_t)i];
      dcols[(size_t)i].binary_data = bin ? dout + off_b[(size_t)i] : nullptr;
      dcols[(size_t)i].binary_capacity = bin_cap[(size_t)i];
    }
    // the zero padding is part of the readable range: loads are range-checked per dword against it, and
    // a page ending at an unaligned offset close to n_bytes (raw file bytes) needs its last dword whole
    rc = decode_impl(ctx, (const uint8_t*)ctx->host_bytes.p, n_bytes + pad, n_bytes, dcols.data(), n_cols, pages,
                     n_pages, (uint32_t*)ctx->host_counts.p, st);
    if (rc) return rc;
    rc = pqg_sync(ctx, &st2);
    if (rc != PQG_ERR_INVALID_ARG || st2.page != -1 || !ctx->last || attempt == 1) break;
    // binary capacity: size every BYTE_ARRAY column to the byte count the device produced
    bool grew = false;
    for (int i = 0; i < n_cols; i++) {
      const uint64_t o = ctx->last->L.bin_total_off[(size_t)i];
      if (o == ~0ull) continue;
      uint64_t t = 0;
      if (hipMemcpy(&t, (uint8_t*)ctx->last->buf[B_BSCRATCH].p + o, sizeof(t), hipMemcpyDeviceToHost) != hipSuccess) return PQG_ERR_HIP;
      if (t > bin_cap[(size_t)i]) { bin_cap[(size_t)i] = t; grew = true; }
    }
    if (!grew) break;
  }
  for (int i = 0; i < n_cols; i++) cols[i].values_written = dcols[(size_t)i].values_written;
  if (rc && st) *st = st2;
  phase("h2d+decode");
  // device -> pinned -> host arrays (decoded values are valid up to the first error): the D2H goes
  // in HOST_CHUNK pieces, each followed by an event; worker threads copy the fixed-width values
  // and levels out of each piece as it lands
  uint8_t* dout = (uint8_t*)ctx->host_out.p;
  const uint8_t* po = (const uint8_t*)ctx->pin_out.p;
  std::vector<HostCopy> jobs;
  for (int i = 0; i < n_cols && !staged; i++) {
    const int w = out_width(cols[i]);
    const uint64_t n = std::min<uint64_t>(cols[i].values_written, cols[i].values_capacity);
    if (!bin_out(cols[i]) && cols[i].values && n)
      jobs.push_back({(uint8_t*)cols[i].values, off_v[(size_t)i], n * (uint64_t)w});
    if (cols[i].max_def > 0 && cols[i].def_levels)
      jobs.push_back({cols[i].def_levels, off_d[(size_t)i], std::min(slots[(size_t)i], cols[i].levels_capacity)});
    if (cols[i].max_rep > 0 && cols[i].rep_levels)
      jobs.push_back({cols[i].rep_levels, off_r[(size_t)i], std::min(slots[(size_t)i], cols[i].levels_capacity)});
  }
  const uint64_t n_chunks = (total + HOST_CHUNK - 1) / HOST_CHUNK;
  std::vector<hipEvent_t> ev((size_t)n_chunks, nullptr);
  bool ok = true;
  // odd chunks on a second stream (a second DMA queue), after the decode
  hipStream_t s2 = s;
  hipEvent_t dec_done = nullptr;
  if (n_chunks > 1) {
    if (!ctx->copy_stream && hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking) != hipSuccess)
      ctx->copy_stream = nullptr;
    if (ctx->copy_stream && hipEventCreateWithFlags(&dec_done, hipEventDisableTiming) == hipSuccess &&
        hipEventRecord(dec_done, s) == hipSuccess && hipStreamWaitEvent(ctx->copy_stream, dec_done, 0) == hipSuccess)
      s2 = ctx->copy_stream;
  }
  // The copy threads start first and take each piece once it is queued and its event has completed:
  // hipMemcpyAsync into pinned memory measured blocking here (its events had all completed when the
  // threads started, r05w), so a queue-then-copy order ran the host copies after the whole D2H.
  std::vector<std::atomic<int>> queued((size_t)n_chunks);
  for (auto& q : queued) q.store(0, std::memory_order_relaxed);
  const int T = std::max(1, std::min<int>(host_threads(total), (int)n_chunks));
  std::vector<int> wok((size_t)T, 1);
  std::vector<std::thread> th;
  std::vector<double> t_dma((size_t)n_chunks, 0.0);  // (PQG_HOST_TIMING: when each piece was seen landed)
  const auto t_d0 = std::chrono::steady_clock::now();
  for (int t = 0; t < T && !staged; t++)
    th.emplace_back([&, t] {
      if (hipSetDevice(ctx->device) != hipSuccess) { wok[(size_t)t] = 0; return; }
      for (uint64_t k = (uint64_t)t; k < n_chunks; k += (uint64_t)T) {
        int q;
        while ((q = queued[(size_t)k].load(std::memory_order_acquire)) == 0) std::this_thread::yield();
        if (q < 0 || hipEventSynchronize(ev[(size_t)k]) != hipSuccess) { wok[(size_t)t] = 0; return; }
        if (timing) t_dma[(size_t)k] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_d0).count();
        copy_range(jobs, po, k * HOST_CHUNK, std::min(total, (k + 1) * HOST_CHUNK));
      }
    });
  for (uint64_t k = 0; k < n_chunks; k++) {
    const uint64_t a = k * HOST_CHUNK, len = std::min(HOST_CHUNK, total - a);
    hipStream_t sk = (k & 1) ? s2 : s;
    ok = ok && hipMemcpyAsync((uint8_t*)ctx->pin_out.p + a, dout + a, len, hipMemcpyDeviceToHost, sk) == hipSuccess &&
         hipEventCreateWithFlags(&ev[(size_t)k], hipEventDisableTiming) == hipSuccess &&
         hipEventRecord(ev[(size_t)k], sk) == hipSuccess;
    queued[(size_t)k].store(ok ? 1 : -1, std::memory_order_release);  // (-1: the threads stop)
  }
  std::vector<uint32_t> counts((size_t)std::max(n_pages, 1));
  if (ok && n_pages)
    ok = hipMemcpyAsync(counts.data(), ctx->host_counts.p, sizeof(uint32_t) * (size_t)n_pages, hipMemcpyDeviceToHost, s) == hipSuccess;
  for (auto& x : th) x.join();
  for (int v : wok) ok = ok && v;
  if (timing && n_chunks && !staged)
    std::fprintf(stderr, "pqg_decode_host   last D2H piece seen landed %.3f ms after the copy threads started (%d threads)\n",
                 *std::max_element(t_dma.begin(), t_dma.end()), T);
  if (s2 != s && hipStreamSynchronize(s2) != hipSuccess) ok = false;
  for (hipEvent_t e : ev)
    if (e) (void)hipEventDestroy(e);
  if (dec_done) (void)hipEventDestroy(dec_done);
  if (!ok || hipStreamSynchronize(s) != hipSuccess) return PQG_ERR_HIP;
  phase("d2h+copy");
  if (staged) {
    // outputs stay in pin_out: describe them (pqg_staged_column)
    ctx->staged.resize(nc);
    for (int i = 0; i < n_cols; i++) {
      pqg_staged_output& o = ctx->staged[(size_t)i];
      o.values = po + off_v[(size_t)i];
      o.def_levels = want_d[(size_t)i] ? po + off_d[(size_t)i] : nullptr;
      o.rep_levels = want_r[(size_t)i] ? po + off_r[(size_t)i] : nullptr;
      o.n_values = std::min<uint64_t>(cols[i].values_written, slots[(size_t)i]);
      o.n_slots = slots[(size_t)i];
      o.binary = nullptr;
      o.n_binary = 0;
      if (bin_out(cols[i])) {
        const uint64_t nb = (uint64_t)((const int64_t*)o.values)[o.n_values];
        if (nb > bin_cap[(size_t)i]) {  // the device's count did not fit even after the resize
          if (rc == PQG_OK) {
            rc = PQG_ERR_INVALID_ARG;
            set_status(st, rc, -1, (int64_t)nb, "binary capacity");
          }
        } else {
          o.binary = po + off_b[(size_t)i];
          o.n_binary = nb;
        }
      }
    }
    if (h_page_value_counts && n_pages) std::memcpy(h_page_value_counts, counts.data(), sizeof(uint32_t) * (size_t)n_pages);
    return rc;
  }
  for (int i = 0; i < n_cols; i++) {
    if (!bin_out(cols[i])) continue;
    // offsets[n + 1] and the bytes they span
    const uint64_t n = std::min<uint64_t>(cols[i].values_written, cols[i].values_capacity ? cols[i].values_capacity - 1 : 0);
    const int64_t* offs = (const int64_t*)(po + off_v[(size_t)i]);
    if (cols[i].values && cols[i].values_capacity) par_memcpy(cols[i].values, offs, (n + 1) * sizeof(int64_t));
    const uint64_t nb = (uint64_t)offs[n];
    if (nb > cols[i].binary_capacity) {
      if (rc == PQG_OK) {
        rc = PQG_ERR_INVALID_ARG;
        if (st) {
          st->code = rc;
          st->page = -1;
          st->value_index = (int64_t)nb;
          std::snprintf(st->message, sizeof(st->message), "binary capacity: column %d needs %llu bytes", i,
                        (unsigned long long)nb);
        }
      }
    } else if (cols[i].binary_data && nb) {
      par_memcpy(cols[i].binary_data, po + off_b[(size_t)i], nb);
    }
  }
  if (h_page_value_counts && n_pages) std::memcpy(h_page_value_counts, counts.data(), sizeof(uint32_t) * (size_t)n_pages);
  phase("binary");
  return rc;
}

int pqg_decode_host(pqg_ctx* ctx, const uint8_t* h_bytes, uint64_t n_bytes, pqg_column_desc* cols, int n_cols,
                    const pqg_page_desc* pages, int n_pages, uint32_t* h_page_value_counts, pqg_status* st) {
  static const uint8_t empty = 0;
  if (n_bytes && !h_bytes) {
    if (st) { std::memset(st, 0, sizeof(*st)); st->page = -1; }
    return PQG_ERR_INVALID_ARG;
  }
  return host_path(ctx, h_bytes ? h_bytes : &empty, n_bytes, cols, n_cols, pages, n_pages, h_page_value_counts, st);
}

int pqg_host_input(pqg_ctx* ctx, uint64_t n_bytes, uint8_t** buf) {
  if (!ctx || !buf) return PQG_ERR_INVALID_ARG;
  *buf = nullptr;
  if (hipSetDevice(ctx->device) != hipSuccess) return PQG_ERR_HIP;
  // the decode pads with 1,024 zero bytes after n_bytes (host_path's `pad`)
  if (ctx->pin_in.ensure(n_bytes + 1024) != hipSuccess) return PQG_ERR_HIP;
  ctx->staged.clear();
  *buf = (uint8_t*)ctx->pin_in.p;
  return PQG_OK;
}

int pqg_decode_staged(pqg_ctx* ctx, uint64_t n_bytes, pqg_column_desc* cols, int n_cols, const pqg_page_desc* pages,
                      int n_pages, uint32_t* h_page_value_counts, pqg_status* st) {
  return host_path(ctx, nullptr, n_bytes, cols, n_cols, pages, n_pages, h_page_value_counts, st);
}

int pqg_staged_column(pqg_ctx* ctx, int col, pqg_staged_output* out) {
  if (!ctx || !out || col < 0 || (size_t)col >= ctx->staged.size()) return PQG_ERR_INVALID_ARG;
  *out = ctx->staged[(size_t)col];
  return PQG_OK;
}

void pqg_copy_out(void* dst, const void* src, uint64_t n) {
  if (n && dst && src) par_memcpy(dst, src, n);
}

int pqg_assemble(pqg_ctx* ctx, const uint8_t* d_def_levels, const uint8_t* d_rep_levels, uint64_t n_slots,
                 pqg_assembly_node* path, int depth, uint64_t* n_records, pqg_status* st) {
  if (st) { std::memset(st, 0, sizeof(*st)); st->page = -1; }
  if (!ctx || !path || depth <= 0 || depth > (int)pqg::ASM_MAX_NODES) {
    set_status(st, PQG_ERR_INVALID_ARG, -1, -1, "assembly arguments");
    return PQG_ERR_INVALID_ARG;
  }
  // levels of every node (ColumnIO repetition / definition level)
  pqg::AsmParams P;
  std::memset(&P, 0, sizeof(P));
  P.n_nodes = (uint32_t)depth;
  uint32_t r = 0, d = 0;
  for (int k = 0; k < depth; k++) {
    const int rp = path[k].repetition;
    if (rp != PQG_REQUIRED && rp != PQG_OPTIONAL && rp != PQG_REPEATED) {
      set_status(st, PQG_ERR_INVALID_ARG, -1, k, "assembly node repetition");
      return PQG_ERR_INVALID_ARG;
    }
    if (rp == PQG_REPEATED) {
      r++;
      d++;
      if (r >= pqg::ASM_MAX_DEPTHS) {
        set_status(st, PQG_ERR_UNSUPPORTED, -1, k, "assembly: more than 7 repetition levels");
        return PQG_ERR_UNSUPPORTED;
      }
      P.DR[r] = d;
    } else if (rp == PQG_OPTIONAL) {
      d++;
    }
    P.kind[k] = rp;
    P.depth[k] = r;
    P.D[k] = d;
    P.validity[k] = rp == PQG_OPTIONAL ? path[k].validity : nullptr;
    P.offsets[k] = rp == PQG_REPEATED ? path[k].offsets : nullptr;
  }
  P.max_rep = r;
  if (d > 254) {
    set_status(st, PQG_ERR_UNSUPPORTED, -1, -1, "assembly: definition level above 254");
    return PQG_ERR_UNSUPPORTED;
  }
  if (n_slots && ((d > 0 && !d_def_levels) || (r > 0 && !d_rep_levels))) {
    set_status(st, PQG_ERR_INVALID_ARG, -1, -1, "assembly levels");
    return PQG_ERR_INVALID_ARG;
  }
  if (hipSetDevice(ctx->device) != hipSuccess) return PQG_ERR_HIP;
  hipStream_t s = ctx->stream;
  const uint32_t n_blocks = (uint32_t)((n_slots + 4095) / 4096);
  const size_t cnt_bytes = sizeof(uint64_t) * pqg::ASM_MAX_DEPTHS * (size_t)std::max<uint32_t>(n_blocks, 1);
  if (ctx->asm_scratch.ensure(cnt_bytes + 256) != hipSuccess || ctx->pin_err.ensure(256) != hipSuccess) return PQG_ERR_HIP;
  uint64_t* counts = (uint64_t*)ctx->asm_scratch.p;  // block counts (count pass) / look-back status words
  uint64_t* totals = (uint64_t*)((uint8_t*)ctx->asm_scratch.p + cnt_bytes);
  uint32_t* ticket = (uint32_t*)(totals + pqg::ASM_MAX_DEPTHS);
  bool any_out = false, bounded = true;
  for (int k = 0; k < depth; k++) {
    any_out = any_out || P.validity[k] || P.offsets[k];
    // entries of any depth <= n_slots: outputs sized for that bound need no count round trip
    if ((P.validity[k] && path[k].capacity < n_slots) || (P.offsets[k] && path[k].capacity < n_slots + 1)) bounded = false;
  }
  const uint8_t* dl = d > 0 ? d_def_levels : nullptr;
  const uint8_t* rl = r > 0 ? d_rep_levels : nullptr;
  // the single pass: status words, totals and the ticket zeroed, then one kernel (outputs + totals)
  auto emit = [&]() -> hipError_t {
    hipError_t e2 = hipMemsetAsync(ctx->asm_scratch.p, 0, cnt_bytes + sizeof(uint64_t) * pqg::ASM_TOTAL_WORDS, s);
    if (e2 == hipSuccess) e2 = pqg::launch_assemble(s, dl, rl, n_slots, P, counts, n_blocks, totals, ticket, 1);
    if (e2 == hipSuccess && n_blocks == 0)  // no slots: closing offsets only (offsets[0] = 0)
      for (int k = 0; k < depth && e2 == hipSuccess; k++)
        if (P.kind[k] == PQG_REPEATED && P.offsets[k]) e2 = hipMemsetAsync(P.offsets[k], 0, sizeof(int64_t), s);
    return e2;
  };
  const bool one_pass = any_out && bounded;
  hipError_t e = one_pass ? emit() : pqg::launch_assemble(s, dl, rl, n_slots, P, counts, n_blocks, totals, ticket, 0);
  uint64_t* h_tot = (uint64_t*)ctx->pin_err.p;
  if (e == hipSuccess) e = hipMemcpyAsync(h_tot, totals, sizeof(uint64_t) * pqg::ASM_TOTAL_WORDS, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) {
    set_status(st, PQG_ERR_HIP, -1, -1, hipGetErrorString(e));
    return PQG_ERR_HIP;
  }
  // a look-back wait timed out (k_asm_onepass; the count pass leaves the flag word as it was)
  if (one_pass && h_tot[pqg::ASM_TIMEOUT_WORD] == ~0ull) {
    set_status(st, PQG_ERR_TIMEOUT, -1, -1, "assembly look-back");
    return PQG_ERR_TIMEOUT;
  }
  if (n_records) *n_records = h_tot[0];
  int bad = -1;
  for (int k = 0; k < depth; k++) {
    path[k].n_entries = h_tot[P.depth[k]];
    uint64_t need = 0;
    if (P.kind[k] == PQG_OPTIONAL && P.validity[k]) need = h_tot[P.depth[k]];
    if (P.kind[k] == PQG_REPEATED && P.offsets[k]) need = h_tot[P.depth[k] - 1] + 1;
    if (need > path[k].capacity && bad < 0) bad = k;
  }
  if (bad >= 0) {
    set_status(st, PQG_ERR_INVALID_ARG, -1, bad, "assembly output capacity");
    return PQG_ERR_INVALID_ARG;
  }
  if (!any_out || one_pass) return PQG_OK;  // counts only, or already emitted
  e = emit();
  if (e == hipSuccess)
    e = hipMemcpyAsync(h_tot + pqg::ASM_TIMEOUT_WORD, totals + pqg::ASM_TIMEOUT_WORD, sizeof(uint64_t), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) {
    set_status(st, PQG_ERR_HIP, -1, -1, hipGetErrorString(e));
    return PQG_ERR_HIP;
  }
  if (h_tot[pqg::ASM_TIMEOUT_WORD] == ~0ull) {
    set_status(st, PQG_ERR_TIMEOUT, -1, -1, "assembly look-back");
    return PQG_ERR_TIMEOUT;
  }
  return PQG_OK;
}

int pqg_assemble_schema(pqg_ctx* ctx, pqg_schema_node* nodes, int n_nodes, const pqg_schema_leaf* leaves, int n_leaves,
                        uint64_t* n_records, pqg_status* st) {
  if (st) { std::memset(st, 0, sizeof(*st)); st->page = -1; }
  if (!ctx || !nodes || n_nodes <= 0 || (n_leaves > 0 && !leaves) || n_leaves < 0) {
    set_status(st, PQG_ERR_INVALID_ARG, -1, -1, "schema assembly arguments");
    return PQG_ERR_INVALID_ARG;
  }
  for (int k = 0; k < n_nodes; k++)
    if (nodes[k].parent >= k || nodes[k].parent < -1) {
      set_status(st, PQG_ERR_INVALID_ARG, -1, k, "schema node parent");
      return PQG_ERR_INVALID_ARG;
    }
  std::vector<int> owner((size_t)n_nodes, -1);  // leaf whose pass wrote the node's outputs
  uint64_t records = 0;
  for (int li = 0; li < n_leaves; li++) {
    const pqg_schema_leaf& lf = leaves[li];
    if (lf.node < 0 || lf.node >= n_nodes) {
      set_status(st, PQG_ERR_INVALID_ARG, li, -1, "schema leaf node");
      return PQG_ERR_INVALID_ARG;
    }
    for (int k = 0; k < n_nodes; k++)
      if (nodes[k].parent == lf.node) {
        set_status(st, PQG_ERR_INVALID_ARG, li, k, "schema leaf has children");
        return PQG_ERR_INVALID_ARG;
      }
    // the leaf's path: root's child .. leaf
    std::vector<int> chain;
    for (int k = lf.node; k >= 0; k = nodes[k].parent) chain.push_back(k);
    std::reverse(chain.begin(), chain.end());
    if (chain.size() > pqg::ASM_MAX_NODES) {
      set_status(st, PQG_ERR_UNSUPPORTED, li, -1, "schema assembly: path too deep");
      return PQG_ERR_UNSUPPORTED;
    }
    std::vector<pqg_assembly_node> path(chain.size());
    for (size_t q = 0; q < chain.size(); q++) {
      const pqg_schema_node& n = nodes[chain[q]];
      pqg_assembly_node& a = path[q];
      std::memset(&a, 0, sizeof(a));
      a.repetition = n.repetition;
      if (owner[(size_t)chain[q]] < 0) {  // first leaf under this node: it writes the outputs
        a.validity = n.validity;
        a.offsets = n.offsets;
        a.capacity = n.capacity;
      }
    }
    uint64_t nrec = 0;
    const int rc = pqg_assemble(ctx, lf.d_def_levels, lf.d_rep_levels, lf.n_slots, path.data(), (int)path.size(), &nrec, st);
    if (rc) {
      if (st) st->page = li;
      if (st && rc == PQG_ERR_INVALID_ARG && st->value_index >= 0 && st->value_index < (int64_t)chain.size())
        st->value_index = chain[(size_t)st->value_index];  // path position -> node index
      return rc;
    }
    if (li > 0 && nrec != records) {
      set_status(st, PQG_ERR_CORRUPT, li, -1, "schema assembly: leaves disagree on the record count");
      return PQG_ERR_CORRUPT;
    }
    records = nrec;
    for (size_t q = 0; q < chain.size(); q++) {
      const int k = chain[q];
      if (owner[(size_t)k] < 0) {
        owner[(size_t)k] = li;
        nodes[k].n_entries = path[q].n_entries;
      } else if (nodes[k].n_entries != path[q].n_entries) {
        set_status(st, PQG_ERR_CORRUPT, li, k, "schema assembly: leaves disagree on a node's entries");
        return PQG_ERR_CORRUPT;
      }
    }
  }
  if (n_records) *n_records = records;
  return PQG_OK;
}

int pqg_unpack_runs(pqg_ctx* ctx, int bit_width, const uint8_t* d_in, const uint64_t* d_in_offsets,
                    const uint32_t* d_counts, const uint64_t* d_out_offsets, int32_t* d_out, int n_runs) {
  if (!ctx || bit_width < 0 || bit_width > 32 || n_runs < 0) return PQG_ERR_INVALID_ARG;
  if (n_runs == 0) return PQG_OK;
  if (!d_in || !d_in_offsets || !d_counts || !d_out_offsets || !d_out) return PQG_ERR_INVALID_ARG;
  if (hipSetDevice(ctx->device) != hipSuccess) return PQG_ERR_HIP;
  // the kernel grid-strides inside each run; 64 blocks x 256 lanes per run
  hipError_t e = pqg::launch_unpack_runs(ctx->stream, bit_width, d_in, ~0ull >> 1, d_in_offsets, d_counts, d_out_offsets,
                                         d_out, n_runs, 1u << 14);
  return e == hipSuccess ? PQG_OK : PQG_ERR_HIP;
}

// ---- record filter (pqgpu_filter_host.cpp builds the filter, pqgpu_filter.hip runs it) -----------
static_assert(sizeof(pqg_filter_node) == 32 && sizeof(pqg_filter_column) == 40 && sizeof(pqg_filter_result) == 16,
              "filter ABI layout");

static_assert(sizeof(pqg_filter_dictionary) == 24, "filter dictionary ABI layout");
static_assert(sizeof(pqg_filter_record_column) == 64, "filter record column ABI layout");
static_assert(sizeof(pqg_filter_column_type) == 16, "filter column type ABI layout");

// The launches of pqg_filter_run / pqg_filter_run_dict once pqg::filter_bind has accepted the columns, and
// with `rec` (whose dt is `dt`) those of pqg_filter_run_records with contains leaves.
static int filter_launch(pqg_ctx* ctx, const pqg_filter* filter, const pqg::FilterCols& fc, const pqg::FilterDictTab* dt,
                         uint64_t n_rows, uint64_t* d_bitmap, int64_t* d_row_ids, uint64_t row_ids_capacity,
                         pqg_filter_result* d_result, pqg::FilterRecDev* rec = nullptr) {
  if (hipSetDevice(ctx->device) != hipSuccess) return PQG_ERR_HIP;
  const uint64_t dict_words = dt ? PQG_FILTER_MAX_NODES + dt->table_words : 0;
  const uint64_t scratch_words =
      rec ? pqg::filter_records_scratch_words(n_rows, fc.n_nullable, dict_words, rec->rt.n_leaves, rec->rt.n_rep,
                                              rec->rt.max_slots)
          : pqg::filter_scratch_words(n_rows, fc.n_nullable, dict_words);
  if (ctx->filter_scratch.ensure(8 * (size_t)scratch_words) != hipSuccess) return PQG_ERR_HIP;
  if (rec) rec->rt.bitmaps = pqg::filter_records_bitmaps((uint64_t*)ctx->filter_scratch.p, n_rows, fc.n_nullable, dict_words);
  if (ctx->filter_serial != filter->serial) {
    if (ctx->filter_image.ensure(filter->image.size()) != hipSuccess) return PQG_ERR_HIP;
    ctx->filter_serial = 0;
    if (hipMemcpyAsync(ctx->filter_image.p, filter->image.data(), filter->image.size(), hipMemcpyHostToDevice,
                       ctx->stream) != hipSuccess)
      return PQG_ERR_HIP;
    ctx->filter_serial = filter->serial;
  }
  if (dt) {
    // the dictionary table goes up like pqg_take's column table: through a pinned slot that is reused
    // once the copy out of it has run
    constexpr size_t slot_bytes = sizeof(pqg::FilterRecDev);  // a FilterDictTab, or the FilterRecDev it begins
    const size_t tab_bytes = rec ? sizeof(pqg::FilterRecDev) : sizeof(pqg::FilterDictTab);
    if (ctx->filter_dict.ensure(slot_bytes) != hipSuccess || ctx->filter_dict_pin.ensure(slot_bytes * pqg_ctx::TAKE_SLOTS) != hipSuccess)
      return PQG_ERR_HIP;
    const uint32_t slot = ctx->filter_dict_seq++ % pqg_ctx::TAKE_SLOTS;
    hipEvent_t& ev = ctx->filter_dict_ev[slot];
    if (!ev) {
      if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) return PQG_ERR_HIP;
    } else if (hipEventSynchronize(ev) != hipSuccess) {
      return PQG_ERR_HIP;
    }
    void* pin = (uint8_t*)ctx->filter_dict_pin.p + slot * slot_bytes;
    std::memcpy(pin, rec ? (const void*)rec : (const void*)dt, tab_bytes);
    if (hipMemcpyAsync(ctx->filter_dict.p, pin, tab_bytes, hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
        hipEventRecord(ev, ctx->stream) != hipSuccess)
      return PQG_ERR_HIP;
  }
  if (rec) {
    const hipError_t e = pqg::launch_filter_records(
        ctx->stream, (const uint8_t*)ctx->filter_image.p, (uint32_t)filter->image.size(), fc, n_rows,
        (uint64_t*)ctx->filter_scratch.p, d_bitmap, d_row_ids, row_ids_capacity, d_result,
        (const pqg::FilterRecDev*)ctx->filter_dict.p, rec, filter->binary_paths);
    return e == hipSuccess ? PQG_OK : PQG_ERR_HIP;
  }
  const hipError_t e =
      pqg::launch_filter(ctx->stream, (const uint8_t*)ctx->filter_image.p, (uint32_t)filter->image.size(), fc, n_rows,
                         (uint64_t*)ctx->filter_scratch.p, d_bitmap, d_row_ids, row_ids_capacity, d_result,
                         dt ? (const pqg::FilterDictTab*)ctx->filter_dict.p : nullptr, dt, filter->binary_paths);
  return e == hipSuccess ? PQG_OK : PQG_ERR_HIP;
}

int pqg_filter_run(pqg_ctx* ctx, const pqg_filter* filter, const pqg_filter_column* cols, int n_cols, uint64_t n_rows,
                   uint64_t* d_bitmap, int64_t* d_row_ids, uint64_t row_ids_capacity, pqg_filter_result* d_result) {
  if (!ctx || !filter || !d_result) return PQG_ERR_INVALID_ARG;
  if (n_rows && !d_bitmap) return PQG_ERR_INVALID_ARG;
  pqg::FilterCols fc;
  const int rc = pqg::filter_bind(filter, cols, nullptr, n_cols, n_rows, &fc, nullptr, nullptr);
  if (rc != PQG_OK) return rc;
  return filter_launch(ctx, filter, fc, nullptr, n_rows, d_bitmap, d_row_ids, row_ids_capacity, d_result);
}

int pqg_filter_run_dict(pqg_ctx* ctx, const pqg_filter* filter, const pqg_filter_column* cols,
                        const pqg_filter_dictionary* dicts, int n_cols, uint64_t n_rows, uint64_t* d_bitmap,
                        int64_t* d_row_ids, uint64_t row_ids_capacity, pqg_filter_result* d_result) {
  if (!ctx || !filter || !d_result) return PQG_ERR_INVALID_ARG;
  if (n_rows && !d_bitmap) return PQG_ERR_INVALID_ARG;
  pqg::FilterCols fc;
  pqg::FilterDictTab dt;
  bool any_dict = false;
  const int rc = pqg::filter_bind(filter, cols, dicts, n_cols, n_rows, &fc, &dt, &any_dict);
  if (rc != PQG_OK) return rc;
  return filter_launch(ctx, filter, fc, any_dict ? &dt : nullptr, n_rows, d_bitmap, d_row_ids, row_ids_capacity, d_result);
}

int pqg_filter_run_records(pqg_ctx* ctx, const pqg_filter* filter, const pqg_filter_record_column* cols,
                           const pqg_filter_dictionary* dicts, int n_cols, uint64_t n_rows, uint64_t* d_bitmap,
                           int64_t* d_row_ids, uint64_t row_ids_capacity, pqg_filter_result* d_result) {
  if (!ctx || !filter || !d_result) return PQG_ERR_INVALID_ARG;
  if (n_rows && !d_bitmap) return PQG_ERR_INVALID_ARG;
  pqg::FilterCols fc;
  pqg::FilterRecDev rec;
  bool any_dict = false;
  const int rc = pqg::filter_bind_records(filter, cols, dicts, n_cols, n_rows, &fc, &rec.dt, &any_dict, &rec.rt);
  if (rc != PQG_OK) return rc;
  // without a contains leaf every named column is flat: the launches of pqg_filter_run_dict as they are
  if (!rec.rt.n_leaves)
    return filter_launch(ctx, filter, fc, any_dict ? &rec.dt : nullptr, n_rows, d_bitmap, d_row_ids, row_ids_capacity,
                         d_result);
  return filter_launch(ctx, filter, fc, &rec.dt, n_rows, d_bitmap, d_row_ids, row_ids_capacity, d_result, &rec);
}

int pqg_decode_dictionary(pqg_ctx* ctx, const uint8_t* d_bytes, uint64_t n_bytes, pqg_column_desc* col, pqg_status* st) {
  if (st) { std::memset(st, 0, sizeof(*st)); st->page = -1; }
  if (!ctx || !col) return PQG_ERR_INVALID_ARG;
  int err = PQG_OK;
  const int ew = elem_width(col->physical_type, col->type_length);
  // the checks pqg_decode makes of a column's dictionary page, in its order (PlainValuesDictionary)
  if (col->dict_offset < 0) err = PQG_ERR_NO_DICTIONARY;
  else if (col->dict_encoding != PQG_PLAIN && col->dict_encoding != PQG_PLAIN_DICTIONARY) err = PQG_ERR_DICT_ENCODING;
  else if (col->physical_type == PQG_FIXED_LEN_BYTE_ARRAY && col->type_length <= 0) err = PQG_ERR_CORRUPT;
  else if ((uint64_t)col->dict_offset + col->dict_size > n_bytes) err = PQG_ERR_INVALID_ARG;
  else if (col->physical_type == PQG_BOOLEAN ? ((uint64_t)col->dict_num_values + 7) / 8 > col->dict_size
                                             : ew > 0 && (uint64_t)col->dict_num_values * (uint64_t)ew > col->dict_size)
    err = PQG_ERR_EOF;
  if (err) {
    set_status(st, err, -1, -1, "dictionary page");
    return err;
  }
  // a dictionary page is the PLAIN values of a required column: one V1 page of a one-column batch
  pqg_column_desc& d = ctx->dict_desc;
  d = *col;
  d.max_rep = d.max_def = 0;
  d.dict_offset = -1;
  d.dict_size = d.dict_num_values = 0;
  d.flags = 0;
  d.def_levels = d.rep_levels = nullptr;
  d.levels_capacity = 0;
  d.values_written = 0;
  pqg_page_desc g;
  std::memset(&g, 0, sizeof(g));
  g.offset = (uint64_t)col->dict_offset;
  g.size = col->dict_size;
  g.num_values = col->dict_num_values;
  g.column = 0;
  g.version = 1;
  g.encoding = PQG_PLAIN;
  g.rl_encoding = g.dl_encoding = PQG_RLE;
  const int rc = decode_impl(ctx, d_bytes, n_bytes, n_bytes, &d, 1, &g, 1, nullptr, st);
  if (rc == PQG_OK) ctx->dict_user = col;  // pqg_sync hands values_written on
  return rc;
}

// ---- row selection (pqgpu_take_host.cpp validates, pqgpu_take.hip runs) ---------------------------
static_assert(sizeof(pqg_take_column) == 88 && sizeof(pqg_take_counts) == 16 && sizeof(pqg_take_result) == 16,
              "take ABI layout");

int pqg_take(pqg_ctx* ctx, const uint64_t* d_bitmap, uint64_t n_rows, const pqg_take_column* cols, int n_cols,
             uint64_t out_rows_capacity, pqg_take_counts* d_counts, pqg_take_result* d_result) {
  pqg::TakeColDev tab[PQG_TAKE_MAX_COLUMNS];
  const int rc = pqg::take_validate(ctx != nullptr, d_bitmap, n_rows, cols, n_cols, out_rows_capacity, d_counts, d_result, tab);
  if (rc != PQG_OK) return rc;
  bool any_nullable = false, any_binary = false;
  for (int i = 0; i < n_cols; i++) {
    any_nullable |= tab[i].dl != nullptr;
    any_binary |= tab[i].kind == pqg::TAKE_BINARY;
  }
  if (hipSetDevice(ctx->device) != hipSuccess) return PQG_ERR_HIP;
  constexpr size_t slot_bytes = pqg_ctx::TAKE_SLOT_BYTES;
  static_assert(sizeof(tab) <= slot_bytes, "a pinned slot holds the table");
  if (ctx->take_scratch.ensure(8 * (size_t)pqg::take_scratch_words(n_rows, (uint32_t)n_cols)) != hipSuccess ||
      ctx->take_cols.ensure(slot_bytes) != hipSuccess || ctx->take_pin.ensure(slot_bytes * pqg_ctx::TAKE_SLOTS) != hipSuccess)
    return PQG_ERR_HIP;
  if (n_cols) {
    const uint32_t slot = ctx->take_seq++ % pqg_ctx::TAKE_SLOTS;
    hipEvent_t& ev = ctx->take_ev[slot];
    if (!ev) {
      if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) return PQG_ERR_HIP;
    } else if (hipEventSynchronize(ev) != hipSuccess) {  // the copy out of this slot TAKE_SLOTS calls ago
      return PQG_ERR_HIP;
    }
    void* pin = (uint8_t*)ctx->take_pin.p + slot * slot_bytes;
    std::memcpy(pin, tab, sizeof(pqg::TakeColDev) * (size_t)n_cols);
    if (hipMemcpyAsync(ctx->take_cols.p, pin, sizeof(pqg::TakeColDev) * (size_t)n_cols, hipMemcpyHostToDevice, ctx->stream) !=
            hipSuccess ||
        hipEventRecord(ev, ctx->stream) != hipSuccess)
      return PQG_ERR_HIP;
  }
  const hipError_t e = pqg::launch_take(ctx->stream, d_bitmap, n_rows, (const pqg::TakeColDev*)ctx->take_cols.p, (uint32_t)n_cols,
                                        any_nullable, any_binary, out_rows_capacity, (uint64_t*)ctx->take_scratch.p, d_counts,
                                        d_result, ctx->take_staged);
  return e == hipSuccess ? PQG_OK : PQG_ERR_HIP;
}

// ---- record selection on repeated columns --------------------------------------------------------
static_assert(sizeof(pqg_take_record_column) == 128 && sizeof(pqg_take_record_counts) == 32, "take_records ABI layout");

int pqg_take_records(pqg_ctx* ctx, const uint64_t* d_bitmap, uint64_t n_rows, const pqg_take_record_column* cols,
                     int n_cols, uint64_t out_rows_capacity, pqg_take_record_counts* d_counts,
                     pqg_take_result* d_result) {
  pqg::TakeRecDev tab[pqg::TAKE_REC_MAX_RECORDS];
  pqg::TakeRecPlan plan;
  const int rc = pqg::take_records_validate(ctx != nullptr, d_bitmap, n_rows, cols, n_cols, out_rows_capacity, d_counts,
                                            d_result, tab, &plan);
  if (rc != PQG_OK) return rc;
  if (hipSetDevice(ctx->device) != hipSuccess) return PQG_ERR_HIP;
  constexpr size_t slot_bytes = pqg_ctx::TAKE_SLOT_BYTES;
  static_assert(sizeof(tab) <= slot_bytes, "a pinned slot holds the table");
  const uint64_t words = pqg::take_records_scratch_words(plan.max_rows, (uint32_t)n_cols, plan.slot_words);
  if (ctx->take_scratch.ensure(8 * (size_t)words) != hipSuccess || ctx->take_cols.ensure(slot_bytes) != hipSuccess ||
      ctx->take_pin.ensure(slot_bytes * pqg_ctx::TAKE_SLOTS) != hipSuccess)
    return PQG_ERR_HIP;
  if (plan.n_records) {  // the table goes up through the pinned slots of pqg_take
    const uint32_t slot = ctx->take_seq++ % pqg_ctx::TAKE_SLOTS;
    hipEvent_t& ev = ctx->take_ev[slot];
    if (!ev) {
      if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) return PQG_ERR_HIP;
    } else if (hipEventSynchronize(ev) != hipSuccess) {
      return PQG_ERR_HIP;
    }
    void* pin = (uint8_t*)ctx->take_pin.p + slot * slot_bytes;
    std::memcpy(pin, tab, sizeof(pqg::TakeRecDev) * (size_t)plan.n_records);
    if (hipMemcpyAsync(ctx->take_cols.p, pin, sizeof(pqg::TakeRecDev) * (size_t)plan.n_records, hipMemcpyHostToDevice,
                       ctx->stream) != hipSuccess ||
        hipEventRecord(ev, ctx->stream) != hipSuccess)
      return PQG_ERR_HIP;
  }
  const hipError_t e = pqg::launch_take_records(ctx->stream, d_bitmap, n_rows, (const pqg::TakeRecDev*)ctx->take_cols.p,
                                                (uint32_t)n_cols, plan, out_rows_capacity, (uint64_t*)ctx->take_scratch.p,
                                                d_counts, d_result, ctx->take_staged);
  return e == hipSuccess ? PQG_OK : PQG_ERR_HIP;
}

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
  const uint32_t slot = ctx->crc_seq++ % pqg_ctx::CRC_SLOTS;
  hipEvent_t& ev = ctx->crc_ev[slot];
  if (!ev) {
    if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) return PQG_ERR_HIP;
  } else if (hipEventSynchronize(ev) != hipSuccess) {  // the fold of this slot CRC_SLOTS calls ago
    return PQG_ERR_HIP;
  }
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
  if (e != hipSuccess || hipEventRecord(ev, ctx->stream) != hipSuccess) return PQG_ERR_HIP;
  return PQG_OK;
}

int pqg_crc32_sync(pqg_ctx* ctx, const int32_t* d_status, int n_jobs, pqg_status* st) {
  if (!ctx || n_jobs < 0) return PQG_ERR_INVALID_ARG;
  if (hipStreamSynchronize(ctx->stream) != hipSuccess) return PQG_ERR_HIP;
  if (st) set_status(st, PQG_OK, -1, -1, "crc32");
  if (!d_status || n_jobs == 0) return PQG_OK;
  std::vector<int32_t> h((size_t)n_jobs);
  if (hipMemcpy(h.data(), d_status, sizeof(int32_t) * (size_t)n_jobs, hipMemcpyDeviceToHost) != hipSuccess)
    return PQG_ERR_HIP;
  for (int j = 0; j < n_jobs; j++)
    if (h[(size_t)j]) {
      set_status(st, h[(size_t)j], j, -1,
                 h[(size_t)j] == PQG_ERR_CRC ? "could not verify page integrity, CRC checksum verification failed" : "crc32 job");
      return h[(size_t)j];
    }
  return PQG_OK;
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
  if (!ctx || n_jobs < 0) return PQG_ERR_INVALID_ARG;
  if (hipStreamSynchronize(ctx->stream) != hipSuccess) return PQG_ERR_HIP;
  if (st) set_status(st, PQG_OK, -1, -1, "snappy");
  if (!d_status || n_jobs == 0) return PQG_OK;
  std::vector<int32_t> h((size_t)n_jobs);
  if (hipMemcpy(h.data(), d_status, sizeof(int32_t) * (size_t)n_jobs, hipMemcpyDeviceToHost) != hipSuccess)
    return PQG_ERR_HIP;
  for (int j = 0; j < n_jobs; j++)
    if (h[(size_t)j]) {
      set_status(st, h[(size_t)j], j, -1, "snappy block");
      return h[(size_t)j];
    }
  return PQG_OK;
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
  if (!ctx || n_jobs < 0) return PQG_ERR_INVALID_ARG;
  if (hipStreamSynchronize(ctx->stream) != hipSuccess) return PQG_ERR_HIP;
  if (st) set_status(st, PQG_OK, -1, -1, "lz4_raw");
  if (!d_status || n_jobs == 0) return PQG_OK;
  std::vector<int32_t> h((size_t)n_jobs);
  if (hipMemcpy(h.data(), d_status, sizeof(int32_t) * (size_t)n_jobs, hipMemcpyDeviceToHost) != hipSuccess)
    return PQG_ERR_HIP;
  for (int j = 0; j < n_jobs; j++)
    if (h[(size_t)j]) {
      set_status(st, h[(size_t)j], j, -1, "lz4_raw block");
      return h[(size_t)j];
    }
  return PQG_OK;
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
  if (!ctx || n_jobs < 0) return PQG_ERR_INVALID_ARG;
  if (hipStreamSynchronize(ctx->stream) != hipSuccess) return PQG_ERR_HIP;
  if (st) set_status(st, PQG_OK, -1, -1, "gzip");
  if (!d_status || n_jobs == 0) return PQG_OK;
  std::vector<int32_t> h((size_t)n_jobs);
  if (hipMemcpy(h.data(), d_status, sizeof(int32_t) * (size_t)n_jobs, hipMemcpyDeviceToHost) != hipSuccess)
    return PQG_ERR_HIP;
  for (int j = 0; j < n_jobs; j++)
    if (h[(size_t)j]) {
      set_status(st, h[(size_t)j], j, -1, "gzip block");
      return h[(size_t)j];
    }
  return PQG_OK;
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
  if (!ctx || n_jobs < 0) return PQG_ERR_INVALID_ARG;
  if (hipStreamSynchronize(ctx->stream) != hipSuccess) return PQG_ERR_HIP;
  if (st) set_status(st, PQG_OK, -1, -1, "zstd");
  if (!d_status || n_jobs == 0) return PQG_OK;
  std::vector<int32_t> h((size_t)n_jobs);
  if (hipMemcpy(h.data(), d_status, sizeof(int32_t) * (size_t)n_jobs, hipMemcpyDeviceToHost) != hipSuccess)
    return PQG_ERR_HIP;
  for (int j = 0; j < n_jobs; j++)
    if (h[(size_t)j]) {
      set_status(st, h[(size_t)j], j, -1, "zstd frame");
      return h[(size_t)j];
    }
  return PQG_OK;
}

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
  // every run's slice first (SingleBufferInputStream.slice throws before any unpack)
  uint64_t n_bytes = 0, n_vals = 0;
  uint32_t max_count = 0;
  for (int r = 0; r < n_runs; r++) {
    if (counts[r] % 8u != 0) return PQG_ERR_INVALID_ARG;
    const uint64_t need = (uint64_t)counts[r] * (uint64_t)bit_width / 8u;
    if (in_offsets[r] > in_len || need > in_len - in_offsets[r]) return PQG_ERR_EOF;
    if (need && !in) return PQG_ERR_INVALID_ARG;
    n_bytes += (need + 15) & ~uint64_t(15);
    n_vals += counts[r];
    max_count = std::max(max_count, counts[r]);
  }
  if (n_vals == 0) return PQG_OK;
  ctx->staged.clear();  // pin_in / pin_out are reused: an earlier staged decode's outputs are gone
  if (hipSetDevice(ctx->device) != hipSuccess) return PQG_ERR_HIP;
  hipStream_t s = ctx->stream;
  // pinned image: [run bytes, each 16-B aligned][in_off u64 x n][out_off u64 x n][counts u32 x n]
  auto al = [](uint64_t x) { return (x + 255) & ~uint64_t(255); };
  const uint64_t o_in = al(n_bytes + 16), o_out = o_in + 8ull * (uint64_t)n_runs, o_cnt = o_out + 8ull * (uint64_t)n_runs;
  const uint64_t img = al(o_cnt + 4ull * (uint64_t)n_runs);
  if (ctx->pin_in.ensure(img) != hipSuccess || ctx->pin_out.ensure(4 * n_vals) != hipSuccess ||
      ctx->host_runs.ensure(img + 4 * n_vals + 256) != hipSuccess)
    return PQG_ERR_HIP;
  uint8_t* pin = (uint8_t*)ctx->pin_in.p;
  uint64_t* pin_in_off = (uint64_t*)(pin + o_in);
  uint64_t* pin_out_off = (uint64_t*)(pin + o_out);
  uint32_t* pin_cnt = (uint32_t*)(pin + o_cnt);
  uint64_t b = 0, v = 0;
  for (int r = 0; r < n_runs; r++) {
    const uint64_t need = (uint64_t)counts[r] * (uint64_t)bit_width / 8u;
    if (need) std::memcpy(pin + b, in + in_offsets[r], need);
    const uint64_t padded = (need + 15) & ~uint64_t(15);
    std::memset(pin + b + need, 0, padded - need);
    pin_in_off[r] = b;
    pin_out_off[r] = v;
    pin_cnt[r] = counts[r];
    b += padded;
    v += counts[r];
  }
  std::memset(pin + n_bytes, 0, o_in - n_bytes);
  uint8_t* d = (uint8_t*)ctx->host_runs.p;
  int32_t* dout = (int32_t*)(d + img);
  if (hipMemcpyAsync(d, pin, img, hipMemcpyHostToDevice, s) != hipSuccess) return PQG_ERR_HIP;
  for (int r0 = 0; r0 < n_runs; r0 += 65535) {  // grid.y holds the run index
    const int nr = std::min(n_runs - r0, 65535);
    const hipError_t e = pqg::launch_unpack_runs(s, bit_width, d, n_bytes + 16, (const uint64_t*)(d + o_in) + r0,
                                                 (const uint32_t*)(d + o_cnt) + r0, (const uint64_t*)(d + o_out) + r0,
                                                 dout, nr, max_count);
    if (e != hipSuccess) return PQG_ERR_HIP;
  }
  if (hipMemcpyAsync(ctx->pin_out.p, dout, (size_t)(4 * n_vals), hipMemcpyDeviceToHost, s) != hipSuccess) return PQG_ERR_HIP;
  if (hipStreamSynchronize(s) != hipSuccess) return PQG_ERR_HIP;
  std::memcpy(out, ctx->pin_out.p, (size_t)(4 * n_vals));
  return PQG_OK;
}

}  // extern "C"

// ---- ParquetReadRouter.read with the page's runs cached --------------------------------------------

namespace {

// Bounds of one walk: what a miss decodes in its single round trip.
constexpr uint64_t ROUTER_MAX_VALUES = 1u << 22;
constexpr size_t ROUTER_MAX_RUNS = 1u << 16;

// Served from the cache when the run at this stream position (stream_left bytes before the end) was
// walked, with the same width and count, and its bytes are the ones unpacked then.
bool router_hit(RouterCache& c, int w, const uint8_t* in, uint64_t need, uint64_t stream_left, int count,
                int32_t* out) {
  if (c.w != w || stream_left > c.tail_len || c.off.empty()) return false;
  const uint64_t pos = c.tail_len - stream_left;
  const auto it = std::lower_bound(c.off.begin(), c.off.end(), pos);
  if (it == c.off.end() || *it != pos) return false;
  const size_t r = (size_t)(it - c.off.begin());
  if (c.cnt[r] != (uint32_t)count) return false;
  if (need && std::memcmp(in, c.bytes.data() + pos, need) != 0) return false;
  std::memcpy(out, c.vals.data() + c.vo[r], (size_t)count * 4);
  c.hits++;
  return true;
}

}  // namespace

extern "C" {

int pqg_router_cache_lookup(pqg_ctx* ctx, int bit_width, const uint8_t* run, size_t stream_left, int count,
                            int32_t* out, int* hit) {
  if (!ctx || !hit || bit_width < 0 || bit_width > 32 || count < 0 || count % 8 != 0 || (count && !out))
    return PQG_ERR_INVALID_ARG;
  *hit = 0;
  const uint64_t need = (uint64_t)count * (uint64_t)bit_width / 8u;
  if (need > stream_left) return PQG_ERR_EOF;
  if (need && !run) return PQG_ERR_INVALID_ARG;
  if (count == 0) {
    *hit = 1;
    return PQG_OK;
  }
  *hit = router_hit(ctx->router, bit_width, run, need, stream_left, count, out) ? 1 : 0;
  return PQG_OK;
}

int pqg_router_read_page(pqg_ctx* ctx, int bit_width, const uint8_t* in, size_t stream_left, int count, int32_t* out) {
  int hit = 0;
  const int lrc = pqg_router_cache_lookup(ctx, bit_width, in, stream_left, count, out, &hit);
  if (lrc != PQG_OK || hit) return lrc;
  if (!in) return PQG_ERR_INVALID_ARG;
  RouterCache& c = ctx->router;
  const uint64_t L = stream_left, need = (uint64_t)count * (uint64_t)bit_width / 8u;
  // Walk the hybrid stream after this run (RunLengthBitPackingHybridDecoder.readNext :80-109 header
  // forms; BytesUtils.readUnsignedVarInt :202-211) and list every bit-packed run whose bytes are in the
  // stream. The walk is a prediction of the caller's next reads: bytes past the hybrid stream (data the
  // caller reads otherwise) may parse as runs, which are decoded and never served; a header that cannot
  // be a run ends the walk. Runs the walk missed are served by a later miss.
  c.w = -1;
  c.off.clear();
  c.cnt.clear();
  c.vo.clear();
  c.off.push_back(0);
  c.cnt.push_back((uint32_t)count);
  c.vo.push_back(0);
  uint64_t total = (uint64_t)count, q = need;
  const uint32_t nb_rle = ((uint32_t)bit_width + 7u) / 8u;
  while (q < L && c.off.size() < ROUTER_MAX_RUNS) {
    uint32_t hdr = 0, sh = 0, b = 0;
    uint64_t k = q;
    bool ok = true;
    while (true) {
      if (k >= L || sh > 28) { ok = false; break; }
      b = in[k++];
      if (!(b & 0x80u)) break;
      hdr |= (b & 0x7Fu) << sh;
      sh += 7;
    }
    if (!ok) break;
    hdr |= b << sh;
    if (!(hdr & 1u)) {  // RLE run: count, then the value in ceil(w / 8) bytes
      q = k + nb_rle;
      continue;
    }
    const uint64_t groups = hdr >> 1, vals = groups * 8u, bytes = groups * (uint64_t)bit_width;
    if (vals > 0x7FFFFFF8u || k + bytes > L || total + vals > ROUTER_MAX_VALUES) break;
    if (vals) {
      c.off.push_back(k);
      c.cnt.push_back((uint32_t)vals);
      c.vo.push_back(total);
      total += vals;
    }
    q = k + bytes;
  }
  c.vals.resize(total);
  const uint64_t keep = c.off.size() > 1 ? c.off.back() + (uint64_t)c.cnt.back() * (uint64_t)bit_width / 8u : need;
  c.bytes.assign(in, in + keep);
  c.tail_len = L;
  c.misses++;
  const int rc = pqg_router_read_runs(ctx, bit_width, in, (size_t)L, c.off.data(), c.cnt.data(), (int)c.off.size(),
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

