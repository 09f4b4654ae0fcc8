// pqgpu_api.hip — the C ABI of include/pqgpu.h: contexts, plans (create / launch / destroy), pqg_sync with
// the re-runs and the error download, pqg_decode and pqg_decode_dictionary. The other entry points, by
// subsystem: pqgpu_api_hostpath.hip (pqg_decode_host / _staged and their staging copies),
// pqgpu_api_ops.hip (assembly, pqg_unpack_runs, record filters, take), pqgpu_api_codecs.hip (page
// checksums and the four decompressors), pqgpu_api_router.hip (pqg_router_*). pqgpu_ctx.h holds the
// context, the plan and the owners of their device resources.
//
// Host work that only computes goes to plain C++, where it is tested without a device: the planner
// (pqgpu_plan_host.cpp), error resolution and the router's stream walk (pqgpu_api_host.cpp), the
// validation of the filter, take and checksum calls (pqgpu_*_host.cpp). These files allocate, copy,
// launch and synchronise; every byte of page data is decoded by the kernels. There is no CPU decode
// fallback: without a usable HIP device every entry point returns PQG_ERR_NO_DEVICE.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstring>
#include <new>
#include <type_traits>
#include <vector>

#include "pqgpu_ctx.h"

using pqg::ColumnDev;
using pqg::PageWork;
using pqg::bin_out;
using pqg::elem_width;
// pqg::Cls
using pqg::C_DICT4; using pqg::C_DICT8; using pqg::C_IDS; using pqg::C_PLAIN; using pqg::C_BOOL; using pqg::C_DELTA4;
using pqg::C_DELTA8; using pqg::C_BSS; using pqg::C_BINP; using pqg::C_DLBA; using pqg::C_DBA; using pqg::C_RLEBOOL;
using pqg::C_DD; using pqg::C_DDG; using pqg::C_NCLS;

namespace {

const char* kNames[] = {"OK", "INVALID_ARG", "UNSUPPORTED", "HIP", "NO_DEVICE"};

template <class T>
PlanBufInit uploaded(PlanBuf b, const std::vector<T>& v, size_t min_elems) {
  return PlanBufInit{b, v.data(), sizeof(T) * v.size(), sizeof(T) * std::max(v.size(), min_elems), false};
}

}  // namespace

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
    case PQG_ERR_TAG: return "TAG";
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
  c->stream = hip_stream ? (hipStream_t)hip_stream : c->own_stream.get_or_create();
  if (!c->stream) {
    delete c;
    return PQG_ERR_HIP;
  }
  // one after the other, right after the main stream (pqg_ctx: round-robin placement on hardware queues)
  (void)c->side.stream.get_or_create();
  (void)c->bin.stream.get_or_create();
  (void)c->fix.stream.get_or_create();
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
    case PQG_DISPATCH_AES_TILE_BYTES:
      if (value < 0 || !pqg::aes_tile_ok((uint32_t)value)) return PQG_ERR_INVALID_ARG;
      ctx->aes_tile = (uint32_t)value;
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
  c->aes_wipe_keys(true);  // pqg_decrypt_pages' copies of the callers' keys, on the host and on the device
  delete c;
  return PQG_OK;
}

// Kernels one launch of the plan runs (in its current modes).
static int plan_kernels(const pqg_plan* P) {
  return pqg::plan_kernel_count(P->L, P->plain_fused, P->dict_fused, P->null_hints);
}

// valid_bytes: the caller's data ends there (page and dictionary extents are checked against it); the
// kernels may read up to n_bytes (pqg_decode_host's zero padding past the caller's bytes)
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
    dent_fork = ctx->dent_stream.get_or_create() && ctx->ev_dent_fork.get_or_create() && ctx->ev_dent.get_or_create() &&
                hipEventRecord(ctx->ev_dent_fork.e, s) == hipSuccess &&
                hipStreamWaitEvent(ctx->dent_stream.s, ctx->ev_dent_fork.e, 0) == hipSuccess;
    if (dent_fork) {
      e = launch_dent(ctx->dent_stream.s);
      if (e == hipSuccess && hipEventRecord(ctx->ev_dent.e, ctx->dent_stream.s) != hipSuccess) e = hipErrorUnknown;
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
  const bool ev_ok = want && ctx->ev_fork.get_or_create() && hipEventRecord(ctx->ev_fork.e, s) == hipSuccess;
  if (ev_ok && pf) fork = ctx->side.fork(ctx->ev_fork.e);
  if (ev_ok && has_bin && (has_fixed || hints)) fork_bin = ctx->bin.fork(ctx->ev_fork.e);
  if (ev_ok && (fork || fork_bin || hints) && has_fixed) fork_fix = ctx->fix.fork(ctx->ev_fork.e);
  if (e == hipSuccess && hints)  // the level sections, verified against the header counts, beside the value kernels
    e = pqg::launch_levels(s, P->d_bytes, P->n_bytes, work, cols, lists + P->L.levels_off, P->L.levels_n, err, ecount,
                           (uint32_t*)((uint8_t*)P->buf[B_BSCRATCH].p + P->L.hint_off));
  if (e == hipSuccess && pf) {  // PLAIN-only BYTE_ARRAY columns: one pass (after the levels: n_values, out_offset)
    uint8_t* scb = (uint8_t*)P->buf[B_BSCRATCH].p;
    uint64_t* ps = (uint64_t*)P->buf[B_PSTATUS].p;
    e = pqg::launch_bin_plain(fork ? ctx->side.stream.s : s, P->d_bytes, P->n_bytes, work, cols, (const int32_t*)P->buf[B_PCOL_PAGES].p,
                              (const int32_t*)P->buf[B_PCOL_START].p, P->L.n_pcols, (const uint64_t*)P->buf[B_PSEGS].p, P->L.n_psegs, ps,
                              ps + P->L.n_psegs, (uint32_t*)(scb + P->L.pticket_off), P->pseg_epoch,
                              (uint32_t*)(scb + P->L.pflag_off), P->err_epoch, err, ecount, P->L.plain_pg, P->L.n_pcp);
    if (fork && !ctx->side.record()) e = hipErrorUnknown;
  }
  const hipStream_t sb = fork_bin ? ctx->bin.stream.s : s;  // BYTE_ARRAY kernels of the other columns
  const hipStream_t sf = fork_fix ? ctx->fix.stream.s : s;  // fixed-width columns
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
                                g == 1 && dent_fork ? ctx->ev_dent.e : nullptr);
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
  // (the side queue's join event was recorded behind its one kernel)
  if (fork && !ctx->side.wait(s)) e = hipErrorUnknown;
  if (fork_bin && !ctx->bin.join(s)) e = hipErrorUnknown;
  if (fork_fix && !ctx->fix.join(s)) e = hipErrorUnknown;
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
  delete P;
  return PQG_OK;
}

}  // extern "C"

namespace {

// The first error of a launched plan in (page, value) order (pqg::resolve_page_errors), after the
// download of its error words; then the BYTE_ARRAY capacity check.
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
    pqg::decode_error_words(&errs, P->err_epoch);
  }
  int first = -1;
  int64_t index = -1;
  const char* what = "";
  const int rc = pqg::resolve_page_errors(P->L, errs, &P->page_errs, &first, &index, &what);
  if (rc) {
    set_status(st, rc, first, index, what);
    return rc;
  }
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
  if (rc == PQG_ERR_TIMEOUT && P->dict_fused && pqg::page_is_dict_class(P->L, tpage)) {
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
  if (rc == PQG_ERR_TIMEOUT && P->L.n_segs && P->seg_walk && pqg::page_is_binp(P->L, tpage2)) {
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
  return pqg::dict_page_eof_code(page.data(), page.size(), user.dict_num_values);
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
    // pqg_decode_dictionaries: page i is dictionary i
    const bool dict_batch = P == ctx->last && ctx->dicts_user && ctx->last_cols == ctx->dicts_desc.data();
    if (prc == PQG_ERR_EOF && dict_batch && pst.page >= 0 && pst.page < P->L.n_pages &&
        ctx->dicts_desc[(size_t)pst.page].physical_type == PQG_BYTE_ARRAY) {
      prc = dict_page_eof_code(P, ctx->dicts_user[pst.page]);
      set_status(&pst, prc, pst.page, pst.value_index, "dictionary page");
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
      if (dict_batch)
        for (int i = 0; i < P->L.n_cols; i++) ctx->dicts_user[i].values_written = ctx->dicts_desc[(size_t)i].values_written;
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

}  // extern "C"

int pqg::decode_impl(pqg_ctx* ctx, const uint8_t* d_bytes, uint64_t n_bytes, uint64_t valid_bytes, pqg_column_desc* cols,
                     int n_cols, const pqg_page_desc* pages, int n_pages, uint32_t* d_page_value_counts, pqg_status* st) {
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
  ctx->dicts_user = nullptr;
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

extern "C" {

int pqg_decode(pqg_ctx* ctx, const uint8_t* d_bytes, uint64_t n_bytes, pqg_column_desc* cols, int n_cols,
               const pqg_page_desc* pages, int n_pages, uint32_t* d_page_value_counts, pqg_status* st) {
  return pqg::decode_impl(ctx, d_bytes, n_bytes, n_bytes, cols, n_cols, pages, n_pages, d_page_value_counts, st);
}

// The checks pqg_decode makes of a column's dictionary page, in its order (PlainValuesDictionary).
static int dict_page_check(const pqg_column_desc& col, uint64_t n_bytes) {
  const int ew = elem_width(col.physical_type, col.type_length);
  if (col.dict_offset < 0) return PQG_ERR_NO_DICTIONARY;
  if (col.dict_encoding != PQG_PLAIN && col.dict_encoding != PQG_PLAIN_DICTIONARY) return PQG_ERR_DICT_ENCODING;
  if (col.physical_type == PQG_FIXED_LEN_BYTE_ARRAY && col.type_length <= 0) return PQG_ERR_CORRUPT;
  if ((uint64_t)col.dict_offset + col.dict_size > n_bytes) return PQG_ERR_INVALID_ARG;
  if (col.physical_type == PQG_BOOLEAN ? ((uint64_t)col.dict_num_values + 7) / 8 > col.dict_size
                                       : ew > 0 && (uint64_t)col.dict_num_values * (uint64_t)ew > col.dict_size)
    return PQG_ERR_EOF;
  return PQG_OK;
}

// A dictionary page is the PLAIN values of a required column: V1 page `g` of column `column` of a batch, whose
// descriptor `d` is the caller's without levels, flags and dictionary.
static void dict_page_as_column(const pqg_column_desc& col, int column, pqg_column_desc* d, pqg_page_desc* g) {
  *d = col;
  d->max_rep = d->max_def = 0;
  d->dict_offset = -1;
  d->dict_size = d->dict_num_values = 0;
  d->flags = 0;
  d->def_levels = d->rep_levels = nullptr;
  d->levels_capacity = 0;
  d->values_written = 0;
  std::memset(g, 0, sizeof(*g));
  g->offset = (uint64_t)col.dict_offset;
  g->size = col.dict_size;
  g->num_values = col.dict_num_values;
  g->column = column;
  g->version = 1;
  g->encoding = PQG_PLAIN;
  g->rl_encoding = g->dl_encoding = PQG_RLE;
}

int pqg_decode_dictionary(pqg_ctx* ctx, const uint8_t* d_bytes, uint64_t n_bytes, pqg_column_desc* col, pqg_status* st) {
  if (st) { std::memset(st, 0, sizeof(*st)); st->page = -1; }
  if (!ctx || !col) return PQG_ERR_INVALID_ARG;
  const int err = dict_page_check(*col, n_bytes);
  if (err) {
    set_status(st, err, -1, -1, "dictionary page");
    return err;
  }
  pqg_page_desc g;
  dict_page_as_column(*col, 0, &ctx->dict_desc, &g);
  const int rc = pqg::decode_impl(ctx, d_bytes, n_bytes, n_bytes, &ctx->dict_desc, 1, &g, 1, nullptr, st);
  if (rc == PQG_OK) ctx->dict_user = col;  // pqg_sync hands values_written on
  return rc;
}

int pqg_decode_dictionaries(pqg_ctx* ctx, const uint8_t* d_bytes, uint64_t n_bytes, pqg_column_desc* cols, int n,
                            pqg_status* st) {
  if (st) { std::memset(st, 0, sizeof(*st)); st->page = -1; }
  if (!ctx || n < 0 || (n > 0 && !cols)) return PQG_ERR_INVALID_ARG;
  if (n == 0) return PQG_OK;
  for (int i = 0; i < n; i++) {
    const int err = dict_page_check(cols[i], n_bytes);
    if (err) {
      set_status(st, err, i, -1, "dictionary page");
      return err;
    }
    // the capacity contract of pqg_decode_dictionary, per dictionary (decode_impl makes the same check per
    // column, after this one has passed)
    const uint64_t need = (uint64_t)cols[i].dict_num_values + (bin_out(cols[i]) ? 1 : 0);  // offsets[n + 1]
    if (need > cols[i].values_capacity || (need && !cols[i].values)) {
      set_status(st, PQG_ERR_INVALID_ARG, i, i, "output capacity");
      return PQG_ERR_INVALID_ARG;
    }
  }
  // the descriptors of an earlier batch are about to go: nothing may point at them any more (a batch that
  // was never synchronised loses its values_written, not its memory safety)
  ctx->dicts_user = nullptr;
  if (ctx->last_cols == ctx->dicts_desc.data()) ctx->last_cols = nullptr;
  // one plan of n required one-page columns. Its PLAIN BYTE_ARRAY pages take one wave each
  // (PQG_DISPATCH_PLAIN_ONE_PASS = 3: k_bin_plain_pg, which follows a page from its start and waits on nothing);
  // the tile form's look-back orders tiles over the whole grid, which n short pages do not need
  ctx->dicts_desc.assign((size_t)n, pqg_column_desc{});
  std::vector<pqg_page_desc> pages((size_t)n);
  for (int i = 0; i < n; i++) dict_page_as_column(cols[i], i, &ctx->dicts_desc[(size_t)i], &pages[(size_t)i]);
  const int plain_mode = ctx->plain_mode;
  ctx->plain_mode = 3;
  const int rc = pqg::decode_impl(ctx, d_bytes, n_bytes, n_bytes, ctx->dicts_desc.data(), n, pages.data(), n, nullptr, st);
  ctx->plain_mode = plain_mode;
  if (rc == PQG_OK) ctx->dicts_user = cols;  // pqg_sync hands values_written on
  return rc;
}

}  // extern "C"
