// pqgpu_ctx.h — the context and the plan behind the C ABI, shared by the pqgpu_api*.hip files, and the
// owners of what they hold on the device: buffers, streams, events, the event ring of the pinned upload
// slots and the side queues of a launch. Every owner releases in its destructor, so pqg_ctx_destroy and
// pqg_plan_destroy name no member; the device must be current when a context or a plan is deleted.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <vector>

#include "pqgpu_internal.h"
#include "pqgpu_api_host.h"
#include "pqgpu_take.h"
#include "pqgpu_crc.h"
#include "pqgpu_aes.h"

namespace pqg {

struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  hipError_t ensure(size_t n) {
    if (n <= cap) return hipSuccess;
    release();
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
  PinnedBuf() = default;
  PinnedBuf(const PinnedBuf&) = delete;
  PinnedBuf& operator=(const PinnedBuf&) = delete;
  ~PinnedBuf() { release(); }
  hipError_t ensure(size_t n) {
    if (n <= cap) return hipSuccess;
    release();
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

// A non-blocking stream created at first need (null when that failed); drained before it is destroyed.
struct Stream {
  hipStream_t s = nullptr;
  Stream() = default;
  Stream(const Stream&) = delete;
  Stream& operator=(const Stream&) = delete;
  ~Stream() {
    if (!s) return;
    (void)hipStreamSynchronize(s);
    (void)hipStreamDestroy(s);
  }
  hipStream_t get_or_create() {
    if (!s && hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) s = nullptr;
    return s;
  }
};

// An event without timing, created at first need (null when that failed).
struct Event {
  hipEvent_t e = nullptr;
  Event() = default;
  Event(const Event&) = delete;
  Event& operator=(const Event&) = delete;
  ~Event() {
    if (e) (void)hipEventDestroy(e);
  }
  hipEvent_t get_or_create() {
    if (!e && hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) e = nullptr;
    return e;
  }
};

// The events of N pinned upload slots used in turn. acquire() hands out the next slot once the stream
// work that read it N calls ago has run (its event; created at the slot's first use); the caller fills the
// slot, queues the work that reads it and publish()es. The ring owns the events only: the pinned and
// device memory of the slots, and how it is sized, stay with the caller.
template <int N>
struct SlotRing {
  Event ev[N];
  uint32_t seq = 0;
  bool acquire(uint32_t* slot) {
    *slot = seq++ % (uint32_t)N;
    Event& e = ev[*slot];
    if (!e.e) return e.get_or_create() != nullptr;
    return hipEventSynchronize(e.e) == hipSuccess;
  }
  bool publish(uint32_t slot, hipStream_t s) { return hipEventRecord(ev[slot].e, s) == hipSuccess; }
};

// A second queue of pqg_plan_launch: forked from the caller's stream at an event recorded there, joined
// back into it through an event of its own.
struct SideQueue {
  Stream stream;
  Event joined;
  // false when anything fails: the launch then runs this queue's kernels on the caller's stream
  bool fork(hipEvent_t ev_fork) {
    return stream.get_or_create() && joined.get_or_create() && hipStreamWaitEvent(stream.s, ev_fork, 0) == hipSuccess;
  }
  bool record() { return hipEventRecord(joined.e, stream.s) == hipSuccess; }
  bool wait(hipStream_t main) { return hipStreamWaitEvent(main, joined.e, 0) == hipSuccess; }
  bool join(hipStream_t main) { return record() && wait(main); }
};

}  // namespace pqg

inline void set_status(pqg_status* st, int code, int page, int64_t idx, const char* what) {
  if (!st) return;
  st->code = code;
  st->page = page;
  st->value_index = idx;
  std::snprintf(st->message, sizeof(st->message), "%s: %s (page %d, index %lld)", what, pqg_error_name(code), page,
                (long long)idx);
}

// Error words: 3 per page + 3 per column (dictionary pages), padded to 16 bytes; the error
// counter follows them in the same allocation.
inline size_t err_region_bytes(int n_pages, int n_cols) {
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

struct pqg_plan {
  pqg_ctx* ctx = nullptr;
  const uint8_t* d_bytes = nullptr;
  uint64_t n_bytes = 0;
  pqg::PlanLayout L;  // what the planner computed from the descriptors (pqgpu_plan.h)
  pqg::DevBuf buf[B_COUNT];
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

struct pqg_ctx {
  int device = 0;
  // the caller's stream, or own_stream (first member: the last one destroyed)
  pqg::Stream own_stream;
  hipStream_t stream = nullptr;
  pqg_plan* last = nullptr;          // plan of the most recent pqg_decode (owned)
  pqg_plan* last_launched = nullptr; // plan of the most recent launch (decode or plan_launch)
  std::vector<pqg_plan*> unsynced;   // plans launched since the last pqg_sync, in launch order
  std::vector<pqg_staged_output> staged;  // pqg_decode_staged: where each column's outputs are in pin_out
  pqg_column_desc* last_cols = nullptr;
  pqg::PinnedBuf pin_in, pin_out, pin_err;
  pqg::DevBuf host_bytes, host_out, host_counts, host_runs;
  pqg::DevBuf asm_scratch;                // pqg_assemble: block counts + totals
  pqg::Stream copy_stream;                // pqg_decode_host: second D2H queue (odd output chunks)
  pqg::DevBuf zstd_scratch;               // pqg_zstd_decompress: literal buffers, ZSTD_LIT_SCRATCH per grid wave
  pqg::DevBuf zstd_seqs, zstd_mode;       // pqg_zstd_decompress: sequence records of the lane-per-page pre-pass, per-job mode
  pqg::DevBuf gzip_recs, gzip_mode;       // pqg_gzip_decompress: back-reference records of the token pre-pass, per-job count
  // pqg_plan_launch forks at ev_fork (recorded on the caller's stream after the levels) and joins before
  // the launch ends. side: the one-pass PLAIN BYTE_ARRAY kernel, on a second queue beside the other
  // columns' kernels;
  pqg::Event ev_fork;
  pqg::SideQueue side;
  // bin: the BYTE_ARRAY kernels of the other columns (dictionary walk / ids / map, per-value walks,
  // offset scan, copies) on a third, beside the fixed-width columns' kernels;
  pqg::SideQueue bin;
  // fix: the fixed-width columns' kernels on a fourth. The three streams are created one after the other
  // with the context, so that HIP's round-robin puts them on different hardware queues; the caller's
  // stream only waits while they run (a queue shared with it costs nothing then).
  pqg::SideQueue fix;
  // ... and the tile walk of large dictionaries beside the id walk of their dictionary-direct pages, whose
  // ids need no entries (C_DDG: the entries are first read by k_dd_gsums, which waits for ev_dent)
  pqg::Stream dent_stream;
  pqg::Event ev_dent_fork, ev_dent;
  // pqg_ctx_set_dispatch: kernel-choice overrides for the plans created on this ctx
  int plain_mode = 2;       // PQG_DISPATCH_PLAIN_ONE_PASS
  bool dict_direct = true;  // PQG_DISPATCH_DICT_DIRECT
  bool dict_fused = true;   // PQG_DISPATCH_DICT_FUSED
  bool null_hints = true;   // PQG_DISPATCH_NULL_HINTS
  uint32_t gz_prepass_min = pqg::GZ_PREPASS_MIN;  // PQG_DISPATCH_GZIP_PREPASS_MIN
  bool zstd_prepass = true;  // PQG_DISPATCH_ZSTD_PREPASS
  pqg::RouterCache router;  // pqg_router_read_page
  // pqg_filter_run: per-tile counts, and the device image of the filter uploaded last (by its serial)
  pqg::DevBuf filter_scratch, filter_image;
  uint64_t filter_serial = 0;
  // pqg_filter_run_dict: the FilterDictTab on the device and the pinned slots it is copied from (a slot is
  // reused once the copy out of it has run: filter_dict_ring)
  static constexpr int FILTER_DICT_SLOTS = 4;
  pqg::DevBuf filter_dict;
  pqg::PinnedBuf filter_dict_pin;
  pqg::SlotRing<FILTER_DICT_SLOTS> filter_dict_ring;
  // pqg_filter_row_groups: the device image of the row-group form of the filter uploaded last (by its serial);
  // per slot the column table + work list in growable pinned memory, their device copy, and the hit flags and
  // per-word counts (a slot is reused once the launches that read it have run: rg_ring)
  static constexpr int RG_SLOTS = 2;
  pqg::DevBuf rg_image;
  uint64_t rg_serial = 0;
  pqg::PinnedBuf rg_pin[RG_SLOTS];
  pqg::DevBuf rg_dev[RG_SLOTS], rg_scratch[RG_SLOTS];
  pqg::SlotRing<RG_SLOTS> rg_ring;
  // pqg_decode_dictionary: the one-column batch it decodes (last_cols points at dict_desc until the next
  // decode) and the caller's descriptor that pqg_sync fills from it
  pqg_column_desc dict_desc = {};
  pqg_column_desc* dict_user = nullptr;
  // pqg_decode_dictionaries: the same for a batch of n dictionary pages, one column each
  std::vector<pqg_column_desc> dicts_desc;
  pqg_column_desc* dicts_user = nullptr;
  // pqg_take: per-tile counts; the column table on the device and the pinned slots it is copied from
  // (a slot is reused once the copy out of it has run: take_ring)
  static constexpr int TAKE_SLOTS = 4;
  // one slot holds the table of either call (pqg_take: TakeColDev, pqg_take_records: TakeRecDev)
  static constexpr size_t TAKE_SLOT_BYTES = sizeof(pqg::TakeRecDev) * pqg::TAKE_REC_MAX_RECORDS;
  pqg::DevBuf take_scratch, take_cols;
  pqg::PinnedBuf take_pin;
  pqg::SlotRing<TAKE_SLOTS> take_ring;
  bool take_staged = true;  // PQG_DISPATCH_TAKE_STAGED
  // pqg_crc32_pages: the constants of crc_tile on the device (built at the first call and when the tile
  // size changes), and per slot the job + tile tables in growable pinned memory, their device copy and
  // the tiles' partial values (a slot is reused once the fold that read it has run: crc_ring)
  static constexpr int CRC_SLOTS = 2;
  uint32_t crc_tile = PQG_CRC_TILE_BYTES;  // PQG_DISPATCH_CRC_TILE_BYTES
  uint32_t crc_tab_tile = 0;
  pqg::DevBuf crc_tab;
  pqg::PinnedBuf crc_pin[CRC_SLOTS];
  pqg::DevBuf crc_dev[CRC_SLOTS], crc_partial[CRC_SLOTS];
  pqg::SlotRing<CRC_SLOTS> crc_ring;
  // pqg_decrypt_pages: te0 on the device (built at the first call), and per slot the job, tile, AAD and key
  // tables in growable pinned memory, their device copy and the tiles' GHASH partials (aes_ring, as above)
  static constexpr int AES_SLOTS = 2;
  uint32_t aes_tile = PQG_AES_TILE_BYTES;  // PQG_DISPATCH_AES_TILE_BYTES
  pqg::DevBuf aes_te0;
  pqg::PinnedBuf aes_pin[AES_SLOTS];
  pqg::DevBuf aes_dev[AES_SLOTS], aes_partial[AES_SLOTS];
  pqg::SlotRing<AES_SLOTS> aes_ring;
  // the key material of the last call (pqg::aes_build_key), reused while the keys and the tile size stay;
  // wiped when it is replaced and when the ctx goes (aes_wipe_keys, which also clears the pinned slots)
  std::vector<uint8_t> aes_keys_seen;
  uint32_t aes_keys_tile = 0;
  std::vector<uint32_t> aes_keymat;
  void aes_wipe_keys(bool slots) {
    volatile uint8_t* p = aes_keys_seen.data();
    for (size_t i = 0; i < aes_keys_seen.size(); i++) p[i] = 0;
    volatile uint32_t* w = aes_keymat.data();
    for (size_t i = 0; i < aes_keymat.size(); i++) w[i] = 0;
    aes_keys_seen.clear();
    aes_keymat.clear();
    aes_keys_tile = 0;
    for (int s = 0; slots && s < AES_SLOTS; s++) {
      volatile uint8_t* q = (volatile uint8_t*)aes_pin[s].p;
      for (size_t i = 0; q && i < aes_pin[s].cap; i++) q[i] = 0;
      if (aes_dev[s].p) (void)hipMemset(aes_dev[s].p, 0, aes_dev[s].cap);
    }
  }
};

// pqg_decode on a batch whose readable bytes (n_bytes) reach past the caller's data (valid_bytes):
// pqgpu_api.hip; pqg_decode_host pads the batch with zero bytes (pqgpu_api_hostpath.hip)
namespace pqg {
int decode_impl(pqg_ctx* ctx, const uint8_t* d_bytes, uint64_t n_bytes, uint64_t valid_bytes, pqg_column_desc* cols,
                int n_cols, const pqg_page_desc* pages, int n_pages, uint32_t* d_page_value_counts, pqg_status* st);
}
