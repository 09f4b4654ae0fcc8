// pqgpu_api_host.h — the host-only logic of the C ABI (pqgpu_api_host.cpp): the hybrid-stream walk and the
// run cache of pqg_router_read_page, the pinned image of pqg_router_read_runs, error resolution of a
// launched plan, the length-prefix walk of a BYTE_ARRAY dictionary page. Plain C++ with no HIP include, so
// that tests/c/api_host_main.cpp runs it under AddressSanitizer + UndefinedBehaviorSanitizer without a
// device; the pqgpu_api*.hip files keep the allocations, the copies and the launches.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "pqgpu_plan.h"

namespace pqg {

// ---- pqg_router_read_page / pqg_router_cache_lookup ------------------------------------------------

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

// Bounds of one walk: what a miss decodes in its single round trip.
constexpr uint64_t ROUTER_MAX_VALUES = 1u << 22;
constexpr size_t ROUTER_MAX_RUNS = 1u << 16;

// Served from the cache when the run at this stream position (stream_left bytes before the end) was
// walked, with the same width and count, and its bytes are the ones unpacked then.
bool router_hit(RouterCache& c, int w, const uint8_t* in, uint64_t need, uint64_t stream_left, int count, int32_t* out);

// pqg_router_cache_lookup on the context's cache (null: no context): the argument checks, then router_hit.
int router_cache_lookup(RouterCache* c, int bit_width, const uint8_t* run, size_t stream_left, int count, int32_t* out,
                        int* hit);

// The walk of a miss: lists the requested run (count values at in[0]) and every bit-packed run after it
// in [0, stream_left) into c.off / c.cnt / c.vo, sizes c.vals for their values and keeps the walked bytes
// in c.bytes. c.w stays -1 until the caller has unpacked the runs into c.vals.
void router_walk(RouterCache& c, int bit_width, const uint8_t* in, uint64_t stream_left, int count);

// ---- pqg_router_read_runs: the pinned image ---------------------------------------------------------

// [run bytes, each 16-B aligned][in_off u64 x n][out_off u64 x n][counts u32 x n]
struct RouterRunsImage {
  uint64_t n_bytes = 0, n_vals = 0;  // padded run bytes; values of all runs
  uint32_t max_count = 0;
  uint64_t o_in = 0, o_out = 0, o_cnt = 0, img = 0;  // table offsets and the image's size
};
// Every run's slice (SingleBufferInputStream.slice throws before any unpack), then the image's offsets.
// PQG_OK, PQG_ERR_INVALID_ARG or PQG_ERR_EOF; n_vals == 0: nothing to unpack.
int router_runs_layout(int bit_width, const uint8_t* in, size_t in_len, const uint64_t* in_offsets, const uint32_t* counts,
                       int n_runs, RouterRunsImage* im);
// Writes the image (im.img bytes at pin).
void router_runs_fill(const RouterRunsImage& im, int bit_width, const uint8_t* in, const uint64_t* in_offsets,
                      const uint32_t* counts, int n_runs, uint8_t* pin);

// ---- error resolution of a launched plan ------------------------------------------------------------

// Raw error words of the device -> keys: a word of the launch's epoch gives its key, words of earlier
// launches are stale (no error in this one: ~0).
void decode_error_words(std::vector<uint64_t>* errs, uint32_t epoch);

// Every page's own first error (pqg_page_errors) from the decoded words (empty: no kernel reported) and
// the planner's host errors, then the batch's first in page order: its code is returned (PQG_OK: none)
// with the page, the status value index and what the status message names.
int resolve_page_errors(const PlanLayout& L, const std::vector<uint64_t>& errs, std::vector<pqg_page_error>* page_errs,
                        int* first_page, int64_t* index, const char** what);

// pqg_sync's timeout re-runs: is the failing page one of the fused dictionary kernel's / a PLAIN
// BYTE_ARRAY page
inline int page_class(const PlanLayout& L, int page) { return page >= 0 && page < L.n_pages ? L.page_cls[(size_t)page] : -1; }
inline bool page_is_dict_class(const PlanLayout& L, int page) {
  const int c = page_class(L, page);
  return c == C_DICT4 || c == C_DICT8 || c == C_IDS || c == C_DD || c == C_DDG;
}
inline bool page_is_binp(const PlanLayout& L, int page) { return page_class(L, page) == C_BINP; }

// ---- pqg_decode_dictionary --------------------------------------------------------------------------

// The length prefixes of a BYTE_ARRAY dictionary page of n_values entries that the decode refused with
// PQG_ERR_EOF: PQG_ERR_CORRUPT where an entry reaches past the page (PlainBinaryDictionary's slice),
// PQG_ERR_EOF where a prefix does.
int dict_page_eof_code(const uint8_t* bytes, size_t size, uint32_t n_values);

}  // namespace pqg
