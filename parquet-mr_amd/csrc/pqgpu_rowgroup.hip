// pqgpu_rowgroup.hip — the row-group dictionary filter on the device (pqg_filter_row_groups;
// DictionaryFilter.canDrop for every row group of a file in one call).
//
// One memset and four launches on the context's stream, whatever the number of row groups and columns; none
// waits on another workgroup and there are no atomics (every dependency is a launch boundary):
//   k_rg_any   one wave per item of a host-built flat work list (row group, slot, tile of RG_TILE entries):
//              64 entries per step, lane = entry, the entry loaded once for every leaf of the slot that
//              compares with a value; a leaf that holds on some entry stores the constant 1 into its
//              (row group, node) flag (zeroed beforehand; several waves may store the same 1)
//   k_rg_fold  one lane per row group: the post-order program over the flags and the (row group, slot) flag
//              words, "cannot match" per node as one bit of a 64-bit mask; the drop bitmap word by ballot,
//              the word's kept count beside it
//   k_rg_scan  one workgroup: exclusive scan of the kept counts, the result
//   k_rg_emit  one lane per row group: the kept ids ascending, bounded by the capacity
// The work list is flat because dictionary sizes differ widely between row groups: a grid sized by the
// largest would be mostly empty.
#include <cstring>

#include "pqgpu_ctx.h"
#include "pqgpu_filter_device.h"
#include "pqgpu_rowgroup.h"

namespace pqg {

// ---- k_rg_any --------------------------------------------------------------------------------
template <bool BIN>
__device__ __forceinline__ void rg_any_item(const uint8_t* __restrict__ image, uint32_t image_bytes,
                                            const RgItem* __restrict__ items, uint64_t n_items,
                                            const RgColDev* __restrict__ cols, uint32_t n_slots,
                                            uint32_t* __restrict__ hits) {
  extern __shared__ __align__(16) uint8_t lds[];
  stage_image(lds, image, image_bytes);
  __syncthreads();
  const uint64_t item = (uint64_t)blockIdx.x * FT_WPB + wave_id();
  if (item >= n_items) return;
  const FilterDevHeader& h = *(const FilterDevHeader*)lds;
  const FilterDevNode* nodes = (const FilterDevNode*)(lds + sizeof(FilterDevHeader));
  const uint32_t n_nodes = uni(h.n_nodes), n_leaves = uni(h.n_leaves);
  const uint8_t* order = (const uint8_t*)(nodes + n_nodes);
  const uint64_t* cells = (const uint64_t*)(lds + uni(h.cells_off));
  const uint8_t* lbytes = lds + uni(h.bytes_off);
  const uint32_t g = uni(items[item].group), st = uni(items[item].slot_tile);
  const uint32_t slot = st >> 24, tile = st & 0xFFFFFFu;
  const RgColDev& c = cols[(uint64_t)g * n_slots + slot];
  const void* values = (const void*)(uintptr_t)uni64((uint64_t)(uintptr_t)c.values);
  const uint8_t* binary = (const uint8_t*)(uintptr_t)uni64((uint64_t)(uintptr_t)c.binary);
  const uint32_t n = uni(c.n_entries);
  // the slot's leaves stand together in `order`
  uint32_t l0 = 0;
  while (l0 < n_leaves && uni(nodes[uni(order[l0])].slot) != slot) l0++;
  uint32_t l1 = l0;
  while (l1 < n_leaves && uni(nodes[uni(order[l1])].slot) == slot) l1++;
  if (l0 == l1) return;
  const int32_t type = (int32_t)uni(nodes[uni(order[l0])].type);
  const uint32_t width = BIN ? uni(nodes[uni(order[l0])].width) : 0u;
  uint64_t want = 0, hit = 0;  // wave-uniform: bit l - l0 = leaf l compares with a value / held on some entry
  for (uint32_t l = l0; l < l1; l++)
    if (!(uni(nodes[uni(order[l])].flags) & PQG_FILTER_NULL_LITERAL)) want |= 1ull << (l - l0);
  const uint64_t e0 = (uint64_t)tile * RG_TILE;
  const uint64_t end = e0 + RG_TILE < n ? e0 + RG_TILE : n;
  const uint32_t lane = lane_id();
  for (uint64_t e = e0; e < end && hit != want; e += 64) {
    const uint64_t idx = e + lane;
    const bool valid = idx < n;  // every load stays inside [0, n_entries)
    const LaneValue v = load_value<true, BIN>(type, width, values, binary, valid, idx, n);
    for (uint32_t l = l0; l < l1; l++) {
      const uint64_t bit = 1ull << (l - l0);
      if (!(want & ~hit & bit)) continue;
      const FilterDevNode nd = nodes[uni(order[l])];
      const LaneValue lv = leaf_value<BIN>(nd, type, valid, v);
      if (__ballot(valid && leaf_eval<BIN>(nd, valid, lv, cells, lbytes))) hit |= bit;
    }
  }
  if (lane == 0)
    for (uint32_t l = l0; l < l1; l++)
      if (hit & (1ull << (l - l0))) gst(&hits[(uint64_t)g * n_nodes + uni(order[l])], 1u);
}
__global__ __launch_bounds__(64 * FT_WPB) void k_rg_any(const uint8_t* __restrict__ image, uint32_t image_bytes,
                                                        const RgItem* __restrict__ items, uint64_t n_items,
                                                        const RgColDev* __restrict__ cols, uint32_t n_slots,
                                                        uint32_t* __restrict__ hits) {
  rg_any_item<false>(image, image_bytes, items, n_items, cols, n_slots, hits);
}
__global__ __launch_bounds__(64 * FT_WPB) void k_rg_any_bin(const uint8_t* __restrict__ image, uint32_t image_bytes,
                                                            const RgItem* __restrict__ items, uint64_t n_items,
                                                            const RgColDev* __restrict__ cols, uint32_t n_slots,
                                                            uint32_t* __restrict__ hits) {
  rg_any_item<true>(image, image_bytes, items, n_items, cols, n_slots, hits);
}

// ---- k_rg_fold -------------------------------------------------------------------------------
// A leaf's "cannot match" from what the host knows of the chunk (`flags`, RG_USABLE in them), the
// dictionary's size and whether the leaf held on some entry: the table of include/pqgpu.h.
__device__ __forceinline__ bool rg_leaf_cannot(const FilterDevNode& nd, uint32_t flags, uint32_t n_entries, bool any) {
  const bool missing = (flags & PQG_RG_MISSING) != 0;
  const bool usable = (flags & RG_USABLE) != 0;
  const bool no_null = !(flags & PQG_RG_MAY_CONTAIN_NULL);
  if (nd.flags & PQG_FILTER_NULL_LITERAL) {
    if (nd.op == PQG_FILTER_NOTEQ) return missing;
    if (nd.op == PQG_FILTER_NOTIN) return (nd.flags & FILTER_DEV_NULL_ONLY) && missing;
    return false;  // eq(null), in with null
  }
  if (nd.op == PQG_FILTER_NOTEQ) return usable && n_entries >= 1 && !any && no_null;
  if (nd.op == PQG_FILTER_NOTIN) return usable && !any && no_null;
  return missing || (usable && !any);
}

__global__ __launch_bounds__(64 * FT_WPB) void k_rg_fold(const uint8_t* __restrict__ image, uint32_t image_bytes,
                                                         const RgColDev* __restrict__ cols, uint32_t n_slots,
                                                         const uint32_t* __restrict__ hits, uint64_t n_groups,
                                                         uint64_t* __restrict__ bitmap, uint64_t* __restrict__ counts) {
  extern __shared__ __align__(16) uint8_t lds[];
  stage_image(lds, image, image_bytes);
  __syncthreads();
  const FilterDevHeader& h = *(const FilterDevHeader*)lds;
  const FilterDevNode* nodes = (const FilterDevNode*)(lds + sizeof(FilterDevHeader));
  const uint32_t n_nodes = uni(h.n_nodes);
  const uint64_t word = (uint64_t)blockIdx.x * FT_WPB + wave_id();
  const uint64_t g = word * 64 + lane_id();
  const bool in = g < n_groups;
  uint64_t cannot = 0;  // bit i: node i cannot match in this lane's row group (children have smaller indices)
  for (uint32_t i = 0; i < n_nodes; i++) {
    const FilterDevNode nd = nodes[i];
    const uint32_t op = uni(nd.op);
    bool v = false;
    if (op == PQG_FILTER_AND) {
      v = ((cannot >> nd.left) | (cannot >> nd.right)) & 1u;
    } else if (op == PQG_FILTER_OR) {
      v = ((cannot >> nd.left) & (cannot >> nd.right)) & 1u;
    } else if (op == PQG_FILTER_CONTAINS) {
      v = (cannot >> nd.left) & 1u;
    } else if (in) {
      const RgColDev& c = cols[g * n_slots + nd.slot];
      v = rg_leaf_cannot(nd, c.flags, c.n_entries, hits[g * n_nodes + i] != 0);
    }
    cannot |= (uint64_t)v << i;
  }
  const bool drop = in && ((cannot >> (n_nodes - 1)) & 1u);
  const uint64_t dm = __ballot(drop), km = __ballot(in && !drop);
  if (lane_id() == 0 && word * 64 < n_groups) {  // the bits past n_groups are 0
    gst(&bitmap[word], dm);
    gst(&counts[word], (uint64_t)__popcll(km));
  }
}

// ---- k_rg_scan, k_rg_emit --------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_rg_scan(uint64_t* __restrict__ counts, uint64_t n_words,
                                                 pqg_rowgroup_result* __restrict__ result) {
  const uint64_t total = block_excl_scan_u64<FS_PER>(counts, n_words);
  if (threadIdx.x != 0) return;
  result->n_kept = total;
  result->error = PQG_OK;
  result->error_group = -1;
}

__global__ __launch_bounds__(64 * FT_WPB) void k_rg_emit(const uint64_t* __restrict__ bitmap, const uint64_t* __restrict__ counts,
                                                         uint64_t n_groups, int64_t* __restrict__ kept_ids, uint64_t capacity) {
  const uint64_t word = (uint64_t)blockIdx.x * FT_WPB + wave_id();
  if (word * 64 >= n_groups) return;
  const uint32_t lane = lane_id();
  const uint64_t g = word * 64 + lane;
  const bool kept = g < n_groups && !((bitmap[word] >> lane) & 1u);
  const uint64_t pos = counts[word] + lanes_below(__ballot(kept));
  if (kept && pos < capacity) gst(&kept_ids[pos], (int64_t)g);
}

static hipError_t launch_rowgroups(hipStream_t st, const uint8_t* d_image, uint32_t image_bytes, bool bin,
                                   const RgColDev* d_cols, const RgItem* d_items, uint64_t n_items, uint32_t n_slots,
                                   uint32_t n_nodes, uint64_t n_groups, uint64_t* scratch, uint64_t* bitmap,
                                   int64_t* kept_ids, uint64_t capacity, pqg_rowgroup_result* result) {
  uint32_t* hits = (uint32_t*)scratch;
  uint64_t* counts = scratch + rowgroup_hit_words(n_groups, n_nodes);
  const uint64_t n_words = (n_groups + 63) / 64;
  const uint32_t wgs = (uint32_t)((n_words + FT_WPB - 1) / FT_WPB);
  if (n_groups && hipMemsetAsync(hits, 0, 8 * (size_t)rowgroup_hit_words(n_groups, n_nodes), st) != hipSuccess)
    return hipGetLastError();
  if (n_items)
    hipLaunchKernelGGL(bin ? k_rg_any_bin : k_rg_any, dim3((uint32_t)((n_items + FT_WPB - 1) / FT_WPB)), dim3(64 * FT_WPB),
                       image_bytes, st, d_image, image_bytes, d_items, n_items, d_cols, n_slots, hits);
  if (n_groups)
    hipLaunchKernelGGL(k_rg_fold, dim3(wgs), dim3(64 * FT_WPB), image_bytes, st, d_image, image_bytes, d_cols, n_slots,
                       (const uint32_t*)hits, n_groups, bitmap, counts);
  hipLaunchKernelGGL(k_rg_scan, dim3(1), dim3(256), 0, st, counts, n_words, result);
  if (n_groups && kept_ids && capacity)
    hipLaunchKernelGGL(k_rg_emit, dim3(wgs), dim3(64 * FT_WPB), 0, st, (const uint64_t*)bitmap, (const uint64_t*)counts,
                       n_groups, kept_ids, capacity);
  return hipGetLastError();
}

}  // namespace pqg

static_assert(sizeof(pqg_rowgroup_column) == 32 && sizeof(pqg_rowgroup_result) == 16 && sizeof(pqg_page_encoding_stat) == 12,
              "row-group filter ABI layout");

extern "C" int pqg_filter_row_groups(pqg_ctx* ctx, const pqg_filter* filter, const pqg_rowgroup_column* cols, int n_cols,
                                     uint64_t n_row_groups, uint64_t* d_drop_bitmap, int64_t* d_kept_ids,
                                     uint64_t kept_capacity, pqg_rowgroup_result* d_result) {
  if (!ctx || !filter || !d_result) return PQG_ERR_INVALID_ARG;
  if (n_row_groups && !d_drop_bitmap) return PQG_ERR_INVALID_ARG;
  pqg::RgPlan plan;
  const int rc = pqg::rowgroup_bind(filter, cols, n_cols, n_row_groups, &plan);
  if (rc != PQG_OK) return rc;
  if (hipSetDevice(ctx->device) != hipSuccess) return PQG_ERR_HIP;
  if (ctx->rg_serial != filter->serial) {
    if (ctx->rg_image.ensure(filter->rg_image.size()) != hipSuccess) return PQG_ERR_HIP;
    ctx->rg_serial = 0;
    if (hipMemcpyAsync(ctx->rg_image.p, filter->rg_image.data(), filter->rg_image.size(), hipMemcpyHostToDevice,
                       ctx->stream) != hipSuccess)
      return PQG_ERR_HIP;
    ctx->rg_serial = filter->serial;
  }
  // the column table and the work list go up in one copy, through a pinned slot that is reused once the
  // launches that read its device copy and its scratch have run
  uint32_t slot;
  if (!ctx->rg_ring.acquire(&slot)) return PQG_ERR_HIP;
  const size_t col_bytes = sizeof(pqg::RgColDev) * plan.cols.size();  // a multiple of 8: the items follow
  const size_t bytes = col_bytes + sizeof(pqg::RgItem) * plan.items.size();
  const size_t scratch_bytes = 8 * (size_t)pqg::rowgroup_scratch_words(n_row_groups, plan.n_nodes);
  // grown by half again, so that a run of calls with rising row-group counts does not reallocate each time
  if ((ctx->rg_pin[slot].cap < bytes + 16 && ctx->rg_pin[slot].ensure(bytes + bytes / 2 + 16) != hipSuccess) ||
      (ctx->rg_dev[slot].cap < bytes + 16 && ctx->rg_dev[slot].ensure(bytes + bytes / 2 + 16) != hipSuccess) ||
      (ctx->rg_scratch[slot].cap < scratch_bytes + 16 &&
       ctx->rg_scratch[slot].ensure(scratch_bytes + scratch_bytes / 2 + 16) != hipSuccess))
    return PQG_ERR_HIP;
  uint8_t* pin = (uint8_t*)ctx->rg_pin[slot].p;
  if (col_bytes) std::memcpy(pin, plan.cols.data(), col_bytes);
  if (bytes > col_bytes) std::memcpy(pin + col_bytes, plan.items.data(), bytes - col_bytes);
  if (bytes && hipMemcpyAsync(ctx->rg_dev[slot].p, pin, bytes, hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
    return PQG_ERR_HIP;
  const uint8_t* dev = (const uint8_t*)ctx->rg_dev[slot].p;
  const hipError_t e = pqg::launch_rowgroups(
      ctx->stream, (const uint8_t*)ctx->rg_image.p, (uint32_t)filter->rg_image.size(), filter->binary_paths,
      (const pqg::RgColDev*)dev, (const pqg::RgItem*)(dev + col_bytes), plan.items.size(), plan.n_slots, plan.n_nodes,
      n_row_groups, (uint64_t*)ctx->rg_scratch[slot].p, d_drop_bitmap, d_kept_ids, kept_capacity, d_result);
  if (e != hipSuccess || !ctx->rg_ring.publish(slot, ctx->stream)) return PQG_ERR_HIP;
  return PQG_OK;
}
