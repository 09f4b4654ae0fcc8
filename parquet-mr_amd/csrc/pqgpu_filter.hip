// pqgpu_filter.hip — record-level filter2 predicates over decoded columns (pqg_filter_run,
// pqg_filter_run_dict, and at the end of the file contains() on list columns: pqg_filter_run_records).
//
// Five launches on the context's stream, none of which waits on another workgroup (every
// cross-tile dependency is a launch boundary):
//   k_filter_rank  per nullable column and tile: rows with dl == max_def
//   k_filter_scan  one workgroup per column: exclusive scan of those counts (a tile's first dense
//                  value index), the total checked against the column's n_values
//   k_filter_eval  one wave per tile of PQG_FILTER_TILE_ROWS rows, 64 rows per step, lane = row
//   k_filter_scan  the tiles' selected counts -> first row id slot per tile, n_selected, the result
//   k_filter_emit  bitmap words -> ascending row ids, bounded by the capacity
// A tile is one wave's work: 64 steps of 64 rows, lane k keeping the bitmap word of step k, so the
// tile's 64 words leave as one 512-byte store.
// With dictionary-id columns (pqg_filter_run_dict) one launch goes first when a leaf has a verdict table:
//   k_filter_dict  one wave per 64 entries of a leaf's dictionary: the leaf on every entry, one bit each
// and k_filter_eval<true> takes a leaf's verdict on such a column as bit `id` of its table.
// BIN: a program with a leaf on an INT96 / FIXED_LEN_BYTE_ARRAY column or under the signed-integer or FLOAT16
// order runs the *_bin form of k_filter_dict, k_filter_eval, k_filter_eval_records and k_filter_contains:
// the same code with those paths compiled in. Every other program runs the kernels without them.
#include "pqgpu_filter_device.h"

namespace pqg {

// ---- k_filter_rank ---------------------------------------------------------------------------
__global__ __launch_bounds__(64 * FT_WPB) void k_filter_rank(const FilterCols cols, uint64_t n_rows, uint64_t n_tiles,
                                                             uint64_t* __restrict__ rank) {
  const uint64_t tile = (uint64_t)blockIdx.x * FT_WPB + wave_id();
  if (tile >= n_tiles) return;
  const uint32_t ni = blockIdx.y;
  const FilterColDev& c = cols.c[cols.null_slot[ni]];
  const uint8_t* __restrict__ dl = c.dl;
  const uint32_t md = (uint32_t)c.max_def;
  const uint32_t lane = lane_id();
  const uint64_t row0 = tile * FT_ROWS;
  uint32_t cnt = 0;
  if (((uintptr_t)dl & 3u) == 0) {
#pragma unroll 4
    for (uint32_t k = 0; k < FT_ROWS / 256; k++) {
      const uint64_t r = row0 + 4ull * (k * 64u + lane);
      if (r + 4 <= n_rows) {
        const uint32_t w = *(const uint32_t*)(dl + r);
        cnt += ((w & 0xFFu) == md) + (((w >> 8) & 0xFFu) == md) + (((w >> 16) & 0xFFu) == md) + ((w >> 24) == md);
      } else {
        for (uint32_t b = 0; b < 4; b++)
          if (r + b < n_rows) cnt += dl[r + b] == md;
      }
    }
  } else {
    for (uint32_t s = 0; s < FT_STEPS; s++) {
      const uint64_t r = row0 + s * 64u + lane;
      if (r < n_rows) cnt += dl[r] == md;
    }
  }
  uint32_t total;
  (void)wave_excl_scan_u32(cnt, &total);
  if (lane == 0) gst(&rank[(uint64_t)ni * n_tiles + tile], (uint64_t)total);
}

// ---- k_filter_scan ---------------------------------------------------------------------------
// One workgroup per row of `arr` (n_tiles words each): exclusive scan in place, FS_PER tiles per thread
// per round. FINAL = false (the rank counts of nullable column blockIdx.x): the total goes to
// totals[blockIdx.x] and bad[blockIdx.x] says whether it differs from the column's n_values.
// FINAL = true (the selected counts, one row): writes the result, with the first bad column; DICT: when
// the counts are right, the lowest column with an id outside its dictionary (dict_bad, per slot).
template <bool FINAL, bool DICT = false>
__global__ __launch_bounds__(256) void k_filter_scan(uint64_t* __restrict__ arr, uint64_t n_tiles, const FilterCols cols,
                                                     uint64_t* __restrict__ totals, uint64_t* __restrict__ bad,
                                                     pqg_filter_result* __restrict__ result,
                                                     const uint64_t* __restrict__ dict_bad) {
  const uint64_t carry = block_excl_scan_u64<FS_PER>(arr + (uint64_t)blockIdx.x * n_tiles, n_tiles);
  if (threadIdx.x != 0) return;
  if (!FINAL) {
    gst(&totals[blockIdx.x], carry);
    gst(&bad[blockIdx.x], (uint64_t)(carry != cols.c[cols.null_slot[blockIdx.x]].n_values));
  } else {
    int32_t err_col = -1;
    for (uint32_t ni = 0; ni < cols.n_nullable; ni++) {
      const int32_t col = cols.c[cols.null_slot[ni]].column;
      if (bad[ni] && (err_col < 0 || col < err_col)) err_col = col;
    }
    int32_t err = err_col >= 0 ? PQG_ERR_INVALID_ARG : PQG_OK;
    if (DICT && err_col < 0) {
      for (uint32_t s = 0; s < cols.n_slots; s++) {
        const int32_t col = cols.c[s].column;
        if (dict_bad[s] && (err_col < 0 || col < err_col)) err_col = col;
      }
      if (err_col >= 0) err = PQG_ERR_DICT_ID;
    }
    result->n_selected = carry;
    result->error = err;
    result->error_column = err_col;
  }
}

// ---- k_filter_dict ---------------------------------------------------------------------------
// Grid (64-entry words / FT_WPB, table leaves): a wave evaluates its leaf on 64 entries of the leaf's
// dictionary, lane = entry, and stores the ballot as one word of the leaf's table. Entries past n_entries: 0.
template <bool BIN>
__device__ __forceinline__ void filter_dict_words(const uint8_t* __restrict__ image, uint32_t image_bytes,
                                                  const FilterDictTab* __restrict__ dt, uint64_t* __restrict__ tables) {
  extern __shared__ __align__(16) uint8_t lds[];
  stage_image(lds, image, image_bytes);
  __syncthreads();
  const FilterDevHeader& h = *(const FilterDevHeader*)lds;
  const FilterDevNode* nodes = (const FilterDevNode*)(lds + sizeof(FilterDevHeader));
  const uint64_t* cells = (const uint64_t*)(lds + uni(h.cells_off));
  const uint8_t* lbytes = lds + uni(h.bytes_off);
  const uint32_t ni = uni(dt->table_leaf[blockIdx.y]);
  const FilterDevNode nd = nodes[ni];
  const FilterDictSlot ds = dt->slot[uni(nd.slot)];
  const uint32_t n = uni(ds.n_entries);
  const uint64_t word = (uint64_t)blockIdx.x * FT_WPB + wave_id();
  if (word >= ((uint64_t)n + 63) / 64) return;
  const uint32_t type = uni(nd.type);
  const uint64_t e = word * 64 + lane_id();
  const bool valid = e < n;
  const LaneValue v = leaf_value<BIN>(
      nd, (int32_t)type, valid, load_value<true, BIN>((int32_t)type, BIN ? uni(nd.width) : 0u, ds.values, ds.binary, valid, e, n));
  const uint64_t m = __ballot(valid && leaf_eval<BIN>(nd, valid, v, cells, lbytes));
  if (lane_id() == 0) gst(&tables[uni64(dt->leaf_off[ni]) + word], m);
}
__global__ __launch_bounds__(64 * FT_WPB) void k_filter_dict(const uint8_t* __restrict__ image, uint32_t image_bytes,
                                                             const FilterDictTab* __restrict__ dt,
                                                             uint64_t* __restrict__ tables) {
  filter_dict_words<false>(image, image_bytes, dt, tables);
}
__global__ __launch_bounds__(64 * FT_WPB) void k_filter_dict_bin(const uint8_t* __restrict__ image, uint32_t image_bytes,
                                                                 const FilterDictTab* __restrict__ dt,
                                                                 uint64_t* __restrict__ tables) {
  filter_dict_words<true>(image, image_bytes, dt, tables);
}

// ---- k_filter_eval ---------------------------------------------------------------------------
// DICT = false is pqg_filter_run's kernel. DICT = true: slots with a dictionary (dt->slot[s].is_dict) hold
// uint32 ids; a leaf's verdict on a row is bit `id` of the leaf's table (staged in LDS behind the image when
// dt->in_lds, else read from `tables`), a row without a value takes the leaf's verdict on null, and an id
// outside the dictionary sets the slot's word of dict_bad (every writer stores 1) and matches nothing.
// REC (with DICT; k_filter_eval_records): rows are records, `dt` is the FilterDictTab that begins a
// FilterRecDev, a repeated slot and every leaf under a CONTAINS node are skipped, and a CONTAINS node's 64
// records of step s are word tile * 64 + s of its leaf's record bitmap (k_filter_contains wrote it): lane i
// loads the word of node i one step ahead.
template <bool DICT, bool REC, bool BIN>
__device__ __forceinline__ void filter_eval_tile(const uint8_t* __restrict__ image, uint32_t image_bytes,
                                                 const FilterCols& cols, uint64_t n_rows, uint64_t n_tiles,
                                                 const uint64_t* __restrict__ rank, uint64_t* __restrict__ bitmap,
                                                 uint64_t* __restrict__ sel, const FilterDictTab* __restrict__ dt,
                                                 const uint64_t* __restrict__ tables, uint64_t* __restrict__ dict_bad) {
  extern __shared__ __align__(16) uint8_t lds[];
  stage_image(lds, image, image_bytes);
  const uint64_t* lds_tables = (const uint64_t*)(lds + image_bytes);  // image_bytes is a multiple of 8
  bool in_lds = false;
  if (DICT) {
    in_lds = uni(dt->in_lds) != 0;
    if (in_lds) {
      const uint32_t words = (uint32_t)uni64(dt->table_words);
      for (uint32_t i = threadIdx.x; i < words; i += 64u * FT_WPB) ((uint64_t*)(lds + image_bytes))[i] = tables[i];
    }
  }
  __syncthreads();
  const uint64_t tile = (uint64_t)blockIdx.x * FT_WPB + wave_id();
  if (tile >= n_tiles) return;
  const FilterDevHeader& h = *(const FilterDevHeader*)lds;
  const FilterDevNode* nodes = (const FilterDevNode*)(lds + sizeof(FilterDevHeader));
  const uint32_t n_nodes = uni(h.n_nodes), n_leaves = uni(h.n_leaves), n_slots = uni(h.n_slots);
  const uint8_t* order = (const uint8_t*)(nodes + n_nodes);
  const uint64_t* cells = (const uint64_t*)(lds + uni(h.cells_off));
  const uint8_t* lbytes = lds + uni(h.bytes_off);

  const uint32_t lane = lane_id();
  const uint64_t row0 = tile * FT_ROWS;
  const uint64_t n_words = (n_rows + 63) / 64;
  const uint32_t steps = n_words - tile * FT_STEPS < FT_STEPS ? (uint32_t)(n_words - tile * FT_STEPS) : FT_STEPS;

  // lane s holds slot s's state: the dense index of the tile's next non-null row
  uint64_t next_idx = 0;
  if (lane < n_slots) {
    const FilterColDev& c = cols.c[lane];
    if (c.null_idx >= 0) next_idx = rank[(uint64_t)c.null_idx * n_tiles + tile];
  }
  uint64_t node_mask = 0;  // lane i holds the 64-row mask of node i in the current step
  uint64_t my_word = 0;    // lane k keeps the bitmap word of step k
  uint32_t n_sel = 0;
  const uint64_t* my_bm = nullptr;  // REC: lane i of a CONTAINS node i: the tile's words of its record bitmap
  uint64_t bm_next = 0;
  if (REC) {
    const FilterRecTab& rt = ((const FilterRecDev*)dt)->rt;
    if (lane < n_nodes && nodes[lane].op == PQG_FILTER_CONTAINS)
      my_bm = rt.bitmaps + (uint64_t)rt.node_leaf[lane] * rt.bitmap_words + tile * FT_STEPS;
    if (my_bm && steps) bm_next = my_bm[0];
  }

  for (uint32_t s = 0; s < steps; s++) {
    const uint64_t row = row0 + s * 64u + lane;
    const bool in = row < n_rows;
    uint32_t li = 0;
    uint64_t bm_word = 0;
    if (REC) {
      bm_word = bm_next;
      if (my_bm && s + 1 < steps) bm_next = my_bm[s + 1];
    }
    for (uint32_t sl = 0; sl < n_slots; sl++) {
      const FilterColDev& c = cols.c[sl];
      const int32_t type = c.type;
      if (REC && c.null_idx == FILTER_NULL_IDX_REPEATED) {  // its leaves all stand under CONTAINS nodes
        while (li < n_leaves && uni(nodes[uni(order[li])].slot) == sl) li++;
        continue;
      }
      bool valid;
      uint64_t idx;
      if (c.max_def == 0) {
        valid = in;
        idx = row;
      } else if (!c.dl) {
        valid = false;
        idx = 0;
      } else {
        valid = in && c.dl[row] == (uint8_t)c.max_def;
        const uint64_t vb = __ballot(valid);
        const uint64_t base = rdl64(next_idx, sl);
        idx = base + lanes_below(vb);
        if (lane == sl) next_idx = base + (uint32_t)__popcll(vb);
      }
      valid = valid && idx < c.n_values;  // every value load stays inside the column
      if (DICT && uni(dt->slot[sl].is_dict)) {
        const uint32_t n_entries = uni(dt->slot[sl].n_entries);
        const uint32_t id = valid ? ((const uint32_t*)c.values)[idx] : 0u;
        const bool ok = valid && id < n_entries;  // every table read stays inside the table
        if (valid && !ok) gst(&dict_bad[sl], (uint64_t)1);
        while (li < n_leaves) {
          const uint32_t ni = uni(order[li]);
          const FilterDevNode nd = nodes[ni];
          if (uni(nd.slot) != sl) break;
          if (REC && (nd.flags & FILTER_DEV_CONTAINED)) {  // on a missing column: the bitmap says false
            li++;
            continue;
          }
          bool verdict;
          if (nd.flags & PQG_FILTER_NULL_LITERAL) {
            verdict = (nd.op == PQG_FILTER_EQ || nd.op == PQG_FILTER_IN) ? !valid : valid;
          } else {
            uint64_t w = 0;
            if (ok) {
              const uint64_t o = uni64(dt->leaf_off[ni]) + (id >> 6);
              w = in_lds ? lds_tables[o] : tables[o];
            }
            // a null row: what leaf_eval gives without a value
            verdict = valid ? ((w >> (id & 63u)) & 1u) != 0 : (nd.op == PQG_FILTER_NOTEQ || nd.op == PQG_FILTER_NOTIN);
          }
          const uint64_t m = __ballot(verdict);
          if (lane == ni) node_mask = m;
          li++;
        }
        continue;
      }
      const uint32_t width = BIN && li < n_leaves ? uni(nodes[uni(order[li])].width) : 0u;  // the column's, in its leaves
      const LaneValue v = load_value<false, BIN>(type, width, c.values, c.binary, valid, idx, 0);
      // every leaf on this column (the column is loaded once per step)
      while (li < n_leaves) {
        const uint32_t ni = uni(order[li]);
        const FilterDevNode nd = nodes[ni];
        if (uni(nd.slot) != sl) break;
        if (REC && (nd.flags & FILTER_DEV_CONTAINED)) {
          li++;
          continue;
        }
        const LaneValue lv = leaf_value<BIN>(nd, type, valid, v);
        const uint64_t m = __ballot(leaf_eval<BIN>(nd, valid, lv, cells, lbytes));
        if (lane == ni) node_mask = m;
        li++;
      }
    }
    if (REC && my_bm) node_mask = bm_word;
    // and / or on wave-uniform 64-row masks (children have smaller indices)
    for (uint32_t i = 0; i < n_nodes; i++) {
      const uint32_t op = uni(nodes[i].op);
      if (op != PQG_FILTER_AND && op != PQG_FILTER_OR) continue;
      const uint64_t a = rdl64(node_mask, uni(nodes[i].left)), b = rdl64(node_mask, uni(nodes[i].right));
      const uint64_t m = op == PQG_FILTER_AND ? (a & b) : (a | b);
      if (lane == i) node_mask = m;
    }
    const uint64_t word = rdl64(node_mask, n_nodes - 1) & __ballot(in);  // rows past n_rows: 0
    if (lane == s) my_word = word;
    n_sel += (uint32_t)__popcll(word);
  }
  if (lane < steps) gst_nt(&bitmap[tile * FT_STEPS + lane], my_word);
  if (lane == 0) gst(&sel[tile], (uint64_t)n_sel);
}
template <bool DICT>
__global__ __launch_bounds__(64 * FT_WPB) void k_filter_eval(const uint8_t* __restrict__ image, uint32_t image_bytes,
                                                             const FilterCols cols, uint64_t n_rows, uint64_t n_tiles,
                                                             const uint64_t* __restrict__ rank, uint64_t* __restrict__ bitmap,
                                                             uint64_t* __restrict__ sel,
                                                             const FilterDictTab* __restrict__ dt,
                                                             const uint64_t* __restrict__ tables,
                                                             uint64_t* __restrict__ dict_bad) {
  filter_eval_tile<DICT, false, false>(image, image_bytes, cols, n_rows, n_tiles, rank, bitmap, sel, dt, tables, dict_bad);
}
template <bool DICT>
__global__ __launch_bounds__(64 * FT_WPB) void k_filter_eval_bin(const uint8_t* __restrict__ image, uint32_t image_bytes,
                                                                 const FilterCols cols, uint64_t n_rows, uint64_t n_tiles,
                                                                 const uint64_t* __restrict__ rank,
                                                                 uint64_t* __restrict__ bitmap, uint64_t* __restrict__ sel,
                                                                 const FilterDictTab* __restrict__ dt,
                                                                 const uint64_t* __restrict__ tables,
                                                                 uint64_t* __restrict__ dict_bad) {
  filter_eval_tile<DICT, false, true>(image, image_bytes, cols, n_rows, n_tiles, rank, bitmap, sel, dt, tables, dict_bad);
}
// pqg_filter_run_records with contains leaves: the records form, a kernel of its own
__global__ __launch_bounds__(64 * FT_WPB) void k_filter_eval_records(const uint8_t* __restrict__ image, uint32_t image_bytes,
                                                                     const FilterCols cols, uint64_t n_rows, uint64_t n_tiles,
                                                                     const uint64_t* __restrict__ rank,
                                                                     uint64_t* __restrict__ bitmap, uint64_t* __restrict__ sel,
                                                                     const FilterRecDev* __restrict__ rd,
                                                                     const uint64_t* __restrict__ tables,
                                                                     uint64_t* __restrict__ dict_bad) {
  filter_eval_tile<true, true, false>(image, image_bytes, cols, n_rows, n_tiles, rank, bitmap, sel, &rd->dt, tables, dict_bad);
}
__global__ __launch_bounds__(64 * FT_WPB) void k_filter_eval_records_bin(
    const uint8_t* __restrict__ image, uint32_t image_bytes, const FilterCols cols, uint64_t n_rows, uint64_t n_tiles,
    const uint64_t* __restrict__ rank, uint64_t* __restrict__ bitmap, uint64_t* __restrict__ sel,
    const FilterRecDev* __restrict__ rd, const uint64_t* __restrict__ tables, uint64_t* __restrict__ dict_bad) {
  filter_eval_tile<true, true, true>(image, image_bytes, cols, n_rows, n_tiles, rank, bitmap, sel, &rd->dt, tables, dict_bad);
}

// ---- k_filter_emit ---------------------------------------------------------------------------
// Row ids of a tile: its first output slot is sel[tile] (scanned), lane k expands word k.
__global__ __launch_bounds__(64 * FT_WPB) void k_filter_emit(const uint64_t* __restrict__ bitmap, uint64_t n_rows,
                                                             uint64_t n_tiles, const uint64_t* __restrict__ sel,
                                                             int64_t* __restrict__ row_ids, uint64_t capacity) {
  const uint64_t tile = (uint64_t)blockIdx.x * FT_WPB + wave_id();
  if (tile >= n_tiles) return;
  const uint32_t lane = lane_id();
  const uint64_t n_words = (n_rows + 63) / 64;
  const uint64_t wi = tile * FT_STEPS + lane;
  uint64_t w = wi < n_words ? bitmap[wi] : 0;
  uint32_t total;
  const uint32_t before = wave_excl_scan_u32((uint32_t)__popcll(w), &total);
  uint64_t pos = sel[tile] + before;
  const int64_t base = (int64_t)(wi * 64);
  while (w && pos < capacity) {
    gst(&row_ids[pos], base + (int64_t)__builtin_ctzll(w));
    w &= w - 1;
    pos++;
  }
}

// ---- launch ----------------------------------------------------------------------------------
hipError_t launch_filter(hipStream_t st, const uint8_t* d_image, uint32_t image_bytes, const FilterCols& cols,
                         uint64_t n_rows, uint64_t* scratch, uint64_t* bitmap, int64_t* row_ids, uint64_t row_ids_capacity,
                         pqg_filter_result* result, const FilterDictTab* d_dict, const FilterDictTab* h_dict, bool bin) {
  const uint64_t n_tiles = filter_tiles(n_rows);
  uint64_t* rank = scratch;
  uint64_t* sel = rank + (uint64_t)cols.n_nullable * n_tiles;
  uint64_t* totals = sel + n_tiles;
  uint64_t* bad = totals + PQG_FILTER_MAX_NODES;
  uint64_t* dict_bad = bad + PQG_FILTER_MAX_NODES;      // with dictionaries only
  uint64_t* tables = dict_bad + PQG_FILTER_MAX_NODES;
  const uint32_t wgs = (uint32_t)((n_tiles + FT_WPB - 1) / FT_WPB);
  if (d_dict) {
    if (hipMemsetAsync(dict_bad, 0, 8 * PQG_FILTER_MAX_NODES, st) != hipSuccess) return hipGetLastError();
    if (h_dict->n_tables)
      hipLaunchKernelGGL(bin ? k_filter_dict_bin : k_filter_dict,
                         dim3((uint32_t)((h_dict->max_words + FT_WPB - 1) / FT_WPB), h_dict->n_tables), dim3(64 * FT_WPB),
                         image_bytes, st, d_image, image_bytes, d_dict, tables);
  }
  if (cols.n_nullable) {
    if (n_tiles)
      hipLaunchKernelGGL(k_filter_rank, dim3(wgs, cols.n_nullable), dim3(64 * FT_WPB), 0, st, cols, n_rows, n_tiles, rank);
    hipLaunchKernelGGL(k_filter_scan<false>, dim3(cols.n_nullable), dim3(256), 0, st, rank, n_tiles, cols, totals, bad,
                       result, (const uint64_t*)nullptr);
  }
  if (!d_dict) {
    if (n_tiles)
      hipLaunchKernelGGL(bin ? k_filter_eval_bin<false> : k_filter_eval<false>, dim3(wgs), dim3(64 * FT_WPB), image_bytes, st, d_image, image_bytes, cols,
                         n_rows, n_tiles, rank, bitmap, sel, (const FilterDictTab*)nullptr, (const uint64_t*)nullptr,
                         (uint64_t*)nullptr);
    hipLaunchKernelGGL(k_filter_scan<true>, dim3(1), dim3(256), 0, st, sel, n_tiles, cols, totals, bad, result,
                       (const uint64_t*)nullptr);
  } else {
    const uint32_t lds_bytes = image_bytes + (h_dict->in_lds ? (uint32_t)h_dict->table_words * 8u : 0u);
    if (n_tiles)
      hipLaunchKernelGGL(bin ? k_filter_eval_bin<true> : k_filter_eval<true>, dim3(wgs), dim3(64 * FT_WPB), lds_bytes, st, d_image, image_bytes, cols,
                         n_rows, n_tiles, rank, bitmap, sel, d_dict, tables, dict_bad);
    hipLaunchKernelGGL((k_filter_scan<true, true>), dim3(1), dim3(256), 0, st, sel, n_tiles, cols, totals, bad, result,
                       dict_bad);
  }
  if (n_tiles && row_ids && row_ids_capacity)
    hipLaunchKernelGGL(k_filter_emit, dim3(wgs), dim3(64 * FT_WPB), 0, st, bitmap, n_rows, n_tiles, sel, row_ids,
                       row_ids_capacity);
  return hipGetLastError();
}

// ==== contains() on list columns (pqg_filter_run_records) ========================================
// Ahead of the launches above, for the repeated columns the predicate names (numbered by FilterRecTab):
//   k_filter_rec_count  per (repeated column, tile of slots): slots with rep == 0 and slots with
//                       def == max_def, the level bytes read as dwords; tile 0 also the verdict on slot 0
//   k_filter_rec_scan   one workgroup per repeated column: both counts scanned in place (a tile's first
//                       record index and first dense value index), the totals checked against n_rows and
//                       n_values; the column's verdict goes into `bad` behind the flat nullable columns
//   k_filter_contains   per (group of up to 4 contains leaves of one column, tile of slots): 64 steps of
//                       64 slots, lane = slot, the value loaded once; each leaf's hits are folded to one
//                       bit per record and ORed into the leaf's record bitmap
// and k_filter_eval_records reads the bitmaps. scratch behind launch_filter's (u64 words):
// flags[PQG_FILTER_MAX_NODES] (slot 0 continues a record, per repeated column), bitmaps[n_leaves][T * 64]
// (T = tiles of n_rows; both zeroed by one memset), starts[n_rep][S], vals[n_rep][S] (S = tiles of the
// largest n_slots).
struct RecFilterScratch {
  uint64_t *flags, *bitmaps, *starts, *vals;
};
static __host__ __device__ inline RecFilterScratch rec_filter_scratch(uint64_t* base, uint64_t bitmap_words,
                                                                      uint32_t n_leaves, uint32_t n_rep, uint64_t s_tiles) {
  RecFilterScratch r;
  r.flags = base;
  r.bitmaps = r.flags + PQG_FILTER_MAX_NODES;
  r.starts = r.bitmaps + (uint64_t)n_leaves * bitmap_words;
  r.vals = r.starts + (uint64_t)n_rep * s_tiles;
  return r;
}
uint64_t filter_records_scratch_words(uint64_t n_rows, uint32_t n_nullable, uint64_t dict_words, uint32_t n_leaves,
                                      uint32_t n_rep, uint64_t max_slots) {
  return filter_scratch_words(n_rows, n_nullable, dict_words) + PQG_FILTER_MAX_NODES +
         (uint64_t)n_leaves * filter_tiles(n_rows) * FT_STEPS + 2ull * n_rep * filter_tiles(max_slots);
}

// ---- k_filter_rec_count ----------------------------------------------------------------------
__global__ __launch_bounds__(64 * FT_WPB) void k_filter_rec_count(const FilterCols cols, const FilterRecDev* __restrict__ rd,
                                                                  uint64_t s_tiles, uint64_t* __restrict__ flags,
                                                                  uint64_t* __restrict__ starts, uint64_t* __restrict__ vals) {
  const uint32_t ri = blockIdx.y;
  const FilterColDev& c = cols.c[uni(rd->rt.rep_slot[ri])];
  const uint8_t* __restrict__ rl = (const uint8_t*)uni64((uint64_t)(uintptr_t)rd->rt.rl[ri]);
  const uint8_t* __restrict__ dl = c.dl;
  const uint64_t n = uni64(rd->rt.n_slots[ri]);
  const uint32_t md = (uint32_t)c.max_def;
  const uint64_t tile = (uint64_t)blockIdx.x * FT_WPB + wave_id();
  if (tile * FT_ROWS >= n) return;
  const uint32_t lane = lane_id();
  const uint64_t row0 = tile * FT_ROWS;
  const bool words = ((((uintptr_t)rl) | ((uintptr_t)dl)) & 3u) == 0;
  uint32_t n_start = 0, n_val = 0;
  // a lane takes 4 slots at a time: their level bytes are one dword each
#pragma unroll 4
  for (uint32_t k = 0; k < FT_ROWS / 256; k++) {
    const uint64_t r = row0 + 4ull * (k * 64u + lane);
    if (r >= n) continue;
    if (words && r + 4 <= n) {
      const uint32_t w = *(const uint32_t*)(rl + r), v = *(const uint32_t*)(dl + r);
      n_start += ((w & 0xFFu) == 0) + (((w >> 8) & 0xFFu) == 0) + (((w >> 16) & 0xFFu) == 0) + ((w >> 24) == 0);
      n_val += ((v & 0xFFu) == md) + (((v >> 8) & 0xFFu) == md) + (((v >> 16) & 0xFFu) == md) + ((v >> 24) == md);
    } else {
      for (uint32_t b = 0; b < 4 && r + b < n; b++) {
        n_start += rl[r + b] == 0;
        n_val += dl[r + b] == md;
      }
    }
  }
  uint32_t t_start, t_val;
  (void)wave_excl_scan_u32(n_start, &t_start);
  (void)wave_excl_scan_u32(n_val, &t_val);
  if (lane == 0) {
    gst(&starts[(uint64_t)ri * s_tiles + tile], (uint64_t)t_start);
    gst(&vals[(uint64_t)ri * s_tiles + tile], (uint64_t)t_val);
    if (tile == 0) gst(&flags[ri], (uint64_t)(rl[0] != 0));  // a column does not begin inside a record
  }
}

// ---- k_filter_rec_scan -----------------------------------------------------------------------
// Workgroup ri: the two count rows of repeated column ri over the column's own tiles, in place;
// bad[first_bad + ri] = slot 0 continues a record, or the record starts are not n_rows, or the slots with a
// value are not n_values (k_filter_scan<true> reads it with the flat columns' verdicts).
__global__ __launch_bounds__(256) void k_filter_rec_scan(const FilterCols cols, const FilterRecDev* __restrict__ rd,
                                                         uint64_t s_tiles, uint64_t n_rows, const uint64_t* __restrict__ flags,
                                                         uint64_t* __restrict__ starts, uint64_t* __restrict__ vals,
                                                         uint64_t* __restrict__ bad, uint32_t first_bad) {
  const uint32_t ri = blockIdx.x;
  const uint64_t n = rd->rt.n_slots[ri];
  const uint64_t tiles = (n + FT_ROWS - 1) / FT_ROWS;
  const uint64_t n_start = block_excl_scan_u64<FS_PER>(starts + (uint64_t)ri * s_tiles, tiles);
  const uint64_t n_val = block_excl_scan_u64<FS_PER>(vals + (uint64_t)ri * s_tiles, tiles);
  if (threadIdx.x != 0) return;
  const uint64_t n_values = cols.c[rd->rt.rep_slot[ri]].n_values;
  gst(&bad[first_bad + ri], (uint64_t)((n && flags[ri]) || n_start != n_rows || n_val != n_values));
}

// ---- k_filter_contains -----------------------------------------------------------------------
// Grid (slot tiles / FT_WPB, groups of contains leaves): a wave takes one tile of its group's column and
// evaluates the group's leaves (up to FILTER_CONTAINS_GROUP, all on that column) on one load of the levels
// and of the value. K = 1, 2 or 4 is the run's largest group (one launch either way): a single contains
// per column, the common case, does not carry the registers and loops of four. Per step of 64 slots: the slot's record index as k_rec_expand computes it (tile base +
// starts up to and including the lane - 1), its dense value index from the ballot of def == max_def, the
// value (or the id) loaded once, and per leaf `hit` = the ballot of slots that have a value and match (the
// leaf on the value, or bit `id` of the leaf's verdict table). The hits are folded to one bit per record the
// step touches (at most 64 consecutive records: segment 0 is the record continuing from the step before,
// then one per start): the last lane of every segment tests `hit` over its segment and sends the verdict to
// the lane of the segment's number with one ds_permute (the other lanes send 0 to the lanes behind, so the
// addresses are a permutation), and a ballot gives the step's record mask.
// Per leaf, lane k keeps word k of the tile's record range, counted from the word of the tile's first
// record; a tile of 4,096 one-slot records that starts mid-word reaches a 65th word, kept wave-uniform in
// `extra`. A word strictly between the tile's first and last record word holds only records that lie wholly
// inside this tile: plain store. The first and the last word may be shared with the neighbouring tiles (a
// record may span tiles): 64-bit agent-scope atomic OR without return, only when non-zero. The bitmaps were
// zeroed before the launch. Nothing is written for a record index of -1 or >= n_rows (such a slot never
// hits), so every store stays inside ceil(n_rows / 64) words.
template <uint32_t K, bool BIN>
__device__ __forceinline__ void filter_contains_tile(const uint8_t* __restrict__ image, uint32_t image_bytes,
                                                     const FilterCols& cols, uint64_t n_rows, uint64_t s_tiles,
                                                     const FilterRecDev* __restrict__ rd, const uint64_t* __restrict__ starts,
                                                     const uint64_t* __restrict__ vals, const uint64_t* __restrict__ tables,
                                                     uint64_t* __restrict__ dict_bad) {
  static_assert(K <= FILTER_CONTAINS_GROUP, "a group holds at most FILTER_CONTAINS_GROUP leaves");
  extern __shared__ __align__(16) uint8_t lds[];
  stage_image(lds, image, image_bytes);
  const uint64_t* lds_tables = (const uint64_t*)(lds + image_bytes);
  const bool in_lds = uni(rd->dt.in_lds) != 0;
  if (in_lds) {
    const uint32_t words = (uint32_t)uni64(rd->dt.table_words);
    for (uint32_t i = threadIdx.x; i < words; i += 64u * FT_WPB) ((uint64_t*)(lds + image_bytes))[i] = tables[i];
  }
  __syncthreads();
  const uint32_t gi = blockIdx.y;
  const uint32_t ri = uni(rd->rt.group_rep[gi]);
  const uint32_t cnt = uni(rd->rt.group_n[gi]);
  const FilterDevHeader& h = *(const FilterDevHeader*)lds;
  const FilterDevNode* nodes = (const FilterDevNode*)(lds + sizeof(FilterDevHeader));
  const uint64_t* cells = (const uint64_t*)(lds + uni(h.cells_off));
  const uint8_t* lbytes = lds + uni(h.bytes_off);
  uint32_t leaf[K], ni[K];
#pragma unroll
  for (uint32_t k = 0; k < K; k++) {
    leaf[k] = k < cnt ? uni(rd->rt.group_leaf[gi][k]) : 0u;
    ni[k] = uni(rd->rt.leaf_node[leaf[k]]);
  }
  const uint32_t sl = uni(nodes[ni[0]].slot);
  const FilterColDev& c = cols.c[sl];
  const uint64_t n = uni64(rd->rt.n_slots[ri]);
  const uint64_t tile = (uint64_t)blockIdx.x * FT_WPB + wave_id();
  if (tile * FT_ROWS >= n) return;
  const uint8_t* __restrict__ rl = (const uint8_t*)uni64((uint64_t)(uintptr_t)rd->rt.rl[ri]);
  const uint8_t* __restrict__ dl = c.dl;
  const uint8_t md = (uint8_t)c.max_def;
  const int32_t type = c.type;
  const uint64_t n_values = c.n_values;
  const bool is_dict = uni(rd->dt.slot[sl].is_dict) != 0;
  const uint32_t n_entries = uni(rd->dt.slot[sl].n_entries);

  const uint32_t lane = lane_id();
  const uint64_t row0 = tile * FT_ROWS;
  uint64_t run = uni64(starts[(uint64_t)ri * s_tiles + tile]);      // record starts before the step
  uint64_t next_idx = uni64(vals[(uint64_t)ri * s_tiles + tile]);   // values before the step
  const uint64_t wb = run ? (run - 1) >> 6 : 0;                     // the word of the tile's first record
  uint64_t my_word[K], extra[K];  // per leaf: lane k holds word wb + k of its record bitmap, extra word wb + 64
#pragma unroll
  for (uint32_t k = 0; k < K; k++) my_word[k] = extra[k] = 0;
  const uint64_t low = (2ull << lane) - 1ull;  // lanes up to and including this one

  for (uint32_t s = 0; s < FT_STEPS; s++) {
    const uint64_t slot = row0 + s * 64u + lane;
    if (row0 + s * 64u >= n) break;
    const bool in = slot < n;
    const uint8_t rep = in ? rl[slot] : 1;
    const uint8_t def = in ? dl[slot] : 0;
    const uint64_t start = __ballot(in && rep == 0);
    // starts up to and including this slot, minus 1: before the column's first start it wraps to 2^64 - 1,
    // which no n_rows exceeds
    const uint64_t rec = run + lanes_below(start) + ((start >> lane) & 1ull) - 1ull;
    const uint64_t rec0 = run + (start & 1ull) - 1ull;  // lane 0's record: segment 0
    run += (uint32_t)__popcll(start);
    bool valid = in && def == md;
    const uint64_t vb = __ballot(valid);
    const uint64_t idx = next_idx + lanes_below(vb);
    next_idx += (uint32_t)__popcll(vb);
    valid = valid && idx < n_values && rec < n_rows;  // every value load stays inside the column
    uint64_t hit[K];
    if (is_dict) {
      const uint32_t id = valid ? ((const uint32_t*)c.values)[idx] : 0u;
      const bool ok = valid && id < n_entries;  // every table read stays inside the table
      if (valid && !ok) gst(&dict_bad[sl], (uint64_t)1);
#pragma unroll
      for (uint32_t k = 0; k < K; k++) {
        hit[k] = 0;
        if (k >= cnt) continue;
        uint64_t w = 0;
        if (ok) {
          const uint64_t o = uni64(rd->dt.leaf_off[ni[k]]) + (id >> 6);
          w = in_lds ? lds_tables[o] : tables[o];
        }
        hit[k] = __ballot(((w >> (id & 63u)) & 1u) != 0);
      }
    } else {
      const LaneValue v = load_value<false, BIN>(type, BIN ? uni(nodes[ni[0]].width) : 0u, c.values, c.binary, valid, idx, 0);
#pragma unroll
      for (uint32_t k = 0; k < K; k++) {
        hit[k] = 0;
        if (k >= cnt) continue;
        const FilterDevNode nd = nodes[ni[k]];
        const LaneValue lv = leaf_value<BIN>(nd, type, valid, v);
        hit[k] = __ballot(valid && leaf_eval<BIN>(nd, valid, lv, cells, lbytes));
      }
    }
    uint64_t any = 0;
#pragma unroll
    for (uint32_t k = 0; k < K; k++) any |= hit[k];
    if (any == 0) continue;
    // segments: lane l closes one when lane l + 1 starts a record (lane 63 always does)
    const uint64_t last = (start >> 1) | (1ull << 63);
    const bool is_last = ((last >> lane) & 1ull) != 0;
    const uint32_t dest = is_last ? lanes_below(last) : (uint32_t)__popcll(last) + lanes_below(~last);
    const uint64_t mine = start & low;  // starts up to and including this lane: the highest begins its segment
    const uint32_t seg0 = mine ? 63u - (uint32_t)__builtin_clzll(mine) : 0u;
    const uint64_t seg = is_last ? low & ~((1ull << seg0) - 1ull) : 0;  // the lanes of the segment this lane closes
    uint64_t first = rec0;
    const bool before = first == ~0ull;  // segment 0 precedes the column's first record: it never hits
    if (before) first = 0;
    const uint64_t o = first - wb * 64;  // below 65 * 64 whenever a record mask has a bit
    const uint32_t w = (uint32_t)(o >> 6), sh = (uint32_t)(o & 63u);
#pragma unroll
    for (uint32_t k = 0; k < K; k++) {
      if (hit[k] == 0) continue;
      const int got = __builtin_amdgcn_ds_permute((int)(dest << 2), (int)((hit[k] & seg) != 0));
      uint64_t rec_mask = __ballot(got != 0);  // bit j: record rec0 + j
      if (before) rec_mask >>= 1;
      const uint64_t lo = rec_mask << sh, hi = sh ? rec_mask >> (64u - sh) : 0;
      if (lane == w) my_word[k] |= lo;
      if (lane == w + 1) my_word[k] |= hi;
      if (w == 64) extra[k] |= lo;
      if (w == 63) extra[k] |= hi;
    }
  }
  if (run == 0) return;  // no record has begun by the tile's end
  const uint64_t wl = (run - 1) >> 6;  // the word of the tile's last record
  const uint64_t bitmap_words = uni64(rd->rt.bitmap_words);
#pragma unroll
  for (uint32_t k = 0; k < K; k++) {
    if (k >= cnt) continue;
    uint64_t* __restrict__ bm = rd->rt.bitmaps + (uint64_t)leaf[k] * bitmap_words;
    if (my_word[k]) {
      const uint64_t wi = wb + lane;
      if (wi == wb || wi == wl) (void)__hip_atomic_fetch_or(&bm[wi], my_word[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      else gst(&bm[wi], my_word[k]);
    }
    if (extra[k] && lane == 0) {
      const uint64_t wi = wb + 64;
      if (wi == wl) (void)__hip_atomic_fetch_or(&bm[wi], extra[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      else gst(&bm[wi], extra[k]);
    }
  }
}

template <uint32_t K>
__global__ __launch_bounds__(64 * FT_WPB) void k_filter_contains(const uint8_t* __restrict__ image, uint32_t image_bytes,
                                                                 const FilterCols cols, uint64_t n_rows, uint64_t s_tiles,
                                                                 const FilterRecDev* __restrict__ rd,
                                                                 const uint64_t* __restrict__ starts,
                                                                 const uint64_t* __restrict__ vals,
                                                                 const uint64_t* __restrict__ tables,
                                                                 uint64_t* __restrict__ dict_bad) {
  filter_contains_tile<K, false>(image, image_bytes, cols, n_rows, s_tiles, rd, starts, vals, tables, dict_bad);
}
template <uint32_t K>
__global__ __launch_bounds__(64 * FT_WPB) void k_filter_contains_bin(const uint8_t* __restrict__ image, uint32_t image_bytes,
                                                                     const FilterCols cols, uint64_t n_rows, uint64_t s_tiles,
                                                                     const FilterRecDev* __restrict__ rd,
                                                                     const uint64_t* __restrict__ starts,
                                                                     const uint64_t* __restrict__ vals,
                                                                     const uint64_t* __restrict__ tables,
                                                                     uint64_t* __restrict__ dict_bad) {
  filter_contains_tile<K, true>(image, image_bytes, cols, n_rows, s_tiles, rd, starts, vals, tables, dict_bad);
}

// ---- launch ----------------------------------------------------------------------------------
// d_rec / h_rec: the FilterRecDev on the device and on the host (h_rec->rt.bitmaps already points into the
// scratch: filter_records_bitmaps).
uint64_t* filter_records_bitmaps(uint64_t* scratch, uint64_t n_rows, uint32_t n_nullable, uint64_t dict_words) {
  return rec_filter_scratch(scratch + filter_scratch_words(n_rows, n_nullable, dict_words), 0, 0, 0, 0).bitmaps;
}
hipError_t launch_filter_records(hipStream_t st, const uint8_t* d_image, uint32_t image_bytes, const FilterCols& cols,
                                 uint64_t n_rows, uint64_t* scratch, uint64_t* bitmap, int64_t* row_ids,
                                 uint64_t row_ids_capacity, pqg_filter_result* result, const FilterRecDev* d_rec,
                                 const FilterRecDev* h_rec, bool bin) {
  const FilterDictTab& hd = h_rec->dt;
  const FilterRecTab& hr = h_rec->rt;
  const uint64_t n_tiles = filter_tiles(n_rows), s_tiles = filter_tiles(hr.max_slots);
  uint64_t* rank = scratch;
  uint64_t* sel = rank + (uint64_t)cols.n_nullable * n_tiles;
  uint64_t* totals = sel + n_tiles;
  uint64_t* bad = totals + PQG_FILTER_MAX_NODES;
  uint64_t* dict_bad = bad + PQG_FILTER_MAX_NODES;
  uint64_t* tables = dict_bad + PQG_FILTER_MAX_NODES;
  const RecFilterScratch R = rec_filter_scratch(tables + hd.table_words, hr.bitmap_words, hr.n_leaves, hr.n_rep, s_tiles);
  const FilterDictTab* d_dict = &d_rec->dt;
  const uint32_t wgs = (uint32_t)((n_tiles + FT_WPB - 1) / FT_WPB), s_wgs = (uint32_t)((s_tiles + FT_WPB - 1) / FT_WPB);
  const uint32_t lds_bytes = image_bytes + (hd.in_lds ? (uint32_t)hd.table_words * 8u : 0u);
  if (hipMemsetAsync(dict_bad, 0, 8 * PQG_FILTER_MAX_NODES, st) != hipSuccess) return hipGetLastError();
  if (hipMemsetAsync(R.flags, 0, 8 * (PQG_FILTER_MAX_NODES + (size_t)hr.n_leaves * hr.bitmap_words), st) != hipSuccess)
    return hipGetLastError();
  if (hd.n_tables)
    hipLaunchKernelGGL(bin ? k_filter_dict_bin : k_filter_dict, dim3((uint32_t)((hd.max_words + FT_WPB - 1) / FT_WPB), hd.n_tables),
                       dim3(64 * FT_WPB), image_bytes, st, d_image, image_bytes, d_dict, tables);
  if (hr.n_rep) {
    if (s_tiles)
      hipLaunchKernelGGL(k_filter_rec_count, dim3(s_wgs, hr.n_rep), dim3(64 * FT_WPB), 0, st, cols, d_rec, s_tiles, R.flags,
                         R.starts, R.vals);
    hipLaunchKernelGGL(k_filter_rec_scan, dim3(hr.n_rep), dim3(256), 0, st, cols, d_rec, s_tiles, n_rows, R.flags, R.starts,
                       R.vals, bad, cols.n_nullable);
    if (s_tiles) {
      uint32_t largest = 1;
      for (uint32_t g = 0; g < hr.n_groups; g++) largest = hr.group_n[g] > largest ? hr.group_n[g] : largest;
      auto* kernel = largest == 1 ? k_filter_contains<1> : largest == 2 ? k_filter_contains<2> : k_filter_contains<FILTER_CONTAINS_GROUP>;
      if (bin)
        kernel = largest == 1 ? k_filter_contains_bin<1>
                              : largest == 2 ? k_filter_contains_bin<2> : k_filter_contains_bin<FILTER_CONTAINS_GROUP>;
      hipLaunchKernelGGL(kernel, dim3(s_wgs, hr.n_groups), dim3(64 * FT_WPB), lds_bytes, st, d_image, image_bytes, cols, n_rows,
                         s_tiles, d_rec, R.starts, R.vals, tables, dict_bad);
    }
  }
  if (cols.n_nullable) {
    if (n_tiles)
      hipLaunchKernelGGL(k_filter_rank, dim3(wgs, cols.n_nullable), dim3(64 * FT_WPB), 0, st, cols, n_rows, n_tiles, rank);
    hipLaunchKernelGGL(k_filter_scan<false>, dim3(cols.n_nullable), dim3(256), 0, st, rank, n_tiles, cols, totals, bad,
                       result, (const uint64_t*)nullptr);
  }
  if (n_tiles)
    hipLaunchKernelGGL(bin ? k_filter_eval_records_bin : k_filter_eval_records, dim3(wgs), dim3(64 * FT_WPB), lds_bytes, st, d_image, image_bytes, cols,
                       n_rows, n_tiles, rank, bitmap, sel, d_rec, tables, dict_bad);
  // the verdicts of the repeated columns stand behind those of the flat nullable ones
  FilterCols all = cols;
  for (uint32_t ri = 0; ri < hr.n_rep; ri++) all.null_slot[all.n_nullable++] = hr.rep_slot[ri];
  hipLaunchKernelGGL((k_filter_scan<true, true>), dim3(1), dim3(256), 0, st, sel, n_tiles, all, totals, bad, result,
                     dict_bad);
  if (n_tiles && row_ids && row_ids_capacity)
    hipLaunchKernelGGL(k_filter_emit, dim3(wgs), dim3(64 * FT_WPB), 0, st, bitmap, n_rows, n_tiles, sel, row_ids,
                       row_ids_capacity);
  return hipGetLastError();
}

}  // namespace pqg
