// pqgpu_api_ops.hip — the C ABI's operations on decoded columns: record assembly (pqg_assemble,
// pqg_assemble_schema), pqg_unpack_runs, the record filters (pqg_filter_run, _run_dict, _run_records) and
// row selection (pqg_take, pqg_take_records).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "pqgpu_ctx.h"

extern "C" {

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
    if (ctx->filter_dict.ensure(slot_bytes) != hipSuccess ||
        ctx->filter_dict_pin.ensure(slot_bytes * pqg_ctx::FILTER_DICT_SLOTS) != hipSuccess)
      return PQG_ERR_HIP;
    uint32_t slot;
    if (!ctx->filter_dict_ring.acquire(&slot)) return PQG_ERR_HIP;
    void* pin = (uint8_t*)ctx->filter_dict_pin.p + slot * slot_bytes;
    std::memcpy(pin, rec ? (const void*)rec : (const void*)dt, tab_bytes);
    if (hipMemcpyAsync(ctx->filter_dict.p, pin, tab_bytes, hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
        !ctx->filter_dict_ring.publish(slot, ctx->stream))
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
    uint32_t slot;
    if (!ctx->take_ring.acquire(&slot)) return PQG_ERR_HIP;  // (waits for the copy out of this slot TAKE_SLOTS calls ago)
    void* pin = (uint8_t*)ctx->take_pin.p + slot * slot_bytes;
    std::memcpy(pin, tab, sizeof(pqg::TakeColDev) * (size_t)n_cols);
    if (hipMemcpyAsync(ctx->take_cols.p, pin, sizeof(pqg::TakeColDev) * (size_t)n_cols, hipMemcpyHostToDevice, ctx->stream) !=
            hipSuccess ||
        !ctx->take_ring.publish(slot, ctx->stream))
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
    uint32_t slot;
    if (!ctx->take_ring.acquire(&slot)) return PQG_ERR_HIP;
    void* pin = (uint8_t*)ctx->take_pin.p + slot * slot_bytes;
    std::memcpy(pin, tab, sizeof(pqg::TakeRecDev) * (size_t)plan.n_records);
    if (hipMemcpyAsync(ctx->take_cols.p, pin, sizeof(pqg::TakeRecDev) * (size_t)plan.n_records, hipMemcpyHostToDevice,
                       ctx->stream) != hipSuccess ||
        !ctx->take_ring.publish(slot, ctx->stream))
      return PQG_ERR_HIP;
  }
  const hipError_t e = pqg::launch_take_records(ctx->stream, d_bitmap, n_rows, (const pqg::TakeRecDev*)ctx->take_cols.p,
                                                (uint32_t)n_cols, plan, out_rows_capacity, (uint64_t*)ctx->take_scratch.p,
                                                d_counts, d_result, ctx->take_staged);
  return e == hipSuccess ? PQG_OK : PQG_ERR_HIP;
}

}  // extern "C"
