// plan_layout.cpp — the planner of pqg_plan_create (csrc/pqgpu_plan_host.cpp, pqg::plan_layout) on its own,
// without a device: built with AddressSanitizer + UndefinedBehaviorSanitizer by tests/test_plan_layout.py.
// The descriptor tables are made here (hand-written cases and a seeded PRNG); the output pointers in them
// are small fake addresses, which the planner may copy but never read through.
//   plan_layout cases     every case under every dispatch setting: accepted (then the invariants below hold)
//                         or refused as the case expects
//   plan_layout digest    one line per case: return code, then for every distinct layout the settings that give
//                         it (plain_mode, dict_direct, null_hints digits) and a 64-bit FNV-1a hash of its full
//                         digest line (plan_digest.h: every scalar, a hash per table; then plan_kernel_count in
//                         all eight mode combinations): tests/golden/plan/layout_digest.txt
//   plan_layout digest-full   the full digest lines themselves, to see what differs when a hash does
//   plan_layout fuzz N    N single-field mutations of the small cases: accepted + invariants, or refused
// The last line of every mode is "cases=<n> ok=<accepted> invalid=<refused>".
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <string>
#include <vector>

#include "plan_digest.h"

#ifndef PLAN_LAYOUT_CALL  // (the digest file is recorded with another implementation behind the same signature)
#define PLAN_LAYOUT_CALL pqg::plan_layout
#else
namespace pqg {
int PLAN_LAYOUT_CALL(uint64_t n_bytes, uint64_t valid_bytes, const pqg_column_desc* cols, int n_cols,
                     const pqg_page_desc* pages, int n_pages, const PlanOptions& opt, PlanLayout* out, int* bad_page);
}
#endif

using namespace pqg;

namespace {

struct Case {
  std::string name;
  std::vector<pqg_column_desc> cols;
  std::vector<pqg_page_desc> pages;
  uint64_t end = 0;   // bytes of the imaginary batch buffer handed out so far
  int expect_rc = PQG_OK;
  std::function<void(const PlanLayout&)> check;  // facts of the layout under the default dispatch settings

  uint64_t alloc(uint64_t bytes) {
    const uint64_t o = end;
    end = (end + bytes + 15) & ~15ull;
    return o;
  }
  int col(int type, int type_length = 0, int max_def = 0, int max_rep = 0) {
    pqg_column_desc c;
    std::memset(&c, 0, sizeof(c));
    const uintptr_t fake = 0x10000u * (uintptr_t)(cols.size() + 1);
    c.physical_type = type;
    c.type_length = type_length;
    c.max_def = max_def;
    c.max_rep = max_rep;
    c.dict_offset = -1;
    c.values = (void*)(fake + 0x1000);
    c.values_capacity = ~0ull;
    c.def_levels = (uint8_t*)(fake + 0x2000);
    c.rep_levels = (uint8_t*)(fake + 0x3000);
    c.levels_capacity = ~0ull;
    c.binary_data = (uint8_t*)(fake + 0x4000);
    c.binary_capacity = 1u << 20;
    cols.push_back(c);
    return (int)cols.size() - 1;
  }
  void dict(int ci, uint32_t n, uint32_t size, int enc = PQG_PLAIN) {
    cols[(size_t)ci].dict_offset = (int64_t)alloc(size);
    cols[(size_t)ci].dict_size = size;
    cols[(size_t)ci].dict_num_values = n;
    cols[(size_t)ci].dict_encoding = enc;
  }
  pqg_page_desc& page(int ci, int enc, uint32_t num_values, uint32_t size, int version = 1) {
    pqg_page_desc g;
    std::memset(&g, 0, sizeof(g));
    g.offset = alloc(size);
    g.size = size;
    g.num_values = num_values;
    g.column = ci;
    g.version = version;
    g.encoding = enc;
    g.rl_encoding = PQG_RLE;
    g.dl_encoding = PQG_RLE;
    pages.push_back(g);
    return pages.back();
  }
};

[[noreturn]] void fail(const std::string& where, const char* what) {
  std::fprintf(stderr, "FAILED %s: %s\n", where.c_str(), what);
  std::exit(1);
}
#define REQUIRE(cond) do { if (!(cond)) fail(where, #cond); } while (0)

// ---- the invariants of an accepted layout (none depends on a recorded value)
void check_invariants(const std::string& where, const Case& c, const PlanLayout& L) {
  const int n_pages = (int)c.pages.size(), n_cols = (int)c.cols.size();
  REQUIRE(L.n_pages == n_pages && L.n_cols == n_cols);
  REQUIRE(L.h_work.size() == (size_t)std::max(n_pages, 1) && L.cols.size() == (size_t)std::max(n_cols, 1));
  // scratch regions: aligned, disjoint, inside the buffer; the cleared ones a prefix of whole regions
  std::map<uint64_t, int> starts;
  for (size_t i = 0; i < L.regions.size(); i++) {
    const ScratchRegion& r = L.regions[i];
    REQUIRE(r.off % 256 == 0 && r.bytes > 0);
    const uint64_t next = i + 1 < L.regions.size() ? L.regions[i + 1].off : L.scratch_bytes;
    REQUIRE(r.off + r.bytes >= r.off && r.off + r.bytes <= next);  // (in take order, so sorted and disjoint)
    // cleared per launch, then cleared on the per-value path, then the rest
    REQUIRE(i == 0 || std::min(L.regions[i - 1].clear, CLEAR_EPOCH) <= std::min(r.clear, CLEAR_EPOCH));
    REQUIRE(r.column >= -1 && r.column < n_cols);
    starts[r.off] = (int)r.clear;
  }
  REQUIRE(L.scratch_bytes % 256 == 0);
  uint64_t end_launch = 0, end_pv = 0;
  for (size_t i = 0; i < L.regions.size(); i++) {
    const uint64_t next = i + 1 < L.regions.size() ? L.regions[i + 1].off : L.scratch_bytes;
    if (L.regions[i].clear == CLEAR_LAUNCH) end_launch = next;
    if (L.regions[i].clear <= CLEAR_PER_VALUE) end_pv = next;
  }
  REQUIRE(L.blen_bytes_nf == end_launch && L.blen_bytes == end_pv);
  REQUIRE(L.blen_bytes_nf <= L.blen_bytes && L.blen_bytes <= L.scratch_bytes);
  auto is_region = [&](uint64_t off) { return starts.count(off) != 0; };
  for (const std::vector<uint64_t>* v : {&L.blen_off, &L.bsrc_off, &L.dlen_off, &L.dsrc_off, &L.dent_off, &L.bsum_off,
                                         &L.bin_total_off}) {
    REQUIRE(v->size() == (size_t)std::max(n_cols, 1));
    for (uint64_t o : *v) REQUIRE(o == NO_REGION || is_region(o));
  }
  if (L.n_segs) REQUIRE(is_region(L.seg_status_off) && starts[L.seg_status_off] == CLEAR_LAUNCH && is_region(L.seg_tmp_off));
  if (L.n_pcp) REQUIRE(is_region(L.pticket_off) && starts[L.pticket_off] == CLEAR_LAUNCH && is_region(L.pflag_off) &&
                       starts[L.pflag_off] == CLEAR_EPOCH);
  if (L.null_hints) REQUIRE(is_region(L.hint_off) && starts[L.hint_off] == CLEAR_EPOCH);
  if (L.n_dba_chunks) REQUIRE(is_region(L.dba_meta_off));
  if (L.n_dent_tiles) REQUIRE(is_region(L.dent_rec_off) && is_region(L.dent_scr_off) && is_region(L.dent_tb_off));
  for (int g = 0; g < 2; g++)
    if (L.dd_chunk_n[g]) REQUIRE(is_region(L.dd_sums_off[g]));
  // lists lie inside their tables and name valid pages / columns
  auto pages_ok = [&](const std::vector<int32_t>& v, size_t off, size_t n) {
    if (off + n > v.size()) return false;
    for (size_t i = off; i < off + n; i++)
      if (v[i] < 0 || v[i] >= n_pages) return false;
    return true;
  };
  auto cols_ok = [&](const std::vector<int32_t>& v, size_t off, size_t n) {
    if (off + n > v.size()) return false;
    for (size_t i = off; i < off + n; i++)
      if (v[i] < 0 || v[i] >= n_cols) return false;
    return true;
  };
  REQUIRE(L.levels_off >= 0 && L.levels_n >= 0 && pages_ok(L.flat, (size_t)L.levels_off, (size_t)L.levels_n));
  std::vector<int> listed((size_t)std::max(n_pages, 1), 0);
  size_t flat_total = (size_t)L.levels_n;
  for (int k = 0; k < C_NCLS; k++) {
    REQUIRE(L.cls_off[k] >= 0 && L.cls_n[k] >= 0 && pages_ok(L.flat, (size_t)L.cls_off[k], (size_t)L.cls_n[k]));
    for (int i = 0; i < L.cls_n[k]; i++) {
      const int p = L.flat[(size_t)(L.cls_off[k] + i)];
      listed[(size_t)p]++;
      REQUIRE(L.page_cls[(size_t)p] == k);
    }
    flat_total += (size_t)L.cls_n[k];
  }
  REQUIRE(flat_total == L.flat.size());
  REQUIRE(L.n_binp_fused >= 0 && L.n_binp_seg >= 0 && L.n_binp_fused + L.n_binp_seg <= L.cls_n[C_BINP]);
  // every page: in exactly one class list, or refused by the host, or of a column refused at its first page
  std::vector<int> page_err((size_t)std::max(n_pages, 1), 0), col_err((size_t)std::max(n_cols, 1), 0);
  for (const HostErr& e : L.host_errs) {
    REQUIRE(e.page >= 0 && e.page < n_pages && e.code != PQG_OK);
    page_err[(size_t)e.page] = 1;
    if (e.index == -1) {
      const int ci = L.h_work[(size_t)e.page].column;
      REQUIRE(L.col_first_page[(size_t)ci] == e.page);
      col_err[(size_t)ci] = 1;
    }
  }
  for (int p = 0; p < n_pages; p++) {
    const int ci = L.h_work[(size_t)p].column;
    REQUIRE(ci >= 0 && ci < n_cols && ci == c.pages[(size_t)p].column);
    REQUIRE(listed[(size_t)p] <= 1);
    REQUIRE((listed[(size_t)p] == 1) != (page_err[(size_t)p] || col_err[(size_t)ci]));
    if (!listed[(size_t)p]) REQUIRE(L.page_cls[(size_t)p] == -1);
  }
  REQUIRE(L.n_scan_cols == (int)L.cps.size() - 1 && L.cps[0] == 0 && (size_t)L.cps.back() == L.cp.size());
  REQUIRE(std::is_sorted(L.cps.begin(), L.cps.end()) && pages_ok(L.cp, 0, L.cp.size()) && L.cp.size() == (size_t)L.levels_n);
  REQUIRE(L.n_pcols == (int)L.pcs.size() - 1 && L.pcs[0] == 0 && (size_t)L.pcs.back() == L.pcp.size());
  REQUIRE(std::is_sorted(L.pcs.begin(), L.pcs.end()) && pages_ok(L.pcp, 0, L.pcp.size()) && L.n_pcp == (int)L.pcp.size());
  REQUIRE(L.n_pcp == L.n_binp_fused);
  REQUIRE(cols_ok(L.bl, (size_t)L.off_dict_walk, (size_t)L.n_dict_walk) && pages_ok(L.bl, (size_t)L.off_bind, (size_t)L.n_bind) &&
          pages_ok(L.bl, (size_t)L.off_fixd, (size_t)L.n_fixd) && cols_ok(L.bl, (size_t)L.off_bin_cols, (size_t)L.n_bin_cols) &&
          cols_ok(L.bl, (size_t)L.off_carry, (size_t)L.n_carry) && cols_ok(L.bl, (size_t)L.off_dent_cols, (size_t)L.n_dent_cols));
  REQUIRE((size_t)L.off_dent_start + (size_t)L.n_dent_cols + 1 <= L.bl.size());
  for (int i = 0; i <= L.n_dent_cols; i++) {
    const int32_t v = L.bl[(size_t)(L.off_dent_start + i)];
    REQUIRE(v >= 0 && (uint32_t)v <= L.n_dent_tiles && (i == 0 ? v == 0 : v >= L.bl[(size_t)(L.off_dent_start + i - 1)]));
  }
  REQUIRE((uint32_t)L.bl[(size_t)(L.off_dent_start + L.n_dent_cols)] == L.n_dent_tiles);
  // work lists: sizes, and every entry names a valid page / column (or is the dictionary padding)
  REQUIRE(L.n_bin_blocks == L.bin_blocks.size() && L.n_bin_chunks == L.bin_chunks.size() &&
          L.n_dba_chunks == L.dba_chunks.size() && L.n_segs == L.segs.size() && L.n_dent_tiles == L.dent_tiles.size() &&
          L.n_psegs == L.psegs.size() && L.chunk_total == L.chunk_list.size());
  for (uint64_t e : L.bin_blocks) REQUIRE((e >> 32) < (uint64_t)n_cols);
  for (uint64_t e : L.dent_tiles) REQUIRE((uint32_t)e < (uint32_t)n_cols);
  for (const std::vector<uint64_t>* v : {&L.bin_chunks, &L.dba_chunks, &L.segs, &L.psegs})
    for (uint64_t e : *v) REQUIRE((uint32_t)e < (uint32_t)n_pages);
  for (uint64_t e : L.chunk_list) REQUIRE(e == 0xFFFFFFFFull || (uint32_t)e < (uint32_t)n_pages);
  for (int i = 0; i < N_DICT_CLS; i++) REQUIRE((uint64_t)L.chunk_off[i] + L.chunk_n[i] <= L.chunk_list.size());
  // dictionary-direct chunks: per column [begin, end), begins at whole workgroups, non-decreasing
  for (int g = 0; g < 2; g++) {
    REQUIRE((uint64_t)L.dd_chunk_off[g] + L.dd_chunk_n[g] <= L.chunk_list.size());
    REQUIRE(L.n_dd_cols[g] >= 0 && cols_ok(L.bl, (size_t)L.off_dd_cols[g], (size_t)L.n_dd_cols[g]));
    REQUIRE((size_t)L.off_dd_start[g] + 2 * (size_t)L.n_dd_cols[g] <= L.bl.size());
    int32_t prev = 0;
    for (int i = 0; i < 2 * L.n_dd_cols[g]; i++) {
      const int32_t v = L.bl[(size_t)(L.off_dd_start[g] + i)];
      REQUIRE(v >= prev && (uint32_t)v <= L.dd_chunk_n[g]);
      if (i % 2 == 0) REQUIRE(v % DICT_WPB == 0);
      prev = v;
    }
    REQUIRE((L.n_dd_cols[g] != 0) == (L.cls_n[g ? C_DDG : C_DD] != 0));
  }
  // run records of the dictionary pages: disjoint, inside rec_total
  std::vector<std::pair<uint64_t, uint64_t>> recs;
  for (int k : {(int)C_DICT4, (int)C_DICT8, (int)C_IDS, (int)C_DD, (int)C_DDG})
    for (int i = 0; i < L.cls_n[k]; i++) {
      const PageWork& w = L.h_work[(size_t)L.flat[(size_t)(L.cls_off[k] + i)]];
      recs.push_back({w.rec_base, w.rec_base + std::min(w.num_slots, w.size) + 1});
      REQUIRE(w.chunk_base <= L.chunk_total);
    }
  std::sort(recs.begin(), recs.end());
  for (size_t i = 0; i < recs.size(); i++) {
    REQUIRE(recs[i].second <= L.rec_total);
    REQUIRE(i == 0 || recs[i - 1].second <= recs[i].first);
  }
  // tails: the lists of a plain_fused launch are prefixes of the full ones, split at the one-pass columns
  REQUIRE(L.n_bin_cols_nf >= 0 && L.n_bin_cols_nf <= L.n_bin_cols && L.n_bin_blocks_nf <= L.n_bin_blocks &&
          L.n_bin_chunks_nf <= L.n_bin_chunks);
  std::vector<int> one_pass((size_t)std::max(n_cols, 1), 0);
  for (int p : L.pcp) one_pass[(size_t)L.h_work[(size_t)p].column] = 1;
  for (int i = 0; i < L.n_bin_cols; i++) REQUIRE(one_pass[(size_t)L.bl[(size_t)(L.off_bin_cols + i)]] == (i >= L.n_bin_cols_nf));
  for (uint32_t i = 0; i < L.n_bin_blocks; i++) REQUIRE(one_pass[(size_t)(L.bin_blocks[i] >> 32)] == (i >= L.n_bin_blocks_nf));
  for (uint32_t i = 0; i < L.n_bin_chunks; i++)
    REQUIRE(one_pass[(size_t)L.h_work[(size_t)(uint32_t)L.bin_chunks[i]].column] == (i >= L.n_bin_chunks_nf));
  // kernel count: the split dictionary mode and the level-first order never run fewer kernels
  for (int pf = 0; pf < 2; pf++)
    for (int b = 0; b < 2; b++) {
      REQUIRE(plan_kernel_count(L, pf, false, b) >= plan_kernel_count(L, pf, true, b));
      REQUIRE(plan_kernel_count(L, pf, b, false) >= plan_kernel_count(L, pf, b, true));
      REQUIRE(plan_kernel_count(L, pf, b, b) >= 0);
    }
}

// ---- the cases
const int kTypes[] = {PQG_BOOLEAN, PQG_INT32, PQG_INT64, PQG_INT96, PQG_FLOAT, PQG_DOUBLE, PQG_BYTE_ARRAY, PQG_FIXED_LEN_BYTE_ARRAY};
const int kEncodings[] = {PQG_PLAIN, PQG_PLAIN_DICTIONARY, PQG_RLE, PQG_BIT_PACKED, PQG_DELTA_BINARY_PACKED,
                          PQG_DELTA_LENGTH_BYTE_ARRAY, PQG_DELTA_BYTE_ARRAY, PQG_RLE_DICTIONARY, PQG_BYTE_STREAM_SPLIT, 77};

const ColumnDev& col0(const PlanLayout& L) { return L.cols[0]; }
#define EXPECT(cond) do { if (!(cond)) fail("expectation", #cond); } while (0)

std::vector<Case> build_cases() {
  std::vector<Case> out;
  auto add = [&](const char* name) -> Case& {
    out.emplace_back();
    out.back().name = name;
    return out.back();
  };
  // empty and degenerate tables
  add("empty");
  { Case& c = add("cols_no_pages"); c.col(PQG_INT32); c.col(PQG_BYTE_ARRAY, 0, 1); }
  {
    Case& c = add("col_without_pages");
    c.col(PQG_INT64);
    const int b = c.col(PQG_BYTE_ARRAY);
    c.page(b, PQG_PLAIN, 10, 100);
  }
  {
    Case& c = add("binary_zero_slots");  // the empty_bin_values path
    const int b = c.col(PQG_BYTE_ARRAY);
    c.page(b, PQG_DELTA_LENGTH_BYTE_ARRAY, 0, 16);
    c.check = [](const PlanLayout& L) { EXPECT(L.empty_bin_values.size() == 1 && L.n_bin_blocks == 0); };
  }
  // every physical type x every encoding (required and nullable V2 columns), with and without a dictionary
  for (int t : kTypes)
    for (int e : kEncodings)
      for (int variant = 0; variant < 3; variant++) {
        char name[64];
        std::snprintf(name, sizeof(name), "type%d_enc%d_%s", t, e, variant == 0 ? "req" : variant == 1 ? "nodict" : "opt_v2");
        Case& c = add(name);
        const int ci = c.col(t, t == PQG_FIXED_LEN_BYTE_ARRAY ? 6 : 0, variant == 2 ? 1 : 0);
        if (variant != 1) c.dict(ci, 10, 200);
        c.page(ci, e, 100, 1000, variant == 2 ? 2 : 1).dl_byte_length = variant == 2 ? 20 : 0;
        c.page(ci, e, 33, 500, variant == 2 ? 2 : 1).dl_byte_length = variant == 2 ? 8 : 0;
      }
  for (int tl : {4, 8, 16}) {  // FIXED_LEN_BYTE_ARRAY dictionaries of 4 / 8 bytes take the fixed-width classes
    Case& c = add(tl == 4 ? "flba4_dict" : tl == 8 ? "flba8_dict" : "flba16_dict");
    const int ci = c.col(PQG_FIXED_LEN_BYTE_ARRAY, tl);
    c.dict(ci, 10, 200);
    c.page(ci, PQG_RLE_DICTIONARY, 5000, 900);
    c.check = [tl](const PlanLayout& L) { EXPECT(L.page_cls[0] == (tl == 4 ? C_DICT4 : tl == 8 ? C_DICT8 : C_IDS)); };
  }
  // dictionary-id columns
  for (int k = 0; k < 3; k++) {
    Case& c = add(k == 0 ? "ids_dict_page" : k == 1 ? "ids_plain_page" : "ids_no_dictionary");
    const int ci = c.col(PQG_BYTE_ARRAY, 0, 1);
    c.cols[(size_t)ci].flags = PQG_COLUMN_DICTIONARY_IDS;
    if (k != 2) c.dict(ci, 50, 400);
    c.page(ci, k == 1 ? PQG_PLAIN : PQG_RLE_DICTIONARY, 1000, 700);
    c.page(ci, PQG_PLAIN_DICTIONARY, 10, 70);
    c.check = [k](const PlanLayout& L) { EXPECT(L.host_errs.size() == (k == 0 ? 0u : k == 1 ? 1u : 2u)); };
  }
  // column errors (reported at the column's first page)
  {
    Case& c = add("colerr_dict_encoding");
    const int ci = c.col(PQG_INT32);
    c.dict(ci, 10, 40, PQG_RLE);
    c.page(ci, PQG_RLE_DICTIONARY, 100, 90);
    c.page(ci, PQG_PLAIN, 100, 400);
    c.check = [](const PlanLayout& L) { EXPECT(L.host_errs.size() == 1 && L.host_errs[0].code == PQG_ERR_DICT_ENCODING); };
  }
  {
    Case& c = add("colerr_boolean_dictionary");
    const int ci = c.col(PQG_BOOLEAN);
    c.dict(ci, 2, 2);
    c.page(ci, PQG_PLAIN, 100, 13);
  }
  {
    Case& c = add("colerr_flba_length0");
    const int ci = c.col(PQG_FIXED_LEN_BYTE_ARRAY, 0);
    c.dict(ci, 2, 20);
    c.page(ci, PQG_PLAIN, 100, 13);
    c.check = [](const PlanLayout& L) { EXPECT(L.host_errs.size() == 1 && L.host_errs[0].code == PQG_ERR_CORRUPT); };
  }
  {
    Case& c = add("colerr_flba_length_negative");
    const int ci = c.col(PQG_FIXED_LEN_BYTE_ARRAY, -3);
    c.page(ci, PQG_PLAIN, 100, 13);
    c.page(ci, PQG_DELTA_BYTE_ARRAY, 100, 13);
    c.page(ci, PQG_BYTE_STREAM_SPLIT, 100, 13);
  }
  {
    Case& c = add("colerr_dict_past_end");
    const int ci = c.col(PQG_INT64);
    c.page(ci, PQG_RLE_DICTIONARY, 100, 90);
    c.dict(ci, 10, 80);
    c.cols[(size_t)ci].dict_offset += 16;  // its last 16 bytes lie past valid_bytes
    c.check = [](const PlanLayout& L) { EXPECT(L.host_errs.size() == 1 && L.host_errs[0].code == PQG_ERR_INVALID_ARG); };
  }
  {
    Case& c = add("colerr_dict_offset_huge");  // dict_offset + dict_size near 2^63: no wrap (int64 >= 0 plus uint32)
    const int ci = c.col(PQG_INT64);
    c.page(ci, PQG_RLE_DICTIONARY, 100, 90);
    c.cols[(size_t)ci].dict_offset = INT64_MAX;
    c.cols[(size_t)ci].dict_size = 0xFFFFFFFFu;
    c.cols[(size_t)ci].dict_num_values = 1;
    c.check = [](const PlanLayout& L) { EXPECT(L.host_errs.size() == 1 && L.host_errs[0].code == PQG_ERR_INVALID_ARG); };
  }
  {
    Case& c = add("colerr_dict_values_past_size");
    const int ci = c.col(PQG_DOUBLE);
    c.dict(ci, 11, 80);
    c.page(ci, PQG_RLE_DICTIONARY, 100, 90);
    c.check = [](const PlanLayout& L) { EXPECT(L.host_errs.size() == 1 && L.host_errs[0].code == PQG_ERR_EOF); };
  }
  for (int md : {255, -1, 254}) {
    Case& c = add(md == 255 ? "colerr_max_def_255" : md == -1 ? "colerr_max_def_negative" : "max_def_254");
    const int ci = c.col(PQG_INT32, 0, md);
    c.page(ci, PQG_PLAIN, 100, 500);
    c.check = [md](const PlanLayout& L) { EXPECT(L.host_errs.size() == (md == 254 ? 0u : 1u)); };
  }
  {
    Case& c = add("max_rep_255_and_nested");
    c.page(c.col(PQG_INT32, 0, 3, 255), PQG_PLAIN, 100, 500);
    c.page(c.col(PQG_BYTE_ARRAY, 0, 3, 2), PQG_PLAIN, 100, 500);
  }
  // page errors
  {
    Case& c = add("required_v1_bad_level_encoding");
    const int ci = c.col(PQG_INT32);
    c.page(ci, PQG_PLAIN, 10, 40).rl_encoding = PQG_PLAIN;
    c.page(ci, PQG_PLAIN, 10, 40).dl_encoding = PQG_DELTA_BYTE_ARRAY;
    c.page(ci, PQG_PLAIN, 10, 40).dl_encoding = PQG_BIT_PACKED;
    c.check = [](const PlanLayout& L) { EXPECT(L.host_errs.size() == 2 && L.cls_n[C_PLAIN] == 1); };
  }
  {
    Case& c = add("required_v2_levels_past_size");
    const int ci = c.col(PQG_INT32);
    pqg_page_desc& g = c.page(ci, PQG_PLAIN, 10, 40, 2);
    g.rl_byte_length = 30;
    g.dl_byte_length = 11;
    pqg_page_desc& h = c.page(ci, PQG_PLAIN, 10, 40, 2);
    h.rl_byte_length = 0xFFFFFFFFu;  // the sum does not wrap
    h.dl_byte_length = 2;
    c.page(ci, PQG_PLAIN, 10, 40, 2).dl_byte_length = 40;
    c.check = [](const PlanLayout& L) {
      EXPECT(L.host_errs.size() == 2 && L.host_errs[0].code == PQG_ERR_CORRUPT && L.cls_n[C_PLAIN] == 1);
    };
  }
  for (const char* bad : {"refused_column_negative", "refused_column_past_table", "refused_version_0", "refused_version_3",
                          "refused_past_valid_bytes", "refused_offset_wraps"}) {
    Case& c = add(bad);
    const int ci = c.col(PQG_INT32);
    for (int i = 0; i < 3; i++) c.page(ci, PQG_PLAIN, 10, 40);
    pqg_page_desc& g = c.pages[1];
    const std::string n = bad;
    if (n == "refused_column_negative") g.column = -1;
    if (n == "refused_column_past_table") g.column = 1;
    if (n == "refused_version_0") g.version = 0;
    if (n == "refused_version_3") g.version = 3;
    if (n == "refused_past_valid_bytes") g.offset = c.end - 39;
    if (n == "refused_offset_wraps") g.offset = ~0ull - 20;
    c.expect_rc = PQG_ERR_INVALID_ARG;
  }
  // DELTA_BYTE_ARRAY: both types, carry pages after a DELTA_BYTE_ARRAY page and after a PLAIN page
  for (int t : {PQG_BYTE_ARRAY, PQG_FIXED_LEN_BYTE_ARRAY}) {
    Case& c = add(t == PQG_BYTE_ARRAY ? "dba_binary_carry" : "dba_flba_carry");
    const int ci = c.col(t, 7), cj = c.col(t, 7, 1);
    c.page(ci, PQG_DELTA_BYTE_ARRAY, 600, 3000);
    c.page(cj, PQG_DELTA_BYTE_ARRAY, 255, 900).flags = PQG_PAGE_DBA_CARRY;  // a column's first page may carry the flag
    c.page(ci, PQG_DELTA_BYTE_ARRAY, 257, 2000).flags = PQG_PAGE_DBA_CARRY;
    c.page(ci, PQG_PLAIN, 10, 200);
    c.page(ci, PQG_DELTA_BYTE_ARRAY, 10, 200).flags = PQG_PAGE_DBA_CARRY;  // refused: follows a PLAIN page
    c.page(ci, PQG_DELTA_BYTE_ARRAY, 10, 200).flags = PQG_PAGE_DBA_CARRY;  // refused: follows a refused page
    c.page(ci, PQG_DELTA_BYTE_ARRAY, 0, 20);
    c.check = [](const PlanLayout& L) { EXPECT(L.host_errs.size() == 2 && L.n_carry == 2 && L.cls_n[C_DBA] == 4); };
  }
  // null hints
  for (int k = 0; k < 3; k++) {
    Case& c = add(k == 0 ? "null_hints_all" : k == 1 ? "null_hints_one_missing" : "null_hints_nulls_past_values");
    const int ci = c.col(PQG_INT64, 0, 1), cj = c.col(PQG_BYTE_ARRAY, 0, 2, 1), ck = c.col(PQG_FLOAT);
    for (int i = 0; i < 3; i++) {
      pqg_page_desc& g = c.page(i == 1 ? cj : ci, PQG_PLAIN, 100, 900, 2);
      g.rl_byte_length = i == 1 ? 12 : 0;
      g.dl_byte_length = 20;
      g.flags = (k == 1 && i == 2) ? 0 : PQG_PAGE_NULL_COUNT;
      g.num_nulls = (k == 2 && i == 1) ? 101 : 7 * (uint32_t)i;
    }
    c.page(ck, PQG_PLAIN, 10, 40);
    c.check = [k](const PlanLayout& L) { EXPECT(L.null_hints == (k == 0)); if (k == 0) EXPECT(L.h_work[2].out_offset == 100); };
  }
  {
    Case& c = add("null_hints_v1_page");
    const int ci = c.col(PQG_INT32, 0, 1);
    c.page(ci, PQG_PLAIN, 100, 900, 2).flags = PQG_PAGE_NULL_COUNT;
    c.page(ci, PQG_PLAIN, 100, 900, 1).flags = PQG_PAGE_NULL_COUNT;
  }
  {
    Case& c = add("null_hints_levels_past_size");
    const int ci = c.col(PQG_INT32, 0, 1);
    pqg_page_desc& g = c.page(ci, PQG_PLAIN, 100, 900, 2);
    g.flags = PQG_PAGE_NULL_COUNT;
    g.dl_byte_length = 901;
  }
  // dictionary size thresholds of a dictionary-direct BYTE_ARRAY column
  struct DictCase { const char* name; uint32_t n, bytes; uint32_t id_bytes, global; int walk, tiles; };
  const DictCase dict_cases[] = {
      {"dict_256_entries", 256, 2000, 1, 0, 1, 0},       {"dict_257_entries", 257, 2000, 2, 0, 1, 0},
      {"dict_2048_entries", 2048, 16000, 2, 0, 1, 0},    {"dict_2049_entries", 2049, 16000, 2, 1, 0, 1},
      {"dict_65536_entries", 65536, 300000, 2, 1, 0, 1}, {"dict_65537_entries", 65537, 300000, 0, 0, 0, 1},
      {"dict_dd_max_bytes", 100, DD_DICT_MAX, 1, 0, 0, 1}, {"dict_dd_max_bytes_plus_1", 100, DD_DICT_MAX + 1, 2, 1, 0, 1},
      {"dict_dent_min_minus_1", 100, DENT_MIN - 1, 1, 0, 1, 0}, {"dict_dent_min", 100, DENT_MIN, 1, 0, 0, 1},
      {"dict_large_no_entries", 0, DENT_MIN, 1, 0, 1, 0},
  };
  for (const DictCase& d : dict_cases) {
    Case& c = add(d.name);
    const int ci = c.col(PQG_BYTE_ARRAY);
    c.dict(ci, d.n, d.bytes);
    c.page(ci, PQG_RLE_DICTIONARY, 5000, 4000);
    c.page(ci, PQG_PLAIN_DICTIONARY, 4097, 3000);
    c.check = [d](const PlanLayout& L) {
      EXPECT(col0(L).dict_direct == d.id_bytes && col0(L).dd_global == d.global);
      EXPECT(L.n_dict_walk == d.walk && L.n_dent_cols == d.tiles);
      EXPECT(L.cls_n[d.id_bytes == 0 ? C_IDS : d.global ? C_DDG : C_DD] == 2);
    };
  }
  for (uint32_t nv : {0xFFFFFFFEu, 0xFFFFFFFFu}) {  // the largest slot counts a header can carry
    Case& c = add(nv == 0xFFFFFFFEu ? "dict_slots_2p32_minus_2" : "dict_slots_2p32_minus_1");
    const int ci = c.col(PQG_BYTE_ARRAY);
    c.dict(ci, 10, 100);
    c.page(ci, PQG_RLE_DICTIONARY, nv, 4000);
    c.check = [](const PlanLayout& L) { EXPECT(col0(L).dict_direct == 1 && L.cls_n[C_DD] == 1); };
  }
  {
    Case& c = add("dict_binary_mixed_pages");  // not dictionary-direct: a PLAIN page among the dictionary pages
    const int ci = c.col(PQG_BYTE_ARRAY, 0, 1);
    c.dict(ci, 100, DENT_MIN);
    c.page(ci, PQG_RLE_DICTIONARY, 5000, 4000);
    c.page(ci, PQG_PLAIN, 512, 3000);
    c.page(ci, PQG_DELTA_LENGTH_BYTE_ARRAY, 513, 3000);
    c.check = [](const PlanLayout& L) { EXPECT(L.n_bind == 1 && L.n_dent_cols == 1 && L.n_bin_chunks == 10 + 1 + 2); };
  }
  // PLAIN BYTE_ARRAY pages on either side of the segment walk (a column that is not PLAIN-only)
  for (uint32_t bytes : {16384u, 16385u}) {
    Case& c = add(bytes == 16384 ? "plain_binary_16384_bytes" : "plain_binary_16385_bytes");
    const int ci = c.col(PQG_BYTE_ARRAY);
    c.page(ci, PQG_PLAIN, 1000, bytes);
    c.page(ci, PQG_DELTA_LENGTH_BYTE_ARRAY, 10, 100);
    c.check = [bytes](const PlanLayout& L) { EXPECT(L.n_segs == (bytes == 16384 ? 0u : 3u) && L.n_pcp == 0); };
  }
  for (uint32_t bytes : {16384u, 16385u, 0u}) {  // PLAIN-only: the one-pass path
    Case& c = add(bytes == 16384 ? "plain_only_16384_bytes" : bytes ? "plain_only_16385_bytes" : "plain_only_0_bytes");
    const int ci = c.col(PQG_BYTE_ARRAY);
    c.page(ci, PQG_PLAIN, bytes ? 1000 : 0, bytes);
    c.check = [bytes](const PlanLayout& L) {
      EXPECT(L.n_pcp == 1 && L.n_segs == 0 && L.n_psegs == (bytes ? (bytes + BP_TILE - 1) / BP_TILE : 1u));
    };
  }
  for (uint32_t nv : {(1u << 24) - 2u, (1u << 24) - 1u}) {
    Case& c = add(nv == (1u << 24) - 2u ? "plain_only_slots_2p24_minus_2" : "plain_only_slots_2p24_minus_1");
    const int ci = c.col(PQG_BYTE_ARRAY);
    c.page(ci, PQG_PLAIN, nv, 1u << 20);
    c.check = [nv](const PlanLayout& L) { EXPECT(L.n_pcp == (nv == (1u << 24) - 2u ? 1 : 0)); };
  }
  for (uint32_t np : {BW_SEG_MAX_PAGES - 1, BW_SEG_MAX_PAGES}) {
    Case& c = add(np == BW_SEG_MAX_PAGES ? "plain_pages_at_seg_max" : "plain_pages_below_seg_max");
    const int ci = c.col(PQG_BYTE_ARRAY), cj = c.col(PQG_BYTE_ARRAY, 0, 1);
    for (uint32_t i = 0; i + 2 < np; i++) c.page(ci, PQG_PLAIN, 3, 20);
    c.page(cj, PQG_PLAIN, 3, 40000);
    c.page(cj, PQG_DELTA_LENGTH_BYTE_ARRAY, 3, 40);
    c.page(ci, PQG_PLAIN, 3, 20);
    c.check = [np](const PlanLayout& L) {
      EXPECT(L.plain_pg == (np == BW_SEG_MAX_PAGES) && L.n_pcp == (int)np - 1 && (L.n_segs != 0) == (np != BW_SEG_MAX_PAGES));
    };
  }
  // several columns: dictionary-direct columns whose pages interleave, a one-pass column between them
  {
    Case& c = add("interleaved_dict_direct");
    const int a = c.col(PQG_BYTE_ARRAY), p = c.col(PQG_BYTE_ARRAY), b = c.col(PQG_BYTE_ARRAY, 0, 1), g = c.col(PQG_BYTE_ARRAY),
              f = c.col(PQG_INT32), h = c.col(PQG_BYTE_ARRAY);
    c.dict(a, 300, 3000);
    c.dict(b, 20, 150);
    c.dict(g, 3000, 70000);
    c.dict(f, 64, 256);
    c.dict(h, 5, 64);
    for (int i = 0; i < 3; i++) {
      c.page(b, PQG_RLE_DICTIONARY, 4090 + (uint32_t)i * 9000, 2000, 2).dl_byte_length = 100;
      c.page(g, PQG_RLE_DICTIONARY, 70000, 60000);
      c.page(p, PQG_PLAIN, 2000, 30000);
      c.page(a, PQG_PLAIN_DICTIONARY, 4093, 3000);
      c.page(f, PQG_RLE_DICTIONARY, 777, 300);
      c.page(h, i == 1 ? PQG_DELTA_LENGTH_BYTE_ARRAY : PQG_RLE_DICTIONARY, 100, 300);
    }
    c.check = [](const PlanLayout& L) {
      EXPECT(L.n_dd_cols[0] == 2 && L.n_dd_cols[1] == 1 && L.cls_n[C_DD] == 6 && L.cls_n[C_DDG] == 3 && L.n_pcols == 1);
      EXPECT(L.bl[(size_t)L.off_dd_cols[0]] == 0 && L.bl[(size_t)L.off_dd_cols[0] + 1] == 2);  // sorted by column
      EXPECT(L.dd_chunk_n[0] == (3 + 1) + (1 + 4 + 6) && L.cls_n[C_IDS] == 2 && L.n_bind == 2);  // one padding entry
    };
  }
  return out;
}

struct Variant { int plain_mode, dict_direct, null_hints; };

std::vector<Variant> variants() {
  std::vector<Variant> v;
  v.push_back({2, 1, 1});  // the defaults first
  for (int pm = 0; pm < 4; pm++)
    for (int dd = 0; dd < 2; dd++)
      for (int nh = 0; nh < 2; nh++)
        if (!(pm == 2 && dd == 1 && nh == 1)) v.push_back({pm, dd, nh});
  return v;
}

// Runs the planner on exactly-sized heap copies of the tables.
int run(const Case& c, const Variant& v, PlanLayout* L, int* bad_page) {
  const std::vector<pqg_column_desc> cols(c.cols);
  const std::vector<pqg_page_desc> pages(c.pages);
  const PlanOptions opt{v.plain_mode, v.dict_direct != 0, v.null_hints != 0};
  return PLAN_LAYOUT_CALL(c.end + 64, c.end, cols.empty() ? nullptr : cols.data(), (int)cols.size(),
                          pages.empty() ? nullptr : pages.data(), (int)pages.size(), opt, L, bad_page);
}

std::string tag(const Case& c, const Variant& v) {
  char b[32];
  std::snprintf(b, sizeof(b), "/pm%d/dd%d/nh%d", v.plain_mode, v.dict_direct, v.null_hints);
  return c.name + b;
}

enum { NO_DIGEST = 0, DIGEST_HASHED, DIGEST_FULL };

int mode_cases(int digest) {
  const std::vector<Case> cases = build_cases();
  long n = 0, ok = 0, invalid = 0;
  for (const Case& c : cases) {
    std::vector<std::pair<std::string, std::string>> lines;  // digest body, the settings that produced it
    bool first = true;
    for (const Variant& v : variants()) {
      PlanLayout L;
      int bad_page = -2;
      const int rc = run(c, v, &L, &bad_page);
      const std::string where = tag(c, v);
      n++;
      if (rc != c.expect_rc || (rc != PQG_OK && rc != PQG_ERR_INVALID_ARG)) fail(where, "return code");
      if (rc == PQG_OK) {
        ok++;
        if (!digest) check_invariants(where, c, L);  // (the digest mode only prints)
        if (first && c.check) c.check(L);
      } else {
        invalid++;
        if (bad_page != 1) fail(where, "refused page");  // (every refusal case spoils its page 1)
      }
      first = false;
      if (digest) {
        char head[48], setting[8];
        std::snprintf(head, sizeof(head), " rc=%d bad_page=%d |", rc, bad_page);
        std::snprintf(setting, sizeof(setting), "%d%d%d", v.plain_mode, v.dict_direct, v.null_hints);
        std::string body = head;
        if (rc == PQG_OK) {
          body += plan_digest::line(L) + " | kernels";  // plan_kernel_count in every mode combination
          for (int m = 0; m < 8; m++) body += " " + std::to_string(plan_kernel_count(L, m & 4, m & 2, m & 1));
        }
        auto it = std::find_if(lines.begin(), lines.end(), [&](const auto& l) { return l.first == body; });
        if (it == lines.end()) lines.push_back({body, setting});
        else it->second += std::string(",") + setting;
      }
    }
    // the settings (plain_mode, dict_direct, null_hints) that give each distinct result
    if (digest == DIGEST_FULL)
      for (const auto& l : lines) std::printf("%s %s%s\n", c.name.c_str(), l.second.c_str(), l.first.c_str());
    if (digest == DIGEST_HASHED) {
      std::printf("%s rc=%d", c.name.c_str(), c.expect_rc);
      for (const auto& l : lines)
        std::printf(" %s=%016llx", l.second.c_str(), (unsigned long long)plan_digest::fnv(l.first.data(), l.first.size()));
      std::printf("\n");
    }
  }
  std::printf("cases=%ld ok=%ld invalid=%ld\n", n, ok, invalid);
  return 0;
}

// ---- fuzz: deterministic single-field mutations of the small cases
struct Field { size_t off, size; };
#define FIELD(T, f) Field{offsetof(T, f), sizeof(((T*)0)->f)}
const Field kPageFields[] = {FIELD(pqg_page_desc, offset), FIELD(pqg_page_desc, size), FIELD(pqg_page_desc, num_values),
                             FIELD(pqg_page_desc, column), FIELD(pqg_page_desc, version), FIELD(pqg_page_desc, encoding),
                             FIELD(pqg_page_desc, rl_encoding), FIELD(pqg_page_desc, dl_encoding),
                             FIELD(pqg_page_desc, rl_byte_length), FIELD(pqg_page_desc, dl_byte_length),
                             FIELD(pqg_page_desc, flags), FIELD(pqg_page_desc, num_nulls)};
const Field kColFields[] = {FIELD(pqg_column_desc, physical_type), FIELD(pqg_column_desc, type_length),
                            FIELD(pqg_column_desc, max_rep), FIELD(pqg_column_desc, max_def),
                            FIELD(pqg_column_desc, dict_offset), FIELD(pqg_column_desc, dict_size),
                            FIELD(pqg_column_desc, dict_num_values), FIELD(pqg_column_desc, dict_encoding),
                            FIELD(pqg_column_desc, flags), FIELD(pqg_column_desc, values),
                            FIELD(pqg_column_desc, binary_capacity)};

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() {  // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

void mutate(void* rec, const Field& f, uint64_t how) {
  uint64_t v = 0;
  std::memcpy(&v, (char*)rec + f.off, f.size);
  switch (how % 4) {
    case 0: v = 0; break;
    case 1: v = ~0ull; break;
    default: v ^= 1ull << ((how >> 2) % (8 * f.size)); break;  // (bit flips: half of the mutations)
  }
  std::memcpy((char*)rec + f.off, &v, f.size);
}

int mode_fuzz(long N) {
  std::vector<Case> small;
  for (const Case& c : build_cases())
    if (!c.pages.empty() && c.pages.size() <= 8 && c.expect_rc == PQG_OK) small.push_back(c);
  const std::vector<Variant> vs = variants();
  long ok = 0, invalid = 0;
  for (long it = 0; it < N; it++) {
    Case c = small[rnd() % small.size()];
    const Variant v = vs[rnd() % vs.size()];
    const bool full_range = it < 12;  // a fixed dozen keep the whole 32-bit range of num_values / size
    if (full_range) {
      pqg_page_desc& g = c.pages[rnd() % c.pages.size()];
      // size / num_values, six each: all ones three times (on different pages), and bit 31, 26 or 21 flipped
      const long j = it / 2;
      mutate(&g, kPageFields[1 + it % 2], j % 2 == 0 ? 1 : 2 + 4 * (uint64_t)(31 - 5 * (j / 2)));
      if (it % 2 == 0) c.end = std::max<uint64_t>(c.end, g.offset + g.size);  // (so that the larger size is accepted)
    } else if (rnd() % 10 < 6 || c.cols.empty()) {  // 60 % page descriptors
      mutate(&c.pages[rnd() % c.pages.size()], kPageFields[rnd() % (sizeof(kPageFields) / sizeof(Field))], rnd());
    } else {
      mutate(&c.cols[rnd() % c.cols.size()], kColFields[rnd() % (sizeof(kColFields) / sizeof(Field))], rnd());
    }
    if (!full_range)
      for (pqg_page_desc& g : c.pages) {  // bounded host vectors
        g.num_values &= (1u << 20) - 1;
        g.size &= (1u << 20) - 1;
      }
    PlanLayout L;
    int bad_page = -2;
    const int rc = run(c, v, &L, &bad_page);
    char where[64];
    std::snprintf(where, sizeof(where), "mutation %ld of %s", it, tag(c, v).c_str());
    if (rc == PQG_OK) {
      ok++;
      check_invariants(where, c, L);
    } else if (rc == PQG_ERR_INVALID_ARG) {
      invalid++;
      if (bad_page < 0 || bad_page >= (int)c.pages.size()) fail(where, "refused page");
    } else {
      fail(where, "return code");
    }
  }
  std::printf("cases=%ld ok=%ld invalid=%ld\n", N, ok, invalid);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "cases") return mode_cases(NO_DIGEST);
  if (mode == "digest") return mode_cases(DIGEST_HASHED);
  if (mode == "digest-full") return mode_cases(DIGEST_FULL);
  if (mode == "fuzz" && argc > 2) return mode_fuzz(std::atol(argv[2]));
  std::fprintf(stderr, "usage: plan_layout cases | digest | digest-full | fuzz N\n");
  return 2;
}
