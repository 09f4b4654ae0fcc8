// pqgpu_plan_host.cpp — the planner of pqg_plan_create (pqgpu_plan.h): descriptor validation, page
// classification, work lists and the scratch layout. Plain C++: no HIP, no device, and the output pointers
// of the descriptors are copied but never dereferenced (tests/c/plan_layout.cpp drives it under
// AddressSanitizer + UndefinedBehaviorSanitizer).
#include "pqgpu_plan.h"

#include <algorithm>
#include <cstring>

namespace pqg {

namespace {

// The layout under construction and what only the planner needs of it. Sized for max(n_cols, 1) /
// max(n_pages, 1) like the tables themselves.
struct Planner {
  const uint64_t valid_bytes;
  const pqg_column_desc* const cols;
  const int n_cols;
  const pqg_page_desc* const pages;
  const int n_pages;
  const PlanOptions opt;
  PlanLayout& L;

  const size_t nc, np;
  std::vector<int> col_err;
  std::vector<std::vector<int>> cls_lists;
  std::vector<int> lvl_list;
  std::vector<std::vector<int>> col_pages;      // nullable columns' pages (k_scan_offsets)
  std::vector<std::vector<int>> col_all_pages;  // every column's pages, in page order
  std::vector<uint64_t> slot_acc, val_acc;
  // per column: FIXED_LEN_BYTE_ARRAY with DELTA_BYTE_ARRAY pages, any carry page
  std::vector<uint8_t> dba_fixed, dba_carry;
  std::vector<uint8_t> plain_col, dict_direct, dd_glob, seg_page;
  std::vector<int32_t> dict_walk, bind, fixd, bin_cols, carry_cols, dent_cols, dent_start;
  std::vector<int32_t> dd_cols[2], dd_start[2];
  uint64_t sc = 0;  // bytes of bscratch taken so far

  Planner(uint64_t valid_bytes_, const pqg_column_desc* cols_, int n_cols_, const pqg_page_desc* pages_, int n_pages_,
          const PlanOptions& opt_, PlanLayout& L_)
      : valid_bytes(valid_bytes_), cols(cols_), n_cols(n_cols_), pages(pages_), n_pages(n_pages_), opt(opt_), L(L_),
        nc((size_t)std::max(n_cols_, 1)), np((size_t)std::max(n_pages_, 1)), col_err(nc, 0), cls_lists(C_NCLS),
        col_pages(nc), col_all_pages(nc), slot_acc(nc, 0), val_acc(nc, 0), dba_fixed(nc, 0), dba_carry(nc, 0),
        plain_col(nc, 0), dict_direct(nc, 0), dd_glob(nc, 0), seg_page(np, 0) {}

  // ---- bscratch regions. Every region starts 256-byte aligned, in the order it is taken here.
  //
  // Cleared before every launch (CLEAR_LAUNCH; blen_bytes_nf ends after the last of them):
  //   blen          per-value lengths / dictionary ids of the columns outside the one-pass PLAIN path
  //   seg_status    k_bin_walk_seg's status words + ticket
  //   pticket       k_bin_plain's ticket
  // Cleared before a launch on the per-value PLAIN path only (CLEAR_PER_VALUE; blen_bytes ends after them):
  //   blen          of the one-pass PLAIN columns (k_bin_bases / k_bin_plain do not touch it)
  // Epoch-tagged (CLEAR_EPOCH: zeroed at plan creation and when the error epoch wraps):
  //   pflag         k_bin_plain / k_bin_plain_pg store the launch's epoch when a page is inexact
  //   hint          k_levels stores the launch's epoch when a header null count is wrong
  // Never cleared (CLEAR_NEVER), with the kernel that writes each before it is read:
  //   dd_ids        compact ids of dictionary-direct columns: k_dict_fused_dd (split mode: k_dict_tiles_dd)
  //                 writes every slot that k_dd_str / k_dd_gsums / k_dd_gstr read
  //   seg_tmp       k_bin_walk_seg: each segment writes its own lengths and sources before it reads them
  //   dba_prefix    FIXED_LEN_BYTE_ARRAY columns with DELTA_BYTE_ARRAY pages (their ColumnDev::bsrc): the
  //                 prefix lengths, k_delta, before the DELTA_BYTE_ARRAY copy kernels
  //   bsrc          BYTE_ARRAY columns' value sources: k_bin_walk, k_bin_walk_seg, k_delta (DELTA_LENGTH /
  //                 DELTA_BYTE_ARRAY, there the prefix lengths) or k_bin_dict_map, before the offset scan
  //                 and the copies
  //   block_sums    k_bin_block_sums, before k_bin_block_bases / k_bin_offsets
  //   bin_total     k_bin_block_bases (one-pass PLAIN columns: k_bin_bases; dictionary-direct columns:
  //                 k_dd_bases), before pqg_sync reads it
  //   dict_len,     the dictionary's entries: k_bin_walk in dictionary mode, or k_dent_scatter for the
  //   dict_src      dictionaries walked per tile, before any page kernel of the column maps an id. Entries
  //                 past an error in the dictionary page keep whatever the allocation held
  //   dict_ent      k_dent_scatter, before k_dd_gsums (which waits for it). Allocated after the cleared
  //                 prefix, so like dict_len / dict_src it is never zeroed (advisor finding 1, round 6)
  //   dba_meta      k_delta (DELTA_BYTE_ARRAY lengths), before k_dba_tail .. k_dba_chunks
  //   dd_sums       chunk byte sums of the C_DD pages: k_dict_fused_dd / k_dict_tiles_dd, before k_dd_bases
  //   ddg_sums      the same of the C_DDG pages: k_dd_gsums, before k_dd_bases
  //   dent_rec,     k_dent_walk, before k_dent_resolve / k_dent_scatter
  //   dent_scr, dent_tb (dent_tb: k_dent_resolve)
  uint64_t take(const char* name, int column, uint64_t bytes, RegionClear clear) {
    const uint64_t o = sc;
    L.regions.push_back(ScratchRegion{name, column, o, bytes, clear});
    sc = (sc + bytes + 255) & ~uint64_t(255);
    return o;
  }
  // end of the last region cleared at least as often as `clear` (the cleared regions form a prefix)
  uint64_t cleared_end(RegionClear clear) const {
    uint64_t end = 0;
    for (size_t i = 0; i < L.regions.size(); i++)
      if (L.regions[i].clear <= clear) end = i + 1 < L.regions.size() ? L.regions[i + 1].off : sc;
    return end;
  }

  void columns() {
    L.cols.resize(nc);
    L.col_first_page.assign(nc, -1);
    L.col_nullable.assign(nc, 0);
    L.col_required_values.assign(nc, 0);
    for (int i = 0; i < n_cols; i++) {
      const pqg_column_desc& c = cols[i];
      ColumnDev& d = L.cols[(size_t)i];
      std::memset(&d, 0, sizeof(d));
      d.physical_type = c.physical_type;
      d.type_length = c.type_length;
      d.max_rep = c.max_rep;
      d.max_def = c.max_def;
      d.elem_width = elem_width(c.physical_type, c.type_length);
      d.values = c.values;
      d.binary_data = c.binary_data;
      d.binary_capacity = bin_out(c) ? c.binary_capacity : 0;
      d.def_levels = c.max_def > 0 ? c.def_levels : nullptr;
      d.rep_levels = c.max_rep > 0 ? c.rep_levels : nullptr;
      L.col_nullable[(size_t)i] = (c.max_def > 0 || c.max_rep > 0) ? 1 : 0;
      if (c.max_def > 254 || c.max_rep > 254 || c.max_def < 0 || c.max_rep < 0) col_err[(size_t)i] = PQG_ERR_UNSUPPORTED;
      if (c.dict_offset >= 0) {
        // PlainValuesDictionary ctor :47-53 and the typed readers: validated from the descriptor
        if (c.dict_encoding != PQG_PLAIN && c.dict_encoding != PQG_PLAIN_DICTIONARY) {
          col_err[(size_t)i] = PQG_ERR_DICT_ENCODING;
        } else if (c.physical_type == PQG_BOOLEAN) {
          col_err[(size_t)i] = PQG_ERR_UNSUPPORTED;
        } else if (c.physical_type == PQG_FIXED_LEN_BYTE_ARRAY && c.type_length <= 0) {
          col_err[(size_t)i] = PQG_ERR_CORRUPT;  // PlainBinaryDictionary :106 checkArgument(length > 0)
        } else if ((uint64_t)c.dict_offset + c.dict_size > valid_bytes) {  // (no wrap: offset < 2^63, size < 2^32)
          col_err[(size_t)i] = PQG_ERR_INVALID_ARG;
        } else if (d.elem_width > 0 && (uint64_t)c.dict_num_values * (uint64_t)d.elem_width > c.dict_size) {
          col_err[(size_t)i] = PQG_ERR_EOF;
        }
        d.dict_n = c.dict_num_values;
        d.dict_offset = (uint64_t)c.dict_offset;
        d.dict_bytes = c.dict_size;
      }
    }
  }

  // Page descriptors -> PageWork, the level list and one class list per kernel class. false: page
  // *bad_page is refused.
  bool classify_pages(int* bad_page) {
    L.h_work.resize(np);
    L.page_cls.assign(np, -1);
    // per column: class of its previous page (-2: none yet; PQG_PAGE_DBA_CARRY needs a DELTA_BYTE_ARRAY one)
    std::vector<int> col_last_cls(nc, -2);
    for (int p = 0; p < n_pages; p++) {
      const pqg_page_desc& g = pages[p];
      PageWork& w = L.h_work[(size_t)p];
      std::memset(&w, 0, sizeof(w));
      if (g.column < 0 || g.column >= n_cols || g.offset + g.size > valid_bytes || g.offset + g.size < g.offset || (g.version != 1 && g.version != 2)) {
        *bad_page = p;
        return false;
      }
      const int ci = g.column;
      const pqg_column_desc& c = cols[ci];
      if (L.col_first_page[(size_t)ci] < 0) {
        L.col_first_page[(size_t)ci] = p;
        if (col_err[(size_t)ci]) L.host_errs.push_back(HostErr{p, 0, -1, col_err[(size_t)ci]});
      }
      col_all_pages[(size_t)ci].push_back(p);
      w.base = g.offset;
      w.size = g.size;
      w.num_slots = g.num_values;
      w.column = ci;
      w.version = g.version;
      w.rl_encoding = g.rl_encoding;
      w.dl_encoding = g.dl_encoding;
      w.rl_len = g.rl_byte_length;
      w.dl_len = g.dl_byte_length;
      w.pflags = g.flags;
      w.slot_offset = slot_acc[(size_t)ci];
      slot_acc[(size_t)ci] += g.num_values;
      const bool nullable = L.col_nullable[(size_t)ci] != 0;
      if (!nullable) {
        // required column: no level sections are consumed (ZeroIntegerValuesReader / BIT_PACKED
        // width 0 / NullIntIterator), values = header num_values
        if (g.version == 1 && ((g.rl_encoding != PQG_RLE && g.rl_encoding != PQG_BIT_PACKED) ||
                               (g.dl_encoding != PQG_RLE && g.dl_encoding != PQG_BIT_PACKED))) {
          L.host_errs.push_back(HostErr{p, 0, 0, PQG_ERR_UNSUPPORTED});
          continue;
        }
        uint64_t lv = g.version == 2 ? (uint64_t)g.rl_byte_length + g.dl_byte_length : 0;
        if (lv > g.size) {
          L.host_errs.push_back(HostErr{p, 0, 0, PQG_ERR_CORRUPT});
          continue;
        }
        w.data_begin = (uint32_t)lv;
        w.n_values = g.num_values;
        w.out_offset = val_acc[(size_t)ci];
        val_acc[(size_t)ci] += g.num_values;
      } else {
        lvl_list.push_back(p);
        col_pages[(size_t)ci].push_back(p);
      }
      const int last_cls = col_last_cls[(size_t)ci];
      col_last_cls[(size_t)ci] = -1;
      if (col_err[(size_t)ci]) continue;  // dictionary page unusable: ColumnReaderBase ctor threw
      // value class (Encoding.getValuesReader / getDictionaryBasedValuesReader dispatch)
      const int t = c.physical_type;
      const int ew = elem_width(t, c.type_length);
      int cls = -1, herr = 0;
      if (ids_mode(c)) {
        // readValueDictionaryId: dictionary pages give their ids (any physical type, k_dict_fused<4, IDS>
        // writing straight into the column's uint32 values); other readers throw (ValuesReader.java:123-125)
        if (g.encoding != PQG_PLAIN_DICTIONARY && g.encoding != PQG_RLE_DICTIONARY) herr = PQG_ERR_UNSUPPORTED;
        else if (c.dict_offset < 0) herr = PQG_ERR_NO_DICTIONARY;
        else if (t == PQG_BOOLEAN) herr = PQG_ERR_UNSUPPORTED;
        else cls = C_IDS;
      } else
      switch (g.encoding) {
        case PQG_PLAIN_DICTIONARY:
        case PQG_RLE_DICTIONARY:
          if (c.dict_offset < 0) herr = PQG_ERR_NO_DICTIONARY;
          else if (t == PQG_BOOLEAN) herr = PQG_ERR_UNSUPPORTED;
          else if (t == PQG_BYTE_ARRAY) { cls = C_IDS; w.bin_kind = BIN_DICT; }
          else if (ew == 8) cls = C_DICT8;
          else if (ew == 4) cls = C_DICT4;
          else if (ew > 0) cls = C_IDS;      // FLBA / INT96: ids, then k_gather_fixed
          else herr = PQG_ERR_UNSUPPORTED;
          break;
        case PQG_PLAIN:
          if (t == PQG_BOOLEAN) cls = C_BOOL;
          else if (t == PQG_BYTE_ARRAY) { cls = C_BINP; w.bin_kind = BIN_PLAIN; }
          else if (ew > 0) cls = C_PLAIN;
          else herr = PQG_ERR_UNSUPPORTED;
          break;
        case PQG_RLE:  // Encoding.RLE values: BOOLEAN only (getMaxLevel :255-271)
          if (t == PQG_BOOLEAN) cls = C_RLEBOOL;
          else herr = PQG_ERR_UNSUPPORTED;
          break;
        case PQG_DELTA_BINARY_PACKED:
          if (t == PQG_INT64) cls = C_DELTA8;
          else if (t == PQG_INT32) cls = C_DELTA4;
          else herr = PQG_ERR_UNSUPPORTED;
          break;
        case PQG_DELTA_LENGTH_BYTE_ARRAY:
          if (t == PQG_BYTE_ARRAY) { cls = C_DLBA; w.bin_kind = BIN_DLBA; }
          else herr = PQG_ERR_UNSUPPORTED;   // Encoding.java :204-207
          break;
        case PQG_BYTE_STREAM_SPLIT:
          if (t == PQG_FLOAT || t == PQG_DOUBLE || t == PQG_INT32 || t == PQG_INT64 ||
              (t == PQG_FIXED_LEN_BYTE_ARRAY && ew > 0))
            cls = C_BSS;
          else
            herr = PQG_ERR_UNSUPPORTED;      // Encoding.java :130-143
          break;
        case PQG_DELTA_BYTE_ARRAY:
          // Encoding.java :219-222: BYTE_ARRAY and FIXED_LEN_BYTE_ARRAY (whose values must then be
          // type_length bytes each: k_delta reports any other length as PQG_ERR_CORRUPT)
          if (t == PQG_BYTE_ARRAY || (t == PQG_FIXED_LEN_BYTE_ARRAY && ew > 0)) {
            cls = C_DBA;
            w.bin_kind = BIN_DBA;
            if (t == PQG_FIXED_LEN_BYTE_ARRAY) dba_fixed[(size_t)ci] = 1;
            if (g.flags & PQG_PAGE_DBA_CARRY) {
              // setPreviousReader casts the previous page's reader to DeltaByteArrayReader
              if (last_cls != -2 && last_cls != C_DBA) { cls = -1; herr = PQG_ERR_UNSUPPORTED; }
              else dba_carry[(size_t)ci] = 1;
            }
          } else {
            herr = PQG_ERR_UNSUPPORTED;
          }
          break;
        default:
          herr = PQG_ERR_UNSUPPORTED;
      }
      if (herr) {
        L.host_errs.push_back(HostErr{p, 0, 2, herr});
        continue;
      }
      L.page_cls[(size_t)p] = cls;
      col_last_cls[(size_t)ci] = cls;
      cls_lists[(size_t)cls].push_back(p);
    }
    for (int i = 0; i < n_cols; i++) L.col_required_values[(size_t)i] = val_acc[(size_t)i];
    return true;
  }

  // V2 header null counts as a verified hint (PQG_PAGE_NULL_COUNT): only when every nullable page of the
  // plan carries a usable one, so that no value kernel has to wait for k_levels
  void null_hints() {
    if (!opt.null_hints || lvl_list.empty()) return;
    bool all = true;
    for (int p : lvl_list) {
      const pqg_page_desc& g = pages[p];
      all = all && g.version == 2 && (g.flags & PQG_PAGE_NULL_COUNT) && g.num_nulls <= g.num_values &&
            (uint64_t)g.rl_byte_length + g.dl_byte_length <= g.size;
    }
    if (!all) return;
    std::vector<uint64_t> acc(nc, 0);
    for (int p : lvl_list) {  // (page order within each column)
      const pqg_page_desc& g = pages[p];
      PageWork& w = L.h_work[(size_t)p];
      w.n_values = g.num_values - g.num_nulls;
      w.data_begin = g.rl_byte_length + g.dl_byte_length;
      w.out_offset = acc[(size_t)g.column];
      acc[(size_t)g.column] += w.n_values;
    }
    L.null_hints = true;
  }

  // pages of column i that are in class `cls` and have fewer slots than max_slots (default: every page)
  int count_cls(int i, int cls, uint64_t max_slots = ~0ull) const {
    int n = 0;
    for (int p : col_all_pages[(size_t)i])
      n += L.page_cls[(size_t)p] == cls && (uint64_t)L.h_work[(size_t)p].num_slots < max_slots ? 1 : 0;
    return n;
  }

  // PLAIN-only BYTE_ARRAY columns (every page PLAIN, no descriptor error, < 2^24 - 1 slots per page):
  // one pass: k_bin_bases + k_bin_plain over 2 KiB tiles of their pages when the plan has fewer than
  // BW_SEG_MAX_PAGES PLAIN pages, k_bin_plain_pg (one wave per page, which fills the chip) with more
  // (there the tiles measured slower than the per-value walk + copy: C3 10.4 vs 6.4 ms, profiles/r03/plain_ab)
  // pqg_ctx_set_dispatch(PQG_DISPATCH_PLAIN_ONE_PASS) overrides the choice (tests and A/B): 0 = no
  // one-pass path (every plan per value), 3 = every plan one wave per page
  void plain_columns() {
    const int plain_mode = opt.plain_mode;
    const bool many_plain = (cls_lists[C_BINP].size() >= BW_SEG_MAX_PAGES && plain_mode != 1) || plain_mode == 3;
    L.plain_pg = many_plain;
    L.pcs.assign(1, 0);
    for (int i = 0; i < n_cols; i++) {
      const int npg = (int)col_all_pages[(size_t)i].size();
      plain_col[(size_t)i] = bin_out(cols[i]) && !ids_mode(cols[i]) && !col_err[(size_t)i] && !dba_fixed[(size_t)i] &&
                             npg > 0 && count_cls(i, C_BINP, (1u << 24) - 1u) == npg && plain_mode != 0;
      if (!plain_col[(size_t)i]) continue;
      for (int p : col_all_pages[(size_t)i]) {
        L.pcp.push_back(p);
        if (many_plain) continue;
        const uint32_t ntile = std::max<uint32_t>((L.h_work[(size_t)p].size + BP_TILE - 1) / BP_TILE, 1u);
        for (uint32_t k = 0; k < ntile; k++) L.psegs.push_back((uint64_t)(uint32_t)p | ((uint64_t)k << 32));
      }
      L.pcs.push_back((int32_t)L.pcp.size());
    }
    L.n_psegs = (uint32_t)L.psegs.size();
    L.n_pcols = (int)L.pcs.size() - 1;
    L.n_pcp = (int)L.pcp.size();
  }

  // dictionary-direct BYTE_ARRAY columns (ColumnDev::dict_direct): every data page dictionary-encoded,
  // the dictionary page small enough to stage (DD_DICT_MAX bytes, at most 2,048 entries): their pages
  // leave C_IDS for C_DD (no ids stored, no offset scan or copy of their own). Nullable and nested
  // columns too (round 6): the walk decodes a page's n_values ids from its data section, which k_levels
  // (or the V2 header counts) give, and values are indexed by out_offset like every other class.
  // Larger dictionaries (at most 65,536 entries: u16 ids) take C_DDG: their entries and value bytes are
  // gathered from HBM instead of LDS (k_dd_gsums / k_dd_gstr; round 6)
  void dict_direct_columns() {
    for (int i = 0; i < n_cols; i++) {
      const int npg = (int)col_all_pages[(size_t)i].size();
      dict_direct[(size_t)i] = cols[i].physical_type == PQG_BYTE_ARRAY && bin_out(cols[i]) && !ids_mode(cols[i]) &&
                               !col_err[(size_t)i] && !dba_fixed[(size_t)i] && !plain_col[(size_t)i] &&
                               cols[i].dict_offset >= 0 && cols[i].dict_num_values <= 65536 &&
                               npg > 0 && count_cls(i, C_IDS) == npg && opt.dict_direct;
      dd_glob[(size_t)i] = dict_direct[(size_t)i] && (cols[i].dict_size > DD_DICT_MAX || cols[i].dict_num_values > 2048);
    }
    std::vector<int> keep, dd, ddg;
    for (int p : cls_lists[C_IDS]) {
      const int c = L.h_work[(size_t)p].column;
      (!dict_direct[(size_t)c] ? keep : dd_glob[(size_t)c] ? ddg : dd).push_back(p);
    }
    auto by_col = [&](int a, int b) { return L.h_work[(size_t)a].column < L.h_work[(size_t)b].column; };
    std::stable_sort(dd.begin(), dd.end(), by_col);
    std::stable_sort(ddg.begin(), ddg.end(), by_col);
    for (int p : dd) L.page_cls[(size_t)p] = C_DD;
    for (int p : ddg) L.page_cls[(size_t)p] = C_DDG;
    cls_lists[C_IDS].swap(keep);
    cls_lists[C_DD].swap(dd);
    cls_lists[C_DDG].swap(ddg);
    for (int i = 0; i < n_cols; i++) {
      ColumnDev& d = L.cols[(size_t)i];
      d.dict_direct = dict_direct[(size_t)i] ? id_bytes(i) : 0u;
      d.dd_global = dd_glob[(size_t)i];
    }
  }
  // bytes of a dictionary-direct column's compact ids
  uint32_t id_bytes(int i) const { return cols[i].dict_num_values <= 256 && !dd_glob[(size_t)i] ? 1u : 2u; }

  // PLAIN BYTE_ARRAY pages walked in segments when there are few of them (k_bin_walk_seg)
  void plain_segments() {
    if (cls_lists[C_BINP].empty() || cls_lists[C_BINP].size() >= BW_SEG_MAX_PAGES) return;
    for (int p : cls_lists[C_BINP]) {
      const PageWork& w = L.h_work[(size_t)p];
      if (plain_col[(size_t)w.column]) continue;  // one pass (k_bin_plain); the per-value fallback walks per page
      const uint32_t nseg = (w.size + BW_SEG_BYTES - 1) / BW_SEG_BYTES + 1;  // + 1: tile alignment of the start
      if (nseg < 3) continue;
      seg_page[(size_t)p] = 1;
      for (uint32_t k = 0; k < nseg; k++)
        L.segs.push_back((uint64_t)(uint32_t)p | ((uint64_t)k << 32) | (k + 1 == nseg ? (1ull << 63) : 0ull));
    }
    L.n_segs = (uint32_t)L.segs.size();
  }

  // k_bin_copy chunks of the BYTE_ARRAY pages, the post-pass lists of the dictionary pages, and the
  // final order of the C_BINP list
  void copy_chunks() {
    std::vector<uint64_t> plain_chunks;  // copy chunks of the one-pass columns (per-value fallback only)
    for (int k : {C_IDS, C_BINP, C_DLBA})
      for (int p : cls_lists[(size_t)k]) {
        const PageWork& w = L.h_work[(size_t)p];
        if (k == C_BINP && plain_col[(size_t)w.column]) {
          const uint32_t nch = (w.num_slots + CP_CHUNK_VALUES - 1) / CP_CHUNK_VALUES;
          for (uint32_t j = 0; j < nch; j++) plain_chunks.push_back((uint64_t)(uint32_t)p | ((uint64_t)j << 32));
          continue;
        }
        if (k == C_IDS && ids_mode(cols[w.column])) continue;  // the ids are the output
        if (k == C_IDS && dict_direct[(size_t)w.column]) continue;  // the offset scan writes the bytes
        if (k == C_IDS && cols[w.column].physical_type != PQG_BYTE_ARRAY) {
          fixd.push_back(p);
          continue;
        }
        if (k == C_IDS) bind.push_back(p);
        const uint32_t nch = (w.num_slots + CP_CHUNK_VALUES - 1) / CP_CHUNK_VALUES;
        for (uint32_t j = 0; j < nch; j++) L.bin_chunks.push_back((uint64_t)(uint32_t)p | ((uint64_t)j << 32));
      }
    L.n_bin_chunks_nf = (uint32_t)L.bin_chunks.size();
    L.bin_chunks.insert(L.bin_chunks.end(), plain_chunks.begin(), plain_chunks.end());
    L.n_bin_chunks = (uint32_t)L.bin_chunks.size();
    // PLAIN pages: walked by k_bin_walk_seg (not listed), one wave per page, the one-pass columns last
    std::vector<int> keep, tail, seg;
    for (int p : cls_lists[C_BINP]) {
      if (plain_col[(size_t)L.h_work[(size_t)p].column]) tail.push_back(p);
      else if (!seg_page[(size_t)p]) keep.push_back(p);
      else seg.push_back(p);
    }
    L.n_binp_fused = (int)tail.size();
    L.n_binp_seg = (int)seg.size();
    keep.insert(keep.end(), tail.begin(), tail.end());
    keep.insert(keep.end(), seg.begin(), seg.end());
    cls_lists[C_BINP].swap(keep);
  }

  // DELTA_BYTE_ARRAY pages: BIN_CHUNK-value chunks (upper bound from the slot count)
  void dba_chunks() {
    for (int p : cls_lists[C_DBA]) {
      PageWork& w = L.h_work[(size_t)p];
      w.chunk_base = (uint32_t)L.dba_chunks.size();
      w.reserved = 0;
      const uint32_t nch = (w.num_slots + BIN_CHUNK - 1) / BIN_CHUNK;
      for (uint32_t j = 0; j < nch; j++) L.dba_chunks.push_back((uint64_t)(uint32_t)p | ((uint64_t)j << 32));
    }
    L.n_dba_chunks = (uint32_t)L.dba_chunks.size();
    for (int i = 0; i < n_cols; i++)
      if (dba_carry[(size_t)i]) carry_cols.push_back(i);
  }

  // one dictionary page: run-record capacity (a run covers >= 1 value and its header takes >= 1 byte)
  // and output chunks (slots [j*CH, (j+1)*CH) of the page, upper bound from the slot count)
  void dict_page(int p, int ew) {
    PageWork& w = L.h_work[(size_t)p];
    w.rec_base = L.rec_total;
    L.rec_total += (uint64_t)std::min<uint32_t>(w.num_slots, w.size) + 1;
    w.chunk_base = L.chunk_total;
    const uint32_t nch = dict_page_chunks(w.num_slots, ew);
    for (uint32_t j = 0; j < nch; j++) L.chunk_list.push_back((uint64_t)(uint32_t)p | ((uint64_t)j << 32));
    L.chunk_total += nch;
  }

  void dict_chunks() {
    for (int k = C_DICT4; k < C_DICT4 + N_DICT_CLS; k++) {
      L.chunk_off[k - C_DICT4] = (uint32_t)L.chunk_list.size();
      for (int p : cls_lists[(size_t)k]) dict_page(p, k == C_DICT8 ? 8 : 4);
      L.chunk_n[k - C_DICT4] = (uint32_t)L.chunk_list.size() - L.chunk_off[k - C_DICT4];
    }
    for (int g = 0; g < 2; g++) {  // C_DD, then C_DDG
      L.dd_chunk_off[g] = (uint32_t)L.chunk_list.size();
      for (int p : cls_lists[g ? C_DDG : C_DD]) {  // (sorted by column)
        const int column = L.h_work[(size_t)p].column;
        if (dd_cols[g].empty() || dd_cols[g].back() != column) {  // dd_start: [begin, end) of each column's chunks
          if (!dd_cols[g].empty()) dd_start[g].push_back((int32_t)(L.chunk_list.size() - L.dd_chunk_off[g]));
          while ((L.chunk_list.size() - L.dd_chunk_off[g]) % (uint32_t)DICT_WPB) {  // whole workgroups per column
            L.chunk_list.push_back(0xFFFFFFFFull);
            L.chunk_total++;
          }
          dd_cols[g].push_back(column);
          dd_start[g].push_back((int32_t)(L.chunk_list.size() - L.dd_chunk_off[g]));
          const pqg_column_desc& cc = cols[column];
          if (!g)
            L.dd_region = std::max<uint32_t>(L.dd_region, (uint32_t)(((uint64_t)cc.dict_size + 15u) & ~15ull) +
                                                              4u * (uint32_t)cc.dict_num_values);
        }
        dict_page(p, 4);  // ids
      }
      if (!dd_cols[g].empty()) dd_start[g].push_back((int32_t)(L.chunk_list.size() - L.dd_chunk_off[g]));
      L.dd_chunk_n[g] = (uint32_t)L.chunk_list.size() - L.dd_chunk_off[g];
      L.n_dd_cols[g] = (int)dd_cols[g].size();
    }
  }

  // BYTE_ARRAY and fixed-width dictionary columns: the scratch regions, and with them the column lists
  // (dictionary walks, offset-scan columns and blocks) in the same column order
  void scratch_regions() {
    L.blen_off.assign(nc, NO_REGION);
    L.bsrc_off = L.dlen_off = L.dsrc_off = L.dent_off = L.bsum_off = L.bin_total_off = L.blen_off;
    L.bin_capacity.assign(nc, 0);
    std::vector<uint8_t> needs_ids(nc, 0);
    for (int p : cls_lists[C_IDS]) needs_ids[(size_t)L.h_work[(size_t)p].column] = 1;
    // blen first: the part cleared before every launch (with the one-pass columns' last: not cleared
    // while they take the one-pass path)
    for (int pass = 0; pass < 2; pass++) {
      for (int i = 0; i < n_cols; i++) {
        if (ids_mode(cols[i]) || dict_direct[(size_t)i] || (plain_col[(size_t)i] != 0) != (pass == 1))
          continue;  // ids go straight to the values; dictionary-direct columns store none
        if (bin_out(cols[i]) || needs_ids[(size_t)i] || dba_fixed[(size_t)i])
          L.blen_off[(size_t)i] = take("blen", i, 4 * (slot_acc[(size_t)i] + 1), pass ? CLEAR_PER_VALUE : CLEAR_LAUNCH);
      }
      if (pass == 0) {
        if (!L.segs.empty()) L.seg_status_off = take("seg_status", -1, 8 * (L.segs.size() + 1), CLEAR_LAUNCH);  // + the ticket counter
        if (!L.pcp.empty()) L.pticket_off = take("pticket", -1, 8, CLEAR_LAUNCH);
      }
    }
    // dictionary-direct columns: compact ids (u8 for dictionaries of at most 256 entries, else u16), written
    // by k_dict_fused_dd for every slot k_dd_str reads (not cleared; padded: k_dd_str reads whole dwords)
    for (int i = 0; i < n_cols; i++)
      if (dict_direct[(size_t)i]) L.blen_off[(size_t)i] = take("dd_ids", i, id_bytes(i) * (slot_acc[(size_t)i] + 16), CLEAR_NEVER);
    if (!L.pcp.empty()) L.pflag_off = take("pflag", -1, 8, CLEAR_EPOCH);
    if (L.null_hints) L.hint_off = take("hint", -1, 8, CLEAR_EPOCH);
    if (!L.segs.empty()) L.seg_tmp_off = take("seg_tmp", -1, 4 * 2 * (uint64_t)BW_SEG_CAP * L.segs.size(), CLEAR_NEVER);
    for (int i = 0; i < n_cols; i++)
      if (dba_fixed[(size_t)i]) L.bsrc_off[(size_t)i] = take("dba_prefix", i, 4 * (slot_acc[(size_t)i] + 1), CLEAR_NEVER);  // (ColumnDev::bsrc)
    for (int i0 = 0; i0 < 2 * n_cols; i0++) {  // the one-pass columns last
      const int i = i0 % n_cols;
      if (!bin_out(cols[i]) || (plain_col[(size_t)i] != 0) != (i0 >= n_cols)) continue;
      L.bin_capacity[(size_t)i] = cols[i].binary_capacity;
      const uint64_t dict_words = (uint64_t)cols[i].dict_num_values + 1;
      if (dict_direct[(size_t)i]) {  // the byte total (k_dd_bases) and the dictionary's entries only
        L.bin_total_off[(size_t)i] = take("bin_total", i, 8, CLEAR_NEVER);
        // (dictionaries gathered from HBM: always the tile walk, whose scatter also packs their entries)
        ((cols[i].dict_size >= DENT_MIN || dd_glob[(size_t)i]) && cols[i].dict_num_values ? dent_cols : dict_walk)
            .push_back(i);
        if (dd_glob[(size_t)i]) L.dent_off[(size_t)i] = take("dict_ent", i, 8 * dict_words, CLEAR_NEVER);
        L.dlen_off[(size_t)i] = take("dict_len", i, 4 * dict_words, CLEAR_NEVER);
        L.dsrc_off[(size_t)i] = take("dict_src", i, 4 * dict_words, CLEAR_NEVER);
        continue;
      }
      bin_cols.push_back(i);
      L.bsrc_off[(size_t)i] = take("bsrc", i, 4 * (slot_acc[(size_t)i] + 1), CLEAR_NEVER);
      const uint64_t nb = (slot_acc[(size_t)i] + SCAN_BLOCK - 1) / SCAN_BLOCK;
      L.bsum_off[(size_t)i] = take("block_sums", i, 8 * (nb + 1), CLEAR_NEVER);
      L.bin_total_off[(size_t)i] = take("bin_total", i, 8, CLEAR_NEVER);
      for (uint64_t b = 0; b < nb; b++) L.bin_blocks.push_back(((uint64_t)(uint32_t)i << 32) | b);
      if (nb == 0 && cols[i].values) L.empty_bin_values.push_back(cols[i].values);
      if (cols[i].dict_offset >= 0 && !col_err[(size_t)i]) {
        (cols[i].dict_size >= DENT_MIN && cols[i].dict_num_values ? dent_cols : dict_walk).push_back(i);
        L.dlen_off[(size_t)i] = take("dict_len", i, 4 * dict_words, CLEAR_NEVER);
        L.dsrc_off[(size_t)i] = take("dict_src", i, 4 * dict_words, CLEAR_NEVER);
      }
    }
    L.n_bin_blocks = (uint32_t)L.bin_blocks.size();
    // bin_cols / bin_blocks of the one-pass columns form the tails
    for (int c : bin_cols) L.n_bin_cols_nf += plain_col[(size_t)c] ? 0 : 1;
    for (uint64_t b : L.bin_blocks) L.n_bin_blocks_nf += plain_col[(size_t)(b >> 32)] ? 0u : 1u;
    if (!L.dba_chunks.empty()) L.dba_meta_off = take("dba_meta", -1, 8 * L.dba_chunks.size(), CLEAR_NEVER);
    for (int g = 0; g < 2; g++)
      if (L.dd_chunk_n[g]) L.dd_sums_off[g] = take(g ? "ddg_sums" : "dd_sums", -1, 8 * (uint64_t)L.dd_chunk_n[g], CLEAR_NEVER);
    // large BYTE_ARRAY dictionaries: 2 KiB tiles of their pages, per column in dent_cols order
    dent_start.assign(1, 0);
    for (int i : dent_cols) {
      const uint32_t nt = (cols[i].dict_size + DENT_TILE - 1) / DENT_TILE;
      for (uint32_t t = 0; t < nt; t++) L.dent_tiles.push_back((uint64_t)(uint32_t)i | ((uint64_t)t << 32));
      dent_start.push_back((int32_t)L.dent_tiles.size());
    }
    L.n_dent_tiles = (uint32_t)L.dent_tiles.size();
    if (L.n_dent_tiles) {
      L.dent_rec_off = take("dent_rec", -1, 16ull * L.n_dent_tiles, CLEAR_NEVER);
      L.dent_scr_off = take("dent_scr", -1, 2ull * DENT_CAP * L.n_dent_tiles, CLEAR_NEVER);
      L.dent_tb_off = take("dent_tb", -1, 8ull * L.n_dent_tiles, CLEAR_NEVER);
    }
    L.scratch_bytes = sc;
    L.blen_bytes_nf = cleared_end(CLEAR_LAUNCH);
    L.blen_bytes = cleared_end(CLEAR_PER_VALUE);
    // what the kernels need of a column besides its scratch pointers
    for (int i = 0; i < n_cols; i++) {
      ColumnDev& d = L.cols[(size_t)i];
      if (ids_mode(cols[i])) d.blen = (uint32_t*)cols[i].values;  // the ids are the output
      d.n_slots = slot_acc[(size_t)i];
      if (dba_fixed[(size_t)i]) {  // DELTA_BYTE_ARRAY values go straight to the fixed-width output
        d.binary_data = (uint8_t*)cols[i].values;
        d.binary_capacity = slot_acc[(size_t)i] * (uint64_t)d.elem_width;
      }
    }
  }

  static void append(std::vector<int32_t>& to, const std::vector<int32_t>& from, int* off, int* n) {
    *off = (int)to.size();
    if (n) *n = (int)from.size();
    to.insert(to.end(), from.begin(), from.end());
  }

  // flatten the lists: flat = [levels][class 0]...[class n]; cp / cps; bl
  void flatten_lists() {
    L.flat.assign(lvl_list.begin(), lvl_list.end());
    L.levels_off = 0;
    L.levels_n = (int)lvl_list.size();
    for (int k = 0; k < C_NCLS; k++) {
      L.cls_off[k] = (int)L.flat.size();
      L.cls_n[k] = (int)cls_lists[(size_t)k].size();
      L.flat.insert(L.flat.end(), cls_lists[(size_t)k].begin(), cls_lists[(size_t)k].end());
    }
    L.cps.assign(1, 0);
    for (int i = 0; i < n_cols; i++) {
      if (col_pages[(size_t)i].empty()) continue;
      L.cp.insert(L.cp.end(), col_pages[(size_t)i].begin(), col_pages[(size_t)i].end());
      L.cps.push_back((int32_t)L.cp.size());
    }
    L.n_scan_cols = (int)L.cps.size() - 1;
    append(L.bl, dict_walk, &L.off_dict_walk, &L.n_dict_walk);
    append(L.bl, bind, &L.off_bind, &L.n_bind);
    append(L.bl, fixd, &L.off_fixd, &L.n_fixd);
    append(L.bl, bin_cols, &L.off_bin_cols, &L.n_bin_cols);
    append(L.bl, carry_cols, &L.off_carry, &L.n_carry);
    append(L.bl, dent_cols, &L.off_dent_cols, &L.n_dent_cols);
    append(L.bl, dent_start, &L.off_dent_start, nullptr);
    for (int g = 0; g < 2; g++) {
      append(L.bl, dd_cols[g], &L.off_dd_cols[g], nullptr);
      append(L.bl, dd_start[g], &L.off_dd_start[g], nullptr);
    }
  }
};

}  // namespace

int plan_layout(uint64_t n_bytes, uint64_t valid_bytes, const pqg_column_desc* cols, int n_cols,
                const pqg_page_desc* pages, int n_pages, const PlanOptions& opt, PlanLayout* out, int* bad_page) {
  (void)n_bytes;  // the kernels' read bound; every extent is checked against valid_bytes
  if (bad_page) *bad_page = -1;
  if (!out || n_cols < 0 || n_pages < 0 || (n_cols && !cols) || (n_pages && !pages)) return PQG_ERR_INVALID_ARG;
  *out = PlanLayout();
  out->n_cols = n_cols;
  out->n_pages = n_pages;
  Planner P(valid_bytes, cols, n_cols, pages, n_pages, opt, *out);
  int bad = -1;
  P.columns();
  if (!P.classify_pages(&bad)) {
    if (bad_page) *bad_page = bad;
    return PQG_ERR_INVALID_ARG;
  }
  P.null_hints();
  P.plain_columns();
  P.dict_direct_columns();
  P.plain_segments();
  P.copy_chunks();
  P.dba_chunks();
  P.dict_chunks();
  P.scratch_regions();  // (after the chunk lists: dba_meta and the dd_sums regions are sized by them)
  P.flatten_lists();
  return PQG_OK;
}

int plan_kernel_count(const PlanLayout& L, bool plain_fused, bool dict_fused, bool null_hints) {
  const bool pf = plain_fused;
  int k = (L.levels_n ? 1 : 0) + (L.n_scan_cols && !null_hints ? 1 : 0);
  for (int c = 0; c < C_NCLS; c++) {
    const int n = L.cls_n[c] - (c == C_BINP ? L.n_binp_seg + (pf ? L.n_binp_fused : 0) : 0);
    if (n && c == C_DD) k += dict_fused ? 3 : 4;
    else if (n && c == C_DDG) k += dict_fused ? 4 : 5;
    else if (n) k += (c == C_DICT4 || c == C_DICT8 || c == C_IDS) && !dict_fused ? 2 : 1;
  }
  k += (L.n_dict_walk ? 1 : 0) + (L.n_dent_tiles ? 3 : 0) + (L.n_bind ? 1 : 0) + (L.n_fixd ? 1 : 0) +
       ((pf ? L.n_bin_blocks_nf : L.n_bin_blocks) ? 3 : 0) + ((pf ? L.n_bin_chunks_nf : L.n_bin_chunks) ? 1 : 0) +
       (L.cls_n[C_DBA] ? (L.n_dba_chunks ? 4 : 1) : 0) + (L.n_carry ? 1 : 0) + (L.n_segs ? 1 : 0) +
       (pf ? 2 : 0);
  return k;
}

}  // namespace pqg
