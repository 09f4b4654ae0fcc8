// pqgpu_plan.h — the decode plan as plain data: the per-column / per-page records the kernels read, the
// constants that size their work lists, and the layout the planner (pqgpu_plan_host.cpp: descriptor
// validation, page classification, work lists, scratch regions; plain C++, no HIP) computes from the
// caller's descriptors. pqgpu_api.hip allocates, resolves the scratch offsets to pointers and uploads.
#pragma once
#include <stdint.h>

#include <vector>

#include "../../include/pqgpu.h"

namespace pqg {

// Per output column, on the device.
struct ColumnDev {
  int32_t physical_type;
  int32_t type_length;
  int32_t max_rep;
  int32_t max_def;
  int32_t elem_width;   // bytes per dense value
  uint32_t dict_n;      // dictionary entries (0 if none)
  uint64_t dict_offset; // dictionary page body offset in the batch
  uint64_t dict_bytes;  // dictionary page body bytes
  void* values;
  uint8_t* def_levels;
  uint8_t* rep_levels;
  // BYTE_ARRAY columns: `values` = int64 offsets[n_slots + 1] into binary_data; per value
  // scratch: blen (length; dictionary ids of RLE_DICTIONARY pages until k_bin_dict_map) and
  // bsrc (source byte offset relative to the page body, or to the dictionary page body)
  uint8_t* binary_data;
  uint64_t binary_capacity;
  uint32_t* blen;
  uint32_t* bsrc;
  // BYTE_ARRAY dictionary entries (PlainBinaryDictionary): length and offset in the dictionary page
  uint32_t* dict_len;
  uint32_t* dict_src;
  uint64_t n_slots;        // level slots of the column in the batch (offsets span n_slots + 1)
  uint64_t* block_sums;    // BYTE_ARRAY offset scan: per 4096-value block
  uint64_t* bin_total;     // BYTE_ARRAY: bytes of the decoded values (device, one u64)
  // A required BYTE_ARRAY column whose data pages are all dictionary-encoded and whose dictionary page
  // fits DD_DICT_MAX: its pages take launch_dict_dd (compact ids + chunk byte sums, scan, offsets and
  // bytes); dict_direct = the bytes of its ids in blen (1: u8, 2: u16), 0 for every other column.
  // dd_global: a dictionary too large to stage in LDS (over DD_DICT_MAX bytes or 2,048 entries, at most
  // 65,536 entries: u16 ids): entries and value bytes are gathered from HBM (k_dd_gsums, k_dd_gstr)
  uint32_t dict_direct;
  uint32_t dd_global;
  uint64_t* dict_ent;  // dd_global: entry i = source << 32 | length (k_dent_scatter), one gather per value
};
static_assert(sizeof(ColumnDev) == 152, "ColumnDev layout");

// Per page, on the device. The host fills the descriptor facts; for nullable
// columns k_levels fills data_begin / n_values and k_scan_offsets fills out_offset (or, in a plan
// running on V2 header null counts, the host fills them too and k_levels verifies them).
struct PageWork {
  uint64_t base;        // page body offset in the batch
  uint32_t size;        // page body bytes
  uint32_t num_slots;   // header num_values
  uint32_t data_begin;  // data section start (page-relative)
  uint32_t n_values;    // non-null values to decode
  uint64_t out_offset;  // first dense value index of the page in its column
  uint64_t slot_offset; // first level slot of the page in its column
  int32_t column;
  int32_t version;
  int32_t rl_encoding;
  int32_t dl_encoding;
  uint32_t rl_len;      // V2
  uint32_t dl_len;      // V2
  // dictionary pages: run records (walk -> tiles)
  uint64_t rec_base;    // first run record of the page
  uint32_t chunk_base;  // first output chunk of the page
  uint32_t aux;         // DELTA_LENGTH_BYTE_ARRAY: start of the value bytes (end of the length stream)
  uint32_t bin_kind;    // BYTE_ARRAY pages: BIN_PLAIN / BIN_DLBA / BIN_DICT (source of the value bytes)
  uint32_t reserved;    // DELTA_BYTE_ARRAY (set by k_delta): 0 chunk-parallel copy, 1 serial copy, 2 carry chain
  uint32_t pflags;      // pqg_page_desc.flags (PQG_PAGE_DBA_CARRY)
  uint32_t pad0;
  uint64_t bin_base;    // PLAIN-only BYTE_ARRAY columns (k_bin_bases): value bytes of the column's earlier pages
};
static_assert(sizeof(PageWork) == 104, "PageWork layout");

enum BinKind : uint32_t { BIN_PLAIN = 0, BIN_DLBA = 1, BIN_DICT = 2, BIN_DBA = 3 };

// Output chunk of the dictionary expansion (k_dict_tiles / dict_tiles_body): DICT_CHUNK_TILES x 64 lanes x 16 bytes.
constexpr uint32_t DICT_CHUNK_TILES = 16;
inline uint32_t dict_chunk_values(int elem_width) { return DICT_CHUNK_TILES * 64u * (16u / (uint32_t)elem_width); }
// output chunks of a dictionary page of n slots (slots shifted by up to 16 / width - 1 for 16-B alignment)
inline uint32_t dict_page_chunks(uint32_t n, int elem_width) {
  const uint32_t ch = dict_chunk_values(elem_width);
  return (uint32_t)(((uint64_t)n + (uint32_t)(16 / elem_width) - 1 + ch - 1) / ch);
}
constexpr int DICT_WPB = 4;  // pages (walkers) / chunks (tiles) per workgroup of the dictionary kernels

constexpr uint32_t BIN_CHUNK = 256;     // values per DELTA_BYTE_ARRAY copy chunk
// values per k_bin_copy chunk (one workgroup); A/B on C3 / str_plain / str_dict / C4 (profiles/r03/copy_ab):
// 512 beats 256 (C3 copy 3.65 vs 4.21 ms) and 1,024 (C3 5.73 ms, str_dict 0.80 vs 0.44 ms)
constexpr uint32_t CP_CHUNK_VALUES = 512;
// PLAIN BYTE_ARRAY pages walked in segments of BW_SEG_BYTES (k_bin_walk_seg) when a plan has fewer
// than BW_SEG_MAX_PAGES such pages; BW_SEG_CAP values of scratch per segment (len + src)
constexpr uint32_t BW_SEG_BYTES = 16384;
constexpr uint32_t BW_SEG_CAP = BW_SEG_BYTES / 4 + 2;
constexpr uint32_t BW_SEG_MAX_PAGES = 4096;
constexpr uint32_t SCAN_BLOCK = 4096;   // values per offset-scan block
// dictionary page bytes staged by k_dd_str (dict_direct): 32 KiB since round 5 (8 KiB before; the suite's
// str_dict dictionary, 1,000 entries of 4-32 bytes in 22 KB, then took the per-value path: 0.667 ms, now
// 0.347 ms, profiles/r05/dd32k; k_dd_str's LDS at 32 KiB + the entry table: 4 workgroups per CU)
constexpr uint32_t DD_DICT_MAX = 32768;
constexpr uint32_t DD_ENT_MAX = 2048;  // entries of a dictionary page of at most DD_DICT_MAX bytes (4-byte lengths)
// BYTE_ARRAY dictionary pages of at least DENT_MIN bytes: entries walked per 2 KiB tile in parallel
// (k_dent_walk, k_dent_resolve, k_dent_scatter) instead of one wave per page. tiles: column | tile << 32
// (in column order; dictionary dcols[i]'s tiles are [dstart[i], dstart[i + 1])); scratch per tile: rec
// 16 bytes, scr BW_CAP u16, tb 8 bytes
constexpr uint32_t DENT_MIN = 16384;
constexpr uint32_t DENT_TILE = 2048;
constexpr uint32_t DENT_CAP = DENT_TILE / 4;
constexpr uint32_t BP_TILE = 2048;  // bytes per tile of the one-pass PLAIN BYTE_ARRAY kernel (k_bin_plain)

inline int elem_width(int t, int tl) {
  switch (t) {
    case PQG_BOOLEAN: return 1;
    case PQG_INT32: case PQG_FLOAT: return 4;
    case PQG_INT64: case PQG_DOUBLE: return 8;
    case PQG_INT96: return 12;
    case PQG_FIXED_LEN_BYTE_ARRAY: return tl;
    default: return 0;
  }
}

// PQG_COLUMN_DICTIONARY_IDS columns write uint32 ids; BYTE_ARRAY columns otherwise write offsets + bytes
inline bool ids_mode(const pqg_column_desc& c) { return (c.flags & PQG_COLUMN_DICTIONARY_IDS) != 0; }
inline bool bin_out(const pqg_column_desc& c) { return c.physical_type == PQG_BYTE_ARRAY && !ids_mode(c); }
inline int out_width(const pqg_column_desc& c) { return ids_mode(c) ? 4 : elem_width(c.physical_type, c.type_length); }

// Kernel classes, in launch order after the level pass.
//   C_IDS   dictionary pages whose values are not 4 / 8 bytes (BYTE_ARRAY, FLBA, INT96): ids first
//   C_BINP  PLAIN BYTE_ARRAY          C_DLBA  DELTA_LENGTH_BYTE_ARRAY      C_BSS  BYTE_STREAM_SPLIT
//   C_DBA   DELTA_BYTE_ARRAY (lengths here; values by k_dba_copy after the offset scan)
//   C_DD    dictionary pages of dictionary-direct BYTE_ARRAY columns (ColumnDev::dict_direct): walk + chunk
//           byte sums, per-column scan, offsets + value bytes (launch_dict_dd), no ids stored
//   C_DDG   the same for dictionary-direct columns whose dictionary is gathered from HBM (ColumnDev::dd_global)
enum Cls { C_DICT4 = 0, C_DICT8, C_IDS, C_PLAIN, C_BOOL, C_DELTA4, C_DELTA8, C_BSS, C_BINP, C_DLBA, C_DBA, C_RLEBOOL, C_DD,
           C_DDG, C_NCLS };
constexpr int N_DICT_CLS = 3;  // C_DICT4, C_DICT8, C_IDS: run-record walk + chunk expansion

// Error words (pqg::ErrCount, pqgpu_internal.h): (launch epoch << 48) | (~key & ERR_KEY_MASK), epochs
// 1..ERR_EPOCH_MAX
constexpr uint32_t ERR_EPOCH_MAX = 0xFFFFu;
constexpr uint64_t ERR_KEY_MASK = (1ull << 48) - 1;

struct HostErr {
  int page;
  int kind;  // 0 init, 2 value
  int64_t index;
  int code;
};

// The pqg_ctx dispatch values the planner reads (pqg_ctx_set_dispatch); it reads nothing else of the ctx.
struct PlanOptions {
  int plain_mode;    // PQG_DISPATCH_PLAIN_ONE_PASS
  bool dict_direct;  // PQG_DISPATCH_DICT_DIRECT
  bool null_hints;   // PQG_DISPATCH_NULL_HINTS
};

constexpr uint64_t NO_REGION = ~0ull;

// How a region of the plan's scratch buffer (bscratch) gets its initial state in a launch. The two
// cleared kinds are laid out first, in this order, so the part cleared before a launch is a prefix of
// the buffer:
//   CLEAR_LAUNCH      zeroed before every launch (blen_bytes_nf covers exactly these)
//   CLEAR_PER_VALUE   zeroed before a launch on the per-value PLAIN path only (plain_fused off:
//                     blen_bytes covers these too); the one-pass kernels do not read them
//   CLEAR_EPOCH       zeroed at plan creation and when the error epoch wraps; compared against the epoch
//   CLEAR_NEVER       never zeroed: a kernel of the launch writes every word that a later one reads
enum RegionClear : uint8_t { CLEAR_LAUNCH = 0, CLEAR_PER_VALUE, CLEAR_EPOCH, CLEAR_NEVER };

struct ScratchRegion {
  const char* name;
  int column;  // -1: one per plan
  uint64_t off, bytes;
  RegionClear clear;
};

// Everything plan creation computes from the descriptors before it touches the device.
struct PlanLayout {
  int n_pages = 0, n_cols = 0;
  // ---- tables that are uploaded as they are (cols: after its scratch pointers are resolved)
  std::vector<PageWork> h_work;
  std::vector<ColumnDev> cols;
  std::vector<int32_t> flat;       // page lists: [levels][class 0]...[class n]
  std::vector<int32_t> cp, cps;    // nullable columns' pages by column (k_scan_offsets) and their starts
  // bin_lists: [dictionary walks (columns)][BYTE_ARRAY dictionary pages][FLBA/INT96 dictionary pages]
  // [BYTE_ARRAY columns][carry columns][large-dictionary columns][their tile starts][C_DD columns][their
  // chunk ranges][C_DDG columns][their chunk ranges]
  std::vector<int32_t> bl;
  std::vector<uint64_t> bin_blocks, bin_chunks, dba_chunks;  // column << 32 | block; page | chunk << 32
  std::vector<uint64_t> segs;        // PLAIN BYTE_ARRAY segments (k_bin_walk_seg): page | s << 32 | last << 63
  std::vector<uint64_t> dent_tiles;  // large dictionaries: column | tile << 32
  std::vector<uint64_t> psegs;       // one-pass PLAIN columns: page | tile << 32
  std::vector<int32_t> pcp, pcs;     // ... their pages by column, and the columns' starts
  std::vector<uint64_t> chunk_list;  // dictionary output chunks: page | chunk << 32, 0xFFFFFFFF padding
  // ---- sizes
  uint64_t rec_total = 0;      // run records of the dictionary pages
  uint32_t chunk_total = 0;    // dictionary output chunks (chunk_run entries)
  uint64_t scratch_bytes = 0;  // bscratch
  // ---- bscratch: the named regions in layout order, and the per-column pointers of ColumnDev as byte
  // offsets (NO_REGION: null)
  std::vector<ScratchRegion> regions;
  std::vector<uint64_t> blen_off, bsrc_off, dlen_off, dsrc_off, dent_off, bsum_off, bin_total_off;
  uint64_t blen_bytes = 0;     // leading part of bscratch cleared before every launch
  uint64_t blen_bytes_nf = 0;  // ... when the plan runs plain_fused
  // ---- dictionary classes: ranges in chunk_list
  uint32_t chunk_off[N_DICT_CLS] = {0, 0, 0}, chunk_n[N_DICT_CLS] = {0, 0, 0};
  // C_DD: its chunks in `chunks` (per column in page order, each column's first at a multiple of 4:
  // padding entries of page 0xFFFFFFFF between columns), the per-chunk byte sums / first bytes in
  // bscratch, the columns and their chunk ranges in bin_lists, the LDS of the staged dictionaries
  // ([0]: C_DD, dictionaries staged in LDS; [1]: C_DDG, dictionaries gathered from HBM)
  uint32_t dd_chunk_off[2] = {0, 0}, dd_chunk_n[2] = {0, 0}, dd_region = 16;
  uint64_t dd_sums_off[2] = {NO_REGION, NO_REGION};
  int n_dd_cols[2] = {0, 0}, off_dd_cols[2] = {0, 0}, off_dd_start[2] = {0, 0};
  // ---- ranges in bl
  int n_dict_walk = 0, n_bind = 0, n_fixd = 0, n_bin_cols = 0, n_carry = 0;
  int off_dict_walk = 0, off_bind = 0, off_fixd = 0, off_bin_cols = 0, off_carry = 0;
  // BYTE_ARRAY dictionary pages of at least DENT_MIN bytes: walked per tile (launch_dict_entries)
  uint32_t n_dent_tiles = 0;
  int n_dent_cols = 0, off_dent_cols = 0, off_dent_start = 0;
  uint64_t dent_rec_off = 0, dent_scr_off = 0, dent_tb_off = 0;
  uint32_t n_bin_blocks = 0, n_bin_chunks = 0, n_dba_chunks = 0;
  uint64_t dba_meta_off = NO_REGION;  // DELTA_BYTE_ARRAY per-chunk {suffix base, smallest prefix} in bscratch
  // ---- ranges in flat
  int cls_off[C_NCLS] = {}, cls_n[C_NCLS] = {};
  int levels_off = 0, levels_n = 0;
  int n_scan_cols = 0;
  uint32_t n_segs = 0;
  uint64_t seg_status_off = 0, seg_tmp_off = 0;  // in bscratch: status words + ticket (cleared per launch), scratch
  // PLAIN-only BYTE_ARRAY columns in one pass (k_bin_bases + k_bin_plain); the per-value path's lists
  // hold those columns' entries last, so plain_fused launches skip them
  bool plain_pg = false;  // ... through k_bin_plain_pg (one wave per page) instead of the tiles
  int n_pcp = 0;          // pages of those columns (pcp); the plan starts plain_fused when there are any
  uint32_t n_psegs = 0;
  int n_pcols = 0;
  uint64_t pticket_off = 0, pflag_off = 0;  // in bscratch: ticket (cleared per launch), inexact flag (epoch-tagged)
  int n_binp_fused = 0, n_bin_cols_nf = 0;  // tails of the C_BINP list / bin_cols that belong to those columns
  // pages k_bin_walk_seg walks (the last n_binp_seg of the C_BINP list, after the one-pass columns' pages)
  int n_binp_seg = 0;
  uint32_t n_bin_blocks_nf = 0, n_bin_chunks_nf = 0;
  // V2 header null counts (PQG_PAGE_NULL_COUNT): every nullable page of the plan carries one, so the
  // host filled those pages' n_values / data_begin / out_offset; k_levels verifies the counts into the
  // epoch-tagged word at hint_off
  bool null_hints = false;
  uint64_t hint_off = 0;
  // ---- host-side facts for error resolution and pqg_sync
  std::vector<int> page_cls;  // -1 if not launched
  std::vector<uint8_t> col_nullable;
  std::vector<uint64_t> col_required_values;
  std::vector<int> col_first_page;
  std::vector<uint64_t> bin_capacity;
  std::vector<void*> empty_bin_values;  // BYTE_ARRAY columns without slots: offsets[0] = 0
  std::vector<HostErr> host_errs;
};

// Validates the descriptors and fills *out. PQG_OK, or PQG_ERR_INVALID_ARG with *bad_page = the page whose
// descriptor is refused. valid_bytes: the caller's data ends there (page and dictionary extents are
// checked against it). The output pointers of the column descriptors are copied, never dereferenced.
int plan_layout(uint64_t n_bytes, uint64_t valid_bytes, const pqg_column_desc* cols, int n_cols,
                const pqg_page_desc* pages, int n_pages, const PlanOptions& opt, PlanLayout* out, int* bad_page);

// Kernels one launch of the plan runs in the given modes.
int plan_kernel_count(const PlanLayout& L, bool plain_fused, bool dict_fused, bool null_hints);

}  // namespace pqg
