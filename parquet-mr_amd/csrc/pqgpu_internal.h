// pqgpu_internal.h — device-side tables shared by the kernels and the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pqgpu.h"
#include "pqgpu_filter.h"
#include "pqgpu_plan.h"  // ColumnDev, PageWork, BinKind, the work-list constants

namespace pqg {

// Error counter handle passed to every kernel. Error words and the counter are tagged with the
// plan's launch epoch (1..ERR_EPOCH_MAX) instead of being re-initialised each launch: a word
// holds (epoch << 48) | (~key & ERR_KEY_MASK) and is raised with atomicMax, so the newest epoch
// wins and, inside one epoch, the smallest key (index << 8 | code); the counter holds the epoch
// of the last launch that reported. The region is zeroed only when the epoch wraps.
struct ErrCount {
  uint32_t* p;
  uint32_t epoch;
};

#ifdef PQG_DIAG
// Diagnostic build: the pqg_diag_* variables (pqgpu_device.h) are static, one copy per file; each file that
// reads one sets its own, and the exported pqg_diag_*_set (pqgpu_dict.hip) call these. 0, or 3 on failure.
int diag_nostore_dict_strings(int v), diag_nostore_plain(int v), diag_nostore_kernels(int v);
int diag_wph_kernels(void* p);
#endif

hipError_t launch_dict(int width, hipStream_t st, const uint8_t* bytes, uint64_t n_bytes, PageWork* work,
                       const ColumnDev* cols, const int32_t* list, int n, uint64_t* rec, uint32_t* chunk_run,
                       const uint64_t* chunks, uint32_t n_chunks, uint64_t* pstat, uint32_t* flags, uint32_t epoch,
                       bool fused, uint64_t* err,
                       ErrCount err_count);
// hint_bad: non-null when the plan runs on V2 header null counts (PQG_PAGE_NULL_COUNT): the host filled
// every listed page's n_values / data_begin / out_offset, k_levels only verifies them and stores
// err_count.epoch to *hint_bad on a mismatch or a level error (no PageWork write); null: level-first
hipError_t launch_levels(hipStream_t st, const uint8_t* bytes, uint64_t n_bytes, PageWork* work, const ColumnDev* cols,
                         const int32_t* list, int n, uint64_t* err, ErrCount err_count, uint32_t* hint_bad);
hipError_t launch_scan(hipStream_t st, PageWork* work, const int32_t* col_pages, const int32_t* col_page_start,
                       int n_cols);
hipError_t launch_plain(int kind, hipStream_t st, const uint8_t* bytes, uint64_t n_bytes, PageWork* work,
                        const ColumnDev* cols, const int32_t* list, int n, uint64_t* err, ErrCount err_count);
hipError_t launch_delta(int width, hipStream_t st, const uint8_t* bytes, uint64_t n_bytes, PageWork* work,
                        const ColumnDev* cols, const int32_t* list, int n, uint64_t* err, ErrCount err_count);
// dictionary kernels: MODE 0 = values of a 4/8-byte dictionary; MODE 1 = the ids themselves
// (u32, into ColumnDev::blen) for BYTE_ARRAY / FIXED_LEN_BYTE_ARRAY / INT96 dictionaries
hipError_t launch_dict_ids(hipStream_t st, const uint8_t* bytes, uint64_t n_bytes, PageWork* work,
                           const ColumnDev* cols, const int32_t* list, int n, uint64_t* rec, uint32_t* chunk_run,
                           const uint64_t* chunks, uint32_t n_chunks, uint64_t* pstat, uint32_t* flags,
                           uint32_t epoch, bool fused,
                           uint64_t* err, ErrCount err_count);
// dictionary-direct BYTE_ARRAY columns (ColumnDev::dict_direct): the walk + per-chunk byte sums
// (k_dict_fused_dd, or k_dict_runs + k_dict_tiles_dd in split mode), the per-column scan of the sums
// (k_dd_bases: chunks of column i are sums[dd_start[2i] .. dd_start[2i + 1])), then offsets and value
// bytes (k_dd_str; dd_region = LDS bytes of the staged dictionary page + its u32 entry table)
// global: the columns' dictionaries are gathered from HBM (ColumnDev::dd_global): ids only in the walk's
// expansion, then k_dd_gsums, k_dd_bases, k_dd_gstr
hipError_t launch_dict_dd(hipStream_t st, const uint8_t* bytes, uint64_t n_bytes, PageWork* work,
                          const ColumnDev* cols, const int32_t* list, int n, uint64_t* rec, uint32_t* chunk_run,
                          const uint64_t* chunks, uint32_t n_chunks, uint64_t* pstat, uint32_t* flags,
                          uint32_t epoch, bool fused, uint64_t* err, ErrCount err_count, uint64_t* sums,
                          const int32_t* dd_cols, const int32_t* dd_start, int n_dd_cols, uint32_t dd_region,
                          bool global, hipEvent_t entries_ready = nullptr);
// pqgpu_dict_strings.hip: what launch_dict_dd runs after the ids and sums (`sums` holds the chunks' byte
// sums, or nothing yet when `global`): the wait for entries_ready, k_dd_gsums (global), k_dd_bases, then
// k_dd_str or k_dd_gstr
hipError_t launch_dd_strings(hipStream_t st, const uint8_t* bytes, uint64_t n_bytes, PageWork* work,
                             const ColumnDev* cols, const uint64_t* chunks, uint32_t n_chunks, const uint64_t* pstat,
                             uint64_t* err, ErrCount err_count, uint64_t* sums, const int32_t* dd_cols,
                             const int32_t* dd_start, int n_dd_cols, uint32_t dd_region, bool global,
                             hipEvent_t entries_ready);
// BOOLEAN values with encoding RLE (k_rle_bool runs the level decoder); launch_plain's kind 2
hipError_t launch_rle_bool(hipStream_t st, const uint8_t* bytes, uint64_t n_bytes, PageWork* work,
                           const ColumnDev* cols, const int32_t* list, int n, uint64_t* err, ErrCount err_count);
// DELTA_LENGTH_BYTE_ARRAY lengths (k_delta into blen, records PageWork::aux)
hipError_t launch_dlba_lengths(hipStream_t st, const uint8_t* bytes, uint64_t n_bytes, PageWork* work,
                               const ColumnDev* cols, const int32_t* list, int n, uint64_t* err, ErrCount err_count);
// pqgpu_snappy.hip: one wave per raw Snappy block (jobs: pqg_snappy_job, device array)
// ZSTD frames per job (pqgpu_zstd.hip): a grid of at most ZSTD_GRID one-wave workgroups loops over
// the jobs; scratch = min(n_jobs, ZSTD_GRID) x ZSTD_LIT_SCRATCH bytes of literal buffers (<= 512 MiB)
constexpr uint64_t ZSTD_LIT_SCRATCH = 131072;
constexpr uint32_t ZSTD_GRID = 4096;
// With seqs / mode (both non-null) the sequences are first decoded one lane per job by k_zstd_seq into
// seqs (8-byte records; job j at dst_offset / 5, so seqs holds dst_bytes / 5 + 1 records) and
// replayed by k_zstd; mode[j] (n_jobs int32) says which jobs the pre-pass left to the inline decoder.
hipError_t launch_zstd(hipStream_t st, const uint8_t* src, uint64_t src_bytes, uint8_t* dst, uint64_t dst_bytes,
                       const pqg_snappy_job* jobs, int n_jobs, int32_t* status, uint8_t* scratch, uint64_t* seqs,
                       int32_t* mode);
hipError_t launch_snappy(hipStream_t st, const uint8_t* src, uint64_t src_bytes, uint8_t* dst, uint64_t dst_bytes,
                         const void* jobs, int n_jobs, int32_t* status);
hipError_t launch_lz4raw(hipStream_t st, const uint8_t* src, uint64_t src_bytes, uint8_t* dst, uint64_t dst_bytes,
                         const void* jobs, int n_jobs, int32_t* status);
// With recs / mode (both non-null) the DEFLATE tokens are first decoded one lane per job by k_gzip_seq
// (literals stored in place, back-references as 8-byte records at dst_offset / 3: recs holds
// dst_bytes / 3 + 2 of them) and replayed by k_gzip_replay; mode[j] (n_jobs int32) = the job's record
// count, or -1 for the jobs left to k_gzip.
// Pages of fewer output bytes than prepass_min skip the token pre-pass (one lane builds a dynamic block's
// Huffman tables serially there; k_gzip's wave builds them in parallel, which small pages, with few
// tokens to share the cost, need): PQG_DISPATCH_GZIP_PREPASS_MIN, default GZ_PREPASS_MIN.
constexpr uint32_t GZ_PREPASS_MIN = 16384;
hipError_t launch_gzip(hipStream_t st, const uint8_t* src, uint64_t src_bytes, uint8_t* dst, uint64_t dst_bytes,
                       const void* jobs, int n_jobs, int32_t* status, uint64_t* recs, int32_t* mode,
                       uint32_t prepass_min = GZ_PREPASS_MIN);
// DELTA_BYTE_ARRAY prefix / suffix lengths (k_delta MODE 2: bsrc = prefix, blen = value length, aux;
// dba_meta: per BIN_CHUNK-value chunk {suffix bytes before it, smallest prefix in it};
// PageWork::reserved = 1 when a value is longer than DBA_VB: that page takes the serial copy)
constexpr uint32_t DBA_VB = 2048;  // LDS bytes of one value buffer of the DELTA_BYTE_ARRAY copy
hipError_t launch_dba_lengths(hipStream_t st, const uint8_t* bytes, uint64_t n_bytes, PageWork* work,
                              const ColumnDev* cols, const int32_t* list, int n, uint64_t* err, ErrCount err_count,
                              uint32_t* dba_meta);
// DELTA_BYTE_ARRAY value bytes: chunk tails, per-page chain of chunk tails, chunk copies, serial
// copy of the pages with long values, and (carry_cols: one wave per column) the PQG_PAGE_DBA_CARRY
// pages of each column in page order. FIXED_LEN_BYTE_ARRAY columns write value i at i * type_length
// of `values` (dba_off).
hipError_t launch_dba_copy(hipStream_t st, const uint8_t* bytes, uint64_t n_bytes, PageWork* work,
                           const ColumnDev* cols, const int32_t* list, int n, const uint64_t* chunks,
                           uint32_t n_chunks, const uint32_t* dba_meta, const int32_t* carry_cols, int n_carry_cols,
                           uint64_t* err, ErrCount err_count);
// pqgpu_binary.hip
hipError_t launch_bss(hipStream_t st, const uint8_t* bytes, uint64_t n_bytes, PageWork* work, const ColumnDev* cols,
                      const int32_t* list, int n, uint64_t* err, ErrCount err_count);
// BYTE_ARRAY dictionary pages of at least DENT_MIN bytes, per 2 KiB tile (pqgpu_plan.h)
hipError_t launch_dict_entries(hipStream_t st, const uint8_t* bytes, uint64_t n_bytes, const ColumnDev* cols,
                               const uint64_t* tiles, uint32_t n_tiles, const int32_t* dcols, const int32_t* dstart,
                               int n_dcols, uint64_t* rec, uint16_t* scr, uint64_t* tb, int n_pages, uint64_t* err,
                               ErrCount err_count);
hipError_t launch_bin_walk(hipStream_t st, const uint8_t* bytes, uint64_t n_bytes, PageWork* work,
                           const ColumnDev* cols, const int32_t* list, int n, int dict_walk, int n_pages,
                           uint64_t* err, ErrCount err_count);
// PLAIN-only BYTE_ARRAY columns in one pass: k_bin_bases (one workgroup per column, pages in column
// order in col_pages[col_start[c], col_start[c + 1])) then k_bin_plain over the 2 KiB tiles `segs`
// (page | tile << 32, in column / page / tile order). aggw / incw: per tile, tagged with `epoch`
// (1..255; zeroed when it wraps); ticket: zeroed before the launch; inexact: set to flag_epoch when a
// page's values do not end at its section end (the plan is then re-run on the per-value path).
// per_page (plans with BW_SEG_MAX_PAGES or more PLAIN pages): k_bin_plain_pg, one wave per page of
// col_pages[0, n_pages_total), instead of the tiles.
hipError_t launch_bin_plain(hipStream_t st, const uint8_t* bytes, uint64_t n_bytes, PageWork* work, const ColumnDev* cols,
                            const int32_t* col_pages, const int32_t* col_start, int n_cols, const uint64_t* segs,
                            uint32_t n_segs, uint64_t* aggw, uint64_t* incw, uint32_t* ticket, uint32_t epoch,
                            uint32_t* inexact, uint32_t flag_epoch, uint64_t* err, ErrCount err_count,
                            bool per_page, int n_pages_total);
hipError_t launch_bin_walk_seg(hipStream_t st, const uint8_t* bytes, uint64_t n_bytes, PageWork* work,
                               const ColumnDev* cols, const uint64_t* segs, uint32_t n_segs, uint64_t* status,
                               uint32_t* ticket, uint32_t* tmp, uint64_t* err, ErrCount err_count);
hipError_t launch_bin_dict_map(hipStream_t st, PageWork* work, const ColumnDev* cols, const int32_t* list, int n);
hipError_t launch_gather_fixed(hipStream_t st, const uint8_t* bytes, uint64_t n_bytes, PageWork* work,
                               const ColumnDev* cols, const int32_t* list, int n);
hipError_t launch_bin_scan(hipStream_t st, const uint8_t* bytes, uint64_t n_bytes, const ColumnDev* cols,
                           const int32_t* bin_cols, int n_bin_cols,
                           const uint64_t* blocks, uint32_t n_blocks);
hipError_t launch_bin_copy(hipStream_t st, const uint8_t* bytes, uint64_t n_bytes, PageWork* work,
                           const ColumnDev* cols, const uint64_t* chunks, uint32_t n_chunks, uint64_t* err,
                           ErrCount err_count);
// pqgpu_assembly.hip: levels -> offsets / validity of one leaf column's path
constexpr uint32_t ASM_MAX_DEPTHS = 8;  // repetition depths 0..7 (max_rep <= 7)
constexpr uint32_t ASM_MAX_NODES = 16;  // path length
// 64-bit words at `totals`: the entry counts of depths 0..7, the ticket (its low half), then the look-back
// timeout flag in a word of its own (~0 when a wait timed out): with max_rep == 7 every count word is in use
constexpr uint32_t ASM_TIMEOUT_WORD = ASM_MAX_DEPTHS + 1;
constexpr uint32_t ASM_TOTAL_WORDS = ASM_MAX_DEPTHS + 2;
struct AsmParams {
  uint32_t n_nodes;
  uint32_t max_rep;
  uint32_t DR[ASM_MAX_DEPTHS];          // definition level of the r-th REPEATED node (DR[0] = 0)
  int32_t kind[ASM_MAX_NODES];          // pqg_repetition
  uint32_t depth[ASM_MAX_NODES];        // repetition depth of the node's entries
  uint32_t D[ASM_MAX_NODES];            // definition level of the node
  uint8_t* validity[ASM_MAX_NODES];
  int64_t* offsets[ASM_MAX_NODES];
};
hipError_t launch_assemble(hipStream_t st, const uint8_t* def, const uint8_t* rep, uint64_t n, const AsmParams& P,
                           uint64_t* block_counts, uint32_t n_blocks, uint64_t* totals, uint32_t* ticket, int phase);
// pqgpu_filter.hip: pqg_filter_run / pqg_filter_run_dict (FilterCols, FilterDictTab: pqgpu_filter.h).
// scratch (u64 words): rank[n_nullable][n_tiles], sel[n_tiles], totals[PQG_FILTER_MAX_NODES], bad[PQG_FILTER_MAX_NODES],
// and with dictionaries dict_bad[PQG_FILTER_MAX_NODES] (a slot's bad-id flag), tables[table_words] (the leaves'
// verdict tables, one bit per dictionary entry)
inline uint64_t filter_tiles(uint64_t n_rows) { return (n_rows + PQG_FILTER_TILE_ROWS - 1) / PQG_FILTER_TILE_ROWS; }
inline uint64_t filter_scratch_words(uint64_t n_rows, uint32_t n_nullable, uint64_t dict_words = 0) {
  return ((uint64_t)n_nullable + 1) * filter_tiles(n_rows) + 2 * PQG_FILTER_MAX_NODES + dict_words;
}
// d_dict: the FilterDictTab on the device (null: no dictionary columns), h_dict: the same on the host;
// bin: the program has a binary-order or fixed-width-binary leaf (pqg_filter::binary_paths): the *_bin kernels
hipError_t launch_filter(hipStream_t st, const uint8_t* d_image, uint32_t image_bytes, const FilterCols& cols,
                         uint64_t n_rows, uint64_t* scratch, uint64_t* bitmap, int64_t* row_ids, uint64_t row_ids_capacity,
                         pqg_filter_result* result, const FilterDictTab* d_dict, const FilterDictTab* h_dict, bool bin);
// pqgpu_filter.hip: pqg_filter_run_records with contains leaves (FilterRecDev: pqgpu_filter.h). The scratch is
// launch_filter's with dictionaries, then flags[PQG_FILTER_MAX_NODES], bitmaps[n_leaves][tiles(n_rows) * 64],
// starts[n_rep][tiles(max_slots)], vals[n_rep][tiles(max_slots)] (dict_words = PQG_FILTER_MAX_NODES + table_words).
// h_rec->rt.bitmaps must hold filter_records_bitmaps(...) before it is copied to d_rec.
struct FilterRecDev;
uint64_t filter_records_scratch_words(uint64_t n_rows, uint32_t n_nullable, uint64_t dict_words, uint32_t n_leaves,
                                      uint32_t n_rep, uint64_t max_slots);
uint64_t* filter_records_bitmaps(uint64_t* scratch, uint64_t n_rows, uint32_t n_nullable, uint64_t dict_words);
hipError_t launch_filter_records(hipStream_t st, const uint8_t* d_image, uint32_t image_bytes, const FilterCols& cols,
                                 uint64_t n_rows, uint64_t* scratch, uint64_t* bitmap, int64_t* row_ids,
                                 uint64_t row_ids_capacity, pqg_filter_result* result, const FilterRecDev* d_rec,
                                 const FilterRecDev* h_rec, bool bin);
// pqgpu_take.hip: pqg_take. scratch (u64 words): keep[n_tiles], rank[n_cols][n_tiles], kept[n_cols][n_tiles],
// bytes[n_cols][n_tiles] (per-tile counts, scanned in place), totals[1 + 3 n_cols]
struct TakeColDev;
struct TakeRecDev;
struct TakeRecPlan;
inline uint64_t take_scratch_words(uint64_t n_rows, uint32_t n_cols) {
  return (1 + 3 * (uint64_t)n_cols) * (filter_tiles(n_rows) + 1);
}
hipError_t launch_take(hipStream_t st, const uint64_t* bitmap, uint64_t n_rows, const TakeColDev* d_cols, uint32_t n_cols,
                       bool any_nullable, bool any_binary, uint64_t rows_capacity, uint64_t* scratch,
                       pqg_take_counts* counts, pqg_take_result* result, bool staged);
// pqgpu_take.hip: pqg_take_records. d_recs: plan.n_records records whose own slot bitmaps lie at
// slot_off inside the scratch (layout: see rec_scratch)
uint64_t take_records_scratch_words(uint64_t max_rows, uint32_t n_cols, uint64_t slot_words);
hipError_t launch_take_records(hipStream_t st, const uint64_t* bitmap, uint64_t n_rows, const TakeRecDev* d_recs,
                               uint32_t n_cols, const TakeRecPlan& plan, uint64_t rows_capacity, uint64_t* scratch,
                               pqg_take_record_counts* counts, pqg_take_result* result, bool staged);
// pqgpu_crc.hip: pqg_crc32_pages (CrcTile, CrcJobDev, the constants `tab` of tile_bytes: pqgpu_crc.h).
// partial: n_tiles words; k_crc_tiles (skipped without tiles), then k_crc_fold
struct CrcTile;
struct CrcJobDev;
hipError_t launch_crc(hipStream_t st, const uint8_t* bytes, uint64_t n_bytes, const CrcTile* tiles, uint32_t n_tiles,
                      const CrcJobDev* jobs, uint32_t n_jobs, const uint32_t* tab, uint32_t tile_bytes,
                      uint32_t* partial, uint32_t* crc, int32_t* status);
// pqgpu_aes.hip: pqg_decrypt_pages (AesTile, AesJobDev, the key material `keys` of tile_bytes: pqgpu_aes.h).
// partial: 16 bytes per tile; k_aes_tiles, then k_aes_fold
struct AesTile;
struct AesJobDev;
hipError_t launch_decrypt(hipStream_t st, const uint8_t* src, uint64_t n_src, uint8_t* dst, const AesTile* tiles,
                          uint32_t n_tiles, const AesJobDev* jobs, uint32_t n_jobs, const uint8_t* aad,
                          const uint32_t* te0, const uint32_t* keys, uint32_t tile_bytes, void* partial,
                          int32_t* status);
// pqgpu_aes.hip: pqg_copy_ranges, one wave per range (ranges outside the buffers are skipped)
hipError_t launch_copy_ranges(hipStream_t st, const uint8_t* src, uint64_t n_src, uint8_t* dst, uint64_t n_dst,
                              const pqg_copy_range* ranges, uint32_t n);
hipError_t launch_unpack_runs(hipStream_t st, int w, const uint8_t* in, uint64_t in_bytes, const uint64_t* in_off,
                              const uint32_t* counts, const uint64_t* out_off, int32_t* out, int n_runs,
                              uint32_t max_count);

}  // namespace pqg
