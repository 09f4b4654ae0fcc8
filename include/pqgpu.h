/*
 * pqgpu.h — C ABI of the MI355X-native Parquet column-page decoder.
 *
 * This is the drop-in boundary for parquet-mr's page-decode hot path
 * (SURVEY.md §8b). Every entry point uses plain C types: pointers and sizes,
 * no C++ or torch types. A JNI shim binds it the way
 * parquet-mr would bind a native ValuesReader / ParquetReadRouter backend.
 *
 * Reference interfaces replaced (apache/parquet-mr 1.15.0-SNAPSHOT):
 *   - ValuesReader.initFromPage / readX
 *     parquet-column/src/main/java/org/apache/parquet/column/values/ValuesReader.java:36-203
 *     -> pqg_decode (many pages per call; dense values + levels per column)
 *   - ColumnReaderBase.readPageV1 / readPageV2 / newRLEIterator (page split, levels)
 *     parquet-column/src/main/java/org/apache/parquet/column/impl/ColumnReaderBase.java:738-789
 *     -> pqg_decode (levels decoded on device, data section located on device)
 *   - Encoding.getValuesReader / getDictionaryBasedValuesReader / initDictionary
 *     parquet-column/src/main/java/org/apache/parquet/column/Encoding.java:61-320
 *     -> the (physical_type, encoding) dispatch inside pqg_decode
 *   - ParquetReadRouter.read(bitWidth, in, currentCount, int[] out)
 *     parquet-plugins/parquet-encoding-vector/src/main/java/org/apache/parquet/column/values/bitpacking/ParquetReadRouter.java:57-66
 *     -> pqg_unpack_runs (device batch) / pqg_router_read (host buffers)
 *
 * Threading: a pqg_ctx owns one HIP stream and its device scratch; it is not
 * shared between threads (one ctx per thread per GPU), like a ValuesReader.
 * All pqg_decode / pqg_plan_launch work is asynchronous on the ctx stream
 * until pqg_sync (a launch may fan out to three internal queues of the ctx
 * and joins them back into the ctx stream before it returns). Outputs are
 * valid only after pqg_sync returns: two rare cases are repaired by pqg_sync
 * itself with a host-driven re-launch (a PLAIN BYTE_ARRAY page with bytes
 * after its values, pqg_plan_plain_fallbacks; a fused-kernel timeout,
 * pqg_plan_timeout_fallbacks; a wrong V2 header null count,
 * pqg_plan_null_hint_fallbacks), so work ordered after a launch on the ctx
 * stream by events alone may see outputs that pqg_sync later rewrites.
 * No exception crosses this ABI: every function returns a pqg_error code and
 * fills an optional pqg_status.
 *
 * ABI 6 (this version): the rows a selection bitmap keeps, gathered into compact columns on the
 * device (pqg_take; PQG_DISPATCH_TAKE_STAGED). Added to ABI 6 without a change to what it had:
 * record filters on list columns (PQG_FILTER_CONTAINS, pqg_filter_record_column,
 * pqg_filter_run_records); record filters on dictionary-id columns (pqg_filter_dictionary, pqg_filter_run_dict,
 * PQG_FILTER_DICT_LDS_BYTES) and pqg_decode_dictionary; record selection on repeated columns
 * (pqg_take_record_column, pqg_take_record_counts, pqg_take_records); record filters on INT96 and
 * FIXED_LEN_BYTE_ARRAY columns and the three binary comparators (pqg_filter_binary_order,
 * pqg_filter_column_type, pqg_filter_create_typed); page checksums on the device (pqg_crc_job,
 * pqg_crc32_pages, pqg_crc32_sync, PQG_DISPATCH_CRC_TILE_BYTES) with the host helpers pqg_crc32_combine
 * and pqg_crc_jobs_from_headers; encrypted pages on the device (pqg_decrypt_job, pqg_aes_key,
 * pqg_decrypt_pages, pqg_decrypt_sync, pqg_copy_range, pqg_copy_ranges, PQG_ERR_TAG,
 * PQG_DISPATCH_AES_TILE_BYTES) with the host helper pqg_module_aad.
 * ABI 5: record-level filter2 predicates over decoded columns (pqg_filter_create /
 * pqg_filter_program / pqg_filter_destroy on the host, pqg_filter_run on the device).
 * ABI 4: pqg_page_desc carries the V2 header's num_nulls
 * (PQG_PAGE_NULL_COUNT, 56-byte descriptor), pqg_plan_null_hint_fallbacks.
 * ABI 3: per-page errors (pqg_page_errors) so that a failure
 * surfaces in its own column only; the staged host path (pqg_host_input /
 * pqg_decode_staged / pqg_staged_column) for callers that must not hold host
 * arrays across device work (JNI critical regions); the host batch of router
 * runs (pqg_router_read_runs); levels readers (pqgpu_reader.h).
 */
#ifndef PQGPU_H
#define PQGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PQG_ABI_VERSION 6

/* parquet-format `Type` values (parquet.thrift). */
enum pqg_physical_type {
  PQG_BOOLEAN = 0,
  PQG_INT32 = 1,
  PQG_INT64 = 2,
  PQG_INT96 = 3,
  PQG_FLOAT = 4,
  PQG_DOUBLE = 5,
  PQG_BYTE_ARRAY = 6,
  PQG_FIXED_LEN_BYTE_ARRAY = 7
};

/* parquet-format `Encoding` values (parquet.thrift); see Encoding.java:61-253. */
enum pqg_encoding {
  PQG_PLAIN = 0,
  PQG_PLAIN_DICTIONARY = 2,
  PQG_RLE = 3,
  PQG_BIT_PACKED = 4,
  PQG_DELTA_BINARY_PACKED = 5,
  PQG_DELTA_LENGTH_BYTE_ARRAY = 6,
  PQG_DELTA_BYTE_ARRAY = 7,
  PQG_RLE_DICTIONARY = 8,
  PQG_BYTE_STREAM_SPLIT = 9
};

/*
 * Error codes. Each decode error names the Java exception the reference
 * reader raises for the same bytes, so the JNI shim can rethrow it as
 * ParquetDecodingException (io/ParquetDecodingException.java) with the same
 * meaning. The first failing (page, value index) in page order is reported,
 * which is the value at which the reference's lazy reader would throw.
 */
enum pqg_error {
  PQG_OK = 0,
  PQG_ERR_INVALID_ARG = 1,      /* API misuse (null pointer, bad count, capacity too small) */
  PQG_ERR_UNSUPPORTED = 2,      /* (type, encoding) has no reader: Encoding.java:84,193; UnsupportedOperationException */
  PQG_ERR_HIP = 3,              /* HIP runtime failure */
  PQG_ERR_NO_DEVICE = 4,        /* no HIP device / extension unusable */
  PQG_ERR_TIMEOUT = 5,          /* a fused-kernel wave waited > 2 s of wall time for its page's walk (the
                                   walker was descheduled or starved); not a decode error: the chunk's
                                   output is incomplete, relaunch the plan */
  PQG_ERR_EOF = 10,             /* java.io.EOFException: read past the end of a page section
                                   (SingleBufferInputStream.read :50-55, LittleEndianDataInputStream.readInt/readLong) */
  PQG_ERR_RLE_PAST_END = 11,    /* IllegalArgumentException "Reading past RLE/BitPacking stream."
                                   (RunLengthBitPackingHybridDecoder.java:81) */
  PQG_ERR_BIT_WIDTH = 12,       /* IllegalArgumentException "bitWidth must be >= 0 and <= 32"
                                   (RunLengthBitPackingHybridDecoder.java:55) */
  PQG_ERR_DICT_ID = 13,         /* ArrayIndexOutOfBoundsException in Dictionary.decodeToX
                                   (PlainValuesDictionary.java:159-161 etc.) */
  PQG_ERR_EMPTY_PAGE = 14,      /* IOException "Attempt to read from empty page" (DictionaryValuesReader.java:57-62) */
  PQG_ERR_EMPTY_PACKED_RUN = 15,/* bit-packed run header with 0 groups: AIOOBE on currentBuffer[] (:71) */
  PQG_ERR_DELTA_CONFIG = 16,    /* IllegalArgumentException "miniBlockSize must be multiple of 8"
                                   (DeltaBinaryPackingConfig.java:39) */
  PQG_ERR_DELTA_PAST_END = 17,  /* ParquetDecodingException "no more value to read, total value count is N"
                                   (DeltaBinaryPackingValuesReader.java:115-119) */
  PQG_ERR_CORRUPT = 18,         /* section lengths inconsistent with the page (negative/oversized length prefix) */
  PQG_ERR_NO_DICTIONARY = 19,   /* "could not read page ... as the dictionary was missing" (ColumnReaderBase.java:709-712) */
  PQG_ERR_DICT_ENCODING = 20,   /* "Dictionary data encoding type not supported" (PlainValuesDictionary.java:49-52) */
  PQG_ERR_CRC = 21,             /* ParquetDecodingException "could not verify page integrity, CRC checksum
                                   verification failed" (ParquetFileReader.java:1805-1813) */
  PQG_ERR_TAG = 22              /* TagVerificationException "GCM tag check failed" (AesGcmDecryptor.java:71-72) */
};

/*
 * One data page, already decompressed, located inside the batch byte buffer.
 * Mirrors DataPageV1 (DataPageV1.java:26-141) and DataPageV2 (DataPageV2.java:26-247).
 */
typedef struct pqg_page_desc {
  uint64_t offset;         /* byte offset of the page body in the batch buffer (16-B aligned is fastest) */
  uint32_t size;           /* page body length in bytes (V1: rl + dl + data sections; V2: rl + dl + data) */
  uint32_t num_values;     /* header num_values: level slots including nulls */
  int32_t column;          /* index into the pqg_column_desc table */
  int32_t version;         /* 1 = DataPageV1, 2 = DataPageV2 */
  int32_t encoding;        /* value encoding (pqg_encoding) */
  int32_t rl_encoding;     /* V1 only: RLE or BIT_PACKED (ignored when max_rep == 0) */
  int32_t dl_encoding;     /* V1 only: RLE or BIT_PACKED (ignored when max_def == 0) */
  uint32_t rl_byte_length; /* V2 only: repetition_levels_byte_length */
  uint32_t dl_byte_length; /* V2 only: definition_levels_byte_length */
  uint32_t flags;          /* PQG_PAGE_* (0 for a page written by a current writer) */
  uint32_t num_nulls;      /* V2 only, read when flags has PQG_PAGE_NULL_COUNT: DataPageHeaderV2.num_nulls (ABI 4) */
  uint32_t reserved;       /* 0 (sizeof(pqg_page_desc) = 56) */
} pqg_page_desc;

/* pqg_page_desc.flags: PQG_PAGE_DBA_CARRY — a DELTA_BYTE_ARRAY page whose reader takes the previous
 * page's last value as its starting `previous` (PARQUET-246: DeltaByteArrayWriter before parquet-mr
 * 1.8.0 did not reset `previous` between pages, so the first value of every page after the first may
 * carry a prefix of the previous page's last value). The reader side is
 * ColumnReaderBase.initDataReader (parquet-column/.../column/impl/ColumnReaderBase.java:730-735) ->
 * DeltaByteArrayReader.setPreviousReader (.../values/deltastrings/DeltaByteArrayReader.java:89-95),
 * applied when CorruptDeltaByteArrays.requiresSequentialReads(created_by, DELTA_BYTE_ARRAY)
 * (parquet-column/src/main/java/org/apache/parquet/CorruptDeltaByteArrays.java:31-84) holds: the caller
 * sets the flag on every DELTA_BYTE_ARRAY page of such a column chunk except its first page. The
 * previous page of the column in the batch must be a DELTA_BYTE_ARRAY page (the reference casts its
 * reader to DeltaByteArrayReader), otherwise PQG_ERR_UNSUPPORTED. Flagged pages are decoded in page
 * order, one column at a time. */
#define PQG_PAGE_DBA_CARRY 1

/* pqg_page_desc.flags: PQG_PAGE_NULL_COUNT — `num_nulls` holds the DataPageV2 header's null count
 * (DataPageV2.getNullCount, parquet-column/src/main/java/org/apache/parquet/column/page/DataPageV2.java:197-199;
 * pqg_pages_from_headers sets it for every V2 page). The reference never trusts that count: it decodes
 * the definition levels and reads a value for every slot with dl == max_def (ColumnReaderBase.java:650-676,
 * readPageV2 :760-771). The decoder uses it as a verified hint: when every page of every nullable column
 * of a plan is a V2 page carrying it, each page's value count (num_values - num_nulls) and output offset
 * are known on the host, so the value kernels start at the launch's start beside the level kernel instead
 * of after it. The level kernel still decodes every level section and compares each page's true count;
 * a mismatch (or any level / level-init error on such a page) makes pqg_sync re-run the plan with the
 * counts taken from the levels, as without the hint (pqg_plan_null_hint_fallbacks counts these re-runs),
 * so results and errors are those of the reference whatever the header says. */
#define PQG_PAGE_NULL_COUNT 2

/*
 * One column chunk: the ColumnDescriptor facts the decoder needs (physical
 * type, type length, max rep/def level), its dictionary page (optional) and
 * where its decoded output goes.
 *
 * Output layout (Java-equivalent "dense" form): `values` receives only the
 * non-null values, in slot order, exactly the sequence the reference's
 * ValuesReader returns for slots with dl == max_def (ColumnReaderBase.java:650-676).
 * `def_levels` / `rep_levels` receive one byte per slot (the Java int level;
 * level values above 255 are stored saturated to 255 and therefore never
 * equal max_def, which is limited to <= 254). Element widths: INT32/FLOAT 4,
 * INT64/DOUBLE 8, INT96 12, FIXED_LEN_BYTE_ARRAY type_length, BOOLEAN 1.
 * For pqg_decode these are device pointers; the per-page value counts are
 * written to `page_value_counts` (device, one uint32 per page of the batch, optional).
 */
/* pqg_column_desc.flags: PQG_COLUMN_DICTIONARY_IDS — `values` receives the uint32 dictionary id of
 * every non-null value instead of the value (DictionaryValuesReader.readValueDictionaryId,
 * parquet-column/src/main/java/org/apache/parquet/column/values/dictionary/DictionaryValuesReader.java:67-73),
 * any physical type; a page of the column that is not dictionary-encoded fails with
 * PQG_ERR_UNSUPPORTED (ValuesReader.readValueDictionaryId throws UnsupportedOperationException,
 * ValuesReader.java:142-144). */
#define PQG_COLUMN_DICTIONARY_IDS 1

typedef struct pqg_column_desc {
  int32_t physical_type;     /* pqg_physical_type */
  int32_t type_length;       /* FIXED_LEN_BYTE_ARRAY length */
  int32_t max_rep;           /* ColumnDescriptor.getMaxRepetitionLevel() */
  int32_t max_def;           /* ColumnDescriptor.getMaxDefinitionLevel() */
  int64_t dict_offset;       /* byte offset of the dictionary page body in the batch buffer, -1 if none */
  uint32_t dict_size;        /* dictionary page body bytes */
  uint32_t dict_num_values;  /* DictionaryPageHeader.num_values */
  int32_t dict_encoding;     /* PLAIN or PLAIN_DICTIONARY */
  int32_t flags;             /* PQG_COLUMN_* (0: decode values) */
  void* values;              /* dense output values */
  uint64_t values_capacity;  /* capacity in elements */
  uint8_t* def_levels;       /* per-slot definition levels (may be NULL) */
  uint8_t* rep_levels;       /* per-slot repetition levels (may be NULL) */
  uint64_t levels_capacity;  /* capacity in slots */
  uint8_t* binary_data;      /* BYTE_ARRAY only: value bytes; `values` then holds int64 offsets[n+1] */
  uint64_t binary_capacity;  /* BYTE_ARRAY only: capacity of binary_data in bytes */
  uint64_t values_written;   /* OUT (after pqg_sync / host calls): non-null values decoded */
} pqg_column_desc;

/* First decode error of a call, in (page, value) order. */
typedef struct pqg_status {
  int32_t code;              /* pqg_error */
  int32_t page;              /* index into the page table, -1 if not page-specific */
  int64_t value_index;       /* value index inside the page (data values for value errors, slots for level errors) */
  char message[240];
} pqg_status;

typedef struct pqg_ctx pqg_ctx;
typedef struct pqg_plan pqg_plan;

/* ---- context ------------------------------------------------------------ */

/* Library / ABI version (PQG_ABI_VERSION). */
int pqg_abi_version(void);

/* Number of visible HIP devices (0 when none). */
int pqg_device_count(void);

/* Create a context on `device`. `hip_stream` may be NULL (the ctx creates its
 * own non-blocking stream) or an existing hipStream_t to run on. */
int pqg_ctx_create(int device, void* hip_stream, pqg_ctx** out);
int pqg_ctx_destroy(pqg_ctx* ctx);
/* The hipStream_t the ctx launches on. */
void* pqg_ctx_stream(pqg_ctx* ctx);

/* Kernel-choice overrides for plans created on the ctx afterwards (tests and A/B measurements;
 * the defaults are the measured choices). Decoded results are the same under every setting.
 *   PQG_DISPATCH_PLAIN_ONE_PASS  PLAIN-only BYTE_ARRAY columns: 0 = per-value path (walk, offset
 *                                scan, copy), 1 = one pass, tiles, 2 = one pass, tiles below 4,096
 *                                PLAIN pages and one wave per page from there (default), 3 = one
 *                                pass, one wave per page
 *   PQG_DISPATCH_DICT_DIRECT     dictionary BYTE_ARRAY columns with small dictionaries: 1 = ids
 *                                mapped straight to lengths and bytes (default), 0 = ids, then map
 *   PQG_DISPATCH_DICT_FUSED      dictionary pages: 1 = walk and expansion in one launch (default),
 *                                0 = two launches (the mode a fused launch that timed out re-runs in)
 *   PQG_DISPATCH_NULL_HINTS      nullable columns of V2 pages: 1 = value kernels start from the header
 *                                null counts beside the level decode, which verifies them (default;
 *                                PQG_PAGE_NULL_COUNT), 0 = levels first
 *   PQG_DISPATCH_TAKE_STAGED     pqg_take: 1 = kept values and levels staged in LDS and stored as aligned
 *                                full-wave runs (default), 0 = one store per kept lane
 *   PQG_DISPATCH_GZIP_PREPASS_MIN pqg_gzip_decompress: pages of at least `value` output bytes take the
 *                                token pre-pass + replay, smaller ones the one-wave decoder (default
 *                                16384; 0 = every page); applies to later pqg_gzip_decompress calls
 *   PQG_DISPATCH_ZSTD_PREPASS    pqg_zstd_decompress: 1 = lane-per-page sequence pre-pass + replay (default),
 *                                0 = every page takes the inline sequence decoder (the pre-pass's
 *                                fallback); applies to later pqg_zstd_decompress calls
 *   PQG_DISPATCH_CRC_TILE_BYTES  pqg_crc32_pages: bytes of a range one wave checksums: 4096, 8192, 16384
 *                                or 32768 (default PQG_CRC_TILE_BYTES); applies to later calls
 *   PQG_DISPATCH_AES_TILE_BYTES  pqg_decrypt_pages: ciphertext bytes of a module one wave decrypts: a power
 *                                of two from 1024 to 32768 (default PQG_AES_TILE_BYTES); applies to later calls
 * Returns PQG_ERR_INVALID_ARG for an unknown key or value. Not thread-safe (like the ctx). */
enum pqg_dispatch {
  PQG_DISPATCH_PLAIN_ONE_PASS = 1,
  PQG_DISPATCH_DICT_DIRECT = 2,
  PQG_DISPATCH_GZIP_PREPASS_MIN = 3,
  PQG_DISPATCH_DICT_FUSED = 4,
  PQG_DISPATCH_NULL_HINTS = 5,
  PQG_DISPATCH_TAKE_STAGED = 6,
  PQG_DISPATCH_ZSTD_PREPASS = 7,
  PQG_DISPATCH_CRC_TILE_BYTES = 8,
  PQG_DISPATCH_AES_TILE_BYTES = 9
};
int pqg_ctx_set_dispatch(pqg_ctx* ctx, int key, int value);

/* ---- device-resident batch decode ----------------------------------------
 * `d_bytes` is a 4-byte aligned DEVICE buffer holding every page body (and
 * dictionary page) the descriptors refer to, padded by at least 64 readable
 * bytes after the last page; `n_bytes` is its readable size INCLUDING that
 * padding (device loads are range-checked per dword against it, so a page that
 * ends at an unaligned offset needs the padding inside n_bytes). Page offsets may
 * have any alignment (raw file bytes); 16-B aligned is fastest. Column output
 * pointers are DEVICE pointers. Pages of one column
 * must appear in page order; pages of several columns may be interleaved.
 * Asynchronous: errors are reported by pqg_sync. */
int pqg_decode(pqg_ctx* ctx, const uint8_t* d_bytes, uint64_t n_bytes,
               pqg_column_desc* cols, int n_cols,
               const pqg_page_desc* pages, int n_pages,
               uint32_t* d_page_value_counts, pqg_status* st);

/* Wait for all work on the ctx stream; returns the first decode error of the
 * calls since the previous pqg_sync (every plan launched since then, in launch
 * order, is checked and repaired as described above) and fills
 * cols[i].values_written for the most recent pqg_decode. */
int pqg_sync(pqg_ctx* ctx, pqg_status* st);

/* ---- per-page errors ---------------------------------------------------------
 * pqg_status names the batch's first failing page. A column reader in the
 * reference fails on its own (ColumnReaderBase.readPage / checkRead /
 * readValue, ColumnReaderBase.java:590-676, 738-771): the other columns of the
 * row group stay readable. pqg_page_errors gives every page's own first error
 * in the reference's read order of that page:
 *   DICTIONARY  the column's dictionary page (ColumnReaderBase ctor :448-472; set on the column's
 *               first page of the batch)
 *   RL_INIT / DL_INIT / DATA_INIT   rlReader / dlReader / data reader initFromPage (readPageV1
 *               :738-758; a V2 page's level lengths past the page: RL_INIT)
 *   RL_READ / DL_READ   repetitionLevelColumn / definitionLevelColumn .nextInt() of slot `index`
 *               (checkRead :650-676 reads rl then dl per slot)
 *   VALUE       the read of value `index` of the page (readValue :584-626)
 * Values are decoded only for slots before a level error, and a page's value count
 * (page_value_counts) stops there. A caller serving the pages of one column in
 * order stops at that column's first failing page (pqgpu_reader.h does). */
enum pqg_phase {
  PQG_PHASE_NONE = 0,
  PQG_PHASE_DICTIONARY = 1,
  PQG_PHASE_RL_INIT = 2,
  PQG_PHASE_DL_INIT = 3,
  PQG_PHASE_DATA_INIT = 4,
  PQG_PHASE_RL_READ = 5,
  PQG_PHASE_DL_READ = 6,
  PQG_PHASE_VALUE = 7
};

typedef struct pqg_page_error {
  int32_t code;     /* pqg_error; PQG_OK when the page decoded cleanly */
  int32_t phase;    /* pqg_phase */
  int64_t index;    /* RL_READ / DL_READ: slot in the page; VALUE: value in the page; else -1 */
} pqg_page_error;

/* Every page's error of the most recent pqg_decode / pqg_decode_host / pqg_decode_staged on the
 * ctx, after its pqg_sync (the host calls sync themselves). `n_pages` must equal that call's page
 * count. API / device failures (no page) are not listed: they are the call's return code. */
int pqg_page_errors(pqg_ctx* ctx, pqg_page_error* out, int n_pages);
/* The same for a plan's most recent launch, after pqg_sync. */
int pqg_plan_page_errors(pqg_plan* plan, pqg_page_error* out, int n_pages);

/* ---- prepared plans (bench / steady-state) --------------------------------
 * A plan uploads descriptors once; pqg_plan_launch re-runs the decode of the
 * same page batch with no host work beyond the kernel launches. */
int pqg_plan_create(pqg_ctx* ctx, const uint8_t* d_bytes, uint64_t n_bytes,
                    const pqg_column_desc* cols, int n_cols,
                    const pqg_page_desc* pages, int n_pages, pqg_plan** out, pqg_status* st);
int pqg_plan_launch(pqg_plan* plan);
/* Number of kernel launches one pqg_plan_launch issues. */
int pqg_plan_kernel_count(pqg_plan* plan);
/* Dictionary pages decode in one fused launch (walk + expansion, the expansion waiting for its
 * page's walk). Should an expansion wait longer than 2 s (the GPU did not dispatch the walker it
 * waits for), that launch reports PQG_ERR_TIMEOUT internally and pqg_sync re-runs the plan with the
 * walk and the expansion as two launches; the plan keeps that mode and the caller sees the normal
 * result. The same holds for a segment of a segmented PLAIN BYTE_ARRAY page walk (per-value path,
 * few large pages) whose predecessor segment did not publish within 2 s: the plan re-runs with those
 * pages walked one wave each, and keeps that mode. Returns how many launches of the plan were re-run
 * either way. */
int pqg_plan_timeout_fallbacks(pqg_plan* plan);
/* BYTE_ARRAY columns whose pages are all PLAIN decode in one pass per 2 KiB tile of the pages (walk,
 * offsets and value bytes together), which takes each page's values to fill its data section, as
 * every writer lays them out. A page with bytes after its num_values values (which the reader
 * ignores) is detected on the device, and pqg_sync re-runs the plan on the per-value path (value
 * walk, offset scan, byte copy), which reads exactly num_values values; the plan keeps that path.
 * Returns how many launches of the plan were re-run that way. */
int pqg_plan_plain_fallbacks(pqg_plan* plan);
/* Plans whose nullable columns are all V2 pages with PQG_PAGE_NULL_COUNT start their value kernels
 * from the header null counts (see PQG_PAGE_NULL_COUNT). Returns how many launches of the plan pqg_sync
 * re-ran with the counts taken from the levels because a header count was wrong (the plan then keeps
 * the level-first order). */
int pqg_plan_null_hint_fallbacks(pqg_plan* plan);
int pqg_plan_destroy(pqg_plan* plan);

/* ---- host-buffer decode (the JNI shim's entry: file bytes in, arrays out) --
 * Copies `h_bytes` to the device through pinned staging (hipMemcpyAsync),
 * decodes, and copies values / levels back into the HOST pointers of `cols`.
 * Synchronous. */
int pqg_decode_host(pqg_ctx* ctx, const uint8_t* h_bytes, uint64_t n_bytes,
                    pqg_column_desc* cols, int n_cols,
                    const pqg_page_desc* pages, int n_pages,
                    uint32_t* h_page_value_counts, pqg_status* st);

/* ---- staged host path -------------------------------------------------------
 * pqg_decode_host reads and writes the caller's host arrays while the device works, which a JNI
 * caller may not allow (a Get*ArrayCritical region must not span blocking calls). The staged path
 * keeps the caller's arrays out of device work: the library owns the pinned input and output
 * buffers, and the caller copies in before and out after.
 *   1. pqg_host_input(ctx, n_bytes, &p): pinned buffer of at least n_bytes (+ padding, zeroed by the
 *      decode); the caller writes the page bytes to p[0 .. n_bytes) (JNI: GetByteArrayRegion, or a
 *      memcpy from a direct buffer). Valid until the next pqg_host_input / host call on ctx.
 *   2. pqg_decode_staged(ctx, n_bytes, cols, ...): as pqg_decode_host over those bytes. The output
 *      fields of `cols` (pointers and capacities) are ignored: the values of every column and the
 *      levels of every column with max_def / max_rep > 0 are produced into library memory, sized by
 *      the library. Returns after the outputs are in pinned host memory.
 *   3. pqg_staged_column(ctx, col, &out): where column `col`'s outputs are in that memory; valid
 *      until the next host call on ctx. Copy them out with any memcpy (JNI: Set<Type>ArrayRegion,
 *      or pqg_copy_out inside a short critical region: a plain multi-threaded memcpy, no device call).
 * Codes, statuses and per-page errors as pqg_decode_host. */
typedef struct pqg_staged_output {
  const void* values;        /* n_values elements (BYTE_ARRAY: int64 offsets[n_values + 1]) */
  const uint8_t* def_levels; /* n_slots bytes, NULL if not wanted / max_def == 0 */
  const uint8_t* rep_levels; /* n_slots bytes, NULL if not wanted / max_rep == 0 */
  const uint8_t* binary;     /* BYTE_ARRAY: n_binary value bytes */
  uint64_t n_values;
  uint64_t n_slots;
  uint64_t n_binary;
} pqg_staged_output;

int pqg_host_input(pqg_ctx* ctx, uint64_t n_bytes, uint8_t** buf);
int pqg_decode_staged(pqg_ctx* ctx, uint64_t n_bytes, pqg_column_desc* cols, int n_cols,
                      const pqg_page_desc* pages, int n_pages, uint32_t* h_page_value_counts, pqg_status* st);
int pqg_staged_column(pqg_ctx* ctx, int col, pqg_staged_output* out);
/* memcpy of n bytes spread over up to 8 host threads (large copies out of pinned memory). */
void pqg_copy_out(void* dst, const void* src, uint64_t n);

/* ---- ParquetReadRouter boundary --------------------------------------------
 * Batch of bit-packed runs on the device: run r unpacks counts[r] (multiple of 8)
 * LSB-first values of `bit_width` bits from d_in + in_offsets[r] into
 * d_out + out_offsets[r] (int32). Bit-exact with Packer.LITTLE_ENDIAN
 * BytePacker.unpack8Values (ByteBasedBitPackingGenerator.java:258-308). */
int pqg_unpack_runs(pqg_ctx* ctx, int bit_width, const uint8_t* d_in,
                    const uint64_t* d_in_offsets, const uint32_t* d_counts,
                    const uint64_t* d_out_offsets, int32_t* d_out, int n_runs);

/* ParquetReadRouter.read equivalent on host buffers: consumes
 * count*bit_width/8 bytes of `in` (in_len must cover them, else PQG_ERR_EOF as
 * SingleBufferInputStream.slice throws EOFException) and writes `count` ints.
 * The unpack runs on the GPU (H2D, kernel, D2H); synchronous. A parity entry for the router's
 * call shape: one call per run pays a PCIe round trip, so batch runs through pqg_unpack_runs
 * (device buffers) or decode whole pages with pqg_decode. */
int pqg_router_read(pqg_ctx* ctx, int bit_width, const uint8_t* in, size_t in_len,
                    int count, int32_t* out);

/* Many router reads in one round trip (host buffers): run r is ParquetReadRouter.read(bit_width,
 * in positioned at in_offsets[r], counts[r], ...) and its counts[r] ints go to out + (sum of the
 * earlier counts). One H2D of the bytes the runs cover, one kernel, one D2H, one synchronisation
 * for the whole batch (a page's bit-packed runs, say). counts[r] must be a multiple of 8 (a
 * bit-packed run's currentCount); a run whose counts[r] * bit_width / 8 bytes pass in_len ->
 * PQG_ERR_EOF with nothing written (SingleBufferInputStream.slice throws EOFException before the
 * unpack). Synchronous. */
int pqg_router_read_runs(pqg_ctx* ctx, int bit_width, const uint8_t* in, size_t in_len,
                         const uint64_t* in_offsets, const uint32_t* counts, int n_runs, int32_t* out);

/* ParquetReadRouter.read (parquet-plugins/parquet-encoding-vector/.../ParquetReadRouter.java:57-66)
 * with its contract kept — out[0 .. count) holds the run's values when the call returns — at one
 * device round trip per page instead of per run. `in` is the caller's stream at the run's data start
 * and `stream_left` the bytes left in that stream (ByteBufferInputStream.available(): the run's bytes
 * and everything after them). On a miss the hybrid stream after the run is walked on the host
 * (RunLengthBitPackingHybridDecoder.readNext header forms), this run and every later bit-packed run
 * found are unpacked in one pqg_router_read_runs call, and the results are kept in the context; a
 * later call for a walked run (same width, count, position from the end, and bytes) is served from
 * host memory with no device work. The caller advances its stream by count*bit_width/8 bytes, as
 * after readBatch. Errors as pqg_router_read: count not a multiple of 8 -> INVALID_ARG; the run's
 * bytes past stream_left -> PQG_ERR_EOF (SingleBufferInputStream.slice) with nothing written. */
int pqg_router_read_page(pqg_ctx* ctx, int bit_width, const uint8_t* in, size_t stream_left, int count,
                         int32_t* out);

/* The cache probe of pqg_router_read_page alone (host only, never a device call): needs only the
 * run's count*bit_width/8 bytes at `run`. *hit = 1 with out filled, or 0 with nothing written (then
 * call pqg_router_read_page with the whole stream tail). For callers whose stream tail costs a copy
 * (the JNI shim's heap arrays). */
int pqg_router_cache_lookup(pqg_ctx* ctx, int bit_width, const uint8_t* run, size_t stream_left, int count,
                            int32_t* out, int* hit);

/* Reads served from the page cache (hits) and device round trips (misses) since the context was
 * created. */
int pqg_router_cache_stats(pqg_ctx* ctx, uint64_t* hits, uint64_t* misses);

/* ---- record assembly ---------------------------------------------------------
 * Dremel assembly of ONE leaf column into the columnar form of its records: the
 * Arrow-style equivalent of the converter events parquet-mr's automaton emits
 * (RecordReaderImplementation.read, parquet-column/src/main/java/org/apache/parquet/io/RecordReaderImplementation.java:409-446,
 * built by MessageColumnIO.getRecordReader, io/MessageColumnIO.java:77-130).
 *
 * `path` lists the schema nodes from the root's child down to the leaf. Entries of
 * repetition depth r are the records (r = 0) or the elements of the r-th REPEATED node.
 * A non-REPEATED node has one entry per entry of its depth (the number of REPEATED nodes
 * at or above it); a REPEATED node's entries are its elements. Outputs (device pointers):
 *   OPTIONAL node: validity[entry] = 1 when the node is present (a group the automaton opens,
 *                  or a non-null leaf value);
 *   REPEATED node: offsets[e] for every entry e of the enclosing depth, plus offsets[n] =
 *                  this node's entry count (a list's elements are offsets[e] .. offsets[e+1]).
 * The leaf's non-null values are the dense values pqg_decode wrote for the column.
 * d_def_levels / d_rep_levels: the u8 levels pqg_decode wrote (NULL when the max level is 0).
 * Synchronous. When an output is too small, returns PQG_ERR_INVALID_ARG with every
 * n_entries filled in (nothing written). Outputs sized for the bound (validity: n_slots
 * entries, offsets: n_slots + 1) are written in one pass with a single synchronisation;
 * smaller ones are checked against the counted entries first (one extra round trip). */
enum pqg_repetition { PQG_REQUIRED = 0, PQG_OPTIONAL = 1, PQG_REPEATED = 2 };

typedef struct pqg_assembly_node {
  int32_t repetition;      /* pqg_repetition (parquet-format FieldRepetitionType) */
  int32_t reserved;
  uint8_t* validity;       /* OPTIONAL: 1 byte per entry; may be NULL */
  int64_t* offsets;        /* REPEATED: offsets[n_enclosing_entries + 1]; may be NULL */
  uint64_t capacity;       /* elements the validity / offsets array holds */
  uint64_t n_entries;      /* OUT: entries of this node */
} pqg_assembly_node;

int pqg_assemble(pqg_ctx* ctx, const uint8_t* d_def_levels, const uint8_t* d_rep_levels, uint64_t n_slots,
                 pqg_assembly_node* path, int depth, uint64_t* n_records, pqg_status* st);

/* Record assembly of every leaf of a schema: the columnar form of what the automaton emits when it
 * interleaves all leaves of each record (RecordReaderImplementation ctor :253-330 builds the
 * transitions between leaves — nextColumnIdxForRepLevel, levelToClose — and read() :409-446 walks
 * them). `nodes` is the schema below the message root in depth-first order, each naming its parent
 * (-1: a child of the root); `leaves` gives the levels pqg_decode wrote for each leaf node. Every
 * node's outputs (validity / offsets, as in pqg_assembly_node) come from the first leaf under it in
 * schema order; the other leaves under a node must agree on its entry count, and all leaves on the
 * record count, or the call fails with PQG_ERR_CORRUPT (st->page = the leaf, st->value_index = the
 * node). Synchronous. */
typedef struct pqg_schema_node {
  int32_t parent;          /* index of the parent node (< this index), -1 for a child of the root */
  int32_t repetition;      /* pqg_repetition */
  uint8_t* validity;       /* OPTIONAL: 1 byte per entry; may be NULL */
  int64_t* offsets;        /* REPEATED: offsets[n_enclosing_entries + 1]; may be NULL */
  uint64_t capacity;       /* elements the validity / offsets array holds */
  uint64_t n_entries;      /* OUT: entries of this node */
} pqg_schema_node;

typedef struct pqg_schema_leaf {
  int32_t node;            /* index of the leaf in `nodes` */
  int32_t reserved;
  const uint8_t* d_def_levels;  /* device, NULL when the leaf's max definition level is 0 */
  const uint8_t* d_rep_levels;  /* device, NULL when the leaf's max repetition level is 0 */
  uint64_t n_slots;
} pqg_schema_leaf;

int pqg_assemble_schema(pqg_ctx* ctx, pqg_schema_node* nodes, int n_nodes, const pqg_schema_leaf* leaves, int n_leaves,
                        uint64_t* n_records, pqg_status* st);

/* ---- page decompression (codec SNAPPY) --------------------------------------
 * Replaces the decompression step between the page reader and the value readers:
 * ColumnChunkPageReadStore.readPage (parquet-hadoop/src/main/java/org/apache/parquet/hadoop/ColumnChunkPageReadStore.java:144-172
 * for V1 pages, :218-247 for the data section of compressed V2 pages) calling
 * BytesInputDecompressor.decompress -> SnappyDecompressor (parquet-hadoop/.../hadoop/codec/SnappyDecompressor.java),
 * i.e. xerial Snappy.uncompress of one raw Snappy block into a buffer of the header's
 * uncompressed size. Job j decompresses d_src[src_offset, src_offset + src_size) into
 * d_dst[dst_offset, dst_offset + dst_size); a block whose length varint differs from dst_size
 * or that is malformed fails with PQG_ERR_CORRUPT. d_jobs is a DEVICE array; d_status (device,
 * n_jobs int32, may be NULL) receives each job's code. Asynchronous on the context's stream;
 * pqg_snappy_sync reports the first failing job (st->page = job index). */
typedef struct pqg_snappy_job {
  uint64_t src_offset;
  uint64_t dst_offset;
  uint32_t src_size;
  uint32_t dst_size;
} pqg_snappy_job;

int pqg_snappy_decompress(pqg_ctx* ctx, const uint8_t* d_src, uint64_t src_bytes, uint8_t* d_dst, uint64_t dst_bytes,
                          const pqg_snappy_job* d_jobs, int n_jobs, int32_t* d_status);
int pqg_snappy_sync(pqg_ctx* ctx, const int32_t* d_status, int n_jobs, pqg_status* st);

/* ---- page decompression (codec ZSTD) ------------------------------------------
 * The same step for ZSTD pages: ZstandardCodec -> ZstdDecompressorStream
 * (parquet-hadoop/src/main/java/org/apache/parquet/hadoop/codec/ZstdDecompressorStream.java:31-46,
 * zstd-jni's ZstdInputStream over libzstd) read for exactly the header's uncompressed size
 * (ColumnChunkPageReadStore.java:144-172). Job j decodes the Zstandard frames (RFC 8878; skippable
 * frames skipped, concatenated frames in order) in d_src[src_offset, + src_size) and keeps the first
 * dst_size bytes at d_dst + dst_offset. Frames that end before dst_size -> PQG_ERR_EOF; a malformed
 * frame, a frame content size or content checksum (XXH64) that does not match -> PQG_ERR_CORRUPT;
 * dictionaries are not supported (a frame naming one -> CORRUPT). Asynchronous on the context's
 * stream; the context keeps 128 KiB of device scratch per decoding wave (at most 4,096 waves, each
 * looping over the jobs: 512 MiB at most, whatever the number of pages); the output is read back
 * only inside each job's [dst_offset, dst_offset + dst_size) (no padding needed). pqg_zstd_sync reports the first
 * failing job (st->page = job index). */
typedef pqg_snappy_job pqg_zstd_job;

int pqg_zstd_decompress(pqg_ctx* ctx, const uint8_t* d_src, uint64_t src_bytes, uint8_t* d_dst, uint64_t dst_bytes,
                        const pqg_zstd_job* d_jobs, int n_jobs, int32_t* d_status);
int pqg_zstd_sync(pqg_ctx* ctx, const int32_t* d_status, int n_jobs, pqg_status* st);

/* LZ4_RAW pages (ColumnChunkPageReadStore.readPage -> Lz4RawDecompressor, parquet-hadoop/.../hadoop/
 * codec/Lz4RawDecompressor.java:26-50, aircompressor's Lz4Decompressor underneath): every job is one
 * raw LZ4 block (lz4 block format) decompressed into exactly dst_size bytes (the header's
 * uncompressed size; another length, or a malformed block -> PQG_ERR_CORRUPT in the job's status).
 * Same job table and calling sequence as pqg_snappy_decompress; pqg_lz4_raw_sync reports the first
 * failing job (st->page = job index). */
typedef pqg_snappy_job pqg_lz4_job;

int pqg_lz4_raw_decompress(pqg_ctx* ctx, const uint8_t* d_src, uint64_t src_bytes, uint8_t* d_dst, uint64_t dst_bytes,
                           const pqg_lz4_job* d_jobs, int n_jobs, int32_t* d_status);
int pqg_lz4_raw_sync(pqg_ctx* ctx, const int32_t* d_status, int n_jobs, pqg_status* st);

/* GZIP pages (ColumnChunkPageReadStore.readPage -> CodecFactory.HeapBytesDecompressor.decompress,
 * parquet-hadoop/.../hadoop/CodecFactory.java:155-182, Hadoop's GzipCodec stream read for exactly the
 * page's size): every job is gzip members (RFC 1952) of DEFLATE data (RFC 1951) read until dst_size
 * bytes are produced. The member completing the page has its trailer unread; an earlier member's ISIZE
 * is checked (its CRC-32 is not recomputed on the device). Fewer bytes than dst_size -> PQG_ERR_EOF,
 * malformed data -> PQG_ERR_CORRUPT in the job's status. Same job table and calling sequence as
 * pqg_snappy_decompress; pqg_gzip_sync reports the first failing job (st->page = job index). */
typedef pqg_snappy_job pqg_gzip_job;

int pqg_gzip_decompress(pqg_ctx* ctx, const uint8_t* d_src, uint64_t src_bytes, uint8_t* d_dst, uint64_t dst_bytes,
                        const pqg_gzip_job* d_jobs, int n_jobs, int32_t* d_status);
int pqg_gzip_sync(pqg_ctx* ctx, const int32_t* d_status, int n_jobs, pqg_status* st);

/* ---- page framing (host) ----------------------------------------------------
 * File bytes in: the page headers of one raw column chunk, as
 * ParquetFileReader.Chunk.readAllPages reads them
 * (parquet-hadoop/src/main/java/org/apache/parquet/hadoop/ParquetFileReader.java:1824-1979;
 * header = Thrift compact PageHeader, Util.readPageHeader,
 * parquet-format-structures/src/main/java/org/apache/parquet/format/Util.java:127-131).
 * Host code: no device needed. */
enum pqg_page_type { PQG_DATA_PAGE = 0, PQG_INDEX_PAGE = 1, PQG_DICTIONARY_PAGE = 2, PQG_DATA_PAGE_V2 = 3 };

typedef struct pqg_page_header {
  int32_t type;                          /* pqg_page_type */
  int32_t uncompressed_page_size;
  int32_t compressed_page_size;
  int32_t has_crc;
  uint32_t crc;
  int32_t num_values;                    /* data pages: slots; dictionary page: entries */
  int32_t encoding;                      /* values encoding / dictionary page encoding */
  int32_t definition_level_encoding;     /* DataPageHeader (V1) */
  int32_t repetition_level_encoding;     /* DataPageHeader (V1) */
  int32_t num_nulls;                     /* DataPageHeaderV2 */
  int32_t num_rows;                      /* DataPageHeaderV2 */
  int32_t definition_levels_byte_length; /* DataPageHeaderV2 */
  int32_t repetition_levels_byte_length; /* DataPageHeaderV2 */
  int32_t is_compressed;                 /* DataPageHeaderV2 (default 1) */
  int32_t is_sorted;                     /* DictionaryPageHeader */
  int32_t reserved;
  uint64_t header_offset;                /* offset of the header in the chunk buffer */
  uint64_t body_offset;                  /* offset of the page body (compressed_page_size bytes) */
} pqg_page_header;

/* CRC-32 (java.util.zip.CRC32) of n bytes, continuing from `crc` (0 to start). */
uint32_t pqg_crc32(uint32_t crc, const uint8_t* data, uint64_t n);

/* Walk the page headers of the chunk bytes [chunk, chunk + chunk_len) until `value_count` data
 * values have been read (ColumnMetaData.num_values; < 0: every header up to the end).
 * DICTIONARY_PAGE, DATA_PAGE and DATA_PAGE_V2 headers go to `headers` in order; other page types
 * are skipped (as readAllPages does). verify_crc != 0: pages whose header has a crc are checked
 * (CRC-32 of the page's compressed bytes) -> PQG_ERR_CRC with st->page = the page.
 * Errors: a second dictionary page, unreadable header, V2 level lengths past the page -> CORRUPT;
 * a body past the chunk -> EOF; value count mismatch at the end -> CORRUPT ("Expected N values in
 * column chunk ..."). *n_headers = headers found; capacity too small -> INVALID_ARG with
 * st->value_index = the count needed. */
int pqg_frame_chunk(const uint8_t* chunk, uint64_t chunk_len, int64_t value_count, int verify_crc,
                    pqg_page_header* headers, int capacity, int* n_headers, pqg_status* st);

/* ColumnMetaData.codec (parquet.thrift CompressionCodec; CompressionCodecName in parquet-mr). */
enum pqg_codec {
  PQG_CODEC_UNCOMPRESSED = 0, PQG_CODEC_SNAPPY = 1, PQG_CODEC_GZIP = 2, PQG_CODEC_LZO = 3,
  PQG_CODEC_BROTLI = 4, PQG_CODEC_LZ4 = 5, PQG_CODEC_ZSTD = 6, PQG_CODEC_LZ4_RAW = 7
};

/* Headers of a chunk placed at byte `chunk_offset` of a batch buffer -> the pqg_page_desc entries
 * of its data pages (column index `column`) and the dictionary fields of `col` (may be NULL).
 * `codec` is the chunk's ColumnMetaData.codec; it alone decides which pages are compressed, as
 * ColumnChunkPageReadStore.readPage does (ColumnChunkPageReadStore.java:147-181, :218-257,
 * readDictionaryPage :313-316): with a codec other than UNCOMPRESSED every V1 data page and the
 * dictionary page are compressed whatever their sizes, a V2 page when its is_compressed flag is set.
 * A compressed page -> PQG_ERR_UNSUPPORTED with st->page = its header index (decompress first:
 * pqg_snappy_decompress / pqg_zstd_decompress, then describe the decompressed layout). An
 * UNCOMPRESSED chunk's pages are taken as they are (CodecFactory.NO_OP_DECOMPRESSOR). A codec
 * outside pqg_codec -> PQG_ERR_INVALID_ARG. Replaces the page loop of
 * ParquetFileReader.Chunk.readAllPages (ParquetFileReader.java:1824-1979) + the decompressor choice. */
int pqg_pages_from_headers(const pqg_page_header* headers, int n_headers, int codec, uint64_t chunk_offset,
                           int column, pqg_column_desc* col, pqg_page_desc* pages, int capacity, int* n_pages,
                           pqg_status* st);

/* ---- record filter (filter2 predicates over decoded columns) ---------------------
 * Record-level evaluation of a parquet-mr FilterPredicate (filter2/predicate/FilterApi.java) over the
 * dense columns pqg_decode wrote, on the device: what FilterCompat.FilterPredicateCompat makes
 * FilteringRecordMaterializer do value by value through IncrementallyUpdatedFilterPredicate
 * (filter2/recordlevel/IncrementallyUpdatedFilterPredicateEvaluator.java:45-61 and the generated
 * ValueInspectors, parquet-generator/.../IncrementallyUpdatedFilterPredicateGenerator.java:198-327).
 * pqg_filter_run and pqg_filter_run_dict take flat columns only (max_rep == 0); a row is null when its
 * definition level is below max_def, and a column no value reached (missing from the file) is null in
 * every row. A repeated column is reached through contains() and pqg_filter_run_records (below).
 *
 * The predicate is an array of nodes in post-order (children before parents, one root: the last
 * node; every other node is the child of exactly one node). pqg_filter_create validates it and
 * applies LogicalInverseRewriter (filter2/predicate/LogicalInverseRewriter.java,
 * LogicalInverter.java:56-114) as FilterCompat.get does: not() is pushed down to the leaves
 * (eq<->notEq, lt<->gtEq, ltEq<->gt, in<->notIn, and<->or), so the program the device runs has no
 * NOT. That is observable: not(lt(x, 5)) is gtEq(x, 5), false on a null row.
 *
 * Leaves compare with the column's PrimitiveComparator (schema/PrimitiveComparator.java:68-207):
 * Boolean.compare; signed int32 / int64, or unsigned with PQG_FILTER_UNSIGNED (UINT_32 / UINT_64);
 * Float.compare / Double.compare (a total order: -0.0 < 0.0, every NaN equal and above +Infinity);
 * unsigned lexicographic bytes then length for BYTE_ARRAY. Null rows: eq / lt / ltEq / gt / gtEq / in
 * are false and notEq / notIn true; eq(c, null) holds on null rows only, notEq(c, null) on the others;
 * an in / notIn set containing null behaves as eq / notEq(c, null) (the reference ignores its other
 * members). PQG_ERR_UNSUPPORTED at creation: INT96 and FIXED_LEN_BYTE_ARRAY columns declared through
 * pqg_filter_create's bare type array (pqg_filter_create_typed, below, declares their width and order,
 * and the signed-integer order of a DECIMAL on BYTE_ARRAY); programs over the limits below. PQG_ERR_INVALID_ARG: lt / ltEq / gt / gtEq on BOOLEAN (IllegalArgumentException in
 * the reference) or against null, a malformed table. */
#define PQG_FILTER_TILE_ROWS 4096          /* rows per device tile (one wave; a multiple of 64) */
#define PQG_FILTER_MAX_NODES 64            /* nodes of the rewritten program */
#define PQG_FILTER_MAX_LITERALS 4096       /* literal cells */
#define PQG_FILTER_MAX_LITERAL_BYTES 16384 /* BYTE_ARRAY literal bytes */

enum pqg_filter_op {
  PQG_FILTER_EQ = 0,
  PQG_FILTER_NOTEQ = 1,
  PQG_FILTER_LT = 2,
  PQG_FILTER_LTEQ = 3,
  PQG_FILTER_GT = 4,
  PQG_FILTER_GTEQ = 5,
  PQG_FILTER_IN = 6,
  PQG_FILTER_NOTIN = 7,
  PQG_FILTER_AND = 8,
  PQG_FILTER_OR = 9,
  PQG_FILTER_NOT = 10,
  PQG_FILTER_CONTAINS = 11 /* unary, on a repeated column: see "record filter on list columns" below */
};

#define PQG_FILTER_NULL_LITERAL 1 /* eq / notEq: the literal is null; in / notIn: the set contains null */
#define PQG_FILTER_UNSIGNED 2     /* INT32 / INT64 column annotated UINT_32 / UINT_64: unsigned order */

typedef struct pqg_filter_node {
  int32_t op;             /* pqg_filter_op */
  int32_t column;         /* leaves: index into column_types / the pqg_filter_column table */
  int32_t left;           /* AND / OR / NOT: child node (smaller index); leaves: -1 */
  int32_t right;          /* AND / OR: second child; otherwise -1 */
  uint32_t flags;         /* PQG_FILTER_* */
  uint32_t literal_begin; /* leaves: first literal cell */
  uint32_t n_literals;    /* eq .. gtEq: 1 (0 with PQG_FILTER_NULL_LITERAL); in / notIn: the set's non-null members */
  uint32_t reserved;      /* 0 (sizeof(pqg_filter_node) = 32) */
} pqg_filter_node;

typedef struct pqg_filter pqg_filter;

/* Host only (no device, no ctx). A literal cell holds the raw value bits in 8 bytes: BOOLEAN 0 / 1,
 * INT32 / FLOAT in the low 4 bytes, INT64 / DOUBLE all 8; BYTE_ARRAY: offset | length << 32 into
 * `literal_bytes`. column_types[c] is the pqg_physical_type of column c. The filter keeps copies of
 * everything it needs. Sets of more than 8 members are sorted by comparator order for the device's
 * binary search. */
int pqg_filter_create(const pqg_filter_node* nodes, int n_nodes, const int32_t* column_types, int n_cols,
                      const uint64_t* literals, int n_literals, const uint8_t* literal_bytes,
                      uint64_t n_literal_bytes, pqg_filter** out, pqg_status* st);
/* The rewritten, NOT-free program in post-order (literal_begin indexes the filter's own literal table).
 * Writes min(cap, count) nodes and returns the count; -1 without a filter. */
int pqg_filter_program(const pqg_filter* filter, pqg_filter_node* out, int cap);
int pqg_filter_destroy(pqg_filter* filter);

/* ---- binary comparators: DECIMAL, FIXED_LEN_BYTE_ARRAY, INT96, FLOAT16 (an addition to ABI 6) ----
 * The reference compares a Binary column (BINARY, FIXED_LEN_BYTE_ARRAY, INT96) with one of three
 * comparators, chosen by PrimitiveType.comparator() from the logical type
 * (schema/PrimitiveType.java:239-413, schema/PrimitiveComparator.java:183-295):
 *   UNSIGNED_BYTES   Binary.lexicographicCompare: BINARY / FLBA without annotation, STRING, ENUM, JSON,
 *                    BSON, UUID, INTERVAL
 *   SIGNED_INTEGER   big-endian two's complement, the shorter side padded with its own sign (an empty
 *                    value is non-negative): DECIMAL on BINARY and on FLBA, and every INT96 column
 *   FLOAT16          Float16.compare of the two little-endian bytes (every NaN one value above +Infinity,
 *                    -0.0 below +0.0): FLOAT16 on FLBA(2)
 * eq / notEq / in / notIn use the comparator too (compare(...) == 0): under SIGNED_INTEGER 00 94 equals
 * 00 00 00 94, an empty literal equals every all-zero value, and in(c, {00 01}) matches a stored 01. */
enum pqg_filter_binary_order {
  PQG_FILTER_ORDER_UNSIGNED_BYTES = 0, /* Binary.lexicographicCompare: unsigned bytes, then length */
  PQG_FILTER_ORDER_SIGNED_INTEGER = 1, /* big-endian two's complement; the shorter side padded with its sign */
  PQG_FILTER_ORDER_FLOAT16 = 2         /* Float16.compare of the two little-endian bytes */
};
typedef struct pqg_filter_column_type { /* sizeof == 16 */
  int32_t physical_type; /* pqg_physical_type */
  int32_t type_length;   /* FIXED_LEN_BYTE_ARRAY: >= 1; INT96: 0 or 12; otherwise 0 */
  int32_t binary_order;  /* pqg_filter_binary_order; 0 for the non-binary types */
  int32_t reserved;      /* 0 */
} pqg_filter_column_type;

/* pqg_filter_create with a width and a comparator per column; pqg_filter_create is this function with
 * type_length = 0 and binary_order = 0 in every column, plus its refusal of INT96 / FLBA columns.
 * Literals of BYTE_ARRAY, FIXED_LEN_BYTE_ARRAY and INT96 columns are all BYTE_ARRAY cells
 * (offset | length << 32 into literal_bytes) of any length, 0 included: the comparators define the
 * result when it differs from the column's width. All eight leaf ops are valid on these columns.
 * PQG_ERR_INVALID_ARG beyond pqg_filter_create's, value_index naming the node (for `reserved`, which is
 * checked on every column, the column): non-zero reserved; type_length or binary_order set on a non-binary type;
 * FLBA with type_length < 1; INT96 with a type_length other than 0 or 12, or an order other than
 * SIGNED_INTEGER (the reference has no other comparator for it); FLOAT16 on anything but FLBA with
 * type_length == 2, or with a literal whose length is not 2; PQG_FILTER_UNSIGNED on a binary column.
 * At run time the column's physical_type must equal the declared one and the element width comes from
 * the filter: values = n_values dense elements of 12 bytes (INT96, 4-byte aligned) or type_length bytes
 * (FLBA, any alignment) as pqg_decode leaves them; a dictionary holds n_entries such elements. Every
 * element load stays inside [values, values + n_values * width). pqg_filter_run, pqg_filter_run_dict and
 * pqg_filter_run_records all take such filters. */
int pqg_filter_create_typed(const pqg_filter_node* nodes, int n_nodes, const pqg_filter_column_type* columns,
                            int n_cols, const uint64_t* literals, int n_literals, const uint8_t* literal_bytes,
                            uint64_t n_literal_bytes, pqg_filter** out, pqg_status* st);

/* One decoded column as pqg_decode left it. max_def == 0: a required column, row r is values[r].
 * max_def > 0: def_levels holds one byte per row and values the dense non-null values in row order;
 * def_levels == NULL then means a column missing from the file (every row null; values unused).
 * BYTE_ARRAY: values = int64 offsets[n_values + 1] into binary_data (value i is bytes
 * [offsets[i], offsets[i + 1]), which must be readable: the offsets are the decoder's own). */
typedef struct pqg_filter_column {
  int32_t physical_type;       /* pqg_physical_type, equal to the filter's column_types[c] */
  int32_t max_def;
  const void* values;          /* device */
  const uint8_t* binary_data;  /* device, BYTE_ARRAY only */
  const uint8_t* def_levels;   /* device, may be NULL */
  uint64_t n_values;           /* dense values behind `values` */
} pqg_filter_column;

/* Device-resident outcome of one pqg_filter_run. */
typedef struct pqg_filter_result {
  uint64_t n_selected;   /* rows the predicate holds on, whatever row_ids_capacity is */
  int32_t error;         /* PQG_OK, or PQG_ERR_INVALID_ARG: a nullable column's rows with dl == max_def
                            differ in number from its n_values (the outputs are then undefined) */
  int32_t error_column;  /* the first such column, -1 without an error */
} pqg_filter_result;

/* Evaluate `filter` on rows [0, n_rows) of `cols` (host array of n_cols entries, the filter's n_cols;
 * only the columns the predicate names are read). Asynchronous on the ctx stream; every output is a
 * DEVICE pointer. d_bitmap: ceil(n_rows / 64) words, row r = bit r & 63 of word r >> 6, the bits past
 * n_rows in the last word 0. d_row_ids (may be NULL): the selected rows ascending, the first
 * row_ids_capacity of them. Every value load is checked against n_values: a wrong n_values gives
 * d_result->error, never a read outside the column. n_rows == 0 is valid.
 * Five launches, none of which waits on another workgroup: per-tile non-null counts of the nullable
 * columns, their scan (one workgroup per column), the evaluation, the scan of the tiles' selected
 * counts, the row ids. */
int pqg_filter_run(pqg_ctx* ctx, const pqg_filter* filter, const pqg_filter_column* cols, int n_cols,
                   uint64_t n_rows, uint64_t* d_bitmap, int64_t* d_row_ids, uint64_t row_ids_capacity,
                   pqg_filter_result* d_result);

/* ---- record filter on dictionary ids (an addition to ABI 6) --------------------------------------
 * A leaf's verdict on a dictionary-encoded column depends on the id alone, so the predicate is
 * evaluated once per dictionary entry and looked up per row: decode ids (PQG_COLUMN_DICTIONARY_IDS),
 * filter on the ids, pqg_take, and only the kept rows are ever materialised. The reference evaluates
 * the predicate per value (IncrementallyUpdatedFilterPredicate) and uses the dictionary only to drop
 * whole row groups (filter2/dictionarylevel/DictionaryFilter.java).
 *
 * The decoded dictionary of one filter column, on the device, in the decoder's layout
 * (fixed width: n_entries elements; BYTE_ARRAY: int64 offsets[n_entries + 1] into binary_data).
 * values == NULL: the column holds values, as for pqg_filter_run. */
typedef struct pqg_filter_dictionary {
  const void* values;
  const uint8_t* binary_data;
  uint32_t n_entries;
  uint32_t reserved;   /* 0; sizeof == 24 */
} pqg_filter_dictionary;

/* Bytes of verdict tables (one bit per dictionary entry and leaf, whole 64-bit words per leaf) up to
 * which pqg_filter_run_dict keeps a program's tables in LDS; above it they are read from global memory.
 * 8 KiB: with a small program (image below 2 KiB) a workgroup then allocates at most 10 KiB, and the 8
 * workgroups of 4 waves a CU holds at the evaluation kernel's register use still fit its 160 KiB. */
#define PQG_FILTER_DICT_LDS_BYTES 8192

/* pqg_filter_run with dictionaries: `dicts` is a host array of n_cols entries, or NULL. For a column c
 * with dicts[c].values != NULL, cols[c].values holds the uint32 ids pqg_decode wrote with
 * PQG_COLUMN_DICTIONARY_IDS (4-byte aligned), cols[c].n_values counts them and cols[c].physical_type is
 * the dictionary's type (the filter's column_types[c]); cols[c].binary_data is unused. Everything else
 * is as for pqg_filter_run, and so are the outputs: bit for bit those of pqg_filter_run on the
 * materialised column dictionary[ids]. With dicts == NULL or no entry set it is pqg_filter_run.
 * A row with a value whose id is >= n_entries gives d_result->error = PQG_ERR_DICT_ID with error_column
 * the lowest such column the predicate names (PQG_ERR_INVALID_ARG from the n_values check takes
 * precedence); the dictionary is never read outside [0, n_entries). n_entries == 0 is valid (a column
 * that is null in every row). PQG_ERR_INVALID_ARG before any launch: a dictionary on a missing column,
 * a BYTE_ARRAY dictionary without binary_data, misaligned ids, non-zero `reserved`.
 * One launch more than pqg_filter_run when a leaf without a null literal stands on a dictionary column:
 * first the verdict of every such leaf on every dictionary entry. */
int pqg_filter_run_dict(pqg_ctx* ctx, const pqg_filter* filter, const pqg_filter_column* cols,
                        const pqg_filter_dictionary* dicts, int n_cols, uint64_t n_rows, uint64_t* d_bitmap,
                        int64_t* d_row_ids, uint64_t row_ids_capacity, pqg_filter_result* d_result);

/* ---- record filter on list columns: contains() (an addition to ABI 6) ------------------------------
 * FilterApi.contains(pred) (filter2/predicate/FilterApi.java:262, Operators.Contains,
 * Operators.java:326-462) is the one filter2 predicate that names a repeated column
 * (SchemaCompatibilityValidator.java:177-214 requires maxRepetitionLevel > 0 for it and refuses every
 * other predicate there). It is evaluated record by record (ContainsPredicate and the
 * expectMultipleResults inspectors, IncrementallyUpdatedFilterPredicateGenerator.java:198-327, 339-537).
 *
 * The node: op PQG_FILTER_CONTAINS, `left` = a leaf node (eq .. notIn) on the repeated column, right = -1,
 * column = -1, no flags, no literals. contains(L) holds on a record iff some slot of the record has
 * def == max_def and L's comparison holds on that slot's value (the comparison a flat leaf makes on a row
 * that has a value). A slot without a value never counts (a null element, an empty list, a null list),
 * so a record with no matching value is false for every op, notEq and notIn included
 * (ContainsPredicate.updateNull), unlike flat notEq. notIn means "some value is not a member of the set",
 * the flat filter's reading of notIn applied per value. A column missing from the file is false in every
 * record. and / or above contains nodes stay plain and / or (ContainsAndPredicate is true iff both inner
 * inspectors became true, each over every value of the record: and(contains(l), contains(r))).
 *
 * pqg_filter_create refuses, in the reference's order (LogicalInverseRewriter, then ContainsRewriter,
 * FilterCompat.java:80-91); pqg_status.value_index names the node:
 *   PQG_ERR_INVALID_ARG  a contains node whose child is not a leaf, or with right != -1, flags or literals
 *                        of its own; a child with PQG_FILTER_NULL_LITERAL (Operators.java:429-435)
 *   PQG_ERR_UNSUPPORTED  a NOT anywhere above a contains (LogicalInverter.java:97-99)
 *   ContainsRewriter.visit(And / Or) on the NOT-free tree from the root (ContainsRewriter.java:100-168):
 *   a side that is a plain leaf returns at once (the other side is not examined); a left side that
 *   rewrites to a Contains with a right side that does not is PQG_ERR_UNSUPPORTED ("cannot be composed
 *   with non-Contains predicates"; the mirror case is accepted); two Contains sides on different columns
 *   are PQG_ERR_INVALID_ARG (Operators.java:377-385).
 * pqg_filter_program reports contains nodes as they are; they count against PQG_FILTER_MAX_NODES. A
 * filter with a contains node is PQG_ERR_INVALID_ARG for pqg_filter_run and pqg_filter_run_dict. */
typedef struct pqg_filter_record_column { /* sizeof == 64 */
  pqg_filter_column col;     /* def_levels: one byte per SLOT for a repeated column */
  int32_t max_rep;           /* 0: flat (rep_levels NULL, n_slots == n_rows) */
  int32_t reserved;          /* 0 */
  const uint8_t* rep_levels; /* device, one byte per slot */
  uint64_t n_slots;
} pqg_filter_record_column;

/* pqg_filter_run_dict over records: n_rows counts RECORDS, a repeated column is a stripe of slots as
 * for pqg_take_records, and the outputs are exactly those of pqg_filter_run indexed by record, so
 * d_bitmap goes straight into pqg_take_records on the same ctx. Only the columns the predicate names are
 * read. Without a contains node and with flat columns only the outputs are byte-identical to
 * pqg_filter_run_dict. `dicts` as there (may be NULL); a repeated column may hold dictionary ids.
 * Refused before any launch, PQG_ERR_INVALID_ARG: everything pqg_filter_run_dict refuses; a contains leaf
 * on a present column with max_rep == 0; any other leaf on a column with max_rep > 0; max_rep outside
 * 0..254, non-zero `reserved`, max_rep > 0 with max_def == 0 or without rep_levels, n_slots < n_rows,
 * max_rep == 0 with rep_levels or with n_slots != n_rows. A missing column (max_def > 0, def_levels NULL)
 * is exempt from these. d_result->error = PQG_ERR_INVALID_ARG with error_column the lowest bad column the
 * predicate names when slot 0 of a repeated column has rep != 0, its record starts differ in number from
 * n_rows, or its slots with def == max_def differ in number from n_values (and as for pqg_filter_run on
 * flat columns); PQG_ERR_DICT_ID as for pqg_filter_run_dict, with lower precedence. In every case no load
 * leaves [0, n_slots), [0, n_values), the dictionary or the bitmap's ceil(n_rows / 64) words; a slot
 * whose record index is -1 or >= n_rows contributes nothing.
 * Launches, none of which waits on another workgroup and whose number does not depend on n_cols: with
 * contains leaves, the record starts and values per (repeated column, tile of PQG_FILTER_TILE_ROWS
 * slots), their scans, and one record bitmap per contains leaf (a wave per tile and group of up to four
 * contains leaves of one column, which share one load of the value; at most two 64-bit atomic ORs per
 * leaf and wave, for the words a record spanning tiles shares); then the launches of
 * pqg_filter_run_dict, whose evaluation reads a contains node's 64 records as one word of that bitmap. */
int pqg_filter_run_records(pqg_ctx* ctx, const pqg_filter* filter, const pqg_filter_record_column* cols,
                           const pqg_filter_dictionary* dicts, int n_cols, uint64_t n_rows, uint64_t* d_bitmap,
                           int64_t* d_row_ids, uint64_t row_ids_capacity, pqg_filter_result* d_result);

/* Decode the dictionary page `col` names (dict_offset, dict_size, dict_num_values, dict_encoding,
 * physical_type, type_length; d_bytes / n_bytes as for pqg_decode) into col->values / col->binary_data
 * within values_capacity / binary_capacity, any physical type: the PLAIN values of a required column
 * (PlainValuesDictionary). The levels, max_rep / max_def and flags of `col` are ignored. Errors the
 * descriptor shows are returned at once (PQG_ERR_NO_DICTIONARY, PQG_ERR_DICT_ENCODING, PQG_ERR_EOF for a
 * fixed-width page shorter than its entries, capacities); otherwise asynchronous like pqg_decode, which
 * it counts as: col->values_written and the remaining errors are valid after pqg_sync, and `col` must
 * stay alive until then. */
int pqg_decode_dictionary(pqg_ctx* ctx, const uint8_t* d_bytes, uint64_t n_bytes, pqg_column_desc* col, pqg_status* st);

/* pqg_decode_dictionary for n dictionary pages of one buffer in one plan (an addition to ABI 6): cols[i] names
 * dictionary page i, with its own type and its own output buffers. The checks, the error codes, values_written
 * after pqg_sync and the capacity contract are those of pqg_decode_dictionary, per entry; st->page is the index
 * of the failing dictionary (a descriptor error: the first such entry, and nothing is launched). `cols` must
 * stay alive until pqg_sync. n == 0 is valid and launches nothing. The number of launches does not depend on n:
 * the pages are the n required one-page columns of one plan, whose PLAIN BYTE_ARRAY pages take one wave each
 * (the form PQG_DISPATCH_PLAIN_ONE_PASS = 3 selects, which waits on no other workgroup), whatever the ctx's
 * dispatch setting says. The dictionary pages of every row group of a file can so be decoded before any data
 * page is uploaded (pqg_filter_row_groups, below). */
int pqg_decode_dictionaries(pqg_ctx* ctx, const uint8_t* d_bytes, uint64_t n_bytes, pqg_column_desc* cols, int n,
                            pqg_status* st);

/* ---- row-group dictionary filter (an addition to ABI 6) -------------------------------------------
 * Before a reader with a predicate reads anything it asks which row groups it has to read at all
 * (RowGroupFilter.visit(FilterPredicateCompat), filter2/compat/RowGroupFilter.java:100-115). Its
 * dictionary level is DictionaryFilter.canDrop (filter2/dictionarylevel/DictionaryFilter.java): a row
 * group is dropped when every data page of the column is dictionary-encoded and no dictionary entry can
 * satisfy the predicate. pqg_filter_row_groups answers that for all row groups of a file in one call;
 * what a dropped row group holds is then never uploaded. StatisticsFilter and BloomFilterImpl, the other
 * two levels, are host-only metadata work and not part of this.
 *
 * Host only. DictionaryFilter.hasNonDictionaryPages (DictionaryFilter.java:561-589) over a chunk's
 * ColumnMetaData.encoding_stats (`stats`, n_stats entries; n_stats < 0: the chunk has none) and its
 * `encodings` list. With stats they are converted as ParquetMetadataConverter.convertEncodingStats does
 * (:689-709): the encodings of DATA_PAGE and DATA_PAGE_V2 entries form the data set, an entry with count
 * 0 included; DICTIONARY_PAGE entries are ignored. Then EncodingStats.hasNonDictionaryEncodedPages
 * (EncodingStats.java:77-94) with its short circuit: RLE_DICTIONARY is removed first and PLAIN_DICTIONARY
 * only if RLE_DICTIONARY was absent, so a chunk that lists both returns 1; an empty data set returns 0.
 * Without stats: PLAIN_DICTIONARY must be among `encodings` and nothing else but RLE and BIT_PACKED,
 * otherwise 1 (a chunk with RLE_DICTIONARY only returns 1). Returns 0 or 1. */
typedef struct pqg_page_encoding_stat { int32_t page_type, encoding, count; } pqg_page_encoding_stat; /* sizeof == 12 */
int pqg_chunk_has_non_dictionary_pages(const pqg_page_encoding_stat* stats, int n_stats, /* < 0: no encoding_stats */
                                       const int32_t* encodings, int n_encodings);

/* What the host knows of one column chunk of one row group. */
#define PQG_RG_MISSING            1  /* the file has no such column (meta == null) */
#define PQG_RG_NO_DICTIONARY      2  /* no dictionary page was read (expandDictionary returns null) */
#define PQG_RG_NON_DICT_PAGES     4  /* pqg_chunk_has_non_dictionary_pages */
#define PQG_RG_MAY_CONTAIN_NULL   8  /* statistics absent, num_nulls unset or > 0 */
typedef struct pqg_rowgroup_column {     /* sizeof == 32; entry [g * n_cols + c] of a host table */
  pqg_filter_dictionary dict;            /* decoder layout, device pointers, as for pqg_filter_run_dict */
  uint32_t flags; uint32_t reserved;     /* PQG_RG_*; reserved == 0 */
} pqg_rowgroup_column;
/* Device-resident outcome of one pqg_filter_row_groups. */
typedef struct pqg_rowgroup_result {     /* sizeof == 16 */
  uint64_t n_kept;      /* row groups that might match, whatever kept_capacity is */
  int32_t error;        /* PQG_OK (no launch of this call reports an error of its own today) */
  int32_t error_group;  /* -1 */
} pqg_rowgroup_result;

/* DictionaryFilter.canDrop for n_row_groups row groups. The predicate is the filter's rewritten program,
 * which has no NOT: what RowGroupFilter passes after LogicalInverseRewriter. Filters with contains are
 * accepted. `cols` is a host table of n_row_groups * n_cols entries (n_cols: the filter's); only the
 * columns the predicate names are read. Asynchronous on the ctx stream; every output is a DEVICE pointer.
 * d_drop_bitmap: ceil(n_row_groups / 64) words, bit g set when row group g cannot match, the bits past
 * n_row_groups 0. d_kept_ids (may be NULL): the kept groups ascending, the first kept_capacity of them.
 * n_row_groups == 0 is valid.
 *
 * The dictionary of a (row group, column) is "usable" when none of MISSING, NO_DICTIONARY, NON_DICT_PAGES
 * is set and the column's type is INT32, INT64, FLOAT, DOUBLE, BYTE_ARRAY or FIXED_LEN_BYTE_ARRAY; BOOLEAN
 * and INT96 never drop (expandDictionary, DictionaryFilter.java:91-131). any(L): leaf L holds on at least
 * one dictionary entry taken as a present value. A leaf CANNOT match when:
 *   eq(null), in with null in the set        never (:136-141, :384-390)
 *   notEq(null)                              the column is MISSING (:177-181)
 *   notIn whose set is exactly {null}        the column is MISSING (:446-450)
 *   notIn with null among other members      never (:452-456)
 *   eq lt ltEq gt gtEq in (non-null literal) MISSING, or the dictionary is usable and not any(L)
 *                                            (:143-169, :218-380, :392-437)
 *   notEq(v)                                 usable, n_entries >= 1, not any(L), MAY_CONTAIN_NULL clear: every
 *                                            entry equals v (dictSet.size() == 1 && contains, :183-215)
 *   notIn(S), no null in S                   usable, not any(L), MAY_CONTAIN_NULL clear (:458-489; MISSING
 *                                            gives MIGHT_MATCH)
 * so an empty usable dictionary cannot match eq, in, the ordering leaves and notIn, and might match notEq.
 * Duplicate entries change nothing (the reference compares against a HashSet). `and` cannot match if either
 * side cannot, `or` only if both cannot (:496-504, the inverted and / or of a "can drop" visitor),
 * contains(L) takes L's verdict (Operators.java:459-461, DictionaryFilter.java:492-494); the root's verdict
 * is the drop bit.
 * Equality is equals(), not the comparator: eq, notEq, in and notIn go through HashSet.contains. For a
 * Binary that is byte equality whatever the column's order: a DECIMAL on BYTE_ARRAY stored as 00 01 does
 * not equal the literal 01 here though pqg_filter_run says it does, and FLOAT16 NaNs with different
 * payloads differ. For FLOAT and DOUBLE equals() is the comparator's equality (one NaN, -0.0 != 0.0). So
 * the row-group form of the program keys the equality leaves of binary columns by their unsigned bytes
 * (sets of more than 8 members re-sorted for the binary search); ordering leaves keep the comparator.
 *
 * Refused before any launch, PQG_ERR_INVALID_ARG: a NULL ctx, filter or d_result; n_row_groups > 0 without
 * cols or d_drop_bitmap; n_cols different from the filter's; non-zero `reserved` or unknown flags in a
 * column the predicate names; a usable BYTE_ARRAY dictionary with entries but without binary_data, or any
 * usable dictionary with entries but without values; more than 2^31 - 1 row groups or 2^26 work items
 * (a work item is PQG_RG_TILE_ENTRIES entries of one dictionary).
 * No load leaves [0, n_entries) of a dictionary or, for BYTE_ARRAY, [offsets[0], offsets[n_entries]) of
 * its bytes (offsets are clamped).
 * Launches, none of which waits on another workgroup, without atomics, and whose number does not depend
 * on n_row_groups or n_cols: k_rg_any (a wave per (row group, column, tile of PQG_RG_TILE_ENTRIES entries)
 * of a host-built work list, every leaf of the column on one load of the entry; a hit stores 1 into the
 * (row group, leaf) flag, zeroed in the stream beforehand), k_rg_fold (a lane per row group: the program
 * over the flags, the bitmap word by ballot, the kept count per word), the scan of those counts with the
 * result, and the kept ids. */
#define PQG_RG_TILE_ENTRIES 1024
int pqg_filter_row_groups(pqg_ctx* ctx, const pqg_filter* filter, const pqg_rowgroup_column* cols, int n_cols,
                          uint64_t n_row_groups, uint64_t* d_drop_bitmap, int64_t* d_kept_ids,
                          uint64_t kept_capacity, pqg_rowgroup_result* d_result);

/* ---- row selection ------------------------------------------------------------------------------
 * The last step of decode -> filter -> records: the rows a bitmap keeps, gathered into compact
 * columns in the decoder's own layout. What is reproduced is what the reference hands back after a
 * record filter or a column-index skip: RecordReaderImplementation.read drops the records
 * shouldSkipCurrentRecord names (RecordReaderImplementation.java:440-449,
 * filter2/recordlevel/FilteringRecordMaterializer.java), and SynchronizingColumnReader skips the rows
 * outside the RowRanges (column/impl/SynchronizingColumnReader.java,
 * internal/filter2/columnindex/RowRanges.java). The kept records appear in row order, unchanged: every
 * column shows exactly the value or null it had. The selection is a bitmap, so the bitmap
 * pqg_filter_run wrote and a host-built bitmap of row ranges are equally valid inputs.
 *
 * Element widths: BOOLEAN 1 byte, INT32 / FLOAT / dictionary ids 4, INT64 / DOUBLE 8, INT96 12,
 * FIXED_LEN_BYTE_ARRAY type_length. `values` / `out_values` are naturally aligned for 1 / 4 / 8,
 * 4-byte aligned for INT96, 8-byte aligned for BYTE_ARRAY offsets, unaligned for FIXED_LEN_BYTE_ARRAY. */
#define PQG_TAKE_MAX_COLUMNS 64 /* columns per call; more -> PQG_ERR_UNSUPPORTED */

typedef struct pqg_take_column {
  int32_t physical_type;        /* any pqg_physical_type */
  int32_t max_def;              /* as pqg_filter_column */
  int32_t type_length;          /* FIXED_LEN_BYTE_ARRAY; 0 otherwise */
  int32_t flags;                /* PQG_COLUMN_DICTIONARY_IDS: values are uint32 ids (4-byte elements) */
  const void* values;           /* device, as pqg_decode left it (BYTE_ARRAY: int64 offsets[n_values + 1]) */
  const uint8_t* binary_data;   /* device, BYTE_ARRAY only */
  const uint8_t* def_levels;    /* device; NULL with max_def > 0: missing column, every row null */
  uint64_t n_values;
  void* out_values;             /* device; BYTE_ARRAY: int64 offsets, out_offsets[0] = 0 */
  uint8_t* out_binary_data;     /* device, BYTE_ARRAY only */
  uint8_t* out_def_levels;      /* device, one byte per kept row; NULL allowed when max_def == 0 (a required
                                   column has no levels: never written) or the column is missing */
  uint64_t out_values_capacity; /* elements (BYTE_ARRAY: values; out_values holds capacity + 1 offsets) */
  uint64_t out_binary_capacity; /* bytes */
} pqg_take_column;

/* Per column, device-resident: the full counts whatever the capacities are. */
typedef struct pqg_take_counts {
  uint64_t n_values; /* dense values of the kept rows (a required column: the kept rows) */
  uint64_t n_bytes;  /* BYTE_ARRAY: bytes of those values; 0 otherwise */
} pqg_take_counts;

/* Device-resident outcome of one pqg_take. */
typedef struct pqg_take_result {
  uint64_t n_rows;      /* kept rows, whatever out_rows_capacity is */
  int32_t error;        /* PQG_OK, or PQG_ERR_INVALID_ARG: a nullable column's rows with dl == max_def differ
                           in number from its n_values, or a count exceeds a capacity (kept rows over
                           out_rows_capacity, which counts against every column; a column's values over
                           out_values_capacity; its bytes over out_binary_capacity). The outputs are then
                           undefined, but no byte is written past a stated capacity */
  int32_t error_column; /* the lowest such column, -1 without an error (or with no columns) */
} pqg_take_result;

/* Gather the rows of [0, n_rows) whose bit is set in d_bitmap (row r = bit r & 63 of word r >> 6, the
 * layout pqg_filter_run writes; bits past n_rows in the last word are ignored) into the outputs of
 * `cols` (host array of n_cols entries). Asynchronous on the ctx stream: after a pqg_filter_run on the
 * same ctx no synchronisation is needed. Per column, for the kept rows in ascending order:
 * out_def_levels[j] = the level byte of the j-th kept row; out_values = the dense values of the kept
 * non-null rows (a required column: one per kept row); BYTE_ARRAY: offsets from 0, bytes packed without
 * gaps, out_offsets[n_values_out] written also when nothing was kept and no slot past it. A missing
 * column produces nothing but its counts, which are 0. Every value load is checked against n_values and
 * every store against the capacities. n_rows == 0 and n_cols == 0 are valid (n_cols == 0: just the
 * kept-row count). Refused before any launch, PQG_ERR_INVALID_ARG: a NULL ctx / d_counts / d_result,
 * n_rows > 0 without a bitmap, max_def outside 0..254, FIXED_LEN_BYTE_ARRAY with type_length <= 0, a
 * misaligned or missing pointer the column needs (values with n_values > 0, offsets and bytes of a
 * BYTE_ARRAY column, out_values with a capacity, out_def_levels of a nullable column with
 * out_rows_capacity > 0), a required column with n_values < n_rows; PQG_ERR_UNSUPPORTED: more than
 * PQG_TAKE_MAX_COLUMNS columns. Repeated columns are out of scope (no repetition levels here;
 * pqg_take_records below takes them).
 * Launches, none of which waits on another workgroup and whose number does not depend on n_cols: per
 * (column, tile) counts, their scans, with BYTE_ARRAY columns the kept bytes per tile and their scan,
 * the verdicts, the gather (one wave per column and tile of PQG_FILTER_TILE_ROWS rows). */
int pqg_take(pqg_ctx* ctx, const uint64_t* d_bitmap, uint64_t n_rows, const pqg_take_column* cols, int n_cols,
             uint64_t out_rows_capacity, pqg_take_counts* d_counts, pqg_take_result* d_result);

/* ---- record selection on repeated columns (an addition to ABI 6) ----------------------------------
 * pqg_take for schemas with lists: the bitmap names RECORDS, and every leaf loses the same records,
 * nested leaves included. That is what the reference does: RecordReaderImplementation.read drops a
 * whole record when shouldSkipCurrentRecord says so (RecordReaderImplementation.java:440-449,
 * FilteringRecordMaterializer), and SynchronizingColumnReader skips the rows outside the RowRanges;
 * both act on records. Of its record filters only contains() can name a repeated column
 * (SchemaCompatibilityValidator: "FilterPredicates do not currently support repeated columns" for every
 * other predicate), but the filter's result applies to all columns of the record: the normal case is a
 * filter on flat columns, or a contains() on a list, and a take on every column.
 *
 * A repeated leaf is a stripe of SLOTS (one repetition byte and one definition byte per slot, dense
 * values for the slots with def == max_def), as pqg_decode writes it. Record i of a column is the run of
 * slots from the i-th slot with rep == 0 up to the next such slot. */
typedef struct pqg_take_record_column {
  pqg_take_column col;         /* as for pqg_take; def_levels / out_def_levels hold one byte per SLOT */
  int32_t max_rep;             /* 0: a flat column (rep_levels NULL, n_slots == n_rows, out_rep_levels unused) */
  int32_t reserved;            /* 0 */
  const uint8_t* rep_levels;   /* device, one byte per slot, as pqg_decode wrote them */
  uint64_t n_slots;
  uint8_t* out_rep_levels;     /* device, one byte per kept slot */
  uint64_t out_slots_capacity; /* bounds out_rep_levels and out_def_levels of this column */
} pqg_take_record_column;

/* Per column, device-resident. */
typedef struct pqg_take_record_counts {
  uint64_t n_records; /* record starts found in the column, whatever n_rows is (a flat column: n_rows;
                         a missing column: 0) */
  uint64_t n_slots;   /* kept slots (a flat column: kept rows), whatever the capacities are */
  uint64_t n_values;  /* dense values of the kept slots, whatever the capacities are */
  uint64_t n_bytes;   /* BYTE_ARRAY: bytes of those values; 0 otherwise */
} pqg_take_record_counts;

/* Keep the records of [0, n_rows) whose bit is set in d_bitmap (the layout of pqg_take; bits past n_rows
 * in the last word are ignored). A slot is kept iff its record's bit is set. Per column, for the kept
 * slots in slot order: out_rep_levels and out_def_levels are copied byte for byte (repetition values
 * above 0 are not interpreted); out_values holds the dense values of the kept slots with def == max_def;
 * BYTE_ARRAY columns get offsets from 0, bytes without gaps and the closing offset always written, as
 * for pqg_take; a missing column (max_def > 0, def_levels == NULL) produces only zero counts; dictionary
 * ids travel as 4-byte elements. A column with max_rep == 0 gives outputs byte-identical to pqg_take on
 * `col` (out_rows_capacity bounds its level bytes, as there). d_result->n_rows is the number of kept
 * records. The outputs are valid inputs to pqg_take_records again and to pqg_assemble.
 * d_result->error = PQG_ERR_INVALID_ARG with error_column the lowest bad column when: slot 0 of a
 * repeated column has rep != 0; the column's record starts differ in number from n_rows; its slots with
 * def == max_def differ in number from n_values; the kept records exceed out_rows_capacity (against
 * every column); the kept slots exceed out_slots_capacity, the kept values out_values_capacity, the kept
 * bytes out_binary_capacity. The outputs are then undefined, but no load leaves [0, n_slots),
 * [0, n_values) or the bitmap's ceil(n_rows / 64) words (a slot whose record index is -1 or >= n_rows is
 * simply not kept), and no store passes a stated capacity.
 * Refused before any launch, PQG_ERR_INVALID_ARG: everything pqg_take refuses for `col`; max_rep outside
 * 0..254 or non-zero `reserved`; max_rep > 0 with max_def == 0 (a repeated node always adds a definition
 * level), without rep_levels (a missing column is exempt), or with out_slots_capacity > 0 but no
 * out_rep_levels or no out_def_levels; n_slots < n_rows on a column that is not missing; max_rep == 0
 * with rep_levels or with n_slots != n_rows. PQG_ERR_UNSUPPORTED: more than PQG_TAKE_MAX_COLUMNS
 * columns. n_rows == 0 and n_cols == 0 are valid.
 * Launches, none of which waits on another workgroup and whose number does not depend on n_cols: the
 * record starts per (repeated column, tile of PQG_FILTER_TILE_ROWS slots), their scan, the expansion of
 * the record bitmap into one slot bitmap per repeated column; then the launches of pqg_take with every
 * column on its own bitmap (a flat column on d_bitmap, a repeated one on its slot bitmap, its repetition
 * bytes gathered as a required 1-byte column on the same bitmap). PQG_DISPATCH_TAKE_STAGED applies.
 * The record filter that looks inside a list is contains() (pqg_filter_run_records, above); its bitmap
 * is a valid d_bitmap here on the same ctx without synchronisation. */
int pqg_take_records(pqg_ctx* ctx, const uint64_t* d_bitmap, uint64_t n_rows, const pqg_take_record_column* cols,
                     int n_cols, uint64_t out_rows_capacity, pqg_take_record_counts* d_counts,
                     pqg_take_result* d_result);

/* ---- page checksums (an addition to ABI 6) ----------------------------------------------------------
 * ParquetFileReader.Chunk.readAllPages -> verifyCrc (ParquetFileReader.java:1805-1813): with
 * parquet.page.verify-checksum.enabled the CRC-32 of a page's bytes as they sit in the file (V2: the
 * level sections and the data together, :1925-1931) is compared with PageHeader.crc before anything
 * else touches the page. pqg_crc32_pages computes the checksums of many byte ranges of one device
 * buffer, the same bytes the codec kernels or pqg_decode read afterwards.
 *
 * CRC-32 is linear over GF(2): a range splits into tiles of PQG_CRC_TILE_BYTES whose partial values
 * are computed independently (one wave per tile) and folded per job by a second launch. No workgroup
 * waits on another and there are no atomics. */
#define PQG_CRC_TILE_BYTES 32768    /* bytes of a range one wave checksums (the fastest of 4, 8, 16 and
                                       32 KiB: DESIGN.md §3); PQG_DISPATCH_CRC_TILE_BYTES */
#define PQG_CRC_VERIFY 1            /* pqg_crc_job.flags: compare with `expected` */

typedef struct pqg_crc_job {        /* sizeof == 24 */
  uint64_t offset;    /* first byte of the checksummed range in d_bytes, any alignment */
  uint32_t size;      /* bytes; 0 is valid (CRC 0) */
  uint32_t expected;  /* PageHeader.crc as an unsigned 32-bit value */
  uint32_t flags;     /* PQG_CRC_* */
  uint32_t reserved;  /* 0 */
} pqg_crc_job;

/* d_crc[j] (device, n_jobs, may be NULL) <- java.util.zip.CRC32 of d_bytes[offset, offset + size) of
 * job j (the reflected polynomial 0xEDB88320: what pqg_crc32 and zlib's crc32 compute); d_status[j]
 * (device, n_jobs) <- PQG_OK, or PQG_ERR_CRC when the job has PQG_CRC_VERIFY and the value differs from
 * `expected` (an unsigned comparison, as verifyCrc masks with 0xffffffffL). Asynchronous on the ctx
 * stream. `jobs` is a HOST array (its sizes come from page headers the host parsed); it is copied
 * before the call returns, through growable pinned memory of the ctx. Jobs are independent: they may
 * overlap, repeat and come in any order, and bytes outside a job's range never influence its result.
 * d_bytes is 4-byte aligned and readable up to n_bytes rounded up to 4; no load leaves that range.
 * PQG_ERR_INVALID_ARG, before any launch: NULL ctx; n_jobs < 0; NULL jobs, d_bytes or d_status with
 * n_jobs > 0; a job with offset + size > n_bytes; non-zero reserved; unknown flags.
 * PQG_ERR_UNSUPPORTED: more than 2^28 tiles in one call. n_jobs == 0 is valid and launches nothing.
 * Launches: two (per-tile partials, per-job fold), whatever n_jobs is. */
int pqg_crc32_pages(pqg_ctx* ctx, const uint8_t* d_bytes, uint64_t n_bytes, const pqg_crc_job* jobs, int n_jobs,
                    uint32_t* d_crc, int32_t* d_status);
/* Synchronises the ctx stream and reads d_status back, like the codec *_sync calls: the first failing
 * job is st->page, and the message of a mismatch contains "CRC checksum verification failed". */
int pqg_crc32_sync(pqg_ctx* ctx, const int32_t* d_status, int n_jobs, pqg_status* st);

/* Host only. zlib's crc32_combine: crc(A || B) from crc(A), crc(B) and the length of B (len_b == 0:
 * crc_a ^ crc_b, which zlib's identity gives). For a caller that checksums a page in pieces. */
uint32_t pqg_crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b);
/* Host only. The verifying jobs of a framed chunk (pqg_frame_chunk's headers): every header with
 * has_crc (dictionary page, V1, V2) becomes a job over chunk_offset + body_offset,
 * compressed_page_size bytes, with PQG_CRC_VERIFY and the header's crc; header_of_job[j] (may be NULL)
 * is the header's index. *n_jobs = jobs needed; capacity too small: PQG_ERR_INVALID_ARG with
 * st->value_index = the count needed (as pqg_frame_chunk). */
int pqg_crc_jobs_from_headers(const pqg_page_header* headers, int n_headers, uint64_t chunk_offset, pqg_crc_job* jobs,
                              int32_t* header_of_job, int capacity, int* n_jobs, pqg_status* st);

/* ---- encrypted pages (an addition to ABI 6) ---------------------------------------------------------
 * Parquet Modular Encryption: ColumnChunkPageReadStore decrypts a page between verifyCrc and the
 * decompressor (ColumnChunkPageReadStore.java:140-175, 218-251, 321-322: blockDecryptor.decrypt(bytes,
 * dataPageAAD)). pqg_decrypt_pages decrypts many modules of one device buffer into a second one, where
 * the codec kernels or pqg_decode read the plaintext afterwards.
 *
 * A job is one module as BlockCipher.Encryptor wrote it:
 *   PQG_DECRYPT_GCM  [4-byte LE length][12-byte nonce][ciphertext][16-byte tag]   (AesGcmDecryptor)
 *   PQG_DECRYPT_CTR  [4-byte LE length][12-byte nonce][ciphertext]                (AesCtrDecryptor)
 * (AesCipher.SIZE_LENGTH, NONCE_LENGTH, GCM_TAG_LENGTH). The plaintext has src_size - 32 bytes (GCM) or
 * src_size - 16 (CTR). GCM: J0 = nonce || 00000001, the data counter starts at 2, the tag is checked over
 * the AAD and the ciphertext. CTR: the IV is nonce || 00000001, the counter starts at 1, the AAD is
 * ignored and nothing is verified. The value of the length field is skipped, not checked, as in the
 * reference's decrypt(byte[], byte[]).
 *
 * AES-CTR is independent per 16-byte block and GHASH is a polynomial evaluation over GF(2^128): a module
 * splits into tiles of PQG_AES_TILE_BYTES (one wave per tile: keystream, plaintext, the tile's GHASH
 * partial), and a second launch folds the partials of a module through powers of H together with its
 * AAD blocks, the zero padding and the length block, and compares with E_K(J0) ^ tag. No workgroup waits
 * on another and there are no atomics. */
#define PQG_AES_TILE_BYTES 16384    /* ciphertext bytes one wave decrypts; PQG_DISPATCH_AES_TILE_BYTES */
#define PQG_DECRYPT_GCM 0           /* pqg_decrypt_job.mode: AES_GCM_V1 page modules, and all of AES_GCM_CTR_V1's
                                       other modules */
#define PQG_DECRYPT_CTR 1           /* pqg_decrypt_job.mode: the page modules of AES_GCM_CTR_V1 */
#define PQG_MODULE_DATA_PAGE 2        /* ModuleCipherFactory.ModuleType.DataPage */
#define PQG_MODULE_DICTIONARY_PAGE 3  /* ModuleCipherFactory.ModuleType.DictionaryPage */

typedef struct pqg_decrypt_job {    /* sizeof == 40 */
  uint64_t src_offset;  /* first byte of the module (its length field) in d_src, any alignment */
  uint64_t dst_offset;  /* first byte of the plaintext in d_dst, any alignment */
  uint32_t src_size;    /* bytes of the whole module */
  uint32_t aad_offset;  /* the module's AAD in the host AAD blob (pqg_module_aad); ignored by CTR */
  uint32_t aad_length;
  int32_t mode;         /* PQG_DECRYPT_GCM / PQG_DECRYPT_CTR */
  int32_t key;          /* index into `keys` */
  uint32_t reserved;    /* 0 */
} pqg_decrypt_job;

typedef struct pqg_aes_key {        /* sizeof == 36 */
  uint8_t bytes[32];
  uint32_t size;        /* 16, 24 or 32 */
} pqg_aes_key;

/* d_dst[dst_offset, dst_offset + plaintext size) of job j <- the plaintext of the module at
 * d_src[src_offset, src_offset + src_size); d_status[j] (device, n_jobs) <- PQG_OK, or PQG_ERR_TAG when a
 * GCM module's tag does not verify (AesGcmDecryptor's TagVerificationException). The plaintext of a
 * failed job is undefined, but no store leaves [dst_offset, dst_offset + plaintext size) of any job.
 * Asynchronous on the ctx stream. `jobs`, `keys` and `aad` are HOST arrays (the sizes come from page
 * headers the host parsed, the keys from its key retrieval); they are copied before the call returns,
 * through growable pinned memory of the ctx, the keys as expanded schedules with H and its powers.
 * Jobs are independent: they may share keys and come in any order. d_src and d_dst are 4-byte aligned;
 * d_src is readable up to n_src rounded up to 4 and no load leaves that range.
 * PQG_ERR_INVALID_ARG, before any launch: NULL ctx; n_jobs < 0; NULL jobs, d_src, d_dst, d_status or keys
 * with n_jobs > 0; a job whose module leaves n_src, whose plaintext leaves n_dst or whose AAD leaves
 * aad_bytes; an unknown mode, a key index outside keys, non-zero reserved; a key whose size is not 16, 24
 * or 32 or whose bytes are all zero (AesCipher's constructor); more than 256 keys.
 * Cost of the keys: a call whose keys or tile size differ from the previous call's builds every key's material on
 * the host (the schedule and about tile / 16 + 200 products in GF(2^128): 1,200 at the default tile, well under a
 * millisecond per key), and every call copies 4 (tile / 16) + 9,500 bytes per key (26 KB at the default tile)
 * through pinned memory. The ctx keeps the last call's keys and material to compare and reuse; they are zeroed
 * when replaced and by pqg_ctx_destroy.
 * PQG_ERR_CORRUPT with st->page = the job: a module too short for a plaintext of 1 byte (the reference's
 * "Wrong input length"). PQG_ERR_UNSUPPORTED: more than 2^28 tiles in one call. st may be NULL.
 * n_jobs == 0 is valid and launches nothing. Launches: two (tiles, per-job fold), whatever n_jobs is. */
int pqg_decrypt_pages(pqg_ctx* ctx, const uint8_t* d_src, uint64_t n_src, uint8_t* d_dst, uint64_t n_dst,
                      const pqg_decrypt_job* jobs, int n_jobs, const pqg_aes_key* keys, int n_keys,
                      const uint8_t* aad, uint64_t aad_bytes, int32_t* d_status, pqg_status* st);
/* Synchronises the ctx stream and reads d_status back, like the codec *_sync calls: the first failing
 * job is st->page, and the message of a mismatch contains "GCM tag check failed". */
int pqg_decrypt_sync(pqg_ctx* ctx, const int32_t* d_status, int n_jobs, pqg_status* st);

/* A compressed V2 page is one module over its levels and its compressed data (ColumnChunkPageReadStore.java:228):
 * it is decrypted into the codec's source buffer, and its level bytes go on into the batch. pqg_copy_ranges copies
 * n byte ranges of one device buffer into another in one launch (one wave per range). d_ranges is a DEVICE array,
 * like the codec calls' job tables; a range that leaves n_src or n_dst, or has non-zero reserved, is skipped.
 * Ranges must not overlap in d_dst. Asynchronous on the ctx stream. PQG_ERR_INVALID_ARG: NULL ctx, n < 0, NULL
 * buffers or table with n > 0. n == 0 launches nothing. */
typedef struct pqg_copy_range {     /* sizeof == 24 */
  uint64_t src_offset;
  uint64_t dst_offset;
  uint32_t size;
  uint32_t reserved;  /* 0 */
} pqg_copy_range;
int pqg_copy_ranges(pqg_ctx* ctx, const uint8_t* d_src, uint64_t n_src, uint8_t* d_dst, uint64_t n_dst,
                    const pqg_copy_range* d_ranges, int n);

/* Host only. AesCipher.createModuleAAD (AesCipher.java:72-117) for page modules: out <- file_aad ||
 * module_type || row_group (2 bytes LE) || column (2 bytes LE) [|| page (2 bytes LE)], *out_len = its
 * length. module_type is PQG_MODULE_DATA_PAGE (with the page ordinal) or PQG_MODULE_DICTIONARY_PAGE
 * (without; `page` is ignored). PQG_ERR_INVALID_ARG: another module type, NULL out or out_len, NULL
 * file_aad with a length, a negative ordinal, an ordinal above Short.MAX_VALUE (32767), or a capacity
 * below the length (*out_len is still set). */
int pqg_module_aad(const uint8_t* file_aad, uint32_t file_aad_length, int module_type, int row_group, int column,
                   int page, uint8_t* out, uint32_t capacity, uint32_t* out_len);

/* Human-readable name of an error code. */
const char* pqg_error_name(int code);

#ifdef __cplusplus
}
#endif

#endif /* PQGPU_H */
