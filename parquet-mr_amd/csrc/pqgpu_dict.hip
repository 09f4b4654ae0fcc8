// pqgpu_dict.hip — CDNA4 (gfx950) kernels of RLE_DICTIONARY / PLAIN_DICTIONARY pages: the walk of the
// hybrid id stream into run records (one 64-lane wave per page, the window helpers of pqgpu_hybrid.h),
// the expansion of the records into values or ids (one wave per output chunk), the walk -> expansion
// hand-off of the fused kernels, and their launchers. All integer / byte work: no MFMA.
// Semantics follow the reference reader value for value:
//   RunLengthBitPackingHybridDecoder.readInt/readNext (rle/…Decoder.java:61-109),
//   DictionaryValuesReader.initFromPage/read* (dictionary/DictionaryValuesReader.java:48-118).
#include <hip/hip_runtime.h>

#include <type_traits>

#include "pqgpu_device.h"
#include "pqgpu_hybrid.h"

namespace pqg {

// ---------------------------------------------------------------------------
// Dictionary pages (DictionaryValuesReader): W = 4 or 8 byte values.

template <int W>
__device__ __forceinline__ typename DictVal<W>::T load_dict(rsrc_t d, uint32_t id) {
  if constexpr (W == 8) return ld8_any(d, id * 8u);
  else return ld4_any(d, id * 4u);
}

constexpr uint32_t DICT_LDS_BYTES = 8192;   // dictionary staged in LDS per workgroup when it fits

// Per-wave LDS of the dictionary walk.
struct DictWaveLds {
  uint8_t seg[SEG_BYTES];  // page bytes [seg_lo, seg_lo + SEG_BYTES)
};

// ---------------------------------------------------------------------------
// Dictionary pages in two launches.
//
//   k_dict_runs    one wave per page: follows the run headers of the page's data
//                  section and writes one 8-byte record per run (first value index,
//                  payload: raw RLE id, or 0x80000000 | packed data position), plus,
//                  per output chunk, the record holding the chunk's first value.
//                  No dictionary access, no value stores: latency-bound LDS work.
//   k_dict_tiles   one wave per output chunk (dict_tiles_body: CH_TILES x 64 lanes x
//                  16 bytes) over all chunks of all pages, so the expansion is
//                  balanced regardless of how runs are spread over pages. All
//                  loads of a chunk (records, packed bytes, dictionary) come before
//                  its stores: on CDNA vmcnt counts stores, and a load issued after
//                  stores would wait for all of them.
// k_dict_fused runs both in one grid (the hand-off below); the two launches remain as split mode.

__device__ __forceinline__ uint32_t chunk_values(uint32_t E) { return CH_TILES * WAVE * E; }

// Walk -> expansion hand-off inside one launch (walkers and expansion waves on any CU / XCD).
//
// Every datum handed off — run records, chunk -> record entries, page status, page flag — is
// written and read ONLY with system-scope atomics (sst / sld: global_store / global_load with
// sc0 sc1). On gfx950 those bypass the non-coherent per-XCD L2 (stores write through, loads
// miss), so no cache write-back or invalidate is needed for them; what the hand-off needs is
// ORDER:
//   release (walker): the wave's record stores are complete before the status store, and the
//     status before the flag — s_waitcnt vmcnt(0) (stores count in vmcnt; the wait returns once
//     the write-through stores are acknowledged), plus a compiler barrier so no store is moved
//     across it;
//   acquire (expansion): the status / record loads are issued after the flag load returned the
//     epoch — the flag value feeds the loop's scalar branch, so its load has completed (vmcnt)
//     before any later load issues; a compiler barrier keeps those loads below the branch.
// This is the "{sc0 sc1 stores and loads both sides}" hand-off of MI355X_MICROARCH.md
// (inter-workgroup visibility: every handed-off byte stored sc1 and loaded sc1, every storing wave's
// vmcnt(0) before its flag, the polling wave loads only after its poll matched), which needs no
// agent-scope fence. The memory model's fences (buffer_wbl2 sc1 on release, buffer_inv sc1 on
// acquire) write back / invalidate the caches for the expansion's own traffic too; measured on C2
// (tried in round 2: a release store 1.30x the time, an acquire fence 2.45x, both 2.8x;
// profiles/r02/r02_b/ab).
// Variants measured and removed (git history, profiles/r02): an early partial hand-off after the
// walker's first window (C2 181.5 vs 172.6 us per launch, profiles/r02/early_ab: the extra wait on
// the walker's stores costs more than the early chunks gain); the mark-word chain of the window walk
// (the list walk dict_walk_ls replaced it); two chain steps per iteration through a
// successor-of-successor table, a branch-free 4-byte header parse, and the chain on the vector unit
// (ds_bpermute per run): all within +-1 % (profiles/r02/walk_ls/variants, vchain).
__device__ __forceinline__ void handoff_release() {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // a compiler barrier too (invisible to the waitcnt pass)
}
__device__ __forceinline__ void handoff_acquire() {
  __atomic_signal_fence(__ATOMIC_SEQ_CST);
}

// List walk: 256-byte windows whose chain and records are built without per-position masks.
//   chain    the successors of a lane's 4 positions are packed into one dword (byte b: window
//            offset of the successor of position 4 * lane + b, 0 = the chain stops there — a
//            successor is always past its header, so 0 is free), built by predecode_succ, which
//            parses nothing else; each step is one v_readlane, a byte extract and one v_writelane
//            that appends the position to a list VGPR (lane t = t-th header of the batch): one
//            loop branch per run, no per-position mark words.
//   records  lane t parses the header it holds from the staged bytes (walk_header: count and
//            payload, only at the positions the chain visited), a saturating DPP scan gives the
//            first values, and lane t stores record k + t: one store per run instead of a ballot
//            compaction over 256 positions.
// A window with more than 64 headers on its chain is taken in several batches.
// Semantics are those of readNext :80-109; the scalar path inside this function (slow_header_g) takes
// long varints, 0 / huge group counts and headers crossing the section end.
template <int W, bool SMALL = true>
__device__ __forceinline__ void dict_walk_ls(DictWaveLds& L, PreWin& win, uint32_t N, uint32_t sec_beg,
                                             uint32_t sec_end, int w, uint64_t* rec, uint32_t* chunk_run,
                                             uint32_t CH, uint32_t sh, int page, uint64_t* err, ErrCount err_count,
                                             uint32_t& n_rec, uint32_t& n_ok) {
  const uint32_t lane = lane_id();
  uint32_t pos = sec_beg + 1;  // RunLengthBitPackingHybridDecoder stream position
  uint32_t produced = 0, k = 0;
  int code = 0;
#ifdef PQG_DIAG
  uint64_t dg_pre = 0, dg_chain = 0, dg_emit = 0, dg_win = 0, dg_bat = 0;
  struct DgOut {
    uint64_t *a, *b, *c, *d, *e;
    uint32_t* k;
    int page;
    __device__ ~DgOut() {
      if (pqg_diag_wph && lane_id() == 0) {
        uint64_t* o = pqg_diag_wph + 8 * (uint64_t)page;
        o[0] = *a; o[1] = *b; o[2] = *c; o[3] = *d; o[4] = *e; o[5] = *k;
      }
    }
  } dg_out{&dg_pre, &dg_chain, &dg_emit, &dg_win, &dg_bat, &k, page};
#endif
  auto put_record = [&](uint32_t start, uint32_t end, uint32_t payload) {
    if (lane == 0) {
      sst(rec + k, (uint64_t)start | ((uint64_t)payload << 32));
      uint32_t j = start == 0 ? 0 : (start + sh + CH - 1) / CH;
      for (; j * CH < end + sh; j++) sst(chunk_run + j, k);
    }
    k++;
  };
  while (true) {
    pos = uni(pos);
    produced = uni(produced);
    k = uni(k);
    if (produced >= N) break;
    if (pos >= sec_end) { code = PQG_ERR_RLE_PAST_END; break; }  // readNext :81
    // A bit-packed run of at least 32 data bytes is taken on the scalar unit, without pre-decoding a
    // 256-byte window that holds at most eight headers (few-entry dictionaries of random ids — C4's
    // flag and mode columns, runs of 504 values at w = 1..3 — have one or two per window). The header
    // test reads one byte; an RLE header (C2's usual one) goes straight to the window.
    {
      if (!SMALL && !seg_has(win, pos & ~3u, 8u)) seg_fill(win, pos & ~15u);
      const uint32_t b0 = uni((seg32(win, pos & ~3u) >> ((pos & 3u) * 8u)) & 0xFFu);
      if (b0 & 1u) {
        uint32_t hl, m, nxs, vv;
        uint64_t cnt64;
        const int c2 = slow_header_g([&](uint32_t p) { return wbyte(win, p); }, pos, sec_end, w, hl, m, cnt64, vv, nxs);
        if (c2 == 0 && m && (cnt64 >> 3) * (uint32_t)w >= 32u) {
          const uint32_t left = N - produced;
          const uint32_t take = cnt64 < left ? (uint32_t)cnt64 : left;
          put_record(produced, produced + take, 0x80000000u | vv);
          produced += take;
          pos = nxs < sec_end ? nxs : sec_end;  // readFully of what is left
          continue;
        }
      }
    }
    const uint32_t B = pos & ~3u;
    DIAG_T(dg_t0);
#ifdef PQG_DIAG
    dg_win++;
#endif
    uint32_t js, slowm, inm;
    predecode_succ<SMALL>(win, B, w, sec_end, js, slowm, inm);
    DIAG_ADD(dg_pre, dg_t0);
    uint32_t q = uni(pos - B), nq = 0, t = 0, nxh = 0;
    while (true) {  // batches of at most 64 chain positions
      uint32_t lst = 0;
      t = 0;
      DIAG_T(dg_t1);
#ifdef PQG_DIAG
      dg_bat++;
#endif
      do {  // one step per run: append q to the list (lane t), read its successor
        lst = wrl(q, t, lst);
        nq = (rdl(js, q >> 2) >> ((q & 3u) << 3)) & 0xFFu;
        t++;
        if (nq == 0u) break;
        q = nq;  // (a full batch leaves with q == nq: the next batch's first position)
      } while (t < (uint32_t)WAVE);
      t = uni(t);
      nq = uni(nq);
      DIAG_ADD(dg_chain, dg_t1);
      DIAG_T(dg_t2);
      // the batch's last position q ends the chain here (nq == 0): a run only when it is a
      // fast-path header inside the section (otherwise the scalar path below takes it)
      const uint32_t ql = q >> 2, qb = q & 3u;
      const bool last_run = nq != 0u || (!((rdl(slowm, ql) >> qb) & 1u) && ((rdl(inm, ql) >> qb) & 1u));
      const uint32_t n_v = last_run ? t : t - 1u;
      const uint32_t cap = N - produced;
      // lane t < n_v parses the header it holds (the other lanes parse window offset 0 for nothing)
      bool pk;
      uint32_t c, payload;
      walk_header(win, lst, w, sec_end, pk, c, payload, nxh);
      if (!pk && c == 0) c = cap;  // Java: currentCount goes negative, the value repeats forever
      c = c < cap ? c : cap;
      if (lane >= n_v) c = 0;
      const uint32_t inc = wave_incl_scan_sat(c, cap);
      uint32_t st = __shfl_up(inc, 1);
      if (lane == 0) st = 0;
      const uint32_t total = uni(rdl(inc, WAVE - 1));
      // emitted: the runs that start before the cap (a prefix of the lanes)
      const bool em = c > 0u && st < cap;
      const uint32_t n_em = uni((uint32_t)__builtin_popcountll(__ballot(em)));
      if (em) {
        const uint32_t s_abs = produced + st;
        const uint32_t e_abs = produced + (st + c < cap ? st + c : cap);
        sst(rec + k + lane, (uint64_t)s_abs | ((uint64_t)payload << 32));
        uint32_t j = s_abs == 0 ? 0 : (s_abs + sh + CH - 1) / CH;
        for (; j * CH < e_abs + sh; j++) sst(chunk_run + j, k + lane);
      }
      k = uni(k + n_em);
      produced = uni(produced + total);
      DIAG_ADD(dg_emit, dg_t2);
      if (produced >= N || nq == 0u) break;
      q = nq;  // the chain goes on inside this window: next batch
    }
    if (produced >= N) break;
    // continue after the window's last chain position q
    const uint32_t ql = q >> 2, qb = q & 3u;
    const uint32_t q_slow = (rdl(slowm, ql) >> qb) & 1u;
    const uint32_t q_in = (rdl(inm, ql) >> qb) & 1u;
    if (!q_in) {
      pos = B + q;  // at or past the section end: RLE_PAST_END on the next iteration
    } else if (!q_slow) {
      pos = rdl(nxh, t - 1u);  // leaves the window: the last list lane parsed this header
    } else {
      // scalar re-decode of the header at q (readNext :80-109)
      pos = B + q;
      uint32_t hl, m, nxs, vv;
      uint64_t cnt64;
      code = SMALL ? slow_header_g([&](uint32_t p) { return uni((seg32(win, p & ~3u) >> ((p & 3u) * 8u)) & 0xFFu); },
                                   pos, sec_end, w, hl, m, cnt64, vv, nxs)
                   : slow_header_g([&](uint32_t p) { return wbyte(win, p); }, pos, sec_end, w, hl, m, cnt64, vv, nxs);
      if (code) break;
      if (m == 0 && nxs > sec_end) { code = PQG_ERR_EOF; break; }
      uint64_t cnt = cnt64;
      const uint32_t left = N - produced;
      if (m == 0 && cnt == 0) cnt = left;
      const uint32_t take = cnt < left ? (uint32_t)cnt : left;
      put_record(produced, produced + take, m ? (0x80000000u | vv) : (vv > 0x7FFFFFFFu ? 0x7FFFFFFFu : vv));
      produced += take;
      pos = m ? (nxs < sec_end ? nxs : sec_end) : nxs;
    }
  }
  if (code) {
    if (lane == 0) report(err, err_count, page, 2, produced, code);
    N = produced;
  }
  n_rec = k;
  n_ok = N;
}

// One wave per page (4 per workgroup): the run records of RLE_DICTIONARY / PLAIN_DICTIONARY
// pages (DictionaryValuesReader.initFromPage :48-64 + RunLengthBitPackingHybridDecoder.readNext
// :80-109). The page section is staged in LDS; a 256-byte window is pre-decoded in parallel
// (every lane finds the successor of a header at each of its 4 byte positions), the serial chain
// is one v_readlane per run, and the chain's headers are parsed one per lane (dict_walk_ls).
// One wave per page (4 per workgroup; `group` is the workgroup's index among the walkers).
template <int W>
__device__ __forceinline__ void dict_runs_body(const uint8_t* __restrict__ bytes, uint64_t n_bytes,
                                               const PageWork* __restrict__ work, const ColumnDev* __restrict__ cols,
                                               const int32_t* __restrict__ list, int n_list, uint64_t* rec,
                                               uint32_t* chunk_run, uint64_t* pstat, uint32_t* flags, uint32_t epoch,
                                               uint64_t* err, ErrCount err_count, uint8_t* lds, uint32_t group) {
  DictWaveLds& L = ((DictWaveLds*)lds)[wave_id()];
  const int i_page = (int)(group * WPB + wave_id());
  if (i_page >= n_list) return;
  const int page = list[i_page];
#ifdef PQG_DIAG
  const uint64_t rt_w0 = __builtin_amdgcn_s_memrealtime();
#endif
  const uint32_t lane = lane_id();
  const PageWork pw = work[page];
  const ColumnDev cd = cols[pw.column];
  uint32_t N = uni(pw.n_values);
  const uint32_t sec_beg = uni(pw.data_begin), sec_end = uni(pw.size);
  constexpr uint32_t E = 16u / W;
  const uint32_t CH = chunk_values(E);
  const uint32_t sh = (uint32_t)(pw.out_offset % (uint64_t)E);
  uint32_t n_rec = 0, n_ok = 0;
  (void)cd;
#ifdef PQG_DIAG
  uint64_t rt_w1 = 0, rt_w2 = 0;
#endif
  if (N > 0) {
    PreWin win;
    win.rs = make_rsrc(bytes + pw.base, n_bytes - pw.base);
    win.seg = L.seg;
    if (sec_beg >= sec_end) {
      // empty data section: every read throws "Attempt to read from empty page"
      if (lane == 0) report(err, err_count, page, 2 /*value*/, 0, PQG_ERR_EMPTY_PAGE);
    } else {
      seg_fill(win, sec_beg & ~15u);
      const uint32_t bw = wbyte(win, sec_beg);
#ifdef PQG_DIAG
      rt_w1 = __builtin_amdgcn_s_memrealtime() + (bw > 999u ? 1u : 0u);  // after the staging load
#endif
      if (bw > 32u) {  // RunLengthBitPackingHybridDecoder ctor :55 (thrown at initFromPage)
        if (lane == 0) report(err, err_count, page, 0 /*init*/, 2, PQG_ERR_BIT_WIDTH);
      } else {
        uint64_t* prec = rec + pw.rec_base;
        uint32_t* pcr = chunk_run + pw.chunk_base;
        // SMALL: the whole data section sits in the LDS segment: the walk has no global load
        if (sec_end - win.seg_lo + 264u <= SEG_BYTES)  // every window inside the segment
          dict_walk_ls<W>(L, win, N, sec_beg, sec_end, (int)bw, prec, pcr, CH, sh, page, err, err_count, n_rec, n_ok);
        else
          dict_walk_ls<W, false>(L, win, N, sec_beg, sec_end, (int)bw, prec, pcr, CH, sh, page, err, err_count, n_rec,
                                 n_ok);
      }
    }
  }
  // Publish (see handoff_release): every lane's record / chunk-entry stores, then lane 0's
  // status, then the flag.
#ifdef PQG_DIAG
  rt_w2 = __builtin_amdgcn_s_memrealtime() + (n_rec > 0xFFFFFFF0u ? 1u : 0u);
#endif
  wave_sync();
  handoff_release();
  if (lane == 0) {
    sst(pstat + page, (uint64_t)n_rec | ((uint64_t)n_ok << 32));
    handoff_release();
    sst(flags + page, epoch);
#ifdef PQG_DIAG
    if (pqg_diag_wrt) {
      pqg_diag_wrt[4 * page] = rt_w0;
      pqg_diag_wrt[4 * page + 1] = __builtin_amdgcn_s_memrealtime();
      pqg_diag_wrt[4 * page + 2] = rt_w1;
      pqg_diag_wrt[4 * page + 3] = rt_w2;
    }
#endif
  }
}

template <int W>
__global__ __launch_bounds__(64 * WPB) void k_dict_runs(const uint8_t* __restrict__ bytes, uint64_t n_bytes,
                                                        const PageWork* __restrict__ work,
                                                        const ColumnDev* __restrict__ cols,
                                                        const int32_t* __restrict__ list, int n_list, uint64_t* rec,
                                                        uint32_t* chunk_run, uint64_t* pstat, uint32_t* flags,
                                                        uint32_t epoch, uint64_t* err, ErrCount err_count) {
  __shared__ __attribute__((aligned(16))) DictWaveLds wl_all[WPB];
  dict_runs_body<W>(bytes, n_bytes, work, cols, list, n_list, rec, chunk_run, pstat, flags, epoch, err, err_count,
                    (uint8_t*)wl_all, blockIdx.x);
}

template <int W>
__device__ __forceinline__ typename DictVal<W>::T dict_get_g(bool in_lds, const typename DictVal<W>::T* dict_l,
                                                             rsrc_t drs, uint32_t id) {
  return in_lds ? dict_l[id] : load_dict<W>(drs, id);
}

// One wave per output chunk (CH_TILES tiles of 64 lanes x 16 bytes, i.e. full 1 KB lines).
//
//   load phase  run records of the chunk -> LDS run table {start, payload, value}, RLE
//               values gathered from the dictionary, page bytes of the bit-packed runs ->
//               LDS. Vector loads happen only here, before the wave's first store (on CDNA
//               vmcnt counts stores: a load after stores would wait for all of them).
//   tile sweep  every lane tracks the run holding its element: per tile it advances past
//               the run starts it crossed (usually none), reads the value (RLE) or unpacks
//               the id and gathers (packed), and the wave stores one full 1 KB tile.
constexpr int SPIN_SLEEP = 2;  // s_sleep units (64 cycles) between two polls of a page's ready flag
constexpr uint32_t XT_RUNS = 128;  // run table entries per wave
constexpr uint32_t XT_SEG = 2560;    // LDS bytes for the packed data of one round

constexpr uint32_t XT_LDS_BYTES = DICT_LDS_BYTES + WPB * (XT_RUNS * 16 + XT_SEG);
#ifdef PQG_FAULT_INJECT
// Fault-injection build (tests/build/libpqgpu_faultinject.so, tests/test_gpu_timeout.py only; never
// the product): walker workgroup 0 of every fused launch starts PQG_FAULT_INJECT ticks late, past a
// spin timeout shortened to 0.1 s, so the expansions waiting for its pages time out.
constexpr uint64_t SPIN_TIMEOUT_TICKS = 10000000ull;
#else
constexpr uint64_t SPIN_TIMEOUT_TICKS = 200000000ull;  // 2 s of s_memrealtime (100 MHz)
#endif

// FUSED: launched in the same grid as the walkers (after them in workgroup order, so every
// walker this wave waits for was dispatched first); the page's records are ready once its
// flag holds this launch's epoch.
// IDS: the expansion writes the dictionary ids themselves (u32, into ColumnDev::blen) instead
// of dictionary values: BYTE_ARRAY / FIXED_LEN_BYTE_ARRAY / INT96 dictionaries, whose values
// are materialized by later kernels (k_bin_dict_map + k_bin_copy, k_gather_fixed).
// DD_SUMS (dictionary-direct BYTE_ARRAY columns, ColumnDev::dict_direct; IDS, W = 4): the expansion
// stores the ids compactly (ColumnDev::blen as u8 ids for dict_direct 1, u16 for 2: a quarter / half of
// the u32 id traffic) and the chunk's value bytes, the sum of its ids' entry lengths, to dd[chunk].
// Slots of a page past a walk error (pstat's value count) are left to k_dd_str (empty values).
// DD_IDS (dictionary-direct columns whose dictionary is too large to stage, ColumnDev::dd_global): the
// compact u16 ids only; the chunk sums come from k_dd_gsums, which gathers the entry lengths from HBM.
constexpr int DD_NONE = 0, DD_SUMS = 1, DD_IDS = 2;

template <int W, bool FUSED, bool IDS = false, int DD = DD_NONE>
__device__ __forceinline__ void dict_tiles_body(const uint8_t* __restrict__ bytes, uint64_t n_bytes,
                                                const PageWork* __restrict__ work, const ColumnDev* __restrict__ cols,
                                                const uint64_t* rec, const uint32_t* chunk_run,
                                                const uint64_t* __restrict__ chunks, uint32_t n_chunks,
                                                const uint64_t* pstat, const uint32_t* flags, uint32_t epoch,
                                                uint64_t* err, ErrCount err_count, uint8_t* lds, uint32_t group,
                                                uint64_t* dd = nullptr) {
  typedef typename DictVal<W>::T T;
  static_assert(DD == DD_NONE || (IDS && W == 4), "dictionary-direct modes take the ids of a 4-byte expansion");
  constexpr uint32_t E = 16 / W;
  constexpr uint32_t TV = WAVE * E;  // values per tile
  constexpr uint32_t CH = CH_TILES * TV;
  uint8_t* dict_lds = lds;
  u32x4* tab = (u32x4*)(lds + DICT_LDS_BYTES) + wave_id() * XT_RUNS;
  uint8_t* xseg = lds + DICT_LDS_BYTES + WPB * XT_RUNS * 16 + wave_id() * XT_SEG;
  const uint32_t lane = lane_id();
  const uint32_t c = group * WPB + wave_id();
  // (a chunk list entry of page 0xFFFFFFFF is padding: the host aligns each dictionary-direct column's
  // chunks to whole workgroups, so a workgroup's waves share one dictionary)
  const int page = c < n_chunks ? (int)(uint32_t)chunks[c] : -1;
  // the workgroup's dictionary in LDS when its chunks share one that fits
  int* wg_col = (int*)dict_lds;
  if (lane == 0) wg_col[wave_id()] = page >= 0 ? work[page].column : -1;
  __syncthreads();
  int c0 = -1;
  bool same = true;
#pragma unroll
  for (int q = 0; q < WPB; q++) {
    const int cq = wg_col[q];
    if (cq >= 0) {
      if (c0 < 0) c0 = cq;
      else if (cq != c0) same = false;
    }
  }
  __syncthreads();
  bool dict_in_lds = false;
  uint32_t need = 0;
  // the dictionary is loaded into registers first and written to LDS after this wave's hand-off
  // loads, so its latency overlaps the first flag poll instead of preceding it
  u32x4 dreg[DICT_LDS_BYTES / (16u * 64u * WPB)] = {};
  if (!IDS && same && c0 >= 0) {
    const ColumnDev& cd0 = cols[c0];
    need = (uint32_t)((uint64_t)cd0.dict_n * W <= DICT_LDS_BYTES ? (uint64_t)cd0.dict_n * W : DICT_LDS_BYTES + 1u);
    dict_in_lds = need <= DICT_LDS_BYTES && need <= cd0.dict_bytes;
    if (dict_in_lds) {
      rsrc_t d0 = make_rsrc(bytes + cd0.dict_offset, cd0.dict_bytes);
#pragma unroll
      for (uint32_t r = 0; r < DICT_LDS_BYTES / (16u * 64u * WPB); r++) {
        const uint32_t o = 16u * threadIdx.x + r * 16u * 64u * WPB;
        if (o < need)  // any byte alignment; the piece at the buffer's end dword by dword
          dreg[r] = o + 16u <= cd0.dict_bytes
                        ? __builtin_amdgcn_raw_buffer_load_b128(d0, (int)o, 0, 0)
                        : u32x4{ld4_any(d0, o), ld4_any(d0, o + 4), ld4_any(d0, o + 8), ld4_any(d0, o + 12)};
      }
    }
  }
  const T* dict_l = (const T*)dict_lds;
  // ---- this wave's chunk, part 1: page facts and the hand-off (before the workgroup barrier)
  bool go = false;
  int cpage = -1;
  uint32_t j = 0, dict_n = 0, sec_end = 0, db = 0, N = 0, sh = 0, v_lo = 0, v_hi = 0, n_rec = 0, k = 0;
  uint32_t pre_lo = 0xFFFFFFFFu, pre_hi = 0;  // section bytes staged in xseg ahead of the records
  int w = 0;
  uint64_t pf0 = 0, pf1 = 0;  // records [0, 128) of the page (lane l: l and 64 + l)
  PageWork pw{};
  rsrc_t drs = make_rsrc(bytes, 0), prs = drs;
#ifdef PQG_DIAG
  const uint64_t rt_x0 = __builtin_amdgcn_s_memrealtime();
  uint64_t rt_x1 = 0;
  struct XStamp {
    uint64_t t0, *t1;
    uint32_t c;
    bool on;
    __device__ ~XStamp() {
      if (on && pqg_diag_xrt && lane_id() == 0) {
        uint32_t hw;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        pqg_diag_xrt[4 * (uint64_t)c] = t0;
        pqg_diag_xrt[4 * (uint64_t)c + 1] = *t1;
        pqg_diag_xrt[4 * (uint64_t)c + 2] = __builtin_amdgcn_s_memrealtime();
        pqg_diag_xrt[4 * (uint64_t)c + 3] = (uint64_t)hw;
      }
    }
  } xstamp{rt_x0, &rt_x1, c, c < n_chunks};
#endif
  uint32_t NF = 0;  // DD: the page's values (pstat's N stops at a walk error)
  if (page >= 0) {
    cpage = page;
    j = (uint32_t)(chunks[c] >> 32);
    // page / column facts and the page's bit width do not depend on the walk: loaded before the
    // hand-off, so the compiler barrier there does not serialize them behind the flag
    pw = work[cpage];
    const ColumnDev& cd = cols[pw.column];
    dict_n = uni(cd.dict_n);
    drs = make_rsrc(bytes + cd.dict_offset, cd.dict_bytes);
    prs = make_rsrc(bytes + pw.base, n_bytes - pw.base);
    sec_end = uni(pw.size);
    db = uni(pw.data_begin);
    w = (int)uni((ld32(prs, db & ~3u) >> ((db & 3u) * 8u)) & 0xFFu);
    // a data section that fits xseg is staged whole now (input bytes: no hand-off needed), so the
    // packed bytes of its runs need no load after the records
    if (sec_end > db && sec_end + 8u - (db & ~15u) <= XT_SEG) {
      pre_lo = db & ~15u;
      pre_hi = sec_end + 8u;
#pragma unroll
      for (uint32_t i = 0; i < XT_SEG; i += 16u * WAVE) {
        const uint32_t o = i + 16u * lane;
        if (o < pre_hi - pre_lo) *(u32x4*)(xseg + o) = __builtin_amdgcn_raw_buffer_load_b128(prs, (int)(pre_lo + o), 0, 0);
      }
      // bytes past the section read as 0 (the truncated final group, :96-99): zeroed once here, so
      // the tile sweep's unpack needs no per-value check
      if (lane < 8u) xseg[sec_end - pre_lo + lane] = 0;
    }
    uint64_t pst = 0;
    bool ok = true;
    if (FUSED) {
      // The flag is polled; once it holds this launch's epoch, handoff_acquire orders the status /
      // record / chunk-entry loads below after it (once per chunk, not per poll).
      uint64_t t_wait = 0;
      while (true) {
        if (uni(sld(flags + cpage)) == epoch) {
          handoff_acquire();
#ifdef PQG_DIAG
          rt_x1 = __builtin_amdgcn_s_memrealtime();
#endif
          break;
        }
        __builtin_amdgcn_s_sleep(SPIN_SLEEP);
        // wall-clock bound (s_memrealtime: constant 100 MHz): a walker that never publishes
        // (descheduled, starved) turns into PQG_ERR_TIMEOUT after SPIN_TIMEOUT_TICKS, not a hang
        const uint64_t now = __builtin_amdgcn_s_memrealtime();
        if (t_wait == 0) t_wait = now;
        else if (now - t_wait > SPIN_TIMEOUT_TICKS) {
          if (lane == 0) report(err, err_count, cpage, 2, 0, PQG_ERR_TIMEOUT);
          ok = false;
          break;
        }
      }
    }
    if (ok) {
      // the page status and the chunk's first run in one round trip
      pst = sld(pstat + cpage);
      k = sld(chunk_run + pw.chunk_base + j);
      {  // the page's first 2 x 64 run records in the same round trip
        pf0 = sld(rec + pw.rec_base + lane);
        pf1 = sld(rec + pw.rec_base + WAVE + lane);
      }
      pst = uni64(pst);
      k = uni(k);
      N = (uint32_t)(pst >> 32);  // values covered before a walk error
      NF = DD != DD_NONE ? uni(pw.n_values) : N;
      sh = (uint32_t)(pw.out_offset % (uint64_t)E);
      const uint32_t s_lo = j * CH > sh ? j * CH : sh;
      const uint32_t s_hi = (j + 1) * CH < NF + sh ? (j + 1) * CH : NF + sh;
      go = s_lo < s_hi;
      v_lo = s_lo - sh;
      v_hi = s_hi - sh;
      n_rec = (uint32_t)pst;
    }
  }
  if (dict_in_lds) {
#pragma unroll
    for (uint32_t r = 0; r < DICT_LDS_BYTES / (16u * 64u * WPB); r++) {
      const uint32_t o = 16u * threadIdx.x + r * 16u * 64u * WPB;
      if (o < need) *(u32x4*)(dict_lds + o) = dreg[r];
    }
  }
  // DD_SUMS: the entry lengths
  if constexpr (DD == DD_SUMS) {
    if (same && c0 >= 0) {
      const ColumnDev& cd0 = cols[c0];
      const uint32_t dn = uni(cd0.dict_n);
      dict_in_lds = dn <= DD_ENT_MAX && cd0.dict_bytes <= DD_DICT_MAX;
      if (dict_in_lds) {
        uint32_t* ent = (uint32_t*)dict_lds;
        for (uint32_t i = threadIdx.x; i < dn; i += 64u * WPB) ent[i] = cd0.dict_len[i];
      }
    }
  }
  __syncthreads();
  // ---- part 2: the chunk's run tables and tile sweeps
  auto one_chunk = [&]() {
    const int page = cpage;
    const ColumnDev& cd = cols[pw.column];
    T* const out_base = IDS ? (T*)cd.blen : (T*)cd.values;
    const bool own_dict = dict_in_lds && pw.column == c0;
    const uint64_t* prec = rec + pw.rec_base;
    T* const pag = out_base + (pw.out_offset - sh);  // slot 0 of the page
    const bool out16 = ((uintptr_t)out_base & 15u) == 0;
    const uint32_t wmask = w == 32 ? 0xFFFFFFFFu : (1u << w) - 1u;
    // the walked part of the chunk (DD: slots past a walk error follow as empty values)
    const uint32_t r_hi = DD != DD_NONE ? (v_hi < N ? v_hi : N) : v_hi;
    // DD_SUMS: the lane's byte sum, the column's compact ids (slot 0 of the page), their width
    uint32_t dd_acc = 0;
    const uint32_t* ent_l = (const uint32_t*)dict_lds;
    uint8_t* const idpag = (uint8_t*)cd.blen + (pw.out_offset - sh) * (uint64_t)cd.dict_direct;
    // DD: length of id's entry, 0 past the dictionary. Always from LDS: the plan gives a dictionary-direct
    // column whole workgroups and dictionaries that fit (a global load in the tile loop would make every
    // later wait a vmcnt(0), draining the stores)
    auto dd_entry = [&](uint32_t id) -> uint32_t { return id < dict_n ? ent_l[id] : 0u; };

    uint32_t b_lo = v_lo;
    while (v_lo < r_hi) {
      k = uni(k);
      b_lo = uni(b_lo);
      // ---- load phase: runs k .. k + n_tab - 1 into the table (entry n_tab: end sentinel)
      uint32_t n_tab = 0, b_hi = r_hi, px_lo = 0xFFFFFFFFu, px_hi = 0;
      for (uint32_t t0 = 0; t0 < XT_RUNS; t0 += WAVE) {
        const uint32_t r = k + t0 + lane;
        const bool has = r < n_rec && t0 + lane < XT_RUNS - 1;  // a run of this round
        // records the hand-off prefetched come from the lanes holding them
        const int src = (int)(r & (WAVE - 1u));
        const uint64_t a0 = ((uint64_t)(uint32_t)__shfl((int)(uint32_t)(pf0 >> 32), src) << 32) |
                            (uint32_t)__shfl((int)(uint32_t)pf0, src);
        const uint64_t a1 = ((uint64_t)(uint32_t)__shfl((int)(uint32_t)(pf1 >> 32), src) << 32) |
                            (uint32_t)__shfl((int)(uint32_t)pf1, src);
        const uint64_t rr = r >= n_rec ? 0 : (r < WAVE ? a0 : (r < 2u * WAVE ? a1 : sld(prec + r)));
        const uint32_t st = r < n_rec ? (uint32_t)rr : N;        // (past the runs: end sentinel)
        const uint32_t pl = (uint32_t)(rr >> 32);
        const uint32_t q63 = k + t0 + WAVE;
        const uint32_t nx63 = uni(q63 >= n_rec ? N
                                  : (q63 < 2u * WAVE
                                         ? rdl((uint32_t)(q63 < WAVE ? pf0 : pf1), q63 & (WAVE - 1u))
                                         : (uint32_t)sld(prec + q63)));
        const uint32_t en_n = __shfl_down(st, 1);
        const uint32_t en = lane == WAVE - 1 ? nx63 : en_n;  // end of this lane's run
        const bool live = has && st < r_hi;
        uint32_t vlo = 0, vhi = 0;
        if (live && !(pl & 0x80000000u)) {
          if (pl < dict_n) {
            if constexpr (IDS) {
              vlo = pl;
            } else {
              const uint64_t x = (uint64_t)(own_dict ? dict_l[pl] : load_dict<W>(drs, pl));
              vlo = (uint32_t)x;
              vhi = (uint32_t)(x >> 32);
            }
          }
        }
        tab[t0 + lane] = u32x4{st, pl, vlo, vhi};
        // packed bytes needed by this round: [first packed byte, last packed byte + 8)
        if (live && (pl & 0x80000000u)) {
          const uint32_t e_run = en;
          const uint32_t lo = (pl & 0x7FFFFFFFu) + (uint32_t)(((uint64_t)((st > b_lo ? st : b_lo) - st) * (uint32_t)w) >> 3);
          const uint32_t hi_v = (e_run < r_hi ? e_run : r_hi);
          const uint32_t hi = (pl & 0x7FFFFFFFu) + (uint32_t)(((uint64_t)(hi_v > st ? hi_v - st : 0) * (uint32_t)w + 7) >> 3) + 8u;
          px_lo = lo < px_lo ? lo : px_lo;
          px_hi = hi > px_hi ? hi : px_hi;
        }
        const uint64_t inb = __ballot(has && st < r_hi);
        n_tab += (uint32_t)__builtin_popcountll(inb);
        if (!(inb >> 63)) break;  // this batch ends the round
      }
      n_tab = uni(n_tab);
      // wave min / max of the packed byte range
  #pragma unroll
      for (int o = 32; o >= 1; o >>= 1) {
        const uint32_t a = __shfl_xor(px_lo, o), b = __shfl_xor(px_hi, o);
        px_lo = a < px_lo ? a : px_lo;
        px_hi = b > px_hi ? b : px_hi;
      }
      px_lo = uni(px_lo) & ~15u;
      px_hi = uni(px_hi);
      // round end: the start of the first run not in the table
      if (n_tab >= XT_RUNS - 1) {
        const u32x4 q = tab[XT_RUNS - 1];
        b_hi = uni(q.x) < r_hi ? uni(q.x) : r_hi;
      }
      bool x_lds = true;
      if (px_hi > px_lo && px_lo >= pre_lo && px_hi <= pre_hi) {
        px_lo = pre_lo;  // the section staged before the hand-off covers the round
      } else if (px_hi > px_lo) {
        pre_hi = 0;  // (xseg is overwritten)
        x_lds = px_hi - px_lo <= XT_SEG;
        if (x_lds) {
  #pragma unroll
          for (uint32_t i = 0; i < XT_SEG; i += 16u * WAVE) {
            const uint32_t o = i + 16u * lane;
            if (o < px_hi - px_lo) *(u32x4*)(xseg + o) = __builtin_amdgcn_raw_buffer_load_b128(prs, (int)(px_lo + o), 0, 0);
          }
          for (uint32_t o = (sec_end > px_lo ? sec_end - px_lo : 0u) + lane; o < px_hi - px_lo; o += WAVE) xseg[o] = 0;
        }
      }
      // DICT_ID: RLE runs of the round with an id past the dictionary (reported at the first
      // value of the run inside the chunk)
      for (uint32_t t0 = 0; t0 < n_tab; t0 += WAVE) {
        const u32x4 q = tab[t0 + lane];
        const uint32_t en = tab[t0 + lane + 1].x;
        if (t0 + lane < n_tab && !(q.y & 0x80000000u) && q.y >= dict_n && en > b_lo && q.x < b_hi)
          report(err, err_count, page, 2, q.x > b_lo ? q.x : b_lo, PQG_ERR_DICT_ID);
      }
      __builtin_amdgcn_s_waitcnt(0);  // load phase complete (the wave has not stored yet this round)

      // ---- tile sweep
      auto sweep = [&](auto fast_tag) {
        constexpr bool FAST = decltype(fast_tag)::value;
        auto value = [&](uint32_t ci, uint32_t i, const u32x4& q) -> T {
          if (!(q.y & 0x80000000u)) return (T)(((uint64_t)q.w << 32) | q.z);
          uint32_t id;
          if (FAST) {
            // staged bytes (zeroed past the section end), page value counts below 2^27: 32-bit bit
            // positions and one v_alignbit from the dword pair holding the id's first bit
            const uint32_t bit = (i - q.x) * (uint32_t)w;
            const uint32_t byte = (q.y & 0x7FFFFFFFu) + (bit >> 3);
            const uint32_t o = (byte & ~3u) - px_lo;
            id = __builtin_amdgcn_alignbit(*(const u32_alias*)(xseg + o + 4), *(const u32_alias*)(xseg + o),
                                           ((byte & 3u) << 3) + (bit & 7u)) & wmask;
          } else {
            const uint64_t bit = (uint64_t)(i - q.x) * (uint32_t)w;
            const uint32_t byte = (q.y & 0x7FFFFFFFu) + (uint32_t)(bit >> 3);
            const uint32_t a4 = byte & ~3u;
            uint64_t y = (uint64_t)ld32(prs, a4) | ((uint64_t)ld32(prs, a4 + 4) << 32);
            if (a4 + 8u > sec_end) {  // truncated final group: bytes past the section are 0 (:96-99)
              const int64_t keep = (int64_t)sec_end - (int64_t)a4;
              y = keep <= 0 ? 0 : (y & ((1ull << (8 * keep)) - 1ull));
            }
            y >>= (byte - a4) * 8u + (uint32_t)(bit & 7u);
            id = w == 0 ? 0u : (uint32_t)y & wmask;
          }
          if (id >= dict_n) {
            report(err, err_count, page, 2, i, PQG_ERR_DICT_ID);
            return 0;
          }
          if constexpr (IDS) return (T)id;
          else return FAST ? dict_l[id] : dict_get_g<W>(own_dict, dict_l, drs, id);
          (void)ci;
        };
        const uint32_t t_beg = (b_lo + sh) / TV, t_end = (b_hi + sh + TV - 1) / TV;  // page tiles
        // run of the lane's first element: binary search of the table
        uint32_t p0 = t_beg * TV + E * lane - sh;
        uint32_t pe = p0 < b_lo || p0 > 0x7FFFFFFFu ? b_lo : (p0 >= b_hi ? b_hi - 1 : p0);
        uint32_t ci = 0;
  #pragma unroll
        for (uint32_t step = XT_RUNS / 2; step >= 1; step >>= 1)
          if (ci + step < n_tab && tab[ci + step].x <= pe) ci += step;
        u32x4 cq = tab[ci];
        uint32_t ce = tab[ci + 1].x;
        const uint32_t lo_u = b_lo + sh, hi_u = b_hi + sh;  // the round's slot range
        for (uint32_t t = t_beg; t < t_end; t++) {
          t = uni(t);
          const uint32_t ts = t * TV;  // first slot of the tile
          p0 = ts + E * lane - sh;
          pe = p0 < b_lo || p0 > 0x7FFFFFFFu ? b_lo : (p0 >= b_hi ? b_hi - 1 : p0);
          while (pe >= ce) {  // crossed run starts (divergent, usually no lane)
            ci++;
            cq = tab[ci];
            ce = tab[ci + 1].x;
          }
          // elements outside [b_lo, b_hi) are not stored; they are evaluated at a clamped index
          T v[E];
          v[0] = value(ci, pe, cq);
  #pragma unroll
          for (uint32_t e = 1; e < E; e++) {
            const uint32_t x = p0 + e;  // value index of element e (wraps below 0)
            const uint32_t i = x < b_lo || x > 0x7FFFFFFFu ? b_lo : (x >= b_hi ? b_hi - 1 : x);
            if (i < ce) {
              v[e] = value(ci, i, cq);
            } else {  // the element starts a later run
              uint32_t cj = ci + 1;
              while (cj + 1 < n_tab && tab[cj + 1].x <= i) cj++;
              v[e] = value(cj, i, tab[cj]);
            }
          }
          if constexpr (DD != DD_NONE) {
            const bool whole = ts >= lo_u && ts + TV <= hi_u;
            uint8_t* ip = idpag + (uint64_t)(ts + E * lane) * cd.dict_direct;
            if (cd.dict_direct == 1u) {
              if (whole) gst((uint32_t*)ip, (v[0] & 0xFFu) | (v[1] & 0xFFu) << 8 | (v[2] & 0xFFu) << 16 | v[3] << 24);
            } else if (whole) {
              typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
              gst((u32x2*)ip, u32x2{(v[0] & 0xFFFFu) | v[1] << 16, (v[2] & 0xFFFFu) | v[3] << 16});
            }
  #pragma unroll
            for (uint32_t e = 0; e < E; e++) {
              const uint32_t sl = ts + E * lane + e;
              const bool in = sl >= lo_u && sl < hi_u;
              if constexpr (DD == DD_SUMS) dd_acc += in ? dd_entry((uint32_t)v[e]) : 0u;
              if (in && !whole) {
                if (cd.dict_direct == 1u) gst(ip + e, (uint8_t)v[e]);
                else gst((uint16_t*)ip + e, (uint16_t)v[e]);
              }
            }
          } else {
            T* tp = pag + ts + E * lane;
            if (out16 && ts >= lo_u && ts + TV <= hi_u) {
              if constexpr (W == 8) {
                typedef uint64_t v2 __attribute__((ext_vector_type(2)));
                gst_nt((v2*)tp, v2{v[0], v[1]});
              } else {
                gst_nt((u32x4*)tp, u32x4{v[0], v[1], v[2], v[3]});
              }
            } else {
  #pragma unroll
              for (uint32_t e = 0; e < E; e++)
                if (ts + E * lane + e >= lo_u && ts + E * lane + e < hi_u) gst(tp + e, v[e]);
            }
          }
        }
      };
      if ((IDS || own_dict) && x_lds && N < (1u << 27)) sweep(std::true_type{});
      else sweep(std::false_type{});
      if (b_hi >= r_hi) break;
      k += XT_RUNS - 1;
      b_lo = b_hi;
    }
    if constexpr (DD == DD_SUMS) {
      for (int o = 32; o >= 1; o >>= 1) dd_acc += __shfl_xor(dd_acc, o);
      if (lane == 0) gst(dd + c, (uint64_t)dd_acc);
    }
  };
  if (DD == DD_SUMS && go && !(dict_in_lds && pw.column == c0)) {
    // (never with the plan's layout: whole workgroups per column, dictionaries within DD_DICT_MAX / 2,048
    // entries)
    if (lane == 0) report(err, err_count, cpage, 2, v_lo, PQG_ERR_INVALID_ARG);
    go = false;
  }
  if (go) one_chunk();  // one chunk per wave
  else if (DD == DD_SUMS && page >= 0 && lane == 0) gst(dd + c, (uint64_t)0);
}

template <int W, bool IDS = false>
__global__ __launch_bounds__(64 * WPB) void k_dict_tiles(const uint8_t* __restrict__ bytes, uint64_t n_bytes,
                                                         const PageWork* __restrict__ work,
                                                         const ColumnDev* __restrict__ cols, const uint64_t* rec,
                                                         const uint32_t* chunk_run, const uint64_t* __restrict__ chunks,
                                                         uint32_t n_chunks, const uint64_t* pstat, uint64_t* err,
                                                         ErrCount err_count) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[XT_LDS_BYTES];
  dict_tiles_body<W, false, IDS>(bytes, n_bytes, work, cols, rec, chunk_run, chunks, n_chunks, pstat, nullptr, 0,
                                 err, err_count, lds, blockIdx.x);
}

// Walkers and tiles in one grid: workgroups [0, n_walk) walk pages, the rest expand chunks
// as soon as their page is published, so the expansion overlaps the walk.
template <int W, bool IDS = false>
__global__ __launch_bounds__(64 * WPB) void k_dict_fused(const uint8_t* __restrict__ bytes, uint64_t n_bytes,
                                                         const PageWork* __restrict__ work,
                                                         const ColumnDev* __restrict__ cols,
                                                         const int32_t* __restrict__ list, int n_list,
                                                         uint32_t n_walk, uint64_t* rec, uint32_t* chunk_run,
                                                         const uint64_t* __restrict__ chunks, uint32_t n_chunks,
                                                         uint64_t* pstat, uint32_t* flags, uint32_t epoch,
                                                         uint64_t* err, ErrCount err_count) {
  constexpr uint32_t LB = sizeof(DictWaveLds) * WPB > XT_LDS_BYTES ? sizeof(DictWaveLds) * WPB : XT_LDS_BYTES;
  __shared__ __attribute__((aligned(16))) uint8_t lds[LB];
  // workgroups [0, n_walk) walk (4 pages each), the rest expand (4 chunks each)
  if (blockIdx.x < n_walk) {
#ifdef PQG_FAULT_INJECT
    if (blockIdx.x == 0) {
      const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
      while (__builtin_amdgcn_s_memrealtime() - t0 < (uint64_t)PQG_FAULT_INJECT) __builtin_amdgcn_s_sleep(127);
    }
#endif
    dict_runs_body<W>(bytes, n_bytes, work, cols, list, n_list, rec, chunk_run, pstat, flags, epoch, err, err_count,
                      lds, blockIdx.x);
  } else {
    dict_tiles_body<W, true, IDS>(bytes, n_bytes, work, cols, rec, chunk_run, chunks, n_chunks, pstat, flags, epoch,
                                  err, err_count, lds, blockIdx.x - n_walk);
  }
}

// Dictionary-direct BYTE_ARRAY columns (ColumnDev::dict_direct: required, every data page
// dictionary-encoded, the dictionary page at most DD_DICT_MAX bytes): the ids are never stored.
//   k_dict_fused_dd  walkers + DD_SUMS expansion: per output chunk its compact ids and the bytes of its
//                    values (PlainBinaryDictionary entry lengths, PlainValuesDictionary.java:58-134)
//   k_dd_bases       per column: exclusive scan of its chunks' sums (chunks in page order) -> each chunk's
//                    first byte; the total -> bin_total and offsets[n_slots]
//   k_dd_str         per output chunk: the compact ids -> int64 offsets and the value bytes
// (DictionaryValuesReader.readBytes, DictionaryValuesReader.java:75-82, per value: the id's entry)
// DDM = DD_SUMS (dictionary staged in LDS) or DD_IDS (large dictionaries: ids only, k_dd_gsums sums)
template <int DDM>
__global__ __launch_bounds__(64 * WPB) void k_dict_fused_dd(const uint8_t* __restrict__ bytes, uint64_t n_bytes,
                                                            const PageWork* __restrict__ work,
                                                            const ColumnDev* __restrict__ cols,
                                                            const int32_t* __restrict__ list, int n_list,
                                                            uint32_t n_walk, uint64_t* rec, uint32_t* chunk_run,
                                                            const uint64_t* __restrict__ chunks, uint32_t n_chunks,
                                                            uint64_t* pstat, uint32_t* flags, uint32_t epoch,
                                                            uint64_t* err, ErrCount err_count, uint64_t* sums) {
  constexpr uint32_t LB = sizeof(DictWaveLds) * WPB > XT_LDS_BYTES ? sizeof(DictWaveLds) * WPB : XT_LDS_BYTES;
  __shared__ __attribute__((aligned(16))) uint8_t lds[LB];
  if (blockIdx.x < n_walk) {
#ifdef PQG_FAULT_INJECT
    if (blockIdx.x == 0) {
      const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
      while (__builtin_amdgcn_s_memrealtime() - t0 < (uint64_t)PQG_FAULT_INJECT) __builtin_amdgcn_s_sleep(127);
    }
#endif
    dict_runs_body<4>(bytes, n_bytes, work, cols, list, n_list, rec, chunk_run, pstat, flags, epoch, err, err_count,
                      lds, blockIdx.x);
  } else {
    dict_tiles_body<4, true, true, DDM>(bytes, n_bytes, work, cols, rec, chunk_run, chunks, n_chunks, pstat, flags,
                                        epoch, err, err_count, lds, blockIdx.x - n_walk, sums);
  }
}

// split mode (pqg_sync's re-run after a fused-kernel timeout): the DD_SUMS / DD_IDS expansion after the walk
template <int DDM>
__global__ __launch_bounds__(64 * WPB) void k_dict_tiles_dd(const uint8_t* __restrict__ bytes, uint64_t n_bytes,
                                                            const PageWork* __restrict__ work,
                                                            const ColumnDev* __restrict__ cols, const uint64_t* rec,
                                                            const uint32_t* chunk_run,
                                                            const uint64_t* __restrict__ chunks, uint32_t n_chunks,
                                                            const uint64_t* pstat, uint64_t* err, ErrCount err_count,
                                                            uint64_t* sums) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[XT_LDS_BYTES];
  dict_tiles_body<4, false, true, DDM>(bytes, n_bytes, work, cols, rec, chunk_run, chunks, n_chunks, pstat,
                                       nullptr, 0, err, err_count, lds, blockIdx.x, sums);
}

// ---------------------------------------------------------------------------
// Launchers (host side of this translation unit)

// The launch shape of every dictionary launcher. fused: walkers and expansion in one grid of n_walk +
// n_tile workgroups; split mode (pqg_sync's re-run after a fused-kernel timeout): walk, then expand when
// there are chunks, two launches. extra: the kernels' arguments after err_count (sums).
template <class KFused, class KRuns, class KTiles, class... Extra>
static hipError_t launch_walk_tiles(KFused k_fused, KRuns k_runs, KTiles k_tiles, bool fused, hipStream_t st,
                                    const uint8_t* bytes, uint64_t n_bytes, PageWork* work, const ColumnDev* cols,
                                    const int32_t* list, int n, uint64_t* rec, uint32_t* chunk_run,
                                    const uint64_t* chunks, uint32_t n_chunks, uint64_t* pstat, uint32_t* flags,
                                    uint32_t epoch, uint64_t* err, ErrCount err_count, Extra... extra) {
  if (n <= 0) return hipSuccess;
  const uint32_t n_walk = (uint32_t)(n + WPB - 1) / WPB, n_tile = (n_chunks + WPB - 1) / WPB;
  const dim3 blk(64 * WPB);
  if (fused) {
    hipLaunchKernelGGL(k_fused, dim3(n_walk + n_tile), blk, 0, st, bytes, n_bytes, work, cols, list, n, n_walk, rec,
                       chunk_run, chunks, n_chunks, pstat, flags, epoch, err, err_count, extra...);
  } else {
    hipLaunchKernelGGL(k_runs, dim3(n_walk), blk, 0, st, bytes, n_bytes, work, cols, list, n, rec, chunk_run, pstat,
                       flags, epoch, err, err_count);
    if (n_tile)
      hipLaunchKernelGGL(k_tiles, dim3(n_tile), blk, 0, st, bytes, n_bytes, work, cols, rec, chunk_run, chunks,
                         n_chunks, pstat, err, err_count, extra...);
  }
  return hipGetLastError();
}

#define PQG_DICT_ARGS \
  fused, st, bytes, n_bytes, work, cols, list, n, rec, chunk_run, chunks, n_chunks, pstat, flags, epoch, err, err_count

hipError_t launch_dict(int width, hipStream_t st, const uint8_t* bytes, uint64_t n_bytes, PageWork* work,
                       const ColumnDev* cols, const int32_t* list, int n, uint64_t* rec, uint32_t* chunk_run,
                       const uint64_t* chunks, uint32_t n_chunks, uint64_t* pstat, uint32_t* flags, uint32_t epoch,
                       bool fused, uint64_t* err, ErrCount err_count) {
  if (width == 8)
    return launch_walk_tiles(k_dict_fused<8, false>, k_dict_runs<8>, k_dict_tiles<8, false>, PQG_DICT_ARGS);
  return launch_walk_tiles(k_dict_fused<4, false>, k_dict_runs<4>, k_dict_tiles<4, false>, PQG_DICT_ARGS);
}

hipError_t launch_dict_ids(hipStream_t st, const uint8_t* bytes, uint64_t n_bytes, PageWork* work,
                           const ColumnDev* cols, const int32_t* list, int n, uint64_t* rec, uint32_t* chunk_run,
                           const uint64_t* chunks, uint32_t n_chunks, uint64_t* pstat, uint32_t* flags,
                           uint32_t epoch, bool fused, uint64_t* err, ErrCount err_count) {
  return launch_walk_tiles(k_dict_fused<4, true>, k_dict_runs<4>, k_dict_tiles<4, true>, PQG_DICT_ARGS);
}

hipError_t launch_dict_dd(hipStream_t st, const uint8_t* bytes, uint64_t n_bytes, PageWork* work,
                          const ColumnDev* cols, const int32_t* list, int n, uint64_t* rec, uint32_t* chunk_run,
                          const uint64_t* chunks, uint32_t n_chunks, uint64_t* pstat, uint32_t* flags,
                          uint32_t epoch, bool fused, uint64_t* err, ErrCount err_count, uint64_t* sums,
                          const int32_t* dd_cols, const int32_t* dd_start, int n_dd_cols, uint32_t dd_region,
                          bool global, hipEvent_t entries_ready) {
  if (n <= 0) return hipSuccess;
  const hipError_t e =
      global ? launch_walk_tiles(k_dict_fused_dd<DD_IDS>, k_dict_runs<4>, k_dict_tiles_dd<DD_IDS>, PQG_DICT_ARGS, sums)
             : launch_walk_tiles(k_dict_fused_dd<DD_SUMS>, k_dict_runs<4>, k_dict_tiles_dd<DD_SUMS>, PQG_DICT_ARGS, sums);
  if (e != hipSuccess) return e;
  return launch_dd_strings(st, bytes, n_bytes, work, cols, chunks, n_chunks, pstat, err, err_count, sums, dd_cols,
                           dd_start, n_dd_cols, dd_region, global, entries_ready);
}

#ifdef PQG_DIAG
}  // namespace pqg
// Diagnostic build only: the exported setters (this file's copies here, the other files' through pqg::diag_*).
extern "C" int pqg_diag_nostore_set(int v) {  // 0, or 3 when a copy failed
  return (hipMemcpyToSymbol(HIP_SYMBOL(pqg::pqg_diag_nostore), &v, sizeof(v)) == hipSuccess ? 0 : 3) |
         pqg::diag_nostore_dict_strings(v) | pqg::diag_nostore_plain(v) | pqg::diag_nostore_kernels(v);
}
extern "C" int pqg_diag_set(void*) { return 0; }  // (the buffer it set had no reader; kept for the tools that call it)
extern "C" int pqg_diag_wph_set(void* p) {
  return (hipMemcpyToSymbol(HIP_SYMBOL(pqg::pqg_diag_wph), &p, sizeof(p)) == hipSuccess ? 0 : 3) | pqg::diag_wph_kernels(p);
}
extern "C" int pqg_diag_rt_set(void* walk, void* chunk) {
  return hipMemcpyToSymbol(HIP_SYMBOL(pqg::pqg_diag_wrt), &walk, sizeof(walk)) == hipSuccess &&
                 hipMemcpyToSymbol(HIP_SYMBOL(pqg::pqg_diag_xrt), &chunk, sizeof(chunk)) == hipSuccess
             ? 0
             : 3;
}
namespace pqg {
#endif

}  // namespace pqg
