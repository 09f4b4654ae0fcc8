// pqgpu_api_host.cpp — the host-only logic of the C ABI (pqgpu_api_host.h). No HIP: tests/c/api_host_main.cpp
// runs these functions under AddressSanitizer + UndefinedBehaviorSanitizer without a device.
#include "pqgpu_api_host.h"

#include <algorithm>
#include <cstring>

namespace pqg {

// ---- ParquetReadRouter.read with the page's runs cached --------------------------------------------

bool router_hit(RouterCache& c, int w, const uint8_t* in, uint64_t need, uint64_t stream_left, int count,
                int32_t* out) {
  if (c.w != w || stream_left > c.tail_len || c.off.empty()) return false;
  const uint64_t pos = c.tail_len - stream_left;
  const auto it = std::lower_bound(c.off.begin(), c.off.end(), pos);
  if (it == c.off.end() || *it != pos) return false;
  const size_t r = (size_t)(it - c.off.begin());
  if (c.cnt[r] != (uint32_t)count) return false;
  if (need && std::memcmp(in, c.bytes.data() + pos, need) != 0) return false;
  std::memcpy(out, c.vals.data() + c.vo[r], (size_t)count * 4);
  c.hits++;
  return true;
}

int router_cache_lookup(RouterCache* c, int bit_width, const uint8_t* run, size_t stream_left, int count, int32_t* out,
                        int* hit) {
  if (!c || !hit || bit_width < 0 || bit_width > 32 || count < 0 || count % 8 != 0 || (count && !out))
    return PQG_ERR_INVALID_ARG;
  *hit = 0;
  const uint64_t need = (uint64_t)count * (uint64_t)bit_width / 8u;
  if (need > stream_left) return PQG_ERR_EOF;
  if (need && !run) return PQG_ERR_INVALID_ARG;
  if (count == 0) {
    *hit = 1;
    return PQG_OK;
  }
  *hit = router_hit(*c, bit_width, run, need, stream_left, count, out) ? 1 : 0;
  return PQG_OK;
}

void router_walk(RouterCache& c, int bit_width, const uint8_t* in, uint64_t stream_left, int count) {
  const uint64_t L = stream_left, need = (uint64_t)count * (uint64_t)bit_width / 8u;
  // Walk the hybrid stream after this run (RunLengthBitPackingHybridDecoder.readNext :80-109 header
  // forms; BytesUtils.readUnsignedVarInt :202-211) and list every bit-packed run whose bytes are in the
  // stream. The walk is a prediction of the caller's next reads: bytes past the hybrid stream (data the
  // caller reads otherwise) may parse as runs, which are decoded and never served; a header that cannot
  // be a run ends the walk. Runs the walk missed are served by a later miss.
  c.w = -1;
  c.off.clear();
  c.cnt.clear();
  c.vo.clear();
  c.off.push_back(0);
  c.cnt.push_back((uint32_t)count);
  c.vo.push_back(0);
  uint64_t total = (uint64_t)count, q = need;
  const uint32_t nb_rle = ((uint32_t)bit_width + 7u) / 8u;
  while (q < L && c.off.size() < ROUTER_MAX_RUNS) {
    uint32_t hdr = 0, sh = 0, b = 0;
    uint64_t k = q;
    bool ok = true;
    while (true) {
      if (k >= L || sh > 28) { ok = false; break; }
      b = in[k++];
      if (!(b & 0x80u)) break;
      hdr |= (b & 0x7Fu) << sh;
      sh += 7;
    }
    if (!ok) break;
    hdr |= b << sh;
    if (!(hdr & 1u)) {  // RLE run: count, then the value in ceil(w / 8) bytes
      q = k + nb_rle;
      continue;
    }
    const uint64_t groups = hdr >> 1, vals = groups * 8u, bytes = groups * (uint64_t)bit_width;
    if (vals > 0x7FFFFFF8u || k + bytes > L || total + vals > ROUTER_MAX_VALUES) break;
    if (vals) {
      c.off.push_back(k);
      c.cnt.push_back((uint32_t)vals);
      c.vo.push_back(total);
      total += vals;
    }
    q = k + bytes;
  }
  c.vals.resize(total);
  const uint64_t keep = c.off.size() > 1 ? c.off.back() + (uint64_t)c.cnt.back() * (uint64_t)bit_width / 8u : need;
  c.bytes.assign(in, in + keep);
  c.tail_len = L;
  c.misses++;
}

int router_runs_layout(int bit_width, const uint8_t* in, size_t in_len, const uint64_t* in_offsets, const uint32_t* counts,
                       int n_runs, RouterRunsImage* im) {
  // every run's slice first (SingleBufferInputStream.slice throws before any unpack)
  uint64_t n_bytes = 0, n_vals = 0;
  uint32_t max_count = 0;
  for (int r = 0; r < n_runs; r++) {
    if (counts[r] % 8u != 0) return PQG_ERR_INVALID_ARG;
    const uint64_t need = (uint64_t)counts[r] * (uint64_t)bit_width / 8u;
    if (in_offsets[r] > in_len || need > in_len - in_offsets[r]) return PQG_ERR_EOF;
    if (need && !in) return PQG_ERR_INVALID_ARG;
    n_bytes += (need + 15) & ~uint64_t(15);
    n_vals += counts[r];
    max_count = std::max(max_count, counts[r]);
  }
  im->n_bytes = n_bytes;
  im->n_vals = n_vals;
  im->max_count = max_count;
  // pinned image: [run bytes, each 16-B aligned][in_off u64 x n][out_off u64 x n][counts u32 x n]
  auto al = [](uint64_t x) { return (x + 255) & ~uint64_t(255); };
  im->o_in = al(n_bytes + 16);
  im->o_out = im->o_in + 8ull * (uint64_t)n_runs;
  im->o_cnt = im->o_out + 8ull * (uint64_t)n_runs;
  im->img = al(im->o_cnt + 4ull * (uint64_t)n_runs);
  return PQG_OK;
}

void router_runs_fill(const RouterRunsImage& im, int bit_width, const uint8_t* in, const uint64_t* in_offsets,
                      const uint32_t* counts, int n_runs, uint8_t* pin) {
  uint64_t* pin_in_off = (uint64_t*)(pin + im.o_in);
  uint64_t* pin_out_off = (uint64_t*)(pin + im.o_out);
  uint32_t* pin_cnt = (uint32_t*)(pin + im.o_cnt);
  uint64_t b = 0, v = 0;
  for (int r = 0; r < n_runs; r++) {
    const uint64_t need = (uint64_t)counts[r] * (uint64_t)bit_width / 8u;
    if (need) std::memcpy(pin + b, in + in_offsets[r], need);
    const uint64_t padded = (need + 15) & ~uint64_t(15);
    std::memset(pin + b + need, 0, padded - need);
    pin_in_off[r] = b;
    pin_out_off[r] = v;
    pin_cnt[r] = counts[r];
    b += padded;
    v += counts[r];
  }
  std::memset(pin + im.n_bytes, 0, im.o_in - im.n_bytes);
}

// ---- error resolution -------------------------------------------------------------------------------

void decode_error_words(std::vector<uint64_t>* errs, uint32_t epoch) {
  for (uint64_t& w : *errs)  // words of earlier launches are stale: no error in this one
    w = (w >> 48) == epoch ? (~w & ERR_KEY_MASK) : ~0ull;
}

// Resolve the first error of a launched plan in (page, value) order.
// Per page: init errors (rl init < dl init < data init) first; then value errors
// (values are decoded only for slots before a level error, so a value error is
// always earlier in the reference's read order); then level errors.
int resolve_page_errors(const PlanLayout& L, const std::vector<uint64_t>& errs, std::vector<pqg_page_error>* page_errs,
                        int* first_page, int64_t* index, const char** what) {
  // every page's own first error (pqg_page_errors), then the batch's first in page order
  page_errs->assign((size_t)L.n_pages, pqg_page_error{PQG_OK, PQG_PHASE_NONE, -1});
  if (L.host_errs.empty() && errs.empty()) return PQG_OK;
  std::vector<const HostErr*> herr((size_t)std::max(L.n_pages, 1), nullptr);
  for (const HostErr& h : L.host_errs)
    if (!herr[(size_t)h.page]) herr[(size_t)h.page] = &h;
  int first = -1;
  for (int p = 0; p < L.n_pages; p++) {
    pqg_page_error& pe = (*page_errs)[(size_t)p];
    const HostErr* h = herr[(size_t)p];
    // device-detected dictionary page errors (BYTE_ARRAY dictionary walk, pseudo page n_pages + column):
    // the ColumnReaderBase ctor reads the dictionary before the column's first page
    const int col = L.h_work[(size_t)p].column;
    const uint64_t d = (!errs.empty() && col >= 0 && col < L.n_cols && L.col_first_page[(size_t)col] == p)
                           ? errs[3 * (size_t)(L.n_pages + col)] : ~0ull;
    uint64_t init = errs.empty() ? ~0ull : errs[3 * (size_t)p];
    uint64_t lvl = errs.empty() ? ~0ull : errs[3 * (size_t)p + 1];
    uint64_t val = errs.empty() ? ~0ull : errs[3 * (size_t)p + 2];
    if (d != ~0ull) {
      pe = {(int32_t)(d & 0xFF), PQG_PHASE_DICTIONARY, -1};
    } else if (h && h->index == -1) {  // host-detected dictionary page error: before any page is read
      pe = {h->code, PQG_PHASE_DICTIONARY, -1};
    } else if (h || init != ~0ull) {   // init-phase errors: key = phase (0 rl, 1 dl, 2 data) << 8 | code
      const uint64_t hkey = h ? (((uint64_t)h->index << 8) | (uint64_t)h->code) : ~0ull;
      const uint64_t k = std::min(hkey, init);
      const int ph = (int)(k >> 8);
      pe = {(int32_t)(k & 0xFF), ph == 0 ? PQG_PHASE_RL_INIT : ph == 1 ? PQG_PHASE_DL_INIT : PQG_PHASE_DATA_INIT, -1};
    } else if (val != ~0ull) {
      // values are decoded only for slots before a level error: a value error comes first
      pe = {(int32_t)(val & 0xFF), PQG_PHASE_VALUE, (int64_t)(val >> 8)};
    } else if (lvl != ~0ull) {         // key = (slot << 1 | 0 rl / 1 dl) << 8 | code
      pe = {(int32_t)(lvl & 0xFF), ((lvl >> 8) & 1) ? PQG_PHASE_DL_READ : PQG_PHASE_RL_READ, (int64_t)(lvl >> 9)};
    }
    if (pe.code != PQG_OK && first < 0) first = p;
  }
  if (first < 0) return PQG_OK;
  const pqg_page_error& pe = (*page_errs)[(size_t)first];
  *first_page = first;
  switch (pe.phase) {
    case PQG_PHASE_DICTIONARY: *index = -1; *what = "dictionary page"; break;
    case PQG_PHASE_DATA_INIT: *index = 0; *what = "data init"; break;
    case PQG_PHASE_RL_INIT: case PQG_PHASE_DL_INIT: *index = 0; *what = "level init"; break;
    case PQG_PHASE_VALUE: *index = pe.index; *what = "value decode"; break;
    default: *index = pe.index; *what = "level decode"; break;
  }
  return pe.code;
}

// ---- dictionary pages -------------------------------------------------------------------------------

int dict_page_eof_code(const uint8_t* bytes, size_t size, uint32_t n_values) {
  uint64_t p = 0;
  for (uint32_t i = 0; i < n_values; i++) {
    if (p + 4 > size) return PQG_ERR_EOF;
    uint32_t len;
    std::memcpy(&len, bytes + p, 4);
    if ((int32_t)len < 0 || p + 4 + len > size) return PQG_ERR_CORRUPT;
    p += 4 + (uint64_t)len;
  }
  return PQG_ERR_EOF;
}

}  // namespace pqg
