// pqgpu_api_hostpath.hip — the C ABI's host path: pqg_decode_host and pqg_decode_staged (batch bytes in host
// memory in, decoded columns in host memory out, through the context's pinned staging buffers),
// pqg_host_input, pqg_staged_column and pqg_copy_out.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "pqgpu_ctx.h"

using pqg::bin_out;
using pqg::out_width;

// ---- host copies of the host path (pinned staging <-> caller arrays): one thread moves ~10 GB/s,
// so large copies are spread over up to 8 threads, and the D2H of the outputs is issued in chunks
// whose copies out of pinned memory start as each chunk lands.
namespace {
struct HostCopy {
  uint8_t* dst;
  uint64_t src;  // offset in the pinned buffer
  uint64_t len;
};
// D2H piece: each is copied out by one thread as soon as it lands, so the copy of the last piece is the
// tail after the link (32 MiB pieces: d2h+copy 21-24 ms for 800 MB against 14 ms of link, r05u)
constexpr uint64_t HOST_CHUNK = 8ull << 20;
inline int host_threads(uint64_t bytes) {
  const unsigned hw = std::thread::hardware_concurrency();
  const uint64_t want = bytes / (8ull << 20) + 1;
  // (16 threads measured 38.4 vs 36.9 GB/s for 8 on an 800 MB output: host memory bound, profiles/r05/e2e)
  return (int)std::min<uint64_t>({want, 8ull, hw ? (uint64_t)hw : 1ull});
}
// the parts of `jobs` inside [lo, hi) of the pinned buffer `base`
void copy_range(const std::vector<HostCopy>& jobs, const uint8_t* base, uint64_t lo, uint64_t hi) {
  for (const HostCopy& j : jobs) {
    const uint64_t a = std::max(lo, j.src), b = std::min(hi, j.src + j.len);
    if (a < b) std::memcpy(j.dst + (a - j.src), base + a, b - a);
  }
}
void par_memcpy(void* dst, const void* src, uint64_t n) {
  const int t = host_threads(n);
  if (t <= 1) { std::memcpy(dst, src, n); return; }
  std::vector<std::thread> th;
  const uint64_t per = (n / (uint64_t)t + 4095) & ~4095ull;
  for (int k = 0; k < t; k++) {
    const uint64_t a = std::min(n, per * (uint64_t)k), b = std::min(n, a + per);
    if (a < b) th.emplace_back([=] { std::memcpy((uint8_t*)dst + a, (const uint8_t*)src + a, b - a); });
  }
  for (auto& x : th) x.join();
}
}  // namespace

extern "C" {

// The host path. h_bytes == nullptr: staged (pqg_decode_staged) — the bytes are already in ctx->pin_in,
// the outputs stay in ctx->pin_out and ctx->staged describes them; otherwise the caller's arrays.
static int host_path(pqg_ctx* ctx, const uint8_t* h_bytes, uint64_t n_bytes, pqg_column_desc* cols, int n_cols,
                     const pqg_page_desc* pages, int n_pages, uint32_t* h_page_value_counts, pqg_status* st) {
  if (st) { std::memset(st, 0, sizeof(*st)); st->page = -1; }
  const bool staged = h_bytes == nullptr;
  if (!ctx || n_cols < 0 || n_pages < 0 || (n_cols && !cols) || (n_pages && !pages)) return PQG_ERR_INVALID_ARG;
  if (staged && ctx->pin_in.cap < n_bytes + 1024) return PQG_ERR_INVALID_ARG;  // pqg_host_input first
  ctx->staged.clear();
  if (hipSetDevice(ctx->device) != hipSuccess) return PQG_ERR_HIP;
  hipStream_t s = ctx->stream;
  // PQG_HOST_TIMING=1: phase times of this call on stderr (diagnostics)
  static const bool timing = std::getenv("PQG_HOST_TIMING") != nullptr;
  auto t_last = std::chrono::steady_clock::now();
  auto phase = [&](const char* what) {
    if (!timing) return;
    const auto now = std::chrono::steady_clock::now();
    std::fprintf(stderr, "pqg_decode_host %-10s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(now - t_last).count());
    t_last = now;
  };
  const uint64_t pad = 1024;
  const size_t nc = (size_t)std::max(n_cols, 1);
  std::vector<uint64_t> slots(nc, 0), page_bytes(nc, 0);
  for (int p = 0; p < n_pages; p++)
    if (pages[p].column >= 0 && pages[p].column < n_cols) {
      slots[(size_t)pages[p].column] += pages[p].num_values;
      page_bytes[(size_t)pages[p].column] += pages[p].size;
    }
  // BYTE_ARRAY bytes on the device: PLAIN / DELTA_LENGTH values fit in their pages; dictionary
  // columns may expand, so the first attempt may come back short and is then re-run once at the
  // exact size the device counted
  std::vector<uint64_t> bin_cap(nc, 0);
  for (int i = 0; i < n_cols; i++)
    if (bin_out(cols[i]))
      bin_cap[(size_t)i] = page_bytes[(size_t)i] + (cols[i].dict_offset >= 0 ? 2 * (uint64_t)cols[i].dict_size : 0) + 64;
  if (ctx->host_bytes.ensure(n_bytes + pad) != hipSuccess || ctx->pin_in.ensure(n_bytes + pad) != hipSuccess ||
      ctx->host_counts.ensure(sizeof(uint32_t) * (size_t)std::max(n_pages, 1)) != hipSuccess) {
    set_status(st, PQG_ERR_HIP, -1, -1, "device buffers");
    return PQG_ERR_HIP;
  }
  // host -> pinned -> device (staged: the caller wrote the bytes into pin_in)
  if (!staged) par_memcpy(ctx->pin_in.p, h_bytes, n_bytes);
  std::memset((uint8_t*)ctx->pin_in.p + n_bytes, 0, pad);
  phase("stage-in");
  if (hipMemcpyAsync(ctx->host_bytes.p, ctx->pin_in.p, n_bytes + pad, hipMemcpyHostToDevice, s) != hipSuccess) return PQG_ERR_HIP;
  auto al = [](uint64_t x) { return (x + 255) & ~uint64_t(255); };
  std::vector<uint64_t> off_v(nc), off_d(nc), off_r(nc), off_b(nc);
  std::vector<pqg_column_desc> dcols(cols, cols + n_cols);
  // levels wanted: staged -> every column with a max level > 0; else where the caller gave an array
  std::vector<uint8_t> want_d(nc, 0), want_r(nc, 0);
  for (int i = 0; i < n_cols; i++) {
    want_d[(size_t)i] = cols[i].max_def > 0 && (staged || cols[i].def_levels);
    want_r[(size_t)i] = cols[i].max_rep > 0 && (staged || cols[i].rep_levels);
  }
  uint64_t total = 0;
  int rc = PQG_OK;
  pqg_status st2;
  for (int attempt = 0; attempt < 2; attempt++) {
    // device layout of outputs: per column values | def | rep | binary bytes, 256-B aligned
    total = 0;
    for (int i = 0; i < n_cols; i++) {
      const bool bin = bin_out(cols[i]);
      int w = out_width(cols[i]);
      if (w <= 0) w = 8;
      off_v[(size_t)i] = total;
      total = al(total + (slots[(size_t)i] + (bin ? 1 : 0)) * (uint64_t)w);
      off_d[(size_t)i] = total;
      if (want_d[(size_t)i]) total = al(total + slots[(size_t)i]);
      off_r[(size_t)i] = total;
      if (want_r[(size_t)i]) total = al(total + slots[(size_t)i]);
      off_b[(size_t)i] = total;
      if (bin) total = al(total + bin_cap[(size_t)i]);
    }
    if (ctx->host_out.ensure(total + 256) != hipSuccess || ctx->pin_out.ensure(total + 256) != hipSuccess) {
      set_status(st, PQG_ERR_HIP, -1, -1, "device buffers");
      return PQG_ERR_HIP;
    }
    uint8_t* dout = (uint8_t*)ctx->host_out.p;
    for (int i = 0; i < n_cols; i++) {
      const bool bin = bin_out(cols[i]);
      dcols[(size_t)i].values = dout + off_v[(size_t)i];
      dcols[(size_t)i].values_capacity = slots[(size_t)i] + (bin ? 1 : 0);
      dcols[(size_t)i].def_levels = want_d[(size_t)i] ? dout + off_d[(size_t)i] : nullptr;
      dcols[(size_t)i].rep_levels = want_r[(size_t)i] ? dout + off_r[(size_t)i] : nullptr;
      dcols[(size_t)i].levels_capacity = slots[(size_t)i];
      dcols[(size_t)i].binary_data = bin ? dout + off_b[(size_t)i] : nullptr;
      dcols[(size_t)i].binary_capacity = bin_cap[(size_t)i];
    }
    // the zero padding is part of the readable range: loads are range-checked per dword against it, and
    // a page ending at an unaligned offset close to n_bytes (raw file bytes) needs its last dword whole
    rc = pqg::decode_impl(ctx, (const uint8_t*)ctx->host_bytes.p, n_bytes + pad, n_bytes, dcols.data(), n_cols, pages,
                     n_pages, (uint32_t*)ctx->host_counts.p, st);
    if (rc) return rc;
    rc = pqg_sync(ctx, &st2);
    if (rc != PQG_ERR_INVALID_ARG || st2.page != -1 || !ctx->last || attempt == 1) break;
    // binary capacity: size every BYTE_ARRAY column to the byte count the device produced
    bool grew = false;
    for (int i = 0; i < n_cols; i++) {
      const uint64_t o = ctx->last->L.bin_total_off[(size_t)i];
      if (o == ~0ull) continue;
      uint64_t t = 0;
      if (hipMemcpy(&t, (uint8_t*)ctx->last->buf[B_BSCRATCH].p + o, sizeof(t), hipMemcpyDeviceToHost) != hipSuccess) return PQG_ERR_HIP;
      if (t > bin_cap[(size_t)i]) { bin_cap[(size_t)i] = t; grew = true; }
    }
    if (!grew) break;
  }
  for (int i = 0; i < n_cols; i++) cols[i].values_written = dcols[(size_t)i].values_written;
  if (rc && st) *st = st2;
  phase("h2d+decode");
  // device -> pinned -> host arrays (decoded values are valid up to the first error): the D2H goes
  // in HOST_CHUNK pieces, each followed by an event; worker threads copy the fixed-width values
  // and levels out of each piece as it lands
  uint8_t* dout = (uint8_t*)ctx->host_out.p;
  const uint8_t* po = (const uint8_t*)ctx->pin_out.p;
  std::vector<HostCopy> jobs;
  for (int i = 0; i < n_cols && !staged; i++) {
    const int w = out_width(cols[i]);
    const uint64_t n = std::min<uint64_t>(cols[i].values_written, cols[i].values_capacity);
    if (!bin_out(cols[i]) && cols[i].values && n)
      jobs.push_back({(uint8_t*)cols[i].values, off_v[(size_t)i], n * (uint64_t)w});
    if (cols[i].max_def > 0 && cols[i].def_levels)
      jobs.push_back({cols[i].def_levels, off_d[(size_t)i], std::min(slots[(size_t)i], cols[i].levels_capacity)});
    if (cols[i].max_rep > 0 && cols[i].rep_levels)
      jobs.push_back({cols[i].rep_levels, off_r[(size_t)i], std::min(slots[(size_t)i], cols[i].levels_capacity)});
  }
  const uint64_t n_chunks = (total + HOST_CHUNK - 1) / HOST_CHUNK;
  std::vector<hipEvent_t> ev((size_t)n_chunks, nullptr);
  bool ok = true;
  // odd chunks on a second stream (a second DMA queue), after the decode
  hipStream_t s2 = s;
  hipEvent_t dec_done = nullptr;
  if (n_chunks > 1) {
    if (ctx->copy_stream.get_or_create() && hipEventCreateWithFlags(&dec_done, hipEventDisableTiming) == hipSuccess &&
        hipEventRecord(dec_done, s) == hipSuccess && hipStreamWaitEvent(ctx->copy_stream.s, dec_done, 0) == hipSuccess)
      s2 = ctx->copy_stream.s;
  }
  // The copy threads start first and take each piece once it is queued and its event has completed:
  // hipMemcpyAsync into pinned memory measured blocking here (its events had all completed when the
  // threads started, r05w), so a queue-then-copy order ran the host copies after the whole D2H.
  std::vector<std::atomic<int>> queued((size_t)n_chunks);
  for (auto& q : queued) q.store(0, std::memory_order_relaxed);
  const int T = std::max(1, std::min<int>(host_threads(total), (int)n_chunks));
  std::vector<int> wok((size_t)T, 1);
  std::vector<std::thread> th;
  std::vector<double> t_dma((size_t)n_chunks, 0.0);  // (PQG_HOST_TIMING: when each piece was seen landed)
  const auto t_d0 = std::chrono::steady_clock::now();
  for (int t = 0; t < T && !staged; t++)
    th.emplace_back([&, t] {
      if (hipSetDevice(ctx->device) != hipSuccess) { wok[(size_t)t] = 0; return; }
      for (uint64_t k = (uint64_t)t; k < n_chunks; k += (uint64_t)T) {
        int q;
        while ((q = queued[(size_t)k].load(std::memory_order_acquire)) == 0) std::this_thread::yield();
        if (q < 0 || hipEventSynchronize(ev[(size_t)k]) != hipSuccess) { wok[(size_t)t] = 0; return; }
        if (timing) t_dma[(size_t)k] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_d0).count();
        copy_range(jobs, po, k * HOST_CHUNK, std::min(total, (k + 1) * HOST_CHUNK));
      }
    });
  for (uint64_t k = 0; k < n_chunks; k++) {
    const uint64_t a = k * HOST_CHUNK, len = std::min(HOST_CHUNK, total - a);
    hipStream_t sk = (k & 1) ? s2 : s;
    ok = ok && hipMemcpyAsync((uint8_t*)ctx->pin_out.p + a, dout + a, len, hipMemcpyDeviceToHost, sk) == hipSuccess &&
         hipEventCreateWithFlags(&ev[(size_t)k], hipEventDisableTiming) == hipSuccess &&
         hipEventRecord(ev[(size_t)k], sk) == hipSuccess;
    queued[(size_t)k].store(ok ? 1 : -1, std::memory_order_release);  // (-1: the threads stop)
  }
  std::vector<uint32_t> counts((size_t)std::max(n_pages, 1));
  if (ok && n_pages)
    ok = hipMemcpyAsync(counts.data(), ctx->host_counts.p, sizeof(uint32_t) * (size_t)n_pages, hipMemcpyDeviceToHost, s) == hipSuccess;
  for (auto& x : th) x.join();
  for (int v : wok) ok = ok && v;
  if (timing && n_chunks && !staged)
    std::fprintf(stderr, "pqg_decode_host   last D2H piece seen landed %.3f ms after the copy threads started (%d threads)\n",
                 *std::max_element(t_dma.begin(), t_dma.end()), T);
  if (s2 != s && hipStreamSynchronize(s2) != hipSuccess) ok = false;
  for (hipEvent_t e : ev)
    if (e) (void)hipEventDestroy(e);
  if (dec_done) (void)hipEventDestroy(dec_done);
  if (!ok || hipStreamSynchronize(s) != hipSuccess) return PQG_ERR_HIP;
  phase("d2h+copy");
  if (staged) {
    // outputs stay in pin_out: describe them (pqg_staged_column)
    ctx->staged.resize(nc);
    for (int i = 0; i < n_cols; i++) {
      pqg_staged_output& o = ctx->staged[(size_t)i];
      o.values = po + off_v[(size_t)i];
      o.def_levels = want_d[(size_t)i] ? po + off_d[(size_t)i] : nullptr;
      o.rep_levels = want_r[(size_t)i] ? po + off_r[(size_t)i] : nullptr;
      o.n_values = std::min<uint64_t>(cols[i].values_written, slots[(size_t)i]);
      o.n_slots = slots[(size_t)i];
      o.binary = nullptr;
      o.n_binary = 0;
      if (bin_out(cols[i])) {
        const uint64_t nb = (uint64_t)((const int64_t*)o.values)[o.n_values];
        if (nb > bin_cap[(size_t)i]) {  // the device's count did not fit even after the resize
          if (rc == PQG_OK) {
            rc = PQG_ERR_INVALID_ARG;
            set_status(st, rc, -1, (int64_t)nb, "binary capacity");
          }
        } else {
          o.binary = po + off_b[(size_t)i];
          o.n_binary = nb;
        }
      }
    }
    if (h_page_value_counts && n_pages) std::memcpy(h_page_value_counts, counts.data(), sizeof(uint32_t) * (size_t)n_pages);
    return rc;
  }
  for (int i = 0; i < n_cols; i++) {
    if (!bin_out(cols[i])) continue;
    // offsets[n + 1] and the bytes they span
    const uint64_t n = std::min<uint64_t>(cols[i].values_written, cols[i].values_capacity ? cols[i].values_capacity - 1 : 0);
    const int64_t* offs = (const int64_t*)(po + off_v[(size_t)i]);
    if (cols[i].values && cols[i].values_capacity) par_memcpy(cols[i].values, offs, (n + 1) * sizeof(int64_t));
    const uint64_t nb = (uint64_t)offs[n];
    if (nb > cols[i].binary_capacity) {
      if (rc == PQG_OK) {
        rc = PQG_ERR_INVALID_ARG;
        if (st) {
          st->code = rc;
          st->page = -1;
          st->value_index = (int64_t)nb;
          std::snprintf(st->message, sizeof(st->message), "binary capacity: column %d needs %llu bytes", i,
                        (unsigned long long)nb);
        }
      }
    } else if (cols[i].binary_data && nb) {
      par_memcpy(cols[i].binary_data, po + off_b[(size_t)i], nb);
    }
  }
  if (h_page_value_counts && n_pages) std::memcpy(h_page_value_counts, counts.data(), sizeof(uint32_t) * (size_t)n_pages);
  phase("binary");
  return rc;
}

int pqg_decode_host(pqg_ctx* ctx, const uint8_t* h_bytes, uint64_t n_bytes, pqg_column_desc* cols, int n_cols,
                    const pqg_page_desc* pages, int n_pages, uint32_t* h_page_value_counts, pqg_status* st) {
  static const uint8_t empty = 0;
  if (n_bytes && !h_bytes) {
    if (st) { std::memset(st, 0, sizeof(*st)); st->page = -1; }
    return PQG_ERR_INVALID_ARG;
  }
  return host_path(ctx, h_bytes ? h_bytes : &empty, n_bytes, cols, n_cols, pages, n_pages, h_page_value_counts, st);
}

int pqg_host_input(pqg_ctx* ctx, uint64_t n_bytes, uint8_t** buf) {
  if (!ctx || !buf) return PQG_ERR_INVALID_ARG;
  *buf = nullptr;
  if (hipSetDevice(ctx->device) != hipSuccess) return PQG_ERR_HIP;
  // the decode pads with 1,024 zero bytes after n_bytes (host_path's `pad`)
  if (ctx->pin_in.ensure(n_bytes + 1024) != hipSuccess) return PQG_ERR_HIP;
  ctx->staged.clear();
  *buf = (uint8_t*)ctx->pin_in.p;
  return PQG_OK;
}

int pqg_decode_staged(pqg_ctx* ctx, uint64_t n_bytes, pqg_column_desc* cols, int n_cols, const pqg_page_desc* pages,
                      int n_pages, uint32_t* h_page_value_counts, pqg_status* st) {
  return host_path(ctx, nullptr, n_bytes, cols, n_cols, pages, n_pages, h_page_value_counts, st);
}

int pqg_staged_column(pqg_ctx* ctx, int col, pqg_staged_output* out) {
  if (!ctx || !out || col < 0 || (size_t)col >= ctx->staged.size()) return PQG_ERR_INVALID_ARG;
  *out = ctx->staged[(size_t)col];
  return PQG_OK;
}

void pqg_copy_out(void* dst, const void* src, uint64_t n) {
  if (n && dst && src) par_memcpy(dst, src, n);
}

}  // extern "C"
