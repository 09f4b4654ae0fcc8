// api_host_main.cpp — the host-only logic of the C ABI (csrc/pqgpu_api_host.cpp) on its own, without a
// device: built with AddressSanitizer + UndefinedBehaviorSanitizer by tests/test_api_host.py. Every input
// is copied into a heap block of exactly its size, so that a one-byte overread aborts.
//   api_host_main cases    every case, with what it must give checked here
//   api_host_main digest   the same cases, one line each with everything the functions returned:
//                          tests/golden/api_host/digest.txt (recorded from the code these functions were
//                          moved out of, tools/record_api_host_digest.py)
//   api_host_main fuzz N   N seeded random mutations each of the router's streams, of error-word tables
//                          and of dictionary pages: the invariants below hold and nothing aborts
// The last line of every mode is "cases=<n>".
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../parquet-mr_amd/csrc/pqgpu_api_host.h"

using namespace pqg;

namespace {

bool g_print = false;
int g_cases = 0;

[[noreturn]] void fail(const std::string& where, const char* what) {
  std::fprintf(stderr, "FAILED %s: %s\n", where.c_str(), what);
  std::exit(1);
}
#define REQUIRE(cond) do { if (!(cond)) fail(where, #cond); } while (0)

// a heap block of exactly n bytes (n == 0: a valid pointer to nothing)
struct Block {
  uint8_t* p;
  size_t n;
  explicit Block(const std::vector<uint8_t>& v) : p(new uint8_t[v.size()]), n(v.size()) {
    if (n) std::memcpy(p, v.data(), n);
  }
  Block(const uint8_t* src, size_t len) : p(new uint8_t[len]), n(len) {
    if (n) std::memcpy(p, src, n);
  }
  Block(const Block&) = delete;
  Block& operator=(const Block&) = delete;
  ~Block() { delete[] p; }
};

struct Rng {  // splitmix64
  uint64_t s;
  uint64_t next() {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
  uint32_t below(uint32_t n) { return (uint32_t)(next() % n); }
};

uint64_t fnv(const void* p, size_t n, uint64_t h = 0xCBF29CE484222325ull) {
  const uint8_t* b = (const uint8_t*)p;
  for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 0x100000001B3ull;
  return h;
}
template <class T>
uint64_t fnv_vec(const std::vector<T>& v) { return fnv(v.data(), sizeof(T) * v.size()); }

// ---- a small hybrid (RLE / bit-packed) encoder ----------------------------------------------------------

struct Stream {
  std::vector<uint8_t> b;
  Rng rng{1};
  void varint(uint64_t v) {
    while (v >= 0x80) { b.push_back((uint8_t)(v | 0x80)); v >>= 7; }
    b.push_back((uint8_t)v);
  }
  void data(uint64_t n) { for (uint64_t i = 0; i < n; i++) b.push_back((uint8_t)rng.next()); }
  // the run the caller asks for: its data only (the caller has read its header)
  void first(int count, int w) { data((uint64_t)count * (uint64_t)w / 8u); }
  void rle(uint32_t count, int w) { varint((uint64_t)count << 1); data(((uint32_t)w + 7u) / 8u); }
  void packed(uint32_t groups, int w) { varint(((uint64_t)groups << 1) | 1u); data((uint64_t)groups * (uint64_t)w); }
  void header_only(uint64_t hdr) { varint(hdr); }
};

// what the device would unpack: a value that names its position
int32_t fake_value(uint64_t i) { return (int32_t)(uint32_t)(i * 2654435761u + 12345u); }

// router_walk on an exactly-sized copy of the stream, then the invariants of what it listed
void walk(const std::string& where, RouterCache& c, int w, const std::vector<uint8_t>& bytes, int count) {
  Block in(bytes);
  const uint64_t misses = c.misses;
  router_walk(c, w, in.p, in.n, count);
  REQUIRE(c.w == -1 && c.misses == misses + 1 && c.tail_len == in.n);
  REQUIRE(!c.off.empty() && c.off.size() == c.cnt.size() && c.off.size() == c.vo.size() && c.off.size() <= ROUTER_MAX_RUNS);
  REQUIRE(c.off[0] == 0 && c.cnt[0] == (uint32_t)count && c.vo[0] == 0);
  uint64_t total = 0;
  for (size_t r = 0; r < c.off.size(); r++) {
    REQUIRE(r == 0 || c.off[r] > c.off[r - 1] || (w == 0 && c.off[r] >= c.off[r - 1]));
    REQUIRE(c.cnt[r] % 8u == 0 && (r == 0 || c.cnt[r] > 0));
    REQUIRE(c.off[r] + (uint64_t)c.cnt[r] * (uint64_t)w / 8u <= in.n);
    REQUIRE(c.vo[r] == total);
    total += c.cnt[r];
  }
  REQUIRE(c.vals.size() == total && (total <= ROUTER_MAX_VALUES || c.off.size() == 1));
  REQUIRE(c.bytes.size() <= in.n && (c.bytes.empty() || std::memcmp(c.bytes.data(), in.p, c.bytes.size()) == 0));
  REQUIRE(c.bytes.size() == c.off.back() + (uint64_t)c.cnt.back() * (uint64_t)w / 8u);
}

// the caller's second half of a miss: the runs unpacked into vals, the cache valid for width w
void fill(RouterCache& c, int w) {
  for (size_t i = 0; i < c.vals.size(); i++) c.vals[i] = fake_value(i);
  c.w = w;
}

void print_walk(const char* name, const RouterCache& c, int w, uint64_t left, int count) {
  g_cases++;
  if (!g_print) return;
  std::printf("walk %s w=%d left=%llu count=%d runs=%zu total=%zu keep=%zu tail=%llu misses=%llu off=%016llx cnt=%016llx vo=%016llx bytes=%016llx first=[",
              name, w, (unsigned long long)left, count, c.off.size(), c.vals.size(), c.bytes.size(), (unsigned long long)c.tail_len,
              (unsigned long long)c.misses, (unsigned long long)fnv_vec(c.off), (unsigned long long)fnv_vec(c.cnt),
              (unsigned long long)fnv_vec(c.vo), (unsigned long long)fnv_vec(c.bytes));
  for (size_t r = 0; r < c.off.size() && r < 8; r++)
    std::printf("%s%llu:%u:%llu", r ? " " : "", (unsigned long long)c.off[r], c.cnt[r], (unsigned long long)c.vo[r]);
  std::printf("]\n");
}

// router_cache_lookup with the run in a block of exactly the bytes it may read
struct Lookup { int rc, hit; std::vector<int32_t> out; };
Lookup lookup(RouterCache* c, int w, const uint8_t* run, size_t avail, size_t stream_left, int count) {
  const uint64_t need = count > 0 && w >= 0 && w <= 32 ? (uint64_t)count * (uint64_t)w / 8u : 0;
  Block in(run, (size_t)std::min<uint64_t>(need, avail));
  Lookup l;
  l.out.assign((size_t)std::max(count, 0), -1);
  l.hit = -7;
  l.rc = router_cache_lookup(c, w, run ? in.p : nullptr, stream_left, count, l.out.data(), &l.hit);
  return l;
}

void print_lookup(const char* name, const Lookup& l, const RouterCache& c) {
  g_cases++;
  if (g_print)
    std::printf("lookup %s rc=%d hit=%d out=%016llx hits=%llu\n", name, l.rc, l.hit, (unsigned long long)fnv_vec(l.out),
                (unsigned long long)c.hits);
}

void router_cases() {
  const int widths[] = {0, 1, 7, 8, 9, 31, 32};
  // RLE and bit-packed runs mixed, a bit-packed run of 0 groups, the last run ending at the stream's end;
  // then the same stream one byte short, which loses that run
  for (int w : widths) {
    Stream s;
    s.rng.s = 100 + (uint64_t)w;
    s.first(8, w);
    s.rle(5, w);
    s.packed(2, w);
    s.rle(300, w);
    s.packed(1, w);
    s.packed(0, w);
    s.rle(1, w);
    s.packed(3, w);
    const std::string where = "mixed_w" + std::to_string(w);
    RouterCache c;
    walk(where, c, w, s.b, 8);
    REQUIRE(c.off.size() == 4 && c.cnt[1] == 16 && c.cnt[2] == 8 && c.cnt[3] == 24 && c.bytes.size() == s.b.size());
    print_walk(where.c_str(), c, w, s.b.size(), 8);
    if (w > 0) {
      std::vector<uint8_t> cut(s.b.begin(), s.b.end() - 1);
      RouterCache c2;
      walk(where + "_short", c2, w, cut, 8);
      REQUIRE(c2.off.size() == 3);
      print_walk((where + "_short").c_str(), c2, w, cut.size(), 8);
    }
    // ---- the cache over this walk
    fill(c, w);
    Block base(s.b);
    for (size_t r = 0; r < c.off.size(); r++) {  // a hit on every run
      const Lookup l = lookup(&c, w, base.p + c.off[r], base.n - c.off[r], base.n - c.off[r], (int)c.cnt[r]);
      REQUIRE(l.rc == PQG_OK && l.hit == 1);
      for (uint32_t i = 0; i < c.cnt[r]; i++) REQUIRE(l.out[i] == fake_value(c.vo[r] + i));
      print_lookup((where + "_hit" + std::to_string(r)).c_str(), l, c);
    }
    const size_t r = 1;
    const uint8_t* run = base.p + c.off[r];
    const size_t left = base.n - c.off[r];
    const uint64_t hits = c.hits;
    Lookup l = lookup(&c, w == 32 ? 31 : w + 1, run, left, left, (int)c.cnt[r]);
    REQUIRE(l.hit == 0);
    print_lookup((where + "_miss_width").c_str(), l, c);
    l = lookup(&c, w, run, left, left, (int)c.cnt[r] - 8);
    REQUIRE(l.rc == PQG_OK && l.hit == 0);
    print_lookup((where + "_miss_count").c_str(), l, c);
    if (w > 0) {
      l = lookup(&c, w, run + 1, left - 1, left - 1, (int)c.cnt[r]);
      REQUIRE(l.rc == PQG_OK && l.hit == 0);
      print_lookup((where + "_miss_position").c_str(), l, c);
      std::vector<uint8_t> changed(run, run + (uint64_t)c.cnt[r] * (uint64_t)w / 8u);
      changed.back() ^= 0x10;
      l = lookup(&c, w, changed.data(), changed.size(), left, (int)c.cnt[r]);
      REQUIRE(l.rc == PQG_OK && l.hit == 0);
      print_lookup((where + "_miss_byte").c_str(), l, c);
    }
    l = lookup(&c, w, run, left, left + base.n, (int)c.cnt[r]);  // a position before the walked tail
    REQUIRE(l.rc == PQG_OK && l.hit == 0);
    print_lookup((where + "_miss_before_tail").c_str(), l, c);
    REQUIRE(c.hits == hits);
    l = lookup(&c, w, run, left, left, 0);
    REQUIRE(l.rc == PQG_OK && l.hit == 1 && c.hits == hits);
    print_lookup((where + "_count0").c_str(), l, c);
    l = lookup(&c, w, nullptr, 0, 0, 0);
    REQUIRE(l.rc == PQG_OK && l.hit == 1);
    print_lookup((where + "_count0_null").c_str(), l, c);
  }
  {  // the argument checks of the lookup
    const std::string where = "lookup_args";
    RouterCache c;
    const uint8_t some[16] = {};
    Lookup l = lookup(nullptr, 8, some, 16, 16, 8);
    REQUIRE(l.rc == PQG_ERR_INVALID_ARG);
    print_lookup("args_no_cache", l, c);
    l = lookup(&c, 33, some, 16, 16, 8);
    REQUIRE(l.rc == PQG_ERR_INVALID_ARG);
    print_lookup("args_width_33", l, c);
    l = lookup(&c, -1, some, 16, 16, 8);
    REQUIRE(l.rc == PQG_ERR_INVALID_ARG);
    print_lookup("args_width_neg", l, c);
    l = lookup(&c, 8, some, 16, 16, 4);
    REQUIRE(l.rc == PQG_ERR_INVALID_ARG);
    print_lookup("args_count_4", l, c);
    l = lookup(&c, 8, some, 16, 16, -8);
    REQUIRE(l.rc == PQG_ERR_INVALID_ARG);
    print_lookup("args_count_neg", l, c);
    l = lookup(&c, 8, some, 16, 15, 16);
    REQUIRE(l.rc == PQG_ERR_EOF && l.hit == 0);
    print_lookup("args_eof", l, c);
    l = lookup(&c, 8, nullptr, 0, 16, 8);
    REQUIRE(l.rc == PQG_ERR_INVALID_ARG);
    print_lookup("args_null_run", l, c);
    l = lookup(&c, 8, some, 16, 16, 8);  // nothing walked yet
    REQUIRE(l.rc == PQG_OK && l.hit == 0);
    print_lookup("args_empty_cache", l, c);
    int32_t out[8];
    REQUIRE(router_cache_lookup(&c, 8, some, 16, 8, out, nullptr) == PQG_ERR_INVALID_ARG);
    int hit = 0;
    REQUIRE(router_cache_lookup(&c, 8, some, 16, 8, nullptr, &hit) == PQG_ERR_INVALID_ARG);
  }
  // ---- headers and limits
  struct Lim { const char* name; int w; int count; size_t runs; Stream s; };
  std::vector<Lim> lims;
  auto add = [&](const char* name, int w, int count, size_t runs) -> Stream& {
    lims.push_back(Lim{name, w, count, runs, Stream()});
    lims.back().s.rng.s = 7000 + lims.size();
    lims.back().s.first(count, w);
    return lims.back().s;
  };
  {
    Stream& s = add("header_cut", 8, 8, 2);  // a varint header cut by the end of the buffer
    s.packed(1, 8);
    s.b.push_back(0x83);
  }
  {
    Stream& s = add("header_cut_3_bytes", 8, 8, 1);
    s.b.push_back(0x83); s.b.push_back(0x80); s.b.push_back(0x80);
  }
  {
    Stream& s = add("varint_5_bytes", 0, 8, 1);  // shift 28 in the fifth byte: a header, of a run far too long
    s.header_only(0xF0000001ull);
    s.packed(1, 0);
  }
  {
    Stream& s = add("varint_6_bytes", 0, 8, 1);  // five continuation bytes: the shift passes 28
    for (int i = 0; i < 5; i++) s.b.push_back(0x81);
    s.b.push_back(0x00);
    s.packed(1, 0);
  }
  {
    Stream& s = add("values_7ffffff8_w0", 0, 8, 1);  // exactly 0x7FFFFFF8 values: past ROUTER_MAX_VALUES
    s.packed(0x0FFFFFFFu, 0);
    s.packed(1, 0);
  }
  {
    Stream& s = add("values_80000000_w0", 0, 8, 1);  // 0x80000000 values: past 0x7FFFFFF8
    s.header_only((0x10000000ull << 1) | 1u);
    s.packed(1, 0);
  }
  {
    Stream& s = add("values_7ffffff8_w1", 1, 8, 1);  // ... whose bytes are not in the stream
    s.header_only((0x0FFFFFFFull << 1) | 1u);
    s.packed(1, 1);
  }
  {
    Stream& s = add("values_max_exact", 0, 1 << 21, 3);  // 2^21 + 2^21 - 8 + 8 = ROUTER_MAX_VALUES, then one group more
    s.packed((1u << 18) - 1, 0);
    s.packed(1, 0);
    s.packed(1, 0);
  }
  {
    Stream& s = add("values_max_crossed", 0, 8, 2);  // 8 + 2^21 + 2^21 values
    s.packed(1u << 18, 0);
    s.packed(1u << 18, 0);
    s.packed(1, 0);
  }
  {
    Stream& s = add("runs_max", 0, 8, ROUTER_MAX_RUNS);  // ROUTER_MAX_RUNS reached with runs left in the stream
    for (int i = 0; i < 70000; i++) s.packed(1, 0);
  }
  {
    Stream& s = add("rle_value_cut", 32, 8, 1);  // an RLE run whose value bytes pass the end
    s.varint(6);
    s.b.push_back(0x01);
  }
  add("only_the_run", 9, 16, 1);
  for (Lim& l : lims) {
    const std::string where = l.name;
    RouterCache c;
    walk(where, c, l.w, l.s.b, l.count);
    REQUIRE(c.off.size() == l.runs);
    print_walk(l.name, c, l.w, l.s.b.size(), l.count);
  }
  {  // a second walk on the same cache replaces the first
    const std::string where = "rewalk";
    Stream a, b;
    a.first(8, 8); a.packed(2, 8); a.packed(1, 8);
    b.first(16, 4); b.packed(1, 4);
    RouterCache c;
    walk(where, c, 8, a.b, 8);
    fill(c, 8);
    walk(where, c, 4, b.b, 16);
    REQUIRE(c.off.size() == 2 && c.misses == 2);
    print_walk("rewalk", c, 4, b.b.size(), 16);
    Block base(a.b);
    const Lookup l = lookup(&c, 8, base.p, base.n, base.n, 8);  // the old stream is no longer served
    REQUIRE(l.rc == PQG_OK && l.hit == 0);
    print_lookup("rewalk_old_stream", l, c);
  }
}

// ---- pqg_router_read_runs: the pinned image ---------------------------------------------------------------

void runs_cases() {
  const std::string where = "runs_image";
  Stream s;
  s.data(100);
  Block in(s.b);
  {
    const uint64_t offs[3] = {0, 10, 60};
    const uint32_t cnts[3] = {8, 0, 40};
    RouterRunsImage im;
    REQUIRE(router_runs_layout(7, in.p, in.n, offs, cnts, 3, &im) == PQG_OK);  // 7, 0 and 35 bytes; the last ends at 95
    REQUIRE(im.n_bytes == 16 + 0 + 48 && im.n_vals == 48 && im.max_count == 40);
    REQUIRE(im.o_in == 256 && im.o_out == 256 + 24 && im.o_cnt == 256 + 48 && im.img == 512);
    std::vector<uint8_t> pin((size_t)im.img, 0xEE);
    Block img(pin);
    router_runs_fill(im, 7, in.p, offs, cnts, 3, img.p);
    REQUIRE(std::memcmp(img.p, in.p, 7) == 0 && std::memcmp(img.p + 16, in.p + 60, 35) == 0);
    for (size_t i = 7; i < 16; i++) REQUIRE(img.p[i] == 0);
    for (size_t i = 16 + 35; i < 256; i++) REQUIRE(img.p[i] == 0);
    const uint64_t* o_in = (const uint64_t*)(img.p + im.o_in);
    const uint64_t* o_out = (const uint64_t*)(img.p + im.o_out);
    const uint32_t* o_cnt = (const uint32_t*)(img.p + im.o_cnt);
    REQUIRE(o_in[0] == 0 && o_in[1] == 16 && o_in[2] == 16 && o_out[0] == 0 && o_out[1] == 8 && o_out[2] == 8);
    REQUIRE(o_cnt[0] == 8 && o_cnt[1] == 0 && o_cnt[2] == 40);
    g_cases++;
  }
  {
    RouterRunsImage im;
    const uint64_t off_end[1] = {100};
    const uint32_t c8[1] = {8}, c0[1] = {0}, c4[1] = {4};
    REQUIRE(router_runs_layout(8, in.p, in.n, off_end, c0, 1, &im) == PQG_OK && im.n_vals == 0);  // an empty slice at the end
    REQUIRE(router_runs_layout(8, in.p, in.n, off_end, c8, 1, &im) == PQG_ERR_EOF);
    const uint64_t off_past[1] = {101}, off_last[1] = {92}, off_cut[1] = {93};
    REQUIRE(router_runs_layout(8, in.p, in.n, off_past, c0, 1, &im) == PQG_ERR_EOF);
    REQUIRE(router_runs_layout(8, in.p, in.n, off_last, c8, 1, &im) == PQG_OK && im.n_bytes == 16);  // ends exactly at the end
    REQUIRE(router_runs_layout(8, in.p, in.n, off_cut, c8, 1, &im) == PQG_ERR_EOF);                 // one byte past it
    REQUIRE(router_runs_layout(8, in.p, in.n, off_last, c4, 1, &im) == PQG_ERR_INVALID_ARG);
    REQUIRE(router_runs_layout(8, nullptr, 100, off_last, c8, 1, &im) == PQG_ERR_INVALID_ARG);
    REQUIRE(router_runs_layout(0, nullptr, 0, off_last, c8, 1, &im) == PQG_ERR_EOF);
    const uint64_t off0[1] = {0};
    REQUIRE(router_runs_layout(0, nullptr, 0, off0, c8, 1, &im) == PQG_OK && im.n_vals == 8 && im.n_bytes == 0);
    g_cases++;
  }
}

// ---- error resolution -------------------------------------------------------------------------------------

constexpr uint64_t NONE = ~0ull;

struct Plan {
  PlanLayout L;
  std::vector<uint64_t> errs;  // decoded keys
  Plan(std::vector<int> page_cols, int n_cols) {
    L.n_pages = (int)page_cols.size();
    L.n_cols = n_cols;
    L.h_work.resize((size_t)std::max(L.n_pages, 1));
    std::memset(L.h_work.data(), 0, sizeof(PageWork) * L.h_work.size());
    L.col_first_page.assign((size_t)std::max(n_cols, 1), -1);
    L.page_cls.assign((size_t)std::max(L.n_pages, 1), -1);
    for (int p = 0; p < L.n_pages; p++) {
      const int c = page_cols[(size_t)p];
      L.h_work[(size_t)p].column = c;
      if (c >= 0 && c < n_cols && L.col_first_page[(size_t)c] < 0) L.col_first_page[(size_t)c] = p;
    }
    errs.assign(3 * (size_t)(L.n_pages + std::max(n_cols, 1)), NONE);
  }
  // the keys as the kernels and the planner form them
  Plan& init(int p, int phase, int code) { errs[3 * (size_t)p] = ((uint64_t)phase << 8) | (uint64_t)code; return *this; }
  Plan& level(int p, uint64_t slot, int dl, int code) { errs[3 * (size_t)p + 1] = (((slot << 1) | (uint64_t)dl) << 8) | (uint64_t)code; return *this; }
  Plan& value(int p, uint64_t idx, int code) { errs[3 * (size_t)p + 2] = (idx << 8) | (uint64_t)code; return *this; }
  Plan& dict(int col, int code) { errs[3 * (size_t)(L.n_pages + col)] = (uint64_t)code; return *this; }
  Plan& host_dict(int p, int code) { L.host_errs.push_back(HostErr{p, 0, -1, code}); return *this; }
  Plan& host_init(int p, int phase, int code) { L.host_errs.push_back(HostErr{p, 0, phase, code}); return *this; }
  Plan& no_words() { errs.clear(); return *this; }
};

struct Resolved {
  int rc, first;
  int64_t index;
  std::string what;
  std::vector<pqg_page_error> pe;
};

Resolved resolve(const std::string& where, const Plan& P) {
  Resolved r;
  r.first = -2;
  r.index = -2;
  const char* what = "(unset)";
  // the words in a block of their own size; the page errors start with something stale in them
  std::vector<uint64_t> errs(P.errs);
  errs.shrink_to_fit();
  r.pe.assign(3, pqg_page_error{99, 99, 99});
  r.rc = resolve_page_errors(P.L, errs, &r.pe, &r.first, &r.index, &what);
  r.what = what;
  REQUIRE(r.pe.size() == (size_t)P.L.n_pages);
  int first = -1;
  for (int p = 0; p < P.L.n_pages; p++) {
    const pqg_page_error& e = r.pe[(size_t)p];
    REQUIRE((e.code == PQG_OK) == (e.phase == PQG_PHASE_NONE));
    REQUIRE(e.phase >= PQG_PHASE_NONE && e.phase <= PQG_PHASE_VALUE);
    REQUIRE(e.phase == PQG_PHASE_RL_READ || e.phase == PQG_PHASE_DL_READ || e.phase == PQG_PHASE_VALUE || e.index == -1);
    if (e.code != PQG_OK && first < 0) first = p;
  }
  if (first < 0) {
    REQUIRE(r.rc == PQG_OK && r.first == -2 && r.index == -2 && r.what == "(unset)");
  } else {
    REQUIRE(r.rc == r.pe[(size_t)first].code && r.first == first);
  }
  return r;
}

void print_resolved(const char* name, const Resolved& r) {
  g_cases++;
  if (!g_print) return;
  std::printf("resolve %s rc=%d first=%d index=%lld what=\"%s\" pages=[", name, r.rc, r.first, (long long)r.index, r.what.c_str());
  for (size_t p = 0; p < r.pe.size(); p++)
    std::printf("%s%d/%d/%lld", p ? " " : "", r.pe[p].code, r.pe[p].phase, (long long)r.pe[p].index);
  std::printf("]\n");
}

// one page's expected outcome
void expect(const std::string& where, const Resolved& r, int page, int code, int phase, int64_t index, const char* what,
            int64_t st_index) {
  REQUIRE(r.pe[(size_t)page].code == code && r.pe[(size_t)page].phase == phase && r.pe[(size_t)page].index == index);
  if (r.first == page) REQUIRE(r.rc == code && r.what == what && r.index == st_index);
}

void resolve_cases() {
  // the sources of one page's error, strongest first: each alone, then every pair on one page
  struct Source {
    const char* name;
    void (*put)(Plan&);
    int code, phase;
    int64_t index;
    const char* what;
    int64_t st_index;
  };
  const Source src[] = {
      {"devdict", [](Plan& P) { P.dict(0, PQG_ERR_CORRUPT); }, PQG_ERR_CORRUPT, PQG_PHASE_DICTIONARY, -1, "dictionary page", -1},
      {"hostdict", [](Plan& P) { P.host_dict(1, PQG_ERR_DICT_ENCODING); }, PQG_ERR_DICT_ENCODING, PQG_PHASE_DICTIONARY, -1, "dictionary page", -1},
      {"hostinit", [](Plan& P) { P.host_init(1, 1, PQG_ERR_BIT_WIDTH); }, PQG_ERR_BIT_WIDTH, PQG_PHASE_DL_INIT, -1, "level init", 0},
      {"devinit", [](Plan& P) { P.init(1, 2, PQG_ERR_EOF); }, PQG_ERR_EOF, PQG_PHASE_DATA_INIT, -1, "data init", 0},
      {"value", [](Plan& P) { P.value(1, 77, PQG_ERR_DICT_ID); }, PQG_ERR_DICT_ID, PQG_PHASE_VALUE, 77, "value decode", 77},
      {"level_rl", [](Plan& P) { P.level(1, 5, 0, PQG_ERR_RLE_PAST_END); }, PQG_ERR_RLE_PAST_END, PQG_PHASE_RL_READ, 5, "level decode", 5},
      {"level_dl", [](Plan& P) { P.level(1, 9, 1, PQG_ERR_EOF); }, PQG_ERR_EOF, PQG_PHASE_DL_READ, 9, "level decode", 9},
  };
  const int n_src = (int)(sizeof(src) / sizeof(src[0]));
  // pages 0 (column 1), 1 (column 0, its first page), 2 (column 0)
  for (int a = 0; a < n_src; a++) {
    const std::string where = std::string("alone_") + src[a].name;
    Plan P({1, 0, 0}, 2);
    src[a].put(P);
    const Resolved r = resolve(where, P);
    REQUIRE(r.first == 1 && r.pe[0].code == PQG_OK && r.pe[2].code == PQG_OK);
    expect(where, r, 1, src[a].code, src[a].phase, src[a].index, src[a].what, src[a].st_index);
    print_resolved(where.c_str(), r);
  }
  for (int a = 0; a < n_src; a++)
    for (int b = a + 1; b < n_src; b++) {
      if (a == 2 && b == 3) continue;  // host init with device init: the smaller key, below
      if (a == 5 && b == 6) continue;  // one level word per page
      const std::string where = std::string("pair_") + src[a].name + "_" + src[b].name;
      Plan P({1, 0, 0}, 2);
      src[a].put(P);  // (of two host errors on a page the planner's first counts)
      src[b].put(P);
      const Resolved r = resolve(where, P);  // the earlier of the list wins
      REQUIRE(r.first == 1);
      expect(where, r, 1, src[a].code, src[a].phase, src[a].index, src[a].what, src[a].st_index);
      print_resolved(where.c_str(), r);
    }
  // host init against device init: the smaller key (phase << 8 | code), all three phases on either side
  const int phase_of[3] = {PQG_PHASE_RL_INIT, PQG_PHASE_DL_INIT, PQG_PHASE_DATA_INIT};
  for (int hp = 0; hp < 3; hp++)
    for (int dp = 0; dp < 3; dp++)
      for (int k = 0; k < 2; k++) {
        const int hcode = k ? PQG_ERR_EOF : PQG_ERR_BIT_WIDTH, dcode = k ? PQG_ERR_BIT_WIDTH : PQG_ERR_EOF;
        const std::string where = "init_host" + std::to_string(hp) + "_dev" + std::to_string(dp) + (k ? "_b" : "_a");
        Plan P({0}, 1);
        P.host_init(0, hp, hcode).init(0, dp, dcode);
        const Resolved r = resolve(where, P);
        const bool host_wins = ((hp << 8) | hcode) < ((dp << 8) | dcode);
        const int ph = host_wins ? hp : dp;
        expect(where, r, 0, host_wins ? hcode : dcode, phase_of[ph], -1, ph == 2 ? "data init" : "level init", 0);
        print_resolved(where.c_str(), r);
      }
  {  // host errors alone: no kernel reported, no words downloaded
    const std::string where = "host_only_no_words";
    Plan P({0, 0, 1}, 2);
    P.host_init(1, 0, PQG_ERR_BIT_WIDTH).host_dict(2, PQG_ERR_NO_DICTIONARY).no_words();
    const Resolved r = resolve(where, P);
    expect(where, r, 1, PQG_ERR_BIT_WIDTH, PQG_PHASE_RL_INIT, -1, "level init", 0);
    expect(where, r, 2, PQG_ERR_NO_DICTIONARY, PQG_PHASE_DICTIONARY, -1, "dictionary page", -1);
    REQUIRE(r.first == 1);
    print_resolved(where.c_str(), r);
  }
  {  // a page's second host error is not looked at
    const std::string where = "host_two_on_a_page";
    Plan P({0}, 1);
    P.host_init(0, 2, PQG_ERR_EOF).host_dict(0, PQG_ERR_CORRUPT).no_words();
    const Resolved r = resolve(where, P);
    expect(where, r, 0, PQG_ERR_EOF, PQG_PHASE_DATA_INIT, -1, "data init", 0);
    print_resolved(where.c_str(), r);
  }
  {  // nothing anywhere
    const std::string where = "clean";
    Plan P({0, 1, 0}, 2);
    Resolved r = resolve(where, P);
    REQUIRE(r.rc == PQG_OK);
    print_resolved("clean", r);
    P.no_words();
    r = resolve(where, P);
    REQUIRE(r.rc == PQG_OK);
    print_resolved("clean_no_words", r);
  }
  {  // the dictionary pseudo-page belongs to the column's first page only, wherever that page is
    const std::string where = "dict_first_page_only";
    Plan P({1, 1, 0, 1, 0}, 2);
    P.dict(0, PQG_ERR_CORRUPT);
    Resolved r = resolve(where, P);
    REQUIRE(r.first == 2 && r.pe[4].code == PQG_OK && r.pe[0].code == PQG_OK);
    expect(where, r, 2, PQG_ERR_CORRUPT, PQG_PHASE_DICTIONARY, -1, "dictionary page", -1);
    print_resolved(where.c_str(), r);
    Plan Q({1, 1, 0, 1, 0}, 2);
    Q.dict(1, PQG_ERR_EOF).value(4, 3, PQG_ERR_DICT_ID);
    r = resolve(where, Q);
    REQUIRE(r.first == 0 && r.pe[1].code == PQG_OK && r.pe[3].code == PQG_OK);
    expect(where, r, 0, PQG_ERR_EOF, PQG_PHASE_DICTIONARY, -1, "dictionary page", -1);
    expect(where, r, 4, PQG_ERR_DICT_ID, PQG_PHASE_VALUE, 3, "value decode", 3);
    print_resolved("dict_first_page_only_col1", r);
  }
  {  // a page of no column of the plan takes no dictionary error
    const std::string where = "page_without_column";
    Plan P({-1, 5, 0}, 1);
    P.dict(0, PQG_ERR_CORRUPT).level(0, 1, 1, PQG_ERR_EOF);
    const Resolved r = resolve(where, P);
    expect(where, r, 0, PQG_ERR_EOF, PQG_PHASE_DL_READ, 1, "level decode", 1);
    expect(where, r, 2, PQG_ERR_CORRUPT, PQG_PHASE_DICTIONARY, -1, "dictionary page", -1);
    REQUIRE(r.pe[1].code == PQG_OK);
    print_resolved(where.c_str(), r);
  }
  {  // the first failing page decides the status text
    const std::string where = "first_page_decides";
    Plan P({0, 0, 0, 1}, 2);
    P.value(1, 1ull << 39, PQG_ERR_DELTA_PAST_END).dict(1, PQG_ERR_CORRUPT).level(2, 0, 0, PQG_ERR_EOF);
    const Resolved r = resolve(where, P);
    REQUIRE(r.first == 1 && r.rc == PQG_ERR_DELTA_PAST_END && r.what == "value decode" && r.index == (int64_t)(1ull << 39));
    expect(where, r, 3, PQG_ERR_CORRUPT, PQG_PHASE_DICTIONARY, -1, "dictionary page", -1);
    expect(where, r, 2, PQG_ERR_EOF, PQG_PHASE_RL_READ, 0, "level decode", 0);
    print_resolved(where.c_str(), r);
  }
  for (int n_cols = 0; n_cols < 2; n_cols++) {  // no pages
    const std::string where = "no_pages_cols" + std::to_string(n_cols);
    Plan P({}, n_cols);
    Resolved r = resolve(where, P);
    REQUIRE(r.rc == PQG_OK && r.pe.empty());
    print_resolved(where.c_str(), r);
    P.errs[0] = PQG_ERR_CORRUPT;  // a dictionary word with no page to carry it
    r = resolve(where, P);
    REQUIRE(r.rc == PQG_OK && r.pe.empty());
    print_resolved((where + "_dict_word").c_str(), r);
    P.no_words();
    r = resolve(where, P);
    REQUIRE(r.rc == PQG_OK && r.pe.empty());
    print_resolved((where + "_no_words").c_str(), r);
  }
  {  // raw words: those of another launch epoch are ignored
    const std::string where = "stale_epochs";
    auto raw = [](uint32_t epoch, uint64_t key) { return ((uint64_t)epoch << 48) | (~key & ERR_KEY_MASK); };
    Plan P({0, 0}, 1);
    const uint64_t k_val = (12ull << 8) | PQG_ERR_DICT_ID, k_lvl = (((3ull << 1) | 1ull) << 8) | PQG_ERR_EOF;
    std::vector<uint64_t> words(P.errs.size(), 0);  // a zeroed region: epoch 0
    words[2] = raw(6, k_val);                       // page 0, an earlier launch
    words[3 + 1] = raw(7, k_lvl);                   // page 1, this launch
    words[3 + 2] = raw(8, k_val);                   // page 1, a later epoch (cannot happen; still not this launch)
    words[6] = raw(ERR_EPOCH_MAX, PQG_ERR_CORRUPT); // the dictionary, the last epoch before the wrap
    words.shrink_to_fit();
    std::vector<uint64_t> w7(words), wmax(words), w0(words);
    decode_error_words(&w7, 7);
    for (size_t i = 0; i < w7.size(); i++) REQUIRE(w7[i] == (i == 4 ? k_lvl : NONE));
    P.errs = w7;
    Resolved r = resolve(where, P);
    REQUIRE(r.first == 1 && r.pe[0].code == PQG_OK);
    expect(where, r, 1, PQG_ERR_EOF, PQG_PHASE_DL_READ, 3, "level decode", 3);
    print_resolved("stale_epoch7", r);
    decode_error_words(&wmax, ERR_EPOCH_MAX);
    for (size_t i = 0; i < wmax.size(); i++) REQUIRE(wmax[i] == (i == 6 ? (uint64_t)PQG_ERR_CORRUPT : NONE));
    P.errs = wmax;
    r = resolve(where, P);
    expect(where, r, 0, PQG_ERR_CORRUPT, PQG_PHASE_DICTIONARY, -1, "dictionary page", -1);
    print_resolved("stale_epoch_max", r);
    decode_error_words(&w0, 1);
    for (uint64_t w : w0) REQUIRE(w == NONE);
    P.errs = w0;
    r = resolve(where, P);
    REQUIRE(r.rc == PQG_OK);
    print_resolved("stale_all", r);
    if (g_print) std::printf("decode stale w7=%016llx wmax=%016llx w0=%016llx\n", (unsigned long long)fnv_vec(w7),
                             (unsigned long long)fnv_vec(wmax), (unsigned long long)fnv_vec(w0));
    g_cases++;
  }
  {  // pqg_sync's timeout re-runs look at the failing page's class
    const std::string where = "page_class";
    Plan P({0, 0, 0}, 1);
    for (int c = -1; c < C_NCLS; c++) {
      P.L.page_cls = {c, C_PLAIN, -1};
      const bool dict = c == C_DICT4 || c == C_DICT8 || c == C_IDS || c == C_DD || c == C_DDG;
      REQUIRE(page_is_dict_class(P.L, 0) == dict && page_is_binp(P.L, 0) == (c == C_BINP));
      REQUIRE(!page_is_dict_class(P.L, 1) && !page_is_binp(P.L, 2));
    }
    P.L.page_cls = {C_DICT4, C_BINP, C_BINP};
    REQUIRE(!page_is_dict_class(P.L, -1) && !page_is_binp(P.L, -1) && !page_is_dict_class(P.L, 3) && !page_is_binp(P.L, 3));
    g_cases++;
  }
}

// ---- the length prefixes of a BYTE_ARRAY dictionary page ------------------------------------------------------

struct Dict {
  std::vector<uint8_t> b;
  Dict& entry(uint32_t len, uint32_t present) {  // a prefix saying len, followed by `present` bytes
    for (int i = 0; i < 4; i++) b.push_back((uint8_t)(len >> (8 * i)));
    for (uint32_t i = 0; i < present; i++) b.push_back((uint8_t)('a' + i % 26));
    return *this;
  }
  Dict& cut(size_t n) { b.resize(b.size() - n); return *this; }
};

void dict_case(const char* name, const Dict& d, uint32_t n_values, int want) {
  const std::string where = name;
  Block page(d.b);
  const int rc = dict_page_eof_code(page.p, page.n, n_values);
  REQUIRE(rc == want);
  g_cases++;
  if (g_print) std::printf("dict %s size=%zu n=%u rc=%d\n", name, page.n, n_values, rc);
}

void dict_cases() {
  dict_case("empty_n0", Dict(), 0, PQG_ERR_EOF);
  dict_case("empty_n1", Dict(), 1, PQG_ERR_EOF);
  dict_case("prefix_cut_1", Dict().entry(3, 3).entry(5, 0).cut(3), 2, PQG_ERR_EOF);
  dict_case("prefix_cut_2", Dict().entry(3, 3).entry(5, 0).cut(2), 2, PQG_ERR_EOF);
  dict_case("prefix_cut_3", Dict().entry(3, 3).entry(5, 0).cut(1), 2, PQG_ERR_EOF);
  dict_case("first_prefix_cut_3", Dict().entry(0, 0).cut(1), 1, PQG_ERR_EOF);
  dict_case("negative_length", Dict().entry(3, 3).entry(0x80000000u, 8), 2, PQG_ERR_CORRUPT);
  dict_case("negative_length_minus_1", Dict().entry(0xFFFFFFFFu, 0), 1, PQG_ERR_CORRUPT);
  dict_case("largest_length", Dict().entry(0x7FFFFFFFu, 4), 1, PQG_ERR_CORRUPT);
  dict_case("ends_at_the_end", Dict().entry(3, 3).entry(0, 0).entry(7, 7), 3, PQG_ERR_EOF);
  dict_case("ends_at_the_end_one_more", Dict().entry(3, 3).entry(0, 0).entry(7, 7), 4, PQG_ERR_EOF);
  dict_case("one_byte_past", Dict().entry(3, 3).entry(0, 0).entry(8, 7), 3, PQG_ERR_CORRUPT);
  dict_case("one_byte_past_fewer_values", Dict().entry(3, 3).entry(0, 0).entry(8, 7), 2, PQG_ERR_EOF);
  dict_case("first_entry_past", Dict().entry(1, 0), 5, PQG_ERR_CORRUPT);
}

// ---- seeded random mutation -------------------------------------------------------------------------------

void fuzz(int n) {
  Rng rng{0xA5A5};
  const int widths[] = {0, 1, 2, 3, 7, 8, 9, 16, 17, 24, 31, 32};
  for (int it = 0; it < n; it++) {  // the router: a random hybrid stream, then random bytes of it changed or cut off
    const std::string where = "fuzz_router_" + std::to_string(it);
    const int w = widths[rng.below(12)];
    const int count = 8 * (int)(1 + rng.below(4));
    Stream s;
    s.rng.s = rng.next();
    s.first(count, w);
    for (uint32_t k = rng.below(12); k > 0; k--) {
      const uint32_t kind = rng.below(8);
      if (kind < 3) s.rle(rng.below(1000), w);
      else if (kind < 7) s.packed(rng.below(6), w);
      else s.header_only(rng.next() >> rng.below(64));
    }
    const size_t need = (size_t)count * (size_t)w / 8u;
    for (uint32_t k = rng.below(4); k > 0 && s.b.size() > need; k--) {
      const size_t at = need + rng.below((uint32_t)(s.b.size() - need));
      s.b[at] = rng.below(4) ? (uint8_t)rng.next() : (uint8_t)(0x80 | rng.next());
    }
    if (rng.below(3) == 0 && s.b.size() > need) s.b.resize(need + rng.below((uint32_t)(s.b.size() - need)));
    RouterCache c;
    walk(where, c, w, s.b, count);
    fill(c, w);
    Block base(s.b);
    for (size_t r = 0; r < c.off.size() && r < 16; r++) {
      const Lookup l = lookup(&c, w, base.p + c.off[r], base.n - c.off[r], base.n - c.off[r], (int)c.cnt[r]);
      // (at width 0 several runs share a position; the first of them is served)
      REQUIRE(l.rc == PQG_OK && (l.hit == 1 || w == 0));
      if (l.hit && w > 0) REQUIRE(l.out[0] == fake_value(c.vo[r]) && l.out.back() == fake_value(c.vo[r] + c.cnt[r] - 1));
    }
    const size_t at = rng.below((uint32_t)base.n + 1);
    const int cnt2 = 8 * (int)rng.below(5);
    const Lookup l = lookup(&c, widths[rng.below(12)], base.p + at, base.n - at, base.n - at, cnt2);
    REQUIRE(l.rc == PQG_OK || l.rc == PQG_ERR_EOF);
    g_cases++;
  }
  for (int it = 0; it < n; it++) {  // the resolver: random words and host errors on random small plans
    const std::string where = "fuzz_resolve_" + std::to_string(it);
    const int n_pages = (int)rng.below(7), n_cols = (int)rng.below(4);
    std::vector<int> page_cols;
    for (int p = 0; p < n_pages; p++) page_cols.push_back((int)rng.below((uint32_t)n_cols + 2) - 1);
    Plan P(page_cols, n_cols);
    const uint32_t epoch = 1 + rng.below(ERR_EPOCH_MAX);
    std::vector<uint64_t> raw(P.errs.size());
    for (uint64_t& wd : raw) {
      const uint32_t kind = rng.below(8);
      // any key, with an error code in its low byte as every reporter puts one there
      const uint64_t key = (rng.below(2) ? (rng.next() >> rng.below(64)) & ~0xFFull : (uint64_t)rng.below(3) << 8) | (1 + rng.below(20));
      wd = kind < 4 ? 0 : ((uint64_t)(kind < 7 ? epoch : 1 + rng.below(ERR_EPOCH_MAX)) << 48) | (~key & ERR_KEY_MASK);
    }
    raw.shrink_to_fit();
    decode_error_words(&raw, epoch);
    for (uint64_t wd : raw) REQUIRE(wd == NONE || wd <= ERR_KEY_MASK);
    P.errs = raw;
    for (uint32_t k = n_pages ? rng.below(4) : 0; k > 0; k--)
      P.L.host_errs.push_back(HostErr{(int)rng.below((uint32_t)n_pages), 0, (int64_t)rng.below(4) - 1, (int)(1 + rng.below(20))});
    if (rng.below(5) == 0) P.no_words();
    (void)resolve(where, P);
    g_cases++;
  }
  for (int it = 0; it < n; it++) {  // dictionary pages: random prefixes
    const std::string where = "fuzz_dict_" + std::to_string(it);
    Dict d;
    for (uint32_t k = rng.below(6); k > 0; k--) {
      const uint32_t len = rng.below(4) ? rng.below(20) : (uint32_t)(rng.next() >> rng.below(64));
      d.entry(len, std::min(len, rng.below(24)));
    }
    if (rng.below(3) == 0 && !d.b.empty()) d.cut(rng.below((uint32_t)d.b.size()) % 5 % d.b.size());
    Block page(d.b);
    const int rc = dict_page_eof_code(page.p, page.n, rng.below(8));
    REQUIRE(rc == PQG_ERR_EOF || rc == PQG_ERR_CORRUPT);
    g_cases++;
  }
}

}  // namespace

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "cases" || mode == "digest") {
    g_print = mode == "digest";
    router_cases();
    runs_cases();
    resolve_cases();
    dict_cases();
  } else if (mode == "fuzz" && argc > 2) {
    fuzz(std::atoi(argv[2]));
  } else {
    std::fprintf(stderr, "usage: api_host_main cases | digest | fuzz N\n");
    return 2;
  }
  std::printf("cases=%d\n", g_cases);
  return 0;
}
