// crc_host_main.cpp — the host half of pqg_crc32_pages (csrc/pqgpu_crc_host.cpp) under
// AddressSanitizer + UndefinedBehaviorSanitizer: job validation, the tile-table builder, the generated
// constants and pqg_crc_jobs_from_headers, driven with exactly-sized heap buffers (a write or read one
// element past any of them aborts the run). Arguments: files of raw column-chunk bytes, framed with
// pqg_frame_chunk; their header arrays are then mutated. Prints one line per check group; exit 0 = clean.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../parquet-mr_amd/csrc/pqgpu_crc.h"

namespace {

int g_fail = 0;
#define CHECK(c)                                                          \
  do {                                                                    \
    if (!(c)) {                                                           \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
      g_fail++;                                                           \
    }                                                                     \
  } while (0)

uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint64_t rnd() {
  g_rng ^= g_rng << 13;
  g_rng ^= g_rng >> 7;
  g_rng ^= g_rng << 17;
  return g_rng;
}

const int kDummy = 0;
const void* const kDev = &kDummy;  // stands for a device pointer: validation only tests it for NULL

// Validates the jobs (a heap copy of exactly n) and, when they pass, builds both tables into heap arrays
// of exactly the sizes asked for and checks every entry.
int run(const std::vector<pqg_crc_job>& jobs_in, uint64_t n_bytes, uint32_t tile, bool build = true) {
  const int n = (int)jobs_in.size();
  std::unique_ptr<pqg_crc_job[]> jobs(new pqg_crc_job[(size_t)n]);
  for (int j = 0; j < n; j++) jobs[(size_t)j] = jobs_in[(size_t)j];
  uint64_t n_tiles = ~0ull;
  const int rc = pqg::crc_validate(true, kDev, n_bytes, jobs.get(), n, kDev, tile, &n_tiles);
  if (rc != PQG_OK) {
    CHECK(n_tiles == 0);
    return rc;
  }
  if (!build) return rc;
  std::unique_ptr<pqg::CrcJobDev[]> jd(new pqg::CrcJobDev[(size_t)n]);
  std::unique_ptr<pqg::CrcTile[]> tiles(new pqg::CrcTile[(size_t)n_tiles]);
  pqg::crc_build(jobs.get(), n, tile, jd.get(), tiles.get());
  uint64_t at = 0;
  for (int j = 0; j < n; j++) {
    const pqg_crc_job& J = jobs[(size_t)j];
    const pqg::CrcJobDev& D = jd[(size_t)j];
    CHECK(D.tile_begin == at && D.size == J.size && D.expected == J.expected && D.flags == J.flags);
    CHECK(D.n_tiles == (uint32_t)(((uint64_t)J.size + tile - 1) / tile));
    uint64_t covered = 0;
    for (uint32_t t = 0; t < D.n_tiles; t++) {
      const pqg::CrcTile& X = tiles[(size_t)(at + t)];
      CHECK(X.start == J.offset + covered && X.size >= 1 && X.size <= tile);
      CHECK(X.size == tile || t + 1 == D.n_tiles);  // only the last tile is short
      CHECK(X.flags == (t == 0 ? pqg::CRC_TILE_FIRST : 0u));
      CHECK(X.start + X.size <= n_bytes);
      covered += X.size;
    }
    CHECK(covered == J.size);
    at += D.n_tiles;
  }
  CHECK(at == n_tiles);
  return rc;
}

pqg_crc_job job(uint64_t off, uint32_t size, uint32_t flags = 0, uint32_t reserved = 0) {
  return pqg_crc_job{off, size, 0x12345678u, flags, reserved};
}

void validation_and_tiles() {
  const uint32_t tiles[] = {4096, 8192, 16384, 32768};
  for (uint32_t T : tiles) {
    CHECK(run({}, 0, T) == PQG_OK);  // empty job list
    CHECK(run({}, 100, T) == PQG_OK);
    CHECK(run({job(0, 0), job(50, 0), job(100, 0)}, 100, T) == PQG_OK);  // zero-size jobs, one at the very end
    CHECK(run({job(0, 0)}, 0, T) == PQG_OK);
    CHECK(run({job(0, 100), job(1, 99), job(99, 1)}, 100, T) == PQG_OK);  // ending exactly at n_bytes
    CHECK(run({job(1, 100)}, 100, T) == PQG_ERR_INVALID_ARG);             // one byte past it
    CHECK(run({job(0, 101)}, 100, T) == PQG_ERR_INVALID_ARG);
    CHECK(run({job(101, 0)}, 100, T) == PQG_ERR_INVALID_ARG);
    CHECK(run({job(0, 10), job(~0ull, 2)}, 100, T) == PQG_ERR_INVALID_ARG);  // offset + size wraps
    CHECK(run({job(~0ull - 1, 0xFFFFFFFFu)}, ~0ull, T) == PQG_ERR_INVALID_ARG);
    CHECK(run({job(0, 10, 0, 1)}, 100, T) == PQG_ERR_INVALID_ARG);           // reserved
    CHECK(run({job(0, 10, 2)}, 100, T) == PQG_ERR_INVALID_ARG);              // unknown flag
    CHECK(run({job(0, 10, PQG_CRC_VERIFY | 0x80000000u)}, 100, T) == PQG_ERR_INVALID_ARG);
    CHECK(run({job(0, 10, PQG_CRC_VERIFY)}, 100, T) == PQG_OK);
    std::vector<pqg_crc_job> around;  // sizes around tile multiples, any offset
    for (uint32_t k = 0; k <= 3; k++)
      for (int d = -2; d <= 2; d++) {
        const int64_t s = (int64_t)k * T + d;
        if (s >= 0) around.push_back(job(rnd() % 17, (uint32_t)s, PQG_CRC_VERIFY));
      }
    CHECK(run(around, 3ull * T + 2 + 16, T) == PQG_OK);
    std::vector<pqg_crc_job> many;  // overlapping, repeated, unordered
    for (int i = 0; i < 500; i++) {
      const uint32_t s = (uint32_t)(rnd() % (5 * T));
      many.push_back(job(rnd() % (6ull * T - s), s));
    }
    CHECK(run(many, 6ull * T, T) == PQG_OK);
    // a 4 GiB - 1 job: the tables only, no data
    CHECK(run({job(3, 0xFFFFFFFFu, PQG_CRC_VERIFY), job(0, 1)}, (1ull << 32) + 2, T) == PQG_OK);
    CHECK(run({job(3, 0xFFFFFFFFu)}, (1ull << 32) + 1, T) == PQG_ERR_INVALID_ARG);
  }
  // more tiles than one call takes: refused before anything is built (jobs may overlap)
  CHECK(run(std::vector<pqg_crc_job>(1100, job(0, 0xFFFFFFFFu)), 1ull << 32, 4096, false) == PQG_ERR_UNSUPPORTED);
  // argument refusals
  uint64_t nt = 0;
  pqg_crc_job one = job(0, 1);
  CHECK(pqg::crc_validate(false, kDev, 10, &one, 1, kDev, 16384, &nt) == PQG_ERR_INVALID_ARG);
  CHECK(pqg::crc_validate(true, kDev, 10, &one, -1, kDev, 16384, &nt) == PQG_ERR_INVALID_ARG);
  CHECK(pqg::crc_validate(true, nullptr, 10, &one, 1, kDev, 16384, &nt) == PQG_ERR_INVALID_ARG);
  CHECK(pqg::crc_validate(true, kDev, 10, nullptr, 1, kDev, 16384, &nt) == PQG_ERR_INVALID_ARG);
  CHECK(pqg::crc_validate(true, kDev, 10, &one, 1, nullptr, 16384, &nt) == PQG_ERR_INVALID_ARG);
  CHECK(pqg::crc_validate(true, kDev, 10, &one, 1, kDev, 12345, &nt) == PQG_ERR_INVALID_ARG);
  CHECK(pqg::crc_validate(true, nullptr, 0, nullptr, 0, nullptr, 16384, &nt) == PQG_OK && nt == 0);
  std::printf("validation tiles fail=%d\n", g_fail);
}

void constants() {
  for (uint32_t T : {4096u, 32768u}) {
    const size_t n = pqg::crc_table_words(T);
    std::unique_ptr<uint32_t[]> tab(new uint32_t[n]);
    pqg::crc_build_tables(T, tab.get());
    const uint32_t* xp8 = tab.get() + pqg::CRC_TAB_XP8;
    CHECK(xp8[T] == pqg::CRC_X0 && xp8[T + 1] == pqg::crc_x8n(1) && xp8[0] == pqg::crc_x8n_back(T));
    CHECK(pqg::crc_mulmodp(xp8[T - 77], xp8[T + 77]) == pqg::CRC_X0);  // x^-n * x^n = 1
    CHECK(tab[pqg::crc_tab_xt(T)] == pqg::CRC_X0 && tab[pqg::crc_tab_xt(T) + 64] == pqg::crc_x8n(64ull * T));
    // the row table against byte-at-a-time pqg_crc32 of a dword followed by zeros (no start value, no inversion)
    std::vector<uint8_t> msg(pqg::CRC_ROW, 0);
    const uint32_t d = (uint32_t)rnd();
    std::memcpy(msg.data(), &d, 4);
    uint32_t raw = ~pqg_crc32(~0u, msg.data(), msg.size());
    const uint32_t* row = tab.get() + pqg::CRC_TAB_ROW;
    CHECK((row[d & 0xFF] ^ row[256 + ((d >> 8) & 0xFF)] ^ row[512 + ((d >> 16) & 0xFF)] ^ row[768 + (d >> 24)]) == raw);
    raw = ~pqg_crc32(~0u, msg.data(), 4);
    const uint32_t* s4 = tab.get() + pqg::CRC_TAB_STEP4;
    CHECK((s4[d & 0xFF] ^ s4[256 + ((d >> 8) & 0xFF)] ^ s4[512 + ((d >> 16) & 0xFF)] ^ s4[768 + (d >> 24)]) == raw);
  }
  // combine against pqg_crc32 on real buffers
  std::vector<uint8_t> buf(70000);
  for (auto& b : buf) b = (uint8_t)rnd();
  for (size_t cut : {(size_t)0, (size_t)1, (size_t)16383, (size_t)16384, (size_t)69999, (size_t)70000}) {
    const uint32_t a = pqg_crc32(0, buf.data(), cut), b = pqg_crc32(0, buf.data() + cut, buf.size() - cut);
    CHECK(pqg_crc32_combine(a, b, buf.size() - cut) == pqg_crc32(0, buf.data(), buf.size()));
  }
  std::printf("constants fail=%d\n", g_fail);
}

void headers(const char* path) {
  std::FILE* f = std::fopen(path, "rb");
  if (!f) {
    std::fprintf(stderr, "cannot open %s\n", path);
    g_fail++;
    return;
  }
  std::fseek(f, 0, SEEK_END);
  const long len = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  std::unique_ptr<uint8_t[]> raw(new uint8_t[(size_t)len]);
  CHECK(std::fread(raw.get(), 1, (size_t)len, f) == (size_t)len);
  std::fclose(f);
  int n_h = 0;
  pqg_status st;
  pqg_frame_chunk(raw.get(), (uint64_t)len, -1, 0, nullptr, 0, &n_h, &st);
  std::unique_ptr<pqg_page_header[]> h(new pqg_page_header[(size_t)n_h]);
  CHECK(pqg_frame_chunk(raw.get(), (uint64_t)len, -1, 1, h.get(), n_h, &n_h, &st) == PQG_OK);
  int jobs_seen = 0, refused = 0;
  for (int round = 0; round < 40; round++) {
    std::unique_ptr<pqg_page_header[]> m(new pqg_page_header[(size_t)n_h]);
    for (int i = 0; i < n_h; i++) m[(size_t)i] = h[(size_t)i];
    for (int k = 0; round && k < 3 && n_h; k++) {  // round 0: as framed
      pqg_page_header& x = m[(size_t)(rnd() % (uint64_t)n_h)];
      switch (rnd() % 6) {
        case 0: x.has_crc = !x.has_crc; break;
        case 1: x.compressed_page_size = (int32_t)rnd(); break;
        case 2: x.body_offset = rnd(); break;
        case 3: x.type = (int32_t)(rnd() % 6) - 1; break;
        case 4: x.crc = (uint32_t)rnd(); break;
        default: x.compressed_page_size = -1; break;
      }
    }
    int need = -1;
    const int rc0 = pqg_crc_jobs_from_headers(m.get(), n_h, 0, nullptr, nullptr, 0, &need, &st);
    if (rc0 == PQG_ERR_INVALID_ARG && need <= 0 && st.value_index < 0) {  // a negative size: refused
      refused++;
      continue;
    }
    CHECK(need >= 0 && (need == 0 ? rc0 == PQG_OK : (rc0 == PQG_ERR_INVALID_ARG && st.value_index == need)));
    std::unique_ptr<pqg_crc_job[]> jobs(new pqg_crc_job[(size_t)need]);
    std::unique_ptr<int32_t[]> hoj(new int32_t[(size_t)need]);
    int got = -1;
    CHECK(pqg_crc_jobs_from_headers(m.get(), n_h, 7, jobs.get(), hoj.get(), need, &got, &st) == PQG_OK && got == need);
    for (int j = 0; j < got; j++) {
      const pqg_page_header& x = m[(size_t)hoj[(size_t)j]];
      CHECK(hoj[(size_t)j] >= 0 && hoj[(size_t)j] < n_h && x.has_crc && (j == 0 || hoj[(size_t)j] > hoj[(size_t)j - 1]));
      CHECK(jobs[(size_t)j].offset == 7 + x.body_offset && jobs[(size_t)j].size == (uint32_t)x.compressed_page_size &&
            jobs[(size_t)j].expected == x.crc && jobs[(size_t)j].flags == PQG_CRC_VERIFY && jobs[(size_t)j].reserved == 0);
    }
    if (got > 1) {  // one short: nothing is written past the capacity
      std::unique_ptr<pqg_crc_job[]> few(new pqg_crc_job[(size_t)got - 1]);
      std::unique_ptr<int32_t[]> fewh(new int32_t[(size_t)got - 1]);
      CHECK(pqg_crc_jobs_from_headers(m.get(), n_h, 7, few.get(), fewh.get(), got - 1, &need, &st) == PQG_ERR_INVALID_ARG);
    }
    // the jobs of mutated headers against the chunk's length: in range or refused, never out of bounds
    std::vector<pqg_crc_job> v(jobs.get(), jobs.get() + got);
    const int rc = run(v, 7 + (uint64_t)len, 4096);
    CHECK(rc == PQG_OK || rc == PQG_ERR_INVALID_ARG);
    if (round == 0) CHECK(rc == PQG_OK);
    jobs_seen += got;
  }
  std::printf("headers %s n=%d jobs=%d refused=%d fail=%d\n", path, n_h, jobs_seen, refused, g_fail);
}

}  // namespace

int main(int argc, char** argv) {
  validation_and_tiles();
  constants();
  for (int i = 1; i < argc; i++) headers(argv[i]);
  return g_fail ? 1 : 0;
}
