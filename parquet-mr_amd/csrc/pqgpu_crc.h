// pqgpu_crc.h — pqg_crc32_pages (include/pqgpu.h, "page checksums"): the tables the kernels read,
// shared by the host half (pqgpu_crc_host.cpp: validation, the tile table, the GF(2) helpers and the
// generated constants; plain C++) and the device half (pqgpu_crc.hip).
//
// Algebra. A 32-bit CRC state is a polynomial over GF(2) modulo P (reflected, 0xEDB88320: bit 31 is
// x^0). Feeding a zero byte multiplies the state by x^8, and feeding the dword d to the state s gives
// (s ^ d) * x^32. So "a state v at byte position p" is worth v * x^(8 (E - p)) at the end E of the
// message, whether v was computed from bytes before p or is itself a dword of data at [p, p + 4): states
// of disjoint byte sets add (XOR) once they are moved to one position. P is irreducible, so x has the
// order 2^32 - 1 and a move backwards is a multiplication too (exponents are taken modulo 2^32 - 1):
// bytes masked to zero may be placed after a range's end and are divided out again.
// The 0xFFFFFFFF start value is a dword of data at the job's first byte (XORed into the first four
// bytes, which may lie past the end of a job shorter than that); the final inversion is the fold's.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/pqgpu.h"

namespace pqg {

constexpr uint32_t CRC_POLY = 0xEDB88320u;
constexpr uint32_t CRC_X0 = 0x80000000u;   // x^0
constexpr uint32_t CRC_ROW = 1024;         // bytes a wave loads at once: 16 per lane
constexpr uint32_t CRC_FOLD_LANES = 64;    // k_crc_fold: lane j takes the tiles j, j + 64, ...
constexpr uint64_t CRC_MAX_TILES = 1ull << 28;  // per call
constexpr uint32_t CRC_TILE_FIRST = 1;     // CrcTile::flags: the job's first tile (the start value goes in)

// One (job, tile): size bytes of d_bytes from `start` (the last tile of a job is short, none is empty).
struct CrcTile {
  uint64_t start;
  uint32_t size;
  uint32_t flags;
};
static_assert(sizeof(CrcTile) == 16, "CrcTile layout");

// One job as k_crc_fold sees it: its tiles are tile_begin .. tile_begin + n_tiles of the tile table.
struct CrcJobDev {
  uint64_t tile_begin;
  uint32_t size;
  uint32_t expected;
  uint32_t flags;
  uint32_t n_tiles;
};
static_assert(sizeof(CrcJobDev) == 24 && sizeof(pqg_crc_job) == 24, "crc job layout");

// The constants of one tile size T, as uint32 words in this order (crc_build_tables):
//   step4[4][256]   (b << 8k) * x^32: s * x^32 = the XOR of the four lookups of s's bytes
//   row[4][256]     (b << 8k) * x^(8 * CRC_ROW): the same over a whole row
//   xp8[2 T]        x^(8 (i - T)): moves of -T .. T - 1 bytes
//   xt[65]          x^(8 k T): moves of k tiles
constexpr uint32_t CRC_TAB_STEP4 = 0, CRC_TAB_ROW = 1024, CRC_TAB_XP8 = 2048;
inline uint32_t crc_tab_xt(uint32_t tile) { return CRC_TAB_XP8 + 2 * tile; }
inline size_t crc_table_words(uint32_t tile) { return (size_t)crc_tab_xt(tile) + CRC_FOLD_LANES + 1; }
inline bool crc_tile_ok(uint32_t tile) { return tile == 4096 || tile == 8192 || tile == 16384 || tile == 32768; }

uint32_t crc_mulmodp(uint32_t a, uint32_t b);  // a * b mod P
uint32_t crc_x8n(uint64_t n);                  // x^(8 n) mod P
uint32_t crc_x8n_back(uint64_t n);             // x^(-8 n) mod P
void crc_build_tables(uint32_t tile, uint32_t* out /* crc_table_words(tile) */);

// The host-side refusals of pqg_crc32_pages; on PQG_OK *n_tiles = entries of the tile table.
int crc_validate(bool have_ctx, const void* d_bytes, uint64_t n_bytes, const pqg_crc_job* jobs, int n_jobs,
                 const void* d_status, uint32_t tile, uint64_t* n_tiles);
// The tables of a validated call: jd[n_jobs], tiles[n_tiles], in job order.
void crc_build(const pqg_crc_job* jobs, int n_jobs, uint32_t tile, CrcJobDev* jd, CrcTile* tiles);

}  // namespace pqg
