// pqgpu_aes.h — pqg_decrypt_pages (include/pqgpu.h, "encrypted pages"): the tables the kernels read,
// shared by the host half (pqgpu_aes_host.cpp: validation, key expansion, H and its powers, the tile and
// job tables, pqg_module_aad; plain C++) and the device half (pqgpu_aes.hip).
//
// AES (FIPS-197). The state and the round keys are four big-endian words, w = b0 << 24 | b1 << 16 |
// b2 << 8 | b3, and one table serves all rounds: te0[x] = (2 S[x], S[x], S[x], 3 S[x]) from the top byte
// down; the other three columns of MixColumns are its rotations and S[x] itself is its second byte.
//
// GHASH (SP 800-38D §6.3-6.4). A block is an element of GF(2^128) whose coefficient of x^i is bit i of
// the block counted from the most significant bit of its first byte; the modulus is x^128 + x^7 + x^2 +
// x + 1 (R = 0xE1 << 120). GHASH_H(X_1 .. X_m) = sum of X_i * H^(m + 1 - i): like the CRC (pqgpu_crc.h)
// it splits into pieces that are moved to one position by powers of H and added. Two forms of a block:
//   "bytes"  the 16 bytes as they sit in memory (what the tile kernel loads and the 4-bit table holds)
//   "words"  four big-endian words, words[0] the first four bytes: what the bit-serial product shifts
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/pqgpu.h"

namespace pqg {

constexpr uint32_t AES_ROW = 1024;           // bytes a wave takes at once: one 16-byte block per lane
constexpr uint32_t AES_ROW_BLOCKS = 64;
constexpr uint32_t AES_FOLD_LANES = 64;      // k_aes_fold: lane j takes the items j, j + 64, ...
constexpr uint64_t AES_MAX_TILES = 1ull << 28;  // per call
constexpr uint32_t AES_NONCE = 12, AES_TAG = 16, AES_SIZE = 4;  // AesCipher.NONCE_LENGTH, GCM_TAG_LENGTH, SIZE_LENGTH
constexpr uint32_t AES_MAX_KEYS = 256;  // per call: each costs about 26 KB of material at the default tile

inline bool aes_tile_ok(uint32_t tile) {
  return tile >= AES_ROW && tile <= 32768 && (tile & (tile - 1)) == 0;
}

// One (job, tile): `size` ciphertext bytes (the last tile of a job is short, none is empty) from byte
// `src` of d_src, their plaintext to byte `dst` of d_dst; block0 = index of the tile's first block in its
// module (the counter of block i is ctr0 + i).
struct AesTile {
  uint64_t src;
  uint64_t dst;
  uint32_t size;
  uint32_t job;
  uint32_t block0;
  uint32_t reserved;
};
static_assert(sizeof(AesTile) == 32, "AesTile layout");

// One job as the kernels see it.
struct AesJobDev {
  uint64_t tile_begin;   // its tiles are tile_begin .. tile_begin + n_tiles of the tile table
  uint64_t tag_src;      // GCM: byte of d_src where the 16-byte tag starts
  uint64_t nonce_src;    // byte of d_src where the 12-byte nonce starts (the kernels read it there)
  uint32_t n_tiles;
  uint32_t ct_size;      // ciphertext = plaintext bytes
  uint32_t ctr0;         // counter of the first ciphertext block: 2 (GCM) or 1 (CTR)
  uint32_t mode;         // PQG_DECRYPT_GCM / PQG_DECRYPT_CTR
  uint32_t key;          // index into the key material
  uint32_t aad_block0;   // first 16-byte block of the job's zero-padded AAD in the AAD block table
  uint32_t aad_blocks;
  uint32_t aad_length;   // bytes
  uint32_t reserved[2];
};
static_assert(sizeof(AesJobDev) == 64, "AesJobDev layout");

// The material of one key for tile size T (B = T / 16 blocks), as uint32 words in this order:
//   rk[60]     the expanded schedule, big-endian words (4 (rounds + 1) used)
//   rounds     10, 12 or 14; 3 words of padding
//   h64[32][16][4]  "bytes" form: h64[q][n] = (nibble n at nibble position q of a block) * H^64, so a
//              product by H^64 is the XOR of 32 entries (nibble 2 k of byte k is its high half)
//   pw[B + 1][4]    "words" form: H^k, k = 0 .. B (pw[0] = 1)
//   xt[65][4]       "words" form: H^(k B), k = 0 .. 64
constexpr uint32_t AES_KEY_RK = 0, AES_KEY_ROUNDS = 60, AES_KEY_H64 = 64, AES_KEY_PW = AES_KEY_H64 + 32 * 16 * 4;
inline uint32_t aes_key_xt(uint32_t tile) { return AES_KEY_PW + 4 * (tile / 16 + 1); }
inline uint32_t aes_key_words(uint32_t tile) { return aes_key_xt(tile) + 4 * (AES_FOLD_LANES + 1); }

// ---- plain C++ (pqgpu_aes_host.cpp) -----------------------------------------------------------------
const uint8_t* aes_sbox();                       // S[256]
void aes_te0(uint32_t* out /* 256 */);
// FIPS-197 §5.2: rk[4 (rounds + 1)] big-endian words; returns the rounds (0: bad key size)
int aes_expand_key(const uint8_t* key, uint32_t key_size, uint32_t* rk);
void aes_encrypt_block(const uint32_t* rk, int rounds, const uint8_t in[16], uint8_t out[16]);
void gf_mul(const uint8_t x[16], const uint8_t y[16], uint8_t out[16]);  // SP 800-38D algorithm 1, "bytes" form
void aes_build_key(const uint8_t* key, uint32_t key_size, uint32_t tile, uint32_t* out /* aes_key_words(tile) */);

// The host-side refusals of pqg_decrypt_pages; on PQG_OK *n_tiles = entries of the tile table and
// *aad_blocks = 16-byte blocks of the padded AAD table. A refused job is *bad_job (else -1).
int aes_validate(bool have_ctx, const void* d_src, uint64_t n_src, const void* d_dst, uint64_t n_dst,
                 const pqg_decrypt_job* jobs, int n_jobs, const pqg_aes_key* keys, int n_keys, const uint8_t* aad,
                 uint64_t aad_bytes, const void* d_status, uint32_t tile, uint64_t* n_tiles, uint64_t* aad_blocks,
                 int* bad_job);
// The tables of a validated call: jd[n_jobs], tiles[n_tiles] in job order, aad_out[16 * aad_blocks].
void aes_build(const pqg_decrypt_job* jobs, int n_jobs, const uint8_t* aad, uint32_t tile, AesJobDev* jd,
               AesTile* tiles, uint8_t* aad_out);

}  // namespace pqg
