// pqgpu_aes_host.cpp — the host half of pqg_decrypt_pages (include/pqgpu.h, "encrypted pages") in plain
// C++: the refusals, the key schedule, H and its powers, the tile, job and AAD tables (pqgpu_aes.h), and
// the host-only entry point pqg_module_aad. No HIP here: tests/c builds this file with a sanitizer.
#include <cstring>

#include "pqgpu_aes.h"

namespace pqg {

namespace {

uint8_t xtime(uint8_t a) { return (uint8_t)((a << 1) ^ ((a >> 7) * 0x1B)); }

// S[x] = affine(x^-1) over GF(2^8) mod x^8 + x^4 + x^3 + x + 1 (FIPS-197 §5.1.1): p walks the powers of
// the generator 3, q its inverses
struct Sbox {
  uint8_t s[256];
  Sbox() {
    uint8_t p = 1, q = 1;
    do {
      p = (uint8_t)(p ^ xtime(p));  // p *= 3
      q ^= (uint8_t)(q << 1);       // q /= 3
      q ^= (uint8_t)(q << 2);
      q ^= (uint8_t)(q << 4);
      if (q & 0x80) q ^= 0x09;
      auto rotl = [](uint8_t v, int n) { return (uint8_t)((v << n) | (v >> (8 - n))); };
      s[p] = (uint8_t)(q ^ rotl(q, 1) ^ rotl(q, 2) ^ rotl(q, 3) ^ rotl(q, 4) ^ 0x63);
    } while (p != 1);
    s[0] = 0x63;
  }
};
const Sbox& sbox() {
  static const Sbox t;
  return t;
}

uint32_t be32(const uint8_t* p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }
void put_be32(uint8_t* p, uint32_t v) {
  p[0] = (uint8_t)(v >> 24);
  p[1] = (uint8_t)(v >> 16);
  p[2] = (uint8_t)(v >> 8);
  p[3] = (uint8_t)v;
}
uint32_t sub_word(uint32_t w) {
  const uint8_t* s = sbox().s;
  return (uint32_t)s[w >> 24] << 24 | (uint32_t)s[(w >> 16) & 255] << 16 | (uint32_t)s[(w >> 8) & 255] << 8 | s[w & 255];
}
void words_of(const uint8_t b[16], uint32_t* w) {
  for (int i = 0; i < 4; i++) w[i] = be32(b + 4 * i);
}
uint32_t plain_size(const pqg_decrypt_job& J) {
  return J.src_size - AES_SIZE - AES_NONCE - (J.mode == PQG_DECRYPT_GCM ? AES_TAG : 0);
}

}  // namespace

const uint8_t* aes_sbox() { return sbox().s; }

void aes_te0(uint32_t* out) {
  for (int x = 0; x < 256; x++) {
    const uint8_t s = sbox().s[x], s2 = xtime(s);
    out[x] = (uint32_t)s2 << 24 | (uint32_t)s << 16 | (uint32_t)s << 8 | (uint8_t)(s2 ^ s);
  }
}

int aes_expand_key(const uint8_t* key, uint32_t key_size, uint32_t* rk) {
  if (key_size != 16 && key_size != 24 && key_size != 32) return 0;
  const uint32_t nk = key_size / 4;
  const int rounds = (int)nk + 6;
  for (uint32_t i = 0; i < nk; i++) rk[i] = be32(key + 4 * i);
  uint32_t rcon = 1;
  for (uint32_t i = nk; i < 4u * (uint32_t)(rounds + 1); i++) {
    uint32_t t = rk[i - 1];
    if (i % nk == 0) {
      t = sub_word(t << 8 | t >> 24) ^ (rcon << 24);
      rcon = xtime((uint8_t)rcon);
    } else if (nk > 6 && i % nk == 4) {
      t = sub_word(t);
    }
    rk[i] = rk[i - nk] ^ t;
  }
  return rounds;
}

void aes_encrypt_block(const uint32_t* rk, int rounds, const uint8_t in[16], uint8_t out[16]) {
  uint32_t te[256];
  aes_te0(te);
  auto ror = [](uint32_t v, int n) { return v >> n | v << (32 - n); };
  uint32_t s[4], t[4];
  for (int i = 0; i < 4; i++) s[i] = be32(in + 4 * i) ^ rk[i];
  for (int r = 1; r < rounds; r++) {
    for (int i = 0; i < 4; i++)
      t[i] = te[s[i] >> 24] ^ ror(te[(s[(i + 1) & 3] >> 16) & 255], 8) ^ ror(te[(s[(i + 2) & 3] >> 8) & 255], 16) ^
             ror(te[s[(i + 3) & 3] & 255], 24) ^ rk[4 * r + i];
    std::memcpy(s, t, sizeof(s));
  }
  const uint8_t* sb = sbox().s;
  for (int i = 0; i < 4; i++) {
    const uint32_t v = (uint32_t)sb[s[i] >> 24] << 24 | (uint32_t)sb[(s[(i + 1) & 3] >> 16) & 255] << 16 |
                       (uint32_t)sb[(s[(i + 2) & 3] >> 8) & 255] << 8 | sb[s[(i + 3) & 3] & 255];
    put_be32(out + 4 * i, v ^ rk[4 * rounds + i]);
  }
}

void gf_mul(const uint8_t x[16], const uint8_t y[16], uint8_t out[16]) {
  uint32_t z[4] = {0, 0, 0, 0}, v[4];
  words_of(y, v);
  for (int i = 0; i < 128; i++) {
    if ((x[i >> 3] >> (7 - (i & 7))) & 1)
      for (int k = 0; k < 4; k++) z[k] ^= v[k];
    const uint32_t lsb = v[3] & 1u;
    v[3] = v[3] >> 1 | v[2] << 31;
    v[2] = v[2] >> 1 | v[1] << 31;
    v[1] = v[1] >> 1 | v[0] << 31;
    v[0] = (v[0] >> 1) ^ (lsb ? 0xE1000000u : 0u);
  }
  for (int k = 0; k < 4; k++) put_be32(out + 4 * k, z[k]);
}

void aes_build_key(const uint8_t* key, uint32_t key_size, uint32_t tile, uint32_t* out) {
  std::memset(out, 0, sizeof(uint32_t) * aes_key_words(tile));
  const int rounds = aes_expand_key(key, key_size, out + AES_KEY_RK);
  out[AES_KEY_ROUNDS] = (uint32_t)rounds;
  uint8_t zero[16] = {0}, H[16], one[16] = {0x80};
  aes_encrypt_block(out + AES_KEY_RK, rounds, zero, H);
  // pw[k] = H^k
  const uint32_t B = tile / 16;
  uint8_t p[16], h64[16] = {0}, hb[16];
  std::memcpy(p, one, 16);
  for (uint32_t k = 0; k <= B; k++) {
    words_of(p, out + AES_KEY_PW + 4 * k);
    if (k == AES_ROW_BLOCKS) std::memcpy(h64, p, 16);
    if (k == B) std::memcpy(hb, p, 16);
    gf_mul(p, H, p);
  }
  // xt[k] = H^(k B)
  std::memcpy(p, one, 16);
  for (uint32_t k = 0; k <= AES_FOLD_LANES; k++) {
    words_of(p, out + aes_key_xt(tile) + 4 * k);
    gf_mul(p, hb, p);
  }
  // h64[q][n]: basis[i] = x^i * H^64 (the V of algorithm 1), a nibble's entries are sums of four of them
  uint8_t basis[128][16], x1[16] = {0x40};  // x^1
  std::memcpy(basis[0], h64, 16);
  for (int i = 1; i < 128; i++) gf_mul(basis[i - 1], x1, basis[i]);
  uint8_t* tab = (uint8_t*)(out + AES_KEY_H64);
  for (int q = 0; q < 32; q++)
    for (int n = 0; n < 16; n++) {
      uint8_t* e = tab + 16 * (16 * q + n);
      for (int j = 0; j < 4; j++)
        if (n & (8 >> j))
          for (int b = 0; b < 16; b++) e[b] ^= basis[4 * q + j][b];
    }
}

int aes_validate(bool have_ctx, const void* d_src, uint64_t n_src, const void* d_dst, uint64_t n_dst,
                 const pqg_decrypt_job* jobs, int n_jobs, const pqg_aes_key* keys, int n_keys, const uint8_t* aad,
                 uint64_t aad_bytes, const void* d_status, uint32_t tile, uint64_t* n_tiles, uint64_t* aad_blocks,
                 int* bad_job) {
  if (n_tiles) *n_tiles = 0;
  if (aad_blocks) *aad_blocks = 0;
  if (bad_job) *bad_job = -1;
  if (!have_ctx || n_jobs < 0 || !aes_tile_ok(tile) || !n_tiles || !aad_blocks || !bad_job) return PQG_ERR_INVALID_ARG;
  if (n_jobs == 0) return PQG_OK;
  if (!jobs || !d_src || !d_dst || !d_status || !keys || n_keys <= 0 || (uint32_t)n_keys > AES_MAX_KEYS ||
      (aad_bytes && !aad) || ((uintptr_t)d_src & 3u) || ((uintptr_t)d_dst & 3u))
    return PQG_ERR_INVALID_ARG;
  for (int k = 0; k < n_keys; k++) {
    const pqg_aes_key& K = keys[k];
    if (K.size != 16 && K.size != 24 && K.size != 32) return PQG_ERR_INVALID_ARG;
    uint8_t any = 0;
    for (uint32_t i = 0; i < K.size; i++) any |= K.bytes[i];
    if (!any) return PQG_ERR_INVALID_ARG;  // "All key bytes are zero"
  }
  uint64_t total = 0, blocks = 0;
  for (int j = 0; j < n_jobs; j++) {
    const pqg_decrypt_job& J = jobs[j];
    *bad_job = j;
    if (J.reserved || (J.mode != PQG_DECRYPT_GCM && J.mode != PQG_DECRYPT_CTR) || J.key < 0 || J.key >= n_keys)
      return PQG_ERR_INVALID_ARG;
    if (J.src_offset > n_src || J.src_size > n_src - J.src_offset) return PQG_ERR_INVALID_ARG;
    const uint32_t overhead = AES_SIZE + AES_NONCE + (J.mode == PQG_DECRYPT_GCM ? AES_TAG : 0);
    if (J.src_size < overhead + 1) return PQG_ERR_CORRUPT;  // "Wrong input length"
    const uint32_t n = J.src_size - overhead;
    if (J.dst_offset > n_dst || n > n_dst - J.dst_offset) return PQG_ERR_INVALID_ARG;
    if (J.mode == PQG_DECRYPT_GCM) {
      if (J.aad_offset > aad_bytes || J.aad_length > aad_bytes - J.aad_offset) return PQG_ERR_INVALID_ARG;
      blocks += ((uint64_t)J.aad_length + 15) / 16;
    }
    total += ((uint64_t)n + tile - 1) / tile;
  }
  *bad_job = -1;
  if (total > AES_MAX_TILES || blocks > 0xFFFFFFFFull) return PQG_ERR_UNSUPPORTED;
  *n_tiles = total;
  *aad_blocks = blocks;
  return PQG_OK;
}

void aes_build(const pqg_decrypt_job* jobs, int n_jobs, const uint8_t* aad, uint32_t tile, AesJobDev* jd,
               AesTile* tiles, uint8_t* aad_out) {
  uint64_t at = 0;
  uint32_t ab = 0;
  for (int j = 0; j < n_jobs; j++) {
    const pqg_decrypt_job& J = jobs[j];
    const bool gcm = J.mode == PQG_DECRYPT_GCM;
    const uint32_t n = plain_size(J);
    const uint32_t nt = (uint32_t)(((uint64_t)n + tile - 1) / tile);
    const uint64_t ct = J.src_offset + AES_SIZE + AES_NONCE;
    AesJobDev d;
    std::memset(&d, 0, sizeof(d));
    d.tile_begin = at;
    d.tag_src = ct + n;
    d.nonce_src = J.src_offset + AES_SIZE;
    d.n_tiles = nt;
    d.ct_size = n;
    d.ctr0 = gcm ? 2u : 1u;
    d.mode = (uint32_t)J.mode;
    d.key = (uint32_t)J.key;
    if (gcm) {
      d.aad_block0 = ab;
      d.aad_blocks = (J.aad_length + 15) / 16;
      d.aad_length = J.aad_length;
      std::memset(aad_out + 16 * (size_t)ab, 0, 16 * (size_t)d.aad_blocks);
      if (J.aad_length) std::memcpy(aad_out + 16 * (size_t)ab, aad + J.aad_offset, J.aad_length);
      ab += d.aad_blocks;
    }
    jd[j] = d;
    for (uint32_t t = 0; t < nt; t++) {
      const uint64_t lo = (uint64_t)t * tile;
      const uint64_t left = (uint64_t)n - lo;
      tiles[at + t] = AesTile{ct + lo, J.dst_offset + lo, left < tile ? (uint32_t)left : tile, (uint32_t)j,
                              (uint32_t)(lo / 16), 0u};
    }
    at += nt;
  }
}

}  // namespace pqg

extern "C" {

int pqg_module_aad(const uint8_t* file_aad, uint32_t file_aad_length, int module_type, int row_group, int column,
                   int page, uint8_t* out, uint32_t capacity, uint32_t* out_len) {
  if (out_len) *out_len = 0;
  const bool data = module_type == PQG_MODULE_DATA_PAGE;
  if ((!data && module_type != PQG_MODULE_DICTIONARY_PAGE) || !out || !out_len || (file_aad_length && !file_aad) ||
      file_aad_length > 0xFFFFFFF0u)
    return PQG_ERR_INVALID_ARG;
  // "Wrong row group ordinal" / "can't have more than Short.MAX_VALUE row groups", and so on
  if (row_group < 0 || row_group > 32767 || column < 0 || column > 32767 || (data && (page < 0 || page > 32767)))
    return PQG_ERR_INVALID_ARG;
  const uint32_t n = file_aad_length + 1 + 2 + 2 + (data ? 2 : 0);
  *out_len = n;
  if (capacity < n) return PQG_ERR_INVALID_ARG;
  if (file_aad_length) std::memcpy(out, file_aad, file_aad_length);
  uint8_t* p = out + file_aad_length;
  *p++ = (uint8_t)module_type;
  *p++ = (uint8_t)(row_group & 0xFF);
  *p++ = (uint8_t)(row_group >> 8);
  *p++ = (uint8_t)(column & 0xFF);
  *p++ = (uint8_t)(column >> 8);
  if (data) {
    *p++ = (uint8_t)(page & 0xFF);
    *p++ = (uint8_t)(page >> 8);
  }
  return PQG_OK;
}

}  // extern "C"
