"""AES-128/192/256 with GCM and CTR in plain Python, written from FIPS-197 and SP 800-38D: the expectation of
the decryption tests (tests/test_aes_ref.py pins it to the GCM specification's test cases and to the local
libcrypto). Also the Parquet module framing of BlockCipher.Encryptor (AesGcmEncryptor / AesCtrEncryptor):
[4-byte LE length][12-byte nonce][ciphertext][16-byte tag, GCM only], and the same through libcrypto (ctypes)
for large inputs."""
import ctypes
import ctypes.util
import struct

GCM, CTR = 0, 1
NONCE_LENGTH, GCM_TAG_LENGTH, SIZE_LENGTH = 12, 16, 4


# ---- FIPS-197 ---------------------------------------------------------------------------------------------
def _xtime(a):
    return ((a << 1) ^ 0x1B) & 0xFF if a & 0x80 else a << 1


def _gmul(a, b):
    p = 0
    while b:
        if b & 1:
            p ^= a
        a = _xtime(a)
        b >>= 1
    return p


def _make_sbox():
    # the multiplicative inverse in GF(2^8), then the affine transformation of §5.1.1
    inv = [0] * 256
    for a in range(1, 256):
        for b in range(1, 256):
            if _gmul(a, b) == 1:
                inv[a] = b
                break
    box = []
    for a in range(256):
        b = inv[a]
        s = 0
        for i in range(8):
            bit = ((b >> i) ^ (b >> ((i + 4) % 8)) ^ (b >> ((i + 5) % 8)) ^ (b >> ((i + 6) % 8)) ^ (b >> ((i + 7) % 8)) ^
                   (0x63 >> i)) & 1
            s |= bit << i
        box.append(s)
    return box


SBOX = _make_sbox()
assert SBOX[0] == 0x63 and SBOX[0x53] == 0xED  # FIPS-197 §5.1.1's example
_MUL2 = [_xtime(a) for a in range(256)]
_MUL3 = [_xtime(a) ^ a for a in range(256)]


def expand_key(key):
    """KeyExpansion (§5.2): the list of 4 (Nr + 1) words as 4-byte lists."""
    nk = len(key) // 4
    assert len(key) in (16, 24, 32)
    nr = nk + 6
    w = [list(key[4 * i:4 * i + 4]) for i in range(nk)]
    rcon = 1
    for i in range(nk, 4 * (nr + 1)):
        t = list(w[i - 1])
        if i % nk == 0:
            t = [SBOX[b] for b in t[1:] + t[:1]]
            t[0] ^= rcon
            rcon = _xtime(rcon)
        elif nk > 6 and i % nk == 4:
            t = [SBOX[b] for b in t]
        w.append([a ^ b for a, b in zip(w[i - nk], t)])
    return w


def round_key_words(key):
    """The schedule as big-endian 32-bit words."""
    return [int.from_bytes(bytes(x), "big") for x in expand_key(key)]


def encrypt_block(w, block):
    """Cipher (§5.1) with the expanded key w; the state is column-major: s[4 c + r]."""
    nr = len(w) // 4 - 1
    s = [block[i] ^ w[i // 4][i % 4] for i in range(16)]
    for rnd in range(1, nr + 1):
        s = [SBOX[b] for b in s]
        s = [s[4 * ((c + r) % 4) + r] for c in range(4) for r in range(4)]  # ShiftRows
        if rnd < nr:
            m = []
            for c in range(4):
                a = s[4 * c:4 * c + 4]
                m += [_MUL2[a[0]] ^ _MUL3[a[1]] ^ a[2] ^ a[3], a[0] ^ _MUL2[a[1]] ^ _MUL3[a[2]] ^ a[3],
                      a[0] ^ a[1] ^ _MUL2[a[2]] ^ _MUL3[a[3]], _MUL3[a[0]] ^ a[1] ^ a[2] ^ _MUL2[a[3]]]
            s = m
        s = [s[i] ^ w[4 * rnd + i // 4][i % 4] for i in range(16)]
    return bytes(s)


# ---- SP 800-38D -------------------------------------------------------------------------------------------
_R = 0xE1 << 120


def gf_mul(x, y):
    """Algorithm 1 on blocks as integers (bit 0 of the block = the integer's bit 127)."""
    z, v = 0, y
    for i in range(128):
        if (x >> (127 - i)) & 1:
            z ^= v
        v = (v >> 1) ^ _R if v & 1 else v >> 1
    return z


def gf_pow(h, k):
    p = 1 << 127
    for _ in range(k):
        p = gf_mul(p, h)
    return p


def ghash(h, data):
    if len(data) > _BULK:
        return _ghash_bulk(h, data)
    y = 0
    for i in range(0, len(data), 16):
        y = gf_mul(y ^ int.from_bytes(data[i:i + 16], "big"), h)
    return y


# Inputs above _BULK bytes (the tests' 1 MiB modules) take two faster forms of the same definitions, which
# tests/test_aes_ref.py compares with the plain ones: GHASH with a table of (byte b at byte position i) * H,
# and the keystream with the Cipher's steps applied to all counter blocks at once (numpy).
_BULK = 8192


def _ghash_bulk(h, data):
    v, basis = h, []
    for _ in range(128):  # basis[p] = H * x^p, the V of algorithm 1
        basis.append(v)
        v = (v >> 1) ^ _R if v & 1 else v >> 1
    tab = []
    for i in range(16):
        row = [0] * 256
        for b in range(1, 256):
            low = b & -b
            row[b] = row[b ^ low] ^ basis[8 * i + 7 - (low.bit_length() - 1)]
        tab.append(row)
    y = 0
    for i in range(0, len(data), 16):
        x = (y ^ int.from_bytes(data[i:i + 16], "big")).to_bytes(16, "big")
        y = 0
        for k in range(16):
            y ^= tab[k][x[k]]
    return y


def _ctr_stream_bulk(w, icb, n):
    import numpy as np
    nb = (n + 15) // 16
    nr = len(w) // 4 - 1
    sb, m2, m3 = (np.array(t, dtype=np.uint8) for t in (SBOX, _MUL2, _MUL3))
    rk = np.array([b for word in w for b in word], dtype=np.uint8).reshape(nr + 1, 16)
    shift = [4 * ((c + r) % 4) + r for c in range(4) for r in range(4)]
    s = np.empty((nb, 16), dtype=np.uint8)
    s[:, :12] = np.frombuffer(icb[:12], dtype=np.uint8)
    ctr = (int.from_bytes(icb[12:], "big") + np.arange(nb, dtype=np.uint64)) & 0xFFFFFFFF
    for k in range(4):
        s[:, 12 + k] = (ctr >> np.uint64(8 * (3 - k))).astype(np.uint8)
    s ^= rk[0]
    for rnd in range(1, nr + 1):
        s = sb[s][:, shift]
        if rnd < nr:
            a = s.reshape(nb, 4, 4)
            a0, a1, a2, a3 = a[:, :, 0], a[:, :, 1], a[:, :, 2], a[:, :, 3]
            s = np.stack([m2[a0] ^ m3[a1] ^ a2 ^ a3, a0 ^ m2[a1] ^ m3[a2] ^ a3, a0 ^ a1 ^ m2[a2] ^ m3[a3],
                          m3[a0] ^ a1 ^ a2 ^ m2[a3]], axis=2).reshape(nb, 16)
        s = s ^ rk[rnd]
    return s.tobytes()[:n]


def _xor(a, b):
    if len(a) > _BULK:
        import numpy as np
        return (np.frombuffer(a, dtype=np.uint8) ^ np.frombuffer(b, dtype=np.uint8)).tobytes()
    return bytes(x ^ y for x, y in zip(a, b))


def _ctr_stream(w, icb, n):
    if n > _BULK:
        return _ctr_stream_bulk(w, icb, n)
    out = bytearray()
    head, ctr = icb[:12], int.from_bytes(icb[12:], "big")
    while len(out) < n:
        out += encrypt_block(w, head + struct.pack(">I", ctr & 0xFFFFFFFF))
        ctr += 1
    return bytes(out[:n])


def _pad16(b):
    return b + bytes((-len(b)) % 16)


def hash_subkey(key):
    return int.from_bytes(encrypt_block(expand_key(key), bytes(16)), "big")


def gcm_encrypt(key, iv, plaintext, aad=b""):
    """GCM-AE_K(IV, P, A) with a 96-bit IV and a 128-bit tag -> (ciphertext, tag)."""
    assert len(iv) == 12
    w = expand_key(key)
    h = int.from_bytes(encrypt_block(w, bytes(16)), "big")
    c = _xor(plaintext, _ctr_stream(w, iv + b"\0\0\0\2", len(plaintext)))
    s = ghash(h, _pad16(aad) + _pad16(c) + struct.pack(">QQ", 8 * len(aad), 8 * len(c)))
    tag = s ^ int.from_bytes(encrypt_block(w, iv + b"\0\0\0\1"), "big")
    return c, tag.to_bytes(16, "big")


def gcm_decrypt(key, iv, ciphertext, tag, aad=b""):
    """GCM-AD: the plaintext, or None when the tag does not verify."""
    w = expand_key(key)
    h = int.from_bytes(encrypt_block(w, bytes(16)), "big")
    s = ghash(h, _pad16(aad) + _pad16(ciphertext) + struct.pack(">QQ", 8 * len(aad), 8 * len(ciphertext)))
    if (s ^ int.from_bytes(encrypt_block(w, iv + b"\0\0\0\1"), "big")).to_bytes(16, "big") != bytes(tag):
        return None
    return _xor(ciphertext, _ctr_stream(w, iv + b"\0\0\0\2", len(ciphertext)))


def ctr_crypt(key, nonce, data):
    """AesCtrEncryptor / AesCtrDecryptor: AES/CTR/NoPadding with the IV nonce || 00000001."""
    return _xor(data, _ctr_stream(expand_key(key), nonce + b"\0\0\0\1", len(data)))


# ---- the module framing of BlockCipher.Encryptor -------------------------------------------------------------
def encrypt_module(key, mode, nonce, plaintext, aad=b"", backend=None):
    """[length][nonce][ciphertext][tag]: what AesGcmEncryptor / AesCtrEncryptor.encrypt(true, ...) write.
    backend: None = this file, or a Libcrypto."""
    impl = backend or _Self
    if mode == GCM:
        c, tag = impl.gcm_encrypt(key, nonce, plaintext, aad)
        body = nonce + c + tag
    else:
        body = nonce + impl.ctr_crypt(key, nonce, plaintext)
    return struct.pack("<I", len(body)) + body


def decrypt_module(key, mode, module, aad=b""):
    """AesGcmDecryptor / AesCtrDecryptor.decrypt(lengthAndCiphertext, AAD): the plaintext, None for a tag mismatch."""
    nonce = module[SIZE_LENGTH:SIZE_LENGTH + NONCE_LENGTH]
    body = module[SIZE_LENGTH + NONCE_LENGTH:]
    if mode == GCM:
        assert len(body) > GCM_TAG_LENGTH, "Wrong input length"
        return gcm_decrypt(key, nonce, body[:-GCM_TAG_LENGTH], body[-GCM_TAG_LENGTH:], aad)
    assert len(body) >= 1, "Wrong input length"
    return ctr_crypt(key, nonce, body)


def module_aad(file_aad, module_type, row_group, column, page=-1):
    """AesCipher.createModuleAAD for DataPage (2) and DictionaryPage (3)."""
    for v in (row_group, column) + ((page,) if module_type == 2 else ()):
        if v < 0 or v > 32767:
            raise ValueError("ordinal")
    out = bytes(file_aad) + bytes([module_type]) + struct.pack("<hh", row_group, column)
    return out + struct.pack("<h", page) if module_type == 2 else out


class _Self:
    gcm_encrypt = staticmethod(gcm_encrypt)
    ctr_crypt = staticmethod(ctr_crypt)


# ---- the local libcrypto (EVP), for large inputs and as a second opinion ---------------------------------
class Libcrypto:
    """EVP_aes_{128,192,256}_{gcm,ctr} through ctypes. Libcrypto.load() returns None when there is no library."""

    _GET_TAG, _SET_IVLEN = 0x10, 0x9

    @classmethod
    def load(cls):
        name = ctypes.util.find_library("crypto")
        if not name:
            return None
        try:
            lib = ctypes.CDLL(name)
            lib.EVP_CIPHER_CTX_new.restype = ctypes.c_void_p
            for f in ("EVP_aes_128_gcm", "EVP_aes_192_gcm", "EVP_aes_256_gcm", "EVP_aes_128_ctr", "EVP_aes_192_ctr",
                      "EVP_aes_256_ctr"):
                getattr(lib, f).restype = ctypes.c_void_p
        except (OSError, AttributeError):
            return None
        self = cls()
        self.lib = lib
        return self

    def _run(self, kind, key, iv, data, aad=None):
        lib, vp = self.lib, ctypes.c_void_p
        ctx = vp(lib.EVP_CIPHER_CTX_new())
        try:
            cipher = vp(getattr(lib, f"EVP_aes_{8 * len(key)}_{kind}")())
            assert lib.EVP_EncryptInit_ex(ctx, cipher, None, None, None) == 1
            if kind == "gcm":
                assert lib.EVP_CIPHER_CTX_ctrl(ctx, self._SET_IVLEN, len(iv), None) == 1
            assert lib.EVP_EncryptInit_ex(ctx, None, None, bytes(key), bytes(iv)) == 1
            n = ctypes.c_int()
            if aad:
                assert lib.EVP_EncryptUpdate(ctx, None, ctypes.byref(n), bytes(aad), len(aad)) == 1
            out = ctypes.create_string_buffer(len(data) + 16)
            assert lib.EVP_EncryptUpdate(ctx, out, ctypes.byref(n), bytes(data), len(data)) == 1
            got = n.value
            assert lib.EVP_EncryptFinal_ex(ctx, ctypes.byref(out, got), ctypes.byref(n)) == 1
            got += n.value
            tag = None
            if kind == "gcm":
                t = ctypes.create_string_buffer(16)
                assert lib.EVP_CIPHER_CTX_ctrl(ctx, self._GET_TAG, 16, t) == 1
                tag = t.raw
            return out.raw[:got], tag
        finally:
            lib.EVP_CIPHER_CTX_free(ctx)

    def gcm_encrypt(self, key, iv, plaintext, aad=b""):
        return self._run("gcm", key, iv, plaintext, aad)

    def ctr_crypt(self, key, nonce, data):
        return self._run("ctr", key, nonce + b"\0\0\0\1", data)[0]
