"""tests/aes_ref.py (the expectation of the decryption tests) pinned to the GCM specification's test cases
(McGrew & Viega, "The Galois/Counter Mode of Operation", appendix B: cases 1-4 for 128-bit keys, 13-16 for 256-bit
keys, 7-8 for 192-bit keys) and to the local libcrypto on random modules of the sizes the device tests use;
pqgpu.crypto.module_aad against AesCipher.createModuleAAD's rules."""
import numpy as np
import pytest

import aes_ref
from pqgpu import abi, crypto, native

K3 = "feffe9928665731c6d6a8f9467308308"
P3 = ("d9313225f88406e5a55909c5aff5269a86a7a9531534f7da2e4c303d8a318a721c3c0c95956809532fcf0e2449a6b525"
      "b16aedf5aa0de657ba637b391aafd255")
IV3 = "cafebabefacedbaddecaf888"
A4 = "feedfacedeadbeeffeedfacedeadbeefabaddad2"
C3 = ("42831ec2217774244b7221b784d0d49ce3aa212f2c02a4e035c17e2329aca12e21d514b25466931c7d8f6a5aac84aa05"
      "1ba30b396a0aac973d58e091473f5985")
C15 = ("522dc1f099567d07f47f37a32a84427d643a8cdcbfe5c0c97598a2bd2555d1aa8cb08e48590dbb3da7b08b1056828838"
       "c5f61e6393ba7a0abcc9f662898015ad")
# (case, key, iv, plaintext, aad, ciphertext, tag)
VECTORS = [
    (1, "00" * 16, "00" * 12, "", "", "", "58e2fccefa7e3061367f1d57a4e7455a"),
    (2, "00" * 16, "00" * 12, "00" * 16, "", "0388dace60b6a392f328c2b971b2fe78", "ab6e47d42cec13bdf53a67b21257bddf"),
    (3, K3, IV3, P3, "", C3, "4d5c2af327cd64a62cf35abd2ba6fab4"),
    (4, K3, IV3, P3[:120], A4, C3[:120], "5bc94fbc3221a5db94fae95ae7121a47"),
    (7, "00" * 24, "00" * 12, "", "", "", "cd33b28ac773f74ba00ed1f312572435"),
    (8, "00" * 24, "00" * 12, "00" * 16, "", "98e7247c07f0fe411c267e4384b0f600", "2ff58d80033927ab8ef4d4587514f0fb"),
    (13, "00" * 32, "00" * 12, "", "", "", "530f8afbc74536b9a963b4f1c4cb738b"),
    (14, "00" * 32, "00" * 12, "00" * 16, "", "cea7403d4d606b6e074ec5d3baf39d18", "d0d1c8a799996bf0265b98b5d48ab919"),
    (15, K3 * 2, IV3, P3, "", C15, "b094dac5d93471bdec1a502270e3cc6c"),
    (16, K3 * 2, IV3, P3[:120], A4, C15[:120], "76fc6ece0f4e1768cddf8853bb2d551b"),
]

TILE = 1024  # the tile the device tests force
SIZES = [1, 15, 16, 17, 31, 32, 33, TILE - 1, TILE, TILE + 1, 2 * TILE + 5, 4096 + 1]
LIB = aes_ref.Libcrypto.load()


@pytest.mark.parametrize("case", VECTORS, ids=lambda c: f"case{c[0]}")
def test_gcm_specification_vectors(case):
    _, key, iv, p, a, c, t = (bytes.fromhex(x) if isinstance(x, str) else x for x in case)
    got_c, got_t = aes_ref.gcm_encrypt(key, iv, p, a)
    assert got_c.hex() == c.hex() and got_t.hex() == t.hex()
    assert aes_ref.gcm_decrypt(key, iv, c, t, a) == p
    if c:
        flipped = bytes([c[0] ^ 1]) + c[1:]
        assert aes_ref.gcm_decrypt(key, iv, flipped, t, a) is None
    assert aes_ref.gcm_decrypt(key, iv, c, bytes([t[0] ^ 0x80]) + t[1:], a) is None


def test_fips197_appendix_c_blocks():
    pt = bytes.fromhex("00112233445566778899aabbccddeeff")
    for n, want in ((16, "69c4e0d86a7b0430d8cdb78070b4c55a"), (24, "dda97ca4864cdfe06eaf70a0ec0d7191"),
                    (32, "8ea2b7ca516745bfeafc49904b496089")):
        assert aes_ref.encrypt_block(aes_ref.expand_key(bytes(range(n))), pt).hex() == want


@pytest.mark.skipif(LIB is None, reason="no libcrypto on this machine")
@pytest.mark.parametrize("key_size", [16, 24, 32])
def test_against_libcrypto(key_size):
    rng = np.random.default_rng(key_size)
    for mode in (aes_ref.GCM, aes_ref.CTR):
        for n in SIZES:
            key, nonce = rng.bytes(key_size), rng.bytes(12)
            aad = rng.bytes(int(rng.choice([13, 15, 16, 17, 31, 32, 200])))
            p = rng.bytes(n)
            mine = aes_ref.encrypt_module(key, mode, nonce, p, aad)
            assert mine == aes_ref.encrypt_module(key, mode, nonce, p, aad, backend=LIB), (mode, n)
            assert aes_ref.decrypt_module(key, mode, mine, aad) == p
            assert len(mine) == n + 16 + (16 if mode == aes_ref.GCM else 0)
            assert int.from_bytes(mine[:4], "little") == len(mine) - 4


@pytest.mark.skipif(LIB is None, reason="no libcrypto on this machine")
def test_against_libcrypto_one_mebibyte():
    """1 MiB + 17: the counter's third byte carries."""
    rng = np.random.default_rng(5)
    key, nonce, aad, p = rng.bytes(16), rng.bytes(12), rng.bytes(15), rng.bytes((1 << 20) + 17)
    assert aes_ref.encrypt_module(key, aes_ref.GCM, nonce, p, aad) == aes_ref.encrypt_module(key, aes_ref.GCM, nonce, p, aad, LIB)


def test_bulk_forms_equal_the_plain_ones(monkeypatch):
    """The table GHASH and the numpy keystream that inputs above aes_ref._BULK take, against the plain definitions."""
    rng = np.random.default_rng(9)
    for key_size in (16, 24, 32):
        key, nonce, aad, p = rng.bytes(key_size), rng.bytes(12), rng.bytes(17), rng.bytes(aes_ref._BULK + 21)
        fast = aes_ref.encrypt_module(key, aes_ref.GCM, nonce, p, aad), aes_ref.encrypt_module(key, aes_ref.CTR, nonce, p)
        with monkeypatch.context() as m:
            m.setattr(aes_ref, "_BULK", 1 << 30)
            assert fast == (aes_ref.encrypt_module(key, aes_ref.GCM, nonce, p, aad), aes_ref.encrypt_module(key, aes_ref.CTR, nonce, p))
        assert aes_ref.decrypt_module(key, aes_ref.GCM, fast[0], aad) == p and aes_ref.decrypt_module(key, aes_ref.CTR, fast[1]) == p


def test_libcrypto_gives_case_2():
    if LIB is None:
        pytest.skip("no libcrypto on this machine")
    c, t = LIB.gcm_encrypt(bytes(16), bytes(12), bytes(16))
    assert (c.hex(), t.hex()) == ("0388dace60b6a392f328c2b971b2fe78", "ab6e47d42cec13bdf53a67b21257bddf")


# ---- AesCipher.createModuleAAD ---------------------------------------------------------------------------
def test_module_aad_lengths_and_layout():
    unique = bytes(range(1, 9))  # AAD_FILE_UNIQUE_LENGTH = 8
    d = crypto.module_aad(unique, crypto.DICTIONARY_PAGE, 3, 0x0102)
    p = crypto.module_aad(unique, crypto.DATA_PAGE, 3, 0x0102, 0x0405)
    assert len(d) == 13 and len(p) == 15
    assert d == unique + bytes([3, 3, 0, 2, 1]) and p == unique + bytes([2, 3, 0, 2, 1, 5, 4])
    prefix = b"table-7/"
    assert crypto.module_aad(prefix + unique, crypto.DATA_PAGE, 32767, 0, 32767) == prefix + unique + bytes([2, 255, 127, 0, 0, 255, 127])
    assert len(crypto.module_aad(prefix + unique, crypto.DICTIONARY_PAGE, 0, 0)) == len(prefix) + 13
    assert crypto.module_aad(b"", crypto.DICTIONARY_PAGE, 1, 2, 99) == bytes([3, 1, 0, 2, 0])  # the page ordinal is ignored
    for args in ((unique, crypto.DATA_PAGE, 3, 4, 5), (prefix + unique, crypto.DICTIONARY_PAGE, 7, 8)):
        assert crypto.module_aad(*args) == aes_ref.module_aad(*args)


@pytest.mark.parametrize("args", [(crypto.DATA_PAGE, 32768, 0, 0), (crypto.DATA_PAGE, 0, 32768, 0), (crypto.DATA_PAGE, 0, 0, 32768),
                                  (crypto.DATA_PAGE, -1, 0, 0), (crypto.DATA_PAGE, 0, -1, 0), (crypto.DATA_PAGE, 0, 0, -1),
                                  (crypto.DICTIONARY_PAGE, 40000, 0, 0), (0, 0, 0, 0), (4, 0, 0, 0)])
def test_module_aad_refusals(args):
    with pytest.raises(native.PqgError) as e:
        crypto.module_aad(b"12345678", *args)
    assert e.value.code == abi.ERR_INVALID_ARG
