"""Decoder.upload_chunks on encrypted column chunks, end to end: the chunks the fixtures and the writer build are
encrypted here (tests/aes_ref.py, or the libcrypto it is pinned to), page by page as BlockCipher.Encryptor does,
with AesCipher.createModuleAAD's AADs; upload_chunks + decode then equals the decode of the plain chunks."""
import copy

import numpy as np
import pytest

import aes_ref
import encrypted_fixture as ef
from helpers import assert_same
from pqgpu import abi, crypto, native
from test_crc_host import written_chunks
from test_gpu_crc import codec_chunks
from tools.synth import writer

pytestmark = pytest.mark.gpu
LIB = aes_ref.Libcrypto.load()
FILE_AAD = b"prefix/" + bytes(range(8))


def encrypted(ch, key, mode, row_group, column, rng, file_aad=FILE_AAD):
    """The chunk as a writer with this column key would have written its pages."""
    e = copy.deepcopy(ch)
    e.decryption = crypto.ColumnDecryption(key, file_aad, row_group, column, mode)
    if e.dict_page is not None:
        e.dict_page = aes_ref.encrypt_module(key, mode, rng.bytes(12), ch.dict_page, aes_ref.module_aad(file_aad, 3, row_group, column), LIB)
        e.dict_crc = None
    for k, pg in enumerate(e.pages):
        pg.body = aes_ref.encrypt_module(key, mode, rng.bytes(12), pg.body, aes_ref.module_aad(file_aad, 2, row_group, column, k), LIB)
        pg.crc = None
    return e


def flip(b, at):
    return b[:at] + bytes([b[at] ^ 0x04]) + b[at + 1:]


@pytest.fixture(scope="module")
def picked():
    return codec_chunks()  # every codec, V1 and V2, dictionary pages plain and compressed, nullable columns


@pytest.mark.parametrize("mode", [crypto.GCM, crypto.CTR], ids=["gcm", "ctr"])
def test_every_codec_and_page_version(decoder, picked, mode):
    rng = np.random.default_rng(21 + mode)
    chunks = [ch for ch, _ in picked]
    assert {p.codec for ch in chunks for p in ch.pages} == {writer.UNCOMPRESSED, writer.SNAPPY, writer.ZSTD, writer.GZIP, writer.LZ4_RAW}
    assert {p.version for ch in chunks for p in ch.pages} == {1, 2}
    assert any(p.version == 2 and p.codec and p.rl_byte_length + p.dl_byte_length for ch in chunks for p in ch.pages)
    assert any(ch.dict_codec for ch in chunks) and any(ch.dict_page is not None and not ch.dict_codec for ch in chunks)
    assert any(ch.max_def > 0 for ch in chunks)
    keys = [rng.bytes(16), rng.bytes(24), rng.bytes(32)]
    enc = [encrypted(ch, keys[i % 3], mode, i // 4, i % 4, rng) for i, ch in enumerate(chunks)]
    dbatch = decoder.upload_chunks(enc)
    plain = decoder.upload_chunks(chunks)
    assert np.array_equal(dbatch.bytes.cpu().numpy(), plain.bytes.cpu().numpy())
    cols, st = decoder.decode(dbatch)
    for col, (ch, exp) in zip(cols, picked):
        assert_same(col.numpy(), exp, ch.physical_type)
    # the batch decrypts again from the uploaded modules (what a benchmark re-issues)
    dbatch.bytes.zero_()
    decoder.decrypt_batch(dbatch)
    decoder.decompress(dbatch)
    cols, st = decoder.decode(dbatch)
    for col, (ch, exp) in zip(cols, picked):
        assert_same(col.numpy(), exp, ch.physical_type)


def test_encrypted_and_plain_chunks_in_one_call(decoder, picked):
    rng = np.random.default_rng(23)
    key = rng.bytes(16)
    mixed = [encrypted(ch, key, crypto.GCM if i % 4 else crypto.CTR, 0, i, rng) if i % 2 else ch
             for i, (ch, _) in enumerate(picked)]
    assert any(getattr(c, "decryption", None) is None for c in mixed)
    dbatch = decoder.upload_chunks(mixed)
    plain = decoder.upload_chunks([ch for ch, _ in picked])
    assert np.array_equal(dbatch.bytes.cpu().numpy(), plain.bytes.cpu().numpy())
    cols, st = decoder.decode(dbatch)
    for col, (ch, exp) in zip(cols, picked):
        assert_same(col.numpy(), exp, ch.physical_type)


def test_nullable_dictionary_chunks_and_page_ordinals(decoder):
    """Writer-made nullable dictionary chunks, V1 and V2; the second chunk's pages carry their own ordinals."""
    rng = np.random.default_rng(24)
    v1, v2 = written_chunks()
    key = rng.bytes(32)
    e1 = encrypted(v1, key, crypto.GCM, 2, 0, rng)
    e2 = copy.deepcopy(v2)
    e2.decryption = crypto.ColumnDecryption(key, FILE_AAD, 2, 1, crypto.GCM)
    e2.dict_page = aes_ref.encrypt_module(key, crypto.GCM, rng.bytes(12), v2.dict_page, aes_ref.module_aad(FILE_AAD, 3, 2, 1), LIB)
    for k, pg in enumerate(e2.pages):
        pg.page_ordinal = 100 + k
        pg.body = aes_ref.encrypt_module(key, crypto.GCM, rng.bytes(12), pg.body, aes_ref.module_aad(FILE_AAD, 2, 2, 1, 100 + k), LIB)
    dbatch = decoder.upload_chunks([e1, e2])
    plain = decoder.upload_chunks([v1, v2])
    assert np.array_equal(dbatch.bytes.cpu().numpy(), plain.bytes.cpu().numpy())
    cols, _ = decoder.decode(dbatch)
    want, _ = decoder.decode(plain)
    for a, b in zip(cols, want):
        assert np.array_equal(a.numpy(), b.numpy()) and np.array_equal(a.def_levels.cpu().numpy(), b.def_levels.cpu().numpy())
    # without the ordinals the pages' AADs are those of pages 0, 1, ...: every page fails, the first is named
    for pg in e2.pages:
        del pg.page_ordinal
    with pytest.raises(native.PqgError) as ei:
        decoder.upload_chunks([e1, e2])
    assert ei.value.code == abi.ERR_TAG and "chunk 1, page 0:" in str(ei.value)


def test_tampered_pages_are_named(decoder, picked):
    rng = np.random.default_rng(25)
    key = rng.bytes(16)
    chunks = [ch for ch, _ in picked]
    first = next(i for i, ch in enumerate(chunks) if ch.dict_page is not None and ch.dict_codec)
    later = next(i for i, ch in enumerate(chunks) if i > first and len(ch.pages) > 2 and ch.pages[2].codec)
    sel = [chunks[first], chunks[later]]
    enc = [encrypted(ch, key, crypto.GCM, 0, i, rng) for i, ch in enumerate(sel)]
    decoder.upload_chunks(enc)  # intact
    for at in (16, len(enc[1].pages[2].body) - 17, len(enc[1].pages[2].body) - 1, 5):  # ciphertext, tag, nonce
        bad = copy.deepcopy(enc)
        bad[1].pages[2].body = flip(bad[1].pages[2].body, at)
        with pytest.raises(native.PqgError) as ei:
            decoder.upload_chunks(bad)
        assert ei.value.code == abi.ERR_TAG and "chunk 1, page 2:" in str(ei.value) and "GCM tag check failed" in str(ei.value)
    # a tampered dictionary page is named as one, and comes before a tampered data page of a later chunk
    bad = copy.deepcopy(enc)
    bad[1].pages[2].body = flip(bad[1].pages[2].body, 20)
    bad[0].dict_page = flip(bad[0].dict_page, 30)
    with pytest.raises(native.PqgError) as ei:
        decoder.upload_chunks(bad)
    assert ei.value.code == abi.ERR_TAG and "chunk 0, dictionary page:" in str(ei.value)
    # two pages of a chunk swapped (the descriptions go with the bodies, so the sizes stay consistent; only the
    # ordinals in the AADs no longer fit): both fail, the first is named
    bad = copy.deepcopy(enc)
    bad[1].pages[1], bad[1].pages[2] = bad[1].pages[2], bad[1].pages[1]
    with pytest.raises(native.PqgError) as ei:
        decoder.upload_chunks(bad)
    assert ei.value.code == abi.ERR_TAG and "chunk 1, page 1:" in str(ei.value)
    # the wrong key
    bad = copy.deepcopy(enc)
    bad[0].decryption = crypto.ColumnDecryption(rng.bytes(16), FILE_AAD, 0, 0, crypto.GCM)
    with pytest.raises(native.PqgError) as ei:
        decoder.upload_chunks(bad)
    assert ei.value.code == abi.ERR_TAG and "chunk 0, dictionary page:" in str(ei.value)
    # the decoder works on after the errors
    cols, _ = decoder.decode(decoder.upload_chunks(enc))
    for col, i in zip(cols, (first, later)):
        assert_same(col.numpy(), picked[i][1], chunks[i].physical_type)


def test_refusals(decoder, picked):
    rng = np.random.default_rng(26)
    ch = picked[0][0]
    enc = encrypted(ch, rng.bytes(16), crypto.GCM, 0, 0, rng)
    with pytest.raises(native.PqgError) as ei:
        decoder.upload_chunks([enc], verify_crc=True)
    assert ei.value.code == abi.ERR_UNSUPPORTED
    with pytest.raises(native.PqgError) as ei:
        decoder.upload_chunks([ch, enc], verify_crc=True)
    assert ei.value.code == abi.ERR_UNSUPPORTED
    short = copy.deepcopy(enc)          # "Wrong input length"
    short.pages[0].body = short.pages[0].body[:32]
    with pytest.raises(native.PqgError) as ei:
        decoder.upload_chunks([short])
    assert ei.value.code == abi.ERR_CORRUPT
    zero = copy.deepcopy(enc)           # AesCipher's constructor
    zero.decryption = crypto.ColumnDecryption(bytes(16), FILE_AAD, 0, 0)
    with pytest.raises(native.PqgError) as ei:
        decoder.upload_chunks([zero])
    assert ei.value.code == abi.ERR_INVALID_ARG
    with pytest.raises(native.PqgError):
        crypto.ColumnDecryption(rng.bytes(16), FILE_AAD, 0, 0, mode=7)


@pytest.mark.parametrize("variant", ef.VARIANTS)
def test_pyarrow_encrypted_fixture(decoder, variant):
    """Files another writer encrypted (tests/golden/encrypted_pyarrow_*.parquet): upload_chunks + decode of the
    modules as they sit in the file gives the values pyarrow wrote, and the batch of the host-decrypted pages."""
    entry, raw = ef.load(variant)
    chunks = [ef.chunk(entry, raw, col, decrypt_on_host=False) for col in entry["columns"]]
    dbatch = decoder.upload_chunks(chunks)
    plain = decoder.upload_chunks([ef.chunk(entry, raw, col, decrypt_on_host=True) for col in entry["columns"]])
    assert np.array_equal(dbatch.bytes.cpu().numpy(), plain.bytes.cpu().numpy())
    cols, _ = decoder.decode(dbatch)
    for got, col in zip(cols, entry["columns"]):
        assert_same(got.numpy(), ef.expected(col), col["physical_type"])
