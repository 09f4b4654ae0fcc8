"""The cross-implementation check of the module layout and the AAD: files encrypted by pyarrow (tests/golden/
encrypted_pyarrow_*.parquet, tools/make_encrypted_fixture.py), every page module decrypted with tests/aes_ref.py
under AesCipher.createModuleAAD's AAD, decompressed and decoded by the oracle, against the values pyarrow wrote and,
where pyarrow can read its own file, the values it reads."""
import base64
import os

import numpy as np
import pytest

import encrypted_fixture as ef
from fixtures import decompressed_on_host
from helpers import assert_same
from oracle import pqref
from pqgpu import abi
from tools.synth import writer


@pytest.mark.parametrize("variant", ef.VARIANTS)
def test_modules_decrypt_and_decode(variant):
    entry, raw = ef.load(variant)
    assert [c["name"] for c in entry["columns"]] == ["k", "s"]
    assert [c["physical_type"] for c in entry["columns"]] == [abi.INT64, abi.BYTE_ARRAY]
    assert entry["columns"][0]["pages"][0]["kind"] == "dictionary" and len(bytes.fromhex(entry["file_aad"])) == 8
    for col in entry["columns"]:
        assert col["mode"] == ef.VARIANTS.index(variant) and col["codec"] == writer.SNAPPY
        for pg in col["pages"]:  # the module's own length field
            assert int.from_bytes(raw[pg["offset"]:pg["offset"] + 4], "little") == pg["size"] - 4
        ch = ef.chunk(entry, raw, col, decrypt_on_host=True)
        ref = pqref.decode_batch(writer.build_batch([decompressed_on_host(ch)]))
        assert ref.code == 0, ref.status
        assert_same(ref.columns[0]["values"], ef.expected(col), col["physical_type"])


def test_a_wrong_ordinal_or_key_fails_the_tag():
    import aes_ref
    entry, raw = ef.load("AES_GCM_V1")
    col = entry["columns"][1]
    pg = col["pages"][-1]
    key, file_aad = bytes.fromhex(col["key"]), bytes.fromhex(entry["file_aad"])
    body = raw[pg["offset"]:pg["offset"] + pg["size"]]
    good = aes_ref.module_aad(file_aad, 2, col["row_group"], col["column"], pg["ordinal"])
    assert aes_ref.decrypt_module(key, aes_ref.GCM, body, good) is not None
    for aad in (aes_ref.module_aad(file_aad, 2, col["row_group"], col["column"], pg["ordinal"] + 1),
                aes_ref.module_aad(file_aad, 2, col["row_group"], col["column"] - 1, pg["ordinal"]),
                aes_ref.module_aad(file_aad, 3, col["row_group"], col["column"]), good[1:]):
        assert aes_ref.decrypt_module(key, aes_ref.GCM, body, aad) is None
    assert aes_ref.decrypt_module(bytes.fromhex(entry["columns"][0]["key"]), aes_ref.GCM, body, good) is None


def test_pyarrow_reads_the_same_values():
    """pyarrow's own read of the GCM file (its CTR file names AES_GCM_V1 in the plaintext footer, and pyarrow then
    fails on it itself; the sidecar records that)."""
    pe = pytest.importorskip("pyarrow.parquet.encryption")
    import pyarrow.parquet as pq

    class Kms(pe.KmsClient):
        def __init__(self, config):
            super().__init__()

        def wrap_key(self, key_bytes, master_key_identifier):
            return base64.b64encode(key_bytes)

        def unwrap_key(self, wrapped_key, master_key_identifier):
            return base64.b64decode(wrapped_key)

    entry, _ = ef.load("AES_GCM_V1")
    assert entry["pyarrow_reads_it"] and entry["footer_algorithm"] == "AES_GCM_V1"
    props = pe.CryptoFactory(lambda config: Kms(config)).file_decryption_properties(pe.KmsConnectionConfig(), pe.DecryptionConfiguration())
    table = pq.read_table(os.path.join(ef.GOLDEN, entry["file"]), decryption_properties=props)
    for col in entry["columns"]:
        assert table.column(col["name"]).to_pylist() == col["values"]
    assert np.array_equal(table.column("k").to_numpy(), ef.expected(entry["columns"][0]))
