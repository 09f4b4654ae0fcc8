"""Loader of the cross-implementation fixture tools/make_encrypted_fixture.py wrote into tests/golden/: files that
pyarrow (Arrow's C++ Parquet Modular Encryption) encrypted, and the sidecar with the data keys, the file AAD, the
ordinals, the page modules' places and their (decrypted) page header fields."""
import json
import os

import numpy as np

import aes_ref
from pqgpu import abi, batch, crypto

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SIDECAR = os.path.join(GOLDEN, "encrypted_pyarrow.json")
VARIANTS = ["AES_GCM_V1", "AES_GCM_CTR_V1"]


def load(variant):
    """-> (sidecar entry, file bytes)"""
    with open(SIDECAR) as f:
        entry = json.load(f)[variant]
    with open(os.path.join(GOLDEN, entry["file"]), "rb") as f:
        return entry, f.read()


def expected(col):
    if col["physical_type"] == abi.BYTE_ARRAY:
        return [v.encode() for v in col["values"]]
    return np.array(col["values"], dtype=np.int64)


def chunk(entry, raw, col, decrypt_on_host):
    """The column chunk as batch.ColumnChunk. decrypt_on_host: the page bodies are decrypted here with tests/aes_ref.py
    (every GCM tag must verify); otherwise they stay encrypted modules and the chunk carries its `decryption`."""
    key, file_aad = bytes.fromhex(col["key"]), bytes.fromhex(entry["file_aad"])
    ch = batch.ColumnChunk(physical_type=col["physical_type"], max_def=col["max_def"], values=expected(col))
    for pg in col["pages"]:
        body = raw[pg["offset"]:pg["offset"] + pg["size"]]
        if decrypt_on_host:
            aad = aes_ref.module_aad(file_aad, 3 if pg["kind"] == "dictionary" else 2, col["row_group"], col["column"], pg["ordinal"])
            body = aes_ref.decrypt_module(key, col["mode"], body, aad)
            assert body is not None, "GCM tag"
        if pg["kind"] == "dictionary":
            ch.dict_page, ch.dict_num_values, ch.dict_encoding = body, pg["num_values"], pg["encoding"]
            ch.dict_codec, ch.dict_uncompressed_size = col["codec"], pg["uncompressed_page_size"]
        else:
            assert pg["version"] == 1
            ch.pages.append(batch.Page(body=body, num_values=pg["num_values"], encoding=pg["encoding"], version=1,
                                       rl_encoding=pg["rl_encoding"], dl_encoding=pg["dl_encoding"], codec=col["codec"],
                                       uncompressed_size=pg["uncompressed_page_size"]))
    if not decrypt_on_host:
        ch.decryption = crypto.ColumnDecryption(key, file_aad, col["row_group"], col["column"], col["mode"])
    return ch
