"""Write the cross-implementation fixture of the page decryption: small files encrypted by pyarrow (Arrow's C++
Parquet Modular Encryption, not this project's reading of it), one per algorithm, and a JSON sidecar.

    python tools/make_encrypted_fixture.py [--out tests/golden]

Each file holds 300 rows in one row group: an int64 dictionary column `k` and a string column `s`, SNAPPY,
DataPage V1, plaintext footer, both columns under column keys. The KMS is in memory and its wrapping is reversible
(base64), without double wrapping, so the data keys can be read back from the key material in each column's
ColumnCryptoMetaData. The sidecar (encrypted_pyarrow.json) records per file and column: the data key, the file AAD
(aad_prefix || aad_file_unique of the footer's EncryptionAlgorithm), the row-group and column ordinals, the mode of
the page modules, and for every page the offset and size of its module in the file together with the fields of its
page header, which is itself an encrypted module (always GCM; AAD types DataPageHeader = 4, DictionaryPageHeader = 5)
that this tool decrypts with tests/aes_ref.py; and the column's values as pyarrow reads them back."""
import argparse
import base64
import json
import os
import struct
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import aes_ref  # noqa: E402

ROWS = 300
ALGORITHMS = {"AES_GCM_V1": aes_ref.GCM, "AES_GCM_CTR_V1": aes_ref.CTR}


# ---- Thrift compact protocol, read side: a struct becomes {field id: value} ----------------------------------
def _varint(b, p):
    v = s = 0
    while True:
        c = b[p]
        p += 1
        v |= (c & 0x7F) << s
        s += 7
        if not c & 0x80:
            return v, p


def _zz(v):
    return (v >> 1) ^ -(v & 1)


def _value(b, p, t):
    if t in (1, 2):
        return t == 1, p
    if t == 3:
        return b[p], p + 1
    if t in (4, 5, 6):
        v, p = _varint(b, p)
        return _zz(v), p
    if t == 7:
        return struct.unpack("<d", b[p:p + 8])[0], p + 8
    if t == 8:
        n, p = _varint(b, p)
        return bytes(b[p:p + n]), p + n
    if t in (9, 10):
        h = b[p]
        p += 1
        n, et = h >> 4, h & 15
        if n == 15:
            n, p = _varint(b, p)
        out = []
        for _ in range(n):
            if et in (1, 2):
                out.append(b[p] == 1)
                p += 1
            else:
                v, p = _value(b, p, et)
                out.append(v)
        return out, p
    if t == 12:
        return read_struct(b, p)
    raise ValueError(f"thrift type {t}")


def read_struct(b, p=0):
    fields, last = {}, 0
    while True:
        h = b[p]
        p += 1
        if h == 0:
            return fields, p
        if h >> 4:
            fid = last + (h >> 4)
        else:
            v, p = _varint(b, p)
            fid = _zz(v)
        fields[fid], p = _value(b, p, h & 15)
        last = fid


def page_header_fields(h):
    """The PageHeader fields the decoder needs, from a parsed struct."""
    out = {"type": h[1], "uncompressed_page_size": h[2], "compressed_page_size": h[3]}
    if 5 in h:
        d = h[5]
        out.update(version=1, num_values=d[1], encoding=d[2], dl_encoding=d[3], rl_encoding=d[4])
    elif 7 in h:
        out.update(num_values=h[7][1], encoding=h[7][2])
    elif 8 in h:
        d = h[8]
        out.update(version=2, num_values=d[1], num_nulls=d[2], num_rows=d[3], encoding=d[4], dl_byte_length=d[5],
                   rl_byte_length=d[6], is_compressed=d.get(7, True))
    return out


def describe(path, mode, deks, table):
    raw = open(path, "rb").read()
    assert raw[:4] == b"PAR1" and raw[-4:] == b"PAR1", "a plaintext footer"
    footer_len = struct.unpack("<I", raw[-8:-4])[0]
    fmd, _ = read_struct(raw, len(raw) - 8 - footer_len)
    (alg,) = fmd[8].values()           # EncryptionAlgorithm: AesGcmV1 | AesGcmCtrV1
    # (pyarrow 25 names AES_GCM_V1 in a plaintext footer even when it wrote the pages of AES_GCM_CTR_V1, and then
    # cannot read the file back itself: "Failed decryption finalization". The pages are CTR modules all the same,
    # which the walk below shows; the sidecar records what the footer says.)
    footer_says = {1: "AES_GCM_V1", 2: "AES_GCM_CTR_V1"}[next(iter(fmd[8]))]
    file_aad = alg.get(1, b"") + alg[2]  # aad_prefix || aad_file_unique
    assert not alg.get(3, False)
    columns = []
    for rg_ord, rg in enumerate(fmd[4]):
        for col_ord, cc in enumerate(rg[1]):
            material = json.loads(cc[8][2][2])   # ColumnCryptoMetaData.ENCRYPTION_WITH_COLUMN_KEY.key_metadata
            key = base64.b64decode(material["wrappedDEK"])
            assert key in deks, "the KMS saw this data key"
            md = cc[3]                           # the plaintext ColumnMetaData kept for legacy readers
            start = md[11] if 11 in md and md[11] else md[9]
            end, pos, pages, n_data, seen = start + md[7], start, [], 0, 0
            while pos < end and seen < md[5]:
                hsize = 4 + struct.unpack("<I", raw[pos:pos + 4])[0]
                hmod = raw[pos:pos + hsize]
                # the first module of a chunk that has one is its dictionary page header
                for htype in ((5, 4) if not pages else (4,)):
                    aad = file_aad + bytes([htype]) + struct.pack("<hh", rg_ord, col_ord) + (struct.pack("<h", n_data) if htype == 4 else b"")
                    plain = aes_ref.decrypt_module(key, aes_ref.GCM, hmod, aad)
                    if plain is not None:
                        break
                assert plain is not None, "page header tag"
                h = page_header_fields(read_struct(plain)[0])
                size = 4 + struct.unpack("<I", raw[pos + hsize:pos + hsize + 4])[0]
                assert size == h["compressed_page_size"], "compressed_page_size is the module's size"
                kind = "dictionary" if h["type"] == 2 else "data"
                pages.append(dict(h, kind=kind, header_offset=pos, header_size=hsize, offset=pos + hsize, size=size,
                                  ordinal=n_data if kind == "data" else -1))
                if kind == "data":
                    n_data += 1
                    seen += h["num_values"]
                pos += hsize + size
            assert pos == end and seen == md[5]
            name = md[3][-1].decode()
            vals = table.column(name).to_pylist()
            columns.append({"name": name, "physical_type": md[1], "codec": md[4], "max_def": 1, "num_values": md[5],
                            "key": key.hex(), "row_group": rg_ord, "column": col_ord, "mode": mode,
                            "pages": pages, "values": vals})
    return {"file": os.path.basename(path), "file_aad": file_aad.hex(), "footer_algorithm": footer_says, "columns": columns}


def main():
    import pyarrow as pa
    import pyarrow.parquet as pq
    import pyarrow.parquet.encryption as pe

    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    args = ap.parse_args()
    deks = []

    class Kms(pe.KmsClient):
        """In memory; wrapping is base64, so that the sidecar can hold the data keys."""

        def __init__(self, config):
            super().__init__()

        def wrap_key(self, key_bytes, master_key_identifier):
            deks.append(bytes(key_bytes))
            return base64.b64encode(key_bytes)

        def unwrap_key(self, wrapped_key, master_key_identifier):
            return base64.b64decode(wrapped_key)

    rng = np.random.default_rng(20)
    table = pa.table({"k": pa.array(rng.integers(0, 20, ROWS) * 1000003, pa.int64()),
                      "s": pa.array([f"value-{i % 37}-{'x' * (i % 11)}-{i}" for i in range(ROWS)])})
    sidecar = {}
    for alg, mode in ALGORITHMS.items():
        factory = pe.CryptoFactory(lambda config: Kms(config))
        conn = pe.KmsConnectionConfig()
        conf = pe.EncryptionConfiguration(footer_key="footer", column_keys={"columns": ["k", "s"]}, encryption_algorithm=alg,
                                          plaintext_footer=True, double_wrapping=False, internal_key_material=True,
                                          data_key_length_bits=128)
        path = os.path.join(args.out, f"encrypted_pyarrow_{alg.lower()}.parquet")
        with pq.ParquetWriter(path, table.schema, encryption_properties=factory.file_encryption_properties(conn, conf),
                              compression="snappy", use_dictionary=["k"], data_page_size=1024,
                              data_page_version="1.0") as w:
            w.write_table(table)
        entry = describe(path, mode, deks, table)
        try:  # pyarrow's own read of what it wrote
            back = pq.read_table(path, decryption_properties=factory.file_decryption_properties(conn, pe.DecryptionConfiguration()))
            entry["pyarrow_reads_it"] = bool(back.equals(table))
        except OSError as e:
            entry["pyarrow_reads_it"] = False
            entry["pyarrow_read_error"] = str(e)
        sidecar[alg] = entry
        print(alg, os.path.getsize(path), "bytes;", [(c["name"], len(c["pages"])) for c in entry["columns"]],
              "pyarrow reads it:", entry["pyarrow_reads_it"])
    with open(os.path.join(args.out, "encrypted_pyarrow.json"), "w") as f:
        json.dump(sidecar, f, indent=1)


if __name__ == "__main__":
    main()
