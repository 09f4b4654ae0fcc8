"""C ABI of the page decryption (include/pqgpu.h, additions to ABI 6): the struct sizes (40, 36) and field offsets
of the ctypes mirrors match a compiled C snippet, PQG_ERR_TAG is 22 with its name and its Java exception, the
constants are the header's, the version is still 6, libpqgpu.so exports the new functions and they refuse a NULL ctx."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from pqgpu import abi, native

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LAYOUT_C = r"""
#include <stdio.h>
#include <stddef.h>
#include "pqgpu.h"
#define S(s) printf("%s %zu\n", #s, sizeof(s))
#define O(s, f) printf("%s.%s %zu\n", #s, #f, offsetof(s, f))
#define V(v) printf("%s %d\n", #v, (int)(v))
int main(void) {
  S(pqg_decrypt_job); S(pqg_aes_key); S(pqg_crc_job); S(pqg_status); S(pqg_copy_range);
  O(pqg_decrypt_job, src_offset); O(pqg_decrypt_job, dst_offset); O(pqg_decrypt_job, src_size);
  O(pqg_decrypt_job, aad_offset); O(pqg_decrypt_job, aad_length); O(pqg_decrypt_job, mode); O(pqg_decrypt_job, key);
  O(pqg_decrypt_job, reserved); O(pqg_aes_key, bytes); O(pqg_aes_key, size);
  V(PQG_ERR_TAG); V(PQG_ERR_CRC); V(PQG_DISPATCH_AES_TILE_BYTES); V(PQG_DISPATCH_CRC_TILE_BYTES); V(PQG_AES_TILE_BYTES);
  V(PQG_DECRYPT_GCM); V(PQG_DECRYPT_CTR); V(PQG_MODULE_DATA_PAGE); V(PQG_MODULE_DICTIONARY_PAGE); V(PQG_ABI_VERSION);
  return 0;
}
"""
MIRRORS = {"pqg_decrypt_job": abi.DecryptJob, "pqg_aes_key": abi.AesKey}


def test_ctypes_layout_matches_c(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(LAYOUT_C)
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.rsplit(" ", 1) for line in subprocess.run([str(exe)], capture_output=True, text=True).stdout.splitlines())
    n_fields = 0
    for k, v in got.items():
        if "." in k:
            s, f = k.split(".")
            assert getattr(MIRRORS[s], f).offset == int(v), k
            dt = {"pqg_decrypt_job": abi.DECRYPT_JOB_DTYPE, "pqg_aes_key": abi.AES_KEY_DTYPE}[s]
            assert dt.fields[f][1] == int(v), k
            n_fields += 1
        elif k in MIRRORS:
            assert C.sizeof(MIRRORS[k]) == int(v), k
    assert n_fields == sum(len(m._fields_) for m in MIRRORS.values())
    assert (int(got["pqg_decrypt_job"]), int(got["pqg_aes_key"])) == (40, 36)
    assert int(got["pqg_copy_range"]) == abi.COPY_RANGE_DTYPE.itemsize == 24
    assert (int(got["pqg_crc_job"]), int(got["pqg_status"])) == (24, 256)  # nothing existing grew
    assert int(got["PQG_ERR_TAG"]) == abi.ERR_TAG == 22 and int(got["PQG_ERR_CRC"]) == 21
    assert int(got["PQG_DISPATCH_AES_TILE_BYTES"]) == abi.DISPATCH_AES_TILE_BYTES == 9
    assert int(got["PQG_DISPATCH_CRC_TILE_BYTES"]) == 8
    assert int(got["PQG_AES_TILE_BYTES"]) == abi.AES_TILE_BYTES
    assert (int(got["PQG_DECRYPT_GCM"]), int(got["PQG_DECRYPT_CTR"])) == (abi.DECRYPT_GCM, abi.DECRYPT_CTR)
    assert (int(got["PQG_MODULE_DATA_PAGE"]), int(got["PQG_MODULE_DICTIONARY_PAGE"])) == (2, 3)
    assert (abi.MODULE_DATA_PAGE, abi.MODULE_DICTIONARY_PAGE) == (2, 3)
    assert int(got["PQG_ABI_VERSION"]) == abi.ABI_VERSION == 6


def test_new_functions_are_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], capture_output=True, text=True).stdout
    defined = set(re.findall(r"\bT (pqg_\w+)", out))
    for name in ("pqg_decrypt_pages", "pqg_decrypt_sync", "pqg_module_aad", "pqg_copy_ranges"):
        assert name in defined and name in native.EXPORTS and hasattr(native.lib(), name)


def test_tag_error_name_and_exception():
    L = native.lib()
    assert L.pqg_error_name(abi.ERR_TAG).decode() == "TAG" == abi.ERROR_NAMES[abi.ERR_TAG]
    L.pqg_java_exception.restype = C.c_char_p
    L.pqg_java_exception.argtypes = [C.c_int]
    assert L.pqg_java_exception(abi.ERR_TAG).decode() == "org/apache/parquet/crypto/TagVerificationException"
    assert L.pqg_java_exception(abi.ERR_CRC).decode() == "org/apache/parquet/io/ParquetDecodingException"


def test_null_arguments_are_refused():
    L = native.lib()
    st = abi.Status()
    job = np.zeros(1, dtype=abi.DECRYPT_JOB_DTYPE)
    job["src_size"] = 33
    key = np.zeros(1, dtype=abi.AES_KEY_DTYPE)
    key["size"], key["bytes"][0, 0] = 16, 1
    word = (C.c_uint32 * 16)()
    assert L.pqg_decrypt_pages(None, word, 64, word, 64, job.ctypes.data, 1, key.ctypes.data, 1, None, 0, word,
                               C.byref(st)) == abi.ERR_INVALID_ARG
    assert st.code == abi.ERR_INVALID_ARG
    assert L.pqg_decrypt_pages(None, None, 0, None, 0, None, 0, None, 0, None, 0, None, None) == abi.ERR_INVALID_ARG
    assert L.pqg_decrypt_sync(None, None, 0, C.byref(st)) == abi.ERR_INVALID_ARG
    assert L.pqg_copy_ranges(None, word, 64, word, 64, word, 1) == abi.ERR_INVALID_ARG
    n = C.c_uint32()
    assert L.pqg_module_aad(None, 0, abi.MODULE_DATA_PAGE, 0, 0, 0, None, 0, C.byref(n)) == abi.ERR_INVALID_ARG
