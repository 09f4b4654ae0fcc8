"""C ABI of the record filter on dictionary ids (include/pqgpu.h, additions to ABI 6): the ctypes mirror
of pqg_filter_dictionary matches the C layout, the LDS budget is the header's, the version is still 6,
libpqgpu.so exports the two new functions and both refuse a NULL ctx. No compute calls here."""
import ctypes as C
import os
import re
import subprocess

from pqgpu import abi, native

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LAYOUT_C = r"""
#include <stdio.h>
#include <stddef.h>
#include "pqgpu.h"
#define S(s) printf("%s %zu\n", #s, sizeof(s))
#define O(s, f) printf("%s.%s %zu\n", #s, #f, offsetof(s, f))
int main(void) {
  S(pqg_filter_dictionary); S(pqg_filter_column);
  O(pqg_filter_dictionary, values); O(pqg_filter_dictionary, binary_data);
  O(pqg_filter_dictionary, n_entries); O(pqg_filter_dictionary, reserved);
  printf("PQG_FILTER_DICT_LDS_BYTES %d\nPQG_ABI_VERSION %d\n", PQG_FILTER_DICT_LDS_BYTES, PQG_ABI_VERSION);
  return 0;
}
"""
MIRRORS = {"pqg_filter_dictionary": abi.FilterDictionary, "pqg_filter_column": abi.FilterColumn}


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
            n_fields += 1
        elif k in MIRRORS:
            assert C.sizeof(MIRRORS[k]) == int(v), k
    assert n_fields == len(abi.FilterDictionary._fields_)  # every field of the new mirror was probed
    assert int(got["pqg_filter_dictionary"]) == 24 and int(got["pqg_filter_column"]) == 40  # nothing existing grew
    assert int(got["PQG_FILTER_DICT_LDS_BYTES"]) == abi.FILTER_DICT_LDS_BYTES
    assert abi.FILTER_DICT_LDS_BYTES % 8 == 0  # whole table words
    assert int(got["PQG_ABI_VERSION"]) == abi.ABI_VERSION == 6


def test_new_functions_are_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], capture_output=True, text=True).stdout
    defined = set(re.findall(r"\bT (pqg_\w+)", out))
    for name in ("pqg_filter_run_dict", "pqg_decode_dictionary", "pqg_filter_run"):
        assert name in defined and name in native.EXPORTS and hasattr(native.lib(), name)


def test_null_ctx_is_refused():
    result = abi.FilterResult()
    rc = native.lib().pqg_filter_run_dict(None, None, None, None, 0, 0, None, None, 0, C.addressof(result))
    assert rc == abi.ERR_INVALID_ARG
    desc, st = abi.ColumnDesc(), abi.Status()
    assert native.lib().pqg_decode_dictionary(None, None, 0, C.byref(desc), C.byref(st)) == abi.ERR_INVALID_ARG
