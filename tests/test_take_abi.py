"""C ABI of the row selection (include/pqgpu.h, "row selection"): the ctypes mirrors match the C struct
layouts, libpqgpu.so exports pqg_take, and the call refuses a NULL ctx. No compute calls here."""
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
  S(pqg_take_column); S(pqg_take_counts); S(pqg_take_result);
  O(pqg_take_column, physical_type); O(pqg_take_column, max_def); O(pqg_take_column, type_length);
  O(pqg_take_column, flags); O(pqg_take_column, values); O(pqg_take_column, binary_data);
  O(pqg_take_column, def_levels); O(pqg_take_column, n_values); O(pqg_take_column, out_values);
  O(pqg_take_column, out_binary_data); O(pqg_take_column, out_def_levels);
  O(pqg_take_column, out_values_capacity); O(pqg_take_column, out_binary_capacity);
  O(pqg_take_counts, n_values); O(pqg_take_counts, n_bytes);
  O(pqg_take_result, n_rows); O(pqg_take_result, error); O(pqg_take_result, error_column);
  printf("PQG_TAKE_MAX_COLUMNS %d\nPQG_ABI_VERSION %d\nPQG_DISPATCH_TAKE_STAGED %d\n", PQG_TAKE_MAX_COLUMNS,
         PQG_ABI_VERSION, (int)PQG_DISPATCH_TAKE_STAGED);
  return 0;
}
"""
MIRRORS = {"pqg_take_column": abi.TakeColumn, "pqg_take_counts": abi.TakeCounts, "pqg_take_result": abi.TakeResult}


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
    assert n_fields == sum(len(m._fields_) for m in MIRRORS.values())  # every field of every mirror was probed
    assert int(got["PQG_TAKE_MAX_COLUMNS"]) == abi.TAKE_MAX_COLUMNS
    assert int(got["PQG_ABI_VERSION"]) == abi.ABI_VERSION == 6
    assert int(got["PQG_DISPATCH_TAKE_STAGED"]) == abi.DISPATCH_TAKE_STAGED


def test_pqg_take_is_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], capture_output=True, text=True).stdout
    assert "pqg_take" in set(re.findall(r"\bT (pqg_\w+)", out))
    assert "pqg_take" in native.EXPORTS and hasattr(native.lib(), "pqg_take")


def test_null_ctx_is_refused():
    counts, result = abi.TakeCounts(), abi.TakeResult()
    rc = native.lib().pqg_take(None, None, 0, None, 0, 0, C.addressof(counts), C.addressof(result))
    assert rc == abi.ERR_INVALID_ARG
