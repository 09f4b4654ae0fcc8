"""C ABI of the record selection on repeated columns (include/pqgpu.h): the ctypes mirrors match the C
struct layouts, libpqgpu.so exports pqg_take_records, and the call refuses a NULL ctx. The addition left
PQG_ABI_VERSION at 6. No compute calls here."""
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
  S(pqg_take_record_column); S(pqg_take_record_counts); S(pqg_take_column);
  O(pqg_take_record_column, col); O(pqg_take_record_column, max_rep); O(pqg_take_record_column, reserved);
  O(pqg_take_record_column, rep_levels); O(pqg_take_record_column, n_slots);
  O(pqg_take_record_column, out_rep_levels); O(pqg_take_record_column, out_slots_capacity);
  O(pqg_take_record_counts, n_records); O(pqg_take_record_counts, n_slots); O(pqg_take_record_counts, n_values);
  O(pqg_take_record_counts, n_bytes);
  printf("PQG_TAKE_MAX_COLUMNS %d\nPQG_ABI_VERSION %d\n", PQG_TAKE_MAX_COLUMNS, PQG_ABI_VERSION);
  return 0;
}
"""
MIRRORS = {"pqg_take_record_column": abi.TakeRecordColumn, "pqg_take_record_counts": abi.TakeRecordCounts}


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
    assert dict(abi.TakeRecordColumn._fields_)["col"] is abi.TakeColumn and int(got["pqg_take_column"]) == C.sizeof(abi.TakeColumn)
    assert int(got["PQG_TAKE_MAX_COLUMNS"]) == abi.TAKE_MAX_COLUMNS
    assert int(got["PQG_ABI_VERSION"]) == abi.ABI_VERSION == 6


def test_pqg_take_records_is_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], capture_output=True, text=True).stdout
    assert "pqg_take_records" in set(re.findall(r"\bT (pqg_\w+)", out))
    assert "pqg_take_records" in native.EXPORTS and hasattr(native.lib(), "pqg_take_records")


def test_null_ctx_is_refused():
    counts, result = abi.TakeRecordCounts(), abi.TakeResult()
    rc = native.lib().pqg_take_records(None, None, 0, None, 0, 0, C.addressof(counts), C.addressof(result))
    assert rc == abi.ERR_INVALID_ARG
