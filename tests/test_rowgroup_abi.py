"""C ABI of the row-group dictionary filter (include/pqgpu.h, additions to ABI 6): the struct sizes (32, 16, 12) and
field offsets of the ctypes mirrors match a compiled C snippet, the flag values and the tile size are the header's,
the version is still 6, libpqgpu.so exports the new functions and pqg_filter_row_groups refuses a NULL ctx."""
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
#define V(v) printf("%s %d\n", #v, (int)(v))
int main(void) {
  S(pqg_rowgroup_column); S(pqg_rowgroup_result); S(pqg_page_encoding_stat); S(pqg_filter_dictionary);
  O(pqg_rowgroup_column, dict); O(pqg_rowgroup_column, flags); O(pqg_rowgroup_column, reserved);
  O(pqg_rowgroup_result, n_kept); O(pqg_rowgroup_result, error); O(pqg_rowgroup_result, error_group);
  O(pqg_page_encoding_stat, page_type); O(pqg_page_encoding_stat, encoding); O(pqg_page_encoding_stat, count);
  V(PQG_RG_MISSING); V(PQG_RG_NO_DICTIONARY); V(PQG_RG_NON_DICT_PAGES); V(PQG_RG_MAY_CONTAIN_NULL);
  V(PQG_RG_TILE_ENTRIES); V(PQG_ABI_VERSION);
  return 0;
}
"""
MIRRORS = {"pqg_rowgroup_column": abi.RowGroupColumn, "pqg_rowgroup_result": abi.RowGroupResult,
           "pqg_page_encoding_stat": abi.PageEncodingStat, "pqg_filter_dictionary": abi.FilterDictionary}


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
    assert n_fields == sum(len(MIRRORS[s]._fields_) for s in ("pqg_rowgroup_column", "pqg_rowgroup_result",
                                                              "pqg_page_encoding_stat"))
    assert (int(got["pqg_rowgroup_column"]), int(got["pqg_rowgroup_result"]), int(got["pqg_page_encoding_stat"])) == (32, 16, 12)
    assert int(got["pqg_filter_dictionary"]) == 24  # nothing existing grew
    assert [int(got[k]) for k in ("PQG_RG_MISSING", "PQG_RG_NO_DICTIONARY", "PQG_RG_NON_DICT_PAGES",
                                  "PQG_RG_MAY_CONTAIN_NULL")] == [1, 2, 4, 8]
    assert (abi.RG_MISSING, abi.RG_NO_DICTIONARY, abi.RG_NON_DICT_PAGES, abi.RG_MAY_CONTAIN_NULL) == (1, 2, 4, 8)
    assert int(got["PQG_RG_TILE_ENTRIES"]) == abi.RG_TILE_ENTRIES and abi.RG_TILE_ENTRIES % 64 == 0
    assert int(got["PQG_ABI_VERSION"]) == abi.ABI_VERSION == 6


def test_new_functions_are_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], capture_output=True, text=True).stdout
    defined = set(re.findall(r"\bT (pqg_\w+)", out))
    for name in ("pqg_filter_row_groups", "pqg_chunk_has_non_dictionary_pages", "pqg_decode_dictionaries"):
        assert name in defined and name in native.EXPORTS and hasattr(native.lib(), name)


def test_null_arguments_are_refused():
    result = abi.RowGroupResult()
    L = native.lib()
    assert L.pqg_filter_row_groups(None, None, None, 0, 0, None, None, 0, C.addressof(result)) == abi.ERR_INVALID_ARG
    desc, st = abi.ColumnDesc(), abi.Status()
    assert L.pqg_decode_dictionaries(None, None, 0, C.byref(desc), 1, C.byref(st)) == abi.ERR_INVALID_ARG
    # no stats and no encodings: not dictionary-encoded as far as the list can tell
    assert L.pqg_chunk_has_non_dictionary_pages(None, -1, None, 0) == 1
    assert L.pqg_chunk_has_non_dictionary_pages(None, 0, None, 0) == 0  # stats present but empty: no data pages
