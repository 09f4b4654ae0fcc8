"""pqg_filter_create_typed (csrc/pqgpu_filter_host.cpp) under AddressSanitizer + UndefinedBehaviorSanitizer:
tests/c/filter_typed_sanitize.cpp, a stand-alone program, hands it valid typed tables (FLBA widths 1 .. 40,
INT96, BYTE_ARRAY, the three orders, all eight ops, literals of 0 .. 40 bytes, sets with comparator-equal
members), every refusal the header lists and deterministic bit flips in the node, column-type and literal
tables, all in exactly-sized heap blocks; and it holds the literal keys the host prepares for the device
(128-bit signed-integer keys, FLOAT16 keys, sorted sets) against plain byte-loop comparators on random pairs.
Any out-of-bounds access or undefined behaviour aborts the run. Nothing is loaded into Python."""
import os
import re
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "parquet-mr_amd", "csrc")


def test_filter_create_typed_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "filter_typed_sanitize")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-I", os.path.join(REPO, "include"),
                    os.path.join(REPO, "tests", "c", "filter_typed_sanitize.cpp"), os.path.join(CSRC, "pqgpu_filter_host.cpp"),
                    "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe, "300", "3000"], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
    m = re.fullmatch(r"cases=(\d+) ok=(\d+) invalid=(\d+) pairs=(\d+)\s*", out.stdout)
    assert m, out.stdout
    cases, ok, invalid, pairs = map(int, m.groups())
    n_bases = 9 * 2 * 8 + 41 * 3 + 2
    assert pairs == 3000 and ok + invalid == cases
    assert cases == n_bases + 21 + 2 * 3000 + 50 + (n_bases + 6) // 7 * 300
    # the mutations reach both outcomes: harmless ones stay valid, the others are refused, not crashed on
    assert ok > n_bases + 2 * 3000 + 50 + 300 and invalid > 1000
