"""The host-only logic of the C ABI (csrc/pqgpu_api_host.cpp: the hybrid-stream walk and run cache of
pqg_router_read_page, the pinned image of pqg_router_read_runs, error resolution of a launched plan, the
length-prefix walk of a BYTE_ARRAY dictionary page) without a device: tests/c/api_host_main.cpp, a
stand-alone program, builds its inputs in exactly-sized heap blocks and checks what every case must give.
Built once with AddressSanitizer + UndefinedBehaviorSanitizer (any out-of-bounds access or undefined
behaviour aborts the run) and once plain; the digest of either build must equal
tests/golden/api_host/digest.txt byte for byte: that file was recorded from the text these functions had in
pqgpu_api.hip before they were moved (tools/record_api_host_digest.py).
Nothing is loaded into Python.

Fuzz: N = 5,000 mutations each of router streams, error-word tables and dictionary pages; the sanitized run
takes under a second, the two compilations about 10 s."""
import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = [os.path.join(REPO, "tests", "c", "api_host_main.cpp"),
           os.path.join(REPO, "parquet-mr_amd", "csrc", "pqgpu_api_host.cpp")]
GOLDEN = os.path.join(REPO, "tests", "golden", "api_host", "digest.txt")
FUZZ_N = 5000
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


def _build(exe, flags):
    # plain g++, warnings on, and only the repository's include/ on the include path: this code needs no HIP
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags +
                   ["-I", os.path.join(REPO, "include")] + SOURCES + ["-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("api_host") / "api_host_san"),
                  ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("api_host") / "api_host"), ["-O2"])


def _run(exe, *args):
    out = subprocess.run([exe, *args], capture_output=True, text=True, env=ENV, timeout=300)
    assert out.returncode == 0, (out.stdout[-2000:] + out.stderr)[-4000:]
    m = re.search(r"^cases=(\d+)\s*\Z", out.stdout, re.M)
    assert m, out.stdout[-2000:]
    return out.stdout, int(m.group(1))


def test_cases_under_asan_ubsan(sanitized):
    _, cases = _run(sanitized, "cases")
    assert cases >= 180


def test_digest_matches_the_code_it_was_moved_from(plain, sanitized):
    with open(GOLDEN) as f:
        golden = f.read()
    for exe in (plain, sanitized):
        out, cases = _run(exe, "digest")
        differ = [a.split()[:2] for a, b in zip(out.splitlines(), golden.splitlines()) if a != b]
        assert out == golden, f"results differ from tests/golden/api_host/digest.txt: {differ[:10]}"
    assert set(line.split()[0] for line in golden.splitlines()[:-1]) == {"walk", "lookup", "resolve", "decode", "dict"}


def test_fuzz_under_asan_ubsan(sanitized):
    _, cases = _run(sanitized, "fuzz", str(FUZZ_N))
    assert cases == 3 * FUZZ_N and FUZZ_N >= 2000
