"""The planner of pqg_plan_create (csrc/pqgpu_plan_host.cpp, pqg::plan_layout: descriptor validation, page
classification, work lists, scratch regions) without a device: tests/c/plan_layout.cpp, a stand-alone
program, builds descriptor tables (one case per branch of the planner, each under every dispatch setting,
and deterministic single-field mutations of them), in exactly-sized heap blocks and with fake output
addresses, and checks the invariants of every accepted layout. Built once with AddressSanitizer +
UndefinedBehaviorSanitizer (any out-of-bounds access or undefined behaviour aborts the run) and once plain
for the digest, which must equal tests/golden/plan/layout_digest.txt byte for byte: that file was recorded
from the arithmetic plan creation had before the planner was moved out of pqgpu_api.hip
(tools/record_plan_digest.py).
Nothing is loaded into Python.

Fuzz: N = 20,000 mutations; the whole module (two compilations and five runs) takes about 30 s on an
8-core host, nearly all of it the two compilations; the sanitized fuzz run itself takes under 2 s."""
import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "parquet-mr_amd", "csrc")
SOURCES = [os.path.join(REPO, "tests", "c", "plan_layout.cpp"), os.path.join(CSRC, "pqgpu_plan_host.cpp")]
GOLDEN = os.path.join(REPO, "tests", "golden", "plan", "layout_digest.txt")
FUZZ_N = 20000
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


def _build(exe, flags):
    # plain g++, warnings on, and only the repository's include/ on the include path: the planner needs no HIP
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra"] + flags +
                   ["-I", os.path.join(REPO, "include")] + SOURCES + ["-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("plan") / "plan_layout_san"),
                  ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("plan") / "plan_layout"), ["-O2"])


def _run(exe, *args):
    out = subprocess.run([exe, *args], capture_output=True, text=True, env=ENV, timeout=300)
    assert out.returncode == 0, (out.stdout[-2000:] + out.stderr)[-4000:]
    m = re.search(r"^cases=(\d+) ok=(\d+) invalid=(\d+)\s*\Z", out.stdout, re.M)
    assert m, out.stdout[-2000:]
    cases, ok, invalid = map(int, m.groups())
    assert ok + invalid == cases
    return out.stdout, cases, ok, invalid


def test_cases_under_asan_ubsan(sanitized):
    _, cases, ok, invalid = _run(sanitized, "cases")
    # 16 dispatch settings per case; the refusal cases are refused under every one of them
    assert cases % 16 == 0 and cases >= 16 * 250
    assert invalid == 16 * 6 and ok == cases - invalid


def test_digest_matches_the_recorded_layouts(plain, sanitized):
    with open(GOLDEN) as f:
        golden = f.read()
    for exe in (plain, sanitized):
        out, cases, _, _ = _run(exe, "digest")
        # (a line that differs names the case and the settings; `plan_layout digest-full` prints what was hashed)
        differ = [a.split()[0] for a, b in zip(out.splitlines(), golden.splitlines()) if a != b]
        assert out == golden, f"layouts differ from tests/golden/plan/layout_digest.txt: {differ[:10]}"
    assert len(golden.splitlines()) - 1 == cases // 16  # one line per case


def test_fuzz_under_asan_ubsan(sanitized):
    _, cases, ok, invalid = _run(sanitized, "fuzz", str(FUZZ_N))
    assert cases == FUZZ_N and FUZZ_N >= 2000
    print(f"fuzz: {cases} mutations, refused {invalid / cases:.1%}, accepted {ok / cases:.1%}")
    # only a mutation of column, version or the high bits of offset / size can be refused (about 18 of
    # the 56 bytes of a page descriptor); everything else must be planned
    assert invalid >= 0.05 * cases
    assert ok >= 0.25 * cases
