"""The hand-built Zstandard frames (zstd_build.py, zstd_cases.py) against the oracle
(oracle/zstd_ref.c) and, where pyarrow is installed, against libzstd itself: a legal frame decodes to
the bytes the builder executed, an illegal one is refused by both. This is what makes the frames
trustworthy for tests/test_gpu_zstd_frames.py: a frame libzstd does not decode to the intended bytes
is a builder bug.

The few frames on which libzstd is known to be laxer than RFC 8878 carry libzstd=False in
zstd_cases.py, each with its reason; the oracle (and the device) still refuse them."""
import os
import subprocess

import pytest

from oracle import pqref

from zstd_build import Frame, Lit, execute
from zstd_cases import GROUPS, illegal_cases, legal_cases

LEGAL = legal_cases()
ILLEGAL = illegal_cases()

try:
    import pyarrow as pa
    CODEC = pa.Codec("zstd")
except ImportError:  # the oracle half still runs
    CODEC = None


def test_the_case_lists_are_complete():
    """Every group of the issue's list is there, and libzstd is left out of a handful only."""
    assert {c.group for c in LEGAL} == set(GROUPS)
    assert len(LEGAL) >= 330 and len(ILLEGAL) >= 45
    assert all(c.libzstd for c in LEGAL)
    assert sorted(c.id for c in ILLEGAL if not c.libzstd) == [
        "block-regenerates-over-128-KiB", "huffman-4-long-streams-leftover", "huffman-4-long-streams-short",
        "huffman-4-long-streams-zero-last"]
    assert {c.seq_bits for c in LEGAL if c.group == "bit-budget"} == {64, 65, 74}


def test_executor_repeat_offsets():
    """The builder's executor on a sequence list worked out by hand (RFC 8878 3.1.1.5)."""
    out, rep = bytearray(b"0123456789"), [1, 4, 8]
    execute(out, 0, b"abc", [(1, 3, 3 + 6), (0, 2, 1), (1, 2, 3), (0, 3, 3)], rep)
    # offset 6 -> {6, 1, 4}; ll 0, value 1 -> rep1 = 1 -> {1, 6, 4}; value 3 -> rep2 = 4 -> {4, 1, 6};
    # ll 0, value 3 -> rep0 - 1 = 3 -> {3, 4, 1}
    assert bytes(out) == b"0123456789" + b"a" + b"567" + b"77" + b"b" + b"77" + b"b77" + b"c"
    assert rep == [3, 4, 1]


@pytest.mark.parametrize("c", LEGAL, ids=[c.id for c in LEGAL])
def test_legal_frame(c):
    assert pqref.zstd_decompress(c.frame, c.n) == c.expected[:c.n]
    if CODEC is not None:
        # libzstd's one-shot call takes the whole content (it fails on a smaller destination)
        assert CODEC.decompress(c.frame, decompressed_size=len(c.expected), asbytes=True) == c.expected


@pytest.mark.parametrize("c", ILLEGAL, ids=[c.id for c in ILLEGAL])
def test_illegal_frame(c):
    with pytest.raises(ValueError, match="error 18"):
        pqref.zstd_decompress(c.frame, c.n)
    if CODEC is not None and c.libzstd:
        with pytest.raises(Exception):
            CODEC.decompress(c.frame, decompressed_size=c.n, asbytes=True)


def test_libzstd_checked_every_frame():
    """On a machine with pyarrow the libzstd half ran: all legal frames (the empty ones too), all
    illegal frames but the documented four."""
    pytest.importorskip("pyarrow")
    assert CODEC is not None
    assert sum(1 for c in LEGAL if c.libzstd) == len(LEGAL)
    assert sum(1 for c in ILLEGAL if c.libzstd) == len(ILLEGAL) - 4


def test_frame_needs_a_window_for_a_block_larger_than_its_content():
    """The finding that started this: Single_Segment, content size 7, one 9-byte compressed block.
    Block_Maximum_Size = min(Window_Size, 128 KiB) and a Single_Segment frame's Window_Size is its
    content size, so the frame is illegal; with a Window_Descriptor the same block is fine."""
    seq = [(2, 5, 3 + 2)]
    bad, _ = Frame(single=True).compressed(Lit("raw", b"ab"), seq).finish()
    good, out = Frame().compressed(Lit("raw", b"ab"), seq).finish()
    assert out == b"abababa"
    assert pqref.zstd_decompress(good, 7) == out
    with pytest.raises(ValueError, match="error 18"):
        pqref.zstd_decompress(bad, 7)


def test_oracle_under_asan_ubsan(tmp_path):
    """The oracle's ZSTD decoder on every hand-built frame under AddressSanitizer +
    UndefinedBehaviorSanitizer (host code, the stand-alone driver oracle/sanitize_main.c): exactly-sized
    input and output, so a read past the frame or a write past the page's size aborts the run."""
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    oracle = os.path.join(repo, "oracle")
    exe = str(tmp_path / "sanitize_main")
    subprocess.run(["gcc", "-std=c11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-DPQR_SANITIZE_ZSTD", "-I", oracle, "-I", os.path.join(repo, "include"),
                    os.path.join(oracle, "sanitize_main.c"), os.path.join(oracle, "pqref.c"),
                    os.path.join(oracle, "zstd_ref.c"), os.path.join(oracle, "gzip_ref.c"), "-o", exe], check=True)
    cases = LEGAL + ILLEGAL
    files = []
    for i, c in enumerate(cases):
        files.append(str(tmp_path / f"frame_{i}.bin"))
        with open(files[-1], "wb") as f:
            f.write(b"PQGZ" + c.n.to_bytes(8, "little") + len(c.frame).to_bytes(8, "little") + c.frame)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe] + files, capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stderr[-4000:]
    codes = [int(ln.rsplit("rc=", 1)[1]) for ln in out.stdout.splitlines()]
    assert codes == [0] * len(LEGAL) + [18] * len(ILLEGAL)
