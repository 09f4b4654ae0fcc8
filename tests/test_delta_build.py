"""The hand-built DELTA pages (delta_build.py, delta_cases.py) on the CPU: the builder reproduces the
restated parquet-mr writer byte for byte when given the writer's own choices, and the oracle
(oracle/pqref.c) agrees with the independent Python reader (delta_build.read) on every case: values
bit for bit, bytes consumed, error code. Then the oracle decodes every case under ASan + UBSan. This
is what makes the pages trustworthy for tests/test_gpu_delta_pages.py."""
import os
import subprocess

import numpy as np
import pytest

from oracle import pqref
from pqgpu import abi
from tools.synth import writer

import delta_build as DB
from delta_cases import (ALL_CONFIGS, CONFIGS, GROUPS, INT_GROUPS, batch_of, illegal_cases, legal_cases, path_of,
                         segment_coverage)
from test_oracle_sanitize import serialize

LEGAL = legal_cases()
ILLEGAL = illegal_cases()


def test_the_case_lists_are_complete():
    assert {c.group for c in LEGAL} == set(GROUPS)
    assert {c.group for c in ILLEGAL} == {"varints", "counts", "illegal", "strings"}
    for g in INT_GROUPS:  # every integer page once per type
        a = sorted(c.id[:-4] for c in LEGAL if c.group == g and c.ptype == abi.INT64)
        b = sorted(c.id[:-4] for c in LEGAL if c.group == g and c.ptype == abi.INT32)
        assert a and a == b
    assert len(LEGAL) >= 500 and len(ILLEGAL) >= 150
    assert {c.expect for c in ILLEGAL} == {abi.ERR_EOF, abi.ERR_CORRUPT, abi.ERR_DELTA_CONFIG}


def test_config_table_names_the_paths():
    """The table of delta_cases.py against the dispatch of delta_stream restated in path_of, for both
    value widths."""
    for name, configs in CONFIGS.items():
        for block, mbn in configs:
            assert path_of(block, mbn, 8) == name and path_of(block, mbn, 4) == name, (name, block, mbn)


def test_segment_coverage():
    """Group `segments`: block headers at each of the 4 alignments, and at least one that starts
    within 40 bytes before a multiple of 8 KiB (counted from the builder's header offsets)."""
    cases = [c for c in LEGAL if c.group == "segments" and c.ptype == abi.INT64]
    assert len(cases) == 30 and all(30 << 10 <= len(c.page) <= 62 << 10 for c in cases)
    mods, edges = segment_coverage(cases)
    print("header alignments", sorted(mods), "headers before a segment edge", edges)
    assert mods == {0, 1, 2, 3}
    assert edges >= 1
    assert {(int(c.id.split("-")[2]), int(c.id.split("-")[3])) for c in cases} <= set(ALL_CONFIGS)


# ---- the builder against the writer ---------------------------------------------------------------------

def writer_choices(values, bits, block, mbn):
    """What DeltaBinaryPackingValuesWriterFor{Long,Integer} (restated in tools/synth/pqwriter.cpp,
    DeltaEncoder) chooses for `values`: per block the min delta, the minimal width of every flushed
    miniblock, and what it leaves behind: the width bytes of the miniblocks it does not flush are those
    of the block before, and the padding of the last flushed miniblock is what deltaBlockBuffer still
    holds there (the block before's deltas less its min delta; 0 in a first block), packed masked to
    the miniblock's width."""
    ring, half = 1 << bits, 1 << (bits - 1)
    sgn = lambda x: ((x + half) % ring) - half  # noqa: E731
    mbs = block // mbn
    buf, widths, blocks = [0] * block, [0] * mbn, []
    deltas = [sgn(int(values[i]) - int(values[i - 1])) for i in range(1, len(values))]
    for s in range(0, len(deltas), block):
        cur = deltas[s:s + block]
        md = min(cur)
        for i, d in enumerate(cur):
            buf[i] = (d - md) % ring
        used = (len(cur) + mbs - 1) // mbs
        out = []
        for m in range(used):
            mask = 0
            for x in buf[m * mbs:min((m + 1) * mbs, len(cur))]:
                mask |= x
            widths[m] = mask.bit_length()
            out.append([x & ((1 << widths[m]) - 1) for x in buf[m * mbs:(m + 1) * mbs]])
        blocks.append((md, list(widths), out))
    return blocks


@pytest.mark.parametrize("ptype", [abi.INT64, abi.INT32], ids=["i64", "i32"])
@pytest.mark.parametrize("config", [(128, 4), (2048, 8), (24, 3)], ids=lambda c: f"{c[0]}-{c[1]}")
def test_builder_reproduces_the_writer(config, ptype):
    """50 seeded random arrays: the builder fed the writer's choices (minimal widths, its stale width
    bytes and stale padding deltas, shortest varints) gives writer.delta_encode's bytes exactly, the
    stale padding included."""
    block, mbn = config
    bits = 64 if ptype == abi.INT64 else 32
    for seed in range(50):
        rng = np.random.default_rng(seed * 7 + block)
        n = int(rng.integers(0, 3 * block + 40)) if seed else 0
        scale = int(rng.integers(1, bits))
        vals = rng.integers(-(1 << scale), 1 << scale, size=n, endpoint=False).astype(abi.numpy_dtype(ptype))
        if seed % 3 == 0:
            vals = np.cumsum(vals).astype(vals.dtype)
        first = int(vals[0]) if n else 0
        page = DB.build(block, mbn, n, first, writer_choices(vals, bits, block, mbn))
        assert page == writer.delta_encode(vals, ptype, block, mbn), (seed, n)
        got = DB.read(page)
        assert not isinstance(got, int) and got[1] == len(page)
        assert np.array_equal(got[0].astype(vals.dtype), vals)


# ---- the oracle against the Python reader -----------------------------------------------------------------

def np_type(c):
    return np.int64 if c.ptype == abi.INT64 else np.int32


@pytest.mark.parametrize("c", LEGAL + ILLEGAL, ids=[c.id for c in LEGAL + ILLEGAL])
def test_oracle_agrees_with_the_reader(c):
    """Every DELTA stream of the page through delta_build.read and through the oracle's reader: the
    same values, the same bytes consumed or the same error; then the page as a one-page column through
    pqr_decode: the case's code, and for an integer page the reader's first `want` values."""
    pos, vals = 0, None
    for _ in range(c.streams):
        mine = DB.read(c.page, pos)
        cap = (1 if isinstance(mine, int) else len(mine[0])) + 8
        theirs = pqref.delta_decode(c.page[pos:], cap=cap)
        if isinstance(mine, int):
            assert theirs == (mine, None), (mine, theirs)
            assert not c.legal and mine == c.expect
            break
        assert theirs[1] is not None, ("oracle error", theirs[0])
        assert mine[1] == theirs[1] and np.array_equal(mine[0], theirs[0])
        pos += mine[1]
        vals = vals if vals is not None else mine[0]
    else:
        if c.ptype != abi.BYTE_ARRAY:
            assert c.legal and c.want <= len(vals)
    ref = pqref.decode_batch(batch_of([c]))
    assert ref.code == (0 if c.legal else c.expect), ref.status
    if c.legal:
        assert ref.columns[0]["n_values"] == c.want
        if c.ptype != abi.BYTE_ARRAY:
            assert np.array_equal(ref.columns[0]["values"], vals[:c.want].astype(np_type(c)))
    if c.twin:
        twin = next(t for t in LEGAL if t.id == c.twin)
        assert c.page != twin.page and np.array_equal(vals[:c.want], DB.read(twin.page)[0][:c.want])


def test_strings_decode_to_what_was_built():
    """Group `strings`: the wide-length pages read as lengths below 12, and the two-stream pages take
    their bytes from where the second stream ends."""
    for c in LEGAL:
        if c.group != "strings":
            continue
        ref = pqref.decode_batch(batch_of([c]))
        assert ref.code == 0 and ref.columns[0]["n_values"] == c.want
        lens = [len(v) for v in ref.columns[0]["values"]]
        if c.encoding == abi.DELTA_LENGTH_BYTE_ARRAY:
            longs, used = DB.read(c.page)
            assert max(lens) < 12 and lens == [int(x) & 0xFFFFFFFF for x in longs]
            assert int(np.abs(longs).max()) >> 32 and used + sum(lens) == len(c.page)
        else:
            pre, n1 = DB.read(c.page)
            suf, n2 = DB.read(c.page, n1)
            assert len(pre) >= len(suf) == c.want and n1 + n2 + int(suf.sum()) == len(c.page)
            assert lens == [int(a) + int(b) for a, b in zip(pre, suf)]


def test_oracle_under_asan_ubsan(tmp_path):
    """The oracle on every case under AddressSanitizer + UndefinedBehaviorSanitizer (host code, the
    stand-alone driver oracle/sanitize_main.c; one-column batches in its PQGB format): exit status 0
    and the expected code per case."""
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    oracle = os.path.join(repo, "oracle")
    exe = str(tmp_path / "sanitize_main")
    subprocess.run(["gcc", "-std=c11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-I", oracle, "-I", os.path.join(repo, "include"),
                    os.path.join(oracle, "sanitize_main.c"), os.path.join(oracle, "pqref.c"), "-o", exe], check=True)
    cases = LEGAL + ILLEGAL
    files = []
    for i, c in enumerate(cases):
        files.append(str(tmp_path / f"case_{i}.bin"))
        serialize(batch_of([c]), files[-1])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe] + files, capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, out.stderr[-4000:]
    codes = [int(ln.rsplit("rc=", 1)[1]) for ln in out.stdout.splitlines()]
    assert codes == [0] * len(LEGAL) + [c.expect for c in ILLEGAL]
