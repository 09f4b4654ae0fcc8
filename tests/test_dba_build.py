"""The hand-built DELTA_BYTE_ARRAY pages (dba_build.py, dba_cases.py) on the CPU: every legal case
unrolls (dba_build.unroll, DeltaByteArrayReader.readBytes restated) and the oracle returns exactly
those values; every illegal case fails in both at the same value; and the model of the copy's dispatch
(dba_build.paths) shows that the cases sit on the seams they are named for. This is what makes the
pages trustworthy for tests/test_gpu_dba_forms.py."""
import os
import re

import numpy as np
import pytest

from oracle import pqref
from pqgpu import abi
from pqgpu.batch import build_batch

import dba_build as B
import dba_cases as DC

LEGAL = DC.legal_cases()
ILLEGAL = DC.illegal_cases()
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "parquet-mr_amd", "csrc")


def test_constants_match_the_kernels():
    """The six thresholds of dba_build against their constexpr lines: a retune fails here instead of
    moving the cases off the seams."""
    for fname, name, value in B.CONSTANTS:
        with open(os.path.join(CSRC, fname)) as f:
            found = re.findall(r"^\s*constexpr\s+(?:uint32_t|int)\s+%s\s*=\s*(\d+)\s*;" % name, f.read(), flags=re.M)
        assert found == [str(value)], (fname, name, found)
    assert B.BIN_CHUNK == 4 * B.WAVE


def test_the_case_lists_are_complete():
    count = {g: len(DC.legal_cases(g)) for g in DC.GROUPS}
    assert count == {
        "batch": len(DC.BATCH_SIZES) * len(DC.SHAPES) + 2,
        "tail": len(DC.TAIL_SIZES) * len(DC.SHAPES) + 7,
        "chain_par": len(DC.CHAIN_PAR_CHUNKS) * len(DC.CHAIN_SHAPES),
        "chain_serial": len(DC.CHAIN_SERIAL_VALUES) * len(DC.CHAIN_SHAPES),
        "vb": 5, "lds": 10, "flba": 2 * len(DC.FLBA_WIDTHS), "carry": 2 * len(DC.CARRY_LENGTHS) - 1 + 2}, count
    assert len(DC.illegal_cases("carry")) == len(DC.CARRY_LENGTHS)
    assert len(DC.illegal_cases("illegal")) == len(DC.ILLEGAL_AT) + 4
    assert all(c.kind == "legal" for c in LEGAL) and all(c.kind == "illegal" for c in ILLEGAL)


def test_unroll():
    assert B.unroll([0, 2, 0, 0, 3], [b"abc", b"d", b"", b"xyz", b""]) == [b"abc", b"abd", b"", b"xyz", b"xyz"]
    assert B.unroll([2], [b"c"], previous=b"abc") == [b"abc"]
    with pytest.raises(B.Illegal) as e:
        B.unroll([0, 4], [b"abc", b""])
    assert (e.value.index, e.value.kind) == (1, "prefix")
    with pytest.raises(B.Illegal) as e:
        B.unroll([0, 0, 0], [b"ab", b"", b"c"], suffix_bytes=2)
    assert (e.value.index, e.value.kind) == (2, "eof")


@pytest.mark.parametrize("c", LEGAL, ids=[c.name for c in LEGAL])
def test_oracle_returns_the_unrolled_values(c):
    """The case as the last page of a column (after the page it continues, for a carry case): status 0
    and exactly unroll's values, in both the prefix / suffix stream shapes of the case."""
    ch, want, dl = DC.column_of(c)
    assert want[len(want) - len(c.prefixes):] == c.values()
    ref = pqref.decode_batch(build_batch([ch]))
    assert ref.status[0] == 0, ref.status
    assert ref.columns[0]["n_values"] == len(want)
    got = ref.columns[0]["values"]
    if c.ptype == abi.FIXED_LEN_BYTE_ARRAY:
        assert np.asarray(got).tobytes() == b"".join(want) and len(got) == len(want)
    else:
        assert got == want


@pytest.mark.parametrize("c", ILLEGAL, ids=[c.name for c in ILLEGAL])
def test_oracle_fails_where_unroll_raises(c):
    total = sum(len(s) for s in c.suffixes)
    with pytest.raises(B.Illegal) as e:
        B.unroll(c.prefixes, c.suffixes, c.previous, suffix_bytes=total - c.cut)
    code, index = c.bad
    assert e.value.index == index and (e.value.kind == "eof") == (code == abi.ERR_EOF)
    ch, _, _ = DC.column_of(c)
    ref = pqref.decode_batch(build_batch([ch]))
    assert ref.status == (code, len(ch.pages) - 1, index), ref.status


# ---- the cases reach their seams (from paths alone) -------------------------------------------------------

@pytest.fixture(scope="module")
def routes():
    return {c.name: B.paths(c.prefixes, c.lengths()) for c in LEGAL if c.group != "carry"}


POW2 = [1, 2, 4, 8, 16, 32, 64, 128, 255]


def test_coverage(routes):
    g = lambda group: [(c, routes[c.name]) for c in DC.legal_cases(group)]  # noqa: E731
    # serial and chunk-parallel pages with the longest value exactly at the threshold
    longest = {c.name: max(c.lengths()) for c, _ in g("vb")}
    assert sorted(set(longest.values())) == [B.DBA_VB - 1, B.DBA_VB, B.DBA_VB + 1]
    for c, r in g("vb"):
        assert r["serial"] == (longest[c.name] == B.DBA_VB + 1), c.name
    assert sum(r["serial"] for _, r in g("vb")) == 3
    for c, r in g("flba"):
        assert r["serial"] == (c.type_length == B.DBA_VB + 1)
    assert {c.type_length for c, _ in g("flba")} == set(DC.FLBA_WIDTHS)
    for group in ("batch", "tail", "chain_par", "chain_serial", "lds"):
        assert not any(r["serial"] for _, r in g(group)), group
    # pages of exactly DCP and DCP + 1 chunks, and the chunk counts the issue names
    assert sorted({r["n_chunks"] for _, r in g("chain_par")}) == DC.CHAIN_PAR_CHUNKS and B.DCP in DC.CHAIN_PAR_CHUNKS
    assert {r["n_chunks"] for _, r in g("chain_serial")} == {B.DCP + 1}
    assert sorted({len(c.prefixes) for c, _ in g("chain_serial")}) == [B.DCP * B.BIN_CHUNK + 1, (B.DCP + 1) * B.BIN_CHUNK]
    assert any(len(c.prefixes) == B.DCP * B.BIN_CHUNK for c, _ in g("chain_par"))
    assert all(len(v) == 64 for grp in ("chain_par", "chain_serial") for c, _ in g(grp) for v in c.values()[::997])
    # chain_par: donor chunks at every power-of-two distance and at 255; chunk 255 reads chunk 0
    far = set()
    for c, r in g("chain_par"):
        for ch in r["chunks"]:
            far.update(ch["inherited"])
    assert set(POW2) <= far, sorted(far)
    assert any(r["n_chunks"] == B.DCP and B.DCP - 1 in r["chunks"][B.DCP - 1]["inherited"] for _, r in g("chain_par"))
    # (the ladders take different donors: ladder_up reads many chunks, all_inherit only chunk 0)
    up = next(r for c, r in g("chain_par") if c.name == "chain_par-ladder_up-256")
    assert len({d for ch in up["chunks"] for d in ch["inherited"]}) >= 50
    # tail: donor values at every power-of-two distance and at 255 within one chunk's last value
    assert any(set(POW2) <= set(ch["own"]) for _, r in g("tail") for ch in r["chunks"])
    near = set()
    for _, r in g("tail"):
        for ch in r["chunks"]:
            near.update(ch["own"])
    assert len(near) >= 100, sorted(near)
    assert sorted({len(c.prefixes) for c, _ in g("tail")} & set(DC.TAIL_SIZES)) == DC.TAIL_SIZES
    # chunk-last values long enough for many rounds of 64 bytes, own and inherited
    assert any(len(ch["own"]) > 1500 for _, r in g("tail") for ch in r["chunks"])
    assert any(len(ch["inherited"]) > 1500 for _, r in g("tail") for ch in r["chunks"])
    # a chunk with no own bytes (m_c = |T_c| > 0), and an empty chunk-last value
    assert any(ch["m"] == ch["last_len"] > 0 and not ch["own"] for _, r in g("tail") for ch in r["chunks"][1:])
    assert any(ch["last_len"] == 0 for _, r in g("tail") for ch in r["chunks"])
    # batch: the previous-smaller chain at its full depth, in every page size; empty values in place
    assert sorted({len(c.prefixes) for c, _ in g("batch")}) == DC.BATCH_SIZES
    assert max(b["depth"] for _, r in g("batch") for b in r["batches"]) == B.WAVE - 1
    assert all(b["total"] <= B.DBA_OB and b["suffix"] <= B.DBA_SB for _, r in g("batch") for b in r["batches"])
    for c, _ in g("batch"):
        if "empties" in c.name:
            ln = c.lengths()
            assert [ln[i] for i in (0, 20, 63, 64, 100, 128)] == [0] * 6 and max(ln) > 0
    # lds: the staging and assembly limits, from both sides
    chunk_suffix = {ch["suffix"] for _, r in g("lds") for ch in r["chunks"]}
    assert {B.DBA_SB, B.DBA_SB + 1} <= chunk_suffix
    totals = [[b["total"] for b in r["batches"][4:8]] for _, r in g("lds")]
    assert any(B.DBA_OB in t for t in totals)
    for at in (0, 2, 3):  # the batch over the limit first, in the middle and last, its neighbours small
        assert any(t[at] == B.DBA_OB + 1 and all(x < 1024 for i, x in enumerate(t) if i != at) for t in totals), at
    sufs = [[b["suffix"] for b in r["batches"][4:8]] for _, r in g("lds")]
    assert any(B.DBA_SB in s for s in sufs)
    for at in (0, 2, 3):
        assert any(s[at] == B.DBA_SB + 1 for s in sufs), at
    # a chunk over DBA_SB whose batches all fit: the batch path from dba_values
    assert any(ch["suffix"] > B.DBA_SB and all(b["suffix"] <= B.DBA_SB and b["total"] <= B.DBA_OB
                                               for b in r["batches"][4:8])
               for _, r in g("lds") for ch in r["chunks"][1:2])
    # a chunk of one value (65 537 values), full last chunks, and carry lengths around the threshold
    assert any(len(c.prefixes) % B.BIN_CHUNK == 1 for c, _ in g("chain_serial"))
    carry_last = {len(c.previous) for c in DC.legal_cases("carry")}
    assert carry_last == set(DC.CARRY_LENGTHS)
    for c in DC.legal_cases("carry") + DC.illegal_cases("carry"):
        assert c.prefixes[0] in (0, len(c.previous), len(c.previous) + 1)


def test_short_of_common_repeats_bytes():
    """The shape's prefixes stop short of the common prefix (the suffix starts with the previous
    value's next bytes), the other shapes' suffixes start with a fresh byte almost always."""
    c = DC.case("tail-short_of_common-513")
    vals, short = c.values(), 0
    for i in range(1, len(vals)):
        p = c.prefixes[i]
        short += len(vals[i]) > p and len(vals[i - 1]) > p and vals[i][p] == vals[i - 1][p]
    assert short > 400
