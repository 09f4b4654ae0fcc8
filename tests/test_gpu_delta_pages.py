"""GPU parity of k_delta (csrc/pqgpu_kernels.hip: delta_stream, delta_hdr_parse / delta_hdr_v /
delta_mind_v, delta_expand<E>, delta_expand_seg, delta_generic) on hand-built DELTA_BINARY_PACKED pages
(delta_build.py, delta_cases.py; tests/test_delta_build.py holds every one of them against an
independent Python reader and the oracle): forms DeltaBinaryPackingValuesReader accepts and the
restated parquet-mr writer never emits: widths that are not minimal, widths over 32 in INT32 and
length streams, arbitrary width bytes for the unread miniblocks of a last block, over-long varints,
bytes after the last used miniblock, a header count above the page's.

Every group runs as required columns (the cases' pages with writer pages between them) and, the legal
ones, a second time as optional columns of V2 pages with about 20 % nulls, each case at another
output offset mod 16 bytes and last in its column: what a store past the page's count writes lands in
the column's unwritten tail, which must still hold the decoder fixture's poison byte."""
import numpy as np
import pytest
import torch

from oracle import pqref
from pqgpu import abi
from tools.synth import writer
from tools.synth.writer import ColumnChunk, Page

from delta_cases import GROUPS, chunk_of, illegal_cases, legal_cases
from helpers import assert_same

pytestmark = pytest.mark.gpu
POISON = 0xA5
TYPES = {"i64": abi.INT64, "i32": abi.INT32, "bytes": abi.BYTE_ARRAY}
GROUP_TYPES = [(g, t) for g in GROUPS for t in (("bytes",) if g == "strings" else ("i64", "i32"))]


def cases_of(group, tname, cases=None):
    out = [c for c in (cases if cases is not None else legal_cases()) if c.group == group and c.ptype == TYPES[tname]]
    assert out
    return out


def writer_body(rng, ptype, encoding, n):
    """An ordinary writer page's data section of n values."""
    if ptype == abi.BYTE_ARRAY:
        vals = list(writer.BinaryValues.random(n, 0, 9, seed=int(rng.integers(0, 1 << 30))))
        return writer.dlba_encode(vals) if encoding == abi.DELTA_LENGTH_BYTE_ARRAY else writer.dba_encode(vals)
    walk = np.cumsum(rng.integers(-1000, 1000, size=n)).astype(abi.numpy_dtype(ptype))
    return writer.delta_encode(walk, ptype)


def required_chunks(cases, seed=0):
    """One required column per encoding: case, writer page, case, writer page, ..."""
    rng = np.random.default_rng(seed)
    chunks = {}
    for c in cases:
        ch = chunks.setdefault(c.encoding, ColumnChunk(physical_type=c.ptype))
        ch.pages.append(Page(body=c.page, num_values=c.want, encoding=c.encoding, num_rows=c.want))
        n = int(rng.integers(1, 400))
        ch.pages.append(Page(body=writer_body(rng, c.ptype, c.encoding, n), num_values=n, encoding=c.encoding, num_rows=n))
    for ch in chunks.values():
        ch.n_values_hint = sum(p.num_values for p in ch.pages)
    return list(chunks.values())


def optional_page(rng, body, encoding, n_values, n_nulls):
    dl = np.ones(n_values + n_nulls, dtype=np.uint8)
    dl[rng.permutation(dl.size)[:n_nulls]] = 0
    dls = writer.rle_encode_levels(dl, 1)
    pg = Page(body=dls + body, num_values=dl.size, encoding=encoding, version=2, num_nulls=n_nulls, num_rows=dl.size)
    pg.dl_byte_length = len(dls)
    return pg


def optional_chunks(cases, seed=0):
    """One optional column per case: a writer page of i % 4 values (none for 0), then the case's
    page, V2, nulls in about a fifth of the slots (at least 24, so that a short page's tail has room)."""
    rng = np.random.default_rng(seed)
    chunks, offsets = [], []
    for i, c in enumerate(cases):
        ch = ColumnChunk(physical_type=c.ptype, max_def=1)
        k = i % 4
        if k:
            ch.pages.append(optional_page(rng, writer_body(rng, c.ptype, c.encoding, k), c.encoding, k, 1))
        ch.pages.append(optional_page(rng, c.page, c.encoding, c.want, max(c.want // 4, 24) + i % 3))
        ch.n_values_hint = k + c.want
        chunks.append(ch)
        offsets.append(k)
    return chunks, offsets


def decode_both(decoder, chunks):
    batch = writer.build_batch(chunks)
    ref = pqref.decode_batch(batch)
    counts = torch.zeros(max(batch.n_pages, 1), dtype=torch.int32, device=decoder.device)
    dcols, st = decoder.decode(decoder.upload(batch), page_counts=counts, check=False)
    assert (int(st.code), int(st.page), int(st.value_index)) == ref.status, \
        f"gpu status {st.code, st.page, st.value_index} {st.message} vs oracle {ref.status}"
    return batch, ref, dcols, counts.cpu().numpy().view(np.uint32)[:batch.n_pages]


def check_columns(batch, ref, dcols, counts):
    assert ref.code == 0, ref.status
    assert np.array_equal(counts, ref.page_value_counts)
    for i, cd in enumerate(batch.columns):
        col = dcols[i]
        assert col.n_values == ref.columns[i]["n_values"], i
        assert_same(col.numpy(), ref.columns[i]["values"], cd["physical_type"])
        if cd["physical_type"] == abi.BYTE_ARRAY:
            assert np.array_equal(col.offsets().cpu().numpy(), ref.columns[i]["offsets"][:col.n_values + 1])
        if cd["max_def"] > 0:
            assert np.array_equal(col.def_levels[:batch.column_slots[i]].cpu().numpy(), ref.columns[i]["def_levels"])


@pytest.mark.parametrize("group,tname", GROUP_TYPES, ids=[f"{g}-{t}" for g, t in GROUP_TYPES])
def test_legal_pages(decoder, group, tname):
    """Values bit for bit, n_values, per-page counts and status against the oracle."""
    batch, ref, dcols, counts = decode_both(decoder, required_chunks(cases_of(group, tname)))
    check_columns(batch, ref, dcols, counts)


@pytest.mark.parametrize("group,tname", GROUP_TYPES, ids=[f"{g}-{t}" for g, t in GROUP_TYPES])
def test_legal_pages_optional_columns(decoder, group, tname):
    """The same pages in optional columns: also the levels, and elements [n_values, n_slots) of every
    value tensor still hold the poison byte (BYTE_ARRAY: the offsets past the count all equal the last
    value's end)."""
    assert decoder.poison == POISON
    cases = cases_of(group, tname)
    chunks, offsets = optional_chunks(cases)
    w = 8 if tname != "i32" else 4  # (BYTE_ARRAY: the int64 offsets)
    if len(cases) >= 4:
        assert {(o * w) % 16 for o in offsets} == set(range(0, 16, w))
    batch, ref, dcols, counts = decode_both(decoder, chunks)
    check_columns(batch, ref, dcols, counts)
    bad = []
    for i, c in enumerate(cases):
        col = dcols[i]
        first, n_slots = col.n_values, batch.column_slots[i]
        assert first < n_slots
        if tname == "bytes":
            # a BYTE_ARRAY column's value tensor is offsets[0 .. n_slots], all written by design: the scan of
            # the lengths runs over every slot, and the lengths past the count are cleared before the launch.
            # A length stored past the count would move these offsets off the last value's end
            tail = col.values[first * 8:(n_slots + 1) * 8].cpu().numpy().view(np.int64)
            if not (tail == tail[0]).all():
                bad.append((c.id, "a length past the count", first + int(np.nonzero(tail != tail[0])[0][0]) - 1))
            continue
        tail = col.values[first * w:n_slots * w].cpu().numpy()
        if not (tail == POISON).all():
            bad.append((c.id, "first written element past the count", first + int(np.nonzero(tail != POISON)[0][0]) // w))
    assert not bad, bad


ILLEGAL_TYPES = ["i64", "i32", "bytes"]


@pytest.mark.parametrize("tname", ILLEGAL_TYPES)
def test_illegal_pages(decoder, tname):
    """Each illegal page between two legal pages of its column chunk, beside a column of legal pages:
    the first error (code, page, value index) is the oracle's, and the other column decodes as if
    alone."""
    legal = [c for c in legal_cases() if c.ptype == TYPES[tname] and c.group in ("fat", "strings")]
    other_t = "i32" if tname == "i64" else "i64"
    other = chunk_of([c for c in legal_cases() if c.group == "last-block" and c.ptype == TYPES[other_t]][:12])
    alone = pqref.decode_batch(writer.build_batch([other]))
    assert alone.code == 0
    want0 = alone.columns[0]["values"]
    bad = [c for c in illegal_cases() if c.ptype == TYPES[tname]]
    assert bad
    wrong = []
    for i, c in enumerate(bad):
        same = [x for x in legal if x.encoding == c.encoding]
        chunks = [other, chunk_of([same[i % len(same)], c, same[(i + 1) % len(same)]])]
        batch = writer.build_batch(chunks)
        ref = pqref.decode_batch(batch)
        assert ref.code == c.expect and ref.status[1] == len(other.pages) + 1, (c.id, ref.status)
        dcols, st = decoder.decode(decoder.upload(batch), check=False)
        got = (int(st.code), int(st.page), int(st.value_index))
        if got != ref.status:
            wrong.append((c.id, "status", got, "oracle", ref.status))
            continue
        col0 = dcols[0].values[:want0.size * want0.itemsize].cpu().numpy().view(want0.dtype)
        if not np.array_equal(col0, want0):
            wrong.append((c.id, "the legal column changed"))
    assert not wrong, wrong
