"""GPU parity of the DELTA_BYTE_ARRAY value copy (csrc/pqgpu_binary.hip: dba_batch, dba_values,
k_dba_copy, k_dba_tail, k_dba_chain_par, k_dba_chain, k_dba_chunks, k_dba_carry; the lengths pass
k_delta<4, 2> of csrc/pqgpu_kernels.hip) on hand-built pages (dba_build.py, dba_cases.py): prefixes that
no writer derives (ladders over the values of a batch, of a chunk and over the chunk minima of a page,
runs of equal prefixes, prefixes short of the common prefix, whole chunks that inherit everything, empty
values), at the sizes where the copy changes its path: 64-value batches, 256-value chunks, 256 / 257
chunks per page, 2048 / 2049-byte values, 3072 staged suffix bytes, 4096 assembled bytes.

Every comparison is byte for byte, against dba_build.unroll (the values by construction) and against
the oracle: values, offsets, levels, per-page value counts, status. Each case is the last page of its
own column, behind a filler page of 0..15 bytes (the case's first byte at every residue mod 16), in a
byte buffer cut out of a poisoned tensor: the bytes before the buffer, after it and after the column's
last value must still be poison."""
import numpy as np
import pytest
import torch

from oracle import pqref
from pqgpu import abi
from pqgpu.batch import build_batch

import dba_cases as DC

pytestmark = pytest.mark.gpu
POISON = 0xA5
SLACK = 96  # bytes of the byte buffer past the column's last value


class Placed:
    """Columns of a batch whose BYTE_ARRAY byte buffers are views [off, off + capacity) of poisoned
    tensors; capacity: the column's bytes + SLACK, or `cut` (one column)."""

    def __init__(self, decoder, batch, wants, off=0, cut=None):
        assert decoder.poison == POISON
        self.batch, self.wants, self.off = batch, wants, off
        self.cols = decoder.alloc_columns(batch)
        self.big, self.cap, self.joined = [], [], []
        for i, cd in enumerate(batch.columns):
            data = b"".join(wants[i])
            self.joined.append(data)
            if cd["physical_type"] != abi.BYTE_ARRAY:
                self.big.append(None)
                self.cap.append(None)
                continue
            cap = len(data) + SLACK if cut is None else cut
            big = torch.full((off + cap + 64,), POISON, dtype=torch.uint8, device=decoder.device)
            self.cols[i].binary_data = big[off:off + cap]
            assert self.cols[i].binary_data.data_ptr() % 16 == off % 16
            self.big.append(big)
            self.cap.append(cap)

    def repoison(self):
        for col, big in zip(self.cols, self.big):
            col.values.fill_(POISON)
            if col.def_levels is not None:
                col.def_levels.fill_(POISON)
            if big is not None:
                big.fill_(POISON)

    def check_bytes(self, i, n_values):
        """Column i: the bytes below the capacity are the column's first bytes, everything else is poison."""
        want, name = self.joined[i], f"column {i}"
        if self.big[i] is None:  # FIXED_LEN_BYTE_ARRAY: n values of type_length bytes in `values`
            got = self.cols[i].values[:len(want)].cpu().numpy().tobytes()
            assert len(want) == n_values * self.batch.columns[i]["type_length"]
        else:
            big = self.big[i].cpu().numpy()
            off, cap = self.off, self.cap[i]
            assert (big[:off] == POISON).all(), f"{name}: a byte before the buffer changed"
            assert (big[off + cap:] == POISON).all(), f"{name}: a byte after the buffer changed"
            tail = big[off + min(len(want), cap):off + cap]
            assert (tail == POISON).all(), f"{name}: byte {len(want) + int(np.nonzero(tail != POISON)[0][0])} past the " \
                                           f"column's {len(want)} was written"
            got = big[off:off + min(len(want), cap)].tobytes()
            want = want[:cap]
        if got != want:
            g, w = np.frombuffer(got, dtype=np.uint8), np.frombuffer(want, dtype=np.uint8)
            at = int(np.nonzero(g != w)[0][0])
            ends = np.cumsum([len(v) for v in self.wants[i]])
            v = int(np.searchsorted(ends, at, side="right"))
            raise AssertionError(f"{name}: {int((g != w).sum())} bytes differ, first at byte {at}: value {v}, "
                                 f"byte {at - (int(ends[v - 1]) if v else 0)} of {len(self.wants[i][v])}")


def decode_placed(decoder, chunks, wants, dls=None, off=0, names=None):
    """One upload and decode; status, counts, values, offsets and levels against `wants` and the oracle."""
    batch = build_batch(chunks)
    ref = pqref.decode_batch(batch)
    assert ref.status[0] == 0, ref.status
    pl = Placed(decoder, batch, wants, off=off)
    counts = torch.zeros(max(batch.n_pages, 1), dtype=torch.int32, device=decoder.device)
    rc, st, descs = decoder._decode_once(decoder.upload(batch), pl.cols, counts)
    assert (rc, int(st.code), int(st.page), int(st.value_index)) == (0,) + ref.status, st.message
    assert np.array_equal(counts.cpu().numpy().view(np.uint32)[:batch.n_pages], ref.page_value_counts)
    for i, cd in enumerate(batch.columns):
        name = names[i] if names else i
        n = int(descs[i].values_written)
        rv = ref.columns[i]["values"]
        assert n == len(wants[i]) == ref.columns[i]["n_values"], name
        ref_bytes = b"".join(rv) if cd["physical_type"] == abi.BYTE_ARRAY else np.asarray(rv).tobytes()
        assert ref_bytes == pl.joined[i], f"{name}: the oracle and unroll differ"
        try:
            pl.check_bytes(i, n)
        except AssertionError as e:
            raise AssertionError(f"{name}: {e}") from None
        if cd["physical_type"] == abi.BYTE_ARRAY:
            offs = pl.cols[i].values[:(batch.column_slots[i] + 1) * 8].cpu().numpy().view(np.int64)
            want_offs = np.concatenate([[0], np.cumsum([len(v) for v in wants[i]], dtype=np.int64)])
            assert np.array_equal(offs[:n + 1], want_offs), name
            assert np.array_equal(offs[:n + 1], ref.columns[i]["offsets"][:n + 1]), name
            assert (offs[n:] == offs[n]).all(), f"{name}: a length past the count"
        if cd["max_def"] > 0:
            got_dl = pl.cols[i].def_levels[:batch.column_slots[i]].cpu().numpy()
            assert np.array_equal(got_dl, dls[i]) and np.array_equal(got_dl, ref.columns[i]["def_levels"]), name
    return pl


def columns_for(cases, optional=0):
    out = [DC.column_of(c, k=None if (c.before is not None or c.ptype != abi.BYTE_ARRAY) else i % 16, optional=optional, seed=i)
           for i, c in enumerate(cases)]
    return [o[0] for o in out], [o[1] for o in out], [o[2] for o in out]


@pytest.mark.parametrize("group", [g for g in DC.GROUPS if g != "carry"])
def test_legal_groups(decoder, group):
    cases = DC.legal_cases(group)
    chunks, wants, dls = columns_for(cases)
    decode_placed(decoder, chunks, wants, dls, names=[c.name for c in cases])


def test_vb_pages_side_by_side(decoder):
    """One column of pages whose longest value is 2048, 2049, 2047, 2049, 2048, 2049 bytes: neighbouring
    pages take the chunk-parallel and the serial copy; beside it a 256-chunk page followed by a
    257-chunk page in one column (k_dba_chain_par and k_dba_chain in one launch)."""
    order = ["vb-2048", "vb-2049-next-2049", "vb-2047", "vb-2049-next-2048", "vb-2048", "vb-2049-next-1"]
    chains = ["chain_par-ladder_up-256", "chain_serial-ladder_up-65537", "chain_par-ladder_down-256"]
    chunks, wants = [], []
    for names in (order, chains):
        ch, want = None, []
        for nm in names:
            one, vals, _ = DC.column_of(DC.case(nm))
            if ch is None:
                ch = one
            else:
                ch.pages += one.pages
            want += vals
        ch.n_values_hint = len(want)
        chunks.append(ch)
        wants.append(want)
    decode_placed(decoder, chunks, wants, names=["vb", "chains"])


@pytest.mark.parametrize("version", [2, 1], ids=["v2", "v1"])
@pytest.mark.parametrize("group", ["batch", "tail", "lds"])
def test_optional_columns(decoder, group, version):
    """The same pages behind definition levels with about 20 % nulls (V2 and V1 pages)."""
    cases = DC.legal_cases(group)
    chunks, wants, dls = columns_for(cases, optional=version)
    decode_placed(decoder, chunks, wants, dls, names=[c.name for c in cases])


@pytest.mark.parametrize("off", [1, 4, 8])
def test_unaligned_destination(decoder, off):
    """binary_data 1, 4 and 8 bytes into a 16-byte aligned tensor: dba_batch's 16-byte blocks fall back
    to dword and byte stores; nothing outside the view changes."""
    cases = [DC.case(n) for n in ("batch-ladder_up-129", "batch-short_of_common-128", "lds-batch-total-4097-at-2",
                                  "lds-chunk-suffix-3073", "vb-2049-next-2048", "vb-2048")]
    chunks, wants, dls = columns_for(cases)
    decode_placed(decoder, chunks, wants, dls, off=off, names=[c.name for c in cases])


def first_at_least(lengths, start, least=2):
    return next(i for i in range(start, len(lengths)) if lengths[i] >= least)


SHORT = [  # (case, value the capacity ends in (-k: the first of >= 2 bytes from value k on), bytes of it kept)
    ("chain_par-ladder_down-256", 2 * 256 - 1, 30),       # chunk 1's last value
    ("chain_par-ladder_down-256", 256 * 256 - 1, 30),     # chunk 255's last value
    ("chain_par-ladder_up-256", "last", 1),               # the page's last value (a partial chunk 255)
    ("chain_serial-ladder_up-65537", 101 * 256 - 1, 30),  # a chunk's last value of a 257-chunk page
    ("batch-random-129", -30, 1),                         # the middle of a batch
    ("lds-batch-total-4097-at-2", 256 + 128 + 30, 40),    # inside the batch that takes the per-value loop
    ("vb-2049-next-2048", 130, 1000),                     # inside the 2049-byte value
    ("vb-2049-next-2048", 131, 1000),                     # inside the value after it
]


@pytest.mark.parametrize("name,value,keep", SHORT, ids=[f"{n}-value{v}" for n, v, _ in SHORT])
def test_short_capacity(decoder, name, value, keep):
    """binary_capacity ends inside a value: the call reports the bytes needed, the bytes below the
    capacity are the column's first bytes, nothing past it is written."""
    c = DC.case(name)
    ch, want, _ = DC.column_of(c, k=5)
    lens = [len(v) for v in want]
    if value == "last":
        v = len(lens) - 1
    else:
        v = 1 + (first_at_least(lens[1:], -value) if value < 0 else value)  # (the filler page's value is value 0)
    assert lens[v] > keep
    cap = sum(lens[:v]) + keep
    batch = build_batch([ch])
    pl = Placed(decoder, batch, [want], off=16, cut=cap)
    rc, st, _ = decoder._decode_once(decoder.upload(batch), pl.cols, None)
    assert rc == abi.ERR_INVALID_ARG and st.message.startswith(b"binary capacity"), (rc, st.message)
    assert int(st.value_index) == sum(lens)
    pl.check_bytes(0, len(want))


def test_plan_relaunch(decoder):
    """A plan over the 256-chunk pages launched twice, every output poisoned in between (dba_meta and
    PageWork::reserved are rewritten by each launch)."""
    cases = [DC.case("chain_par-ladder_down-256"), DC.case("chain_par-ladder_up-256"), DC.case("vb-2049-next-1")]
    chunks, wants, _ = columns_for(cases)
    batch = build_batch(chunks)
    pl = Placed(decoder, batch, wants)
    plan = decoder.plan(decoder.upload(batch), pl.cols)
    try:
        for _ in range(2):
            pl.repoison()
            decoder.stream.wait_stream(torch.cuda.current_stream(decoder.device))  # the fills first
            plan.launch()
            rc, st = plan.sync()
            assert rc == 0, st.message
            for i in range(len(cases)):
                pl.check_bytes(i, len(wants[i]))
                offs = pl.cols[i].values[:(len(wants[i]) + 1) * 8].cpu().numpy().view(np.int64)
                assert np.array_equal(offs, np.concatenate([[0], np.cumsum([len(v) for v in wants[i]], dtype=np.int64)]))
    finally:
        plan.close()


def test_carry_pages(decoder):
    """PQG_PAGE_DBA_CARRY pages whose first prefix is 0 or the whole last value of the page before
    (0, 1, 2047, 2048, 2049 bytes: over 2048 k_dba_carry reads it back from the output), one with a
    null-only page between the two."""
    cases = DC.legal_cases("carry")
    chunks, wants, dls = columns_for(cases)
    decode_placed(decoder, chunks, wants, dls, names=[c.name for c in cases])


def status_of(decoder, batch):
    ref = pqref.decode_batch(batch)
    _, st = decoder.decode(decoder.upload(batch), check=False)
    return (int(st.code), int(st.page), int(st.value_index)), ref.status


def test_carry_first_prefix_too_long(decoder):
    wrong = []
    for c in DC.illegal_cases("carry"):
        ch, _, _ = DC.column_of(c)
        got, ref = status_of(decoder, build_batch([ch]))
        if not (got == ref == (abi.ERR_CORRUPT, 1, 0)):
            wrong.append((c.name, got, ref))
    assert not wrong, wrong


def test_illegal_pages(decoder):
    """A prefix longer than the previous value (at a batch's and a chunk's first and last value, in the
    last chunk of a 257-chunk page, after an empty value), a negative prefix, suffix bytes one short:
    the oracle's (code, page, value index), which is the one the page was built to fail at."""
    wrong = []
    for c in DC.illegal_cases("illegal"):
        ch, _, _ = DC.column_of(c, k=3)
        got, ref = status_of(decoder, build_batch([ch]))
        if not (got == ref == (c.bad[0], 1, c.bad[1])):
            wrong.append((c.name, got, ref))
    assert not wrong, wrong
