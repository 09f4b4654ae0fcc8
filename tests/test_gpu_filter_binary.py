"""Record filters on FIXED_LEN_BYTE_ARRAY, INT96 and DECIMAL-on-BYTE_ARRAY columns on the GPU (pqg_filter_run
with a pqg_filter_create_typed filter) against tests/filter_binary_ref.py, bit for bit: the bitmap with its
zero tail bits, the count and the ordered row ids, into outputs pre-filled with 0xA5.

The columns are device tensors laid out as pqg_decode leaves them (dense elements of type_length or 12 bytes,
one definition byte per row); the end-to-end case decodes a writer chunk instead. 4,096 + 65 rows are two
tiles with a ragged last step. Every case asserts on the REFERENCE's result that it selects between 5 % and
95 % of the rows, so none can pass on an empty or a full bitmap. The values make that possible: a tenth are 0,
a tenth are 3 (the pivots of the literals), the rest small integers and full-width random values, from a pool
small enough for the byte-loop reference to stay quick.

INT96 has the signed-integer comparator only (the reference has no other; the ABI refuses the rest)."""
import numpy as np
import pytest
import torch

import filter_binary_ref as B
import filter_ref as R
from pqgpu import abi
from pqgpu import decoder as D
from pqgpu import filter as F
from tools.synth import writer

pytestmark = pytest.mark.gpu

T = abi.FILTER_TILE_ROWS
N = T + 65
FLBA, I96, BA = abi.FIXED_LEN_BYTE_ARRAY, abi.INT96, abi.BYTE_ARRAY
POISON = 0xA5
POISON64 = int(np.array([POISON] * 8, dtype=np.uint8).view(np.int64)[0])
CMP_OPS = [F.eq, F.not_eq, F.lt, F.lt_eq, F.gt, F.gt_eq]


# ---- data ---------------------------------------------------------------------------------------------------

def draw_fixed(rng, width, n):
    """n values of `width` bytes: 10 % zero, 10 % three, 40 % small integers, 40 % random bytes (64 distinct)."""
    lo, hi = (-50, 50) if width > 1 else (-128, 127)
    small = [F.decimal_bytes(int(v), width) for v in rng.integers(lo, hi + 1, size=48)]
    rand = [bytes(rng.integers(0, 256, size=width, dtype=np.uint8)) for _ in range(64)]
    zero, three = F.decimal_bytes(0, width), F.decimal_bytes(3, width)
    kind = rng.random(n)
    pick = rng.integers(0, 1 << 30, size=n)
    return [zero if k < 0.1 else three if k < 0.2 else small[p % 48] if k < 0.6 else rand[p % 64] for k, p in zip(kind, pick)]


def levels(rng, n, all_null_from=None):
    dl = np.where(rng.random(n) < 0.1, 0, 1).astype(np.uint8)
    if all_null_from is not None:
        dl[all_null_from:] = 0
    return dl


def fixed_column(dec, t, width, values, dl=None, offset=0):
    """A DeviceColumn of dense `width`-byte elements; offset: the byte offset of `values` in its allocation."""
    raw = np.frombuffer(b"".join(values), dtype=np.uint8)
    buf = torch.full((offset + raw.size + 24,), POISON, dtype=torch.uint8, device=dec.device)
    buf[offset:offset + raw.size] = torch.from_numpy(raw.copy()).to(dec.device)
    col = D.DeviceColumn(t, buf[offset:], None if dl is None else torch.from_numpy(dl).to(dec.device),
                         type_length=width if t == FLBA else 0)
    col.n_values, col.max_def = len(values), 0 if dl is None else 1
    return col


def binary_column(dec, values, dl=None):
    """A BYTE_ARRAY DeviceColumn: int64 offsets[n + 1] and the bytes."""
    offs = np.concatenate([[0], np.cumsum([len(v) for v in values])]).astype(np.int64)
    data = np.frombuffer(b"".join(values) + bytes([POISON]) * 16, dtype=np.uint8)
    col = D.DeviceColumn(BA, torch.from_numpy(offs.view(np.uint8).copy()).to(dec.device),
                         None if dl is None else torch.from_numpy(dl).to(dec.device),
                         binary_data=torch.from_numpy(data.copy()).to(dec.device))
    col.n_values, col.max_def = len(values), 0 if dl is None else 1
    return col


def ref_column(t, values, dl=None):
    return R.RefColumn(t, values, dl, 0 if dl is None else 1)


# ---- running and comparing ----------------------------------------------------------------------------------

def run(dec, pred, dev, n_rows, filter_fn=None):
    n_words = (n_rows + 63) // 64
    words = torch.full((n_words + 2,), POISON64, dtype=torch.int64, device=dec.device)
    ids = torch.full((n_rows + 2,), POISON64, dtype=torch.int64, device=dec.device)
    result = torch.full((16,), POISON, dtype=torch.uint8, device=dec.device)
    sel = (filter_fn or dec.filter)(pred, dev, n_rows, row_ids=True, capacity=n_rows, out=(words, ids, result))
    return words, ids, sel


def compare(words, ids, sel, want, what):
    n_rows = len(want)
    n_words = (n_rows + 63) // 64
    want_ids = np.flatnonzero(want).astype(np.int64)
    assert sel.count == want_ids.size, what
    got = words.cpu().numpy()
    assert np.array_equal(got[:n_words].view(np.uint64), R.bitmap_words(want)), what  # tail bits included
    assert (got[n_words:] == POISON64).all(), what
    got_ids = ids.cpu().numpy()
    assert np.array_equal(got_ids[:want_ids.size], want_ids), what
    assert (got_ids[want_ids.size:] == POISON64).all(), what


def check(dec, pred, dev, ref, n_rows, bounded=True):
    want = B.evaluate_rows(pred, ref, n_rows)
    share = want.sum() / max(n_rows, 1)
    print(f"{pred!r}: {int(want.sum())} of {n_rows}")
    if bounded:
        assert 0.05 <= share <= 0.95, (repr(pred), share)
    compare(*run(dec, pred, dev, n_rows), want, repr(pred))
    return want


def signed_literal(length):
    """The pivot as `length` bytes: 3, or 0 when there is no byte to hold it."""
    return F.decimal_bytes(3, length) if length else b""


def literal_lengths(width):
    return sorted({0, width - 1, width, width + 1, 40})


def signed_cases(c, width):
    """Every op at every literal length, and sets of 3 and 12 with comparator-equal members."""
    for length in literal_lengths(width):
        for op in CMP_OPS:
            yield op(c, signed_literal(length))
    three = [signed_literal(width), signed_literal(width + 2), b"\x00" * 5]
    twelve = [F.decimal_bytes(v) for v in (3, -1, 7, -20, 11, 19, -33, 2)] + [b"", b"\x00\x00", signed_literal(40),
                                                                             b"\xff" * 9]
    for mk in (F.in_, F.not_in):
        yield mk(c, three)
        yield mk(c, twelve)


def unsigned_cases(c, width, values):
    """Every op at the column's width; the ordering ops at the other lengths too (equality with a literal of
    another length is false by definition); sets of 3 and 12 that hold the other lengths beside the pivots."""
    ranked = sorted(set(values))
    pivot = ranked[int(len(ranked) * 0.4)]
    for op in CMP_OPS:
        yield op(c, F.decimal_bytes(3, width)) if op in (F.eq, F.not_eq) else op(c, pivot)
    for lit in (pivot[:width - 1], pivot + b"\x00", pivot + b"\x00" * (40 - width)):
        if lit:
            for op in (F.lt, F.lt_eq, F.gt, F.gt_eq):
                yield op(c, lit)
    three = [F.decimal_bytes(3, width), F.decimal_bytes(3, width), b""]
    twelve = [F.decimal_bytes(v, width) for v in (3, 0, 3)] + [b"", pivot[:width - 1], pivot + b"\x00", b"\xff" * 40] + ranked[:5]
    for mk in (F.in_, F.not_in):
        yield mk(c, three)
        yield mk(c, twelve)


# ---- flat columns: widths, nulls, alignment, orders, ops, literal lengths ---------------------------------------

SHAPES = [(FLBA, w) for w in (1, 2, 3, 5, 16, 17, 20)] + [(I96, 12)]
# an INT96 column is 4-byte aligned by the ABI: no "offset1" layout for it
LAYOUTS = [(t, w, lay) for t, w in SHAPES for lay in ("required", "nullable", "offset1") if not (t == I96 and lay == "offset1")]


@pytest.mark.parametrize("t,width,layout", LAYOUTS, ids=lambda x: str(x))
def test_fixed_width_columns(decoder, t, width, layout):
    rng = np.random.default_rng(1000 * width + len(layout))
    # nullable: about 10 % nulls in the first tile, and the second tile (the last 65 rows) all null
    dl = levels(rng, N, all_null_from=T) if layout == "nullable" else None
    values = draw_fixed(rng, width, N if dl is None else int(dl.sum()))
    dev = [fixed_column(decoder, t, width, values, dl, offset=1 if layout == "offset1" else 0)]
    ref = [ref_column(t, values, dl)]
    for pred in signed_cases(F.col(0, order="signed_integer"), width):
        check(decoder, pred, dev, ref, N)
    if t == FLBA:
        for pred in unsigned_cases(F.col(0, order="unsigned_bytes"), width, values):
            check(decoder, pred, dev, ref, N)


def test_63_rows(decoder):
    rng = np.random.default_rng(63)
    dl = levels(rng, 63)
    values = draw_fixed(rng, 5, int(dl.sum()))
    dev, ref = [fixed_column(decoder, FLBA, 5, values, dl, offset=1)], [ref_column(FLBA, values, dl)]
    c = F.col(0, order="signed_integer")
    for pred in (F.lt(c, b"\x03"), F.eq(c, b""), F.not_in(c, [b"\x00\x03", b"\x00"]), F.gt_eq(c, signed_literal(40))):
        check(decoder, pred, dev, ref, 63)


F16_SPECIAL = [0x0000, 0x8000, 0x7C00, 0xFC00, 0x7E00, 0x7E01, 0xFE00, 0x7C01, 0xFFFF, 0x0001, 0x8001, 0x03FF]


def test_float16(decoder):
    """±0, both infinities, NaNs of several payloads and signs, subnormals, and random normals."""
    rng = np.random.default_rng(16)
    kind, pick = rng.random(N), rng.integers(0, 1 << 16, size=N)
    bits = [F16_SPECIAL[p % 12] if k < 0.8 else int(p) for k, p in zip(kind, pick)]
    values = [int(b).to_bytes(2, "little") for b in bits]
    for dl in (None, levels(rng, N, all_null_from=T)):
        vals = values if dl is None else values[:int(dl.sum())]
        dev, ref = [fixed_column(decoder, FLBA, 2, vals, dl, offset=1)], [ref_column(FLBA, vals, dl)]
        c = F.col(0, order="float16")
        h = lambda b: int(b).to_bytes(2, "little")
        for lit in (h(0x0000), h(0x8000), h(0x0001)):
            for op in CMP_OPS:
                check(decoder, op(c, lit), dev, ref, N)
        for op in (F.eq, F.not_eq, F.lt, F.gt_eq):  # nothing is above NaN: gt / ltEq are constant
            check(decoder, op(c, h(0x7FFF)), dev, ref, N)
        for mk in (F.in_, F.not_in):
            check(decoder, mk(c, [h(0x8000), h(0xFC00), h(0x7D55)]), dev, ref, N)
            check(decoder, mk(c, [h(x) for x in (0x0000, 0x3C00, 0xBC00, 0x7C00, 0x0001, 0x8001, 0x03FF, 0x4000, 0xC000,
                                                 0x7E00, 0xFE01, 0x5640)]), dev, ref, N)


def draw_decimal_binary(rng, n):
    """Integers as big-endian two's complement of 0 .. 20 bytes (0 also as the empty value)."""
    out = []
    for k, p in zip(rng.random(n), rng.integers(0, 1 << 30, size=n)):
        v = 0 if k < 0.1 else 3 if k < 0.2 else int(p % 101) - 50 if k < 0.6 else (int(p) - (1 << 29)) << int(p % 90)
        least = len(F.decimal_bytes(v))
        length = least + int(p >> 8) % (21 - least)
        out.append(b"" if v == 0 and (p & 1) else F.decimal_bytes(v, max(length, 1)))
    return out


@pytest.mark.parametrize("nullable", [False, True])
def test_decimal_on_byte_array(decoder, nullable):
    """Value lengths 0 .. 20 under the signed order: the 128-bit keys up to 16 bytes, the byte-wise path above,
    in one column. Declared the old way the same column keeps the unsigned byte order."""
    rng = np.random.default_rng(20 + nullable)
    dl = levels(rng, N, all_null_from=T) if nullable else None
    values = draw_decimal_binary(rng, N if dl is None else int(dl.sum()))
    assert {len(v) for v in values} == set(range(21))
    dev, ref = [binary_column(decoder, values, dl)], [ref_column(BA, values, dl)]
    for pred in signed_cases(F.col(0, order="signed_integer"), 8):
        check(decoder, pred, dev, ref, N)
    c = F.col(0, order="signed_integer")
    check(decoder, F.lt(c, F.decimal_bytes(-(1 << 60), 14)), dev, ref, N)  # a 14-byte literal
    check(decoder, F.gt(c, b"\x00" * 30 + b"\x03"), dev, ref, N)       # 31 bytes, 1 significant
    check(decoder, F.lt(c, b"\x7f" + b"\x00" * 16), dev, ref, N, bounded=False)  # 17 significant bytes: no keys
    old = check(decoder, F.lt(F.col(0), b"\x03"), dev, ref, N)
    new = check(decoder, F.lt(c, b"\x03"), dev, ref, N)
    assert (old != new).any()  # FF (-1) is above 03 as unsigned bytes and below it as an integer


def test_combined_with_other_leaves(decoder):
    """and / or with an int64 leaf and with an unsigned-bytes leaf, not() above a signed leaf."""
    rng = np.random.default_rng(31)
    dl = levels(rng, N)
    dec_vals = draw_fixed(rng, 16, int(dl.sum()))
    ints = rng.integers(-20, 20, size=N).astype(np.int64)
    uuid = draw_fixed(rng, 16, N)
    dev = [fixed_column(decoder, FLBA, 16, dec_vals, dl),
           fixed_column(decoder, abi.INT64, 8, [v.tobytes() for v in ints]),
           fixed_column(decoder, FLBA, 16, uuid, offset=1)]
    ref = [ref_column(FLBA, dec_vals, dl), ref_column(abi.INT64, ints), ref_column(FLBA, uuid)]
    d, u = F.col(0, order="signed_integer"), F.col(2, order="unsigned_bytes")
    for pred in (F.and_(F.lt(d, b"\x03"), F.gt_eq(F.col(1), -5)),
                 F.or_(F.eq(d, b""), F.lt(F.col(1), -10)),
                 F.not_(F.lt(d, b"\x03")),  # gtEq: false on a null row
                 F.not_(F.or_(F.in_(d, [b"\x03", b"\x00\x00"]), F.not_(F.gt(F.col(1), 0)))),
                 F.and_(F.not_eq(d, None), F.or_(F.gt(u, uuid[0]), F.eq(d, None))),
                 F.or_(F.eq(d, None), F.and_(F.lt(d, F.decimal_bytes(-3, 16)), F.lt_eq(u, uuid[1])))):
        check(decoder, pred, dev, ref, N)


def test_wrong_physical_type_is_refused(decoder):
    """The run's column must be of the declared type."""
    from pqgpu import native
    values = draw_fixed(np.random.default_rng(1), 4, 100)
    flt = F.Filter(F.lt(F.col(0, order="signed_integer"), b"\x03"), [fixed_column(decoder, FLBA, 4, values)])
    with pytest.raises(native.PqgError) as e:
        decoder.filter(flt, [fixed_column(decoder, abi.INT32, 4, values)], 100)
    assert e.value.code == abi.ERR_INVALID_ARG
    flt.close()


# ---- end to end: writer -> decode -> filter -> take -----------------------------------------------------------

def test_decode_filter_take_decimal(decoder):
    rng = np.random.default_rng(77)
    n = T + 65
    dl = levels(rng, n)
    values = draw_fixed(rng, 5, int(dl.sum()))
    price = writer.write_column_chunk(FLBA, values, abi.PLAIN, def_levels=dl, max_def=1, type_length=5, page_rows=1500)
    qty = rng.integers(0, 100, size=n).astype(np.int32)
    cols, _ = decoder.decode(decoder.upload(writer.build_batch([price, writer.write_column_chunk(abi.INT32, qty, abi.PLAIN)])))
    assert cols[0].physical_type == FLBA and cols[0].type_length == 5
    ref = [ref_column(FLBA, values, dl), ref_column(abi.INT32, qty)]
    pred = F.and_(F.lt(F.col(0, order="signed_integer"), F.decimal_bytes(3)), F.gt(F.col(1), 10))
    want = B.evaluate_rows(pred, ref, n)
    assert 0.05 <= want.mean() <= 0.95
    sel = decoder.filter(pred, cols, n)
    taken = decoder.take(sel, cols)
    assert sel.count == taken.n_rows == int(want.sum())
    assert np.array_equal(sel.row_ids.cpu().numpy(), np.flatnonzero(want))
    valid = dl == 1
    dense = np.cumsum(valid) - valid
    kept = [values[int(i)] for i in dense[want & valid]]
    assert taken.columns[0].numpy().tobytes() == b"".join(kept)
    assert np.array_equal(taken.columns[0].def_levels.cpu().numpy()[:taken.n_rows], dl[want])
    assert np.array_equal(taken.columns[1].numpy(), qty[want])
