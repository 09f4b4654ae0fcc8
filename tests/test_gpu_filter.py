"""pqg_filter_run on the GPU against tests/filter_ref.py, bit for bit: the bitmap (with its zero tail
bits), the count and the ordered row ids. The inputs are real decodes of tools.synth.writer chunks, so
the dense-values + definition-levels layout is the decoder's own; the outputs are pre-filled with 0xA5.
Row counts below a decoded column's are prefixes of it: the dense values of the first n rows are the
first values, and n_values is the number of those rows that hold one."""
import copy

import numpy as np
import pytest
import torch

import filter_ref as R
from pqgpu import abi, native
from pqgpu import filter as F
from test_filter_ref import rewriter_complex
from tools.synth import writer

pytestmark = pytest.mark.gpu

T = abi.FILTER_TILE_ROWS
N_MAIN = 3 * T + 17
SCAN_ROUND = 1024  # tiles k_filter_scan takes per loop iteration (256 threads x 4)
# column order of the main data set: the reference's intColumn / doubleColumn first
I32, F64, BOOL, I64, F32, BIN = range(6)
MAIN_TYPES = [abi.INT32, abi.DOUBLE, abi.BOOLEAN, abi.INT64, abi.FLOAT, abi.BYTE_ARRAY]
MAIN_MAX_DEF = [0, 1, 1, 3, 0, 1]


def draw_values(rng, t, n):
    """Half edge values (filter_ref.EDGE: -0.0, NaNs of both signs, extremes, prefixes, high bytes),
    half random ones near them."""
    pool = R.EDGE[t]
    edge = [pool[int(x)] for x in rng.integers(0, len(pool), size=n)]
    pick = rng.random(n) < 0.5
    if t == abi.BYTE_ARRAY:
        rnd = [bytes(rng.integers(0, 256, size=int(rng.integers(0, 12)), dtype=np.uint8)) for _ in range(n)]
        return [e if p else r for e, r, p in zip(edge, rnd, pick)]
    if t == abi.BOOLEAN:
        return np.array(edge, dtype=np.uint8)
    dt = abi.numpy_dtype(t)
    rnd = rng.integers(-20, 20, size=n).astype(dt) if t in (abi.INT32, abi.INT64) else (rng.standard_normal(n) * 2).astype(dt)
    return np.where(pick, np.array(edge, dtype=dt), rnd)


class Data:
    """Decoded device columns + the reference's view of the same data."""

    def __init__(self, dec, specs, n_rows, page_rows=5000):
        """specs: (physical_type, max_def, def_levels or None, dense values)."""
        chunks = []
        self.ref = []
        for t, max_def, dl, vals in specs:
            chunks.append(writer.write_column_chunk(t, vals, abi.PLAIN, def_levels=dl if max_def else None,
                                                    max_def=max_def, page_rows=page_rows))
            self.ref.append(R.RefColumn(t, vals, dl if max_def else None, max_def))
        self.n_rows = n_rows
        self.dev, _ = dec.decode(dec.upload(writer.build_batch(chunks)))

    def prefix(self, n):
        """(device columns, reference columns) of the first n rows."""
        if n == self.n_rows:
            return self.dev, self.ref
        dev, ref = [], []
        for d, r in zip(self.dev, self.ref):
            d2 = copy.copy(d)
            d2.n_values = int(r.valid(n).sum())
            dev.append(d2)
            ref.append(R.RefColumn(r.physical_type, r.values, r.def_levels, r.max_def))
        return dev, ref


def random_levels(rng, n, max_def, null_fraction=0.1):
    dl = np.full(n, max_def, dtype=np.uint8)
    nulls = rng.random(n) < null_fraction
    dl[nulls] = rng.integers(0, max_def, size=int(nulls.sum()))
    return dl


@pytest.fixture(scope="module")
def main(decoder):
    rng = np.random.default_rng(2024)
    specs = []
    for t, md in zip(MAIN_TYPES, MAIN_MAX_DEF):
        dl = random_levels(rng, N_MAIN, md) if md else None
        k = N_MAIN if dl is None else int((dl == md).sum())
        specs.append((t, md, dl, draw_values(rng, t, k)))
    return Data(decoder, specs, N_MAIN)


POISON = 0xA5
POISON64 = int(np.array([POISON] * 8, dtype=np.uint8).view(np.int64)[0])


def run(dec, pred, dev, n_rows, row_ids=True, capacity=None):
    """One pqg_filter_run into poisoned outputs -> (bitmap words, padding intact, count, row ids, ids tensor, selection)."""
    n_words = (n_rows + 63) // 64
    cap = n_rows if capacity is None else capacity
    words = torch.full((n_words + 2,), POISON64, dtype=torch.int64, device=dec.device)
    ids = torch.full((cap + 2,), POISON64, dtype=torch.int64, device=dec.device) if row_ids else None
    result = torch.full((16,), POISON, dtype=torch.uint8, device=dec.device)
    sel = dec.filter(pred, dev, n_rows, row_ids=row_ids, capacity=cap, out=(words, ids, result))
    return words, ids, sel


def check(dec, pred, dev, ref, n_rows, rows_ref=False, capacity=None, row_ids=True):
    words, ids, sel = run(dec, pred, dev, n_rows, row_ids=row_ids, capacity=capacity)
    want = (R.evaluate_rows if rows_ref else R.evaluate)(pred, ref, n_rows)
    want_ids = np.flatnonzero(want).astype(np.int64)
    n_words = (n_rows + 63) // 64
    assert sel.count == want_ids.size, repr(pred)
    got = words.cpu().numpy()
    assert np.array_equal(got[:n_words].view(np.uint64), R.bitmap_words(want)), repr(pred)  # tail bits included
    assert (got[n_words:] == POISON64).all()
    if row_ids:
        cap = n_rows if capacity is None else capacity
        k = min(cap, want_ids.size)
        got_ids = ids.cpu().numpy()
        assert np.array_equal(got_ids[:k], want_ids[:k]), repr(pred)
        assert (got_ids[k:] == POISON64).all()  # nothing past the count / the capacity
        assert np.array_equal(sel.row_ids.cpu().numpy(), want_ids[:k])
    return want_ids.size


# ---- row counts ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, T - 1, T, T + 1, N_MAIN])
def test_row_counts(decoder, main, n):
    dev, ref = main.prefix(n)
    pred = F.or_(F.and_(F.lt_eq(F.col(I32), 3), F.not_eq(F.col(F64), 1.5)),
                 F.or_(F.eq(F.col(I64), None), F.gt(F.col(BIN), b"ab")))
    check(decoder, pred, dev, ref, n, rows_ref=n <= 65)
    check(decoder, F.not_eq(F.col(BOOL), True), dev, ref, n, rows_ref=n <= 65)


def test_more_tiles_than_one_scan_round(decoder):
    """1,024 tiles + 5 rows: k_filter_scan loops, over the rank counts and over the selected counts."""
    n = SCAN_ROUND * T + 5
    rng = np.random.default_rng(3)
    dl = (rng.random(n) < 0.9).astype(np.uint8)
    vals = rng.integers(-100, 100, size=int(dl.sum())).astype(np.int32)
    data = Data(decoder, [(abi.INT32, 1, dl, vals)], n, page_rows=1 << 20)
    got = check(decoder, F.lt(F.col(0), -80), data.dev, data.ref, n)
    assert got > 0
    check(decoder, F.not_eq(F.col(0), 0), data.dev, data.ref, n, capacity=1000)


# ---- null patterns ---------------------------------------------------------------------------------------

def null_patterns(n, max_def, rng):
    below = lambda k: rng.integers(0, max_def, size=k).astype(np.uint8)  # any level under max_def is null
    none = np.full(n, max_def, dtype=np.uint8)
    all_null = below(n)
    ten = random_levels(rng, n, max_def)
    packed = below(n)          # non-null exactly at the last row of a tile and the first of the next,
    for r in (63, 64, T - 1, T, 2 * T - 1, 2 * T, n - 1):  # of a wave step and the next, and at the end
        packed[r] = max_def
    return {"none": none, "all": all_null, "ten_percent": ten, "packed": packed}


@pytest.mark.parametrize("max_def", [1, 3])
@pytest.mark.parametrize("pattern", ["none", "all", "ten_percent", "packed"])
@pytest.mark.parametrize("t", [abi.INT64, abi.BYTE_ARRAY, abi.BOOLEAN])
def test_null_patterns(decoder, t, pattern, max_def):
    n = 2 * T + 70
    rng = np.random.default_rng(max_def * 7 + len(pattern))
    dl = null_patterns(n, max_def, rng)[pattern]
    vals = draw_values(rng, t, int((dl == max_def).sum()))
    data = Data(decoder, [(t, max_def, dl, vals)], n)
    c = F.col(0)
    lit = R.EDGE[t][1]
    for pred in (F.eq(c, lit), F.not_eq(c, lit), F.eq(c, None), F.not_eq(c, None), F.not_in(c, [lit, R.EDGE[t][0]]),
                 F.not_(F.eq(c, lit))):
        check(decoder, pred, data.dev, data.ref, n)
    if t != abi.BOOLEAN:
        check(decoder, F.not_(F.lt(c, lit)), data.dev, data.ref, n)  # gtEq: false on null rows


def test_missing_column(decoder, main):
    """A column the file does not have is null in every row (TestFiltersWithMissingColumns)."""
    dev = list(main.dev) + [F.MissingColumn(abi.INT64, 1), F.MissingColumn(abi.BYTE_ARRAY, 2)]
    ref = list(main.ref) + [R.RefColumn(abi.INT64, max_def=1, missing=True), R.RefColumn(abi.BYTE_ARRAY, max_def=2, missing=True)]
    m, mb = F.col(6), F.col(7)
    for pred in (F.eq(m, 5), F.not_eq(m, 5), F.eq(m, None), F.not_eq(m, None), F.lt(m, 5), F.in_(m, [1, None]),
                 F.not_in(mb, [b"a"]), F.gt_eq(mb, b""),
                 F.and_(F.not_eq(m, 5), F.lt(F.col(I32), 0)), F.or_(F.eq(mb, b"a"), F.not_(F.gt(m, 0)))):
        check(decoder, pred, dev, ref, N_MAIN)


# ---- leaves ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", range(6), ids=[abi.TYPE_NAMES[t] for t in MAIN_TYPES])
def test_every_op(decoder, main, c):
    t = MAIN_TYPES[c]
    column = F.col(c)
    ops = [F.eq, F.not_eq] + ([] if t == abi.BOOLEAN else [F.lt, F.lt_eq, F.gt, F.gt_eq])
    hits = 0
    for lit in R.EDGE[t]:  # the float edge values, prefixes and high bytes as literals (and as data)
        for mk in ops:
            hits += check(decoder, mk(column, lit), main.dev, main.ref, N_MAIN)
    for mk in (F.eq, F.not_eq):
        hits += check(decoder, mk(column, None), main.dev, main.ref, N_MAIN)
    for mk in (F.in_, F.not_in):
        hits += check(decoder, mk(column, R.EDGE[t][:2]), main.dev, main.ref, N_MAIN)
    assert hits > 0


def set_members(rng, t, k, values):
    """k distinct literals, some of them present in the data."""
    out, seen = [], set()
    while len(out) < k:
        if not out or rng.random() < 0.3:
            v = values[int(rng.integers(0, len(values)))]
        elif t == abi.BYTE_ARRAY:
            v = bytes(rng.integers(0, 256, size=int(rng.integers(0, 12)), dtype=np.uint8))
        elif t in (abi.INT32, abi.INT64):
            v = int(rng.integers(-400, 400))
        else:
            v = abi.numpy_dtype(t).type(rng.standard_normal() * 2)
        key = v if t == abi.BYTE_ARRAY else R.key_array(t, False, np.array([v], dtype=abi.numpy_dtype(t)))[0]
        if key not in seen:
            seen.add(key)
            out.append(v)
    return out


@pytest.mark.parametrize("k", [1, 8, 9, 300])
@pytest.mark.parametrize("c", [I32, F64, I64, F32, BIN])
def test_in_sets(decoder, main, c, k):
    """Linear probing up to 8 members, binary search from 9 on."""
    t = MAIN_TYPES[c]
    rng = np.random.default_rng(100 * c + k)
    members = set_members(rng, t, k, main.ref[c].values)
    n_in = check(decoder, F.in_(F.col(c), members), main.dev, main.ref, N_MAIN)
    n_not = check(decoder, F.not_in(F.col(c), members), main.dev, main.ref, N_MAIN)
    assert n_in + n_not == N_MAIN and n_in > 0
    n_null = check(decoder, F.in_(F.col(c), members + [None]), main.dev, main.ref, N_MAIN)  # a null member
    assert n_null == int((~main.ref[c].valid(N_MAIN)).sum())
    check(decoder, F.not_in(F.col(c), [None] + members), main.dev, main.ref, N_MAIN)
    if t in (abi.INT32, abi.INT64):
        check(decoder, F.in_(F.col(c, unsigned=True), members), main.dev, main.ref, N_MAIN)


def test_boolean_sets(decoder, main):
    for members in ([True], [False, True], [False, None]):
        check(decoder, F.in_(F.col(BOOL), members), main.dev, main.ref, N_MAIN)
        check(decoder, F.not_in(F.col(BOOL), members), main.dev, main.ref, N_MAIN)


@pytest.mark.parametrize("c", [I32, I64])
def test_unsigned_order(decoder, main, c):
    u, s = F.col(c, unsigned=True), F.col(c)
    for lit in (5, -5, 0, -1):
        for mk in (F.lt, F.lt_eq, F.gt, F.gt_eq, F.eq, F.not_eq):
            check(decoder, mk(u, lit), main.dev, main.ref, N_MAIN)
    n_u = check(decoder, F.gt(u, 5), main.dev, main.ref, N_MAIN)
    n_s = check(decoder, F.gt(s, 5), main.dev, main.ref, N_MAIN)
    assert n_u > n_s  # the negative values are above 5 in unsigned order
    check(decoder, F.and_(F.gt(u, 5), F.lt(s, 5)), main.dev, main.ref, N_MAIN)  # one column, both orders


def test_byte_array_edges(decoder):
    """Empty strings, equal prefixes, bytes >= 0x80, values longer than the literal and the reverse."""
    base = [b"", b"a", b"ab", b"abc", b"abcd", b"abcde", b"ab\x80", b"ab\x7f", b"\x80", b"\xff" * 9, b"abcdefgh",
            b"abcdefghi", b"abcdefgh\x00", b"b", b"\x00", b"\x00\x00"]
    n = T + 100
    rng = np.random.default_rng(9)
    vals = [base[int(x)] for x in rng.integers(0, len(base), size=n)]
    data = Data(decoder, [(abi.BYTE_ARRAY, 0, None, vals)], n)
    c = F.col(0)
    for lit in base:
        for mk in (F.eq, F.lt, F.lt_eq, F.gt, F.gt_eq, F.not_eq):
            check(decoder, mk(c, lit), data.dev, data.ref, n)
    check(decoder, F.in_(c, base[:9]), data.dev, data.ref, n)
    check(decoder, F.not_in(c, base[3:]), data.dev, data.ref, n)


# ---- trees -------------------------------------------------------------------------------------------------

def test_rewriter_complex_case(decoder, main):
    complex_, collapsed = rewriter_complex()  # over intColumn = column 0, doubleColumn = column 1 (nullable here)
    a = check(decoder, complex_, main.dev, main.ref, N_MAIN)
    b = check(decoder, collapsed, main.dev, main.ref, N_MAIN)
    assert a == b


def test_random_trees(decoder, main):
    pick = [I32, F64, I64, BIN]
    dev, ref = [main.dev[i] for i in pick], [main.ref[i] for i in pick]
    types = [MAIN_TYPES[i] for i in pick]
    rng = np.random.default_rng(77)
    for _ in range(50):
        check(decoder, R.random_predicate(rng, types, 5), dev, ref, N_MAIN)


def test_one_column_under_several_leaves(decoder, main):
    c, d = F.col(I64), F.col(F64)
    pred = F.and_(F.or_(F.gt(c, 3), F.eq(c, None)), F.and_(F.not_eq(c, 7), F.or_(F.lt(d, 0.0), F.not_(F.lt_eq(c, -3)))))
    check(decoder, pred, main.dev, main.ref, N_MAIN)


# ---- capacity and errors ---------------------------------------------------------------------------------------

def test_capacity_below_the_count(decoder, main):
    pred = F.not_eq(F.col(I32), 0)
    full = check(decoder, pred, main.dev, main.ref, N_MAIN)
    for cap in (0, 1, 100, full - 1, full):
        assert check(decoder, pred, main.dev, main.ref, N_MAIN, capacity=cap) == full  # the count stays the full one


def test_without_row_ids(decoder, main):
    check(decoder, F.lt(F.col(F64), 0.5), main.dev, main.ref, N_MAIN, row_ids=False)
    dev, ref = main.prefix(0)
    check(decoder, F.lt(F.col(F64), 0.5), dev, ref, 0, row_ids=False)


@pytest.mark.parametrize("c", [F64, I64, BIN])
@pytest.mark.parametrize("delta", [-1, 1])
def test_wrong_n_values_is_an_error(decoder, main, c, delta):
    """n_values one too small / too large: the result names the column, and the run ends clean."""
    dev = list(main.dev)
    dev[c] = copy.copy(dev[c])
    dev[c].n_values += delta
    pred = F.or_(F.lt(F.col(I32), 0), F.and_(F.not_eq(F.col(c), None), F.not_eq(F.col(BOOL), True)))
    words, ids, sel = run(decoder, pred, dev, N_MAIN)
    with pytest.raises(native.PqgError) as e:
        sel.count
    assert e.value.code == abi.ERR_INVALID_ARG
    r = sel._result.cpu().numpy()
    assert r[8:16].view(np.int32).tolist() == [abi.ERR_INVALID_ARG, c]
    check(decoder, pred, main.dev, main.ref, N_MAIN)  # the context goes on working


def test_a_required_column_shorter_than_the_rows_is_refused(decoder, main):
    dev = list(main.dev)
    dev[I32] = copy.copy(dev[I32])
    dev[I32].n_values -= 1
    with pytest.raises(native.PqgError) as e:
        decoder.filter(F.lt(F.col(I32), 0), dev, N_MAIN)
    assert e.value.code == abi.ERR_INVALID_ARG


# ---- independence ----------------------------------------------------------------------------------------------

def test_same_filter_twice(decoder, main):
    pred = F.and_(F.lt_eq(F.col(I64), 5), F.not_eq(F.col(F64), 1.5))
    flt = F.Filter(pred, main.dev)
    outs = []
    for _ in range(2):
        words, ids, sel = run(decoder, flt, main.dev, N_MAIN)
        outs.append((sel.count, words.cpu().numpy(), ids.cpu().numpy()))
    other = run(decoder, F.gt(F.col(I32), 0), main.dev, N_MAIN)[2].count  # another program in between
    words, ids, sel = run(decoder, flt, main.dev, N_MAIN)
    outs.append((sel.count, words.cpu().numpy(), ids.cpu().numpy()))
    for o in outs[1:]:
        assert o[0] == outs[0][0] and np.array_equal(o[1], outs[0][1]) and np.array_equal(o[2], outs[0][2])
    assert outs[0][0] == int(R.evaluate(pred, main.ref, N_MAIN).sum()) and other >= 0
    flt.close()


def test_after_a_decode_on_the_same_stream(decoder):
    """Plan launch then filter, no synchronisation between: stream order alone."""
    n = T + 33
    rng = np.random.default_rng(12)
    dl = random_levels(rng, n, 1)
    vals = rng.integers(-50, 50, size=int((dl == 1).sum())).astype(np.int64)
    chunk = writer.write_column_chunk(abi.INT64, vals, abi.PLAIN, def_levels=dl, max_def=1, page_rows=1000)
    plan = decoder.plan(decoder.upload(writer.build_batch([chunk])))
    for col in plan.columns:
        col.values.fill_(POISON)
    torch.cuda.synchronize()
    pred = F.lt_eq(F.col(0), 0)
    plan.launch()
    words, ids, sel = run(decoder, pred, plan.columns, n)
    want = R.evaluate(pred, [R.RefColumn(abi.INT64, vals, dl, 1)], n)
    assert sel.count == int(want.sum())
    assert np.array_equal(words.cpu().numpy()[:(n + 63) // 64].view(np.uint64), R.bitmap_words(want))
    assert np.array_equal(sel.row_ids.cpu().numpy(), np.flatnonzero(want))
    rc, st = plan.sync()
    assert rc == abi.OK
    plan.close()
