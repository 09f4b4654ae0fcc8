"""tests/filter_ref.py pinned to parquet-mr's own known answers: the rewrite to
TestLogicalInverseRewriter (testBaseCases, testComplex :65-97) and TestLogicalInverter, the leaves to
the null table of the generated ValueInspectors, compare() to the PrimitiveComparator edge cases, and
the array evaluation to the row-by-row one. No device, no native code.

The reference's complex predicates contain a user-defined predicate, which is out of scope here: an
in() leaf stands in its place (its inverse, notIn, plays LogicalNotUserDefined's part)."""
import numpy as np
import pytest

import filter_ref as R
from pqgpu import abi
from pqgpu import filter as F

INT, DBL = F.col(0), F.col(1)  # intColumn("a.b.c"), doubleColumn("a.b.c")
UD = F.in_(INT, [1, 2])
NOT_UD = F.not_in(INT, [1, 2])


def test_rewriter_base_cases():
    for p in (F.eq(INT, 17), F.not_eq(INT, 17), F.lt(INT, 17), F.lt_eq(INT, 17), F.gt(INT, 17), F.gt_eq(INT, 17),
              F.and_(F.eq(INT, 17), F.eq(DBL, 12.0)), F.or_(F.eq(INT, 17), F.eq(DBL, 12.0)), UD):
        assert R.same(R.rewrite(p), p)  # assertNoOp
    assert R.same(R.rewrite(F.not_(F.eq(INT, 17))), F.not_eq(INT, 17))
    assert R.same(R.rewrite(F.not_(F.not_eq(INT, 17))), F.eq(INT, 17))
    assert R.same(R.rewrite(F.not_(F.lt(INT, 17))), F.gt_eq(INT, 17))
    assert R.same(R.rewrite(F.not_(F.lt_eq(INT, 17))), F.gt(INT, 17))
    assert R.same(R.rewrite(F.not_(F.gt(INT, 17))), F.lt_eq(INT, 17))
    assert R.same(R.rewrite(F.not_(F.gt_eq(INT, 17))), F.lt(INT, 17))
    assert R.same(R.rewrite(F.not_(UD)), NOT_UD)
    assert R.same(R.rewrite(F.not_(F.and_(F.eq(INT, 17), F.eq(DBL, 12.0)))),
                  F.or_(F.not_eq(INT, 17), F.not_eq(DBL, 12.0)))
    assert R.same(R.rewrite(F.and_(F.not_(F.gt_eq(INT, 17)), F.lt(INT, 7))), F.and_(F.lt(INT, 17), F.lt(INT, 7)))


def rewriter_complex():
    """TestLogicalInverseRewriter.complex and complexCollapsed."""
    complex_ = F.and_(
        F.not_(F.or_(F.lt_eq(DBL, 12.0), F.and_(F.not_(F.or_(F.eq(INT, 7), F.not_eq(INT, 17))), UD))),
        F.or_(F.gt(DBL, 100.0), F.not_(F.gt_eq(INT, 77))))
    collapsed = F.and_(
        F.and_(F.gt(DBL, 12.0), F.or_(F.or_(F.eq(INT, 7), F.not_eq(INT, 17)), NOT_UD)),
        F.or_(F.gt(DBL, 100.0), F.lt(INT, 77)))
    return complex_, collapsed


def test_rewriter_complex():
    complex_, collapsed = rewriter_complex()
    assert R.same(R.rewrite(complex_), collapsed)
    assert not R.same(R.rewrite(complex_), complex_)


def test_inverter():
    assert R.same(R.invert(F.eq(INT, 17)), F.not_eq(INT, 17))
    assert R.same(R.invert(F.not_eq(INT, 17)), F.eq(INT, 17))
    assert R.same(R.invert(F.lt(INT, 17)), F.gt_eq(INT, 17))
    assert R.same(R.invert(F.lt_eq(INT, 17)), F.gt(INT, 17))
    assert R.same(R.invert(F.gt(INT, 17)), F.lt_eq(INT, 17))
    assert R.same(R.invert(F.gt_eq(INT, 17)), F.lt(INT, 17))
    and_pos = F.and_(F.eq(INT, 17), F.eq(DBL, 12.0))
    and_inv = F.or_(F.not_eq(INT, 17), F.not_eq(DBL, 12.0))
    assert R.same(R.invert(and_pos), and_inv)
    or_pos = F.or_(F.eq(INT, 17), F.eq(DBL, 12.0))
    or_inv = F.and_(F.not_eq(INT, 17), F.not_eq(DBL, 12.0))
    assert R.same(R.invert(or_inv), or_pos)
    assert R.same(R.invert(F.not_(F.eq(INT, 17))), F.eq(INT, 17))
    assert R.same(R.invert(UD), NOT_UD) and R.same(R.invert(F.not_(UD)), UD) and R.same(R.invert(NOT_UD), UD)
    # TestLogicalInverter.complex / complexInverse
    complex_ = F.and_(
        F.or_(F.lt_eq(DBL, 12.0), F.and_(F.not_(F.or_(F.eq(INT, 7), F.not_eq(INT, 17))), UD)),
        F.or_(F.gt(DBL, 100.0), F.not_eq(INT, 77)))
    inverse = F.or_(
        F.and_(F.gt(DBL, 12.0), F.or_(F.or_(F.eq(INT, 7), F.not_eq(INT, 17)), NOT_UD)),
        F.and_(F.lt_eq(DBL, 100.0), F.eq(INT, 77)))
    assert R.same(R.invert(complex_), inverse)


C = F.col(0)
NULL_TABLE = [  # (leaf, on a null row, on a row holding 5, on a row holding 9)
    (F.eq(C, 5), False, True, False),
    (F.not_eq(C, 5), True, False, True),
    (F.eq(C, None), True, False, False),
    (F.not_eq(C, None), False, True, True),
    (F.lt(C, 6), False, True, False),
    (F.lt_eq(C, 5), False, True, False),
    (F.gt(C, 5), False, False, True),
    (F.gt_eq(C, 9), False, False, True),
    (F.in_(C, [5, 6]), False, True, False),
    (F.not_in(C, [5, 6]), True, False, True),
    (F.in_(C, [5, None]), True, False, False),      # the set contains null: its other members are ignored
    (F.not_in(C, [5, None]), False, True, True),
]


@pytest.mark.parametrize("leaf,on_null,on_5,on_9", NULL_TABLE, ids=[repr(t[0]) for t in NULL_TABLE])
def test_null_table(leaf, on_null, on_5, on_9):
    assert R.leaf_row(leaf, abi.INT32, None) is on_null
    assert R.leaf_row(leaf, abi.INT32, 5) is on_5
    assert R.leaf_row(leaf, abi.INT32, 9) is on_9
    col = R.RefColumn(abi.INT32, np.array([5, 9], dtype=np.int32), def_levels=[0, 1, 1], max_def=1)
    want = [on_null, on_5, on_9]
    assert R.evaluate_rows(leaf, [col], 3).tolist() == want
    assert R.evaluate(leaf, [col], 3).tolist() == want
    missing = R.RefColumn(abi.INT32, max_def=1, missing=True)  # no value reaches it: null in every row
    assert R.evaluate_rows(leaf, [missing], 2).tolist() == [on_null] * 2
    assert R.evaluate(leaf, [missing], 2).tolist() == [on_null] * 2


def test_not_is_rewritten_not_complemented():
    col = R.RefColumn(abi.INT32, np.array([3, 7], dtype=np.int32), def_levels=[1, 0, 1], max_def=1)
    p = F.not_(F.lt(C, 5))  # gtEq(x, 5): false on the null row, where the complement of lt would be true
    assert R.evaluate_rows(p, [col], 3).tolist() == [False, False, True]
    assert R.evaluate(p, [col], 3).tolist() == [False, False, True]


def test_boolean_inequality_throws():
    with pytest.raises(ValueError):
        R.leaf_row(F.lt(C, True), abi.BOOLEAN, True)


def f32(bits):
    return np.array([bits], dtype=np.uint32).view(np.float32)[0]


def f64(bits):
    return np.array([bits], dtype=np.uint64).view(np.float64)[0]


def test_comparator_edges():
    cmp = R.compare
    assert cmp(abi.BOOLEAN, False, False, True) < 0 and cmp(abi.BOOLEAN, False, True, True) == 0
    # Float.compare / Double.compare: a total order
    for t, mk, qnan, nnan, pnan in ((abi.FLOAT, np.float32, f32(0x7FC00000), f32(0xFFC00001), f32(0x7F800001)),
                                     (abi.DOUBLE, np.float64, f64(0x7FF8000000000000), f64(0xFFF8000000000123),
                                      f64(0x7FF0000000000001))):
        assert cmp(t, False, mk(-0.0), mk(0.0)) < 0 and cmp(t, False, mk(0.0), mk(-0.0)) > 0
        assert cmp(t, False, mk(0.0), mk(0.0)) == 0 and cmp(t, False, mk(-0.0), mk(-0.0)) == 0
        for a in (qnan, nnan, pnan):  # every NaN equals every other NaN, whatever its sign and payload
            for b in (qnan, nnan, pnan):
                assert cmp(t, False, a, b) == 0
            assert cmp(t, False, a, mk(np.inf)) > 0 and cmp(t, False, mk(np.inf), a) < 0  # NaN above +Infinity
            assert cmp(t, False, a, mk(-np.inf)) > 0
        assert cmp(t, False, mk(-np.inf), mk(-1e30)) < 0 and cmp(t, False, mk(np.inf), mk(1e30)) > 0
    # signed and unsigned ints (UINT_32 / UINT_64: x ^ MIN_VALUE)
    assert cmp(abi.INT32, False, -1, 1) < 0 and cmp(abi.INT32, True, -1, 1) > 0
    assert cmp(abi.INT32, True, -2**31, 2**31 - 1) > 0 and cmp(abi.INT32, False, -2**31, 2**31 - 1) < 0
    assert cmp(abi.INT64, False, -1, 1) < 0 and cmp(abi.INT64, True, -1, 1) > 0
    assert cmp(abi.INT64, True, -2**63, 2**63 - 1) > 0 and cmp(abi.INT64, True, 5, 5) == 0
    # Binary.lexicographicCompare: unsigned bytes, then length
    assert cmp(abi.BYTE_ARRAY, False, b"ab", b"abc") < 0 and cmp(abi.BYTE_ARRAY, False, b"abc", b"ab") > 0
    assert cmp(abi.BYTE_ARRAY, False, b"", b"a") < 0 and cmp(abi.BYTE_ARRAY, False, b"", b"") == 0
    assert cmp(abi.BYTE_ARRAY, False, b"a\x80", b"a\x7f") > 0  # 0x80 is 128, not -128
    assert cmp(abi.BYTE_ARRAY, False, b"\xff", b"\x01\x02") > 0 and cmp(abi.BYTE_ARRAY, False, b"ab\x80", b"ab") > 0
    assert cmp(abi.BYTE_ARRAY, False, b"ab\x80", b"ab\x80") == 0


@pytest.mark.parametrize("t,unsigned", [(abi.BOOLEAN, False), (abi.INT32, False), (abi.INT32, True), (abi.INT64, False),
                                        (abi.INT64, True), (abi.FLOAT, False), (abi.DOUBLE, False)])
def test_keys_order_as_compare(t, unsigned):
    """The integer comparator keys (what the device compares) order every pair as compare() does."""
    vals = R.EDGE[t]
    keys = R.key_array(t, unsigned, np.array(vals, dtype=abi.numpy_dtype(t) if t != abi.BOOLEAN else np.uint8))
    for i, a in enumerate(vals):
        for j, b in enumerate(vals):
            c = R.compare(t, unsigned, a, b)
            k = int(keys[i] > keys[j]) - int(keys[i] < keys[j])
            assert int(np.sign(c)) == k, (a, b)


def test_float_equality_edges():
    col = R.RefColumn(abi.DOUBLE, np.array([0.0, -0.0, np.nan, 1e308, np.inf, -np.inf], dtype=np.float64))
    for ev in (R.evaluate_rows, R.evaluate):
        assert ev(F.eq(C, 0.0), [col], 6).tolist() == [True, False, False, False, False, False]
        assert ev(F.eq(C, -0.0), [col], 6).tolist() == [False, True, False, False, False, False]
        assert ev(F.gt(C, 1e308), [col], 6).tolist() == [False, False, True, False, True, False]  # NaN matches
        assert ev(F.eq(C, f64(0xFFF8000000000123)), [col], 6).tolist() == [False, False, True, False, False, False]


def ref_columns(rng, types, n_rows):
    cols = []
    for i, t in enumerate(types):
        max_def = [0, 1, 3][i % 3]
        dl = None
        if max_def:
            dl = rng.integers(0, max_def + 1, size=n_rows).astype(np.uint8)
        k = n_rows if dl is None else int((dl == max_def).sum())
        pool = R.EDGE[t]
        picks = [pool[int(x)] for x in rng.integers(0, len(pool), size=k)]
        vals = picks if t == abi.BYTE_ARRAY else np.array(picks, dtype=abi.numpy_dtype(t) if t != abi.BOOLEAN else np.uint8)
        cols.append(R.RefColumn(t, vals, dl, max_def))
    return cols


def test_array_evaluation_equals_row_by_row():
    rng = np.random.default_rng(5)
    types = [abi.BOOLEAN, abi.INT32, abi.INT64, abi.FLOAT, abi.DOUBLE, abi.BYTE_ARRAY]
    cols = ref_columns(rng, types, 257)
    for _ in range(150):
        p = R.random_predicate(rng, types, 5)
        assert np.array_equal(R.evaluate(p, cols, 257), R.evaluate_rows(p, cols, 257)), repr(p)


def test_bitmap_words():
    bits = np.zeros(130, dtype=bool)
    bits[[0, 63, 64, 129]] = True
    w = R.bitmap_words(bits)
    assert w.tolist() == [1 | 1 << 63, 1, 2]
    assert R.bitmap_words(np.zeros(0, dtype=bool)).size == 0
