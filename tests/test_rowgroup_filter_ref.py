"""tests/rowgroup_filter_ref.py against known answers taken by hand from parquet-mr's DictionaryFilterTest
(parquet-hadoop/src/test/java/org/apache/parquet/filter2/dictionarylevel/DictionaryFilterTest.java): the
dictionaries are rebuilt from the value lists of that file (:120-155: the alphabet, "sharp", intValues,
DECIMAL_VALUES, INT96_VALUES; doubles are the ints, floats twice the ints) and every assertion of the named
tests is restated with its expected outcome. The V2 file's outcomes are used where the test distinguishes (a
FIXED_LEN_BYTE_ARRAY dictionary exists only there). No GPU."""
import numpy as np

import rowgroup_filter_ref as G
from pqgpu import abi
from pqgpu import filter as F

INT_VALUES = [-100, 302, 3333333, 7654321, 1234567, -2000, -77775, 0, 75, 22223, 77, 22221, -444443, 205, 12, 44444,
              889, 66665, -777889, -7, 52, 33, -257, 1111, 775, 26]
I64_MIN, I64_MAX = -2**63, 2**63 - 1
DECIMALS = [-9999999999999999999999999999999999999999, -9999999999999999999999999999999999999998, I64_MIN - 1, I64_MIN,
            I64_MIN + 1, -1, 0, I64_MAX - 1, I64_MAX, I64_MAX + 1, 999999999999999999999999999999999999999,
            9999999999999999999999999999999999999998, 9999999999999999999999999999999999999999]
INT96S = [-9999999999999999999999999999, -9999999999999999999999999998, -1234567890, -1, 0, 1, 1234567890,
          -9999999999999999999999999998, 9999999999999999999999999999]


def fixed(v, n):
    return F.decimal_bytes(v, n)


# column index -> chunk, in the schema's order (:107-119); 12 is "missing_column"
(BINARY, SINGLE, OPT_SINGLE, FIXED, INT32, INT64, DOUBLE, FLOAT, PLAIN_INT32, FALLBACK, INT96, REPEATED, MISSING) = range(13)
CHUNKS = [
    G.RefChunk(abi.BYTE_ARRAY, [bytes([c]) for c in b"abcdefghijklmnopqrstuvwxyz"], may_contain_null=False),
    G.RefChunk(abi.BYTE_ARRAY, [b"sharp"], may_contain_null=False),
    G.RefChunk(abi.BYTE_ARRAY, [b"sharp"], may_contain_null=True),
    G.RefChunk(abi.FIXED_LEN_BYTE_ARRAY, [fixed(v, 17) for v in DECIMALS], may_contain_null=False),
    G.RefChunk(abi.INT32, list(INT_VALUES), may_contain_null=False),
    G.RefChunk(abi.INT64, list(INT_VALUES), may_contain_null=False),
    G.RefChunk(abi.DOUBLE, [v * 1.0 for v in INT_VALUES], may_contain_null=False),
    G.RefChunk(abi.FLOAT, [np.float32(v * 2.0) for v in INT_VALUES], may_contain_null=False),
    G.RefChunk(abi.INT32, None, non_dictionary_pages=True, may_contain_null=False),
    G.RefChunk(abi.BYTE_ARRAY, [bytes([c]) for c in b"abcdefghijklmnopqrstuvwxyz"], non_dictionary_pages=True,
               may_contain_null=False),
    G.RefChunk(abi.INT96, [fixed(v, 12) for v in INT96S], may_contain_null=False),
    G.RefChunk(abi.BYTE_ARRAY, [bytes([c]) for c in b"abcdefghijklmnopqrstuvwxyz"], may_contain_null=False),
    G.RefChunk(abi.BYTE_ARRAY, None, missing=True),
]


def drop(pred):
    return G.can_drop(pred, CHUNKS)


def test_eq_binary():
    b = F.col(BINARY)
    assert not drop(F.eq(b, b"c"))
    assert drop(F.eq(b, b"A"))
    assert not drop(F.eq(b, None))


def test_eq_fixed():
    b = F.col(FIXED, order="signed_integer")
    assert drop(F.eq(b, fixed(-2, 17)))
    assert not drop(F.eq(b, fixed(-1, 17)))
    assert not drop(F.eq(b, None))
    # equals(), not the comparator: the same number in 16 bytes is another Binary
    assert drop(F.eq(b, fixed(-1, 16)))
    assert not drop(F.and_(F.gt_eq(b, fixed(-1, 16)), F.lt_eq(b, fixed(-1, 16))))


def test_eq_int96():
    b = F.col(INT96, order="signed_integer")
    assert not drop(F.eq(b, fixed(-2, 12)))
    assert not drop(F.eq(b, fixed(-1, 12)))
    assert not drop(F.eq(b, None))


def test_not_eq_binary():
    sharp, sharp_null, b = F.col(SINGLE), F.col(OPT_SINGLE), F.col(BINARY)
    assert drop(F.not_eq(sharp, b"sharp"))
    assert not drop(F.not_eq(sharp, b"applause"))
    assert not drop(F.not_eq(sharp_null, b"sharp"))
    assert not drop(F.not_eq(sharp_null, b"applause"))
    assert not drop(F.not_eq(b, b"x"))
    assert not drop(F.not_eq(b, b"B"))
    assert not drop(F.not_eq(b, None))


def test_lt_int():
    i32, lowest = F.col(INT32), min(INT_VALUES)
    assert drop(F.lt(i32, lowest))
    assert not drop(F.lt(i32, lowest + 1))
    assert not drop(F.lt(i32, 2**31 - 1))


def test_lt_fixed():
    f = F.col(FIXED, order="signed_integer")
    assert drop(F.lt(f, fixed(DECIMALS[0], 17)))
    assert not drop(F.lt(f, fixed(DECIMALS[1], 17)))


def test_lt_eq_long():
    i64, lowest = F.col(INT64), min(INT_VALUES)
    assert drop(F.lt_eq(i64, lowest - 1))
    assert not drop(F.lt_eq(i64, lowest))
    assert not drop(F.lt_eq(i64, I64_MAX))


def test_gt_float():
    f, highest = F.col(FLOAT), np.float32(max(INT_VALUES) * 2.0)
    assert drop(F.gt(f, highest))
    assert not drop(F.gt(f, np.float32(highest - np.float32(1.0))))
    assert not drop(F.gt(f, np.float32(1.4e-45)))  # Float.MIN_VALUE


def test_gt_eq_double():
    d, highest = F.col(DOUBLE), max(INT_VALUES) * 1.0
    assert drop(F.gt_eq(d, highest + 0.00000001))
    assert not drop(F.gt_eq(d, highest))
    assert not drop(F.gt_eq(d, 4.9e-324))  # Double.MIN_VALUE


def test_in_binary():
    b = F.col(BINARY)
    set1 = [b"F", b"C", b"h", b"E"]
    assert not drop(F.in_(b, set1)) and not drop(F.not_in(b, set1))
    set2 = [bytes([97 + i]) for i in range(26)] + [b"A"]
    assert not drop(F.in_(b, set2))
    assert drop(F.not_in(b, set2))
    set3 = [b"F", b"C", b"A", b"E"]
    assert drop(F.in_(b, set3)) and not drop(F.not_in(b, set3))
    assert not drop(F.in_(b, [None])) and not drop(F.not_in(b, [None]))
    sharp_null = F.col(OPT_SINGLE)
    assert not drop(F.not_in(sharp_null, [b"sharp"])) and not drop(F.in_(sharp_null, [b"sharp"]))


def test_in_fixed_and_int96():
    b = F.col(FIXED, order="signed_integer")
    set1 = [fixed(v, 17) for v in (-2, -22, 12345)]
    assert drop(F.in_(b, set1)) and not drop(F.not_in(b, set1))
    set2 = [fixed(v, 17) for v in (-1, 0, 12345)]
    assert not drop(F.in_(b, set2)) and not drop(F.not_in(b, set2))
    assert not drop(F.in_(b, [None])) and not drop(F.not_in(b, [None]))
    i96 = F.col(INT96, order="signed_integer")
    for s in ([fixed(v, 12) for v in (-2, 0, 12345)], [fixed(v, 17) for v in (-2, 12345, -789)], [None]):
        assert not drop(F.in_(i96, s)) and not drop(F.not_in(i96, s))


def _letters(wrap=lambda p: p):
    col = F.col(BINARY)
    return [wrap(F.eq(col, v)) for v in (b"B", b"C", b"x", b"y")]


def test_and():
    B, C, x, y = _letters()
    assert drop(F.and_(B, y)) and drop(F.and_(x, C)) and drop(F.and_(B, C))
    assert not drop(F.and_(x, y))


def test_or():
    B, C, x, y = _letters()
    assert not drop(F.or_(B, y)) and not drop(F.or_(x, C)) and not drop(F.or_(x, y))
    assert drop(F.or_(B, C))


def test_contains_and():
    col = F.col(REPEATED)
    B, C, x, y = [F.contains(F.eq(col, v)) for v in (b"B", b"C", b"x", b"y")]
    assert drop(F.and_(B, y)) and drop(F.and_(x, C)) and drop(F.and_(B, C))
    assert not drop(F.and_(x, y))


def test_contains_or():
    col = F.col(REPEATED)
    B, C, x, y = [F.contains(F.eq(col, v)) for v in (b"B", b"C", b"x", b"y")]
    assert not drop(F.or_(B, y)) and not drop(F.or_(x, C)) and not drop(F.or_(x, y))
    assert drop(F.or_(B, C))


def _never_drops(c):
    n = 1000
    for pred in (F.eq(c, -10), F.lt(c, -10), F.lt_eq(c, -10), F.gt(c, n + 10), F.gt_eq(c, n + 10), F.not_eq(c, n + 10)):
        assert not drop(pred)


def test_column_without_dictionary():
    _never_drops(F.col(PLAIN_INT32))


def test_column_with_dictionary_and_plain_encodings():
    c = F.col(FALLBACK)
    for pred in (F.eq(c, b"A"), F.lt(c, b"A"), F.lt_eq(c, b"A"), F.gt(c, b"zz"), F.gt_eq(c, b"zz"), F.not_eq(c, b"zz")):
        assert not drop(pred)


def test_missing_column():
    b = F.col(MISSING)
    assert drop(F.eq(b, b"any")) and not drop(F.eq(b, None))                 # testEqMissingColumn
    assert not drop(F.not_eq(b, b"any")) and drop(F.not_eq(b, None))         # testNotEqMissingColumn
    for op in (F.lt, F.lt_eq, F.gt, F.gt_eq):                                # testLt .. testGtEqMissingColumn
        assert drop(op(b, b"any"))
    # visit(In) / visit(NotIn) on meta == null (:392-395, :446-462)
    assert drop(F.in_(b, [b"any"])) and not drop(F.in_(b, [None, b"any"]))
    assert drop(F.not_in(b, [None])) and not drop(F.not_in(b, [None, b"any"])) and not drop(F.not_in(b, [b"any"]))


def test_rewrite_comes_first():
    b = F.col(SINGLE)
    # not(eq) is notEq after LogicalInverseRewriter: droppable on the single-value column without nulls
    assert drop(F.not_(F.eq(b, b"sharp")))
    assert not drop(F.not_(F.eq(F.col(OPT_SINGLE), b"sharp")))
    # not(or(B, x)) = and(notEq B, notEq x)
    assert drop(F.not_(F.or_(F.eq(b, b"other"), F.eq(b, b"sharp"))))


def test_empty_dictionary_and_duplicates():
    empty = [G.RefChunk(abi.INT64, [], may_contain_null=False)]
    c = F.col(0)
    assert G.can_drop(F.eq(c, 1), empty) and G.can_drop(F.in_(c, [1, 2]), empty) and G.can_drop(F.lt(c, 1), empty)
    assert G.can_drop(F.not_in(c, [1]), empty)
    assert not G.can_drop(F.not_eq(c, 1), empty)  # dictSet.size() == 1 fails
    dup = [G.RefChunk(abi.INT64, [7, 7, 7], may_contain_null=False)]
    assert G.can_drop(F.not_eq(c, 7), dup) and not G.can_drop(F.not_eq(c, 8), dup)
    zeros = [G.RefChunk(abi.DOUBLE, [0.0, float("nan")], may_contain_null=False)]
    assert G.can_drop(F.eq(c, -0.0), zeros) and not G.can_drop(F.eq(c, np.float64("nan")), zeros)


def test_has_non_dictionary_pages():
    D, V2, DICT = abi.DATA_PAGE, abi.DATA_PAGE_V2, abi.DICTIONARY_PAGE
    assert not G.has_non_dictionary_pages([(DICT, abi.PLAIN, 1), (D, abi.RLE_DICTIONARY, 3)], [])
    assert G.has_non_dictionary_pages([(D, abi.RLE_DICTIONARY, 3), (V2, abi.PLAIN, 0)], [])
    assert G.has_non_dictionary_pages([(D, abi.RLE_DICTIONARY, 1), (D, abi.PLAIN_DICTIONARY, 1)], [])
    assert not G.has_non_dictionary_pages([(DICT, abi.PLAIN, 1)], [abi.PLAIN])
    assert not G.has_non_dictionary_pages(None, [abi.PLAIN_DICTIONARY, abi.RLE, abi.BIT_PACKED])
    assert G.has_non_dictionary_pages(None, [abi.RLE_DICTIONARY, abi.RLE])
