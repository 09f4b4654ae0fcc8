"""pqg_filter_create_typed (host only, no device): what it accepts and refuses, that pqg_filter_create is the
same function with zero widths and orders, the routing of F.col(order=...) and F.decimal_bytes; and
tests/filter_binary_ref.py's comparators against the ordered lists of parquet-mr's TestPrimitiveComparator
(tests/golden/filter/binary_orders.txt)."""
import os

import numpy as np
import pytest

import filter_binary_ref as B
import filter_ref as R
from pqgpu import abi, native
from pqgpu import filter as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "filter", "binary_orders.txt")
UB, SI, F16 = abi.FILTER_ORDER_UNSIGNED_BYTES, abi.FILTER_ORDER_SIGNED_INTEGER, abi.FILTER_ORDER_FLOAT16
FLBA, I96, BA = abi.FIXED_LEN_BYTE_ARRAY, abi.INT96, abi.BYTE_ARRAY


def leaf(op, column, begin=0, n=1, flags=0):
    return (op, column, -1, -1, flags, begin, n)


def typed_rc(columns, nodes=None, literals=(2 << 32,), blob=b"\x00\x01\x02\x03", **kw):
    nodes = [leaf(abi.FILTER_EQ, 0)] if nodes is None else nodes
    rc, h, st = F.create_typed(list(nodes), list(literals), blob, list(columns), **kw)
    if rc == abi.OK:
        native.lib().pqg_filter_destroy(h)
    return rc, st.value_index


def test_golden_lists_order_every_pair():
    blocks = B.read_orders(GOLDEN)
    assert [b[0] for b in blocks] == ["testLexicographicalBinaryComparator", "testBinaryAsSignedIntegerComparator",
                                      "testBinaryAsSignedIntegerComparatorWithEquals", "testFloat16Comparator"]
    assert [len(b[2]) for b in blocks] == [10, 16, 1, 8] and len(blocks[2][2][0]) == 5
    for name, order, groups in blocks:
        for i, gi in enumerate(groups):
            for j, gj in enumerate(groups):
                for a in gi:
                    for b in gj:
                        assert B.compare(order, a, b) == (i > j) - (i < j), (name, a.hex(), b.hex())


def test_consequences_the_issue_lists():
    c = B.compare_signed
    assert c(b"\x00\x94", b"\x00\x00\x00\x94") == 0 and c(b"\x00\x00\x00\x94", b"\x00\x00\x00\x00\x00\x94") == 0
    assert c(b"", b"\x00\x00\x00") == 0 and c(b"\x00", b"") == 0
    assert c(b"\xff", b"\x00") < 0
    assert c(b"\x80", b"\xff\x7f") > 0 and c(b"\xff\x7f", b"\x80") < 0  # -129 < -128
    f = B.compare_float16
    nan1, nan2, inf = b"\x01\x7e", b"\xff\xff", b"\x00\x7c"
    assert f(nan1, nan2) == 0 and f(nan1, inf) > 0 and f(inf, nan2) < 0
    assert f(b"\x00\x80", b"\x00\x00") < 0


@pytest.mark.parametrize("columns", [
    [(FLBA, 16, UB)], [(FLBA, 16, SI)], [(FLBA, 1, SI)], [(FLBA, 2, F16)], [(FLBA, 1000, UB)], [(I96, 0, SI)],
    [(I96, 12, SI)], [(BA, 0, UB)], [(BA, 0, SI)],
    [(FLBA, 5, SI), (FLBA, 0, F16)],  # column 1 is malformed, but the predicate does not name it
])
def test_accepts(columns):
    assert typed_rc(columns) == (abi.OK, -1)


def test_all_eight_ops_and_literal_lengths():
    blob = bytes(range(48))
    for op in (abi.FILTER_EQ, abi.FILTER_NOTEQ, abi.FILTER_LT, abi.FILTER_LTEQ, abi.FILTER_GT, abi.FILTER_GTEQ,
               abi.FILTER_IN, abi.FILTER_NOTIN):
        for columns in ([(FLBA, 5, SI)], [(I96, 0, SI)], [(FLBA, 5, UB)], [(BA, 0, SI)]):
            for n in (0, 4, 5, 6, 16, 17, 40):
                assert typed_rc(columns, [leaf(op, 0)], [n << 32], blob) == (abi.OK, -1)
    assert typed_rc([(FLBA, 5, SI)], [leaf(abi.FILTER_EQ, 0, 0, 0, abi.FILTER_NULL_LITERAL)], []) == (abi.OK, -1)


@pytest.mark.parametrize("columns,expect", [
    ([(FLBA, 16, UB, 1)], (abi.ERR_INVALID_ARG, 0)),                      # reserved (names the column)
    ([(abi.INT32, 0, 0), (FLBA, 4, UB, 7)], (abi.ERR_INVALID_ARG, 1)),    # ... on a column nobody names
    ([(abi.INT32, 4, 0)], (abi.ERR_INVALID_ARG, 0)),                      # type_length on a non-binary type
    ([(abi.DOUBLE, 0, SI)], (abi.ERR_INVALID_ARG, 0)),                    # an order on a non-binary type
    ([(BA, 3, UB)], (abi.ERR_INVALID_ARG, 0)),                            # BYTE_ARRAY has no type_length
    ([(FLBA, 0, UB)], (abi.ERR_INVALID_ARG, 0)),
    ([(FLBA, -1, SI)], (abi.ERR_INVALID_ARG, 0)),
    ([(I96, 8, SI)], (abi.ERR_INVALID_ARG, 0)),
    ([(I96, 0, UB)], (abi.ERR_INVALID_ARG, 0)),                           # INT96 compares signed only
    ([(I96, 12, F16)], (abi.ERR_INVALID_ARG, 0)),
    ([(FLBA, 3, F16)], (abi.ERR_INVALID_ARG, 0)),
    ([(BA, 0, F16)], (abi.ERR_INVALID_ARG, 0)),
    ([(FLBA, 4, 3)], (abi.ERR_INVALID_ARG, 0)),                           # no such order
    ([(9, 0, 0)], (abi.ERR_INVALID_ARG, 0)),                              # no such type
])
def test_refuses(columns, expect):
    lit = [0] if columns[0][0] not in (FLBA, I96, BA) else [2 << 32]
    assert typed_rc(columns, literals=lit) == expect


def test_refuses_literals_and_flags():
    f16 = [(FLBA, 2, F16)]
    assert typed_rc(f16, literals=[2 << 32]) == (abi.OK, -1)
    for n in (0, 1, 3):
        assert typed_rc(f16, literals=[n << 32]) == (abi.ERR_INVALID_ARG, 0)
    assert typed_rc(f16, [leaf(abi.FILTER_IN, 0, 0, 2)], [2 << 32, 1 << 32]) == (abi.ERR_INVALID_ARG, 0)
    for columns in ([(FLBA, 4, UB)], [(I96, 0, SI)], [(BA, 0, SI)]):
        assert typed_rc(columns, [leaf(abi.FILTER_EQ, 0, flags=abi.FILTER_UNSIGNED)]) == (abi.ERR_INVALID_ARG, 0)
        assert typed_rc(columns, literals=[(3 << 32) | 2]) == (abi.ERR_INVALID_ARG, 0)  # past the literal bytes
    # the node is named, not the column
    nodes = [leaf(abi.FILTER_EQ, 0), leaf(abi.FILTER_EQ, 1, 1), (abi.FILTER_AND, -1, 0, 1, 0, 0, 0)]
    assert typed_rc([(abi.INT32, 0, 0), (I96, 4, SI)], nodes, [5, 2 << 32]) == (abi.ERR_INVALID_ARG, 1)


def test_create_is_typed_with_zeros():
    types = [abi.INT32, abi.DOUBLE, abi.BOOLEAN, abi.INT64, abi.FLOAT, BA]
    rng = np.random.default_rng(5)
    for _ in range(60):
        c = F.compile(R.random_predicate(rng, types, 5), types)
        assert c.typed is None
        rc1, h1, st1 = F.create(c.nodes, c.literals, c.literal_bytes, c.column_types)
        rc2, h2, st2 = F.create_typed(c.nodes, c.literals, c.literal_bytes, [(t, 0, 0) for t in types])
        assert rc1 == rc2 == abi.OK
        assert F.program(h1) == F.program(h2)
        native.lib().pqg_filter_destroy(h1)
        native.lib().pqg_filter_destroy(h2)
    # the refusals of the bare form stay: typed-with-zeros differs from it on INT96 / FLBA only
    for t in (I96, FLBA):
        rc, h, st = F.create([leaf(abi.FILTER_EQ, 0)], [2 << 32], b"ab", [t])
        assert (rc, st.value_index) == (abi.ERR_UNSUPPORTED, 0)
    assert typed_rc([(I96, 0, 0)]) == (abi.ERR_INVALID_ARG, 0)
    assert typed_rc([(FLBA, 0, 0)]) == (abi.ERR_INVALID_ARG, 0)


class _Col:
    def __init__(self, physical_type, type_length=0, flags=0, dictionary=None):
        self.physical_type, self.type_length, self.flags, self.dictionary = physical_type, type_length, flags, dictionary


def test_col_order_routing():
    cols = [_Col(FLBA, 5), _Col(abi.INT64), _Col(I96), _Col(BA),
            _Col(abi.INT32, flags=abi.COLUMN_DICTIONARY_IDS, dictionary=_Col(FLBA, 16))]
    c = F.compile(F.lt(F.col(0, order="signed_integer"), F.decimal_bytes(-129)), cols)
    assert c.typed == [(FLBA, 5, SI), (abi.INT64, 0, 0), (I96, 0, 0), (BA, 0, 0), (FLBA, 16, 0)]
    assert c.literals == [2 << 32] and c.literal_bytes == b"\xff\x7f"
    c = F.compile(F.and_(F.eq(F.col(4, order="unsigned_bytes"), b"k" * 16), F.gt(F.col(2, order="signed_integer"), b"")), cols)
    assert c.typed[4] == (FLBA, 16, UB) and c.typed[2] == (I96, 0, SI)
    for pred in (F.lt(F.col(0, order="signed_integer"), b"\x01"), F.eq(F.col(2, order="signed_integer"), b"\x00" * 12),
                 F.in_(F.col(3, order="signed_integer"), [b"\x00\x01", b"\x01", None]),
                 F.eq(F.col(4, order="unsigned_bytes"), b"k" * 16)):
        flt = F.Filter(pred, cols)
        assert flt.compiled.typed is not None and flt.program()[0][1] == pred.column.index
        flt.close()
    # order=None: everything as before, refusals included
    assert F.compile(F.eq(F.col(3), b"x"), cols).typed is None
    F.Filter(F.eq(F.col(3), b"x"), cols).close()
    for i in (0, 2, 4):
        with pytest.raises(native.PqgError) as e:
            F.Filter(F.eq(F.col(i), b"x"), cols)
        assert e.value.code == abi.ERR_UNSUPPORTED
    with pytest.raises(native.PqgError) as e:  # the comparator the reference does not have
        F.Filter(F.eq(F.col(2, order="unsigned_bytes"), b"x"), cols)
    assert e.value.code == abi.ERR_INVALID_ARG
    with pytest.raises(ValueError):
        F.col(0, order="signed")
    with pytest.raises(ValueError):
        F.compile(F.and_(F.eq(F.col(3, order="signed_integer"), b"x"), F.eq(F.col(3, order="unsigned_bytes"), b"x")), cols)


def test_decimal_bytes():
    D = F.decimal_bytes
    assert D(0) == b"\x00" and D(1) == b"\x01" and D(-1) == b"\xff" and D(127) == b"\x7f" and D(128) == b"\x00\x80"
    assert D(-128) == b"\x80" and D(-129) == b"\xff\x7f" and D(148) == b"\x00\x94"
    assert D(148, 4) == b"\x00\x00\x00\x94" and D(-2, 3) == b"\xff\xff\xfe" and D(0, 16) == b"\x00" * 16
    assert D(10**38 - 1, 16)[0] == 0x4B and len(D(-10**38, 16)) == 16
    with pytest.raises(OverflowError):
        D(128, 1)
    rng = np.random.default_rng(3)
    for _ in range(300):
        v = int(rng.integers(-2**62, 2**62)) * int(rng.integers(1, 2**40)) >> int(rng.integers(0, 100))
        b = D(v)
        assert int.from_bytes(b, "big", signed=True) == v
        assert D(v, len(b)) == b
        assert B.compare_signed(b, D(v, len(b) + 3)) == 0
        w = int(rng.integers(-2**62, 2**62)) * int(rng.integers(1, 2**20))
        assert B.compare_signed(b, D(w)) == (v > w) - (v < w)


def test_large_signed_set_with_equal_members():
    members = [F.decimal_bytes(v) for v in (5, -7, 300, 2, -129, 10**20, 0, 77)] + [b"\x00\x05", b"\x00\x00\x00\x05", b"",
                                                                                  b"\xff\xff\xf9", b"\x00" * 30 + b"\x02"]
    cols = [_Col(BA), _Col(FLBA, 7), _Col(FLBA, 20)]
    for i in range(3):
        flt = F.Filter(F.in_(F.col(i, order="signed_integer"), members), cols)
        assert flt.program() == [(abi.FILTER_IN, i, -1, -1, 0, 0, len(members))]
        flt.close()
