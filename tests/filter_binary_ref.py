"""Reference semantics of parquet-mr's three binary comparators and of record filters that use them,
restated in Python. Test infrastructure only (the product is csrc/pqgpu_filter*.{cpp,hip}); the conventions
for null rows, null literals and sets are those of tests/filter_ref.py and tests/filter_records_ref.py.

What is restated (paths under parquet-column/src/main/java/org/apache/parquet/):
  compare_unsigned   io/api/Binary.java lexicographicCompare (UNSIGNED_LEXICOGRAPHICAL_BINARY_COMPARATOR,
                     schema/PrimitiveComparator.java:196-207): unsigned bytes over the common length, then the
                     lengths
  compare_signed     BINARY_AS_SIGNED_INTEGER_COMPARATOR (PrimitiveComparator.java:214-279), loop by loop:
                     the signs, compareWithPadding over the longer side's extra bytes, compare over the tail
  compare_float16    schema/Float16.java:108-134 on the two little-endian bytes (BINARY_AS_FLOAT16_COMPARATOR)
  leaf_row           the generated ValueInspectors with compareEquality = comparator.compare(...) == 0 for eq,
                     notEq, in and notIn
Everything here works on bytes, byte by byte: no integer or key form of a value is ever built, so that the
device's 128-bit and FLOAT16 keys are checked against something that shares nothing with them.

A column's comparator comes from the predicate's Column (`order`); None on a BYTE_ARRAY column is the unsigned
order, as pqg_filter_create has it. Values of BYTE_ARRAY, FIXED_LEN_BYTE_ARRAY and INT96 columns are `bytes`."""
import numpy as np

from pqgpu import abi

import filter_records_ref as RR
import filter_ref as R

BINARY_TYPES = (abi.BYTE_ARRAY, abi.INT96, abi.FIXED_LEN_BYTE_ARRAY)


def compare_unsigned(a, b):
    """Binary.lexicographicCompare."""
    n = min(len(a), len(b))
    for i in range(n):
        x, y = a[i] & 0xFF, b[i] & 0xFF
        if x != y:
            return -1 if x < y else 1
    return (len(a) > len(b)) - (len(a) < len(b))


def _to_signed_byte(x):
    return x - 256 if x >= 128 else x


def compare_signed(b1, b2):
    """BINARY_AS_SIGNED_INTEGER_COMPARATOR.compare(ByteBuffer, ByteBuffer)."""
    l1, l2 = len(b1), len(b2)
    p1 = p2 = 0
    neg1 = l1 > 0 and _to_signed_byte(b1[0]) < 0
    neg2 = l2 > 0 and _to_signed_byte(b2[0]) < 0
    if neg1 != neg2:
        return -1 if neg1 else 1
    result = 0

    def with_padding(length, b, p, padding):  # compareWithPadding
        for i in range(p, p + length):
            r = (b[i] & 0xFF) - padding
            if r != 0:
                return r
        return 0

    if l1 < l2:
        diff = l2 - l1
        result = -with_padding(diff, b2, p2, 0xFF if neg1 else 0)
        p2 += diff
    elif l1 > l2:
        diff = l1 - l2
        result = with_padding(diff, b1, p1, 0xFF if neg2 else 0)
        p1 += diff
    if result == 0:
        for i in range(min(l1, l2)):  # compare(length, b1, p1, b2, p2)
            r = (b1[p1 + i] & 0xFF) - (b2[p2 + i] & 0xFF)
            if r != 0:
                result = r
                break
    return (result > 0) - (result < 0)


def _short(x):
    x &= 0xFFFF
    return x - 0x10000 if x >= 0x8000 else x


def compare_float16(a, b):
    """Float16.compare(a.get2BytesLittleEndian(), b.get2BytesLittleEndian())."""
    assert len(a) == 2 and len(b) == 2
    x, y = _short(a[0] | (a[1] << 8)), _short(b[0] | (b[1] << 8))
    x_nan, y_nan = (x & 0x7FFF) > 0x7C00, (y & 0x7FFF) > 0x7C00
    if not x_nan and not y_nan:
        first = 0x8000 - (x & 0xFFFF) if (x & 0x8000) != 0 else x & 0xFFFF
        second = 0x8000 - (y & 0xFFFF) if (y & 0x8000) != 0 else y & 0xFFFF
        if first < second:
            return -1
        if first > second:
            return 1
    x_bits = 0x7E00 if x_nan else x
    y_bits = 0x7E00 if y_nan else y
    return 0 if x_bits == y_bits else (-1 if x_bits < y_bits else 1)


COMPARATORS = {None: compare_unsigned, "unsigned_bytes": compare_unsigned, "signed_integer": compare_signed,
               "float16": compare_float16}


def compare(order, a, b):
    return COMPARATORS[order](bytes(a), bytes(b))


# ---- leaves, rows, records ------------------------------------------------------------------------------

def leaf_row(p, physical_type, value):
    """One leaf on one row (`value` None: a null row). Binary columns compare with the Column's order; every
    other type is filter_ref.leaf_row."""
    if physical_type not in BINARY_TYPES:
        return R.leaf_row(p, physical_type, value)
    cmp = COMPARATORS[getattr(p.column, "order", None)]
    op, lits = p.op, p.values
    if op in (abi.FILTER_LT, abi.FILTER_LTEQ, abi.FILTER_GT, abi.FILTER_GTEQ):
        if value is None:
            return False
        c = cmp(bytes(value), bytes(lits[0]))
        return {abi.FILTER_LT: c < 0, abi.FILTER_LTEQ: c <= 0, abi.FILTER_GT: c > 0, abi.FILTER_GTEQ: c >= 0}[op]
    if op in (abi.FILTER_EQ, abi.FILTER_NOTEQ):
        if lits[0] is None:
            return (value is None) == (op == abi.FILTER_EQ)
        if value is None:
            return op == abi.FILTER_NOTEQ
        return (cmp(bytes(value), bytes(lits[0])) == 0) == (op == abi.FILTER_EQ)
    if any(v is None for v in lits):
        return (value is None) == (op == abi.FILTER_IN)
    if value is None:
        return op == abi.FILTER_NOTIN
    found = any(cmp(bytes(value), bytes(v)) == 0 for v in lits)  # compareEquality, not Set.contains
    return found == (op == abi.FILTER_IN)


class _Memo:
    """leaf_row per distinct value of a leaf (columns here draw from small pools of values)."""

    def __init__(self):
        self.seen = {}

    def __call__(self, p, physical_type, value):
        key = (id(p), None if value is None else bytes(value) if physical_type in BINARY_TYPES else value)
        try:
            return self.seen[key]
        except (KeyError, TypeError):
            pass
        r = leaf_row(p, physical_type, value)
        try:
            self.seen[key] = r
        except TypeError:
            pass
        return r


def evaluate_rows(pred, columns, n_rows):
    """filter_ref.evaluate_rows with the binary comparators: columns[c] is a filter_ref.RefColumn."""
    pred = R.rewrite(pred)
    rows, leaf = {}, _Memo()

    def ev(p, r):
        if p.op == abi.FILTER_AND:
            return ev(p.children[0], r) and ev(p.children[1], r)
        if p.op == abi.FILTER_OR:
            return ev(p.children[0], r) or ev(p.children[1], r)
        c = p.column.index
        if c not in rows:
            rows[c] = columns[c].row_values(n_rows)
        return leaf(p, columns[c].physical_type, rows[c][r])

    return np.array([ev(pred, r) for r in range(n_rows)], dtype=bool)


def evaluate_records(pred, columns, n_rows):
    """Records: contains(leaf) holds when some element of the record's list satisfies the leaf (the flat
    reading of notIn, as filter_records_ref has it); and / or stay as they are; flat leaves per row.
    columns[c]: filter_records_ref.RefListColumn or filter_ref.RefColumn."""
    pred = RR.li_rewrite(pred)
    lists, rows, leaf = {}, {}, _Memo()

    def ev(p, r):
        if p.op == abi.FILTER_AND:
            return ev(p.children[0], r) and ev(p.children[1], r)
        if p.op == abi.FILTER_OR:
            return ev(p.children[0], r) or ev(p.children[1], r)
        if p.op == abi.FILTER_CONTAINS:
            k = p.children[0]
            c = k.column.index
            if c not in lists:
                lists[c] = columns[c].record_values(n_rows)
            return any(leaf(k, columns[c].physical_type, v) for v in lists[c][r])
        c = p.column.index
        if c not in rows:
            rows[c] = columns[c].row_values(n_rows)
        return leaf(p, columns[c].physical_type, rows[c][r])

    return np.array([ev(pred, r) for r in range(n_rows)], dtype=bool)


# ---- golden ordered lists (tests/golden/filter/binary_orders.txt) ------------------------------------------

def read_orders(path):
    """-> list of (block name, order, [group, ...]): the groups ascend, a group's members compare equal.
    A block starts with `[name order]`; a line holds one group, its members separated by `=`; `-` is the empty
    value; `#` starts a comment."""
    blocks = []
    for line in open(path):
        line = line.split("#")[0].strip()
        if not line:
            continue
        if line.startswith("["):
            name, order = line.strip("[]").split()
            blocks.append((name, order, []))
            continue
        blocks[-1][2].append([b"" if m.strip() == "-" else bytes.fromhex(m.strip()) for m in line.split("=")])
    return blocks
