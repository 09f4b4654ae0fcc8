"""Reference semantics of parquet-mr's record-level filter2 evaluation, restated in Python / numpy.
Test infrastructure only (the product is csrc/pqgpu_filter*.{cpp,hip}).

What is restated (paths under parquet-column/src/main/java/org/apache/parquet/):
  rewrite / invert   filter2/predicate/LogicalInverseRewriter.java, LogicalInverter.java:56-114
  compare            schema/PrimitiveComparator.java:68-207 (Boolean.compare, signed / unsigned
                     int32 / int64, Float.compare / Double.compare, Binary.lexicographicCompare)
  leaf               the generated ValueInspectors (parquet-generator/.../
                     IncrementallyUpdatedFilterPredicateGenerator.java:198-327): update(value) for a
                     row with a value, updateNull() for a null row (and a column no value reached)
  evaluate_rows      filter2/recordlevel/IncrementallyUpdatedFilterPredicateEvaluator.java:45-61,
                     row by row
  evaluate           the same over numpy arrays (comparator keys), for large row counts; the CPU tests
                     hold it equal to evaluate_rows

Predicates are pqgpu.filter Predicate trees (plain data: op, column, values, children)."""
import struct

import numpy as np

from pqgpu import abi
from pqgpu import filter as F

INVERSE = {abi.FILTER_EQ: abi.FILTER_NOTEQ, abi.FILTER_NOTEQ: abi.FILTER_EQ, abi.FILTER_LT: abi.FILTER_GTEQ,
           abi.FILTER_GTEQ: abi.FILTER_LT, abi.FILTER_LTEQ: abi.FILTER_GT, abi.FILTER_GT: abi.FILTER_LTEQ,
           abi.FILTER_IN: abi.FILTER_NOTIN, abi.FILTER_NOTIN: abi.FILTER_IN}


# ---- LogicalInverter / LogicalInverseRewriter -----------------------------------------------------

def invert(p):
    """LogicalInverter.invert."""
    if p.op == abi.FILTER_AND:
        return F.or_(invert(p.children[0]), invert(p.children[1]))
    if p.op == abi.FILTER_OR:
        return F.and_(invert(p.children[0]), invert(p.children[1]))
    if p.op == abi.FILTER_NOT:
        return p.children[0]
    return F.Predicate(INVERSE[p.op], p.column, p.values)


def rewrite(p):
    """LogicalInverseRewriter.rewrite: the same predicate without not()."""
    if p.op == abi.FILTER_AND:
        return F.and_(rewrite(p.children[0]), rewrite(p.children[1]))
    if p.op == abi.FILTER_OR:
        return F.or_(rewrite(p.children[0]), rewrite(p.children[1]))
    if p.op == abi.FILTER_NOT:
        return invert(rewrite(p.children[0]))
    return p


def same(a, b):
    """Structural equality of two predicates (FilterPredicate.equals); sets compare as sets."""
    if a.op != b.op or len(a.children) != len(b.children):
        return False
    if a.children:
        return all(same(x, y) for x, y in zip(a.children, b.children))
    if a.column.index != b.column.index or a.column.unsigned != b.column.unsigned:
        return False
    ka = sorted(map(repr, a.values)) if a.op >= abi.FILTER_IN else list(map(repr, a.values))
    kb = sorted(map(repr, b.values)) if b.op >= abi.FILTER_IN else list(map(repr, b.values))
    return ka == kb


def flatten(p):
    """Post-order (left, right, node) list of (op, column, left, right, flags, n non-null literals):
    the shape pqg_filter_program reports."""
    out = []

    def walk(q):
        if q.children:
            kids = [walk(k) for k in q.children]
            out.append((q.op, -1, kids[0], kids[1] if len(kids) > 1 else -1, 0, 0))
        else:
            null = any(v is None for v in q.values)
            flags = (abi.FILTER_UNSIGNED if q.column.unsigned else 0) | (abi.FILTER_NULL_LITERAL if null else 0)
            # a set containing null: its other members are ignored (generator :282-293)
            n = 0 if null else len(q.values)
            out.append((q.op, q.column.index, -1, -1, flags, n))
        return len(out) - 1

    walk(p)
    return out


# ---- PrimitiveComparator ------------------------------------------------------------------------------

def _float_bits(x, double):
    """Float.floatToIntBits / Double.doubleToLongBits: the value's bits as a signed int, one NaN."""
    if double:
        b = struct.unpack("<q", struct.pack("<d", float(x)))[0] if not isinstance(x, np.floating) else int(
            np.asarray(x, dtype=np.float64).reshape(1).view(np.int64)[0])
        return 0x7FF8000000000000 if (b & 0x7FFFFFFFFFFFFFFF) > 0x7FF0000000000000 else b
    b = int(np.asarray(x, dtype=np.float32).reshape(1).view(np.int32)[0])
    return 0x7FC00000 if (b & 0x7FFFFFFF) > 0x7F800000 else b


def compare(physical_type, unsigned, a, b):
    """compare(a, b) of the column's PrimitiveComparator -> negative, 0 or positive."""
    if physical_type == abi.BOOLEAN:  # Boolean.compare
        a, b = bool(a), bool(b)
        return (a > b) - (a < b)
    if physical_type in (abi.INT32, abi.INT64):
        a, b = int(a), int(b)
        if unsigned:  # Integer.compareUnsigned: compare(x + MIN_VALUE, y + MIN_VALUE)
            mask = 0xFFFFFFFF if physical_type == abi.INT32 else 0xFFFFFFFFFFFFFFFF
            a, b = a & mask, b & mask
        return (a > b) - (a < b)
    if physical_type in (abi.FLOAT, abi.DOUBLE):  # Float.compare / Double.compare
        double = physical_type == abi.DOUBLE
        fa, fb = (np.float64(a), np.float64(b)) if double else (np.float32(a), np.float32(b))
        if fa < fb:
            return -1
        if fa > fb:
            return 1
        ba, bb = _float_bits(fa, double), _float_bits(fb, double)
        return 0 if ba == bb else (-1 if ba < bb else 1)
    if physical_type == abi.BYTE_ARRAY:  # Binary.lexicographicCompare: unsigned bytes, then length
        a, b = bytes(a), bytes(b)
        for x, y in zip(a, b):
            if x != y:
                return -1 if x < y else 1
        return (len(a) > len(b)) - (len(a) < len(b))
    raise ValueError(physical_type)


# ---- columns ------------------------------------------------------------------------------------------

class RefColumn:
    """A decoded flat column: dense non-null `values` in row order, one def level per row (None for
    a required column). missing=True: a column no value reaches (null in every row)."""

    def __init__(self, physical_type, values=(), def_levels=None, max_def=0, missing=False):
        self.physical_type = physical_type
        self.values = values
        self.def_levels = None if def_levels is None else np.asarray(def_levels, dtype=np.uint8)
        self.max_def = max_def
        self.missing = missing

    def valid(self, n_rows):
        if self.missing:
            return np.zeros(n_rows, dtype=bool)
        if self.max_def == 0:
            return np.ones(n_rows, dtype=bool)
        return self.def_levels[:n_rows] == self.max_def

    def row_values(self, n_rows):
        """Per row: the value, or None on a null row."""
        out, k = [], 0
        for ok in self.valid(n_rows):
            if ok:
                out.append(self.values[k])
                k += 1
            else:
                out.append(None)
        return out


# ---- ValueInspectors + evaluator, row by row ---------------------------------------------------------------

def leaf_row(p, physical_type, value):
    """One leaf on one row: `value` is None on a null row (updateNull), else update(value)."""
    op, lits = p.op, p.values
    uns = p.column.unsigned

    def cmp(lit):
        return compare(physical_type, uns, value, lit)

    if op in (abi.FILTER_LT, abi.FILTER_LTEQ, abi.FILTER_GT, abi.FILTER_GTEQ):
        if physical_type == abi.BOOLEAN:
            raise ValueError("Operator < / <= / > / >= not supported for Boolean")  # IllegalArgumentException
        if value is None:
            return False
        c = cmp(lits[0])
        return {abi.FILTER_LT: c < 0, abi.FILTER_LTEQ: c <= 0, abi.FILTER_GT: c > 0, abi.FILTER_GTEQ: c >= 0}[op]
    if op in (abi.FILTER_EQ, abi.FILTER_NOTEQ):
        if lits[0] is None:
            return (value is None) == (op == abi.FILTER_EQ)
        if value is None:
            return op == abi.FILTER_NOTEQ
        return (cmp(lits[0]) == 0) == (op == abi.FILTER_EQ)
    if any(v is None for v in lits):  # in / notIn with a null member
        return (value is None) == (op == abi.FILTER_IN)
    if value is None:
        return op == abi.FILTER_NOTIN
    found = any(cmp(v) == 0 for v in lits)
    return found == (op == abi.FILTER_IN)


def evaluate_rows(pred, columns, n_rows):
    """The rewritten predicate on every row -> bool array (IncrementallyUpdatedFilterPredicateEvaluator)."""
    pred = rewrite(pred)
    rows = {}

    def ev(p, r):
        if p.op == abi.FILTER_AND:
            return ev(p.children[0], r) and ev(p.children[1], r)
        if p.op == abi.FILTER_OR:
            return ev(p.children[0], r) or ev(p.children[1], r)
        assert p.op != abi.FILTER_NOT
        c = p.column.index
        if c not in rows:
            rows[c] = columns[c].row_values(n_rows)
        return leaf_row(p, columns[c].physical_type, rows[c][r])

    return np.array([ev(pred, r) for r in range(n_rows)], dtype=bool)


# ---- the same over arrays ----------------------------------------------------------------------------------

def key_array(physical_type, unsigned, values):
    """Comparator keys: a signed int64 (or, for unsigned INT64, uint64) array whose order is compare()'s."""
    if physical_type == abi.BOOLEAN:
        return (np.asarray(values) != 0).astype(np.int64)
    if physical_type == abi.INT32:
        v = np.asarray(values).astype(np.int32)
        return v.view(np.uint32).astype(np.int64) if unsigned else v.astype(np.int64)
    if physical_type == abi.INT64:
        v = np.asarray(values).astype(np.int64)
        return v.view(np.uint64) if unsigned else v
    if physical_type == abi.FLOAT:
        b = np.asarray(values, dtype=np.float32).view(np.int32).astype(np.int64)
        b = np.where((b & 0x7FFFFFFF) > 0x7F800000, 0x7FC00000, b)
        return np.where(b < 0, b ^ 0x7FFFFFFF, b)
    if physical_type == abi.DOUBLE:
        b = np.asarray(values, dtype=np.float64).view(np.int64).copy()
        b = np.where((b & 0x7FFFFFFFFFFFFFFF) > 0x7FF0000000000000, 0x7FF8000000000000, b)
        return np.where(b < 0, b ^ 0x7FFFFFFFFFFFFFFF, b)
    raise ValueError(physical_type)


def _leaf_array(p, col, n_rows):
    valid = col.valid(n_rows)
    op, lits, t = p.op, p.values, col.physical_type
    null_lit = any(v is None for v in lits)
    if null_lit:
        return ~valid if op in (abi.FILTER_EQ, abi.FILTER_IN) else valid.copy()
    n_valid = int(valid.sum())
    if t == abi.BYTE_ARRAY:
        vals = [bytes(v) for v in col.values[:n_valid]] if n_valid else []
        ls = [bytes(v) for v in lits]
        if op in (abi.FILTER_IN, abi.FILTER_NOTIN):
            s = set(ls)
            dense = np.array([v in s for v in vals], dtype=bool)
        else:
            lit = ls[0]  # bytes order in Python: unsigned lexicographic, then length
            fn = {abi.FILTER_EQ: lambda v: v == lit, abi.FILTER_NOTEQ: lambda v: v != lit, abi.FILTER_LT: lambda v: v < lit,
                  abi.FILTER_LTEQ: lambda v: v <= lit, abi.FILTER_GT: lambda v: v > lit, abi.FILTER_GTEQ: lambda v: v >= lit}[op]
            dense = np.array([fn(v) for v in vals], dtype=bool)
    else:
        keys = key_array(t, p.column.unsigned, np.asarray(col.values)[:n_valid] if n_valid else
                         np.zeros(0, dtype=abi.numpy_dtype(t)))
        if t in (abi.INT32, abi.INT64):  # literals may be written signed or unsigned: the same bits
            half = 1 << (31 if t == abi.INT32 else 63)
            lits = [((int(v) + half) % (2 * half)) - half for v in lits]
        lk = key_array(t, p.column.unsigned, np.array(list(lits), dtype=abi.numpy_dtype(t) if t != abi.BOOLEAN else np.uint8))
        if op in (abi.FILTER_IN, abi.FILTER_NOTIN):
            dense = np.isin(keys, lk)
        else:
            k = lk[0]
            dense = {abi.FILTER_EQ: keys == k, abi.FILTER_NOTEQ: keys != k, abi.FILTER_LT: keys < k,
                     abi.FILTER_LTEQ: keys <= k, abi.FILTER_GT: keys > k, abi.FILTER_GTEQ: keys >= k}[op]
    if op in (abi.FILTER_NOTIN,):
        dense = ~dense
    out = np.full(n_rows, op in (abi.FILTER_NOTEQ, abi.FILTER_NOTIN), dtype=bool)  # null rows
    out[valid] = dense
    return out


def evaluate(pred, columns, n_rows):
    """evaluate_rows over arrays."""
    def ev(p):
        if p.op == abi.FILTER_AND:
            return ev(p.children[0]) & ev(p.children[1])
        if p.op == abi.FILTER_OR:
            return ev(p.children[0]) | ev(p.children[1])
        assert p.op != abi.FILTER_NOT
        return _leaf_array(p, columns[p.column.index], n_rows)

    return ev(rewrite(pred))


def bitmap_words(bits):
    """Row r -> bit r & 63 of word r >> 6; the bits past the last row are 0."""
    n_words = (len(bits) + 63) // 64
    padded = np.zeros(n_words * 64, dtype=np.uint8)
    padded[:len(bits)] = bits
    return np.packbits(padded, bitorder="little").view("<u8") if n_words else np.zeros(0, dtype=np.uint64)


# ---- seeded random predicates ------------------------------------------------------------------------------

EDGE = {
    abi.BOOLEAN: [False, True],
    abi.INT32: [0, 1, -1, 2**31 - 1, -2**31, 7, 17],
    abi.INT64: [0, 1, -1, 2**63 - 1, -2**63, 7, 1 << 40],
    abi.FLOAT: [np.float32(x) for x in (0.0, -0.0, 1.5, -1.5, np.inf, -np.inf, np.nan, 3.4e38)] +
               [np.array([0xFFC00001], dtype=np.uint32).view(np.float32)[0]],
    abi.DOUBLE: [np.float64(x) for x in (0.0, -0.0, 1.5, -1.5, np.inf, -np.inf, np.nan, 1e308)] +
                [np.array([0xFFF8000000000123], dtype=np.uint64).view(np.float64)[0]],
    abi.BYTE_ARRAY: [b"", b"a", b"ab", b"abc", b"ab\x80", b"\x80", b"\xff\xff", b"b", b"abcdefgh", b"abcdefghi"],
}


def random_literal(rng, t):
    pool = EDGE[t]
    return pool[int(rng.integers(0, len(pool)))]


def random_predicate(rng, types, depth, allow_not=True):
    """A random tree of at most `depth` levels over columns of the given physical types."""
    r = rng.random()
    if depth > 1 and r < 0.6:
        if allow_not and r < 0.15:
            return F.not_(random_predicate(rng, types, depth - 1, allow_not))
        mk = F.and_ if rng.random() < 0.5 else F.or_
        return mk(random_predicate(rng, types, depth - 1, allow_not), random_predicate(rng, types, depth - 1, allow_not))
    c = int(rng.integers(0, len(types)))
    t = types[c]
    column = F.col(c, unsigned=bool(t in (abi.INT32, abi.INT64) and rng.random() < 0.3))
    ops = [F.eq, F.not_eq, F.in_, F.not_in] + ([] if t == abi.BOOLEAN else [F.lt, F.lt_eq, F.gt, F.gt_eq])
    mk = ops[int(rng.integers(0, len(ops)))]
    if mk in (F.in_, F.not_in):
        k = int(rng.integers(1, 12))
        vals = [random_literal(rng, t) for _ in range(k)]
        if rng.random() < 0.15:
            vals.append(None)
        return mk(column, vals)
    if mk in (F.eq, F.not_eq) and rng.random() < 0.15:
        return mk(column, None)
    return mk(column, random_literal(rng, t))
