"""Reference semantics of parquet-mr's dictionary-level row-group filter, restated in Python on top of
tests/filter_ref.py. Test infrastructure only (the product is csrc/pqgpu_rowgroup*.{cpp,hip}).

What is restated (parquet-hadoop/src/main/java/org/apache/parquet/filter2/dictionarylevel/DictionaryFilter.java):
  expand_dictionary  expandDictionary (:91-131): no dictionary page, BOOLEAN and INT96 give None; otherwise a
                     real Python set of the entries under equals()
  leaf_cannot        visit(Eq) .. visit(NotIn) (:135-489), branch by branch and in the reference's order
  can_drop           visit(And) / visit(Or) (:496-504: "can drop" inverts them), visit(Contains) (:492-494 with
                     Operators.java:459-461: the inner predicate's verdict), on the predicate after
                     LogicalInverseRewriter, which is what RowGroupFilter hands over
  has_non_dictionary_pages   hasNonDictionaryPages (:561-589) with ParquetMetadataConverter.convertEncodingStats
                     (:689-709) and EncodingStats.hasNonDictionaryEncodedPages (EncodingStats.java:77-94)

equals(): Integer / Long by value (the same bits whether a literal is written signed or unsigned), Float / Double
by floatToIntBits / doubleToLongBits (one NaN, -0.0 != 0.0), Binary by its bytes whatever the column's comparator.
The ordering leaves use the column's comparator (filter_ref.compare, filter_binary_ref.compare)."""
import numpy as np

from pqgpu import abi

import filter_binary_ref as B
import filter_records_ref as RR
import filter_ref as R

DECODABLE = (abi.INT32, abi.INT64, abi.FLOAT, abi.DOUBLE, abi.BYTE_ARRAY, abi.FIXED_LEN_BYTE_ARRAY)
BINARY = (abi.BYTE_ARRAY, abi.FIXED_LEN_BYTE_ARRAY, abi.INT96)


class RefChunk:
    """One column chunk of one row group as DictionaryFilter sees it. entries: the dictionary page's values in id
    order (None: no dictionary page was read). missing: the file has no such column (meta == null)."""

    def __init__(self, physical_type, entries=None, missing=False, non_dictionary_pages=False, may_contain_null=True):
        self.physical_type = physical_type
        self.entries = entries
        self.missing = missing
        self.non_dictionary_pages = non_dictionary_pages
        self.may_contain_null = may_contain_null


def equals_key(physical_type, v):
    """A hashable key whose equality is equals() of the Java value."""
    if physical_type == abi.INT32:
        return int(v) & 0xFFFFFFFF
    if physical_type == abi.INT64:
        return int(v) & 0xFFFFFFFFFFFFFFFF
    if physical_type in (abi.FLOAT, abi.DOUBLE):
        return R._float_bits(np.float64(v) if physical_type == abi.DOUBLE else np.float32(v), physical_type == abi.DOUBLE)
    if physical_type in BINARY:
        return bytes(v)
    return bool(v)


def expand_dictionary(ch):
    if ch.entries is None or ch.physical_type not in DECODABLE:
        return None
    return {equals_key(ch.physical_type, e): e for e in ch.entries}  # key -> a representative entry


def _compare(p, physical_type, a, b):
    if physical_type in BINARY:
        return B.compare(getattr(p.column, "order", None), a, b)
    return R.compare(physical_type, p.column.unsigned, a, b)


def leaf_cannot(p, ch):
    """BLOCK_CANNOT_MATCH of one leaf on one chunk."""
    op, lits, t = p.op, p.values, ch.physical_type
    if op == abi.FILTER_EQ:
        if lits[0] is None:
            return False
        if ch.missing:
            return True
        if ch.non_dictionary_pages:
            return False
        d = expand_dictionary(ch)
        return d is not None and equals_key(t, lits[0]) not in d
    if op == abi.FILTER_NOTEQ:
        if lits[0] is None:
            return ch.missing
        if ch.missing or ch.non_dictionary_pages:
            return False
        d = expand_dictionary(ch)
        return d is not None and len(d) == 1 and equals_key(t, lits[0]) in d and not ch.may_contain_null
    if op in (abi.FILTER_LT, abi.FILTER_LTEQ, abi.FILTER_GT, abi.FILTER_GTEQ):
        if ch.missing:
            return True
        if ch.non_dictionary_pages:
            return False
        d = expand_dictionary(ch)
        if d is None:
            return False
        for entry in d.values():
            c = _compare(p, t, lits[0], entry)  # comparator.compare(value, entry)
            if {abi.FILTER_LT: c > 0, abi.FILTER_LTEQ: c >= 0, abi.FILTER_GT: c < 0, abi.FILTER_GTEQ: c <= 0}[op]:
                return False
        return True
    has_null = any(v is None for v in lits)
    if op == abi.FILTER_IN:
        if has_null:
            return False
        if ch.missing:
            return True
        if ch.non_dictionary_pages:
            return False
        d = expand_dictionary(ch)
        if d is None:
            return False
        return not ({equals_key(t, v) for v in lits} & set(d))
    assert op == abi.FILTER_NOTIN
    if len(set(lits)) == 1 and has_null and ch.missing:
        return True
    if has_null or ch.missing or ch.may_contain_null or ch.non_dictionary_pages:
        return False
    d = expand_dictionary(ch)
    if d is None:
        return False
    return set(d) <= {equals_key(t, v) for v in lits}


def can_drop(pred, chunks):
    """DictionaryFilter.canDrop(pred, columns, dictionaries) for one row group: chunks[c] is the RefChunk of
    column c."""
    def ev(p):
        if p.op == abi.FILTER_AND:
            return ev(p.children[0]) or ev(p.children[1])
        if p.op == abi.FILTER_OR:
            return ev(p.children[0]) and ev(p.children[1])
        if p.op == abi.FILTER_CONTAINS:
            return ev(p.children[0])
        assert p.op != abi.FILTER_NOT
        return leaf_cannot(p, chunks[p.column.index])

    return ev(RR.li_rewrite(pred))


def drops(pred, row_groups):
    """can_drop per row group -> bool array."""
    return np.array([can_drop(pred, g) for g in row_groups], dtype=bool)


def has_non_dictionary_pages(encoding_stats, encodings):
    """encoding_stats: None or [(page_type, encoding, count)]; encodings: the chunk's encodings list."""
    if encoding_stats is not None:
        data = {e for t, e, _ in encoding_stats if t in (abi.DATA_PAGE, abi.DATA_PAGE_V2)}
        if not data:
            return False
        if abi.RLE_DICTIONARY in data:
            data.remove(abi.RLE_DICTIONARY)
        elif abi.PLAIN_DICTIONARY in data:
            data.remove(abi.PLAIN_DICTIONARY)
        else:
            return True
        return bool(data)
    enc = set(encodings)
    if abi.PLAIN_DICTIONARY not in enc:
        return True
    return bool(enc - {abi.PLAIN_DICTIONARY, abi.RLE, abi.BIT_PACKED})
