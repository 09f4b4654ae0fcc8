"""Reference semantics of a row selection over decoded flat columns, restated in Python / numpy.
Test infrastructure only (the product is csrc/pqgpu_take*.{cpp,hip}).

What is restated: the records RecordReaderImplementation.read keeps when shouldSkipCurrentRecord names
the others (RecordReaderImplementation.java:440-449, filter2/recordlevel/FilteringRecordMaterializer.java),
and the rows SynchronizingColumnReader leaves after skipping those outside the RowRanges
(column/impl/SynchronizingColumnReader.java): the kept records in row order, every column showing
exactly the value or null it had.

Columns are filter_ref.RefColumn: dense non-null `values` in row order plus one definition level per
row (None for a required column). take() returns, per column, (def_levels_out, dense values_out):
  take_rows   row by row from the definition
  take        the same with numpy index arithmetic, for large inputs; the CPU tests hold them equal
A missing column yields (None, [])."""
import numpy as np

from pqgpu import abi


def _dense(col):
    """The column's values as something indexable by a numpy index array (bytes values: object array)."""
    v = col.values
    if isinstance(v, np.ndarray):
        return v
    a = np.empty(len(v), dtype=object)
    for i, x in enumerate(v):
        a[i] = x
    return a


def take_rows(columns, keep):
    """Row by row: walk the rows, count the values passed, keep what the mask keeps."""
    keep = np.asarray(keep, dtype=bool)
    out = []
    for col in columns:
        if col.missing:
            out.append((None, []))
            continue
        levels, values, k = [], [], 0  # k: dense index of the next row with a value
        for r in range(keep.size):
            has = col.max_def == 0 or col.def_levels[r] == col.max_def
            if keep[r]:
                if col.max_def > 0:
                    levels.append(int(col.def_levels[r]))
                if has:
                    values.append(col.values[k])
            k += has
        out.append((np.array(levels, dtype=np.uint8) if col.max_def > 0 else None, values))
    return out


def take(columns, keep):
    """Vectorised: the source index of row r is the number of rows with a value before r."""
    keep = np.asarray(keep, dtype=bool)
    n = keep.size
    out = []
    for col in columns:
        if col.missing:
            out.append((None, []))
            continue
        dense = _dense(col)
        if col.max_def == 0:
            out.append((None, dense[:n][keep]))
            continue
        dl = col.def_levels[:n]
        valid = dl == col.max_def
        src = np.cumsum(valid) - valid  # exclusive prefix: rows with a value before r
        out.append((dl[keep], dense[src[keep & valid]]))
    return out


def compose(m1, m2):
    """The mask over the original rows that take(take(x, m1), m2) keeps: m2 indexes the rows m1 kept."""
    m1 = np.asarray(m1, dtype=bool)
    m = np.zeros(m1.size, dtype=bool)
    m[np.flatnonzero(m1)[np.asarray(m2, dtype=bool)]] = True
    return m


def as_ref_columns(columns, taken):
    """RefColumns of a take's outcome (to take again, or to filter)."""
    import filter_ref as R
    out = []
    for col, (dl, vals) in zip(columns, taken):
        if col.missing:
            out.append(R.RefColumn(col.physical_type, max_def=col.max_def, missing=True))
        else:
            out.append(R.RefColumn(col.physical_type, vals, dl, col.max_def))
    return out


def values_equal(physical_type, got, want):
    """Bit-for-bit equality of two dense value sequences (floats by their bits)."""
    if physical_type == abi.BYTE_ARRAY:
        return len(got) == len(want) and all(bytes(a) == bytes(b) for a, b in zip(got, want))
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return len(got) == len(want) and (len(got) == 0 or (got.itemsize == want.itemsize and got.tobytes() == want.tobytes()))
