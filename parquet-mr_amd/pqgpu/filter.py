"""filter2 record predicates over decoded columns: the Python face of pqg_filter_* (include/pqgpu.h).

A small predicate DSL named after parquet-mr's FilterApi (filter2/predicate/FilterApi.java):

    from pqgpu import filter as F
    pred = F.and_(F.lt_eq(F.col(0), 9_000), F.not_(F.eq(F.col(2), None)))
    sel = decoder.filter(pred, cols, n_rows)      # cols: the DeviceColumns decode() returned
    sel.count, sel.bitmap, sel.row_ids

`contains(leaf)` is FilterApi.contains on a repeated column: Decoder.filter_records evaluates it per record.
`col(i, order=...)` names the comparator of a binary column ("unsigned_bytes", "signed_integer" for DECIMAL and
INT96, "float16") and makes FIXED_LEN_BYTE_ARRAY and INT96 columns filterable (pqg_filter_create_typed); their
literals are bytes, e.g. `decimal_bytes(-129)`.
`None` is the null literal (eq / not_eq, or a member of an in_ / not_in set). `compile` flattens a
predicate to the node, literal and byte tables of the C ABI; `Filter` is the created pqg_filter
(validated and rewritten without not(), as FilterCompat.get does with LogicalInverseRewriter).
"""
import ctypes as C

import numpy as np

from . import abi, native

_LEAF_OPS = {"eq": abi.FILTER_EQ, "not_eq": abi.FILTER_NOTEQ, "lt": abi.FILTER_LT, "lt_eq": abi.FILTER_LTEQ,
             "gt": abi.FILTER_GT, "gt_eq": abi.FILTER_GTEQ, "in": abi.FILTER_IN, "not_in": abi.FILTER_NOTIN}
OP_NAMES = {v: k for k, v in _LEAF_OPS.items()}
OP_NAMES.update({abi.FILTER_AND: "and", abi.FILTER_OR: "or", abi.FILTER_NOT: "not", abi.FILTER_CONTAINS: "contains"})


class Column:
    """A column of the row group by index; unsigned=True for UINT_32 / UINT_64 annotated columns; order: the
    comparator of a BYTE_ARRAY / FIXED_LEN_BYTE_ARRAY / INT96 column (None: as pqg_filter_create has it)."""

    def __init__(self, index, unsigned=False, order=None):
        if order is not None and order not in abi.FILTER_ORDER_NAMES:
            raise ValueError(f"order must be None or one of {sorted(abi.FILTER_ORDER_NAMES)}, not {order!r}")
        self.index = int(index)
        self.unsigned = bool(unsigned)
        self.order = order


class Predicate:
    """A node of a predicate tree: a leaf (op, column, values) or and / or / not over children."""

    def __init__(self, op, column=None, values=(), children=()):
        self.op = op
        self.column = column
        self.values = tuple(values)
        self.children = tuple(children)

    def __repr__(self):
        if self.children:
            return f"{OP_NAMES[self.op]}({', '.join(map(repr, self.children))})"
        vals = self.values[0] if self.op < abi.FILTER_IN else set(self.values)
        return f"{OP_NAMES[self.op]}(col{self.column.index}{'u' if self.column.unsigned else ''}, {vals!r})"


def col(index, unsigned=False, order=None):
    return Column(index, unsigned, order)


def decimal_bytes(unscaled, length=None):
    """The big-endian two's-complement bytes of the integer `unscaled` (a DECIMAL's unscaled value, an INT96):
    the fewest that hold it, or sign-extended to `length` bytes. For literals of a "signed_integer" column."""
    unscaled = int(unscaled)
    n = (unscaled if unscaled >= 0 else ~unscaled).bit_length() // 8 + 1
    if length is not None:
        if length < n:
            raise OverflowError(f"{unscaled} does not fit {length} bytes")
        n = int(length)
    return unscaled.to_bytes(n, "big", signed=True)


def _leaf(op, column, values):
    if not isinstance(column, Column):
        column = Column(column)
    return Predicate(op, column, values)


def eq(column, value): return _leaf(abi.FILTER_EQ, column, (value,))
def not_eq(column, value): return _leaf(abi.FILTER_NOTEQ, column, (value,))
def lt(column, value): return _leaf(abi.FILTER_LT, column, (value,))
def lt_eq(column, value): return _leaf(abi.FILTER_LTEQ, column, (value,))
def gt(column, value): return _leaf(abi.FILTER_GT, column, (value,))
def gt_eq(column, value): return _leaf(abi.FILTER_GTEQ, column, (value,))
def in_(column, values): return _leaf(abi.FILTER_IN, column, tuple(values))
def not_in(column, values): return _leaf(abi.FILTER_NOTIN, column, tuple(values))
def and_(left, right): return Predicate(abi.FILTER_AND, children=(left, right))
def or_(left, right): return Predicate(abi.FILTER_OR, children=(left, right))
def not_(pred): return Predicate(abi.FILTER_NOT, children=(pred,))


def contains(leaf):
    """FilterApi.contains: some element of the record's list satisfies `leaf` (eq .. not_in on a repeated
    column; Decoder.filter_records evaluates it)."""
    return Predicate(abi.FILTER_CONTAINS, children=(leaf,))


def literal_cell(physical_type, value):
    """The 8-byte literal cell of a non-null value of a fixed-width type (raw value bits)."""
    if physical_type == abi.BOOLEAN:
        return int(bool(value))
    if physical_type == abi.INT32:
        return int(value) & 0xFFFFFFFF
    if physical_type == abi.INT64:
        return int(value) & 0xFFFFFFFFFFFFFFFF
    if physical_type == abi.FLOAT:
        return int(np.asarray(value, dtype=np.float32).reshape(1).view(np.uint32)[0])
    if physical_type == abi.DOUBLE:
        return int(np.asarray(value, dtype=np.float64).reshape(1).view(np.uint64)[0])
    raise native.PqgError(abi.ERR_UNSUPPORTED, what=f"filter literal of type {abi.TYPE_NAMES.get(physical_type)}")


class Compiled:
    """The C ABI tables of a predicate: nodes (post-order, root last), literal cells, literal bytes."""

    def __init__(self, nodes, literals, literal_bytes, column_types, typed=None):
        self.nodes = nodes                  # list of (op, column, left, right, flags, literal_begin, n_literals)
        self.literals = literals            # list of int cells
        self.literal_bytes = literal_bytes  # bytes
        self.column_types = column_types    # list of pqg_physical_type
        self.typed = typed                  # None, or list of (physical_type, type_length, binary_order): create_typed


def column_types(columns):
    """Physical types of `columns`: ints, or objects with .physical_type (DeviceColumn, MissingColumn).
    A column decoded as dictionary ids counts with its dictionary's type when it carries the decoded
    dictionary (DeviceColumn.dictionary, from Decoder.decode_dictionary); without one it is refused."""
    out = []
    for c in columns:
        if getattr(c, "flags", 0) & abi.COLUMN_DICTIONARY_IDS:
            d = getattr(c, "dictionary", None)
            if d is None:
                raise native.PqgError(abi.ERR_UNSUPPORTED, what="filter on a column decoded as dictionary ids")
            out.append(int(d.physical_type))
        else:
            out.append(int(getattr(c, "physical_type", c)))
    return out


def _type_length(column):
    """type_length of a column object (of its dictionary for an ids column); 0 for a bare type."""
    if getattr(column, "flags", 0) & abi.COLUMN_DICTIONARY_IDS:
        column = getattr(column, "dictionary", None)
    return int(getattr(column, "type_length", 0) or 0)


def compile(pred, columns):
    """Flatten `pred` (post-order: left, right, node) to the tables pqg_filter_create takes, or, when a column
    the predicate names carries an `order`, pqg_filter_create_typed (Compiled.typed)."""
    types = column_types(columns)
    nodes, literals, blob = [], [], bytearray()
    orders = {}  # column index -> order name, of the columns named with one

    def walk(p):
        if p.children:
            kids = [walk(k) for k in p.children]
            nodes.append((p.op, -1, kids[0], kids[1] if len(kids) > 1 else -1, 0, 0, 0))
            return len(nodes) - 1
        c = p.column
        flags = abi.FILTER_UNSIGNED if c.unsigned else 0
        values = p.values
        if any(v is None for v in values):
            flags |= abi.FILTER_NULL_LITERAL
            values = [v for v in values if v is not None]
        t = types[c.index] if 0 <= c.index < len(types) else None
        order = getattr(c, "order", None)
        if order is not None:
            if orders.setdefault(c.index, order) != order:
                raise ValueError(f"column {c.index} is named with two orders: {orders[c.index]!r} and {order!r}")
        begin = len(literals)
        for v in values:
            if t == abi.BYTE_ARRAY or (order is not None and t in (abi.INT96, abi.FIXED_LEN_BYTE_ARRAY)):
                b = bytes(v)
                literals.append(len(blob) | (len(b) << 32))
                blob.extend(b)
            elif t is None or t in (abi.INT96, abi.FIXED_LEN_BYTE_ARRAY):
                literals.append(0)  # pqg_filter_create rejects the column
            else:
                literals.append(literal_cell(t, v))
        nodes.append((p.op, c.index, -1, -1, flags, begin, len(values)))
        return len(nodes) - 1

    walk(pred)
    typed = None
    if orders:
        typed = []
        for i, t in enumerate(types):
            tl = _type_length(columns[i]) if t == abi.FIXED_LEN_BYTE_ARRAY else 0
            typed.append((t, tl, abi.FILTER_ORDER_NAMES[orders[i]] if i in orders else 0))
    return Compiled(nodes, literals, bytes(blob), types, typed)


def _tables(nodes, literals, literal_bytes):
    """The node, literal and byte tables as ctypes / numpy arrays (never empty: one spare element each)."""
    arr = (abi.FilterNode * max(1, len(nodes)))()
    for i, nd in enumerate(nodes):
        (arr[i].op, arr[i].column, arr[i].left, arr[i].right, arr[i].flags, arr[i].literal_begin,
         arr[i].n_literals) = nd
    lit = np.asarray(literals, dtype=np.uint64) if len(literals) else np.zeros(1, dtype=np.uint64)
    blob = np.frombuffer(bytes(literal_bytes) + b"\0", dtype=np.uint8)
    return arr, lit, blob


def create(nodes, literals, literal_bytes, types, n_literals=None, n_literal_bytes=None):
    """pqg_filter_create over raw tables -> (rc, handle, status). The table sizes may be overridden
    (tests hand in sizes that disagree with the tables)."""
    arr, lit, blob = _tables(nodes, literals, literal_bytes)
    ty = np.asarray(list(types) or [0], dtype=np.int32)
    h = C.c_void_p()
    st = abi.Status()
    rc = native.lib().pqg_filter_create(
        C.addressof(arr), len(nodes), ty.ctypes.data, len(types), lit.ctypes.data,
        len(literals) if n_literals is None else n_literals, blob.ctypes.data,
        len(literal_bytes) if n_literal_bytes is None else n_literal_bytes, C.byref(h), C.byref(st))
    return rc, h, st


def create_typed(nodes, literals, literal_bytes, columns, n_literals=None, n_literal_bytes=None):
    """pqg_filter_create_typed over raw tables -> (rc, handle, status); `columns`: (physical_type, type_length,
    binary_order) or (..., reserved) per column."""
    arr, lit, blob = _tables(nodes, literals, literal_bytes)
    ct = (abi.FilterColumnType * max(1, len(columns)))()
    for i, c in enumerate(columns):
        ct[i].physical_type, ct[i].type_length, ct[i].binary_order = c[:3]
        ct[i].reserved = c[3] if len(c) > 3 else 0
    h = C.c_void_p()
    st = abi.Status()
    rc = native.lib().pqg_filter_create_typed(
        C.addressof(arr), len(nodes), C.addressof(ct), len(columns), lit.ctypes.data,
        len(literals) if n_literals is None else n_literals, blob.ctypes.data,
        len(literal_bytes) if n_literal_bytes is None else n_literal_bytes, C.byref(h), C.byref(st))
    return rc, h, st


class Filter:
    """A created pqg_filter: `pred` validated and rewritten without not()."""

    def __init__(self, pred, columns):
        self.compiled = compile(pred, columns)
        c = self.compiled
        if c.typed is not None:
            rc, self.handle, st = create_typed(c.nodes, c.literals, c.literal_bytes, c.typed)
        else:
            rc, self.handle, st = create(c.nodes, c.literals, c.literal_bytes, c.column_types)
        native.check(rc, st, "pqg_filter_create_typed" if c.typed is not None else "pqg_filter_create")
        self.n_cols = len(c.column_types)

    def program(self):
        """The rewritten program: list of (op, column, left, right, flags, literal_begin, n_literals)."""
        return program(self.handle)

    def close(self):
        if self.handle:
            native.lib().pqg_filter_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def program(handle):
    out = (abi.FilterNode * abi.FILTER_MAX_NODES)()
    n = native.lib().pqg_filter_program(handle, C.addressof(out), abi.FILTER_MAX_NODES)
    return [(o.op, o.column, o.left, o.right, o.flags, o.literal_begin, o.n_literals) for o in out[:n]]


class MissingColumn:
    """A column of the requested schema that the file does not have: null in every row
    (TestFiltersWithMissingColumns)."""

    def __init__(self, physical_type, max_def=1):
        self.physical_type = physical_type
        self.max_def = max(1, int(max_def))
        self.values = self.def_levels = self.binary_data = None
        self.n_values = 0


class Selection:
    """Outcome of Decoder.filter: `bitmap` (torch int64 view of the uint64 words: row r is bit r & 63 of
    word r >> 6), `row_ids` (torch int64, ascending; None when not asked for) and `count`."""

    def __init__(self, decoder, n_rows, words, ids, result, capacity):
        self._decoder = decoder
        self.n_rows = n_rows
        self.bitmap = words
        self._ids = ids
        self._result = result
        self._capacity = capacity
        self._host = None

    def _sync(self):
        if self._host is None:
            self._decoder.stream.synchronize()
            r = self._result.cpu().numpy()
            n = int(r[:8].view(np.uint64)[0])
            err, err_col = (int(x) for x in r[8:16].view(np.int32))
            if err != abi.OK:
                why = ("a dictionary id outside the dictionary" if err == abi.ERR_DICT_ID else
                       "rows with a value differ from n_values")
                raise native.PqgError(err, what=f"pqg_filter_run: column {err_col}: {why}")
            self._host = n
        return self._host

    @property
    def count(self):
        """Rows selected (the full count, whatever the row id capacity); waits for the stream."""
        return self._sync()

    @property
    def row_ids(self):
        if self._ids is None:
            return None
        return self._ids[:min(self._sync(), self._capacity)]


class ColumnType:
    """A column known by its type alone: what Filter needs of a column (Decoder.filter_row_groups has no
    decoded columns to take the types from)."""

    def __init__(self, physical_type, type_length=0):
        self.physical_type = int(physical_type)
        self.type_length = int(type_length or 0)


class RowGroupColumn:
    """What a reader knows of one column chunk of one row group before it reads a page (Decoder.filter_row_groups):
    `dictionary`, the chunk's decoded dictionary page (the DeviceColumn of Decoder.decode_dictionary /
    decode_dictionaries; None: no dictionary page was read); missing: the file has no such column;
    non_dictionary_pages: framing.has_non_dictionary_pages of the chunk's metadata; may_contain_null: the chunk's
    statistics are absent, leave num_nulls unset or count a null. physical_type / type_length name the column's type
    where no row group carries a dictionary for it (they default to the dictionary's)."""

    def __init__(self, dictionary=None, missing=False, non_dictionary_pages=False, may_contain_null=True,
                 physical_type=None, type_length=0):
        self.dictionary = dictionary
        self.missing = bool(missing)
        self.non_dictionary_pages = bool(non_dictionary_pages)
        self.may_contain_null = bool(may_contain_null)
        self.physical_type = dictionary.physical_type if physical_type is None and dictionary is not None else physical_type
        self.type_length = int(getattr(dictionary, "type_length", 0) or 0) if dictionary is not None else int(type_length)

    @property
    def flags(self):
        return ((abi.RG_MISSING if self.missing else 0) | (abi.RG_NO_DICTIONARY if self.dictionary is None else 0) |
                (abi.RG_NON_DICT_PAGES if self.non_dictionary_pages else 0) |
                (abi.RG_MAY_CONTAIN_NULL if self.may_contain_null else 0))


class RowGroupSelection:
    """Outcome of Decoder.filter_row_groups: `drop` (torch bool, one per row group: the group cannot match),
    `kept` (torch int64, the other groups ascending, at most the capacity asked for), `count` (how many are kept) and `bitmap` (the int64 view of
    the uint64 words: group g is bit g & 63 of word g >> 6). Reading any of the first three waits for the stream."""

    def __init__(self, decoder, n_row_groups, words, ids, result, capacity):
        self._decoder = decoder
        self._capacity = capacity
        self.n_row_groups = n_row_groups
        self.bitmap = words
        self._ids = ids
        self._result = result
        self._host = None

    def _sync(self):
        if self._host is None:
            self._decoder.stream.synchronize()
            r = self._result.cpu().numpy()
            err, group = (int(x) for x in r[8:16].view(np.int32))
            if err != abi.OK:
                raise native.PqgError(err, what=f"pqg_filter_row_groups: row group {group}")
            self._host = int(r[:8].view(np.uint64)[0])
        return self._host

    @property
    def count(self):
        return self._sync()

    @property
    def kept(self):
        return self._ids[:min(self._sync(), self._capacity)]

    @property
    def drop(self):
        import torch
        self._sync()
        shifts = torch.arange(64, dtype=torch.int64, device=self.bitmap.device)
        bits = (self.bitmap.unsqueeze(1) >> shifts) & 1
        return bits.reshape(-1)[:self.n_row_groups].to(torch.bool)
