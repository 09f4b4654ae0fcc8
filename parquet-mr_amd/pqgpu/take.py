"""Row selection: the Python face of pqg_take (include/pqgpu.h, "row selection").

    sel = decoder.filter(pred, cols, n_rows)          # or any int64 bitmap tensor, e.g. of RowRanges
    taken = decoder.take(sel, cols)                   # asynchronous, no sync after the filter
    taken.n_rows, taken.columns                       # wait for the stream once

The returned columns are DeviceColumns in the decoder's own layout (dense values + one level byte per
kept row), so they are valid inputs to Decoder.filter and Decoder.take again.

    taken = decoder.take_records(sel, cols)           # pqg_take_records: repeated columns too, whole records

keeps the records the selection names in every column, lists included (their repetition and definition
bytes and dense values); its columns go into take_records again or into Decoder.assemble.
"""
import ctypes as C

import numpy as np
import torch

from . import abi, native


def is_missing(col):
    return col.max_def > 0 and col.def_levels is None


def is_binary(col):
    return col.physical_type == abi.BYTE_ARRAY and not (getattr(col, "flags", 0) & abi.COLUMN_DICTIONARY_IDS)


def elem_width(col):
    """Bytes per dense element as pqg_take moves them (BYTE_ARRAY: the 8-byte offsets)."""
    if getattr(col, "flags", 0) & abi.COLUMN_DICTIONARY_IDS:
        return 4
    return abi.elem_width(col.physical_type, getattr(col, "type_length", 0))


class Output:
    """Where one column of a take goes: uint8 device tensors (None where the column needs none) and the
    capacities stated to pqg_take, which default to what the tensors hold."""

    def __init__(self, values=None, def_levels=None, binary_data=None, values_capacity=None, binary_capacity=None):
        self.values = values
        self.def_levels = def_levels
        self.binary_data = binary_data
        self.values_capacity = values_capacity
        self.binary_capacity = binary_capacity


def default_capacities(col, n_rows, rows_capacity):
    """(values, bytes) upper bounds known on the host without a sync."""
    if is_missing(col):
        return 0, 0
    n_bytes = int(col.binary_data.numel()) if is_binary(col) else 0
    return min(int(col.n_values), rows_capacity), n_bytes


def alloc_output(device, col, n_rows, rows_capacity, fill=None, slack=0):
    """An Output for `col` at the default capacities, with `slack` extra elements / bytes the capacities
    do not state; fill: byte value written over the tensors."""
    if is_missing(col):
        return Output()
    cap_v, cap_b = default_capacities(col, n_rows, rows_capacity)
    w = elem_width(col)

    def buf(n):
        t = torch.empty(max(n, 16), dtype=torch.uint8, device=device)
        if fill is not None:
            t.fill_(fill)
        return t
    binary = is_binary(col)
    values = buf(((cap_v + 1 if binary else cap_v) + slack) * w)
    levels = buf(rows_capacity + slack) if col.max_def > 0 else None
    data = buf(cap_b + slack) if binary else None
    return Output(values, levels, data, cap_v, cap_b)


class Taken:
    """Outcome of Decoder.take: `n_rows` (kept rows) and `columns` (new DeviceColumns / MissingColumns);
    both wait for the stream once and raise PqgError when the device reported an error."""

    def __init__(self, decoder, cols, state, calls, rows_capacity):
        self._decoder = decoder
        self._cols = cols          # the output columns, n_values not yet set
        self._state = state        # uint8 tensor: per call, pqg_take_result then its pqg_take_counts
        self._calls = calls        # [(first column, n columns, byte offset into state, [(cap values, cap bytes)])]
        self._rows_capacity = rows_capacity
        self._host = None

    def _sync(self):
        if self._host is not None:
            return self._host
        self._decoder.stream.synchronize()
        raw = self._state.cpu().numpy()
        n_rows, counts = 0, []
        for first, n, off, caps in self._calls:
            n_rows = int(raw[off:off + 8].view(np.uint64)[0])
            err, err_col = (int(x) for x in raw[off + 8:off + 16].view(np.int32))
            cnt = raw[off + 16:off + 16 + 16 * n].view(np.uint64).reshape(n, 2)
            if err != abi.OK:
                col = first + err_col if err_col >= 0 else -1
                over = n_rows > self._rows_capacity or (err_col >= 0 and (int(cnt[err_col, 0]) > caps[err_col][0] or
                                                                         int(cnt[err_col, 1]) > caps[err_col][1]))
                why = "a count exceeds its capacity" if over else "rows with a value differ from n_values"
                e = native.PqgError(err, what=f"pqg_take: column {col}: {why}")
                e.column = col
                e.n_rows = n_rows
                e.counts = [(int(a), int(b)) for a, b in cnt]
                raise e
            counts.extend((int(a), int(b)) for a, b in cnt)
        for col, (nv, _) in zip(self._cols, counts):
            col.n_values = nv
            if col.def_levels is not None:
                col.def_levels = col.def_levels[:max(n_rows, 1)]
        self.counts = counts
        self._host = n_rows
        return n_rows

    @property
    def n_rows(self):
        """Rows kept (the full count, whatever the capacities)."""
        return self._sync()

    @property
    def columns(self):
        self._sync()
        return self._cols


def take(decoder, selection, cols, n_rows=None, rows_capacity=None, out=None):
    """Decoder.take."""
    from . import decoder as D
    from . import filter as F
    if isinstance(selection, F.Selection):
        bitmap, n_rows = selection.bitmap, selection.n_rows
    else:
        bitmap = selection
        if n_rows is None:
            raise native.PqgError(abi.ERR_INVALID_ARG, what="take: a bitmap tensor needs n_rows")
        if bitmap.dtype != torch.int64 or bitmap.numel() < (n_rows + 63) // 64:
            raise native.PqgError(abi.ERR_INVALID_ARG, what="take: the bitmap is an int64 tensor of ceil(n_rows / 64) words")
    n_rows = int(n_rows)
    rows_capacity = n_rows if rows_capacity is None else min(int(rows_capacity), n_rows)
    for c in cols:
        if getattr(c, "max_rep", 0) or getattr(c, "rep_levels", None) is not None:
            raise native.PqgError(abi.ERR_UNSUPPORTED, what="take on a repeated column")
    dev = decoder.device
    if out is None:
        out = [alloc_output(dev, c, n_rows, rows_capacity) for c in cols]
    n_calls = max(1, -(-len(cols) // abi.TAKE_MAX_COLUMNS))
    state = torch.empty(16 * n_calls + 16 * max(len(cols), 1), dtype=torch.uint8, device=dev)
    decoder.stream.wait_stream(torch.cuda.current_stream(dev))  # allocations / fills first
    new_cols, calls, off = [], [], 0
    for first in range(0, max(len(cols), 1), abi.TAKE_MAX_COLUMNS):
        part = cols[first:first + abi.TAKE_MAX_COLUMNS]
        arr = (abi.TakeColumn * max(1, len(part)))()
        caps = []
        for i, c in enumerate(part):
            o = out[first + i]
            dflt = default_capacities(c, n_rows, rows_capacity)
            cap_v = dflt[0] if o.values_capacity is None else int(o.values_capacity)
            cap_b = dflt[1] if o.binary_capacity is None else int(o.binary_capacity)
            a = arr[i]
            a.physical_type, a.max_def = c.physical_type, c.max_def
            a.type_length, a.flags = getattr(c, "type_length", 0), getattr(c, "flags", 0)
            a.values = c.values.data_ptr() if c.values is not None else None
            a.binary_data = c.binary_data.data_ptr() if c.binary_data is not None else None
            a.def_levels = c.def_levels.data_ptr() if c.def_levels is not None else None
            a.n_values = c.n_values
            a.out_values = o.values.data_ptr() if o.values is not None else None
            a.out_binary_data = o.binary_data.data_ptr() if o.binary_data is not None else None
            a.out_def_levels = o.def_levels.data_ptr() if o.def_levels is not None else None
            a.out_values_capacity, a.out_binary_capacity = cap_v, cap_b
            caps.append((cap_v, cap_b))
            if is_missing(c):
                new_cols.append(F.MissingColumn(c.physical_type, c.max_def))
            else:
                nc = D.DeviceColumn(c.physical_type, o.values, o.def_levels, None, getattr(c, "type_length", 0), o.binary_data)
                nc.max_def, nc.flags = c.max_def, getattr(c, "flags", 0)
                new_cols.append(nc)
        rc = native.lib().pqg_take(decoder.ctx, bitmap.data_ptr(), n_rows, C.addressof(arr), len(part), rows_capacity,
                                   state.data_ptr() + off + 16, state.data_ptr() + off)
        native.check(rc, what="pqg_take")
        calls.append((first, len(part), off, caps))
        off += 16 + 16 * len(part)
    taken = Taken(decoder, new_cols, state, calls, rows_capacity)
    taken._keep = (selection, cols, out)
    return taken


# ---- whole records: repeated columns too (pqg_take_records) -------------------------------------------

def slots_of(col, n_rows):
    """Level bytes of a column: its slots (a repeated leaf), its rows (a flat one)."""
    if getattr(col, "max_rep", 0) > 0:
        return int(col.n_slots)
    return n_rows


class RecordOutput(Output):
    """Output plus the repetition bytes of a repeated column and the slot capacity stated for it."""

    def __init__(self, values=None, def_levels=None, binary_data=None, values_capacity=None, binary_capacity=None,
                 rep_levels=None, slots_capacity=None):
        super().__init__(values, def_levels, binary_data, values_capacity, binary_capacity)
        self.rep_levels = rep_levels
        self.slots_capacity = slots_capacity


def default_record_capacities(col, n_rows, rows_capacity):
    """(slots, values, bytes) upper bounds known on the host without a sync."""
    if is_missing(col):
        return 0, 0, 0
    n_bytes = int(col.binary_data.numel()) if is_binary(col) else 0
    if getattr(col, "max_rep", 0) > 0:
        return int(col.n_slots), int(col.n_values), n_bytes
    return rows_capacity, min(int(col.n_values), rows_capacity), n_bytes


def alloc_record_output(device, col, n_rows, rows_capacity, fill=None, slack=0):
    """A RecordOutput for `col` at the default capacities (alloc_output for a flat column)."""
    if is_missing(col):
        return RecordOutput()
    if getattr(col, "max_rep", 0) == 0:
        o = alloc_output(device, col, n_rows, rows_capacity, fill, slack)
        return RecordOutput(o.values, o.def_levels, o.binary_data, o.values_capacity, o.binary_capacity)
    cap_s, cap_v, cap_b = default_record_capacities(col, n_rows, rows_capacity)
    w = elem_width(col)

    def buf(n):
        t = torch.empty(max(n, 16), dtype=torch.uint8, device=device)
        if fill is not None:
            t.fill_(fill)
        return t
    binary = is_binary(col)
    return RecordOutput(buf(((cap_v + 1 if binary else cap_v) + slack) * w), buf(cap_s + slack),
                        buf(cap_b + slack) if binary else None, cap_v, cap_b, buf(cap_s + slack), cap_s)


class TakenRecords:
    """Outcome of Decoder.take_records: `n_rows` (kept records), `columns` (DeviceColumns carrying rep_levels,
    def_levels, n_slots and n_values; MissingColumns) and `counts` ((records, slots, values, bytes) per
    column); they wait for the stream once and raise PqgError when the device reported an error."""

    def __init__(self, decoder, cols, state, calls, n_rows_in, rows_capacity):
        self._decoder = decoder
        self._cols = cols
        self._state = state    # uint8 tensor: per call, pqg_take_result then its pqg_take_record_counts
        self._calls = calls    # [(first column, n columns, byte offset into state, [(max_rep, cap slots, cap values, cap bytes, n_values)])]
        self._n_rows_in = n_rows_in
        self._rows_capacity = rows_capacity
        self._host = None

    def _why(self, n_rows, cnt, info):
        max_rep, cap_s, cap_v, cap_b, n_values_in = info
        rec, slots, vals, nbytes = (int(x) for x in cnt)
        if n_rows > self._rows_capacity:
            return f"a count exceeds its capacity: {n_rows} kept records, room for {self._rows_capacity}"
        if max_rep > 0 and rec != self._n_rows_in:
            return f"the column holds {rec} records, the selection {self._n_rows_in}"
        if slots > cap_s or vals > cap_v or nbytes > cap_b:
            return (f"a count exceeds its capacity: {slots} slots / {vals} values / {nbytes} bytes kept, room for "
                    f"{cap_s} / {cap_v} / {cap_b}")
        what = "slots with a value differ from n_values" if max_rep > 0 else "rows with a value differ from n_values"
        return f"{what} ({n_values_in})" + (", or slot 0 continues a record" if max_rep > 0 else "")

    def _sync(self):
        if self._host is not None:
            return self._host
        self._decoder.stream.synchronize()
        raw = self._state.cpu().numpy()
        n_rows, counts = 0, []
        for first, n, off, infos in self._calls:
            n_rows = int(raw[off:off + 8].view(np.uint64)[0])
            err, err_col = (int(x) for x in raw[off + 8:off + 16].view(np.int32))
            cnt = raw[off + 16:off + 16 + 32 * n].view(np.uint64).reshape(n, 4)
            if err != abi.OK:
                col = first + err_col if err_col >= 0 else -1
                why = self._why(n_rows, cnt[err_col], infos[err_col]) if err_col >= 0 else "a count exceeds its capacity"
                e = native.PqgError(err, what=f"pqg_take_records: column {col}: {why}")
                e.column = col
                e.n_rows = n_rows
                e.counts = [tuple(int(x) for x in row) for row in cnt]
                raise e
            counts.extend(tuple(int(x) for x in row) for row in cnt)
        for col, (_, ns, nv, _) in zip(self._cols, counts):
            if col.values is None and col.def_levels is None:
                continue  # a missing column
            col.n_values = nv
            col.n_slots = ns
            if col.def_levels is not None:
                col.def_levels = col.def_levels[:max(ns, 1)]
            if col.rep_levels is not None:
                col.rep_levels = col.rep_levels[:max(ns, 1)]
        self.counts = counts
        self._host = n_rows
        return n_rows

    @property
    def n_rows(self):
        """Records kept (the full count, whatever the capacities)."""
        return self._sync()

    @property
    def columns(self):
        self._sync()
        return self._cols


def take_records(decoder, selection, cols, n_rows=None, rows_capacity=None, out=None):
    """Decoder.take_records."""
    from . import decoder as D
    from . import filter as F
    if isinstance(selection, F.Selection):
        bitmap, n_rows = selection.bitmap, selection.n_rows
    else:
        bitmap = selection
        if n_rows is None:
            raise native.PqgError(abi.ERR_INVALID_ARG, what="take_records: a bitmap tensor needs n_rows")
        if bitmap.dtype != torch.int64 or bitmap.numel() < (n_rows + 63) // 64:
            raise native.PqgError(abi.ERR_INVALID_ARG,
                                  what="take_records: the bitmap is an int64 tensor of ceil(n_rows / 64) words")
    n_rows = int(n_rows)
    rows_capacity = n_rows if rows_capacity is None else min(int(rows_capacity), n_rows)
    for c in cols:
        if getattr(c, "max_rep", 0) > 0 and not is_missing(c) and (c.rep_levels is None or c.n_slots is None):
            raise native.PqgError(abi.ERR_INVALID_ARG, what="take_records: a repeated column carries rep_levels and n_slots")
    dev = decoder.device
    if out is None:
        out = [alloc_record_output(dev, c, n_rows, rows_capacity) for c in cols]
    n_calls = max(1, -(-len(cols) // abi.TAKE_MAX_COLUMNS))
    state = torch.empty(16 * n_calls + 32 * max(len(cols), 1), dtype=torch.uint8, device=dev)
    decoder.stream.wait_stream(torch.cuda.current_stream(dev))  # allocations / fills first
    new_cols, calls, off = [], [], 0
    for first in range(0, max(len(cols), 1), abi.TAKE_MAX_COLUMNS):
        part = cols[first:first + abi.TAKE_MAX_COLUMNS]
        arr = (abi.TakeRecordColumn * max(1, len(part)))()
        infos = []
        for i, c in enumerate(part):
            o = out[first + i]
            max_rep = int(getattr(c, "max_rep", 0))
            dflt = default_record_capacities(c, n_rows, rows_capacity)
            cap_s = dflt[0] if getattr(o, "slots_capacity", None) is None else int(o.slots_capacity)
            cap_v = dflt[1] if o.values_capacity is None else int(o.values_capacity)
            cap_b = dflt[2] if o.binary_capacity is None else int(o.binary_capacity)
            r, a = arr[i], arr[i].col
            a.physical_type, a.max_def = c.physical_type, c.max_def
            a.type_length, a.flags = getattr(c, "type_length", 0), getattr(c, "flags", 0)
            a.values = c.values.data_ptr() if c.values is not None else None
            a.binary_data = c.binary_data.data_ptr() if c.binary_data is not None else None
            a.def_levels = c.def_levels.data_ptr() if c.def_levels is not None else None
            a.n_values = c.n_values
            a.out_values = o.values.data_ptr() if o.values is not None else None
            a.out_binary_data = o.binary_data.data_ptr() if o.binary_data is not None else None
            a.out_def_levels = o.def_levels.data_ptr() if o.def_levels is not None else None
            a.out_values_capacity, a.out_binary_capacity = cap_v, cap_b
            r.max_rep = max_rep
            rl = getattr(c, "rep_levels", None)
            r.rep_levels = rl.data_ptr() if max_rep > 0 and rl is not None else None
            r.n_slots = slots_of(c, n_rows) if not is_missing(c) else n_rows
            orl = getattr(o, "rep_levels", None)
            r.out_rep_levels = orl.data_ptr() if max_rep > 0 and orl is not None else None
            r.out_slots_capacity = cap_s if max_rep > 0 else 0
            infos.append((max_rep, cap_s if max_rep > 0 else max(rows_capacity, n_rows), cap_v, cap_b, int(c.n_values)))
            if is_missing(c):
                m = F.MissingColumn(c.physical_type, c.max_def)
                m.max_rep = max_rep
                new_cols.append(m)
            else:
                nc = D.DeviceColumn(c.physical_type, o.values, o.def_levels, orl if max_rep > 0 else None,
                                    getattr(c, "type_length", 0), o.binary_data)
                nc.max_def, nc.flags, nc.max_rep = c.max_def, getattr(c, "flags", 0), max_rep
                new_cols.append(nc)
        rc = native.lib().pqg_take_records(decoder.ctx, bitmap.data_ptr(), n_rows, C.addressof(arr), len(part),
                                           rows_capacity, state.data_ptr() + off + 16, state.data_ptr() + off)
        native.check(rc, what="pqg_take_records")
        calls.append((first, len(part), off, infos))
        off += 16 + 32 * len(part)
    taken = TakenRecords(decoder, new_cols, state, calls, n_rows, rows_capacity)
    taken._keep = (selection, cols, out)
    return taken
