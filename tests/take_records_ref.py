"""Reference semantics of a record selection over decoded stripes, repeated leaves included, restated in
Python / numpy. Test infrastructure only (the product is csrc/pqgpu_take*.{cpp,hip}, pqg_take_records).

What is restated: RecordReaderImplementation.read drops a whole record when shouldSkipCurrentRecord says
so (RecordReaderImplementation.java:440-449, FilteringRecordMaterializer), and SynchronizingColumnReader
skips the rows outside the RowRanges. Both act on records, so every leaf loses the same records.

A stripe is (rep_levels, def_levels, dense values, max_def): one repetition and one definition byte per
slot, a dense value for every slot with def == max_def (tests/records.shred). Record i is the run of
slots from the i-th slot with rep == 0 up to the next such slot. take() returns, per stripe,
(rep_levels_out, def_levels_out, dense values_out):
  take_slots   slot by slot from the definition
  take         the same with rec = cumsum(rep == 0) - 1, for large inputs; the CPU tests hold them equal
A slot before the first record start (record -1) or of a record past the mask is not kept."""
import numpy as np


def _dense(values):
    if isinstance(values, np.ndarray):
        return values
    a = np.empty(len(values), dtype=object)
    for i, x in enumerate(values):
        a[i] = x
    return a


def take_slots(stripes, keep):
    """Slot by slot: walk the slots, count the record starts and the values passed, keep what the mask keeps."""
    keep = np.asarray(keep, dtype=bool)
    out = []
    for rl, dl, vals, max_def in stripes:
        orl, odl, ovals = [], [], []
        rec, k = -1, 0  # the current record, the dense index of the next slot with a value
        for s in range(len(rl)):
            if rl[s] == 0:
                rec += 1
            has = dl[s] == max_def
            if 0 <= rec < keep.size and keep[rec]:
                orl.append(int(rl[s]))
                odl.append(int(dl[s]))
                if has:
                    ovals.append(vals[k])
            k += has
        out.append((np.array(orl, dtype=np.uint8), np.array(odl, dtype=np.uint8), ovals))
    return out


def slot_mask(rl, keep):
    """The slots a record mask keeps."""
    keep = np.asarray(keep, dtype=bool)
    rec = np.cumsum(np.asarray(rl) == 0) - 1
    ok = (rec >= 0) & (rec < keep.size)
    m = np.zeros(len(rl), dtype=bool)
    m[ok] = keep[rec[ok]]
    return m


def take(stripes, keep):
    """Vectorised: the slot's record is the number of record starts up to it, minus one."""
    out = []
    for rl, dl, vals, max_def in stripes:
        rl, dl = np.asarray(rl, dtype=np.uint8), np.asarray(dl, dtype=np.uint8)
        m = slot_mask(rl, keep)
        valid = dl == max_def
        src = np.cumsum(valid) - valid
        out.append((rl[m], dl[m], _dense(vals)[src[m & valid]]))
    return out


def n_records(rl):
    return int((np.asarray(rl) == 0).sum())
