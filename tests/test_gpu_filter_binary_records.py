"""contains(leaf) on list<FLBA(5) DECIMAL> and list<INT96> columns (pqg_filter_run_records with a
pqg_filter_create_typed filter) against tests/filter_binary_ref.py, bit for bit, on values and on dictionary
ids: records of 0 .. 8 elements with null elements, empty lists and null lists, one record across the tile
boundary of 4,096 slots, one and two contains leaves on a column (k_filter_contains<1> and <2>), and the
Selection fed to take_records, which must keep the reference's records."""
import numpy as np
import pytest
import torch

import filter_binary_ref as B
import filter_records_ref as RR
import test_gpu_filter_binary as G
from pqgpu import abi
from pqgpu import decoder as D
from pqgpu import filter as F

pytestmark = pytest.mark.gpu

FLBA, I96 = G.FLBA, G.I96
N_REC = 1700
MAX_DEF = 3  # optional list of optional elements: 0 null list, 1 empty list, 2 null element, 3 a value


def draw_lists(rng, width, n_rec):
    """Per record: None (null list), [] or 1 .. 8 elements, some None. A third of the lists hold a small value
    or none at all, so contains() is neither always nor never true."""
    pool = G.draw_fixed(rng, width, 4096)
    lists = []
    for r in range(n_rec):
        k = rng.random()
        if k < 0.06:
            lists.append(None)
            continue
        if k < 0.12:
            lists.append([])
            continue
        n = int(rng.integers(1, 9))
        quiet = rng.random() < 0.4  # only large positive values: no leaf below a small pivot matches
        lst = []
        for _ in range(n):
            if rng.random() < 0.12:
                lst.append(None)
            elif quiet:
                lst.append(F.decimal_bytes(1000 + int(rng.integers(0, 1 << 20)), width) if width > 2 else F.decimal_bytes(100, width))
            else:
                lst.append(pool[int(rng.integers(0, len(pool)))])
        lists.append(lst)
    return lists


def stripe(lists):
    """(values, def levels, rep levels) of the lists, as filter_records_ref.from_lists lays them out."""
    vals, dl, rl = [], [], []
    for lst in lists:
        if lst is None or len(lst) == 0:
            dl.append(0 if lst is None else 1)
            rl.append(0)
            continue
        for j, v in enumerate(lst):
            rl.append(0 if j == 0 else 1)
            dl.append(MAX_DEF - 1 if v is None else MAX_DEF)
            if v is not None:
                vals.append(v)
    return vals, np.array(dl, dtype=np.uint8), np.array(rl, dtype=np.uint8)


def list_column(dec, t, width, vals, dl, rl, dictionary=None, ids=None):
    """The repeated DeviceColumn of a stripe: values, or uint32 ids with their dictionary."""
    if dictionary is None:
        col = G.fixed_column(dec, t, width, vals, offset=1 if t == FLBA else 0)
    else:
        raw = np.concatenate([np.asarray(ids, dtype=np.uint32), np.full(4, 0xA5A5A5A5, dtype=np.uint32)]).view(np.uint8)
        col = D.DeviceColumn(t, torch.from_numpy(raw.copy()).to(dec.device), type_length=width if t == FLBA else 0)
        col.flags, col.dictionary, col.n_values = abi.COLUMN_DICTIONARY_IDS, dictionary, len(ids)
    col.def_levels = torch.from_numpy(dl).to(dec.device)
    col.rep_levels = torch.from_numpy(rl).to(dec.device)
    col.max_def, col.max_rep, col.n_slots = MAX_DEF, 1, len(dl)
    return col


def check(dec, pred, dev, ref, n_rec):
    want = B.evaluate_records(pred, ref, n_rec)
    print(f"{pred!r}: {int(want.sum())} of {n_rec}")
    assert 0.05 <= want.mean() <= 0.95, (repr(pred), want.mean())
    words, ids, sel = G.run(dec, pred, dev, n_rec, filter_fn=dec.filter_records)
    G.compare(words, ids, sel, want, repr(pred))
    return want, sel


def predicates(c):
    lit = G.signed_literal
    one = [F.contains(op(c, lit(n))) for op in (F.eq, F.lt, F.lt_eq) for n in (0, 4, 5, 6, 40)]
    one += [F.contains(F.gt(c, F.decimal_bytes(40))), F.contains(F.gt_eq(c, F.decimal_bytes(40, 13))),
            F.contains(F.in_(c, [lit(5), lit(7), b"\x00" * 3])),
            F.contains(F.in_(c, [F.decimal_bytes(v) for v in (3, -1, 7, -20, 11, 19, -33, 2)] + [b"", b"\x00\x00", lit(40), b"\xff" * 9]))]
    two = [F.and_(F.contains(F.lt(c, lit(5))), F.contains(F.gt(c, F.decimal_bytes(20)))),  # K = 2
           F.or_(F.contains(F.eq(c, b"")), F.contains(F.not_in(c, [lit(40), F.decimal_bytes(100), F.decimal_bytes(100, 2)])))]
    return one + two


@pytest.mark.parametrize("form", ["values", "ids"])
@pytest.mark.parametrize("t,width", [(FLBA, 5), (I96, 12)], ids=lambda x: str(x))
def test_contains(decoder, t, width, form):
    rng = np.random.default_rng(width)
    lists = draw_lists(rng, width, N_REC)
    vals, dl, rl = stripe(lists)
    starts = np.flatnonzero(rl == 0)
    assert len(dl) > G.T and not (starts == G.T).any()  # a record lies across the tile boundary
    assert {len(x) for x in lists if x is not None} >= set(range(9))
    ref = [RR.RefListColumn(t, vals, dl, rl, max_def=MAX_DEF, max_rep=1)]
    if form == "values":
        dev = [list_column(decoder, t, width, vals, dl, rl)]
    else:
        entries = list(dict.fromkeys(vals))
        where = {e: i for i, e in enumerate(entries)}
        dev = [list_column(decoder, t, width, vals, dl, rl, G.fixed_column(decoder, t, width, entries),
                           [where[v] for v in vals])]
    kept = None
    for pred in predicates(F.col(0, order="signed_integer")):
        kept = check(decoder, pred, dev, ref, N_REC)
    if form == "ids":
        return
    # the Selection goes into take_records: the reference's records, whole
    want, sel = kept
    taken = decoder.take_records(sel, dev)
    assert taken.n_rows == int(want.sum())
    w_vals, w_dl, w_rl = stripe([lst for lst, k in zip(lists, want) if k])
    out = taken.columns[0]
    assert out.n_slots == len(w_dl) and out.n_values == len(w_vals)
    assert np.array_equal(out.rep_levels.cpu().numpy()[:len(w_rl)], w_rl)
    assert np.array_equal(out.def_levels.cpu().numpy()[:len(w_dl)], w_dl)
    assert out.values[:len(w_vals) * width].cpu().numpy().tobytes() == b"".join(w_vals)


def test_contains_beside_a_flat_leaf(decoder):
    """A flat int64 leaf and a contains on a DECIMAL list in one predicate (the flat leaf on the left, as
    ContainsRewriter admits it)."""
    rng = np.random.default_rng(9)
    lists = draw_lists(rng, 5, N_REC)
    vals, dl, rl = stripe(lists)
    ints = rng.integers(-20, 20, size=N_REC).astype(np.int64)
    flat = G.fixed_column(decoder, abi.INT64, 8, [v.tobytes() for v in ints])
    flat.n_slots = N_REC
    dev = [list_column(decoder, FLBA, 5, vals, dl, rl), flat]
    ref = [RR.RefListColumn(FLBA, vals, dl, rl, max_def=MAX_DEF, max_rep=1), G.ref_column(abi.INT64, ints)]
    c = F.col(0, order="signed_integer")
    check(decoder, F.and_(F.gt(F.col(1), -5), F.contains(F.lt(c, b"\x03"))), dev, ref, N_REC)
    check(decoder, F.or_(F.lt(F.col(1), -15), F.contains(F.eq(c, b""))), dev, ref, N_REC)
