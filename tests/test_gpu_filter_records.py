"""pqg_filter_run_records on the GPU against tests/filter_records_ref.py, bit for bit: the record bitmap (and
the words behind it, which must stay untouched), n_selected and the row ids. Most columns are stripes built
by hand on the host (one repetition and one definition byte per slot, dense values), so that every record
boundary the kernels treat differently sits where the test wants it; one case decodes a synthesized chunk
and runs decode -> filter_records -> take_records -> assemble."""
import copy
import ctypes as C
import json

import numpy as np
import pytest
import torch

import filter_records_ref as RR
import filter_ref as R
import take_records_ref as KR
from oracle import assembly as A
from pqgpu import abi, native
from pqgpu import decoder as D
from pqgpu import filter as F
from test_filter_records_ref import phonebook, phonebook_predicate
from tools.synth import writer

pytestmark = pytest.mark.gpu

T = abi.FILTER_TILE_ROWS
POISON = 0xA5
POISON64 = np.array([0xA5A5A5A5A5A5A5A5], dtype=np.uint64).view(np.int64)[0]


# ---- host stripes -> device columns --------------------------------------------------------------------------

def to_dev(dec, a, pad=16):
    """A device uint8 tensor of the array's bytes, followed by `pad` poison bytes (never empty)."""
    raw = np.frombuffer(np.ascontiguousarray(a).tobytes() + bytes([POISON]) * pad, dtype=np.uint8).copy()
    return torch.from_numpy(raw).to(dec.device)


def value_buffers(dec, t, vals):
    """(values, binary_data) tensors of dense values in the decoder's layout."""
    if t == abi.BYTE_ARRAY:
        offs = np.concatenate([[0], np.cumsum([len(v) for v in vals])]).astype(np.int64)
        return to_dev(dec, offs, 0), to_dev(dec, np.frombuffer(b"".join(bytes(v) for v in vals), dtype=np.uint8))
    dt = np.uint8 if t == abi.BOOLEAN else abi.numpy_dtype(t)
    return to_dev(dec, np.asarray(vals, dtype=dt)), None


def dev_col(dec, ref, dictionary=None):
    """The device column of a RefListColumn / RefColumn. dictionary = (entries, ids): the column holds the
    uint32 ids and carries the decoded dictionary, ref.values being entries[ids]."""
    t = ref.physical_type
    rep = isinstance(ref, RR.RefListColumn)
    if ref.missing:
        m = F.MissingColumn(t, max(ref.max_def, 1))
        m.max_rep = ref.max_rep if rep else 0
        return m
    if dictionary is not None:
        entries, ids = dictionary
        values, binary = to_dev(dec, np.asarray(ids, dtype=np.uint32)), None
        n_values = len(ids)
    else:
        values, binary = value_buffers(dec, t, ref.values)
        n_values = len(ref.values)
    dl = to_dev(dec, ref.def_levels) if ref.max_def > 0 else None
    col = D.DeviceColumn(t, values, dl, to_dev(dec, ref.rep_levels) if rep else None, binary_data=binary)
    col.n_values, col.max_def = n_values, ref.max_def
    if rep:
        col.max_rep, col.n_slots = ref.max_rep, len(ref.rep_levels)
    if dictionary is not None:
        col.flags = abi.COLUMN_DICTIONARY_IDS
        dv, db = value_buffers(dec, t, entries)
        col.dictionary = D.DeviceColumn(t, dv, binary_data=db)
        col.dictionary.n_values = len(entries)
    return col


def run(dec, pred, dev, n_rows, capacity=None):
    """filter_records into poisoned outputs -> (words incl. two guard words, ids or None, (n, err, err_col))."""
    n_words = (n_rows + 63) // 64
    cap = n_rows if capacity is None else capacity
    words = torch.full((n_words + 2,), POISON64, dtype=torch.int64, device=dec.device)
    ids = torch.full((cap + 2,), POISON64, dtype=torch.int64, device=dec.device)
    result = torch.full((16,), POISON, dtype=torch.uint8, device=dec.device)
    sel = dec.filter_records(pred, dev, n_rows, capacity=cap, out=(words, ids, result))
    dec.stream.synchronize()
    r = result.cpu().numpy()
    return sel, words.cpu().numpy().view(np.uint64), ids.cpu().numpy(), (int(r[:8].view(np.uint64)[0]),) + tuple(
        int(x) for x in r[8:16].view(np.int32))


def check(dec, pred, refs, dev, n_rows, want=None):
    want = RR.evaluate(pred, refs, n_rows) if want is None else want
    sel, words, ids, (n, err, err_col) = run(dec, pred, dev, n_rows)
    n_words = (n_rows + 63) // 64
    assert (err, err_col) == (abi.OK, -1), (err, err_col, repr(pred))
    got = np.unpackbits(words[:n_words].view(np.uint8), bitorder="little")[:n_rows].astype(bool)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (repr(pred), bad[:10], n_rows)
    assert np.array_equal(words[:n_words], R.bitmap_words(want)), repr(pred)  # the bits past n_rows are 0
    assert (words[n_words:] == np.uint64(POISON64)).all()
    assert n == int(want.sum())
    assert np.array_equal(ids[:n], np.flatnonzero(want)) and (ids[n:] == POISON64).all()
    assert sel.count == n
    return want


def list_col(t, lens, vals, max_def=2, dl=None):
    """A RefListColumn of records of `lens` slots (0: an empty list, one slot at def 1); every slot of a
    longer record holds a value unless `dl` says otherwise."""
    lens = np.asarray(lens)
    slots = np.maximum(lens, 1)
    n = int(slots.sum())
    rl = np.ones(n, dtype=np.uint8)
    starts = np.cumsum(slots) - slots
    rl[starts] = 0
    if dl is None:
        dl = np.full(n, max_def, dtype=np.uint8)
        dl[starts[lens == 0]] = 1
    assert int((dl == max_def).sum()) == len(vals)
    return RR.RefListColumn(t, vals, dl, rl, max_def=max_def, max_rep=1)


def fill(rng, n_slots, lo=1, hi=6):
    """Record lengths lo..hi-1 filling exactly n_slots slots."""
    lens, left = [], n_slots
    while left:
        k = min(int(rng.integers(lo, hi)), left)
        lens.append(k)
        left -= k
    return lens


EQ7 = F.contains(F.eq(F.col(0), 7))


def int_vals(rng, lens, p=0.1):
    """One int64 per slot of the non-empty records: 7 with probability p, else 0..6."""
    k = int(np.asarray(lens).sum())
    return np.where(rng.random(k) < p, 7, rng.integers(0, 7, size=k)).astype(np.int64)


# ---- record boundaries ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("hit_tile", [0, 1, 2])
def test_record_boundaries(decoder, hit_tile):
    """A record ending exactly at a step boundary (slot 64) and one straddling the next (slot 128); one
    straddling the tile boundary (slot 4,096); one record of 2T + 100 slots whose only hit lies in its first,
    a middle or its last tile (the middle tile has no record start); small records after it."""
    rng = np.random.default_rng(5)
    head = [60, 4, 60, 8] + fill(rng, T - 132 - 7) + [12]   # the 12 straddles slot T: 7 before, 5 after
    big_at = sum(head)
    lens = head + [2 * T + 100] + fill(rng, 300)
    vals = int_vals(rng, lens)
    vals[big_at:big_at + 2 * T + 100] = 3
    at = big_at + (10, T + 17, 2 * T + 99)[hit_tile]
    assert at // T == 1 + hit_tile
    vals[at] = 7
    ref = [list_col(abi.INT64, lens, vals)]
    dev = [dev_col(decoder, ref[0])]
    want = check(decoder, EQ7, ref, dev, len(lens))
    assert want[len(head)]
    vals[at] = 3  # and without the hit the long record is false
    ref = [list_col(abi.INT64, lens, vals)]
    assert not check(decoder, EQ7, ref, [dev_col(decoder, ref[0])], len(lens))[len(head)]


def test_steps_of_64_starts_and_a_carried_record(decoder):
    """Step 0: 63 one-slot records and the first slot of a two-slot record; step 1: that record carried over
    plus 63 starts; step 2: 64 starts. Every hit pattern bit by bit: all, none, alternating, random."""
    lens = [1] * 63 + [2] + [1] * 63 + [1] * 64 + [3, 1]
    rng = np.random.default_rng(6)
    k = sum(lens)
    for vals in (np.full(k, 7), np.zeros(k), np.arange(k) % 2 * 7, np.where(rng.random(k) < 0.5, 7, 1)):
        vals = vals.astype(np.int64)
        for carried in (0, 7):
            vals[64] = carried  # the carried record's only slot in step 1
            vals[63] = 0
            ref = [list_col(abi.INT64, lens, vals)]
            want = check(decoder, EQ7, ref, [dev_col(decoder, ref[0])], len(lens))
            assert want[63] == (carried == 7)


@pytest.mark.parametrize("first", [1, 63, 64])
def test_a_tile_of_one_slot_records_touches_65_words(decoder, first):
    """Tile 1 holds T one-slot records, the first of them record `first`: records first .. first + T - 1
    lie in 65 bitmap words (with the carried record for first = 64)."""
    head = [1] * (first - 1) + [T - (first - 1)]
    assert len(head) == first and sum(head) == T
    lens = head + [1] * T + [2, 1, 5]
    rng = np.random.default_rng(first)
    for p in (0.5, 1.0, 0.02):
        vals = int_vals(rng, lens, p)
        ref = [list_col(abi.INT64, lens, vals)]
        want = check(decoder, EQ7, ref, [dev_col(decoder, ref[0])], len(lens))
        if p == 1.0:
            assert want.all()


@pytest.mark.parametrize("n_rows", [0, 1, 63, 64, 65, 4097])
def test_row_counts(decoder, n_rows):
    rng = np.random.default_rng(100 + n_rows)
    lens = rng.integers(0, 4, size=n_rows)
    ref = [list_col(abi.INT64, lens, int_vals(rng, lens, 0.3))]
    check(decoder, EQ7, ref, [dev_col(decoder, ref[0])], n_rows)
    check(decoder, F.contains(F.not_eq(F.col(0), 7)), ref, [dev_col(decoder, ref[0])], n_rows)


def test_nulls_inside_and_around_lists(decoder):
    """Null lists, empty lists, null elements; a record whose only matching position is a null element; notEq
    and notIn on records without a value are false."""
    lists = [None, [], [None], [None, None], [7], [None, 7], [7, None], [1, None, 2], [1], [None, 1], None, []] * 30
    ref = [RR.from_lists(abi.INT64, lists, max_def=3)]
    dev = [dev_col(decoder, ref[0])]
    n = len(lists)
    for leaf, twelve in ((F.eq(F.col(0), 7), [0, 0, 0, 0, 1, 1, 1, 0, 0, 0, 0, 0]),
                         (F.not_eq(F.col(0), 7), [0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 0, 0]),
                         (F.not_in(F.col(0), [7, 1]), [0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0]),
                         (F.not_in(F.col(0), [9]), [0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 0, 0]),
                         (F.lt(F.col(0), 100), [0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 0, 0])):
        pred = F.contains(leaf)
        want = check(decoder, pred, ref, dev, n)
        assert want[:12].astype(int).tolist() == twelve, repr(pred)
        assert np.array_equal(want, RR.evaluate_records(pred, ref, n))


# ---- every op on every type ----------------------------------------------------------------------------------

def pool(t):
    """30 distinct values of type t around its edge cases."""
    if t == abi.BOOLEAN:
        return [False, True]
    if t in (abi.INT32, abi.INT64):
        b = 31 if t == abi.INT32 else 63
        return [0, 1, -1, 2**b - 1, -2**b, 7, 17] + list(range(100, 123))
    if t in (abi.FLOAT, abi.DOUBLE):
        return R.EDGE[t] + [(np.float32 if t == abi.FLOAT else np.float64)(x / 4) for x in range(8, 29)]
    return R.EDGE[t] + [b"ab" + bytes([x]) for x in range(20)]


@pytest.fixture(scope="module")
def typed(decoder):
    """Per type: a list column of ~300 records (T + 300 for INT32, so more than one tile) over pool(t), with
    null lists, empty lists and null elements, on the host and on the device."""
    out = {}
    for t in (abi.BOOLEAN, abi.INT32, abi.INT64, abi.FLOAT, abi.DOUBLE, abi.BYTE_ARRAY):
        rng = np.random.default_rng(200 + t)
        p = pool(t)
        n = T + 300 if t == abi.INT32 else 300
        lists = []
        for _ in range(n):
            r = rng.random()
            lists.append(None if r < 0.08 else [] if r < 0.16 else
                         [None if rng.random() < 0.15 else p[int(rng.integers(0, len(p)))] for _ in range(int(rng.integers(1, 7)))])
        ref = RR.from_lists(t, lists, max_def=3)
        out[t] = (ref, dev_col(decoder, ref), n)
    return out


@pytest.mark.parametrize("t", [abi.BOOLEAN, abi.INT32, abi.INT64, abi.FLOAT, abi.DOUBLE, abi.BYTE_ARRAY])
def test_every_op(decoder, typed, t):
    ref, dev, n = typed[t]
    rng = np.random.default_rng(300 + t)
    p = pool(t)
    cols = [F.col(0)] + ([F.col(0, unsigned=True)] if t in (abi.INT32, abi.INT64) else [])
    ops = [F.eq, F.not_eq] + ([] if t == abi.BOOLEAN else [F.lt, F.lt_eq, F.gt, F.gt_eq])
    n_checked = 0
    for c in cols:
        for lit in (R.EDGE[t] if t != abi.BOOLEAN else p):
            for mk in ops:
                check(decoder, F.contains(mk(c, lit)), [ref], [dev], n)
                n_checked += 1
        for size in ((1, 2) if t == abi.BOOLEAN else (3, 20)):
            members = [p[i] for i in rng.permutation(len(p))[:size]]
            for mk in (F.in_, F.not_in):
                check(decoder, F.contains(mk(c, members)), [ref], [dev], n)
    assert n_checked >= 4


# ---- composition ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def mixed(decoder):
    """Columns 0, 1: list<int64> and list<binary> of different slot counts; 2: a flat nullable int32; 3: a flat
    required int64; 4: a missing repeated column; 5: a missing flat column. T + 700 records."""
    rng = np.random.default_rng(7)
    n = T + 700
    la, lb = rng.integers(0, 6, size=n), rng.integers(0, 4, size=n)
    words = [b"", b"a", b"ab", b"abc", b"b", b"ab\x80"]
    a = list_col(abi.INT64, la, rng.integers(0, 10, size=int(la.sum())).astype(np.int64))
    b = list_col(abi.BYTE_ARRAY, lb, [words[int(i)] for i in rng.integers(0, len(words), size=int(lb.sum()))])
    valid = rng.random(n) < 0.8
    c = R.RefColumn(abi.INT32, rng.integers(0, 5, size=int(valid.sum())).astype(np.int32), valid.astype(np.uint8), max_def=1)
    d = R.RefColumn(abi.INT64, rng.integers(0, 4, size=n).astype(np.int64), None, 0)
    refs = [a, b, c, d, RR.RefListColumn(abi.INT64, missing=True, max_def=2), R.RefColumn(abi.INT32, max_def=1, missing=True)]
    return refs, [dev_col(decoder, r) for r in refs], n


def test_composition(decoder, mixed):
    refs, dev, n = mixed
    A_, B_ = (lambda v: F.contains(F.eq(F.col(0), v))), (lambda v: F.contains(F.eq(F.col(1), v)))
    flat = F.eq(F.col(2), 3)
    preds = [
        F.and_(A_(1), A_(2)), F.or_(A_(1), A_(2)), F.and_(A_(1), F.and_(A_(2), A_(3))), F.or_(A_(1), F.or_(A_(2), A_(3))),
        F.and_(A_(1), F.or_(F.contains(F.gt(F.col(0), 7)), F.contains(F.not_in(F.col(0), [1, 2, 3])))),
        F.or_(flat, A_(4)), F.and_(F.and_(flat, A_(4)), B_(b"ab")), F.and_(F.and_(F.eq(F.col(3), 1), A_(4)), B_(b"")),
        F.or_(F.not_(F.lt(F.col(2), 2)), F.contains(F.lt(F.col(1), b"ab"))),
        F.or_(F.eq(F.col(2), None), A_(5)),
        # a missing repeated column is false in every record, a missing flat column null in every row
        F.contains(F.not_eq(F.col(4), 1)), F.or_(flat, F.contains(F.gt_eq(F.col(4), 0))),
        F.and_(F.and_(F.not_eq(F.col(5), 1), A_(1)), F.contains(F.eq(F.col(4), 1))),
        F.or_(F.eq(F.col(5), None), B_(b"abc")),
    ]
    # five and nine contains on one column: more than one group of leaves per value load, a group of one
    for k in (5, 9):
        chain = A_(0)
        for v in range(1, k):
            chain = (F.or_ if k == 5 else F.and_)(chain, F.contains((F.gt if v % 2 else F.not_eq)(F.col(0), v)))
        preds.append(chain)
    for p in preds:
        assert RR.outcome(p) == (RR.OK, -1), repr(p)
        want = check(decoder, p, refs, dev, n)
        assert np.array_equal(want[:200], RR.evaluate_records(p, refs, n)[:200])
    assert not check(decoder, preds[10], refs, dev, n).any()


# ---- dictionary-id list columns ------------------------------------------------------------------------------

def dict_column(dec, t, n_entries, lens, rng):
    p = pool(t)
    entries = [p[i % len(p)] for i in range(n_entries)] if t == abi.BYTE_ARRAY else \
        np.arange(-3, n_entries - 3).astype(abi.numpy_dtype(t))
    k = int(np.asarray(lens).sum())
    ids = rng.integers(0, n_entries, size=k).astype(np.uint32)
    vals = [entries[int(i)] for i in ids] if t == abi.BYTE_ARRAY else entries[ids]
    ref = list_col(t, lens, vals)
    return ref, dev_col(dec, ref, (entries, ids)), ids


@pytest.mark.parametrize("n_entries", [1, 64, 65, 3000])
def test_dictionary_id_lists(decoder, n_entries):
    rng = np.random.default_rng(n_entries)
    n = T + 100
    lens = rng.integers(0, 5, size=n)
    for t in (abi.INT64, abi.BYTE_ARRAY):
        ref, dev, _ = dict_column(decoder, t, n_entries, lens, rng)
        vdev = dev_col(decoder, ref)  # the same column holding values
        lits = [b"ab", b"", b"ab\x05"] if t == abi.BYTE_ARRAY else [-3, n_entries // 2, n_entries - 4]
        for lit in lits:
            for mk in (F.eq, F.not_eq, F.lt, F.gt_eq):
                pred = F.contains(mk(F.col(0), lit))
                want = check(decoder, pred, [ref], [dev], n)
                check(decoder, pred, [ref], [vdev], n, want=want)
        check(decoder, F.and_(F.contains(F.in_(F.col(0), lits)), F.contains(F.not_in(F.col(0), lits[:1]))), [ref], [dev], n)


def test_dictionary_tables_in_global_memory(decoder):
    """20 contains leaves over a 3,300-entry dictionary: 20 * 52 table words pass PQG_FILTER_DICT_LDS_BYTES."""
    rng = np.random.default_rng(9)
    n, n_entries = 900, 3300
    assert 20 * ((n_entries + 63) // 64) * 8 > abi.FILTER_DICT_LDS_BYTES
    lens = rng.integers(0, 5, size=n)
    ref, dev, _ = dict_column(decoder, abi.INT64, n_entries, lens, rng)
    pred = F.contains(F.lt(F.col(0), 100))
    for i in range(1, 20):
        pred = F.or_(pred, F.contains(F.eq(F.col(0), 150 * i)))
    assert check(decoder, pred, [ref], [dev], n).any()


def test_an_id_outside_the_dictionary(decoder, mixed):
    refs, dev, n = mixed
    rng = np.random.default_rng(10)
    la = rng.integers(0, 4, size=n)
    ref, col, ids = dict_column(decoder, abi.INT64, 65, la, rng)
    ids = ids.copy()
    ids[len(ids) // 2] = 65
    bad = copy.copy(col)
    bad.values = to_dev(decoder, ids)
    cols = [dev[3], bad]  # the flat required column, then the list of ids
    pred = F.and_(F.and_(F.gt_eq(F.col(0), 0), F.contains(F.gt(F.col(1), 0))), F.contains(F.eq(F.col(1), 5)))
    _, _, _, (_, err, err_col) = run(decoder, pred, cols, n)
    assert (err, err_col) == (abi.ERR_DICT_ID, 1)
    _, _, _, (_, err, err_col) = run(decoder, pred, [dev[3], col], n)
    assert (err, err_col) == (abi.OK, -1)
    # the value count check takes precedence
    bad.n_values -= 1
    _, _, _, (_, err, err_col) = run(decoder, pred, cols, n)
    assert (err, err_col) == (abi.ERR_INVALID_ARG, 1)


# ---- device verdicts -----------------------------------------------------------------------------------------

PRED_01 = F.and_(F.and_(F.gt_eq(F.col(3), 0), F.contains(F.gt(F.col(1), b""))), F.contains(F.gt(F.col(0), 3)))


def broken(mixed, c, **kw):
    refs, dev, n = mixed
    dev = list(dev)
    dev[c] = copy.copy(dev[c])
    for k, v in kw.items():
        setattr(dev[c], k, v)
    return dev, n


def test_slot_0_inside_a_record(decoder, mixed):
    rl = mixed[1][0].rep_levels.clone()
    rl[0] = 1
    dev, n = broken(mixed, 0, rep_levels=rl)
    assert run(decoder, PRED_01, dev, n)[3][1:] == (abi.ERR_INVALID_ARG, 0)
    assert run(decoder, PRED_01, mixed[1], n)[3][1:] == (abi.OK, -1)


@pytest.mark.parametrize("delta", [-1, 1])
def test_record_starts_differ_from_n_rows(decoder, mixed, delta):
    """One start too many: the last slots belong to record n_rows, one past the bitmap, and contribute nothing
    (the guard words behind the bitmap stay as they were)."""
    host = mixed[0][1].rep_levels
    at = int(np.flatnonzero(host == 0)[5]) if delta < 0 else int(np.flatnonzero(host != 0)[5])
    rl = mixed[1][1].rep_levels.clone()
    rl[at] = 1 if delta < 0 else 0
    dev, n = broken(mixed, 1, rep_levels=rl)
    _, words, _, (_, err, err_col) = run(decoder, PRED_01, dev, n)
    assert (err, err_col) == (abi.ERR_INVALID_ARG, 1)
    assert (words[(n + 63) // 64:] == np.uint64(POISON64)).all()
    # both columns bad: the lowest is named
    rl0 = mixed[1][0].rep_levels.clone()
    rl0[int(np.flatnonzero(mixed[0][0].rep_levels != 0)[3])] = 0
    dev[0] = copy.copy(dev[0])
    dev[0].rep_levels = rl0
    assert run(decoder, PRED_01, dev, n)[3][1:] == (abi.ERR_INVALID_ARG, 0)


@pytest.mark.parametrize("delta", [-1, 1])
def test_value_count_differs_from_n_values(decoder, mixed, delta):
    dev, n = broken(mixed, 1, n_values=mixed[1][1].n_values + delta)
    assert run(decoder, PRED_01, dev, n)[3][1:] == (abi.ERR_INVALID_ARG, 1)
    dev, n = broken(mixed, 0, n_values=mixed[1][0].n_values + delta)
    assert run(decoder, PRED_01, dev, n)[3][1:] == (abi.ERR_INVALID_ARG, 0)


# ---- refusals before any launch ------------------------------------------------------------------------------

def test_host_refusals(decoder):
    L = native.lib()
    buf = torch.zeros(8192, dtype=torch.uint8, device=decoder.device)
    p = buf.data_ptr()
    types = [abi.INT64, abi.INT64]
    contains = F.Filter(F.contains(F.eq(F.col(0), 1)), types)
    plain = F.Filter(F.eq(F.col(0), 1), types)
    both = F.Filter(F.or_(F.eq(F.col(1), 1), F.contains(F.eq(F.col(0), 1))), types)

    def column(rep, **kw):
        c = abi.FilterRecordColumn()
        c.col = abi.FilterColumn(physical_type=abi.INT64, max_def=2 if rep else 1, values=p, def_levels=p + 1024, n_values=10)
        c.max_rep, c.n_slots = rep, 20 if rep else 10
        c.rep_levels = p + 2048 if rep else None
        for k, v in kw.items():
            setattr(c.col if hasattr(c.col, k) else c, k, v)
        return c

    def rc(flt, c0, c1=None, n_rows=10, bitmap=p + 4096, result=p + 6144, ctx=decoder.ctx, dicts=None):
        arr = (abi.FilterRecordColumn * 2)(c0, column(0) if c1 is None else c1)
        return L.pqg_filter_run_records(ctx, flt.handle, C.addressof(arr), dicts, 2, n_rows, bitmap, None, 0, result)

    bad = abi.ERR_INVALID_ARG
    assert rc(contains, column(1)) == abi.OK
    assert rc(plain, column(0)) == abi.OK
    assert rc(both, column(1), column(0)) == abi.OK
    assert rc(contains, column(0)) == bad            # contains on a present flat column
    assert rc(plain, column(1)) == bad               # any other leaf on a repeated column
    assert rc(both, column(1), column(1)) == bad
    for flt, rep in ((contains, 1), (plain, 0)):
        assert rc(flt, column(rep), ctx=None) == bad
        assert rc(flt, column(rep), result=None) == bad
        assert rc(flt, column(rep), bitmap=None) == bad
        assert rc(flt, column(rep, max_def=255)) == bad
        assert rc(flt, column(rep, physical_type=abi.INT32)) == bad
        assert rc(flt, column(rep, values=None)) == bad
        assert rc(flt, column(rep, reserved=1)) == bad
        assert rc(flt, column(rep, max_rep=255)) == bad
        assert rc(flt, column(rep, max_rep=-1)) == bad
        assert rc(flt, column(rep, n_slots=9)) == bad  # fewer slots than records
    assert rc(contains, column(1, max_def=0)) == bad   # a repeated node adds a definition level
    assert rc(contains, column(1, rep_levels=None)) == bad
    assert rc(plain, column(0, rep_levels=p + 2048)) == bad
    assert rc(plain, column(0, n_slots=11)) == bad
    assert rc(plain, column(0, max_def=0, n_values=9)) == bad  # a required column has a value per row
    # a missing column is exempt from the structural rules and from the leaf rules
    assert rc(contains, column(1, def_levels=None, rep_levels=None, n_slots=0, reserved=7)) == abi.OK
    assert rc(contains, column(0, def_levels=None)) == abi.OK
    assert rc(plain, column(1, def_levels=None)) == abi.OK
    # a column the predicate does not name is not looked at
    assert rc(contains, column(1), column(0, max_rep=300, reserved=1)) == abi.OK
    # dictionaries: what pqg_filter_run_dict refuses
    dicts = (abi.FilterDictionary * 2)()
    dicts[0].values, dicts[0].n_entries = p + 3072, 4
    assert rc(contains, column(1), dicts=C.addressof(dicts)) == abi.OK
    dicts[0].reserved = 1
    assert rc(contains, column(1), dicts=C.addressof(dicts)) == bad
    dicts[0].reserved = 0
    assert rc(contains, column(1, values=p + 2), dicts=C.addressof(dicts)) == bad  # misaligned ids
    assert rc(contains, column(1, def_levels=None), dicts=C.addressof(dicts)) == bad  # a dictionary on a missing column
    # a filter with a contains node has no place in the calls without repetition levels
    flat = (abi.FilterColumn * 2)(column(0).col, column(0).col)
    assert L.pqg_filter_run(decoder.ctx, contains.handle, C.addressof(flat), 2, 10, p + 4096, None, 0, p + 6144) == bad
    assert L.pqg_filter_run_dict(decoder.ctx, contains.handle, C.addressof(flat), None, 2, 10, p + 4096, None, 0, p + 6144) == bad
    assert L.pqg_filter_run(decoder.ctx, plain.handle, C.addressof(flat), 2, 10, p + 4096, None, 0, p + 6144) == abi.OK
    decoder.stream.synchronize()
    # Decoder.filter keeps refusing repeated columns
    ref = list_col(abi.INT64, [1, 2], np.array([1, 2, 3], dtype=np.int64))
    with pytest.raises(native.PqgError) as e:
        decoder.filter(F.eq(F.col(0), 1), [dev_col(decoder, ref)], 2)
    assert e.value.code == abi.ERR_UNSUPPORTED
    for f in (contains, plain, both):
        f.close()


def test_flat_predicates_equal_decoder_filter(decoder, mixed):
    """Without a contains node, over flat columns (values and dictionary ids): byte for byte Decoder.filter."""
    refs, dev, n = mixed
    rng = np.random.default_rng(12)
    entries = np.arange(40, dtype=np.int64)
    ids = rng.integers(0, 40, size=n).astype(np.uint32)
    idc = dev_col(decoder, R.RefColumn(abi.INT64, entries[ids], None, 0), (entries, ids))
    cols = [dev[2], dev[3], dev[5], idc]
    for pred in (F.eq(F.col(0), 3), F.or_(F.not_(F.lt(F.col(0), 2)), F.eq(F.col(1), 1)), F.and_(F.eq(F.col(2), None), F.gt(F.col(1), 0)),
                 F.or_(F.in_(F.col(3), [1, 5, 39]), F.eq(F.col(0), None))):
        a = decoder.filter(pred, cols, n)
        b = decoder.filter_records(pred, cols, n)
        assert a.count == b.count
        assert torch.equal(a.bitmap, b.bitmap) and torch.equal(a.row_ids, b.row_ids)
        assert torch.equal(a._result, b._result)


# ---- decode -> filter_records -> take_records -> assemble ----------------------------------------------------

def test_end_to_end(decoder):
    """A synthesized chunk with a list<int64> leaf, a list<binary> leaf and a flat column: the decoder's own
    stripes are filtered with contains(), the selection goes into take_records with no sync in between, and
    the kept stripes equal the reference's take of the oracle's view; assemble on the taken levels gives the
    list offsets of the kept records."""
    rng = np.random.default_rng(13)
    n = T + 500
    la, lb = rng.integers(0, 6, size=n), rng.integers(0, 4, size=n)
    words = [b"", b"x", b"xy", b"xyz", b"y"]
    a = list_col(abi.INT64, la, rng.integers(0, 50, size=int(la.sum())).astype(np.int64))
    b = list_col(abi.BYTE_ARRAY, lb, [words[int(i)] for i in rng.integers(0, len(words), size=int(lb.sum()))])
    ids = np.arange(n, dtype=np.int64)
    chunks = [writer.write_column_chunk(abi.INT64, a.values, abi.PLAIN, def_levels=a.def_levels, rep_levels=a.rep_levels,
                                        max_def=2, max_rep=1, page_rows=3000),
              writer.write_column_chunk(abi.BYTE_ARRAY, b.values, abi.PLAIN, def_levels=b.def_levels, rep_levels=b.rep_levels,
                                        max_def=2, max_rep=1, page_rows=3000),
              writer.write_column_chunk(abi.INT64, ids, abi.PLAIN, page_rows=3000)]
    dev, _ = decoder.decode(decoder.upload(writer.build_batch(chunks)))
    assert [c.max_rep for c in dev] == [1, 1, 0] and dev[0].n_slots == len(a.rep_levels)
    refs = [a, b, R.RefColumn(abi.INT64, ids, None, 0)]
    pred = F.and_(F.and_(F.lt(F.col(2), n - 100), F.contains(F.lt(F.col(0), 5))), F.contains(F.gt_eq(F.col(1), b"xy")))
    keep = RR.evaluate(pred, refs, n)
    assert 50 < keep.sum() < n - 50
    sel = decoder.filter_records(pred, dev, n)
    taken = decoder.take_records(sel, dev)
    assert taken.n_rows == int(keep.sum()) == sel.count
    stripes = [(a.rep_levels, a.def_levels, a.values, 2), (b.rep_levels, b.def_levels, b.values, 2),
               (np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8), ids, 0)]
    for col, s in zip(taken.columns, stripes):
        (rl, dl, vals), = KR.take([s], keep)
        assert col.n_slots == len(rl) and col.n_values == len(vals)
        if s[3]:
            assert np.array_equal(col.rep_levels.cpu().numpy()[:len(rl)], rl)
            assert np.array_equal(col.def_levels.cpu().numpy()[:len(dl)], dl)
        got = col.numpy()
        assert list(got) == list(vals)
    path = [A.OPTIONAL, A.REPEATED]
    got = decoder.assemble(path, taken.columns[0].n_slots, taken.columns[0].def_levels, taken.columns[0].rep_levels)
    kept_lens = la[keep]
    assert got["records"] == taken.n_rows
    assert got["nodes"][1]["offsets"].cpu().numpy().tolist() == np.concatenate([[0], np.cumsum(kept_lens)]).tolist()


def test_phonebook_known_answers_on_the_device(decoder):
    cols, ids, cases = phonebook()
    dev = [dev_col(decoder, c) for c in cols]
    for case in cases:
        pred = phonebook_predicate(case["pred"])
        want = check(decoder, pred, cols, dev, len(ids))
        assert ids[want].tolist() == case["ids"], case
    assert json.dumps(cases[1]["pred"]) == '["contains", ["not_eq", "kind", "cell"]]'
