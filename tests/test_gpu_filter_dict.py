"""pqg_filter_run_dict on the GPU: record filters evaluated on dictionary-id columns, bit for bit against
tests/filter_ref.py on the materialised values dictionary[ids] and against pqg_filter_run on the value
decode of the same chunks: the bitmap (with its zero tail bits), the count, the ordered row ids and the
untouched padding of outputs pre-filled with 0xA5, as tests/test_gpu_filter.py compares them.

The id columns are real decodes (PQG_COLUMN_DICTIONARY_IDS) of tools.synth.writer dictionary chunks and
their dictionaries come from Decoder.decode_dictionary. Parquet has no BOOLEAN dictionary pages (pqg_decode
refuses them), so the BOOLEAN id columns are built by hand: ids = the decoded values, dictionary
[false, true]. Row counts below a decoded column's are prefixes of it, as in test_gpu_filter.py."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import filter_ref as R
import take_ref  # noqa: F401  (the chain test checks against it through test_gpu_take.check)
from pqgpu import abi, native
from pqgpu import decoder as D
from pqgpu import filter as F
from test_gpu_filter import POISON64, draw_values, random_levels, run, set_members
from test_gpu_take import busy_stream
from test_gpu_take import check as check_take
from tools.synth import writer

pytestmark = pytest.mark.gpu

T = abi.FILTER_TILE_ROWS
N_MAIN = 3 * T + 17
BOOL, I32, I64, F32, F64, BIN = range(6)
TYPES = [abi.BOOLEAN, abi.INT32, abi.INT64, abi.FLOAT, abi.DOUBLE, abi.BYTE_ARRAY]
LDS = abi.FILTER_DICT_LDS_BYTES


# ---- building columns ------------------------------------------------------------------------------------

def ids_of(col):
    return col.values[:4 * col.n_values].cpu().numpy().view(np.uint32).copy()


def materialise(col):
    """dictionary[ids] on the host: what the reference evaluates."""
    d, ids = col.dictionary.numpy(), ids_of(col)
    if col.physical_type == abi.BYTE_ARRAY:
        return [d[int(i)] for i in ids]
    return np.asarray(d)[ids] if len(ids) else np.zeros(0, dtype=abi.numpy_dtype(col.physical_type))


def boolean_ids(dec, value_col):
    """A BOOLEAN id column by hand: ids = the values, dictionary [false, true]."""
    col = D.DeviceColumn(abi.BOOLEAN, value_col.typed().to(torch.int32).view(torch.uint8), value_col.def_levels)
    col.n_values, col.max_def, col.flags = value_col.n_values, value_col.max_def, abi.COLUMN_DICTIONARY_IDS
    col.dictionary = D.DeviceColumn(abi.BOOLEAN, torch.tensor([0, 1] + [0xA5] * 14, dtype=torch.uint8, device=dec.device))
    col.dictionary.n_values = 2
    return col


def decode_chunks(dec, chunks):
    """The chunks decoded as values and as ids (+ dictionaries) -> (value columns, id columns)."""
    vbatch = writer.build_batch(chunks)
    vals, _ = dec.decode(dec.upload(vbatch))
    ibatch = writer.build_batch(chunks)
    for i in range(len(chunks)):
        if ibatch.columns[i]["dict_offset"] >= 0:
            ibatch.columns[i]["flags"] = abi.COLUMN_DICTIONARY_IDS
    dbatch = dec.upload(ibatch)
    ids, _ = dec.decode(dbatch)
    for i, c in enumerate(ids):
        if c.flags & abi.COLUMN_DICTIONARY_IDS:
            c.dictionary = dec.decode_dictionary(dbatch, i)
        else:
            assert c.physical_type == abi.BOOLEAN
            ids[i] = boolean_ids(dec, c)
    return vals, ids


class Data:
    """One set of columns three ways: id columns, value columns of the same chunks, reference columns over
    the materialised values. `mixed` lists the id columns then the value columns (2k columns)."""

    def __init__(self, dec, specs, n_rows, page_rows=5000):
        """specs: (physical_type, max_def, def_levels or None, dense values)."""
        chunks = [writer.write_column_chunk(t, v, abi.PLAIN if t == abi.BOOLEAN else abi.RLE_DICTIONARY,
                                            def_levels=dl if md else None, max_def=md, page_rows=page_rows)
                  for t, md, dl, v in specs]
        self.setup(dec, chunks, [(md, dl) for _, md, dl, _ in specs], n_rows)

    def setup(self, dec, chunks, levels, n_rows):
        self.n_rows = n_rows
        self.vals, self.ids = decode_chunks(dec, chunks)
        self.ref = [R.RefColumn(c.physical_type, materialise(c), dl if md else None, md) for c, (md, dl) in zip(self.ids, levels)]

    @classmethod
    def from_ids(cls, dec, columns, n_rows, page_rows=5000):
        """columns: (physical_type, dictionary values, ids, max_def, def_levels) through write_dict_column_from_ids."""
        self = cls.__new__(cls)
        chunks = [writer.write_dict_column_from_ids(t, dv, ids, page_rows=page_rows, def_levels=dl if md else None, max_def=md)
                  for t, dv, ids, md, dl in columns]
        self.setup(dec, chunks, [(md, dl) for _, _, _, md, dl in columns], n_rows)
        return self

    def prefix(self, n):
        if n == self.n_rows:
            return self.ids, self.vals, self.ref
        ids, vals = [], []
        for i, v, r in zip(self.ids, self.vals, self.ref):
            i2, v2 = copy.copy(i), copy.copy(v)
            i2.n_values = v2.n_values = int(r.valid(n).sum())
            ids.append(i2)
            vals.append(v2)
        return ids, vals, self.ref


def outputs(dec, pred, dev, n_rows, **kw):
    words, ids, sel = run(dec, pred, dev, n_rows, **kw)
    count = sel.count
    return count, words.cpu().numpy(), None if ids is None else ids.cpu().numpy(), sel


def check(dec, pred, dev_ids, dev_vals, ref, n_rows, capacity=None, row_ids=True):
    """pqg_filter_run_dict on dev_ids against the reference and, when dev_vals is given, against
    pqg_filter_run on it: count, bitmap words with tail bits, row ids, poison past them."""
    count, words, ids, sel = outputs(dec, pred, dev_ids, n_rows, capacity=capacity, row_ids=row_ids)
    want = R.evaluate(pred, ref, n_rows)
    want_ids = np.flatnonzero(want).astype(np.int64)
    n_words = (n_rows + 63) // 64
    print(f"{pred!r}: n_rows {n_rows} selected {count} (reference {want_ids.size})")
    assert count == want_ids.size, repr(pred)
    assert np.array_equal(words[:n_words].view(np.uint64), R.bitmap_words(want)), repr(pred)
    assert (words[n_words:] == POISON64).all()
    if row_ids:
        k = min(n_rows if capacity is None else capacity, want_ids.size)
        assert np.array_equal(ids[:k], want_ids[:k]), repr(pred)
        assert (ids[k:] == POISON64).all()
        assert np.array_equal(sel.row_ids.cpu().numpy(), want_ids[:k])
    if dev_vals is not None:
        vcount, vwords, vids, _ = outputs(dec, pred, dev_vals, n_rows, capacity=capacity, row_ids=row_ids)
        assert vcount == count and np.array_equal(vwords, words), repr(pred)
        assert vids is None or np.array_equal(vids, ids), repr(pred)
    return count


def main_specs(rng, max_def, n=N_MAIN):
    specs = []
    for t in TYPES:
        dl = random_levels(rng, n, max_def) if max_def else None
        k = n if dl is None else int((dl == max_def).sum())
        specs.append((t, max_def, dl, draw_values(rng, t, k)))
    return specs


@pytest.fixture(scope="module")
def mains(decoder):
    """The six types at max_def 0, 1 and 3."""
    return {md: Data(decoder, main_specs(np.random.default_rng(500 + md), md), N_MAIN) for md in (0, 1, 3)}


# ---- types and nullability -----------------------------------------------------------------------------------

@pytest.mark.parametrize("max_def", [0, 1, 3])
def test_random_trees_over_id_and_value_columns(decoder, mains, max_def):
    """40 trees of depth <= 4 whose leaves name id columns (0-5) and value columns (6-11) of every type."""
    d = mains[max_def]
    rng = np.random.default_rng(40 + max_def)
    hits = 0
    for _ in range(40):
        pred = R.random_predicate(rng, TYPES + TYPES, 4)
        hits += check(decoder, pred, d.ids + d.vals, d.vals + d.vals, d.ref + d.ref, N_MAIN)
    assert hits > 0


@pytest.mark.parametrize("c", range(6), ids=[abi.TYPE_NAMES[t] for t in TYPES])
@pytest.mark.parametrize("max_def", [0, 1, 3])
def test_every_op_on_an_id_column(decoder, mains, max_def, c):
    d = mains[max_def]
    t, column = TYPES[c], F.col(c)
    ops = [F.eq, F.not_eq] + ([] if t == abi.BOOLEAN else [F.lt, F.lt_eq, F.gt, F.gt_eq])
    preds = [mk(column, lit) for lit in R.EDGE[t] for mk in ops]
    preds += [mk(column, None) for mk in (F.eq, F.not_eq)] + [mk(column, R.EDGE[t][:2]) for mk in (F.in_, F.not_in)]
    preds += [F.not_(p) for p in preds[:4]]  # not() pushed down onto the leaf
    assert sum(check(decoder, p, d.ids, d.vals, d.ref, N_MAIN) for p in preds) > 0


def test_the_dictionary_is_what_the_value_decode_reads(decoder, mains):
    """dictionary[ids] equals the value decode of the same chunk, every type and nullability."""
    for d in mains.values():
        for i, v in zip(d.ids, d.vals):
            got, want = materialise(i), v.numpy()
            assert i.n_values == v.n_values
            if i.physical_type == abi.BYTE_ARRAY:
                assert got == want
            else:
                assert np.asarray(got).tobytes() == np.asarray(want).tobytes()  # NaN payloads and -0.0 included


# ---- row counts ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, T - 1, T, T + 1])
def test_row_counts(decoder, mains, n):
    ids, vals, ref = mains[1].prefix(n)
    pred = F.or_(F.and_(F.lt_eq(F.col(I32), 3), F.not_eq(F.col(F64), 1.5)),
                 F.or_(F.eq(F.col(I64), None), F.gt(F.col(BIN), b"ab")))
    check(decoder, pred, ids, vals, ref, n)
    check(decoder, F.not_eq(F.col(BOOL), True), ids, vals, ref, n)


# ---- dictionary sizes ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("t", [abi.INT64, abi.BYTE_ARRAY])
@pytest.mark.parametrize("n_entries", [1, 64, 65, 1000])
def test_dictionary_sizes(decoder, n_entries, t):
    """One word, exactly one word, one entry into the second, 16 words (k_filter_dict: several waves)."""
    n = T + 100
    rng = np.random.default_rng(n_entries)
    if t == abi.INT64:
        entries = rng.permutation(n_entries).astype(np.int64) - n_entries // 2
        lits = [int(entries[0]), int(entries[-1]), 0, n_entries]
    else:
        entries = [b"k%05d" % int(x) for x in rng.permutation(n_entries)]
        lits = [entries[0], entries[-1], b"k00000", b"k"]
    dl = random_levels(rng, n, 1)
    ids = rng.integers(0, n_entries, size=int((dl == 1).sum()))
    ids[:2] = [n_entries - 1, 0]  # the last entry (the last bit of the last word) is used
    data = Data.from_ids(decoder, [(t, entries, ids, 1, dl)], n)
    assert data.ids[0].dictionary.n_values == n_entries
    c = F.col(0)
    for lit in lits:
        for mk in (F.eq, F.not_eq, F.lt, F.gt_eq):
            check(decoder, mk(c, lit), data.ids, data.vals, data.ref, n)
    check(decoder, F.in_(c, lits), data.ids, data.vals, data.ref, n)


def test_tables_on_both_sides_of_the_lds_budget(decoder):
    """Two table leaves on one id column: 2 x 511 words (16 bytes under PQG_FILTER_DICT_LDS_BYTES, staged in LDS),
    2 x 512 (exactly the budget, still LDS) and 2 x 513 (16 bytes over: read from global memory). Same ids,
    same predicates; the larger dictionaries only add entries no row uses, so all three must agree."""
    per_leaf = LDS // 2 // 8  # words per table at exactly the budget
    n = T + 500
    rng = np.random.default_rng(8)
    used = (per_leaf - 1) * 64
    entries = rng.integers(-2**40, 2**40, size=(per_leaf + 1) * 64).astype(np.int64)
    ids = rng.integers(0, used, size=n)
    ids[:3] = [used - 1, 0, 63]
    preds = [F.and_(F.gt(F.col(0), 0), F.not_eq(F.col(0), int(entries[5]))),
             F.or_(F.in_(F.col(0), [int(x) for x in entries[:20]]), F.lt(F.col(0, unsigned=True), 1 << 39))]
    got = []
    for words in (per_leaf - 1, per_leaf, per_leaf + 1):
        data = Data.from_ids(decoder, [(abi.INT64, entries[:words * 64], ids, 0, None)], n, page_rows=1 << 20)
        assert data.ids[0].dictionary.n_values == words * 64
        assert (2 * words * 8 <= LDS) == (words <= per_leaf)
        for p in preds:
            check(decoder, p, data.ids, data.vals, data.ref, n)
            got.append(outputs(decoder, p, data.ids, n)[1:3])
    for k in range(len(preds)):
        for other in (got[k + len(preds)], got[k + 2 * len(preds)]):
            assert np.array_equal(got[k][0], other[0]) and np.array_equal(got[k][1], other[1])


def test_byte_array_dictionary_entry_lengths(decoder):
    """Entries of length 0, 1, 3, 4, 5, 33 and 70, shared prefixes, bytes >= 0x80."""
    entries = [b"", b"a", b"abc", b"abcd", b"abcde", b"abcd" + b"\xff" * 29, b"abcde" + b"\x80" * 65, b"ab\x80", b"\xff\xfe"]
    assert [len(e) for e in entries[:7]] == [0, 1, 3, 4, 5, 33, 70]
    n = T + 100
    rng = np.random.default_rng(5)
    ids = rng.integers(0, len(entries), size=n)
    data = Data.from_ids(decoder, [(abi.BYTE_ARRAY, entries, ids, 0, None)], n)
    c = F.col(0)
    for lit in entries + [b"abcd" + b"\xff" * 28, b"abcde" + b"\x80" * 66, b"abd"]:
        for mk in (F.eq, F.lt, F.lt_eq, F.gt, F.gt_eq, F.not_eq):
            check(decoder, mk(c, lit), data.ids, data.vals, data.ref, n)
    check(decoder, F.in_(c, entries[2:7]), data.ids, data.vals, data.ref, n)
    check(decoder, F.not_in(c, entries[:9] + [b"zz"] * 3), data.ids, data.vals, data.ref, n)


def test_duplicate_entries_zeros_and_nans(decoder):
    """Duplicate entries, 0.0 and -0.0, and two NaN payloads are distinct ids with the comparator's verdicts."""
    n = T + 64
    rng = np.random.default_rng(6)
    f32 = np.array([0.0, -0.0, 1.5, 0.0], dtype=np.float32).tolist()
    f32 = np.concatenate([np.array(f32, dtype=np.float32), np.array([0x7FC00000, 0xFFC00001], dtype=np.uint32).view(np.float32)])
    f64 = np.concatenate([np.array([0.0, -0.0, 1.5, -0.0], dtype=np.float64),
                          np.array([0x7FF8000000000000, 0xFFF8000000000123], dtype=np.uint64).view(np.float64)])
    i64 = np.array([5, 5, 7, 5, -1], dtype=np.int64)
    cols = [(abi.FLOAT, f32, rng.integers(0, len(f32), size=n), 0, None),
            (abi.DOUBLE, f64, rng.integers(0, len(f64), size=n), 0, None),
            (abi.INT64, i64, rng.integers(0, len(i64), size=n), 0, None),
            (abi.BYTE_ARRAY, [b"x", b"x", b"", b"x\x00", b""], rng.integers(0, 5, size=n), 0, None)]
    data = Data.from_ids(decoder, cols, n)
    assert [c.dictionary.n_values for c in data.ids] == [6, 6, 5, 5]  # the duplicates stay entries of their own
    lits = {0: [np.float32(0.0), np.float32(-0.0), f32[4], f32[5]], 1: [np.float64(0.0), np.float64(-0.0), f64[4], f64[5]],
            2: [5, 7], 3: [b"x", b""]}
    for c, ls in lits.items():
        for lit in ls:
            for mk in (F.eq, F.not_eq, F.lt, F.lt_eq, F.gt, F.gt_eq):
                check(decoder, mk(F.col(c), lit), data.ids, data.vals, data.ref, n)
        check(decoder, F.in_(F.col(c), ls[:2]), data.ids, data.vals, data.ref, n)
    n_nan = check(decoder, F.eq(F.col(0), np.float32(np.nan)), data.ids, data.vals, data.ref, n)
    assert n_nan == int((ids_of(data.ids[0]) >= 4).sum())  # both payloads are the one NaN of Float.compare


# ---- sets and unsigned leaves -----------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [9, 40])
@pytest.mark.parametrize("c", [I32, F64, I64, BIN])
def test_in_sets(decoder, mains, c, k):
    """The binary-search probe (more than 8 members) runs per dictionary entry."""
    d = mains[1]
    members = set_members(np.random.default_rng(100 * c + k), TYPES[c], k, d.ref[c].values)
    n_in = check(decoder, F.in_(F.col(c), members), d.ids, d.vals, d.ref, N_MAIN)
    n_not = check(decoder, F.not_in(F.col(c), members), d.ids, d.vals, d.ref, N_MAIN)
    assert n_in + n_not == N_MAIN and n_in > 0
    check(decoder, F.not_in(F.col(c), [None] + members), d.ids, d.vals, d.ref, N_MAIN)


@pytest.mark.parametrize("c", [I32, I64])
def test_signed_and_unsigned_leaves_on_one_id_column(decoder, mains, c):
    """Two leaves, two tables over one dictionary: the unsigned flag is the leaf's."""
    d = mains[1]
    u, s = F.col(c, unsigned=True), F.col(c)
    n_u = check(decoder, F.gt(u, 5), d.ids, d.vals, d.ref, N_MAIN)
    n_s = check(decoder, F.gt(s, 5), d.ids, d.vals, d.ref, N_MAIN)
    assert n_u > n_s  # the negative values are above 5 in unsigned order
    for lit in (5, -5, 0, -1):
        check(decoder, F.and_(F.gt(u, lit), F.lt(s, lit)), d.ids, d.vals, d.ref, N_MAIN)
        check(decoder, F.or_(F.lt_eq(u, lit), F.not_(F.lt_eq(s, lit))), d.ids, d.vals, d.ref, N_MAIN)


# ---- nulls -------------------------------------------------------------------------------------------------------

def hand_column(dec, t, ids, def_levels, max_def, dictionary):
    """An id column over hand-built tensors, laid out as decode() leaves it."""
    raw = torch.from_numpy(np.concatenate([np.asarray(ids, dtype=np.uint32), np.full(4, 0xA5A5A5A5, dtype=np.uint32)]).view(np.uint8))
    col = D.DeviceColumn(t, raw.to(dec.device), None if def_levels is None else torch.from_numpy(def_levels).to(dec.device))
    col.n_values, col.max_def, col.flags, col.dictionary = len(ids), max_def, abi.COLUMN_DICTIONARY_IDS, dictionary
    return col


def test_an_all_null_column_with_an_empty_dictionary(decoder, mains):
    n = N_MAIN
    d = mains[1]
    for t in (abi.INT64, abi.BYTE_ARRAY):
        empty = D.DeviceColumn(t, torch.zeros(16, dtype=torch.uint8, device=decoder.device), None, None, 0,
                               torch.zeros(16, dtype=torch.uint8, device=decoder.device) if t == abi.BYTE_ARRAY else None)
        dl = np.zeros(n, dtype=np.uint8)
        col = hand_column(decoder, t, [], dl, 1, empty)
        ids, ref = d.ids + [col], d.ref + [R.RefColumn(t, [], dl, 1)]
        lit = 5 if t == abi.INT64 else b"a"
        c = F.col(6)
        for pred in (F.eq(c, lit), F.not_eq(c, lit), F.lt(c, lit), F.eq(c, None), F.not_eq(c, None), F.not_in(c, [lit]),
                     F.and_(F.not_eq(c, lit), F.lt(F.col(I32), 0))):
            check(decoder, pred, ids, None, ref, n)


def test_a_missing_column_beside_id_columns(decoder, mains):
    d = mains[3]
    miss = [F.MissingColumn(abi.INT64, 1), F.MissingColumn(abi.BYTE_ARRAY, 2)]
    ids, vals = d.ids + miss, d.vals + miss
    ref = d.ref + [R.RefColumn(abi.INT64, max_def=1, missing=True), R.RefColumn(abi.BYTE_ARRAY, max_def=2, missing=True)]
    m, mb = F.col(6), F.col(7)
    for pred in (F.and_(F.not_eq(m, 5), F.lt(F.col(I32), 0)), F.or_(F.eq(mb, b"a"), F.not_(F.gt(F.col(BIN), b"ab"))),
                 F.and_(F.eq(m, None), F.in_(F.col(I64), [0, 1, 7]))):
        check(decoder, pred, ids, vals, ref, N_MAIN)


@pytest.mark.parametrize("max_def", [1, 3])
def test_null_literals_on_id_columns(decoder, mains, max_def):
    """eq(c, null) / not_in(c, [.., null]) depend on validity alone: no table, and alone no k_filter_dict launch."""
    d = mains[max_def]
    for c, t in enumerate(TYPES):
        col, lit = F.col(c), R.EDGE[t][1]
        n_null = check(decoder, F.eq(col, None), d.ids, d.vals, d.ref, N_MAIN)
        assert n_null == int((~d.ref[c].valid(N_MAIN)).sum()) > 0
        for pred in (F.not_eq(col, None), F.not_in(col, [lit, None]), F.in_(col, [None, lit]), F.not_(F.eq(col, None)),
                     F.or_(F.eq(col, None), F.eq(col, lit))):
            check(decoder, pred, d.ids, d.vals, d.ref, N_MAIN)


# ---- errors -------------------------------------------------------------------------------------------------------

def with_bad_id(dec, data, c, bad):
    """data.ids with column c's id of the last non-null row (a row of the last tile) replaced by `bad`."""
    col = data.ids[c]
    ids = ids_of(col)
    assert data.ref[c].valid(N_MAIN)[3 * T:].any()
    ids[-1] = bad
    dl = col.def_levels.cpu().numpy() if col.def_levels is not None else None
    out = list(data.ids)
    out[c] = hand_column(dec, col.physical_type, ids, dl, col.max_def, col.dictionary)
    return out


@pytest.mark.parametrize("c", [I64, BIN])
@pytest.mark.parametrize("which", ["n_entries", "0xFFFFFFFF"])
def test_an_id_outside_the_dictionary_is_an_error(decoder, mains, which, c):
    d = mains[1]
    bad = d.ids[c].dictionary.n_values if which == "n_entries" else 0xFFFFFFFF
    dev = with_bad_id(decoder, d, c, bad)
    lit = R.EDGE[TYPES[c]][1]
    pred = F.or_(F.lt(F.col(I32), 0), F.and_(F.not_eq(F.col(c), lit), F.not_eq(F.col(BOOL), True)))
    for p in (pred, F.eq(F.col(c), None)):  # with a table, and on a leaf that needs none
        words, ids, sel = run(decoder, p, dev, N_MAIN)
        with pytest.raises(native.PqgError) as e:
            sel.count
        assert e.value.code == abi.ERR_DICT_ID
        assert sel._result.cpu().numpy()[8:16].view(np.int32).tolist() == [abi.ERR_DICT_ID, c]
    # the lowest column of two; a column the predicate does not name is not read
    both = with_bad_id(decoder, d, F32, 0xFFFFFFFF)
    both[c] = dev[c]
    words, ids, sel = run(decoder, F.and_(F.gt(F.col(F32), np.float32(0)), pred), both, N_MAIN)
    with pytest.raises(native.PqgError):
        sel.count
    assert sel._result.cpu().numpy()[8:16].view(np.int32).tolist() == [abi.ERR_DICT_ID, min(c, F32)]
    other = F.and_(F.lt_eq(F.col(I32), 3), F.not_eq(F.col(F64), 1.5))
    check(decoder, other, dev, d.vals, d.ref, N_MAIN)
    check(decoder, pred, d.ids, d.vals, d.ref, N_MAIN)  # the context goes on working


@pytest.mark.parametrize("delta", [-1, 1])
def test_wrong_n_values_is_an_error_and_comes_first(decoder, mains, delta):
    d = mains[1]
    dev = with_bad_id(decoder, d, I32, 0xFFFFFFFF)  # a bad id in a lower column as well
    dev[I64] = copy.copy(dev[I64])
    dev[I64].n_values += delta
    pred = F.or_(F.lt(F.col(I32), 0), F.not_eq(F.col(I64), 7))
    words, ids, sel = run(decoder, pred, dev, N_MAIN)
    with pytest.raises(native.PqgError) as e:
        sel.count
    assert e.value.code == abi.ERR_INVALID_ARG
    assert sel._result.cpu().numpy()[8:16].view(np.int32).tolist() == [abi.ERR_INVALID_ARG, I64]


def test_refusals_before_any_launch(decoder, mains):
    d = mains[1]
    pred = F.lt(F.col(I64), 0)

    def refused(edit):
        dev = list(d.ids)
        dev[I64] = copy.copy(dev[I64])
        edit(dev[I64])
        with pytest.raises(native.PqgError) as e:
            decoder.filter(pred, dev, N_MAIN)
        return e.value.code

    def misalign(c): c.values = c.values[2:]
    def no_levels(c): c.def_levels = None  # max_def stays 1: a missing column that carries a dictionary
    assert refused(misalign) == abi.ERR_INVALID_ARG
    assert refused(no_levels) == abi.ERR_INVALID_ARG
    dev = list(d.ids)
    dev[BIN] = copy.copy(dev[BIN])
    dev[BIN].dictionary = copy.copy(dev[BIN].dictionary)
    dev[BIN].dictionary.binary_data = None
    with pytest.raises(native.PqgError) as e:
        decoder.filter(F.eq(F.col(BIN), b"a"), dev, N_MAIN)
    assert e.value.code == abi.ERR_INVALID_ARG
    # non-zero reserved, through the C ABI
    flt = F.Filter(pred, d.ids)
    cols = (abi.FilterColumn * 6)()
    dicts = (abi.FilterDictionary * 6)()
    c = d.ids[I64]
    cols[I64].physical_type, cols[I64].max_def, cols[I64].n_values = abi.INT64, c.max_def, c.n_values
    cols[I64].values, cols[I64].def_levels = c.values.data_ptr(), c.def_levels.data_ptr()
    dicts[I64].values, dicts[I64].n_entries, dicts[I64].reserved = c.dictionary.values.data_ptr(), c.dictionary.n_values, 1
    for i, t in enumerate(TYPES):
        cols[i].physical_type = t
    words = torch.zeros(N_MAIN // 64 + 1, dtype=torch.int64, device=decoder.device)
    result = torch.zeros(16, dtype=torch.uint8, device=decoder.device)
    rc = native.lib().pqg_filter_run_dict(decoder.ctx, flt.handle, C.addressof(cols), C.addressof(dicts), 6, N_MAIN,
                                          words.data_ptr(), None, 0, result.data_ptr())
    assert rc == abi.ERR_INVALID_ARG
    dicts[I64].reserved = 0
    rc = native.lib().pqg_filter_run_dict(decoder.ctx, flt.handle, C.addressof(cols), C.addressof(dicts), 6, N_MAIN,
                                          words.data_ptr(), None, 0, result.data_ptr())
    assert rc == abi.OK
    decoder.stream.synchronize()
    assert int(result.cpu().numpy()[:8].view(np.uint64)[0]) == int(R.evaluate(pred, d.ref, N_MAIN).sum())
    flt.close()


# ---- capacity -------------------------------------------------------------------------------------------------------

def test_row_id_capacity_and_no_row_ids(decoder, mains):
    d = mains[1]
    pred = F.not_eq(F.col(I32), 0)
    full = check(decoder, pred, d.ids, d.vals, d.ref, N_MAIN)
    for cap in (0, 1, 100, full - 1):
        assert check(decoder, pred, d.ids, d.vals, d.ref, N_MAIN, capacity=cap) == full
    check(decoder, F.lt(F.col(F64), 0.5), d.ids, d.vals, d.ref, N_MAIN, row_ids=False)
    ids, vals, ref = d.prefix(0)
    check(decoder, F.lt(F.col(F64), 0.5), ids, vals, ref, 0, row_ids=False)


# ---- decode ids -> filter on ids -> take ------------------------------------------------------------------------------

def test_filter_then_take_without_a_sync(decoder, mains):
    """Late materialisation: the selection of a filter on id columns gathers id and value columns, stream order alone."""
    d = mains[1]
    pred = F.and_(F.in_(F.col(BIN), R.EDGE[abi.BYTE_ARRAY][:4]), F.or_(F.gt(F.col(I64), 0), F.eq(F.col(F32), None)))
    keep = R.evaluate(pred, d.ref, N_MAIN)
    assert 0 < keep.sum() < N_MAIN
    dev = [d.ids[I64], d.ids[BIN], d.vals[F64], d.vals[BIN], d.ids[I32]]
    ref = [R.RefColumn(c.physical_type, ids_of(c), d.ref[i].def_levels, 1) for c, i in ((d.ids[I64], I64), (d.ids[BIN], BIN))]
    ref += [d.ref[F64], d.ref[BIN], R.RefColumn(abi.INT32, ids_of(d.ids[I32]), d.ref[I32].def_levels, 1)]
    sel = decoder.filter(pred, d.ids, N_MAIN)
    taken, outs, want = check_take(decoder, dev, ref, keep, selection=sel)
    assert taken.n_rows == int(keep.sum()) == sel.count
    # the kept ids materialise to the kept values
    kept_ids = taken.columns[0].values[:4 * taken.columns[0].n_values].cpu().numpy().view(np.uint32)
    kept_rows = keep & d.ref[I64].valid(N_MAIN)
    dense = np.cumsum(d.ref[I64].valid(N_MAIN)) - 1
    assert np.array_equal(np.asarray(d.ids[I64].dictionary.numpy())[kept_ids], np.asarray(d.ref[I64].values)[dense[kept_rows]])


# ---- the pinned dictionary-table slots -----------------------------------------------------------------------------

def test_slot_reuse_in_queued_calls(decoder):
    """2 * FILTER_DICT_SLOTS + 1 calls of pqg_filter_run_dict queued on one context with no wait between them: one
    filter, one id column of 256 rows, a dictionary of 4 entries that differs from call to call (entry j lies
    below the literal in call k when bit j of k + 1 is set). The dictionary table goes up through a pinned slot
    that the call FILTER_DICT_SLOTS later reuses: a slot overwritten before the copy out of it has run shows as
    a call that selected by another call's dictionary."""
    n, calls = 256, 9
    rng = np.random.default_rng(92)
    ids = rng.integers(0, 4, size=n).astype(np.uint32)
    assert set(ids) == {0, 1, 2, 3}
    pred = F.lt(F.col(0), 50)
    cols, refs = [], []
    for k in range(calls):
        entries = np.array([1 if (k + 1) >> j & 1 else 100 for j in range(4)], dtype=np.int32)
        raw = np.concatenate([entries, np.full(4, 0x5A5A5A5A, dtype=np.int32)]).view(np.uint8)
        d = D.DeviceColumn(abi.INT32, torch.from_numpy(raw).to(decoder.device))
        d.n_values = 4
        cols.append(hand_column(decoder, abi.INT32, ids, None, 0, d))
        refs.append(R.RefColumn(abi.INT32, entries[ids], None, 0))
    flt = F.Filter(pred, [cols[0]])
    held = busy_stream(decoder)
    runs = [run(decoder, flt, [c], n) for c in cols]
    seen = set()
    for (words, _, sel), ref in zip(runs, refs):
        want = R.evaluate(pred, [ref], n)
        assert sel.count == int(want.sum())
        got = words.cpu().numpy()
        assert np.array_equal(got[:n // 64].view(np.uint64), R.bitmap_words(want))
        assert (got[n // 64:] == POISON64).all()
        assert np.array_equal(sel.row_ids.cpu().numpy(), np.flatnonzero(want))
        seen.add(want.tobytes())
    assert len(seen) == calls  # every call has an answer of its own
    del held


# ---- decode_dictionary -------------------------------------------------------------------------------------------------

def dictionary_chunk(t, rng, n_entries, n, type_length=0):
    """(chunk, its dictionary entries in id order, the dense values): distinct entries, each used, ids in
    first-appearance order as the writer assigns them."""
    if t == abi.BYTE_ARRAY:
        entries = [bytes(rng.integers(0, 256, size=int(rng.integers(0, 40)), dtype=np.uint8)) for _ in range(n_entries)]
        entries = list(dict.fromkeys(entries))
    elif t in (abi.INT96, abi.FIXED_LEN_BYTE_ARRAY):
        w = abi.elem_width(t, type_length)
        entries = list(dict.fromkeys(rng.integers(1, 256, size=w, dtype=np.uint8).tobytes() for _ in range(n_entries)))
    else:
        entries = (rng.permutation(4000)[:n_entries] - 2000).astype(abi.numpy_dtype(t))
        if t in (abi.FLOAT, abi.DOUBLE):
            entries = entries / 4
    ids = np.concatenate([np.arange(len(entries)), rng.integers(0, len(entries), size=n - len(entries))])
    vals = [entries[int(i)] for i in ids] if not isinstance(entries, np.ndarray) else entries[ids]
    return writer.write_column_chunk(t, vals, abi.RLE_DICTIONARY, type_length=type_length), entries, vals


@pytest.mark.parametrize("t,tl", [(abi.INT32, 0), (abi.INT64, 0), (abi.INT96, 0), (abi.FLOAT, 0), (abi.DOUBLE, 0),
                                  (abi.BYTE_ARRAY, 0), (abi.FIXED_LEN_BYTE_ARRAY, 7)], ids=lambda x: str(x))
def test_decode_dictionary_every_type(decoder, t, tl):
    """The decoded dictionary is the writer's, entry for entry, and dictionary[ids] is the value decode."""
    rng = np.random.default_rng(t)
    chunk, entries, vals = dictionary_chunk(t, rng, 37, 500, tl)
    batch = writer.build_batch([chunk])
    batch.columns[0]["flags"] = abi.COLUMN_DICTIONARY_IDS
    dbatch = decoder.upload(batch)
    cols, _ = decoder.decode(dbatch)
    dic = decoder.decode_dictionary(dbatch, 0)
    assert dic.n_values == len(entries) == batch.columns[0]["dict_num_values"] and dic.max_def == 0
    got = dic.numpy()
    ids = ids_of(cols[0])
    if t == abi.BYTE_ARRAY:
        assert got == list(entries) and [got[int(i)] for i in ids] == list(vals)
    elif t in (abi.INT96, abi.FIXED_LEN_BYTE_ARRAY):
        assert got.tobytes() == b"".join(entries) and got[ids].tobytes() == b"".join(vals)
    else:
        assert got.tobytes() == entries.tobytes() and got[ids].tobytes() == np.asarray(vals).tobytes()
    vcols, _ = decoder.decode(decoder.upload(writer.build_batch([chunk])))  # the value decode of the same chunk
    if t == abi.BYTE_ARRAY:
        assert vcols[0].numpy() == [got[int(i)] for i in ids]
    else:
        assert vcols[0].numpy().tobytes() == got[ids].tobytes()


def test_decode_dictionary_of_a_boolean_page(decoder):
    """No writer emits one, but a PLAIN BOOLEAN page decodes like any required column's."""
    chunk = writer.write_column_chunk(abi.INT32, np.arange(10, dtype=np.int32), abi.RLE_DICTIONARY)
    bits = np.array([1, 0, 0, 1, 1, 1, 0, 1, 0, 1, 1], dtype=np.uint8)
    chunk.dict_page = writer.plain_encode(bits, abi.BOOLEAN)
    chunk.dict_num_values = len(bits)
    chunk.physical_type = abi.BOOLEAN
    batch = writer.build_batch([chunk])
    dic = decoder.decode_dictionary(decoder.upload(batch), 0)
    assert dic.n_values == len(bits) and np.array_equal(dic.numpy(), bits)


@pytest.mark.parametrize("t", [abi.INT64, abi.BYTE_ARRAY])
def test_a_dictionary_page_cut_short(decoder, t):
    """The page holds fewer entries than its header says: the code pqg_decode reports for the same page."""
    rng = np.random.default_rng(3)
    chunk, entries, vals = dictionary_chunk(t, rng, 20, 100)
    chunk.dict_page = chunk.dict_page[:len(chunk.dict_page) - 3]
    batch = writer.build_batch([chunk])
    dbatch = decoder.upload(batch)
    cols, st = decoder.decode(dbatch, check=False)
    assert st.code != abi.OK and (t != abi.INT64 or st.code == abi.ERR_EOF)
    with pytest.raises(native.PqgError) as e:
        decoder.decode_dictionary(dbatch, 0)
    assert e.value.code == st.code


def test_decode_dictionary_errors(decoder):
    chunk = writer.write_column_chunk(abi.INT64, np.arange(50, dtype=np.int64), abi.RLE_DICTIONARY, dict_page_encoding=abi.RLE)
    dbatch = decoder.upload(writer.build_batch([chunk]))
    _, st = decoder.decode(dbatch, check=False)
    with pytest.raises(native.PqgError) as e:
        decoder.decode_dictionary(dbatch, 0)
    assert e.value.code == st.code == abi.ERR_DICT_ENCODING
    plain = decoder.upload(writer.build_batch([writer.write_column_chunk(abi.INT64, np.arange(50, dtype=np.int64), abi.PLAIN)]))
    with pytest.raises(native.PqgError) as e:
        decoder.decode_dictionary(plain, 0)
    assert e.value.code == abi.ERR_NO_DICTIONARY
    # a decode after it goes on as usual
    cols, _ = decoder.decode(plain)
    assert np.array_equal(cols[0].numpy(), np.arange(50))
