"""pqg_filter_row_groups on the GPU (Decoder.filter_row_groups), compared bit for bit with
tests/rowgroup_filter_ref.py: the drop bitmap with its tail bits, the kept ids, the count, and nothing written past
the capacity. Row-group counts around the bitmap word seams, dictionary sizes around the 64-entry step and the
PQG_RG_TILE_ENTRIES tile, every physical type, every operator under every flag combination, empty dictionaries,
duplicates, NaNs and signed zeros, sets on both sides of the linear / binary-search threshold, equals() against the
comparator on DECIMAL and FLOAT16 columns, long and empty BYTE_ARRAY entries, random trees with and without not(),
contains, missing columns, and two calls queued without a sync. Dictionaries are hand-built device columns in the
decoder's layout (tests/test_gpu_rowgroup_decode.py decodes real pages)."""
import numpy as np
import pytest
import torch

import filter_ref as R
import rowgroup_filter_ref as G
import test_gpu_filter_binary as GB
from pqgpu import abi, native
from pqgpu import decoder as D
from pqgpu import filter as F

pytestmark = pytest.mark.gpu

POISON, POISON64 = 0xA5, np.int64(np.uint64(0xA5A5A5A5A5A5A5A5).astype(np.int64))
BA, FLBA, I96 = abi.BYTE_ARRAY, abi.FIXED_LEN_BYTE_ARRAY, abi.INT96
NP_TYPES = {abi.BOOLEAN: np.uint8, abi.INT32: np.int32, abi.INT64: np.int64, abi.FLOAT: np.float32, abi.DOUBLE: np.float64}


def dev_dictionary(dec, t, entries, width=0):
    """The decoded dictionary of `entries` as a DeviceColumn in the decoder's layout, poison behind it."""
    if t == BA:
        return GB.binary_column(dec, [bytes(e) for e in entries])
    if t in (FLBA, I96):
        return GB.fixed_column(dec, t, width, [bytes(e) for e in entries], offset=1 if t == FLBA else 0)
    raw = np.asarray(entries, dtype=NP_TYPES[t]).view(np.uint8)
    buf = torch.full((raw.size + 24,), POISON, dtype=torch.uint8, device=dec.device)
    buf[:raw.size] = torch.from_numpy(raw.copy()).to(dec.device)
    col = D.DeviceColumn(t, buf)
    col.n_values = len(entries)
    return col


class Chunk:
    """One column chunk of one row group for both sides: the RefChunk and the RowGroupColumn."""

    def __init__(self, dec, t, entries=None, missing=False, non_dictionary_pages=False, may_contain_null=True, width=0):
        self.ref = G.RefChunk(t, entries, missing, non_dictionary_pages, may_contain_null)
        d = None if entries is None else dev_dictionary(dec, t, entries, width)
        self.dev = F.RowGroupColumn(d, missing, non_dictionary_pages, may_contain_null, physical_type=t, type_length=width)


def run(dec, pred, groups, capacity=None):
    """groups: [[Chunk per column] per row group] -> the selection, with poisoned outputs checked against the
    reference for the bitmap (tail bits included), the ids up to the capacity, the count, and what lies behind."""
    n = len(groups)
    n_words = (n + 63) // 64
    capacity = n if capacity is None else capacity
    words = torch.full((n_words + 2,), POISON64, dtype=torch.int64, device=dec.device)
    ids = torch.full((capacity + 2,), POISON64, dtype=torch.int64, device=dec.device)
    result = torch.full((16,), POISON, dtype=torch.uint8, device=dec.device)
    sel = dec.filter_row_groups(pred, [[c.dev for c in g] for g in groups], capacity=capacity, out=(words, ids, result))
    want = G.drops(pred, [[c.ref for c in g] for g in groups]) if n else np.zeros(0, dtype=bool)
    what = repr(pred)
    kept = np.flatnonzero(~want).astype(np.int64)
    assert sel.count == kept.size, what
    got = words.cpu().numpy()
    assert np.array_equal(got[:n_words].view(np.uint64), R.bitmap_words(want)), what
    assert (got[n_words:] == POISON64).all(), what
    got_ids = ids.cpu().numpy()
    m = min(kept.size, capacity)
    assert np.array_equal(got_ids[:m], kept[:m]), what
    assert (got_ids[m:] == POISON64).all(), what
    assert np.array_equal(sel.drop.cpu().numpy(), want) and np.array_equal(sel.kept.cpu().numpy(), kept[:m]), what
    return want


@pytest.mark.parametrize("n_groups", [0, 1, 2, 63, 64, 65, 130])
def test_row_group_counts_and_capacities(decoder, n_groups):
    rng = np.random.default_rng(n_groups)
    # one int64 column; every third group holds the literal
    shared = [dev_dictionary(decoder, abi.INT64, rng.integers(100, 200, size=20)),
              dev_dictionary(decoder, abi.INT64, np.concatenate([rng.integers(100, 200, size=19), [7]]))]
    groups = []
    for g in range(n_groups):
        hit = g % 3 == 1
        c = Chunk(decoder, abi.INT64, None, may_contain_null=False)
        c.ref.entries = shared[hit].typed().cpu().numpy().tolist()
        c.dev = F.RowGroupColumn(shared[hit], may_contain_null=False)
        groups.append([c])
    pred = F.eq(F.col(0), 7) if n_groups else F.Filter(F.eq(F.col(0), 7), [abi.INT64])
    want = run(decoder, pred, groups)
    n_kept = int((~want).sum())
    if n_groups >= 2:
        assert 0 < n_kept < n_groups
    for cap in sorted({0, max(n_kept - 1, 0), n_kept, n_kept + 3}):
        run(decoder, pred, groups, capacity=cap)
    run(decoder, F.not_(pred) if n_groups else pred, groups)  # notEq: nothing drops (dictionaries of 20 entries)


def test_dictionary_sizes_in_one_call(decoder):
    """Skewed dictionaries in one work list: the literal sits in the last entry, or nowhere."""
    sizes = [0, 1, 63, 64, 65, 1023, 1024, 1025, 4097]
    groups = []
    for n in sizes:
        for hit in (False, True):
            entries = np.arange(1000, 1000 + n, dtype=np.int64)
            if hit and n:
                entries[-1] = 7
            groups.append([Chunk(decoder, abi.INT64, entries.tolist(), may_contain_null=False),
                           Chunk(decoder, BA, [b"k%07d" % (7 if hit and i == n - 1 else 1000 + i) for i in range(n)],
                                 may_contain_null=False)])
    for c in (0, 1):
        lit = 7 if c == 0 else b"k0000007"
        want = run(decoder, F.eq(F.col(c), lit), groups)
        assert want.tolist() == [not (hit and n) for n in sizes for hit in (False, True)]
        run(decoder, F.in_(F.col(c), [lit, lit]), groups)
        run(decoder, F.not_eq(F.col(c), lit), groups)   # drops only the one-entry hit
        run(decoder, F.gt(F.col(c), 5000 if c == 0 else b"k0005000"), groups)  # holds on the last tile of 4,097 only
    run(decoder, F.and_(F.eq(F.col(0), 7), F.lt(F.col(1), b"k0000008")), groups)


TYPE_CASES = [
    (abi.BOOLEAN, 0, [True], True, False),
    (abi.INT32, 0, [5, -3, 2**31 - 1], 5, 6),
    (abi.INT64, 0, [5, -3, 2**63 - 1], -3, 6),
    (abi.FLOAT, 0, [np.float32(1.5), np.float32(-2.0)], np.float32(1.5), np.float32(1.25)),
    (abi.DOUBLE, 0, [1.5, -2.0], -2.0, 1.25),
    (BA, 0, [b"ab", b"", b"abc"], b"abc", b"abd"),
    (FLBA, 3, [b"\x00\x00\x05", b"\xff\xff\xfd"], b"\x00\x00\x05", b"\x00\x00\x06"),
    (I96, 12, [F.decimal_bytes(5, 12), F.decimal_bytes(-3, 12)], F.decimal_bytes(5, 12), F.decimal_bytes(6, 12)),
]


@pytest.mark.parametrize("t,width,entries,present,absent", TYPE_CASES, ids=[abi.TYPE_NAMES[c[0]] for c in TYPE_CASES])
def test_every_physical_type(decoder, t, width, entries, present, absent):
    order = "signed_integer" if t in (FLBA, I96) else None
    c = F.col(0, order=order)
    groups = [[Chunk(decoder, t, entries, may_contain_null=False, width=width)],
              [Chunk(decoder, t, entries[:1], may_contain_null=False, width=width)],
              [Chunk(decoder, t, [], may_contain_null=False, width=width)],
              [Chunk(decoder, t, None, missing=True, width=width)]]
    ops = [F.eq, F.not_eq] + ([] if t == abi.BOOLEAN else [F.lt, F.lt_eq, F.gt, F.gt_eq])
    drops = 0
    for lit in (present, absent):
        for op in ops:
            drops += int(run(decoder, op(c, lit), groups)[:3].sum())
        drops += int(run(decoder, F.in_(c, [lit]), groups)[:3].sum())
        drops += int(run(decoder, F.not_in(c, [lit]), groups)[:3].sum())
    # BOOLEAN and INT96 never drop on a dictionary; every other type does somewhere
    assert (drops == 0) == (t in (abi.BOOLEAN, I96))


LEAF_OPS = [F.eq, F.not_eq, F.lt, F.lt_eq, F.gt, F.gt_eq]


@pytest.mark.parametrize("t", [abi.INT64, BA], ids=["int64", "binary"])
def test_every_operator_under_every_flag_combination(decoder, t):
    """16 flag combinations x dictionaries that hold only the literal, the literal among others, not the literal,
    and nothing."""
    val = (lambda v: v) if t == abi.INT64 else (lambda v: b"v%03d" % v)
    dicts = [[val(7), val(7)], [val(3), val(7), val(9)], [val(3), val(9)], []]
    groups = []
    for flags in range(16):
        for entries in dicts:
            no_dict = bool(flags & abi.RG_NO_DICTIONARY)
            groups.append([Chunk(decoder, t, None if no_dict else entries, missing=bool(flags & abi.RG_MISSING),
                                 non_dictionary_pages=bool(flags & abi.RG_NON_DICT_PAGES),
                                 may_contain_null=bool(flags & abi.RG_MAY_CONTAIN_NULL))])
            assert groups[-1][0].dev.flags == flags
    c = F.col(0)
    seen = set()
    for op in LEAF_OPS:
        for lit in (val(7), None) if op in (F.eq, F.not_eq) else (val(7),):
            seen.add(tuple(run(decoder, op(c, lit), groups).tolist()))
    for mk in (F.in_, F.not_in):
        for s in ([val(7)], [val(7), val(3), val(9)], [None], [None, val(7)], [val(1)]):
            seen.add(tuple(run(decoder, mk(c, s), groups).tolist()))
    assert len(seen) >= 8  # the cases differ from each other: the reference is not a constant here


def test_empty_dictionaries_and_duplicates(decoder):
    groups = [[Chunk(decoder, abi.INT32, [], may_contain_null=False)],
              [Chunk(decoder, abi.INT32, [], may_contain_null=True)],
              [Chunk(decoder, abi.INT32, [4] * 130, may_contain_null=False)],
              [Chunk(decoder, abi.INT32, [4] * 64 + [5], may_contain_null=False)]]
    c = F.col(0)
    assert run(decoder, F.not_eq(c, 4), groups).tolist() == [False, False, True, False]  # an empty set has no single member
    assert run(decoder, F.not_in(c, [4]), groups).tolist() == [True, False, True, False]
    assert run(decoder, F.eq(c, 4), groups).tolist() == [True, True, False, False]
    assert run(decoder, F.in_(c, [4, 5]), groups).tolist() == [True, True, False, False]
    assert run(decoder, F.lt(c, 100), groups).tolist() == [True, True, False, False]
    assert run(decoder, F.not_in(c, [5, 4]), groups).tolist() == [True, False, True, True]


@pytest.mark.parametrize("t", [abi.FLOAT, abi.DOUBLE], ids=["float", "double"])
def test_nans_and_signed_zeros(decoder, t):
    f = np.float32 if t == abi.FLOAT else np.float64
    bits = np.uint32 if t == abi.FLOAT else np.uint64
    other_nan = np.array([0xFFC00001 if t == abi.FLOAT else 0xFFF8000000000123], dtype=bits).view(f)[0]
    groups = [[Chunk(decoder, t, [f(0.0)], may_contain_null=False)], [Chunk(decoder, t, [f(-0.0)], may_contain_null=False)],
              [Chunk(decoder, t, [other_nan], may_contain_null=False)], [Chunk(decoder, t, [f(1.0), f("inf")], may_contain_null=False)]]
    c = F.col(0)
    assert run(decoder, F.eq(c, f(0.0)), groups).tolist() == [False, True, True, True]     # -0.0 != 0.0
    assert run(decoder, F.eq(c, f(-0.0)), groups).tolist() == [True, False, True, True]
    assert run(decoder, F.eq(c, f("nan")), groups).tolist() == [True, True, False, True]   # one NaN
    assert run(decoder, F.not_eq(c, f("nan")), groups).tolist() == [False, False, True, False]
    assert run(decoder, F.gt(c, f("inf")), groups).tolist() == [True, True, False, True]   # NaN above +Infinity
    assert run(decoder, F.lt(c, f(0.0)), groups).tolist() == [True, False, True, True]     # -0.0 < 0.0
    run(decoder, F.in_(c, [f("nan"), f(0.0), f(2.0)]), groups)
    run(decoder, F.not_in(c, [other_nan, f(-0.0)]), groups)


@pytest.mark.parametrize("t", [abi.INT64, BA, FLBA], ids=["int64", "binary", "decimal_flba"])
@pytest.mark.parametrize("n_set", [1, 8, 9, 300])
def test_in_set_sizes(decoder, t, n_set):
    """Sets on both sides of the linear / binary-search threshold; every member is probed once from a dictionary
    that holds only it."""
    rng = np.random.default_rng(n_set)
    nums = rng.choice(np.arange(-5000, 5000), size=n_set + 40, replace=False)
    val = {abi.INT64: int, BA: lambda v: b"s%+06d" % int(v), FLBA: lambda v: F.decimal_bytes(int(v), 4)}[t]
    members, others = [val(v) for v in nums[:n_set]], [val(v) for v in nums[n_set:]]
    width = 4 if t == FLBA else 0
    groups = [[Chunk(decoder, t, others, may_contain_null=False, width=width)],
              [Chunk(decoder, t, others + [members[-1]], may_contain_null=False, width=width)],
              [Chunk(decoder, t, list(members), may_contain_null=False, width=width)],
              [Chunk(decoder, t, list(members) + others[:1], may_contain_null=False, width=width)]]
    groups += [[Chunk(decoder, t, [m], may_contain_null=False, width=width)] for m in members[:40]]
    c = F.col(0, order="signed_integer" if t == FLBA else None)
    want = run(decoder, F.in_(c, members), groups)
    assert want.tolist() == [True, False, False, False] + [False] * min(n_set, 40)
    want = run(decoder, F.not_in(c, members), groups)
    assert want.tolist() == [False, False, True, False] + [True] * min(n_set, 40)


def test_equality_is_equals_not_the_comparator(decoder):
    """A DECIMAL on BYTE_ARRAY stored as 00 01 does not equal the literal 01 here (Binary.equals), though the
    comparator, and so the record filter, says it does; ordering leaves keep the comparator."""
    groups = [[Chunk(decoder, BA, [b"\x00\x01"], may_contain_null=False)], [Chunk(decoder, BA, [b"\x01"], may_contain_null=False)]]
    c = F.col(0, order="signed_integer")
    assert run(decoder, F.eq(c, b"\x01"), groups).tolist() == [True, False]
    assert run(decoder, F.and_(F.gt_eq(c, b"\x01"), F.lt_eq(c, b"\x01")), groups).tolist() == [False, False]
    assert run(decoder, F.not_eq(c, b"\x01"), groups).tolist() == [False, True]
    assert run(decoder, F.in_(c, [b"\x01", b"\x00\x00\x01"]), groups).tolist() == [True, False]
    twelve = [F.decimal_bytes(v) for v in (1, 3, -1, 7, -20, 11, 19, -33, 2)] + [b"", b"\x00\x00", b"\xff" * 9]
    assert run(decoder, F.in_(c, twelve), groups).tolist() == [True, False]        # re-sorted by bytes for the search
    assert run(decoder, F.not_in(c, twelve), groups).tolist() == [False, True]
    # the record filter on the same filter object still compares: the two images do not disturb each other
    flt = F.Filter(F.eq(c, b"\x01"), [BA])
    col = GB.binary_column(decoder, [b"\x00\x01", b"\x01", b"\x02"])
    assert decoder.filter(flt, [col], 3).count == 2
    sel = decoder.filter_row_groups(flt, [[g[0].dev] for g in groups])
    assert sel.drop.cpu().numpy().tolist() == [True, False] and decoder.filter(flt, [col], 3).count == 2
    # FLOAT16: NaNs with different payloads are one value to Float16.compare and two to equals()
    nan_a, nan_b = (0x7E00).to_bytes(2, "little"), (0x7E01).to_bytes(2, "little")
    halves = [[Chunk(decoder, FLBA, [nan_a], may_contain_null=False, width=2)], [Chunk(decoder, FLBA, [nan_b], may_contain_null=False, width=2)]]
    h = F.col(0, order="float16")
    assert run(decoder, F.eq(h, nan_a), halves).tolist() == [False, True]
    assert run(decoder, F.gt_eq(h, nan_a), halves).tolist() == [False, False]


def test_binary_entry_lengths(decoder):
    long_a, long_b = b"x" * 4999 + b"a", b"x" * 4999 + b"b"
    entries = [b"", b"q", b"y" * 33, long_a]
    groups = [[Chunk(decoder, BA, entries, may_contain_null=False)], [Chunk(decoder, BA, entries[:3], may_contain_null=False)],
              [Chunk(decoder, BA, [b""], may_contain_null=False)], [Chunk(decoder, BA, [long_b, long_a, b""] * 30, may_contain_null=False)]]
    c = F.col(0)
    assert run(decoder, F.eq(c, long_a), groups).tolist() == [False, True, True, False]
    assert run(decoder, F.eq(c, long_b), groups).tolist() == [True, True, True, False]
    assert run(decoder, F.eq(c, b""), groups).tolist() == [False, False, False, False]
    assert run(decoder, F.not_eq(c, b""), groups).tolist() == [False, False, True, False]
    assert run(decoder, F.gt(c, long_a), groups).tolist() == [False, False, True, False]
    assert run(decoder, F.eq(c, b"y" * 33), groups).tolist() == [False, False, True, True]
    assert run(decoder, F.lt(c, b"\x00"), groups).tolist() == [False, False, False, False]
    run(decoder, F.in_(c, [b"y" * 32, long_b[:4999], b"q"]), groups)


@pytest.mark.parametrize("allow_not", [False, True], ids=["not_free", "with_not"])
def test_random_trees(decoder, allow_not):
    rng = np.random.default_rng(11 + allow_not)
    types = [abi.INT32, abi.INT64, abi.FLOAT, abi.DOUBLE, BA, abi.BOOLEAN]
    groups = []
    for g in range(70):
        row = []
        for t in types:
            kind = rng.random()
            n = int(rng.choice([0, 1, 1, 2, 5, 70]))
            entries = [R.random_literal(rng, t) for _ in range(n)]
            row.append(Chunk(decoder, t, None if kind < 0.1 else entries, missing=kind > 0.9,
                             non_dictionary_pages=0.1 <= kind < 0.2, may_contain_null=bool(rng.random() < 0.5)))
        groups.append(row)
    dropped = kept = 0
    for _ in range(40):
        pred = R.random_predicate(rng, types, 4, allow_not=allow_not)
        want = run(decoder, pred, groups)
        dropped += int(want.sum())
        kept += int((~want).sum())
    assert dropped > 100 and kept > 100


def test_contains_and_missing_columns(decoder):
    letters = [bytes([c]) for c in b"abcdefghijklmnopqrstuvwxyz"]
    groups = [[Chunk(decoder, BA, letters, may_contain_null=False), Chunk(decoder, abi.INT32, None, missing=True)],
              [Chunk(decoder, BA, [b"B", b"x"], may_contain_null=False), Chunk(decoder, abi.INT32, [3], may_contain_null=False)],
              [Chunk(decoder, BA, None, missing=True), Chunk(decoder, abi.INT32, [3, 4])]]
    col = F.col(0)
    B, C, x, y = [F.contains(F.eq(col, v)) for v in (b"B", b"C", b"x", b"y")]
    assert run(decoder, F.and_(B, y), groups).tolist() == [True, True, True]
    assert run(decoder, F.and_(x, y), groups).tolist() == [False, True, True]
    assert run(decoder, F.or_(B, C), groups).tolist() == [True, False, True]
    assert run(decoder, F.or_(x, C), groups).tolist() == [False, False, True]
    assert run(decoder, F.contains(F.not_eq(col, b"x")), groups).tolist() == [False, False, False]
    i = F.col(1)
    assert run(decoder, F.eq(i, 3), groups).tolist() == [True, False, False]
    assert run(decoder, F.eq(i, None), groups).tolist() == [False, False, False]
    assert run(decoder, F.not_eq(i, None), groups).tolist() == [True, False, False]
    assert run(decoder, F.not_in(i, [None]), groups).tolist() == [True, False, False]
    assert run(decoder, F.not_in(i, [None, 3]), groups).tolist() == [False, False, False]
    assert run(decoder, F.not_in(i, [3]), groups).tolist() == [False, True, False]
    assert run(decoder, F.or_(F.eq(col, b"x"), F.gt(i, 3)), groups).tolist() == [False, False, False]
    assert run(decoder, F.and_(F.eq(col, b"x"), F.gt(i, 3)), groups).tolist() == [True, True, True]


def test_refusals(decoder):
    d = dev_dictionary(decoder, BA, [b"a"])
    flt = F.Filter(F.eq(F.col(1), b"a"), [abi.INT32, BA])
    good = [[F.RowGroupColumn(None, physical_type=abi.INT32), F.RowGroupColumn(d)]]
    assert decoder.filter_row_groups(flt, good).count == 1
    with pytest.raises(native.PqgError) as e:  # not the filter's column count
        decoder.filter_row_groups(flt, [[F.RowGroupColumn(d)]])
    assert e.value.code == abi.ERR_INVALID_ARG
    d.binary_data = None
    with pytest.raises(native.PqgError) as e:  # a BYTE_ARRAY dictionary without its bytes
        decoder.filter_row_groups(flt, good)
    assert e.value.code == abi.ERR_INVALID_ARG


def test_queued_calls_share_no_scratch(decoder):
    """Calls queued without a sync between them (more than the ctx has table slots), on different filters and
    tables of different sizes, then read back in any order."""
    rng = np.random.default_rng(5)
    calls = []
    for k, n in enumerate([130, 3, 65, 1, 64]):
        groups = [[Chunk(decoder, abi.INT64, rng.integers(0, 6, size=int(rng.integers(0, 5))).tolist(), may_contain_null=False)]
                  for _ in range(n)]
        pred = F.or_(F.eq(F.col(0), k), F.gt(F.col(0), 4))
        calls.append((pred, groups, decoder.filter_row_groups(pred, [[c.dev for c in g] for g in groups])))
    for pred, groups, sel in reversed(calls):
        want = G.drops(pred, [[c.ref for c in g] for g in groups])
        assert np.array_equal(sel.drop.cpu().numpy(), want)
        assert np.array_equal(sel.kept.cpu().numpy(), np.flatnonzero(~want))
