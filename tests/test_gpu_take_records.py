"""pqg_take_records on the GPU against tests/take_records_ref.py, bit for bit: per column the repetition and
definition bytes of the kept slots, the dense values of the kept slots with a value, BYTE_ARRAY offsets and
bytes, the counts. The inputs are real decodes of tools.synth.writer chunks with rep_levels / max_rep, so
the stripes are the decoder's own. Every output is pre-filled with 0xA5 and holds a few elements more than
its stated capacity; everything past the produced counts must still be 0xA5."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import filter_ref as R
import take_records_ref as KR
import take_ref as K
from oracle import assembly as A
from pqgpu import abi, native
from pqgpu import filter as F
from pqgpu import take as T_
from records import random_record, shred
from tools.synth import writer

pytestmark = pytest.mark.gpu

T = abi.FILTER_TILE_ROWS
N_SLOTS = 3 * T + 17
POISON = 0xA5
SLACK = 3  # elements / bytes every output holds past its stated capacity


# ---- inputs ----------------------------------------------------------------------------------------------

def draw(rng, t, k, type_length=0):
    """k dense values of type t."""
    if t == abi.BYTE_ARRAY:
        return [bytes(rng.integers(0, 256, size=int(rng.integers(0, 9)), dtype=np.uint8)) for _ in range(k)]
    if t in (abi.INT96, abi.FIXED_LEN_BYTE_ARRAY):
        w = abi.elem_width(t, type_length)
        return [rng.integers(0, 256, size=w, dtype=np.uint8).tobytes() for _ in range(k)]
    if t == abi.BOOLEAN:
        return rng.integers(0, 2, size=k).astype(np.uint8)
    return rng.integers(-2**31, 2**31 - 1, size=k).astype(abi.numpy_dtype(t))


def levels(rng, lens, max_rep, max_def, p_null=0.2):
    """(rl, dl) of records of `lens` slots; length 0: an empty or null list, one slot below max_def.
    Repetition values inside a record are 1..max_rep."""
    lens = np.asarray(lens)
    slots = np.maximum(lens, 1)
    n = int(slots.sum())
    rl = rng.integers(1, max_rep + 1, size=n).astype(np.uint8)
    starts = np.cumsum(slots) - slots
    rl[starts] = 0
    dl = np.where(rng.random(n) < p_null, rng.integers(0, max_def, size=n), max_def).astype(np.uint8)
    empty = starts[lens == 0]
    dl[empty] = rng.integers(0, max_def, size=empty.size)
    return rl, dl


def spec(rng, t, n_rows, lens=None, max_rep=0, max_def=0, **kw):
    """One column: lens -> a repeated leaf (max_rep >= 1), otherwise a flat column of n_rows rows."""
    if max_rep:
        rl, dl = levels(rng, lens, max_rep, max_def)
    else:
        rl = np.zeros(n_rows, dtype=np.uint8)
        dl = np.where(rng.random(n_rows) < 0.25, rng.integers(0, max(max_def, 1), size=n_rows), max_def).astype(np.uint8)
    k = int((dl == max_def).sum())
    vals = kw.pop("vals", None)
    if vals is None:
        vals = draw(rng, t, k, kw.get("type_length", 0))
    return dict(t=t, max_rep=max_rep, max_def=max_def, rl=rl, dl=dl, vals=vals, **kw)


class Stripes:
    """Decoded device columns + the reference's stripes (rl, dl, dense values, max_def) of the same data."""

    def __init__(self, dec, specs, n_rows, page_rows=5000):
        chunks = []
        for s in specs:
            chunks.append(writer.write_column_chunk(
                s["t"], s["vals"], s.get("encoding", abi.PLAIN), def_levels=s["dl"] if s["max_def"] else None,
                rep_levels=s["rl"] if s["max_rep"] else None, max_def=s["max_def"], max_rep=s["max_rep"],
                type_length=s.get("type_length", 0), page_rows=page_rows))
        batch = writer.build_batch(chunks)
        for i, s in enumerate(specs):
            if s.get("ids"):
                batch.columns[i]["flags"] = abi.COLUMN_DICTIONARY_IDS
        self.dev, _ = dec.decode(dec.upload(batch))
        self.ref = []
        for s, d in zip(specs, self.dev):
            vals = s["vals"]
            if s.get("ids"):  # what the decode left: uint32 dictionary ids
                assert d.flags & abi.COLUMN_DICTIONARY_IDS
                vals = d.values[:4 * d.n_values].cpu().numpy().view(np.uint32).copy()
            assert d.max_rep == s["max_rep"] and d.n_slots == len(s["dl"]) and d.n_values == len(vals)
            self.ref.append((s["rl"], s["dl"], vals, s["max_def"]))
        self.n_rows = n_rows
        assert all(KR.n_records(r[0]) == n_rows for r in self.ref)


def bitmap_tensor(dec, mask, garbage_tail=False, exact=False):
    words = R.bitmap_words(np.asarray(mask, dtype=bool)).copy()
    if words.size == 0 and not exact:
        words = np.zeros(1, dtype=np.uint64)
    n = len(mask)
    if garbage_tail and n % 64:
        words[-1] |= np.uint64(0xFFFFFFFFFFFFFFFF) << np.uint64(n % 64)
    return torch.from_numpy(words.view(np.int64)).to(dec.device)


def outputs(dec, dev, n_rows, rows_capacity=None):
    cap = n_rows if rows_capacity is None else min(rows_capacity, n_rows)
    return [T_.alloc_record_output(dec.device, c, n_rows, cap, fill=POISON, slack=SLACK) for c in dev]


def dense_bytes(vals):
    if isinstance(vals, np.ndarray) and vals.dtype != object:
        return np.ascontiguousarray(vals).tobytes()
    return b"".join(bytes(v) for v in vals)


def intact(t, start):
    return bool((t.cpu().numpy()[start:] == POISON).all())


def check_outputs(dev, ref, outs, keep, counts, n_rows):
    """The outputs and the counts against take_records_ref, and the poison past them."""
    want = []
    for i, (d, o) in enumerate(zip(dev, outs)):
        if T_.is_missing(d):
            assert counts[i] == (0, 0, 0, 0) and o.values is None and o.def_levels is None and o.rep_levels is None
            want.append(None)
            continue
        (wrl, wdl, wvals), = KR.take([ref[i]], keep)
        want.append((wrl, wdl, wvals))
        ns, nv = len(wrl), len(wvals)
        if d.max_rep > 0:
            assert np.array_equal(o.rep_levels.cpu().numpy()[:ns], wrl), i
            assert intact(o.rep_levels, ns), i
        else:
            assert getattr(o, "rep_levels", None) is None
        if d.max_def > 0:
            assert np.array_equal(o.def_levels.cpu().numpy()[:ns], wdl), i
            assert intact(o.def_levels, ns), i
        raw = o.values.cpu().numpy()
        if T_.is_binary(d):
            data = b"".join(bytes(v) for v in wvals)
            assert counts[i] == (n_rows, ns, nv, len(data)), i
            offs = np.concatenate([[0], np.cumsum([len(v) for v in wvals])]).astype(np.int64)
            assert np.array_equal(raw[:8 * (nv + 1)].view(np.int64), offs), i
            assert intact(o.values, 8 * (nv + 1)), i  # no offset slot past the closing one
            assert o.binary_data.cpu().numpy()[:len(data)].tobytes() == data, i
            assert intact(o.binary_data, len(data)), i
        else:
            w = T_.elem_width(d)
            assert counts[i] == (n_rows, ns, nv, 0), i
            assert raw[:nv * w].tobytes() == dense_bytes(wvals), i
            assert intact(o.values, nv * w), i
    return want


def check(dec, data, keep, selection=None, garbage_tail=False, dev=None, ref=None):
    """One take_records into poisoned outputs, compared with the reference."""
    dev = data.dev if dev is None else dev
    ref = data.ref if ref is None else ref
    n = len(keep)
    outs = outputs(dec, dev, n)
    if selection is None:
        taken = dec.take_records(bitmap_tensor(dec, keep, garbage_tail), dev, n_rows=n, out=outs)
    else:
        taken = dec.take_records(selection, dev, out=outs)
    assert taken.n_rows == int(np.asarray(keep).sum())
    want = check_outputs(dev, ref, outs, keep, taken.counts, n)
    for c, d, w in zip(taken.columns, dev, want):
        assert c.physical_type == d.physical_type and c.max_def == d.max_def and getattr(c, "max_rep", 0) == d.max_rep
        if w is not None:
            assert c.n_values == len(w[2]) and c.n_slots == len(w[0]) and c.type_length == d.type_length and c.flags == d.flags
    return taken, outs, want


# ---- tile boundaries -------------------------------------------------------------------------------------

def small_records(rng, n_slots):
    """Record lengths 1..5 filling exactly n_slots slots."""
    lens = []
    left = n_slots
    while left:
        k = min(int(rng.integers(1, 6)), left)
        lens.append(k)
        left -= k
    return lens


def layout_long(rng):
    """Small records up to slot T exactly (a record starts at the tile boundary), one record of 2T + 5 slots
    (tile 2 holds no record start, tiles 2 and 3 begin mid-record), small records to the end: the last record
    ends in the partial tile."""
    return small_records(rng, T) + [2 * T + 5] + small_records(rng, N_SLOTS - (3 * T + 5))


def layout_ones(rng):
    """Tile 1 holds T one-slot records whose first record index is no multiple of 64, so its slots read 65
    bitmap words; small records around it, the last record ending in the partial tile."""
    head = small_records(rng, T)
    while len(head) % 64 == 0:
        head = small_records(rng, T)
    return head + [1] * T + small_records(rng, N_SLOTS - 2 * T)


LAYOUTS = {"long": layout_long, "ones": layout_ones}


@pytest.fixture(scope="module")
def tiles(decoder):
    out = {}
    for name, fn in LAYOUTS.items():
        rng = np.random.default_rng(len(name))
        lens = fn(rng)
        assert sum(lens) == N_SLOTS
        n = len(lens)
        specs = [spec(rng, abi.INT32, n, lens, 1, 2), spec(rng, abi.INT64, n, max_def=1),
                 spec(rng, abi.BYTE_ARRAY, n, lens, 1, 3)]
        out[name] = Stripes(decoder, specs, n)
    return out


def masks(n, rng):
    z = np.zeros(n, dtype=bool)
    first, last, alt = z.copy(), z.copy(), z.copy()
    first[0] = last[-1] = True
    alt[::2] = True
    return {"all": ~z, "none": z, "first": first, "last": last, "alternating": alt, "random10": rng.random(n) < 0.1,
            "random90": rng.random(n) < 0.9}


@pytest.mark.parametrize("shape", ["all", "none", "first", "last", "alternating", "random10", "random90"])
@pytest.mark.parametrize("layout", ["long", "ones"])
def test_tile_boundaries(decoder, tiles, layout, shape):
    data = tiles[layout]
    keep = masks(data.n_rows, np.random.default_rng(31))[shape]
    taken, outs, want = check(decoder, data, keep)
    if shape == "all":  # the output is the input, levels included
        for d, o in zip(data.dev, outs):
            assert torch.equal(o.def_levels[:d.n_slots], d.def_levels[:d.n_slots])
            if d.max_rep:
                assert torch.equal(o.rep_levels[:d.n_slots], d.rep_levels[:d.n_slots])


@pytest.mark.parametrize("layout", ["long", "ones"])
def test_garbage_bits_past_n_rows_are_ignored(decoder, tiles, layout):
    data = tiles[layout]
    n = data.n_rows
    assert n % 64
    keep = np.zeros(n, dtype=bool)
    keep[n - 1] = keep[n // 2] = True
    check(decoder, data, keep, garbage_tail=True)


# ---- every kind in one call ------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def kinds(decoder):
    rng = np.random.default_rng(41)
    n = T + 150

    def lens():
        return rng.integers(0, 5, size=n)
    words = rng.integers(-2**40, 2**40, size=50).astype(np.int64)
    bl = lens()
    bin_spec = spec(rng, abi.BYTE_ARRAY, n, bl, 1, 2)
    for j in range(0, len(bin_spec["vals"]), 7):
        bin_spec["vals"][j] = b""
    bin_spec["vals"][40] = bytes(rng.integers(0, 256, size=70_000, dtype=np.uint8))  # over 64 KiB
    dict_spec = spec(rng, abi.INT64, n, lens(), 1, 2, encoding=abi.RLE_DICTIONARY, ids=True)
    dict_spec["vals"] = words[rng.integers(0, 50, size=len(dict_spec["vals"]))]
    specs = [spec(rng, abi.INT32, n, lens(), 1, 2),
             spec(rng, abi.INT64, n, lens(), 2, 3),  # list<list<int64>>: repetition values 0 / 1 / 2
             spec(rng, abi.BOOLEAN, n, lens(), 1, 2),
             spec(rng, abi.INT96, n, lens(), 1, 1),
             spec(rng, abi.FIXED_LEN_BYTE_ARRAY, n, lens(), 1, 3, type_length=5),
             bin_spec, dict_spec,
             spec(rng, abi.DOUBLE, n, max_def=2),  # a flat nullable column
             spec(rng, abi.INT32, n)]              # a flat required column
    assert set(np.unique(specs[1]["rl"])) == {0, 1, 2}
    assert len({len(s["dl"]) for s in specs}) > 5  # columns of different n_slots
    data = Stripes(decoder, specs, n)
    data.dev.append(F.MissingColumn(abi.INT64, 2))  # a missing column
    data.dev[-1].max_rep = 1
    data.ref.append(None)
    return data


@pytest.mark.parametrize("staged", [1, 0])
def test_every_kind_in_one_call(decoder, kinds, staged):
    decoder.set_dispatch(abi.DISPATCH_TAKE_STAGED, staged)
    try:
        rng = np.random.default_rng(42)
        n = kinds.n_rows
        odd = rng.random(n) < 0.4
        odd[:T] = False
        odd[5] = True  # tile 0 keeps exactly one record, so the later tiles' output bases are odd
        for keep in (odd, rng.random(n) < 0.05, np.ones(n, dtype=bool)):
            taken, outs, want = check(decoder, kinds, keep)
            assert isinstance(taken.columns[-1], F.MissingColumn)
        assert taken.counts[5][3] > 70_000 and taken.columns[6].flags & abi.COLUMN_DICTIONARY_IDS
    finally:
        decoder.set_dispatch(abi.DISPATCH_TAKE_STAGED, 1)


def test_more_columns_than_one_call(decoder):
    """70 small int32 columns over device tensors, every third a list: Decoder.take_records splits them over
    two pqg_take_records calls, and an error in the second call names the column by its index in `cols`."""
    from pqgpu import decoder as D
    n = 300
    rng = np.random.default_rng(43)
    dev, ref = [], []
    for i in range(70):
        s = spec(rng, abi.INT32, n, rng.integers(0, 4, size=n), 1, 2) if i % 3 == 2 else spec(rng, abi.INT32, n, max_def=i % 3)
        to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(decoder.device)  # noqa: E731
        col = D.DeviceColumn(abi.INT32, to(s["vals"]).view(torch.uint8) if len(s["vals"]) else torch.zeros(16, dtype=torch.uint8, device=decoder.device),
                             to(s["dl"]) if s["max_def"] else None, to(s["rl"]) if s["max_rep"] else None)
        col.n_values, col.max_def, col.max_rep, col.n_slots = len(s["vals"]), s["max_def"], s["max_rep"], len(s["dl"])
        dev.append(col)
        ref.append((s["rl"], s["dl"], s["vals"], s["max_def"]))
    taken, outs, want = check(decoder, None, rng.random(n) < 0.5, dev=dev, ref=ref)
    assert len(taken.columns) == 70 and len(taken._calls) == 2
    bad = list(dev)
    bad[68] = copy.copy(dev[68])
    bad[68].n_values -= 1
    with pytest.raises(native.PqgError) as e:
        decoder.take_records(bitmap_tensor(decoder, rng.random(n) < 0.5), bad, n_rows=n).n_rows  # half kept: no capacity is short
    assert e.value.code == abi.ERR_INVALID_ARG and e.value.column == 68 and "differ from n_values" in str(e.value)


# ---- flat columns: pqg_take itself -----------------------------------------------------------------------

def test_flat_columns_equal_pqg_take(decoder, kinds, tiles):
    for dev, n in ((kinds.dev[7:9] + [F.MissingColumn(abi.INT32, 1)], kinds.n_rows), (tiles["long"].dev[1:2], tiles["long"].n_rows)):
        rng = np.random.default_rng(n)
        for keep, cap in ((rng.random(n) < 0.3, None), (rng.random(n) < 0.7, None), (rng.random(n) < 0.5, 10)):
            bm = bitmap_tensor(decoder, keep)
            a = [T_.alloc_output(decoder.device, c, n, n if cap is None else cap, fill=POISON, slack=SLACK) for c in dev]
            b = outputs(decoder, dev, n, cap)
            ta = decoder.take(bm, dev, n_rows=n, rows_capacity=cap, out=a)
            tb = decoder.take_records(bm, dev, n_rows=n, rows_capacity=cap, out=b)
            decoder.stream.synchronize()
            ra, rb = ta._state.cpu().numpy(), tb._state.cpu().numpy()
            assert ra[:16].tobytes() == rb[:16].tobytes()  # n_rows, error, error_column
            ca = ra[16:].view(np.uint64).reshape(-1, 2)
            cb = rb[16:].view(np.uint64).reshape(-1, 4)
            assert np.array_equal(ca, cb[:, 2:])
            for oa, ob in zip(a, b):
                for x, y in ((oa.values, ob.values), (oa.def_levels, ob.def_levels), (oa.binary_data, ob.binary_data)):
                    assert (x is None and y is None) or torch.equal(x, y)


# ---- composition -----------------------------------------------------------------------------------------

def test_take_of_take(decoder, kinds):
    rng = np.random.default_rng(51)
    n = kinds.n_rows
    m1 = rng.random(n) < 0.6
    taken, outs, want = check(decoder, kinds, m1)
    k = taken.n_rows
    ref1 = [None if w is None else (w[0], w[1], w[2], r[3]) for w, r in zip(want, kinds.ref)]
    m2 = rng.random(k) < 0.5
    second, outs2, want2 = check(decoder, None, m2, dev=taken.columns, ref=ref1)
    both = K.compose(m1, m2)
    for d, r, w2 in zip(kinds.dev, kinds.ref, want2):
        if r is None:
            continue
        (rl, dl, vals), = KR.take([r], both)
        assert np.array_equal(rl, w2[0]) and np.array_equal(dl, w2[1])
        assert dense_bytes(vals) == dense_bytes(w2[2])


N_ = A.Node
SCHEMA = [N_("id", A.REQUIRED), N_("xs", A.REPEATED), N_("grid", A.REPEATED, [N_("row", A.REPEATED)]),
          N_("box", A.OPTIONAL, [N_("items", A.REPEATED, [N_("v", A.OPTIONAL)])])]


def test_assemble_on_the_taken_levels(decoder):
    """Shredded records of a nested schema: a filter on the flat leaf feeds take_records with no sync in
    between, and Decoder.assemble on the taken levels gives the offsets and validity the oracle computes from
    the reference's taken stripes."""
    rng = np.random.default_rng(52)
    recs = [random_record(SCHEMA, rng) for _ in range(T + 40)]
    n = len(recs)
    chains = A.schema_leaves(SCHEMA)
    specs = []
    for chain, (rl, dl, vals) in zip(chains, shred(SCHEMA, recs)):
        max_r, max_d = A.levels_of([c.repetition for c in chain])[-1]
        specs.append(dict(t=abi.INT64, max_rep=max_r, max_def=max_d, rl=rl, dl=dl, vals=np.array(vals, dtype=np.int64)))
    data = Stripes(decoder, specs, n)
    pred = F.lt(F.col(0), 100)
    sel = decoder.filter(pred, data.dev[:1], n)
    flat_ref = [R.RefColumn(abi.INT64, specs[0]["vals"], None, 0)]
    keep = R.evaluate(pred, flat_ref, n)
    taken, outs, want = check(decoder, data, keep, selection=sel)
    assert 0 < taken.n_rows < n
    for chain, col, (rl, dl, vals) in list(zip(chains, taken.columns, want))[1:]:  # the repeated leaves
        path = [c.repetition for c in chain]
        exp = A.columnar(path, A.fsm_events(path, [c.name for c in chain], rl, dl, list(vals)))
        got = decoder.assemble(path, col.n_slots, col.def_levels, col.rep_levels)
        assert got["records"] == exp["records"] == taken.n_rows
        for k, rp in enumerate(path):
            if rp == A.OPTIONAL:
                assert got["nodes"][k]["validity"].cpu().numpy().tolist() == exp["validity"][k]
            if rp == A.REPEATED:
                assert got["nodes"][k]["offsets"].cpu().numpy().tolist() == exp["offsets"][k]


# ---- device verdicts -------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def verdicts(decoder):
    """2T + 64 records (a multiple of 64: the bitmap tensor ends at the last needed word); column 1 is the
    one the tests break."""
    rng = np.random.default_rng(61)
    n = 2 * T + 64
    specs = [spec(rng, abi.INT32, n), spec(rng, abi.INT64, n, rng.integers(0, 4, size=n), 1, 2),
             spec(rng, abi.BYTE_ARRAY, n, rng.integers(0, 3, size=n), 1, 2)]
    return Stripes(decoder, specs, n)


def expect_error(decoder, data, dev, keep, column, word, outs=None, rows_capacity=None):
    n = data.n_rows
    outs = outputs(decoder, dev, n, rows_capacity) if outs is None else outs
    taken = decoder.take_records(bitmap_tensor(decoder, keep, exact=True), dev, n_rows=n, rows_capacity=rows_capacity, out=outs)
    with pytest.raises(native.PqgError) as e:
        taken.n_rows
    assert e.value.code == abi.ERR_INVALID_ARG and e.value.column == column and word in str(e.value), str(e.value)
    assert e.value.n_rows == int(keep.sum())
    for d, o in zip(dev, outs):  # nothing past a stated capacity
        cap_s, cap_v, cap_b = T_.default_record_capacities(d, n, n if rows_capacity is None else rows_capacity)
        cap_s = cap_s if o.slots_capacity is None else o.slots_capacity
        cap_v = cap_v if o.values_capacity is None else o.values_capacity
        cap_b = cap_b if o.binary_capacity is None else o.binary_capacity
        assert intact(o.values, (cap_v + 1 if T_.is_binary(d) else cap_v) * T_.elem_width(d))
        if o.def_levels is not None:
            assert intact(o.def_levels, cap_s)
        if o.rep_levels is not None:
            assert intact(o.rep_levels, cap_s)
        if o.binary_data is not None:
            assert intact(o.binary_data, cap_b)
    return e.value


def test_slot_0_inside_a_record(decoder, verdicts):
    dev = list(verdicts.dev)
    dev[1] = copy.copy(dev[1])
    dev[1].rep_levels = dev[1].rep_levels.clone()
    dev[1].rep_levels[0] = 1
    keep = np.random.default_rng(62).random(verdicts.n_rows) < 0.5
    e = expect_error(decoder, verdicts, dev, keep, 1, "records")
    assert e.counts[1][0] == verdicts.n_rows - 1 and e.counts[0][0] == verdicts.n_rows


@pytest.mark.parametrize("delta", [-1, 1])
def test_record_starts_differ_from_n_rows(decoder, verdicts, delta):
    """One start too many: the last slots belong to record n_rows, one past the bitmap."""
    dev = list(verdicts.dev)
    rl = verdicts.ref[1][0]
    dev[1] = copy.copy(dev[1])
    dev[1].rep_levels = dev[1].rep_levels.clone()
    at = int(np.flatnonzero(rl == 0)[5]) if delta < 0 else int(np.flatnonzero(rl != 0)[5])
    dev[1].rep_levels[at] = 1 if delta < 0 else 0
    keep = np.ones(verdicts.n_rows, dtype=bool)
    e = expect_error(decoder, verdicts, dev, keep, 1, "records")
    assert e.counts[1][0] == verdicts.n_rows + delta
    kept_slots = KR.slot_mask(dev[1].rep_levels.cpu().numpy()[:dev[1].n_slots], keep).sum()
    assert e.counts[1][1] == kept_slots  # a slot of record n_rows is simply not kept


@pytest.mark.parametrize("delta", [-1, 1])
def test_wrong_n_values(decoder, verdicts, delta):
    dev = list(verdicts.dev)
    dev[2] = copy.copy(dev[2])
    dev[2].n_values += delta
    keep = np.random.default_rng(63).random(verdicts.n_rows) < 0.5
    e = expect_error(decoder, verdicts, dev, keep, 2, "differ from n_values")
    assert e.counts[2][0] == verdicts.n_rows


@pytest.mark.parametrize("which", ["records", "slots", "values", "bytes"])
def test_capacity_one_short(decoder, verdicts, which):
    keep = np.random.default_rng(64).random(verdicts.n_rows) < 0.5
    kept = int(keep.sum())
    full = []
    for r in verdicts.ref:
        (rl, dl, vals), = KR.take([r], keep)
        full.append((verdicts.n_rows, len(rl), len(vals), sum(len(v) for v in vals) if not isinstance(vals, np.ndarray) or vals.dtype == object else 0))
    rows_capacity = kept - 1 if which == "records" else None
    outs = outputs(decoder, verdicts.dev, verdicts.n_rows, rows_capacity)
    named = 0
    if which == "slots":
        outs[1].slots_capacity, named = full[1][1] - 1, 1
    elif which == "values":
        outs[1].values_capacity, named = full[1][2] - 1, 1
    elif which == "bytes":
        outs[2].binary_capacity, named = full[2][3] - 1, 2
    e = expect_error(decoder, verdicts, verdicts.dev, keep, named, "capacity", outs=outs, rows_capacity=rows_capacity)
    assert e.counts == full  # the full counts, whatever the capacities


# ---- host refusals, empty input --------------------------------------------------------------------------

def test_host_refusals(decoder):
    L = native.lib()
    dev = decoder.device
    buf = torch.zeros(8192, dtype=torch.uint8, device=dev)
    state = torch.zeros(16 + 32 * abi.TAKE_MAX_COLUMNS, dtype=torch.uint8, device=dev)  # the result, then the counts of every column
    p, counts, result = buf.data_ptr(), state.data_ptr() + 16, state.data_ptr()

    def column(rep=1, **kw):
        c = abi.TakeRecordColumn()
        c.col = abi.TakeColumn(physical_type=abi.INT64, max_def=2 if rep else 1, values=p, def_levels=p + 1024,
                               n_values=10, out_values=p + 2048, out_def_levels=p + 3072, out_values_capacity=20)
        c.max_rep = rep
        c.n_slots = 20 if rep else 10
        if rep:
            c.rep_levels, c.out_rep_levels, c.out_slots_capacity = p + 4096, p + 5120, 20
        for k, v in kw.items():
            if hasattr(c.col, k):
                setattr(c.col, k, v)
            else:
                setattr(c, k, v)
        return c

    def rc(col, n_cols=1, bitmap=p + 512, n_rows=10, counts=counts, result=result, ctx=decoder.ctx):
        arr = (abi.TakeRecordColumn * max(n_cols, 1))(*([col] * max(n_cols, 1)))
        return L.pqg_take_records(ctx, bitmap, n_rows, C.addressof(arr), n_cols, n_rows, counts, result)

    bad = abi.ERR_INVALID_ARG
    for mr in (0, 1):
        assert rc(column(mr)) == abi.OK
        assert rc(column(mr), ctx=None) == bad
        assert rc(column(mr), result=None) == bad
        assert rc(column(mr), counts=None) == bad
        assert rc(column(mr), bitmap=None) == bad
        assert rc(column(mr, max_def=255)) == bad
        assert rc(column(mr, physical_type=abi.FIXED_LEN_BYTE_ARRAY, type_length=0)) == bad
        assert rc(column(mr, values=None)) == bad
        assert rc(column(mr, out_values=None)) == bad
        assert rc(column(mr, out_def_levels=None)) == bad
        assert rc(column(mr, physical_type=abi.BYTE_ARRAY)) == bad  # no binary_data
        assert rc(column(mr, values=p + 4)) == bad  # int64 values at a 4-byte boundary
        assert rc(column(mr, reserved=1)) == bad
        assert rc(column(mr, max_rep=255)) == bad
        assert rc(column(mr, max_rep=-1)) == bad
        assert rc(column(mr, n_slots=9)) == bad  # fewer slots than records
        assert rc(column(mr), n_cols=abi.TAKE_MAX_COLUMNS) == abi.OK
        assert rc(column(mr), n_cols=abi.TAKE_MAX_COLUMNS + 1) == abi.ERR_UNSUPPORTED
        assert rc(column(mr), n_cols=-1) == bad
    assert rc(column(0, max_def=0, n_values=9)) == bad  # a required column has a value per row
    assert rc(column(0, rep_levels=p + 4096)) == bad
    assert rc(column(0, n_slots=11)) == bad
    assert rc(column(1, max_def=0, def_levels=None, out_def_levels=None)) == bad  # a repeated node adds a definition level
    assert rc(column(1, rep_levels=None)) == bad
    assert rc(column(1, out_rep_levels=None)) == bad
    assert rc(column(1, out_rep_levels=None, out_def_levels=None, out_slots_capacity=0)) == abi.OK
    assert rc(column(1, def_levels=None, rep_levels=None, n_slots=0)) == abi.OK  # a missing repeated column
    decoder.stream.synchronize()
    # the Python layer: a bare bitmap needs its row count
    with pytest.raises(native.PqgError):
        decoder.take_records(torch.zeros(1, dtype=torch.int64, device=dev), [])


def test_empty_input(decoder, tiles):
    data = tiles["long"]
    # no records: nothing is read, the counts are 0
    empty = []
    for d in data.dev:
        e = copy.copy(d)
        e.n_values, e.n_slots = 0, 0
        empty.append(e)
    outs = [T_.alloc_record_output(decoder.device, c, 0, 0, fill=POISON, slack=SLACK) for c in empty]
    taken = decoder.take_records(bitmap_tensor(decoder, np.zeros(0, dtype=bool)), empty, n_rows=0, out=outs)
    assert taken.n_rows == 0
    assert taken.counts == [(0, 0, 0, 0)] * len(empty)
    for d, o in zip(empty, outs):
        if T_.is_binary(d):
            assert o.values.cpu().numpy()[:8].view(np.int64)[0] == 0 and intact(o.values, 8)  # the closing offset
        else:
            assert intact(o.values, 0)
        assert intact(o.def_levels, 0) and (o.rep_levels is None or intact(o.rep_levels, 0))
    assert decoder.take_records(bitmap_tensor(decoder, np.ones(70, dtype=bool)), [], n_rows=70).n_rows == 70  # no columns
    # a column of 0 slots beside records is refused on the host: every record has a slot
    with pytest.raises(native.PqgError) as e:
        decoder.take_records(bitmap_tensor(decoder, np.ones(data.n_rows, dtype=bool)), [data.dev[1], empty[0]], n_rows=data.n_rows)
    assert e.value.code == abi.ERR_INVALID_ARG
