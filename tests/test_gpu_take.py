"""pqg_take on the GPU against tests/take_ref.py, bit for bit: per column the level bytes of the kept
rows, the dense values of the kept non-null rows, BYTE_ARRAY offsets and bytes, the counts. The inputs
are real decodes of tools.synth.writer chunks, so the dense-values + definition-levels layout is the
decoder's own. Every output is pre-filled with 0xA5 and holds a few elements more than its stated
capacity; everything past the produced counts must still be 0xA5. Row counts below a decoded column's
are prefixes of it, as in test_gpu_filter.py."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import filter_ref as R
import take_ref as K
from pqgpu import abi, native
from pqgpu import decoder as D
from pqgpu import filter as F
from pqgpu import take as T_
from test_gpu_filter import MAIN_MAX_DEF, MAIN_TYPES, Data, draw_values, random_levels
from tools.synth import writer

pytestmark = pytest.mark.gpu

T = abi.FILTER_TILE_ROWS
N_MAIN = 3 * T + 17
I32, F64, BOOL, I64, F32, BIN = range(6)
POISON = 0xA5
SLACK = 3  # elements / bytes every output holds past its stated capacity


@pytest.fixture(scope="module")
def main(decoder):
    rng = np.random.default_rng(77)
    specs = []
    for t, md in zip(MAIN_TYPES, MAIN_MAX_DEF):
        dl = random_levels(rng, N_MAIN, md, 0.2) if md else None
        k = N_MAIN if dl is None else int((dl == md).sum())
        specs.append((t, md, dl, draw_values(rng, t, k)))
    return Data(decoder, specs, N_MAIN)


def decode(dec, specs, page_rows=5000):
    """specs: dicts t, max_def, dl, vals (+ type_length, encoding, ids) -> (device columns, reference columns)."""
    chunks = []
    for s in specs:
        chunks.append(writer.write_column_chunk(s["t"], s["vals"], s.get("encoding", abi.PLAIN),
                                                def_levels=s["dl"] if s["max_def"] else None, max_def=s["max_def"],
                                                type_length=s.get("type_length", 0), page_rows=page_rows))
    batch = writer.build_batch(chunks)
    for i, s in enumerate(specs):
        if s.get("ids"):
            batch.columns[i]["flags"] = abi.COLUMN_DICTIONARY_IDS
    dev, _ = dec.decode(dec.upload(batch))
    ref = []
    for s, d in zip(specs, dev):
        vals = s["vals"]
        if s.get("ids"):  # what the decode left: uint32 dictionary ids
            assert d.flags & abi.COLUMN_DICTIONARY_IDS
            vals = d.values[:4 * d.n_values].cpu().numpy().view(np.uint32).copy()
        ref.append(R.RefColumn(s["t"], vals, s["dl"] if s["max_def"] else None, s["max_def"]))
    return dev, ref


def device_column(t, values, def_levels=None, max_def=1):
    """A DeviceColumn over existing tensors, laid out as decode() leaves it."""
    col = D.DeviceColumn(t, values.view(torch.uint8), def_levels)
    col.n_values = values.numel()
    col.max_def = 0 if def_levels is None else max_def
    return col


def bitmap_tensor(dec, mask, garbage_tail=False):
    words = R.bitmap_words(np.asarray(mask, dtype=bool)).copy()
    if words.size == 0:
        words = np.zeros(1, dtype=np.uint64)
    n = len(mask)
    if garbage_tail and n % 64:
        words[-1] |= np.uint64(0xFFFFFFFFFFFFFFFF) << np.uint64(n % 64)
    return torch.from_numpy(words.view(np.int64)).to(dec.device)


def outputs(dec, dev, n_rows, rows_capacity=None):
    cap = n_rows if rows_capacity is None else min(rows_capacity, n_rows)
    return [T_.alloc_output(dec.device, c, n_rows, cap, fill=POISON, slack=SLACK) for c in dev]


def dense_bytes(vals):
    if isinstance(vals, np.ndarray) and vals.dtype != object:
        return np.ascontiguousarray(vals).tobytes()
    return b"".join(bytes(v) for v in vals)


def intact(raw, start):
    return bool((raw[start:] == POISON).all())


def check_outputs(dev, ref, outs, keep, counts):
    """The outputs and the counts against take_ref, and the poison past them."""
    want = K.take(ref, keep)
    kept = int(np.asarray(keep, dtype=bool).sum())
    for i, (d, o, (wdl, wvals)) in enumerate(zip(dev, outs, want)):
        if T_.is_missing(d):
            assert counts[i] == (0, 0) and o.values is None and o.def_levels is None
            continue
        n_out = len(wvals)
        raw = o.values.cpu().numpy()
        if d.max_def > 0:
            lv = o.def_levels.cpu().numpy()
            assert np.array_equal(lv[:kept], wdl), i
            assert intact(lv, kept), i
        if T_.is_binary(d):
            data = b"".join(bytes(v) for v in wvals)
            assert counts[i] == (n_out, len(data)), i
            offs = np.concatenate([[0], np.cumsum([len(v) for v in wvals])]).astype(np.int64)
            assert np.array_equal(raw[:8 * (n_out + 1)].view(np.int64), offs), i
            assert intact(raw, 8 * (n_out + 1)), i  # no offset slot past the closing one
            got = o.binary_data.cpu().numpy()
            assert got[:len(data)].tobytes() == data, i
            assert intact(got, len(data)), i
        else:
            w = T_.elem_width(d)
            assert counts[i] == (n_out, 0), i
            assert raw[:n_out * w].tobytes() == dense_bytes(wvals), i
            assert intact(raw, n_out * w), i
    return want


def busy_stream(dec, passes=24):
    """A few milliseconds of work on the decoder's stream, so that calls queued right behind it are all made
    before the first of them runs. Returns the tensor it works on: keep it until the stream has been waited for."""
    x = torch.zeros(1 << 27, dtype=torch.float32, device=dec.device)
    dec.stream.wait_stream(torch.cuda.current_stream(dec.device))
    with torch.cuda.stream(dec.stream):
        for _ in range(passes):
            x.add_(1.0)
    return x


def check(dec, dev, ref, keep, selection=None, garbage_tail=False):
    """One take into poisoned outputs, compared with the reference; returns (taken, outputs, reference outcome)."""
    n = len(keep)
    outs = outputs(dec, dev, n)
    if selection is None:
        taken = dec.take(bitmap_tensor(dec, keep, garbage_tail), dev, n_rows=n, out=outs)
    else:
        taken = dec.take(selection, dev, out=outs)
    assert taken.n_rows == int(np.asarray(keep).sum())
    want = check_outputs(dev, ref, outs, keep, taken.counts)
    for c, d, (nv, _) in zip(taken.columns, dev, taken.counts):
        assert c.physical_type == d.physical_type and c.max_def == d.max_def
        if not T_.is_missing(d):
            assert c.n_values == nv and c.type_length == d.type_length and c.flags == d.flags
    return taken, outs, want


# ---- row counts ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, T - 1, T, T + 1, N_MAIN])
def test_row_counts(decoder, main, n):
    dev, ref = main.prefix(n)
    rng = np.random.default_rng(n)
    check(decoder, dev, ref, rng.random(n) < 0.3)
    # the bitmap of a real filter selection, taken without a host sync in between
    pred = F.or_(F.lt_eq(F.col(I32), 3), F.eq(F.col(I64), None))
    sel = decoder.filter(pred, dev, n)
    check(decoder, dev, ref, R.evaluate(pred, ref, n), selection=sel)


# ---- mask shapes -----------------------------------------------------------------------------------------

def mask_shapes(n, ref):
    z = np.zeros(n, dtype=bool)
    first, last, alt, tile = z.copy(), z.copy(), z.copy(), z.copy()
    first[0] = last[-1] = True
    alt[::2] = True
    tile[T:2 * T] = True
    return {"none": z, "all": ~z, "first": first, "last": last, "alternating": alt, "one_tile": tile,
            "only_null_rows": ~ref[F64].valid(n)}


@pytest.mark.parametrize("shape", ["none", "all", "first", "last", "alternating", "one_tile", "only_null_rows"])
def test_mask_shapes(decoder, main, shape):
    keep = mask_shapes(N_MAIN, main.ref)[shape]
    taken, outs, want = check(decoder, main.dev, main.ref, keep)
    if shape == "all":  # the output is the input, levels included
        for d, o in zip(main.dev, outs):
            if d.def_levels is not None:
                assert torch.equal(o.def_levels[:N_MAIN], d.def_levels[:N_MAIN])
            if not T_.is_binary(d):
                k = d.n_values * T_.elem_width(d)
                assert torch.equal(o.values[:k], d.values[:k])
    if shape == "only_null_rows":
        assert taken.counts[F64] == (0, 0) and taken.n_rows > 0


def test_garbage_bits_past_n_rows_are_ignored(decoder, main):
    for n in (65, T + 1, N_MAIN):
        dev, ref = main.prefix(n)
        keep = np.zeros(n, dtype=bool)
        keep[n - 1] = keep[n // 2] = True
        check(decoder, dev, ref, keep, garbage_tail=True)


# ---- every width -----------------------------------------------------------------------------------------

def odd_base_mask(rng, n):
    """Tile 0 keeps exactly one row, so the later tiles' output bases are odd; 40 % from there on."""
    keep = rng.random(n) < 0.4
    keep[:T] = False
    keep[5] = True
    return keep


def test_every_width(decoder):
    n = 2 * T + 70
    rng = np.random.default_rng(11)
    specs = []
    for t, tl, md in [(abi.INT96, 0, 0), (abi.INT96, 0, 2), (abi.FIXED_LEN_BYTE_ARRAY, 1, 0), (abi.FIXED_LEN_BYTE_ARRAY, 1, 1),
                      (abi.FIXED_LEN_BYTE_ARRAY, 5, 0), (abi.FIXED_LEN_BYTE_ARRAY, 5, 1),
                      (abi.FIXED_LEN_BYTE_ARRAY, 16, 0), (abi.FIXED_LEN_BYTE_ARRAY, 16, 3), (abi.BOOLEAN, 0, 0),
                      (abi.BOOLEAN, 0, 1)]:
        dl = random_levels(rng, n, md, 0.25) if md else None
        k = n if dl is None else int((dl == md).sum())
        w = abi.elem_width(t, tl)
        if t == abi.BOOLEAN:
            vals = rng.integers(0, 2, size=k).astype(np.uint8)
        else:
            vals = [rng.integers(0, 256, size=w, dtype=np.uint8).tobytes() for _ in range(k)]
        specs.append(dict(t=t, type_length=tl, max_def=md, dl=dl, vals=vals))
    dev, ref = decode(decoder, specs)
    for keep in (odd_base_mask(rng, n), rng.random(n) < 0.05, np.ones(n, dtype=bool)):
        check(decoder, dev, ref, keep)


def test_dictionary_ids(decoder):
    n = T + 300
    rng = np.random.default_rng(12)
    words = rng.integers(-2**40, 2**40, size=50).astype(np.int64)
    specs = []
    for md in (0, 1):
        dl = random_levels(rng, n, md, 0.3) if md else None
        k = n if dl is None else int((dl == md).sum())
        specs.append(dict(t=abi.INT64, max_def=md, dl=dl, vals=words[rng.integers(0, 50, size=k)], encoding=abi.RLE_DICTIONARY,
                          ids=True))
    dev, ref = decode(decoder, specs)
    taken, outs, want = check(decoder, dev, ref, odd_base_mask(rng, n))
    assert taken.counts[0][0] > 0 and all(c.flags & abi.COLUMN_DICTIONARY_IDS for c in taken.columns)


# ---- BYTE_ARRAY ------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def binary(decoder):
    n = 2 * T + 10
    rng = np.random.default_rng(13)

    def values(k):
        vals = [bytes(rng.integers(0, 256, size=int(rng.integers(0, 20)), dtype=np.uint8)) for _ in range(k)]
        for j in range(0, k, 7):
            vals[j] = b""
        vals[100] = bytes(rng.integers(0, 256, size=70_000, dtype=np.uint8))  # more than a tile's worth of staging
        return vals
    dl = random_levels(rng, n, 1, 0.2)
    dl[95:125] = 1
    specs = [dict(t=abi.BYTE_ARRAY, max_def=0, dl=None, vals=values(n)),
             dict(t=abi.BYTE_ARRAY, max_def=1, dl=dl, vals=values(int((dl == 1).sum())))]
    return decode(decoder, specs) + (n,)


def binary_masks(n):
    z = np.zeros(n, dtype=bool)
    runs, ends, long_only, around = z.copy(), z.copy(), z.copy(), z.copy()
    for a, b in ((90, 131), (T - 40, T + 40), (2 * T - 3, 2 * T + 3), (300, 301), (303, 367)):
        runs[a:b] = True
    ends[[0, T - 1, T, 2 * T - 1, 2 * T, n - 1]] = True
    long_only[95:110] = True
    around[[99, 101]] = True  # the neighbours of the long value, not the value itself
    return {"none": z, "all": ~z, "runs": runs, "tile_ends": ends, "long": long_only, "around_long": around}


@pytest.mark.parametrize("shape", ["none", "all", "runs", "tile_ends", "long", "around_long"])
def test_byte_array(decoder, binary, shape):
    dev, ref, n = binary
    keep = binary_masks(n)[shape]
    taken, outs, want = check(decoder, dev, ref, keep)
    for o, (nv, nb) in zip(outs, taken.counts):
        offs = o.values.cpu().numpy()[:8 * (nv + 1)].view(np.int64)
        assert offs[0] == 0 and offs[-1] == nb  # also when nothing is kept: the closing offset is slot 0
    if shape in ("all", "runs", "long"):
        assert taken.counts[0][1] > 70_000


# ---- missing column, scan loop, many columns -------------------------------------------------------------

def test_missing_column(decoder, main):
    dev = [F.MissingColumn(abi.BYTE_ARRAY, 2)] + list(main.dev) + [F.MissingColumn(abi.INT64, 1)]
    ref = [R.RefColumn(abi.BYTE_ARRAY, max_def=2, missing=True)] + list(main.ref) + [R.RefColumn(abi.INT64, max_def=1, missing=True)]
    rng = np.random.default_rng(14)
    taken, outs, want = check(decoder, dev, ref, rng.random(N_MAIN) < 0.5)
    assert isinstance(taken.columns[0], F.MissingColumn) and taken.columns[0].max_def == 2
    only = decoder.take(bitmap_tensor(decoder, np.ones(10, dtype=bool)), [F.MissingColumn(abi.INT32, 1)], n_rows=10)
    assert only.n_rows == 10 and only.counts == [(0, 0)]
    assert decoder.take(bitmap_tensor(decoder, np.ones(70, dtype=bool)), [], n_rows=70).n_rows == 70  # no columns: the count


def test_more_tiles_than_one_scan_round(decoder):
    """1,024 tiles + 5 rows: the cross-tile scans loop. One nullable int32 column over device tensors."""
    n = 1024 * T + 5
    rng = np.random.default_rng(15)
    dl = (rng.random(n) < 0.8).astype(np.uint8)
    vals = rng.integers(-2**31, 2**31 - 1, size=int(dl.sum()), dtype=np.int64).astype(np.int32)
    keep = rng.random(n) < 0.37
    dev = decoder.device
    col = device_column(abi.INT32, torch.from_numpy(vals).to(dev), torch.from_numpy(dl).to(dev))
    outs = outputs(decoder, [col], n)
    taken = decoder.take(bitmap_tensor(decoder, keep), [col], n_rows=n, out=outs)
    valid = dl == 1
    want = vals[(np.cumsum(valid) - valid)[keep & valid]]
    assert taken.n_rows == int(keep.sum()) and taken.counts == [(want.size, 0)]
    got = outs[0].values.cpu().numpy()
    assert np.array_equal(got[:4 * want.size].view(np.int32), want) and intact(got, 4 * want.size)
    lv = outs[0].def_levels.cpu().numpy()
    assert np.array_equal(lv[:taken.n_rows], dl[keep]) and intact(lv, taken.n_rows)


def test_more_columns_than_one_call(decoder):
    """70 small int32 columns: Decoder.take splits them over two pqg_take calls."""
    n = 300
    rng = np.random.default_rng(16)
    dev, ref = [], []
    for i in range(70):
        md = i % 3
        dl = random_levels(rng, n, md, 0.3) if md else None
        k = n if dl is None else int((dl == md).sum())
        vals = rng.integers(-1000, 1000, size=k).astype(np.int32)
        dev.append(device_column(abi.INT32, torch.from_numpy(vals).to(decoder.device),
                                 None if dl is None else torch.from_numpy(dl).to(decoder.device), md))
        ref.append(R.RefColumn(abi.INT32, vals, dl, md))
    taken, outs, want = check(decoder, dev, ref, rng.random(n) < 0.5)
    assert len(taken.columns) == 70 and len(taken._calls) == 2
    bad = list(dev)
    bad[67] = copy.copy(dev[67])
    bad[67].n_values -= 1  # an error in the second call names the column by its index in `cols`
    with pytest.raises(native.PqgError) as e:
        decoder.take(bitmap_tensor(decoder, np.ones(n, dtype=bool)), bad, n_rows=n).n_rows
    assert e.value.code == abi.ERR_INVALID_ARG and e.value.column == 67


# ---- errors ----------------------------------------------------------------------------------------------

def test_wrong_n_values(decoder, main):
    keep = np.random.default_rng(17).random(N_MAIN) < 0.5
    bm = bitmap_tensor(decoder, keep)
    for delta in (-1, 1):
        for cols_bad, named in (([I64], I64), ([BIN, F64], F64)):
            dev = list(main.dev)
            for c in cols_bad:
                dev[c] = copy.copy(main.dev[c])
                dev[c].n_values += delta
            with pytest.raises(native.PqgError) as e:
                decoder.take(bm, dev, n_rows=N_MAIN, out=outputs(decoder, dev, N_MAIN)).n_rows
            assert e.value.code == abi.ERR_INVALID_ARG and e.value.column == named
            assert "rows with a value differ from n_values" in str(e.value)


@pytest.mark.parametrize("which", ["rows", "values", "bytes"])
def test_capacity_one_short(decoder, main, which):
    keep = np.random.default_rng(18).random(N_MAIN) < 0.5
    kept = int(keep.sum())
    want = K.take(main.ref, keep)
    full = [(len(v), sum(len(x) for x in v) if main.dev[i].physical_type == abi.BYTE_ARRAY else 0) for i, (_, v) in enumerate(want)]
    outs = outputs(decoder, main.dev, N_MAIN, rows_capacity=kept - 1 if which == "rows" else None)
    rows_capacity, named = None, None
    if which == "rows":
        rows_capacity, named = kept - 1, 0
    elif which == "values":
        outs[I64].values_capacity, named = full[I64][0] - 1, I64
    else:
        outs[BIN].binary_capacity, named = full[BIN][1] - 1, BIN
    taken = decoder.take(bitmap_tensor(decoder, keep), main.dev, n_rows=N_MAIN, rows_capacity=rows_capacity, out=outs)
    with pytest.raises(native.PqgError) as e:
        taken.n_rows
    assert e.value.code == abi.ERR_INVALID_ARG and e.value.column == named and "capacity" in str(e.value)
    assert e.value.n_rows == kept and e.value.counts == full  # the full counts, whatever the capacities
    for d, o in zip(main.dev, outs):  # nothing past a stated capacity
        w = T_.elem_width(d)
        cap_v, cap_b = T_.default_capacities(d, N_MAIN, N_MAIN if rows_capacity is None else rows_capacity)
        cap_v = cap_v if o.values_capacity is None else o.values_capacity
        cap_b = cap_b if o.binary_capacity is None else o.binary_capacity
        assert intact(o.values.cpu().numpy(), (cap_v + 1 if T_.is_binary(d) else cap_v) * w)
        if o.def_levels is not None:
            assert intact(o.def_levels.cpu().numpy(), N_MAIN if rows_capacity is None else rows_capacity)
        if o.binary_data is not None:
            assert intact(o.binary_data.cpu().numpy(), cap_b)


def test_host_refusals(decoder, main):
    L = native.lib()
    dev = decoder.device
    buf = torch.zeros(4096, dtype=torch.uint8, device=dev)
    # one pqg_take_result, then a pqg_take_counts per column of the largest call below
    state = torch.zeros(C.sizeof(abi.TakeResult) + abi.TAKE_MAX_COLUMNS * C.sizeof(abi.TakeCounts), dtype=torch.uint8,
                        device=dev)
    p, counts, result = buf.data_ptr(), state.data_ptr() + C.sizeof(abi.TakeResult), state.data_ptr()

    def column(**kw):
        c = abi.TakeColumn(physical_type=abi.INT64, max_def=1, values=p, def_levels=p + 1024, n_values=10, out_values=p + 2048,
                           out_def_levels=p + 3072, out_values_capacity=10)
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    def rc(col, n_cols=1, bitmap=p + 512, n_rows=10, counts=counts, result=result, ctx=decoder.ctx):
        arr = (abi.TakeColumn * max(n_cols, 1))(*([col] * max(n_cols, 1)))
        return L.pqg_take(ctx, bitmap, n_rows, C.addressof(arr), n_cols, n_rows, counts, result)

    assert rc(column()) == abi.OK
    assert rc(column(), ctx=None) == abi.ERR_INVALID_ARG
    assert rc(column(), result=None) == abi.ERR_INVALID_ARG
    assert rc(column(), counts=None) == abi.ERR_INVALID_ARG
    assert rc(column(), bitmap=None) == abi.ERR_INVALID_ARG
    assert rc(column(), bitmap=None, n_rows=0) == abi.OK
    assert rc(column(max_def=255)) == abi.ERR_INVALID_ARG
    assert rc(column(max_def=-1)) == abi.ERR_INVALID_ARG
    assert rc(column(physical_type=abi.FIXED_LEN_BYTE_ARRAY, type_length=0)) == abi.ERR_INVALID_ARG
    assert rc(column(values=None)) == abi.ERR_INVALID_ARG
    assert rc(column(out_values=None)) == abi.ERR_INVALID_ARG
    assert rc(column(out_def_levels=None)) == abi.ERR_INVALID_ARG
    assert rc(column(physical_type=abi.BYTE_ARRAY)) == abi.ERR_INVALID_ARG  # no binary_data
    assert rc(column(values=p + 4)) == abi.ERR_INVALID_ARG  # int64 values at a 4-byte boundary
    assert rc(column(max_def=0, n_values=9)) == abi.ERR_INVALID_ARG  # a required column has a value per row
    assert rc(column(), n_cols=abi.TAKE_MAX_COLUMNS) == abi.OK
    assert rc(column(), n_cols=abi.TAKE_MAX_COLUMNS + 1) == abi.ERR_UNSUPPORTED
    assert rc(column(), n_cols=-1) == abi.ERR_INVALID_ARG
    decoder.stream.synchronize()
    # the Python layer: repeated columns as Decoder.filter refuses them, a bare bitmap needs its row count
    rep = copy.copy(main.dev[I32])
    rep.rep_levels = torch.zeros(N_MAIN, dtype=torch.uint8, device=dev)
    bm = bitmap_tensor(decoder, np.ones(N_MAIN, dtype=bool))
    with pytest.raises(native.PqgError) as e:
        decoder.take(bm, [rep], n_rows=N_MAIN)
    assert e.value.code == abi.ERR_UNSUPPORTED
    with pytest.raises(native.PqgError):
        decoder.take(bm, [main.dev[I32]])


# ---- round trip, same stream -----------------------------------------------------------------------------

def test_round_trip(decoder, main):
    """The taken columns are valid inputs: the predicate that selected them selects every one of them, and a
    take of the take is the reference's composition."""
    pred = F.and_(F.gt(F.col(I32), -5), F.not_eq(F.col(F64), 1.5))
    sel = decoder.filter(pred, main.dev, N_MAIN)
    m1 = R.evaluate(pred, main.ref, N_MAIN)
    taken, outs, want = check(decoder, main.dev, main.ref, m1, selection=sel)
    k = taken.n_rows
    assert 0 < k < N_MAIN
    again = decoder.filter(pred, taken.columns, k)
    assert again.count == k
    assert np.array_equal(again.row_ids.cpu().numpy(), np.arange(k))
    ref1 = K.as_ref_columns(main.ref, want)
    m2 = np.random.default_rng(19).random(k) < 0.5
    second, outs2, want2 = check(decoder, taken.columns, ref1, m2)
    both = K.take(main.ref, K.compose(m1, m2))
    for d, (dla, va), (dlb, vb) in zip(main.dev, want2, both):
        assert (dla is None and dlb is None) or np.array_equal(dla, dlb)
        assert K.values_equal(d.physical_type, va, vb)


def test_back_to_back_on_one_stream(decoder, main, binary):
    """Two different takes and a filter issued without synchronising: the scratch of one is not clobbered by
    the next."""
    bdev, bref, bn = binary
    rng = np.random.default_rng(20)
    k1, k2 = rng.random(N_MAIN) < 0.6, rng.random(bn) < 0.2
    pred = F.lt(F.col(I64), 2)
    o1, o2, o3 = outputs(decoder, main.dev, N_MAIN), outputs(decoder, bdev, bn), outputs(decoder, main.dev, N_MAIN)
    b1, b2 = bitmap_tensor(decoder, k1), bitmap_tensor(decoder, k2)
    torch.cuda.synchronize()
    t1 = decoder.take(b1, main.dev, n_rows=N_MAIN, out=o1)
    sel = decoder.filter(pred, main.dev, N_MAIN)
    t2 = decoder.take(b2, bdev, n_rows=bn, out=o2)
    t3 = decoder.take(sel, main.dev, out=o3)
    k3 = R.evaluate(pred, main.ref, N_MAIN)
    assert (t1.n_rows, t2.n_rows, t3.n_rows) == (int(k1.sum()), int(k2.sum()), int(k3.sum()))
    check_outputs(main.dev, main.ref, o1, k1, t1.counts)
    check_outputs(bdev, bref, o2, k2, t2.counts)
    check_outputs(main.dev, main.ref, o3, k3, t3.counts)
    assert np.array_equal(sel.row_ids.cpu().numpy(), np.flatnonzero(k3))


def test_direct_store_variant(decoder, main, binary):
    """DISPATCH_TAKE_STAGED = 0 (one store per kept lane, kept for the A/B) computes the same."""
    decoder.set_dispatch(abi.DISPATCH_TAKE_STAGED, 0)
    try:
        rng = np.random.default_rng(21)
        check(decoder, main.dev, main.ref, rng.random(N_MAIN) < 0.3)
        check(decoder, binary[0], binary[1], binary_masks(binary[2])["runs"])
    finally:
        decoder.set_dispatch(abi.DISPATCH_TAKE_STAGED, 1)


# ---- the pinned table slots ------------------------------------------------------------------------------------

def test_slot_reuse_in_queued_calls(decoder):
    """2 * TAKE_SLOTS + 1 calls queued on one context with no wait between them, each with a bitmap and output
    tensors of its own. A call's column table goes up through a pinned slot that the call TAKE_SLOTS later
    reuses: a slot overwritten before the copy out of it has run shows as a call that wrote into another
    call's outputs and left its own poisoned."""
    n, calls = 256, 9
    rng = np.random.default_rng(91)
    vals = rng.integers(-2**31, 2**31 - 1, size=n, dtype=np.int32)
    col = device_column(abi.INT32, torch.from_numpy(vals).to(decoder.device))
    ref = [R.RefColumn(abi.INT32, vals, None, 0)]
    keeps = [rng.random(n) < 0.5 for _ in range(calls)]
    assert len({k.tobytes() for k in keeps}) == calls
    bitmaps = [bitmap_tensor(decoder, k) for k in keeps]
    outs = [outputs(decoder, [col], n) for _ in range(calls)]
    held = busy_stream(decoder)
    taken = [decoder.take(b, [col], n_rows=n, out=o) for b, o in zip(bitmaps, outs)]
    for keep, o, t in zip(keeps, outs, taken):
        assert t.n_rows == int(keep.sum())
        check_outputs([col], ref, o, keep, t.counts)
    del held
