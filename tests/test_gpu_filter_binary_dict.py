"""The leaves of tests/test_gpu_filter_binary.py on dictionary-id columns (pqg_filter_run_dict with a
pqg_filter_create_typed filter): FLBA, INT96 and BYTE_ARRAY dictionaries under the signed-integer, unsigned and
FLOAT16 orders. The id columns are real decodes (PQG_COLUMN_DICTIONARY_IDS) of dictionary chunks and their
dictionaries come from Decoder.decode_dictionary; dictionaries of 1, 64, 65 and 70,000 entries, the last of
which puts a leaf's verdict table past PQG_FILTER_DICT_LDS_BYTES. Every result must equal, bit for bit, both
tests/filter_binary_ref.py on dictionary[ids] and pqg_filter_run on the materialised column; an id equal to
n_entries gives PQG_ERR_DICT_ID."""
import numpy as np
import pytest
import torch

import filter_binary_ref as B
import test_gpu_filter_binary as G
from pqgpu import abi, native
from pqgpu import decoder as D
from pqgpu import filter as F
from tools.synth import writer

pytestmark = pytest.mark.gpu

N = G.N
FLBA, I96, BA = G.FLBA, G.I96, G.BA


def id_column(dec, t, width, entries, ids, dl):
    """The decoded id column of a dictionary chunk (entries in id order), with its decoded dictionary."""
    if t == BA:
        chunk = writer.write_dict_column_from_ids(BA, entries, ids, page_rows=1500, def_levels=dl, max_def=1)
    else:
        # the writer's fast path sizes fixed-width entries by the physical type alone: give it INT96 entries of
        # the right count, then put the real type, width and dictionary page in
        chunk = writer.write_dict_column_from_ids(I96, [b""] * len(entries), ids, page_rows=1500, def_levels=dl, max_def=1)
        chunk.physical_type, chunk.type_length = t, width if t == FLBA else 0
        chunk.dict_page = writer.plain_encode(entries, t, width)
    batch = writer.build_batch([chunk])
    batch.columns[0]["flags"] = abi.COLUMN_DICTIONARY_IDS
    dbatch = dec.upload(batch)
    cols, _ = dec.decode(dbatch)
    col = cols[0]
    assert col.flags & abi.COLUMN_DICTIONARY_IDS
    col.dictionary = dec.decode_dictionary(dbatch, 0)
    assert col.dictionary.n_values == len(entries) and col.dictionary.type_length == (width if t == FLBA else 0)
    return col


def draw_entries(rng, t, width, order, n):
    """n dictionary entries; every tenth is the pivot 0 and the one after it the pivot 3 (FLOAT16: +0 and -0), so
    that equality selects about a tenth of the rows whatever the dictionary's size."""
    if order == "float16":
        out = [int(G.F16_SPECIAL[p % 12] if k < 0.8 else p).to_bytes(2, "little")
               for k, p in zip(rng.random(n), rng.integers(0, 1 << 16, size=n))]
        pivots = (b"\x00\x00", b"\x00\x80")
    else:
        out = G.draw_decimal_binary(rng, n) if t == BA else G.draw_fixed(rng, width, n)
        pivots = (F.decimal_bytes(0, width), F.decimal_bytes(3, width))
    for i in range(0, n, 10):
        out[i] = pivots[0]
        if i + 1 < n:
            out[i + 1] = pivots[1]
    return out


def cases(order, width, values):
    c = F.col(0, order=order)
    if order == "signed_integer":
        return list(G.signed_cases(c, width))
    if order == "unsigned_bytes":
        return list(G.unsigned_cases(c, width, values))
    h = lambda b: int(b).to_bytes(2, "little")
    return [op(c, h(0x0000)) for op in G.CMP_OPS] + [F.eq(c, h(0x7FFF)), F.lt(c, h(0x7E00)),
                                                     F.not_in(c, [h(0x8000), h(0xFC00), h(0x7D55)]),
                                                     F.in_(c, [h(x) for x in (0, 0x3C00, 0xBC00, 0x7C00, 1, 0x8001, 0x3FF,
                                                                              0x4000, 0xC000, 0x7E00, 0xFE01, 0x5640)])]


KINDS = [(FLBA, 5, "signed_integer"), (FLBA, 16, "signed_integer"), (FLBA, 16, "unsigned_bytes"), (FLBA, 17, "signed_integer"),
         (FLBA, 3, "unsigned_bytes"), (I96, 12, "signed_integer"), (BA, 8, "signed_integer"), (FLBA, 2, "float16")]


@pytest.mark.parametrize("n_entries", [1, 64, 65, 70_000])
@pytest.mark.parametrize("t,width,order", KINDS, ids=lambda x: str(x))
def test_dictionary_ids(decoder, t, width, order, n_entries):
    rng = np.random.default_rng(n_entries + 7 * width + len(order))
    entries = draw_entries(rng, t, width, order, n_entries)
    dl = G.levels(rng, N, all_null_from=G.T)
    n_values = int(dl.sum())
    ids = np.concatenate([[n_entries - 1, 0], rng.integers(0, n_entries, size=n_values - 2)]).astype(np.int32)
    values = [entries[int(i)] for i in ids]
    col = id_column(decoder, t, width, entries, ids, dl)
    dev_values = [G.binary_column(decoder, values, dl) if t == BA else G.fixed_column(decoder, t, width, values, dl, offset=1 if t == FLBA else 0)]
    ref = [G.ref_column(t, values, dl)]
    words_past_lds = (n_entries + 63) // 64 * 8 > abi.FILTER_DICT_LDS_BYTES
    assert words_past_lds == (n_entries == 70_000)
    for pred in cases(order, width, values):
        # one entry: every row holds the same value, so a leaf is all or nothing on the valid rows
        want = G.check(decoder, pred, [col], ref, N, bounded=n_entries > 1)
        G.compare(*G.run(decoder, pred, dev_values, N), want, repr(pred))  # pqg_filter_run on the materialised column


def hand_ids(dec, dictionary, ids):
    raw = np.concatenate([np.asarray(ids, dtype=np.uint32), np.full(4, 0xA5A5A5A5, dtype=np.uint32)]).view(np.uint8)
    col = D.DeviceColumn(dictionary.physical_type, torch.from_numpy(raw.copy()).to(dec.device))
    col.n_values, col.max_def, col.flags, col.dictionary = len(ids), 0, abi.COLUMN_DICTIONARY_IDS, dictionary
    return col


@pytest.mark.parametrize("t,width,order", [(FLBA, 5, "signed_integer"), (I96, 12, "signed_integer"), (FLBA, 2, "float16")],
                         ids=lambda x: str(x))
def test_id_equal_to_n_entries(decoder, t, width, order):
    rng = np.random.default_rng(3)
    entries = draw_entries(rng, t, width, order, 65)
    dictionary = G.fixed_column(decoder, t, width, entries)
    ids = rng.integers(0, 65, size=300).astype(np.uint32)
    pred = F.lt(F.col(0, order=order), entries[0])
    good = decoder.filter(pred, [hand_ids(decoder, dictionary, ids)], 300)
    want = B.evaluate_rows(pred, [G.ref_column(t, [entries[int(i)] for i in ids])], 300)
    assert good.count == int(want.sum())
    ids[170] = 65
    with pytest.raises(native.PqgError) as e:
        decoder.filter(pred, [hand_ids(decoder, dictionary, ids)], 300).count
    assert e.value.code == abi.ERR_DICT_ID
