"""Decoder.decode_dictionaries (pqg_decode_dictionaries) and the whole row-group path on the GPU: many dictionary
pages of every physical type decoded in one call and held equal to one decode_dictionary call each; a cut-short
page among good ones named by its index; upload_chunks on chunks that carry only their dictionary page, plain and
SNAPPY-compressed; and, end to end on a synthetic file of 6 row groups: upload the dictionaries only, decode
them, filter_row_groups, upload only the kept groups' chunks, decode, filter, take, which must give what filtering
every group gives."""
import copy

import numpy as np
import pytest

from pqgpu import abi, batch, framing, native
from pqgpu import filter as F
from tools.synth import writer

pytestmark = pytest.mark.gpu

BA, FLBA, I96 = abi.BYTE_ARRAY, abi.FIXED_LEN_BYTE_ARRAY, abi.INT96
TYPES = [(abi.BOOLEAN, 0), (abi.INT32, 0), (abi.INT64, 0), (I96, 0), (abi.FLOAT, 0), (abi.DOUBLE, 0), (BA, 0), (FLBA, 5)]


def draw_entries(rng, t, tl, n):
    if t == abi.BOOLEAN:
        return (rng.integers(0, 2, size=n)).astype(np.uint8)
    if t in (abi.INT32, abi.INT64, abi.FLOAT, abi.DOUBLE):
        return rng.integers(-2**31, 2**31, size=n).astype(abi.numpy_dtype(t))
    if t == BA:
        return [bytes(rng.integers(0, 256, size=int(k), dtype=np.uint8)) for k in rng.choice([0, 1, 7, 33, 300], size=n)]
    w = abi.elem_width(t, tl)
    return [bytes(rng.integers(0, 256, size=w, dtype=np.uint8)) for _ in range(n)]


def dictionary_chunk(t, tl, entries):
    """A column chunk that carries only its dictionary page."""
    return batch.ColumnChunk(physical_type=t, type_length=tl, pages=[], dict_page=writer.plain_encode(entries, t, tl),
                             dict_num_values=len(entries), dict_encoding=abi.PLAIN)


def same(col, entries):
    got = col.numpy()
    if isinstance(entries, list):
        return [bytes(x) for x in (got if isinstance(got, list) else got.tolist())] == entries
    return np.array_equal(got.view(np.uint8), np.ascontiguousarray(entries).view(np.uint8))


@pytest.mark.parametrize("n", [1, 2, 65])
def test_decode_dictionaries_equals_single_calls(decoder, n):
    rng = np.random.default_rng(n)
    kinds = [TYPES[(k + n) % len(TYPES)] for k in range(n)]
    sizes = [int(s) for s in rng.choice([1, 63, 64, 65, 700], size=n)]
    entries = [draw_entries(rng, t, tl, s) for (t, tl), s in zip(kinds, sizes)]
    chunks = [dictionary_chunk(t, tl, e) for (t, tl), e in zip(kinds, entries)]
    dbatch = decoder.upload_chunks(chunks)  # chunks with pages == []
    assert dbatch.batch.n_pages == 0
    cols = decoder.decode_dictionaries(dbatch, range(n))
    assert len(cols) == n
    for k in range(n):
        assert cols[k].n_values == sizes[k] and cols[k].physical_type == kinds[k][0], k
        assert same(cols[k], entries[k]), (k, kinds[k])
        one = decoder.decode_dictionary(dbatch, k)
        assert one.n_values == cols[k].n_values and same(one, entries[k]), k
    # a subset, in another order
    pick = list(range(n))[::-2]
    for k, c in zip(pick, decoder.decode_dictionaries(dbatch, pick)):
        assert same(c, entries[k]), k
    assert decoder.decode_dictionaries(dbatch, []) == []


def test_a_bad_page_names_its_index(decoder):
    rng = np.random.default_rng(9)
    strings = draw_entries(rng, BA, 0, 40)
    chunks = [dictionary_chunk(abi.INT64, 0, draw_entries(rng, abi.INT64, 0, 10)), dictionary_chunk(BA, 0, strings),
              dictionary_chunk(abi.INT32, 0, draw_entries(rng, abi.INT32, 0, 5)), dictionary_chunk(BA, 0, strings)]
    chunks[3].dict_page = chunks[3].dict_page[:-3]   # its last entry reaches past the page
    with pytest.raises(native.PqgError) as e:
        decoder.decode_dictionaries(decoder.upload_chunks(chunks), range(4))
    assert e.value.status.page == 3 and e.value.code in (abi.ERR_CORRUPT, abi.ERR_EOF)
    with pytest.raises(native.PqgError) as one:      # the code is pqg_decode_dictionary's
        decoder.decode_dictionary(decoder.upload_chunks(chunks), 3)
    assert one.value.code == e.value.code
    chunks[3] = dictionary_chunk(BA, 0, strings)
    chunks[2].dict_page = chunks[2].dict_page[:-1]   # a fixed-width page shorter than its entries: refused at once
    with pytest.raises(native.PqgError) as e:
        decoder.decode_dictionaries(decoder.upload_chunks(chunks), range(4))
    assert e.value.code == abi.ERR_EOF and e.value.status.page == 2
    good = decoder.decode_dictionaries(decoder.upload_chunks(chunks), [0, 1, 3])  # the ctx decodes on after an error
    assert same(good[1], strings) and same(good[2], strings)


def test_dictionary_only_upload_with_snappy_pages(decoder):
    rng = np.random.default_rng(4)
    full, entries = [], []
    for g in range(5):
        vals = [b"word%05d" % int(v) for v in rng.integers(0, 50 + 40 * g, size=3000)]
        full.append(writer.write_column_chunk(BA, vals, abi.RLE_DICTIONARY))
        nums = rng.integers(0, 30, size=3000).astype(np.int64) * 1000
        full.append(writer.write_column_chunk(abi.INT64, nums, abi.RLE_DICTIONARY))
    packed = [writer.snappy_chunk(c) if k % 3 else c for k, c in enumerate(full)]  # compressed and plain side by side
    only = []
    for c in packed:
        d = copy.copy(c)
        d.pages = []
        only.append(d)
    assert any(c.dict_codec == writer.SNAPPY for c in only) and any(c.dict_codec == writer.UNCOMPRESSED for c in only)
    dbatch = decoder.upload_chunks(only)
    assert dbatch.batch.n_pages == 0
    got = decoder.decode_dictionaries(dbatch, range(len(only)))
    # the same dictionaries from the whole chunks, one call each
    whole = decoder.upload_chunks(packed)
    for k in range(len(only)):
        want = decoder.decode_dictionary(whole, k)
        assert got[k].n_values == want.n_values == full[k].dict_num_values > 0
        a, b = got[k].numpy(), want.numpy()
        assert (a == b) if isinstance(a, list) else np.array_equal(a, b), k


def test_end_to_end_six_row_groups(decoder):
    """Columns k (int64) and s (string), 6 row groups with dictionaries of their own; and(eq(k, 7000), in(s, ...))."""
    rng = np.random.default_rng(21)
    n_rows = 5000
    lits = [b"needle", b"pin"]
    groups = []   # per row group: ([chunk k, chunk s], k values, s values)
    for g in range(6):
        k_pool = np.arange(10, 40, dtype=np.int64) * 1000 + g
        s_pool = [b"hay%03d" % i for i in range(60)]
        if g in (1, 2, 4):
            k_pool[3] = 7000
        if g in (2, 3, 4):
            s_pool[g] = lits[g % 2]
        k = k_pool[rng.integers(0, k_pool.size, size=n_rows)]
        s = [s_pool[i] for i in rng.integers(0, len(s_pool), size=n_rows)]
        chunks = [writer.write_column_chunk(abi.INT64, k, abi.RLE_DICTIONARY), writer.write_column_chunk(BA, s, abi.RLE_DICTIONARY)]
        if g % 2:
            chunks = [writer.snappy_chunk(c) for c in chunks]
        groups.append((chunks, k, s))
    pred = F.and_(F.eq(F.col(0), 7000), F.in_(F.col(1), lits))

    def read(which):
        """decode -> filter -> take of the row groups `which`: the kept (k, s) pairs in file order."""
        out = []
        if not which:
            return out
        dbatch = decoder.upload_chunks([c for g in which for c in groups[g][0]])
        cols, _ = decoder.decode(dbatch)
        for j in range(len(which)):
            pair = cols[2 * j:2 * j + 2]
            taken = decoder.take(decoder.filter(pred, pair, n_rows), pair)
            kk, ss = taken.columns[0].numpy(), taken.columns[1].numpy()
            out += list(zip(kk.tolist(), ss))
        return out

    # 1. the dictionary pages alone
    only = []
    for chunks, _, _ in groups:
        for c in chunks:
            d = copy.copy(c)
            d.pages = []
            only.append(d)
    dicts = decoder.decode_dictionaries(decoder.upload_chunks(only), range(12))
    # 2. what the footer says of every chunk
    table = []
    for g, (chunks, _, _) in enumerate(groups):
        row = []
        for j, c in enumerate(chunks):
            stats = [(abi.DICTIONARY_PAGE, abi.PLAIN, 1), (abi.DATA_PAGE, abi.RLE_DICTIONARY, len(c.pages))]
            row.append(F.RowGroupColumn(dicts[2 * g + j], non_dictionary_pages=framing.has_non_dictionary_pages(stats, []),
                                        may_contain_null=False))
        table.append(row)
    sel = decoder.filter_row_groups(pred, table)
    kept = sel.kept.cpu().numpy().tolist()
    assert kept == [2, 4] and sel.count == 2 and sel.drop.cpu().numpy().tolist() == [True, True, False, True, False, True]
    # 3. only the kept groups are uploaded and decoded
    got = read(kept)
    want = read(list(range(6)))
    truth = [(int(a), b) for _, k, s in groups for a, b in zip(k.tolist(), s) if a == 7000 and b in lits]
    assert got == want == truth and len(truth) > 0
