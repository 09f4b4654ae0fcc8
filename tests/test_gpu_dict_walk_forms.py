"""GPU parity of the dictionary list walk (dict_walk_ls: successor-only window pre-decode, chain,
headers parsed by the lanes that own them) on hand-built RLE / bit-packed hybrid id sections, page
bodies of helpers.make chunks replaced by bytes([w]) + runs.

The shapes are the smallest at which the walk can go wrong: a header at window offsets 0-3 and
252-255 (the last lane, whose header needs the dwords past the window), RLE values lying in the next
window, a header as the section's last byte, header lengths 1-5 for both run kinds, the value sizes
0-4 bytes, windows of 65 / 128 / 129 / 256 headers (batches of 64), packed runs below and at the
scalar shortcut (32 data bytes) ending at / crossing a window edge or cut by the section end, the
page's value count cutting a batch at its 1st / 2nd / 63rd / 64th run, sections around the size
where the walk stops being LDS-only and one of three LDS segments, and the headers that go to the
scalar path (0 groups, varints of 5 bytes and more, values / headers cut by the section end).

A page's first header is at page offset 1 (after the width byte), windows are 256 bytes from the
4-aligned position of their first header: window_offsets() restates that, and
test_shapes_reach_the_window_edges checks (without a GPU) that the cases put headers where this
text says, and that the oracle accepts every non-error case and gives the expected error code for
the others. Every GPU case is compared with the oracle as test_gpu_parity.run_both does: values,
per-page counts, first error code / page / value index.
"""
import numpy as np
import pytest

from oracle import pqref
from pqgpu import abi
from tools.synth import writer

from helpers import make
from test_gpu_parity import run_both

CARD = 5  # dictionary entries of every column here: ids 0..4
SEG_BYTES = 3072  # the walk's LDS segment; sections of at most SEG_BYTES - 264 bytes are LDS-only


def uvarint(v):
    out = bytearray()
    while True:
        b = v & 0x7F
        v >>= 7
        if v:
            out.append(b | 0x80)
        else:
            out.append(b)
            return bytes(out)


def rle(count, value, w):
    return uvarint(count << 1) + int(value).to_bytes((w + 7) // 8, "little")


def packed(groups, ids, w, cut=0):
    """A packed run of `groups` groups holding `ids` (fewer than 8 * groups: the data stops early,
    as at a section end), its last `cut` data bytes dropped."""
    bits = 0
    for i, v in enumerate(ids):
        bits |= int(v) << (i * w)
    data = bits.to_bytes((len(ids) * w + 7) // 8, "little")
    return uvarint((groups << 1) | 1) + data[:len(data) - cut]


def filler(nbytes, w, rng):
    """RLE runs (1- and 2-byte headers) of exactly nbytes bytes, and their value count."""
    nb = (w + 7) // 8
    s1, s2 = 1 + nb, 2 + nb
    for b in range(nbytes // s2 + 1):
        if (nbytes - b * s2) % s1 == 0:
            a = (nbytes - b * s2) // s1
            break
    else:
        raise AssertionError((nbytes, w))
    out, n = bytearray(), 0
    for k in rng.permutation(a + b):
        c = int(rng.integers(1, 64)) if k < a else int(rng.integers(64, 200))
        out += rle(c, int(rng.integers(0, CARD)) if w else 0, w)
        n += c
    assert len(out) == nbytes
    return bytes(out), n


def mixed(nbytes, w, rng):
    """Random RLE runs and packed runs of 1-4 groups, exactly nbytes bytes."""
    out, n = bytearray(), 0
    top = min(CARD, 1 << w)
    while nbytes - len(out) > 64 + 5 * w:
        if rng.random() < 0.6:
            c = int(rng.integers(1, 300))
            out += rle(c, int(rng.integers(0, top)), w)
            n += c
        else:
            g = int(rng.integers(1, 5))
            out += packed(g, rng.integers(0, top, size=8 * g).tolist(), w)
            n += 8 * g
    tail, nt = filler(nbytes - len(out), w, rng)
    return bytes(out) + tail, n + nt


def window_offsets(body, n):
    """Window offsets of the headers the walk takes through a pre-decoded window (not the packed
    runs of 32 data bytes and more, which it takes before any window), up to the first error."""
    w, end, pos, produced, B, offs = body[0], len(body), 1, 0, None, []
    nb = (w + 7) // 8
    while produced < n and pos < end:
        h, hl = 0, 0
        while pos + hl < end:
            b = body[pos + hl]
            h |= (b & 0x7F) << (7 * hl)
            hl += 1
            if b < 0x80:
                break
        else:  # the section ends inside the header
            offs.append(pos - (pos & ~3 if B is None or pos - B >= 256 else B))
            break
        if h & 1:
            g = h >> 1
            if g == 0 or g >= 1 << 28:
                offs.append(pos - (pos & ~3 if B is None or pos - B >= 256 else B))
                break
            nx, c = min(pos + hl + g * w, end), 8 * g
            if g * w >= 32:
                produced, pos, B = produced + c, nx, None
                continue
        else:
            nx, c = pos + hl + nb, (h >> 1) or n
        if B is None or pos - B >= 256:
            B = pos & ~3
        offs.append(pos - B)
        if nx > end:
            break
        produced, pos = produced + c, nx
        if hl > 4:
            B = None  # taken by the scalar path: the next header opens a window
    return offs


WORDS = [b"", b"a", b"bc", b"def", b"ghijklmnopqrstuvwxyz"]


def chunk(pages, ptype=abi.INT64, card=CARD, dictionary=None):
    """A dictionary column whose pages are [(body, value count)]: `card` entries 0 .. card - 1 (words
    for BYTE_ARRAY), or the entries of `dictionary` (INT32 / INT64) in the order given."""
    rows = 8  # values per page of the column that make() writes (replaced below)
    if dictionary is not None:
        card = len(dictionary)
        rows = max(8, -(-card // len(pages)))
        vals = np.resize(np.asarray(dictionary, dtype=abi.numpy_dtype(ptype)), rows * len(pages))
        assert len(set(vals[:card].tolist())) == card  # distinct, cycled: entry i gets id i
    elif ptype == abi.BYTE_ARRAY:
        vals = [WORDS[i % card] for i in range(rows * len(pages))]
    else:
        vals = (np.arange(rows * len(pages)) % card).astype(abi.numpy_dtype(ptype))
    ch = make(ptype, vals, abi.RLE_DICTIONARY, page_rows=rows)
    assert len(ch.pages) == len(pages) and ch.dict_num_values == card
    for pg, (body, n) in zip(ch.pages, pages):
        pg.body, pg.num_values, pg.num_rows = body, n, n
    ch.values = None
    ch.n_values_hint = sum(n for _, n in pages)
    return ch


# ---- the cases: name -> (pages, expected oracle code) ---------------------------------------------

def _placement(w):
    """A probe header at window offsets 252..255 (its value bytes in the next window when they do
    not fit), then runs that open the next window at offset (probe end) & 3."""
    rng = np.random.default_rng(w)
    pages = []
    for t in (252, 253, 254, 255):
        head, n = filler(t - 1, w, rng)
        tail, nt = filler(40, w, rng)
        pages.append((bytes([w]) + head + rle(3, 2, w) + tail, n + 3 + nt))
    return pages


def _header_lengths_rle():
    w = 8
    big = bytes([w]) + rle(63, 1, w) + rle(64, 2, w) + rle(8191, 3, w) + rle(8192, 4, w) + rle(5, 0, w)
    return [(big, 63 + 64 + 8191 + 8192 + 5),
            (bytes([w]) + rle(7, 1, w) + rle(1 << 20, 3, w), 3000),          # 4-byte header, capped
            (bytes([w]) + rle(7, 1, w) + rle(1 << 27, 4, w), 3000),          # 5-byte header: scalar path
            (bytes([w]) + rle(7, 1, w) + rle(0, 2, w) + rle(9, 1, w), 2500)]  # count 0: to the page end


def _header_lengths_packed():
    """w = 0: no data bytes, so runs of any group count stay below the scalar shortcut; w = 1: the
    same headers through the shortcut, the long ones cut by the section end and zero-filled."""
    pages = [(bytes([0]) + b"".join(packed(g, [], 0) for g in (63, 64, 8191, 8192)) + rle(5, 0, 0),
              8 * (63 + 64 + 8191 + 8192) + 5),
             (bytes([0]) + rle(7, 0, 0) + packed(1 << 20, [], 0), 3000),
             (bytes([0]) + rle(7, 0, 0) + packed(1 << 27, [], 0), 3000)]
    rng = np.random.default_rng(11)
    body = bytes([1]) + b"".join(packed(g, rng.integers(0, 2, size=8 * g).tolist(), 1) for g in (63, 64, 8191, 8192))
    pages.append((body, 8 * (63 + 64 + 8191 + 8192)))
    for g in (1 << 20, 1 << 27):
        pages.append((bytes([1]) + rle(7, 1, 1) + packed(g, rng.integers(0, 2, size=8 * 100).tolist(), 1), 3000))
    return pages


def _width(w):
    rng = np.random.default_rng(100 + w)
    pages = [(bytes([w]) + sec, n) for sec, n in (mixed(700, w, rng), mixed(1500, w, rng))]
    if w >= 25:  # an RLE value of 4 bytes at the last lane: bytes 253 .. 258 of the staged window
        head, n = filler(252, w, rng)
        pages.append((bytes([w]) + head + uvarint(300 << 1) + (4).to_bytes(4, "little"), n + 300))
    return pages


def _header_windows(w):
    """K consecutive RLE headers of count 1 (w = 0: 1 byte each, w = 1: 2 bytes): batches of 64."""
    pages = []
    for K in (63, 64, 65, 128, 129, 256, 600):
        ids = [(k * 7 % 2) if w else 0 for k in range(K)]
        pages.append((bytes([w]) + b"".join(rle(1, v, w) for v in ids), K))
    return pages


def _packed_w10():
    w, rng = 10, np.random.default_rng(10)
    pages = []
    for g in (1, 3, 4):
        ids = rng.integers(0, CARD, size=8 * g).tolist()
        run = packed(g, ids, w)
        tail, nt = filler(30, w, rng)
        for start in (256 - len(run), 256 - len(run) + 9):  # ends at the window edge / leaves the window
            head, n = filler(start - 1, w, rng)
            pages.append((bytes([w]) + head + run + tail, n + 8 * g + nt))
        for cut in (1, 2, w):  # the section ends before the run does: zero-filled
            head, n = filler(47, w, rng)
            pages.append((bytes([w]) + head + packed(g, ids, w, cut=cut), n + 8 * g))
    return pages


def _cap():
    """70 RLE runs of 3 values: the page's value count ends inside run 1, 2, 63, 64, 65 of the window;
    and pages of 1, 7, 8, 9 values whose first run is a packed group or an RLE run of 20."""
    w = 1
    runs = bytes([w]) + b"".join(rle(3, k & 1, w) for k in range(70))
    pages = [(runs, n) for n in (1, 3, 4, 3 * 62 + 1, 3 * 62 + 3, 3 * 63 + 2, 3 * 64, 3 * 64 + 1)]
    first = bytes([w]) + packed(1, [1, 0, 0, 1, 1, 0, 1, 0], w) + rle(20, 1, w)
    first_rle = bytes([w]) + rle(20, 1, w) + packed(1, [1, 0, 0, 1, 1, 0, 1, 0], w)
    return pages + [(b, n) for b in (first, first_rle) for n in (1, 7, 8, 9)]


def _section_lengths():
    rng = np.random.default_rng(5)
    small = SEG_BYTES - 264
    pages = []
    for size in (small - 16, small - 1, small, small + 1, small + 16, 3 * SEG_BYTES + 77):
        sec, n = mixed(size - 1, 8, rng)
        pages.append((bytes([8]) + sec, n))
    return pages


def _error(form, where):
    """[good page, bad page, good page]; the bad header at window offset 255 (first window) or 0 (a
    window opened at page offset 256)."""
    w, rng = 8, np.random.default_rng(len(form) + where)
    head, n = filler((255 if where == 255 else 256) - 1, w, rng)
    bad, more = {"groups0": (bytes([0x01]) + rle(4, 1, w), 30),
                 "varint6": (bytes([0x88, 0x80, 0x80, 0x80, 0x80, 0x00, 2]) + rle(4, 1, w), 8),
                 "value_cut": (uvarint(40 << 1), 30),
                 "header_cut": (bytes([0x88, 0x80]), 30)}[form]
    good = (bytes([w]) + filler(60, w, rng)[0], 20)
    return [good, (bytes([w]) + head + bad, n + more), good]


def _dict_id():
    """An RLE value past the dictionary, 4 bytes with the top bit set (read unmasked): DICT_ID from the
    expansion at the run's first value."""
    w, rng = 32, np.random.default_rng(32)
    head, n = filler(100, w, rng)
    return [(bytes([w]) + head + uvarint(6 << 1) + (0xFFFFFFF0).to_bytes(4, "little") + rle(3, 1, w), n + 9)]


CASES = {}
for _w in (8, 32):
    CASES[f"placement_w{_w}"] = (_placement(_w), 0)
CASES["header_lengths_rle"] = (_header_lengths_rle(), 0)
CASES["header_lengths_packed"] = (_header_lengths_packed(), 0)
for _w in (0, 1, 8, 9, 16, 17, 24, 25, 32):
    CASES[f"width_{_w}"] = (_width(_w), 0)
for _w in (0, 1):
    CASES[f"header_windows_w{_w}"] = (_header_windows(_w), 0)
CASES["packed_w10"] = (_packed_w10(), 0)
CASES["cap"] = (_cap(), 0)
CASES["section_lengths"] = (_section_lengths(), 0)
CASES["varint6_0"] = (_error("varint6", 0), 0)      # a 6-byte varint is no error to the reader:
CASES["varint6_255"] = (_error("varint6", 255), 0)  # the shift count wraps, the scalar path takes it
for _where in (0, 255):
    CASES[f"groups0_{_where}"] = (_error("groups0", _where), abi.ERR_EMPTY_PACKED_RUN)
    CASES[f"value_cut_{_where}"] = (_error("value_cut", _where), abi.ERR_EOF)
    CASES[f"header_cut_{_where}"] = (_error("header_cut", _where), abi.ERR_EOF)
CASES["dict_id"] = (_dict_id(), abi.ERR_DICT_ID)


def test_shapes_reach_the_window_edges():
    """No GPU: the oracle's verdict on every case, and where the cases put their headers."""
    seen = set()
    for name, (pages, code) in CASES.items():
        ref = pqref.decode_batch(writer.build_batch([chunk(pages)]))
        assert ref.code == code, (name, ref.status)
        for body, n in pages:
            seen.update(window_offsets(body, n))
    assert {0, 1, 2, 3, 252, 253, 254, 255} <= seen
    for name in ("groups0", "value_cut", "header_cut", "varint6"):
        for where in (0, 255):
            body, n = CASES[f"{name}_{where}"][0][1]
            assert window_offsets(body, n)[-1 if name != "varint6" else -2] == where, (name, where)
    for w, most in ((0, 256), (1, 128)):  # header_windows: a window full of headers
        offs = window_offsets(*CASES[f"header_windows_w{w}"][0][-1])
        starts = [i for i in range(len(offs)) if i == 0 or offs[i] < offs[i - 1]] + [len(offs)]
        assert most in np.diff(starts)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_dict_walk_forms(decoder, name):
    pages, code = CASES[name]
    batch, ref, _ = run_both(decoder, [chunk(pages)], expect_error=code != 0)
    assert ref.code == code, ref.status


@pytest.mark.gpu
@pytest.mark.parametrize("ptype", [abi.INT32, abi.BYTE_ARRAY])
def test_dict_walk_other_columns(decoder, ptype):
    """The walker is shared: INT32 (k_dict_fused<4>) and a BYTE_ARRAY dictionary column."""
    pages = _placement(8) + _width(9) + _header_windows(1)[2:4] + _packed_w10()[:5]
    batch, ref, _ = run_both(decoder, [chunk(pages, ptype)])
    assert ref.code == 0, ref.status
