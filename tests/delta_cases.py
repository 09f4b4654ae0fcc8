"""The named hand-built DELTA pages (delta_build.py), in groups.

Every case is checked in three places, none skipped: delta_build.read and the oracle
(tests/test_delta_build.py, the oracle also under ASan + UBSan) and the device
(tests/test_gpu_delta_pages.py).

Configurations (block size, miniblocks), named by the path delta_stream (csrc/pqgpu_kernels.hip) sends
them to. With mbs = block / mbn: `seg_big` is block <= 2048, mbn <= 8, mbs % 16 == 0 and
block * W % 16 == 0; a page with (block > 512 or mbn > 8) and not seg_big is decoded block by block
(delta_generic); of the others, mbs % 16 == 0 (and block * W % 16 == 0) takes the segment expansion
(delta_expand_seg) and the rest delta_expand<E>, E = 1, 2, 4, 8 for block <= 64, 128, 256, 512:

    delta_expand<1>   (8, 1)  (24, 3)        mbs 8: not a multiple of 16
    delta_expand<2>   (72, 3)                mbs 24
    delta_expand<4>   (200, 5)               mbs 40
    delta_expand<8>   (360, 5)               mbs 72
    segment           (16, 1) (128, 4) (2048, 8)      mbs 16, 32, 256
    block by block    (128, 16) (1032, 3) (4096, 4)   16 miniblocks; 1032 > 512 with mbs 344; 4096 > 2048
"""
import functools
from dataclasses import dataclass

import numpy as np

from pqgpu import abi
from pqgpu.batch import ColumnChunk, Page, build_batch

import delta_build as DB

CONFIGS = {
    "expand1": [(8, 1), (24, 3)],
    "expand2": [(72, 3)],
    "expand4": [(200, 5)],
    "expand8": [(360, 5)],
    "segment": [(16, 1), (128, 4), (2048, 8)],
    "generic": [(128, 16), (1032, 3), (4096, 4)],
}
ALL_CONFIGS = [c for v in CONFIGS.values() for c in v]
GROUPS = ["widths", "mixes", "fat", "last-block", "varints", "counts", "segments", "strings"]
INT_GROUPS = GROUPS[:-1]  # built once, run as INT64 and as INT32 (the reader is the same: readInteger = (int) readLong)
M64 = (1 << 64) - 1


def path_of(block, mbn, width):
    """The dispatch of delta_stream (its seg_big / E lines) for values of `width` bytes."""
    mbs = block // mbn
    seg_big = block <= 2048 and mbn <= 8 and mbs % 16 == 0 and (block * width) % 16 == 0
    if (block > 512 or mbn > 8) and not seg_big:
        return "generic"
    if mbs % 16 == 0 and (block * width) % 16 == 0:
        return "segment"
    return "expand%d" % (1 if block <= 64 else 2 if block <= 128 else 4 if block <= 256 else 8)


@dataclass
class Case:
    id: str
    group: str
    ptype: int          # abi.INT32 / abi.INT64 / abi.BYTE_ARRAY
    page: bytes         # the page's data section
    want: int           # the page's value count
    legal: bool
    expect: int = 0     # error code of the page's decode (illegal cases)
    encoding: int = abi.DELTA_BINARY_PACKED
    streams: int = 1    # DELTA streams at the page's start (DELTA_BYTE_ARRAY: 2)
    twin: str = None    # group `fat`: the minimal-width page of the same numbers
    headers: tuple = ()  # byte offsets of the block headers (group `segments`)


# ---- block makers ---------------------------------------------------------------------------------------

def rand_below(rng, w, n):
    """n random integers below 2 ** w (Python integers, w up to 64)."""
    if w == 0:
        return [0] * n
    raw = rng.integers(0, 1 << 63, size=n, dtype=np.uint64).astype(object) * 2 + rng.integers(0, 2, size=n).astype(object)
    return [int(x) >> (64 - w) for x in raw]


def rand_min_delta(rng):
    k = int(rng.integers(0, 5))
    if k == 0:
        return int(rng.integers(-5, 6))
    if k == 1:
        return int(rng.integers(-2**31, 2**31))
    if k == 2:
        return -int(rng.integers(1, 2**40))
    return int(rng.integers(-2**62, 2**62))


def make_blocks(rng, block, mbn, total, width_of, *, unused=0, padding="random", min_delta=None, delta_of=None,
                write_unused=False):
    """Blocks for a page of `total` values. width_of(b, m) -> declared width of used miniblock m of
    block b; delta_of(b, m, w, n) -> its n deltas (default: random below 2 ** w, 2 ** w - 1 among them).
    unused: the width byte of the unread miniblocks of the last block (an int, or a function of m).
    padding: "random" | "ones" for the deltas past `total` in the last used miniblock.
    write_unused: the unread miniblocks' data is written out too (their widths must be <= 64)."""
    mbs = block // mbn
    n_d = max(total - 1, 0)
    blocks = []
    for b in range((n_d + block - 1) // block):
        in_block = min(block, n_d - b * block)
        used = (in_block + mbs - 1) // mbs
        widths, deltas = [], []
        for m in range(mbn):
            if m < used:
                w = width_of(b, m)
                real = min(mbs, in_block - m * mbs)
                if delta_of is not None:
                    d = list(delta_of(b, m, w, real))
                else:
                    d = rand_below(rng, w, real)
                    if w and real:
                        d[int(rng.integers(0, real))] = (1 << w) - 1
                top = (1 << w) - 1
                d += [top] * (mbs - real) if padding == "ones" else rand_below(rng, w, mbs - real)
                widths.append(w)
                deltas.append(d)
            else:
                w = unused(m) if callable(unused) else unused
                widths.append(w)
                if write_unused:
                    deltas.append(rand_below(rng, w, mbs))
        md = min_delta if min_delta is not None else rand_min_delta(rng)
        blocks.append((md(b) if callable(md) else md, widths, deltas))
    return blocks


def page_of(rng, block, mbn, total, width_of, *, first=None, pad=None, trailing=b"", **kw):
    first = int(rng.integers(-2**62, 2**62)) if first is None else first
    return DB.build_ex(block, mbn, total, first, make_blocks(rng, block, mbn, total, width_of, **kw), pad=pad,
                       trailing=trailing)


# ---- groups -----------------------------------------------------------------------------------------------

def group_widths(add):
    """Every used width 0..64 at least once per configuration, cycled over the miniblocks of
    consecutive blocks; deltas random below 2 ** w with 2 ** w - 1 among them."""
    for k, (block, mbn) in enumerate(ALL_CONFIGS):
        rng = np.random.default_rng(100 + k)
        mbs = block // mbn
        n_mb = 67  # used miniblocks: 65 widths and two more
        seen = []

        def width_of(b, m, mbn=mbn, k=k, seen=seen):
            w = (b * mbn + m + 7 * k) % 65
            seen.append(w)
            return w
        page, _ = page_of(rng, block, mbn, 1 + n_mb * mbs - 3, width_of)
        assert set(seen) == set(range(65))
        add(f"widths-{block}-{mbn}", page, 1 + n_mb * mbs - 3)


MIXES = {"0-64-1-33": [0, 64, 1, 33], "64-0-0-64": [64, 0, 0, 64], "32-33": [32, 33, 32, 33], "33-32": [33, 32, 33, 32]}
MIX_CONFIGS = [(128, 4), (2048, 8), (16, 1), (360, 5), (128, 16), (24, 3)]


def group_mixes(add):
    rng = np.random.default_rng(200)
    for name, pat in MIXES.items():
        for block, mbn in MIX_CONFIGS:
            # the pattern over the miniblocks of a block (one-miniblock blocks: over the blocks); 6.5 blocks
            total = 1 + 6 * block + block // 2 + 3
            page, _ = page_of(rng, block, mbn, total, lambda b, m, pat=pat, mbn=mbn: pat[(m if mbn > 1 else b) % 4])
            add(f"mix-{name}-{block}-{mbn}", page, total)
    # header-only blocks, many in a row: the fast chain with dbytes == 0
    for (block, mbn), nb in [((8, 1), 150), ((128, 4), 150), ((360, 5), 70), ((2048, 8), 10), ((128, 16), 70)]:
        total = 1 + nb * block - 5
        page, _ = page_of(rng, block, mbn, total, lambda b, m: 0, min_delta=lambda b: (b % 7) - 3)
        add(f"mix-all-zero-{block}-{mbn}", page, total)
    # a zero-width miniblock as the page's very last bytes (two used of four; all four used)
    for used in (2, 4):
        total = 1 + 128 * 3 + 32 * (used - 1) + 9
        page, _ = page_of(rng, 128, 4, total, lambda b, m, used=used: 0 if (b == 3 and m == used - 1) else 5)
        add(f"mix-zero-width-last-{used}", page, total)
    # every delta 2 ** 64 - 1 with min delta 1 (each step adds 0), and sums that wrap past 2 ** 63
    for block, mbn in [(128, 4), (360, 5), (128, 16), (8, 1)]:
        total = 1 + 3 * block + 11
        page, _ = page_of(rng, block, mbn, total, lambda b, m: 64, min_delta=1, padding="ones",
                          delta_of=lambda b, m, w, n: [M64] * n, first=-77)
        add(f"mix-all-ones-{block}-{mbn}", page, total)
        page, _ = page_of(rng, block, mbn, total, lambda b, m: 62, min_delta=2**61, first=2**63 - 6)
        add(f"mix-wrap-{block}-{mbn}", page, total)
    # INT32 columns: deltas whose high 32 bits are set (low words 0: the int value does not move; random low words)
    for block, mbn in [(128, 4), (2048, 8), (72, 3), (128, 16)]:
        total = 1 + 2 * block + 40
        page, _ = page_of(rng, block, mbn, total, lambda b, m: 33 + (7 * m + b) % 32, min_delta=-(2**40) + 1,
                          delta_of=lambda b, m, w, n: [(x >> 32) << 32 for x in rand_below(rng, w, n)])
        add(f"mix-high-words-only-{block}-{mbn}", page, total)
        page, _ = page_of(rng, block, mbn, total, lambda b, m: 40 + (5 * m + b) % 25)
        add(f"mix-high-words-{block}-{mbn}", page, total)


def group_fat(add):
    """Deltas below 8 declared at widths wider than they need; `twin` names the width-3 page."""
    for block, mbn in [(128, 4), (24, 3), (2048, 8), (128, 16), (360, 5)]:
        total = 1 + 2 * block + block // 3
        nums = np.random.default_rng(300 + block).integers(0, 8, size=4 * block).tolist()
        for w in (3, 7, 8, 31, 32, 40, 64):
            it = iter(nums)
            page, _ = page_of(np.random.default_rng(0), block, mbn, total, lambda b, m, w=w: w, first=1000, min_delta=-3,
                              padding="ones", delta_of=lambda b, m, w_, n, it=it: [next(it) for _ in range(n)])
            # (the padding deltas are the width's all-ones: they differ between the twins and are never read)
            add(f"fat-{block}-{mbn}-w{w}", page, total, twin=None if w == 3 else f"fat-{block}-{mbn}-w3")


def group_last_block(add):
    """Every number of used miniblocks in the last block; total - 1 ending a miniblock exactly, one
    before it and one after it; unread miniblocks' width bytes 0, 65 and 0xFF; padding deltas all
    ones; 1, 7 and 64 trailing bytes; the unread miniblocks' data written out in full."""
    k = 0
    for block, mbn in [(128, 4), (360, 5), (2048, 8)]:
        mbs = block // mbn
        rng = np.random.default_rng(400 + block)
        for used in range(1, mbn + 1):
            for how, n_last in (("exact", used * mbs), ("before", used * mbs - 1), ("after", (used - 1) * mbs + 1)):
                fill = (0, 65, 0xFF)[k % 3]
                trailing = bytes(rng.integers(0, 256, size=(0, 1, 7, 64)[(k // 3) % 4], dtype=np.uint8))
                total = 1 + 2 * block + n_last
                page, _ = page_of(rng, block, mbn, total, lambda b, m: int(rng.integers(0, 65)), unused=fill,
                                  padding="ones", trailing=trailing)
                add(f"last-{block}-{mbn}-used{used}-{how}-fill{fill}-trail{len(trailing)}", page, total)
                k += 1
        for used in (1, mbn // 2, mbn - 1):
            total = 1 + block + (used - 1) * mbs + 5
            page, _ = page_of(rng, block, mbn, total, lambda b, m: 9 + m, unused=lambda m: 17 + m, padding="ones",
                              write_unused=True)
            add(f"last-{block}-{mbn}-used{used}-unread-data-written", page, total)


def group_varints(add, add_illegal):
    rng = np.random.default_rng(500)
    w5 = lambda b, m: 5  # noqa: E731
    for block, mbn in [(128, 4), (8, 1), (128, 16)]:
        total = 1 + 2 * block + 3
        n_blocks = 3
        for n in range(2, 6):  # over-long block size, miniblock count and total: n bytes each
            pad = {"block": n - len(DB.varint(block)), "mbn": n - 1, "total": n - len(DB.varint(total))}
            page, _ = page_of(rng, block, mbn, total, w5, pad=pad, first=3, min_delta=-2)
            add(f"var-header-{n}-bytes-{block}-{mbn}", page, total)
        for n in range(2, 11):  # over-long first value and min deltas: n bytes each (their values take 1 byte)
            page, _ = page_of(rng, block, mbn, total, w5, first=-4, min_delta=7,
                              pad={"first": n - 1, "min": {b: n - 1 for b in range(n_blocks)}})
            add(f"var-first-and-min-{n}-bytes-{block}-{mbn}", page, total)
        # min deltas that need 9 and 10 bytes, and over-long ones of 11 and 12
        page, _ = page_of(rng, block, mbn, total, w5, min_delta=lambda b: (-2**61 - 5, 2**63 - 1, -2**63)[b])
        add(f"var-min-9-10-bytes-{block}-{mbn}", page, total)
        assert [len(DB.varint(DB.zigzag64(v))) for v in (-2**61 - 5, 2**63 - 1, -2**63)] == [9, 10, 10]
        page, _ = page_of(rng, block, mbn, total, w5, min_delta=lambda b: (2**62, -9, 12345)[b],
                          pad={"min": {0: 11 - 9, 1: 12 - 1, 2: 11 - 3}})
        add(f"var-min-11-12-bytes-{block}-{mbn}", page, total)
        # 11 and 12 raw bytes whose last bytes land on masked shifts (byte 10: << 70 & 63 = 6, byte 11: << 13)
        raw = {0: b"\x80" * 10 + b"\x03", 1: b"\x82" + b"\x80" * 10 + b"\x01", 2: b"\xff" * 11 + b"\x7f"}
        page, _ = page_of(rng, block, mbn, total, w5, min_delta=0, pad={"min": raw})
        add(f"var-min-raw-masked-shifts-{block}-{mbn}", page, total)
        for name, first in (("min", -2**63), ("max", 2**63 - 1), ("minus1", -1)):
            page, _ = page_of(rng, block, mbn, total, w5, first=first)
            add(f"var-first-{name}-{block}-{mbn}", page, total)
        # a 6-byte unsigned varint: the sixth byte is shifted by 35 & 31 = 3
        t8 = (total >> 3) << 3
        page, _ = page_of(rng, block, mbn, t8, w5, pad={"total": b"\x80" * 5 + bytes([t8 >> 3])})
        add(f"var-total-6-bytes-{block}-{mbn}", page, t8)
        page, _ = page_of(rng, block, mbn, total, w5, pad={"block": 6 - len(DB.varint(block)), "mbn": 5})
        add(f"var-block-mbn-6-bytes-{block}-{mbn}", page, total)
        # a 5-byte unsigned varint whose top bits make the int negative. A count of at most -miniblock size
        # is a negative array size in allocateValuesBuffer :83-87; one in (-miniblock size, 0) rounds to no
        # miniblock, and the page reads as an empty one (the first value is still read)
        mbs = block // mbn
        for name, neg in (("min-int", b"\x80\x80\x80\x80\x08"), ("minus-256", DB.varint((1 << 32) - 256)),
                          ("minus-miniblock", DB.varint((1 << 32) - mbs))):
            page, _ = page_of(rng, block, mbn, total, w5, pad={"total": neg})
            add_illegal(f"var-total-negative-{name}-{block}-{mbn}", page, total, abi.ERR_CORRUPT)
        for name, neg in (("minus-1", b"\xff\xff\xff\xff\x0f"), ("above-minus-miniblock", DB.varint((1 << 32) - mbs + 1))):
            page, _ = page_of(rng, block, mbn, total, w5, pad={"total": neg})
            add(f"var-total-negative-{name}-reads-empty-{block}-{mbn}", page, 0)
        # a negative miniblock count: the configuration's precondition (block size a multiple of 8 x miniblocks,
        # in doubles) comes first, then new int[miniblocks] fails
        page, _ = page_of(rng, block, mbn, total, w5, pad={"mbn": DB.varint((1 << 32) - mbn)})
        add_illegal(f"var-mbn-negative-{block}-{mbn}", page, total, abi.ERR_CORRUPT)
        page, _ = page_of(rng, block, mbn, total, w5, pad={"mbn": DB.varint((1 << 32) - 3)})
        add_illegal(f"var-mbn-minus-3-{block}-{mbn}", page, total, abi.ERR_DELTA_CONFIG)
    # one slow-header block (a 9-byte min delta) at block 0, 1, 62, 63, 64, 65 of 70: where the batch is cut
    for block, mbn in [(128, 4), (8, 1)]:
        total = 1 + 70 * block - 2
        for at in (0, 1, 62, 63, 64, 65):
            page, _ = page_of(rng, block, mbn, total, lambda b, m: (3 * b + m) % 20, pad={"min": {at: 9 - 1}},
                              min_delta=lambda b: b % 50 - 9)
            add(f"var-slow-header-at-{at}-{block}-{mbn}", page, total)


WANT_CONFIGS = [(128, 4), (72, 3), (2048, 8), (128, 16)]


def group_counts(add, add_illegal):
    rng = np.random.default_rng(600)
    for block, mbn in WANT_CONFIGS + [(8, 1)]:
        for total in (0, 1, 2):  # total 0: the first value is still read
            page, _ = page_of(rng, block, mbn, total, lambda b, m: 13, unused=0xFF)
            add(f"count-total-{total}-{block}-{mbn}", page, total)
    for block, mbn in WANT_CONFIGS:
        mbs = block // mbn
        total = 1 + 3 * block + 17
        width_of = lambda b, m: 1 + (b + 3 * m) % 64  # noqa: E731
        page, offs = page_of(np.random.default_rng(601), block, mbn, total, width_of, padding="ones")
        # the same page with a width of 65 in block 2's second miniblock, and cut inside block 2's data
        bad = bytearray(page)
        hdr = offs[2]
        mlen = 1
        while page[hdr + mlen - 1] & 0x80:
            mlen += 1
        bad[hdr + mlen + 1] = 65
        cut = page[:offs[3] - 5]
        for name, want in (("0", 0), ("1", 1), ("mid", mbs + 5), ("block", block), ("block+1", 1 + block),
                           ("block+2", 2 + block)):
            add(f"count-want-{name}-of-{total}-{block}-{mbn}", page, want)
            add_illegal(f"count-want-{name}-then-width-65-{block}-{mbn}", bytes(bad), want, abi.ERR_CORRUPT)
            add_illegal(f"count-want-{name}-then-cut-{block}-{mbn}", cut, want, abi.ERR_EOF)


def group_illegal(add_illegal):
    """Used width 65 / 255 in block 0 and in a last block's used miniblock, miniblock count 0, a
    block size that is no multiple of 8 * miniblocks, first value missing, width bytes cut, data one
    byte short in the last used miniblock."""
    rng = np.random.default_rng(700)
    for block, mbn in [(128, 4), (128, 16), (360, 5), (2048, 8)]:
        mbs = block // mbn
        total = 1 + 2 * block + mbs + 3  # last block: two used miniblocks
        page, offs = page_of(rng, block, mbn, total, lambda b, m: 6, min_delta=5, unused=0xFF)
        for w in (65, 255):
            for b, m in ((0, 0), (2, 1)):
                bad = bytearray(page)
                bad[offs[b] + 1 + m] = w
                add_illegal(f"bad-width-{w}-block-{b}-{block}-{mbn}", bytes(bad), total, abi.ERR_CORRUPT)
        hdr = len(DB.varint(block)) + 1 + len(DB.varint(total))
        add_illegal(f"bad-mbn-0-{block}-{mbn}", DB.build(block, 0, total, 1, []) + page[hdr:], total, abi.ERR_DELTA_CONFIG)
        add_illegal(f"bad-block-size-{block + 8}-{mbn}", DB.varint(block + 8) + page[len(DB.varint(block)):], total,
                    abi.ERR_DELTA_CONFIG)
        add_illegal(f"bad-no-first-value-{block}-{mbn}", page[:hdr], total, abi.ERR_EOF)
        add_illegal(f"bad-widths-cut-{block}-{mbn}", page[:offs[1] + 1 + mbn - 1], total, abi.ERR_EOF)
        add_illegal(f"bad-data-one-short-{block}-{mbn}", page[:-1], total, abi.ERR_EOF)
        assert len(page) == offs[2] + 1 + mbn + 2 * 6 * mbs // 8


SEG = 8192      # DSEG: the decoder's staged segment
HDR_SPAN = 40   # bytes a block header may touch (delta_stream)


def group_segments(add, seeds=range(30)):
    """Pages of 30-60 KiB: random configuration, random width per miniblock, 0..3 bytes of varint
    padding: block headers at every position mod 4 and close before a multiple of 8 KiB."""
    for seed in seeds:
        rng = np.random.default_rng(800 + seed)
        block, mbn = ALL_CONFIGS[int(rng.integers(0, len(ALL_CONFIGS)))]
        size = int(rng.integers(34 << 10, 59 << 10))
        mbs = block // mbn
        widths, acc = [], 0  # blocks of random widths until the page has its size
        while acc < size:
            ws = [int(x) for x in rng.integers(0, 65, size=mbn)]
            n = 6 + mbn + sum(ws) * mbs // 8  # (about: the header varints vary)
            if acc + n > 60 << 10:
                if acc >= 34 << 10:
                    break
                continue
            widths.append(ws)
            acc += n
        n_blocks = len(widths)
        total = 1 + n_blocks * block - int(rng.integers(0, mbs))
        pad = {"first": int(rng.integers(0, 4)), "min": {b: int(rng.integers(0, 4)) for b in range(n_blocks)}}
        page, offs = page_of(rng, block, mbn, total, lambda b, m: widths[b][m], pad=pad)
        add(f"seg-{seed}-{block}-{mbn}", page, total, headers=tuple(offs))


def segment_coverage(cases):
    """(header offsets mod 4 seen, headers that start within HDR_SPAN bytes before a multiple of SEG)."""
    mods, edges = set(), 0
    for c in cases:
        for h in c.headers:
            mods.add(h % 4)
            edges += 0 < SEG - h % SEG <= HDR_SPAN
    return mods, edges


# ---- strings -----------------------------------------------------------------------------------------------

def int_stream(rng, block, mbn, ints, wide, unused=0xFF):
    """A DELTA stream whose values read as the given Java ints. wide: widths 33..64 with random high
    words (the long values are ints + k * 2 ** 32); else minimal-ish widths with garbage unread widths."""
    n = len(ints)
    if n == 0:
        return DB.build(block, mbn, 0, 0, [])
    lows = [(ints[i] - ints[i - 1]) & 0xFFFFFFFF for i in range(1, n)]
    if wide:
        md = int(rng.integers(-2**40, 2**40))

        def delta_of(b, m, w, cnt, st=[0]):
            out = []
            for _ in range(cnt):
                lo = (lows[st[0]] - md) & 0xFFFFFFFF
                out.append(((int(rng.integers(0, 1 << 31)) & ((1 << (w - 32)) - 1)) << 32) | lo)
                st[0] += 1
            return out
        blocks = make_blocks(rng, block, mbn, n, lambda b, m: 33 + (b + 5 * m) % 32, unused=unused, min_delta=md,
                             delta_of=delta_of)
        first = ints[0] + (int(rng.integers(0, 1 << 20)) << 32)
    else:
        sd = [DB.i32(ints[i] - ints[i - 1]) for i in range(1, n)]
        mds = [min(sd[b * block:(b + 1) * block]) for b in range((n - 1 + block - 1) // block)]
        mbs = block // mbn

        def width_of(b, m):
            seg = sd[b * block + m * mbs: b * block + (m + 1) * mbs]
            return max(x - mds[b] for x in seg).bit_length() + (b + m) % 3  # up to two bits more than needed

        def delta_of(b, m, w, cnt):
            s = b * block + m * mbs
            return [x - mds[b] for x in sd[s:s + cnt]]
        blocks = make_blocks(rng, block, mbn, n, width_of, unused=unused, min_delta=lambda b: mds[b], delta_of=delta_of)
        first = ints[0]
    return DB.build(block, mbn, n, first, blocks)


def group_strings(add, add_illegal):
    rng = np.random.default_rng(900)
    alphabet = np.frombuffer(b"abcdefghij", dtype=np.uint8)
    for k, (block, mbn) in enumerate([(128, 4), (8, 1), (128, 16), (2048, 8), (360, 5)]):
        n = 2 * block + block // 2 + 3
        unused = (0xFF, 0x2A)[k % 2]  # unread widths: one the fast header parse refuses, one it would sum
        lens = rng.integers(0, 12, size=n).tolist()
        data = alphabet[rng.integers(0, alphabet.size, size=sum(lens))].tobytes()
        # lengths at widths 33..64: (int) of each long is the small length (2 ** 32 + 3 reads as 3)
        add(f"dlba-wide-lengths-{block}-{mbn}", int_stream(rng, block, mbn, lens, wide=True, unused=unused) + data, n,
            ptype=abi.BYTE_ARRAY, encoding=abi.DELTA_LENGTH_BYTE_ARRAY)
        bad = list(lens)
        bad[block + 7] = -5  # (int) negative: in.slice(negative) at that value
        add_illegal(f"dlba-negative-length-{block}-{mbn}", int_stream(rng, block, mbn, bad, wide=True, unused=unused) + data, n,
                    abi.ERR_CORRUPT, ptype=abi.BYTE_ARRAY, encoding=abi.DELTA_LENGTH_BYTE_ARRAY)
    # DELTA_BYTE_ARRAY: prefix and suffix-length streams of different configurations, garbage unread
    # widths in both, and a prefix stream that holds more values than the suffix stream (and the page)
    # (unread widths over 64 send the last block to the scalar header walk; those of at most 64 stay on the
    # fast parse, where counting them would move the start of the next stream)
    for name, cp, cs, extra, up, us in (("8-1-then-2048-8", (8, 1), (2048, 8), 0, 0xC8, 0x41),
                                        ("128-16-then-128-4", (128, 16), (128, 4), 0, 0xC8, 0x41),
                                        ("2048-8-then-8-1", (2048, 8), (8, 1), 0, 0x11, 0x3F),
                                        ("128-4-then-360-5", (128, 4), (360, 5), 0, 0x40, 0x07),
                                        ("360-5-then-128-4", (360, 5), (128, 4), 0, 0x21, 0x40),
                                        ("longer-prefix-stream", (128, 4), (128, 16), 7, 0x3F, 0x11)):
        n = 700
        vals, prev = [], b""
        for _ in range(n):
            keep = int(rng.integers(0, len(prev) + 1))
            prev = prev[:keep] + alphabet[rng.integers(0, alphabet.size, size=int(rng.integers(0, 9)))].tobytes()
            vals.append(prev)
        prefixes, suffixes, prev = [], [], b""
        for v in vals:
            k = 0
            while k < min(len(prev), len(v)) and prev[k] == v[k]:
                k += 1
            prefixes.append(k)
            suffixes.append(v[k:])
            prev = v
        page = int_stream(rng, *cp, prefixes + [int(x) for x in rng.integers(0, 5, size=extra)], wide=False, unused=up) + \
            int_stream(rng, *cs, [len(s) for s in suffixes], wide=False, unused=us) + b"".join(suffixes)
        add(f"dba-{name}", page, n, ptype=abi.BYTE_ARRAY, encoding=abi.DELTA_BYTE_ARRAY, streams=2)


# ---- the lists -----------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _built():
    legal, illegal = [], []

    def adder(group):
        def add(cid, page, want, **kw):
            legal.append(Case(cid, group, kw.pop("ptype", None), page, want, True, **kw))

        def add_illegal(cid, page, want, expect, **kw):
            illegal.append(Case(cid, group, kw.pop("ptype", None), page, want, False, expect, **kw))
        return add, add_illegal
    group_widths(adder("widths")[0])
    group_mixes(adder("mixes")[0])
    group_fat(adder("fat")[0])
    group_last_block(adder("last-block")[0])
    group_varints(*adder("varints"))
    group_counts(*adder("counts"))
    group_illegal(adder("illegal")[1])
    group_segments(adder("segments")[0])
    group_strings(*adder("strings"))
    out_l, out_i = [], []
    for src, dst in ((legal, out_l), (illegal, out_i)):
        for c in src:
            if c.ptype is None:  # an integer page: once per type
                for t, tn in ((abi.INT64, "i64"), (abi.INT32, "i32")):
                    dst.append(Case(f"{c.id}-{tn}", c.group, t, c.page, c.want, c.legal, c.expect, c.encoding, c.streams,
                                    f"{c.twin}-{tn}" if c.twin else None, c.headers))
            else:
                dst.append(c)
    ids = [c.id for c in out_l + out_i]
    assert len(ids) == len(set(ids))
    return tuple(out_l), tuple(out_i)


def chunk_of(cases):
    """A required column whose pages are the cases' pages (one type, one encoding family)."""
    ch = ColumnChunk(physical_type=cases[0].ptype)
    for c in cases:
        assert c.ptype == ch.physical_type
        ch.pages.append(Page(body=c.page, num_values=c.want, encoding=c.encoding, num_rows=c.want))
    ch.n_values_hint = sum(c.want for c in cases)
    return ch


def batch_of(cases):
    return build_batch([chunk_of(cases)])


def legal_cases():
    return list(_built()[0])


def illegal_cases():
    return list(_built()[1])
