"""The hand-built Zstandard frames (zstd_build.py) that tests/test_zstd_build.py holds against the
oracle and libzstd, and tests/test_gpu_zstd_frames.py against the device decoder: constructs libzstd's
encoder never or rarely emits, at the sizes where csrc/pqgpu_zstd.hip takes another path (ZS_RING 4096,
ZS_CAP 512, ZS_SB 64, ZS_FLUSH 1024 and its 2 KiB drain, ZS_WIN 1024, ZS_HWIN 256, ZS_LIT_MAX 131072,
record room dst_size / 5, 64 stream bits per sequence in the pre-pass).

GROUPS names the legal groups (a static list: collecting tests builds no frame).
A Case is (id, group, frame, expected, n, seq_bits, libzstd): `expected` the frame's whole content
(None: the frame is illegal), `n` the size asked of the decoder (the page's uncompressed size; legal
frames decode to expected[:n]), seq_bits the most stream bits one sequence takes (0: not recorded),
libzstd False where libzstd is known to differ (each with its reason at the case)."""
import functools
from collections import namedtuple

import numpy as np

from zstd_build import (FSE, Bits, ML_BASE, ML_BITS, LL_BASE, LL_BITS, PREDEF, REPEAT, RLE, Frame, Lit, Tab, concat, ncount_bytes,
                        nseq_bytes, skippable, tree_direct)

Case = namedtuple("Case", "id group frame expected n seq_bits libzstd")
GROUPS = ("header", "literals", "tables", "codes", "repeat-offsets", "bit-budget", "nseq", "execution")
MODE_NAME = {PREDEF: "predef", RLE: "rle", FSE: "fse", REPEAT: "repeat"}


def rnd(n, seed=0, hi=256):
    return np.random.default_rng(seed).integers(0, hi, size=n, dtype=np.uint8).tobytes()


def skew(n, seed=0, top=200):
    """Bytes with a skewed histogram (Huffman-compressible), symbols 1..top."""
    return np.minimum(np.random.default_rng(seed).zipf(1.5, size=n), top).astype(np.uint8).tobytes()


def _legal():
    cases = []

    def add(group, cid, fe, n=None, seq_bits=0):
        frame, expected = fe if isinstance(fe, tuple) else fe.finish()
        cases.append(Case(cid, group, frame, expected, len(expected) if n is None else n, seq_bits, True))

    # ---- frame header
    g = "header"
    add(g, "fcs-width-0", Frame(fcs_bytes=0).raw(rnd(50)))
    add(g, "fcs-width-1", Frame(single=True, fcs_bytes=1).raw(rnd(50)))
    add(g, "fcs-width-2", Frame(single=True, fcs_bytes=2).raw(rnd(300)))
    add(g, "fcs-width-4", Frame(single=True, fcs_bytes=4).raw(rnd(50)))
    add(g, "fcs-width-8", Frame(single=True, fcs_bytes=8).raw(rnd(50)))
    add(g, "fcs-width-2-with-window", Frame(fcs_bytes=2).raw(rnd(300)))
    add(g, "fcs-255", Frame(single=True).raw(rnd(255)))
    add(g, "fcs-256", Frame(single=True).raw(rnd(256)))
    add(g, "fcs-65791", Frame(single=True).raw(rnd(65791)))
    add(g, "fcs-65792", Frame(single=True).raw(rnd(65792)))
    for w in (1, 2, 4):
        add(g, f"dictionary-id-zero-{w}-bytes", Frame(did_bytes=w, did=0).raw(rnd(40)))
    add(g, "window-descriptor-mantissa", Frame(window=(2, 5)).compressed(Lit("raw", rnd(30)), [(10, 20, 3 + 7)]))
    add(g, "window-descriptor-largest-exponent", Frame(window=(21, 7)).raw(rnd(30)))
    add(g, "checksum", Frame(checksum=True).compressed(Lit("raw", rnd(30)), [(10, 20, 3 + 7)]))
    add(g, "empty-frame", Frame().raw(b"", last=True))
    add(g, "empty-frame-single-segment", Frame(single=True).raw(b"", last=True))
    add(g, "empty-frame-then-real", concat(Frame().raw(b"").finish(), Frame().raw(rnd(33)).finish()))
    add(g, "raw-block-past-dst-size", Frame().raw(rnd(100)).raw(rnd(50, 1)), n=37)
    add(g, "rle-block-past-dst-size", Frame().raw(rnd(10)).rle(0x5A, 5000).raw(rnd(50, 1)), n=2500)
    # libzstd holds only compressed blocks against Block_Maximum_Size: an oversized raw / RLE block passes
    add(g, "raw-block-over-window-size", Frame(window=(0, 0)).raw(rnd(3000)))
    add(g, "rle-block-over-window-size", Frame(window=(0, 0)).rle(7, 3000))

    # ---- literals
    g = "literals"
    s = skew(600, 3)
    for sf in range(4):
        k = 21 if sf == 2 else 20  # (Size_Format 2 of raw / RLE literals is format 0 with an odd size)
        add(g, f"lit-raw-sf{sf}", Frame().compressed(Lit("raw", rnd(k), sf=sf), [(5, 6, 3 + 4)]))
        add(g, f"lit-rle-sf{sf}", Frame().compressed(Lit("rle", b"q" * k, sf=sf), [(5, 6, 3 + 4)]))
        add(g, f"lit-huf-sf{sf}", Frame().compressed(Lit("huf", s, sf=sf), [(5, 6, 3 + 4)]))
        add(g, f"lit-treeless-sf{sf}", Frame().compressed(Lit("huf", s)).compressed(Lit("treeless", s[100:400], sf=sf), [(5, 6, 3 + 4)]))
    for n in (0, 1, 31, 32, 4095, 4096):
        add(g, f"lit-raw-regen-{n}", Frame().raw(b"xy").compressed(Lit("raw", rnd(n, n)), [(n, 4, 3 + 2)]))
    for n in (0, 1, 31, 32, 4095, 4096, 131072 - 4):
        add(g, f"lit-rle-regen-{n}", Frame().raw(b"xy").compressed(Lit("rle", b"r" * n), [(n, 4, 3 + 2)]))
    add(g, "lit-rle-regen-131072", Frame().compressed(Lit("rle", b"r" * 131072)))
    for n in (1, 1023, 1024, 16383, 16384, 131072):
        add(g, f"lit-huf-regen-{n}", Frame().compressed(Lit("huf", skew(n, n, 30))))
    for n in (6, 7, 8, 9):
        add(g, f"lit-4-streams-{n}-bytes", Frame().compressed(Lit("huf", skew(n, n, 5), sf=1)))
    wide = bytes(np.random.default_rng(9).integers(0, 129, size=1500, dtype=np.uint8))  # 8-bit codes: 375-byte streams
    add(g, "lit-4-streams-longer-than-window", Frame().compressed(Lit("huf", wide, sf=2, weights=[1] * 128)))
    add(g, "lit-1-stream-longer-than-window", Frame().compressed(Lit("huf", wide[:900], sf=0, weights=[1] * 128)))
    add(g, "huf-direct-2-symbols", Frame().compressed(Lit("huf", rnd(100, 1, 2), weights=[1], tree="direct")))
    add(g, "huf-direct-128-weights", Frame().compressed(Lit("huf", wide[:300], weights=[1] * 128, tree="direct")))
    add(g, "huf-direct-odd-weight-count", Frame().compressed(Lit("huf", rnd(100, 2, 4), weights=[1, 1, 2], tree="direct")))
    deep = [1, 1] + list(range(2, 11))  # 12 symbols, code lengths 11, 11, 10, ..., 1
    add(g, "huf-depth-11", Frame().compressed(Lit("huf", bytes(range(12)) * 3 + rnd(200, 3, 12), weights=deep, tree="direct")))
    add(g, "huf-fse-weights-log5", Frame().compressed(Lit("huf", skew(2000, 5), tree="fse", fse_log=5)))
    add(g, "huf-fse-weights-log6", Frame().compressed(Lit("huf", skew(2000, 6), tree="fse", fse_log=6)))
    add(g, "huf-fse-weights-255", Frame().compressed(Lit("huf", rnd(3000, 7), tree="fse", fse_log=6)))
    add(g, "treeless-across-raw-literals-block",
        Frame().compressed(Lit("huf", s)).compressed(Lit("raw", rnd(9)), [(4, 5, 3 + 3)]).compressed(Lit("treeless", s[:99])))
    add(g, "treeless-across-raw-block", Frame().compressed(Lit("huf", s)).raw(rnd(9)).compressed(Lit("treeless", s[:99])))
    add(g, "treeless-across-rle-block", Frame().compressed(Lit("huf", s)).rle(3, 9).compressed(Lit("treeless", s[:99])))

    # ---- sequence tables: every mode of every table, after a block that left a table to repeat
    g = "tables"
    three = [(2, 4, 3 + 5), (2, 4, 3 + 5), (2, 4, 3 + 5)]  # one code per field: any mode can carry it
    for lm in range(4):
        for om in range(4):
            for mm in range(4):
                f = Frame().raw(rnd(8, 2)).compressed(Lit("raw", rnd(8)), three, ll=Tab(FSE), of=Tab(FSE), ml=Tab(FSE))
                f.compressed(Lit("raw", rnd(8, 1)), three, ll=Tab(lm), of=Tab(om), ml=Tab(mm))
                add(g, f"modes-ll-{MODE_NAME[lm]}-of-{MODE_NAME[om]}-ml-{MODE_NAME[mm]}", f)
    rng = np.random.default_rng(21)
    mixed = [(int(rng.integers(0, 24)), int(rng.integers(3, 30)), int(rng.integers(4, 40))) for _ in range(150)]
    mlits = rnd(sum(q[0] for q in mixed) + 7, 4)
    add(g, "fse-log-min", Frame().raw(rnd(40)).compressed(Lit("raw", mlits), mixed, ll=Tab(FSE, log=5), of=Tab(FSE, log=5), ml=Tab(FSE, log=5)))
    add(g, "fse-log-max", Frame().raw(rnd(40)).compressed(Lit("raw", mlits), mixed, ll=Tab(FSE, log=9), of=Tab(FSE, log=8), ml=Tab(FSE, log=9)))
    add(g, "fse-less-than-one-counts",
        Frame().raw(rnd(40)).compressed(Lit("raw", mlits), mixed, ll=Tab(FSE, log=6, lt1=True), of=Tab(FSE, log=6, lt1=True), ml=Tab(FSE, log=7, lt1=True)))
    gaps = [(0, 3, 4), (20, 40, 4 + 60), (0, 3, 4), (35, 3, 4), (0, 131, 2000)]  # codes far apart: zero runs of 3 and more
    add(g, "fse-zero-run-flags", Frame().raw(rnd(2100)).compressed(Lit("raw", rnd(60, 5)), gaps, ll=Tab(FSE, log=5), of=Tab(FSE, log=5), ml=Tab(FSE, log=5)))
    add(g, "fse-single-symbol-full-count",
        Frame().raw(rnd(8, 2)).compressed(Lit("raw", rnd(8)), three, ll=Tab(FSE, log=5, norm=[0, 0, 32]), of=Tab(FSE, log=5, norm=[0, 0, 0, 32]),
                           ml=Tab(FSE, log=6, norm=[0, 64])))
    rep3 = dict(ll=Tab(REPEAT), of=Tab(REPEAT), ml=Tab(REPEAT))
    add(g, "repeat-after-predefined", Frame().raw(rnd(8, 2)).compressed(Lit("raw", rnd(8)), three).compressed(Lit("raw", rnd(8, 1)), three, **rep3))
    add(g, "repeat-after-rle",
        Frame().raw(rnd(8, 2)).compressed(Lit("raw", rnd(8)), three, ll=Tab(RLE), of=Tab(RLE), ml=Tab(RLE)).compressed(Lit("raw", rnd(8, 1)), three, **rep3))
    fse3 = dict(ll=Tab(FSE, log=6), of=Tab(FSE, log=5), ml=Tab(FSE, log=7))
    add(g, "repeat-after-fse", Frame().raw(rnd(40)).compressed(Lit("raw", mlits), mixed, **fse3).compressed(Lit("raw", mlits), mixed[::-1], **rep3))
    add(g, "repeat-across-block-without-sequences",
        Frame().raw(rnd(40)).compressed(Lit("raw", mlits), mixed, **fse3).compressed(Lit("raw", rnd(5))).compressed(Lit("raw", mlits), mixed, **rep3))
    add(g, "repeat-across-raw-and-rle-blocks",
        Frame().raw(rnd(40)).compressed(Lit("raw", mlits), mixed, **fse3).raw(rnd(5)).rle(1, 9).compressed(Lit("raw", mlits), mixed, **rep3))

    # ---- code ranges: every LL / ML code with its extra bits all zero and all one (as far as a block
    # of 128 KiB allows: LL 35 and ML 52 stop at the block's size), offset codes up to the output's size
    g = "codes"
    for c in range(36):
        top = min(LL_BASE[c] + (1 << LL_BITS[c]) - 1, 131072 - 3)
        f = Frame().raw(rnd(16)).compressed(Lit("rle", b"L" * LL_BASE[c]), [(LL_BASE[c], 3, 3 + 5)])
        add(g, f"ll-code-{c}", f.compressed(Lit("rle", b"M" * top), [(top, 3, 3 + 5)]))
    for c in range(53):
        top = min(ML_BASE[c] + (1 << ML_BITS[c]) - 1, 131072 - 1)
        f = Frame().raw(rnd(16)).compressed(Lit("raw", b"a"), [(1, ML_BASE[c], 3 + 5)])
        add(g, f"ml-code-{c}", f.compressed(Lit("raw", b"b"), [(1, top, 3 + 9)]))
    f = Frame().raw(rnd(70000)).raw(rnd(70000, 1))
    ofs = []
    for c in range(2, 18):
        ofs += [(1, 5, 1 << c)] + ([(1, 5, (2 << c) - 1)] if c < 17 else [])
    add(g, "of-codes-2-to-17", f.compressed(Lit("raw", rnd(len(ofs), 2)), ofs))

    # ---- repeat offsets
    g = "repeat-offsets"
    hist = [(1, 4, 3 + 10), (1, 4, 3 + 20), (1, 4, 3 + 30)]  # leaves {30, 20, 10}
    for ofv in (1, 2, 3):
        for ll, name in ((0, "ll-0"), (2, "ll-positive")):
            # (the sequences after it read all three history slots back)
            add(g, f"offset-value-{ofv}-{name}",
                Frame().raw(rnd(64)).compressed(Lit("raw", rnd(12, ofv)), hist + [(ll, 5, ofv), (1, 4, 1), (1, 3, 3), (1, 3, 3), (1, 3, 2)]))
    add(g, "history-across-blocks",
        Frame().raw(rnd(64)).compressed(Lit("raw", rnd(3)), hist).raw(rnd(7)).compressed(Lit("raw", rnd(4, 1)), [(1, 5, 3), (0, 4, 3), (2, 6, 2), (1, 3, 1)]))
    first = Frame().raw(rnd(64)).compressed(Lit("raw", rnd(3)), hist).finish()
    second = Frame().compressed(Lit("raw", rnd(10, 8)), [(8, 3, 1), (1, 3, 2), (1, 3, 3)]).finish()  # offsets 1, 4, 8
    add(g, "history-reset-in-second-frame", concat(first, second))

    # ---- bit budget of one sequence: LL code 34 (15 bits) + ML code 52 (16 bits) + states of 9 + 9 + 8
    # bits + offset code 7 = 64 stream bits, offset code 8 = 65. (LL 35 with ML 52, 16 + 16 bits, would
    # regenerate more than a block may hold.)
    g = "bit-budget"
    for ofc, prefix in ((7, 300), (8, 600), (17, 131072)):
        lln, mln, ofn = [511] + [0] * 33 + [-1], [511] + [0] * 51 + [-1], [0, 0, 255] + [0] * (ofc - 3) + [-1]
        f = Frame()
        for k in range(0, prefix, 65536):
            f.raw(rnd(min(65536, prefix - k), k))
        f.compressed(Lit("rle", b"z" * 32769), [(32768 + 1, 65539 + 1, (1 << ofc) + 1), (0, 3, 4 + 3)],
                     ll=Tab(FSE, log=9, norm=lln), of=Tab(FSE, log=8, norm=ofn), ml=Tab(FSE, log=9, norm=mln))
        bits = f.seq_bits
        assert bits == 57 + ofc, bits
        add(g, f"sequence-of-{bits}-bits", f, seq_bits=bits)

    # ---- Number_of_Sequences: its three forms, and more sequences than the pre-pass has record room for
    g = "nseq"
    zero_bit = dict(ll=Tab(RLE), of=Tab(RLE), ml=Tab(RLE))  # a sequence costs no stream bits

    def start():  # (a miscounted sequence costs no bits either: the content size and the literals after
        return Frame(fcs_bytes=4).raw(rnd(16))  # the last sequence are what show it)

    def many(f, k, ml=3, **kw):
        return f.compressed(Lit("raw", b"\xEE\xDD"), [(0, ml, 1)] * k, **zero_bit, **kw)

    for k in (127, 128, 0x7EFF, 0x7F00, 33000):
        add(g, f"nseq-{k}", many(start(), k))
    add(g, "nseq-0-in-2-byte-form", start().compressed(Lit("raw", rnd(9)), nseq_form=2))  # libzstd: no sequences
    add(g, "nseq-5-in-2-byte-form", many(start(), 5, nseq_form=2))
    add(g, "nseq-127-in-2-byte-form", many(start(), 127, nseq_form=2))
    # 33,000 records > (16 + 99,000) / 5: the pre-pass gives the job up; in two blocks it still does
    add(g, "nseq-33000-in-two-blocks", many(many(start(), 16500), 16500))
    # with matches of 6 the same 33,000 sequences fit the room ((16 + 198,000) / 5)
    add(g, "nseq-33000-in-two-blocks-within-record-room", many(many(start(), 16500, ml=6), 16500, ml=6))

    # ---- execution
    g = "execution"
    for off in (1, 2, 3, 5, 7, 8):
        for ln in (3, 63, 64, 65, 511, 512, 513, 70000):
            add(g, f"overlap-offset-{off}-length-{ln}", Frame().raw(rnd(8, off)).compressed(Lit("raw", rnd(5, ln)), [(2, ln, 3 + off)]))
    for off in (4095, 4096, 4097, 100000):
        f = Frame().raw(rnd(off + 10, off))
        add(g, f"offset-{off}", f.compressed(Lit("raw", rnd(20, 1)), [(3, 200, 3 + off), (5, 1000, 3 + off), (1, 6000, 1), (2, 70, 3 + off - 60)]))
    for at in (512, 1024, 2048):  # the batch limit, the flush point, the drain point
        for back in (10, 5000):  # a near match (the ring) and a far one (read back from memory)
            # the block starts at a multiple of 2 KiB, so `at` is the same point counted from the
            # block's start (batches) and from the page's (flushes and drains)
            pre = rnd(2048 if back < 2048 else 6144, at)
            lead = at - 10
            add(g, f"match-straddles-{at}-offset-{back}",
                Frame().raw(pre).compressed(Lit("raw", rnd(lead + 9, 3)), [(lead, 40, 3 + back), (3, 30, 1), (1, 600, 3 + back), (2, 3, 2)]))
            add(g, f"literals-straddle-{at}-offset-{back}",
                Frame().raw(pre).compressed(Lit("raw", rnd(lead + 60, 4)), [(lead - 20, 6, 3 + back), (4, 4, 1), (50, 9, 3 + back)]))
    for total in (511, 512, 513):  # a batch of exactly / one under / one over ZS_CAP output bytes
        seqs = [(4, 12, 3 + 6)] * 31 + [(4, total - 496 - 4, 3 + 9)] + [(1, 3, 1), (2, 7, 3 + 30)] * 3
        add(g, f"batch-of-{total}-bytes", Frame().raw(rnd(40)).compressed(Lit("raw", rnd(4 * 32 + 9 + 3, total)), seqs))
    for k in (63, 64, 65, 129):
        add(g, f"batch-of-{k}-short-sequences", Frame().raw(rnd(40)).compressed(Lit("raw", rnd(k + 2, k)), [(1, 3, 3 + 1 + i % 30) for i in range(k)]))
    short = [(1, 4, 3 + 8), (2, 3, 1), (0, 5, 3 + 12)]
    for where, seqs in (("first", [(3, 600, 3 + 5)] + short * 2), ("middle", short + [(700, 3, 3 + 5), (0, 900, 3 + 2)] + short),
                        ("last", short * 2 + [(513, 513, 3 + 4000)])):
        add(g, f"long-sequence-{where}", Frame().raw(rnd(4100)).compressed(Lit("raw", rnd(sum(q[0] for q in seqs) + 4, 6)), seqs))
    # a sequence bitstream of several KiB (the decoders read it through LDS windows of 1 KiB and 512 bytes),
    # and literals consumed across the replay's 1 KiB staging windows, raw and Huffman-decoded
    rng = np.random.default_rng(33)
    busy = [(int(rng.integers(0, 300)), int(rng.integers(3, 40)), int(rng.integers(4, 60000))) for _ in range(3000)]
    blits = skew(sum(q[0] for q in busy) + 11, 8, 60)
    wide_tabs = dict(ll=Tab(FSE, log=9), of=Tab(FSE, log=8), ml=Tab(FSE, log=9))
    add(g, "bitstream-of-several-KiB-raw-literals",
        Frame().raw(rnd(60000)).compressed(Lit("raw", blits[:100000]), busy[:600], **wide_tabs))
    add(g, "bitstream-of-several-KiB-huffman-literals", Frame().raw(rnd(60000)).compressed(Lit("huf", blits[:110000]), busy[:650], **wide_tabs))
    add(g, "trailing-literals", Frame().raw(rnd(20)).compressed(Lit("raw", rnd(700, 2)), [(3, 5, 3 + 4)]))
    add(g, "no-trailing-literals", Frame().raw(rnd(20)).compressed(Lit("raw", rnd(3, 2)), [(3, 5, 3 + 4)]))
    add(g, "block-of-128-KiB", Frame().compressed(Lit("rle", b"k" * 1000), [(1000, 130072, 3 + 1)]))
    add(g, "block-of-128-KiB-after-block", Frame().raw(rnd(5000)).compressed(Lit("raw", rnd(1000, 1)), [(1000, 130072, 3 + 4500)]))
    three_frames = [Frame(checksum=bool(i & 1)).raw(rnd(30, i)).compressed(Lit("raw", rnd(12, i)), [(10, 40, 3 + 25), (0, 9, 2)]).finish()
                    for i in range(3)]
    add(g, "three-frames-and-skippable-frames", concat(three_frames[0], skippable(5, 0), three_frames[1], skippable(0, 15), three_frames[2]))
    ids = [c.id for c in cases]
    assert len(set(ids)) == len(ids)
    return cases


def _illegal():
    cases = []

    def add(cid, frame, n, libzstd=True):
        if isinstance(frame, Frame):
            frame = frame.finish()[0]
        cases.append(Case(cid, "illegal", frame, None, n, 0, libzstd))

    def block(payload, n=24, pre=b"0123456789abcdef"):
        """A frame of a raw block and one compressed block given byte for byte; n: what the frame would
        hold without its defect (the prefix + 8 Huffman literals, or + 2 literals and a match of 3), so
        that the defect alone refuses it, not a size that does not fit."""
        return Frame(check=False).raw(pre).raw_compressed(payload), n

    one = [(2, 5, 3 + 2)]
    # ---- frame level
    add("reserved-frame-header-bit", Frame(reserved=True).raw(rnd(20)), 20)
    add("dictionary-id-nonzero", Frame(did_bytes=1, did=5).raw(rnd(20)), 20)
    add("block-type-3", Frame().raw(rnd(5)).reserved_block(), 20)
    add("fcs-larger-than-content", Frame(single=True, fcs=21).raw(rnd(20)), 20)
    add("fcs-smaller-than-content", Frame(single=True, fcs=19).raw(rnd(20)), 20)
    add("fcs-larger-than-content-2-bytes", Frame(fcs_bytes=2, fcs=301).raw(rnd(300)), 300)
    # Block_Maximum_Size = min(Window_Size, 128 KiB); Window_Size of a Single_Segment frame is its content size
    add("compressed-block-over-content-size", Frame(single=True).compressed(Lit("raw", b"ab"), one), 7)
    add("compressed-block-over-window-size", Frame(window=(0, 0)).compressed(Lit("raw", rnd(1100)), [(2, 5, 3 + 2)]), 1105)
    # ---- block level
    add("modes-reserved-bits", Frame().compressed(Lit("raw", b"ab"), one, modes_reserved=1), 7)
    add("repeat-mode-without-table", Frame(check=False).compressed(Lit("raw", b"ab"), one, ll=Tab(REPEAT)), 7)
    add("repeat-mode-without-table-after-block-without-sequences",
        Frame(check=False).compressed(Lit("raw", b"ab")).compressed(Lit("raw", b"ab"), one, of=Tab(REPEAT)), 9)
    add("treeless-without-tree", Frame().compressed(Lit("treeless", rnd(40, 1, 2))), 40)
    add("treeless-without-tree-after-raw-literals", Frame().compressed(Lit("raw", rnd(9))).compressed(Lit("treeless", rnd(40, 1, 2))), 49)
    # trees and tables end with their frame
    # (the second frame is encoded with what the first one left, so only the reset at the frame's start refuses it)
    hs = skew(200, 3)
    f1, f2 = Frame().compressed(Lit("huf", hs)), Frame()
    f2.st = f1.st
    add("treeless-with-tree-of-previous-frame", f1.finish()[0] + f2.compressed(Lit("treeless", hs[:60])).finish()[0], 260)
    f1, f2 = Frame().raw(b"0123456789").compressed(Lit("raw", b"ab"), one, ll=Tab(FSE), of=Tab(FSE), ml=Tab(FSE)), Frame()
    f2.st = f1.st
    add("repeat-mode-with-table-of-previous-frame",
        f1.finish()[0] + f2.raw(b"0123456789").compressed(Lit("raw", b"ab"), one, ll=Tab(REPEAT), of=Tab(REPEAT), ml=Tab(REPEAT)).finish()[0], 34)
    add("literals-regenerate-over-128-KiB", Frame(check=False).compressed(Lit("rle", b"k" * 131073)), 131073)
    # libzstd bounds a block's output by the destination only; RFC 8878 3.1.1.2.3 by Block_Maximum_Size
    add("block-regenerates-over-128-KiB", Frame(check=False).compressed(Lit("rle", b"k" * 1000), [(1000, 130073, 3 + 1)]), 131073, libzstd=False)
    # ---- tables and trees
    for k, shift, sym in (("ll", 6, 36), ("of", 4, 32), ("ml", 2, 53)):
        add(f"rle-symbol-{k}-{sym}", *block(bytes([2 << 3]) + b"ab" + nseq_bytes(1) + bytes([RLE << shift, sym, 0x01]), n=21))
    for k, shift, log in (("ll", 6, 10), ("of", 4, 9), ("ml", 2, 10)):
        add(f"accuracy-log-{k}-{log}", *block(bytes([2 << 3]) + b"ab" + nseq_bytes(1) + bytes([FSE << shift]) + ncount_bytes([1 << log], log) + b"\x01", n=21))
    # counts that leave part of the table unassigned when the symbols run out
    add("counts-do-not-sum-to-table-size", *block(bytes([2 << 3]) + b"ab" + nseq_bytes(1) + bytes([FSE << 6]) + ncount_bytes([1] + [0] * 35, 5) + b"\x01\x01", n=21))
    huf = lambda tree, stream, regen=8: (2 | (regen << 4) | ((len(tree) + len(stream)) << 14)).to_bytes(3, "little") + tree + stream + b"\0"
    add("huffman-weights-not-power-of-two", *block(huf(tree_direct([3, 1]), b"\xff\x01")))
    add("huffman-weight-13", *block(huf(tree_direct([13, 1]), b"\xff\x01")))
    add("huffman-weight-12", *block(huf(tree_direct([12]), b"\xff\x01")))
    # two 1-bit codes in a 2-bit table: libzstd wants two symbols of weight 1 (a complete tree has them)
    onebit = Bits()
    for v in (0, 1, 1, 0, 1, 0, 0, 1):
        onebit.put(v, 1)
    add("huffman-no-symbol-of-weight-1", *block(huf(tree_direct([2]), onebit.backward())))
    for k in (3, 4, 5):  # libzstd: 4 streams hold at least 6 literals
        add(f"huffman-4-streams-{k}-bytes", Frame().compressed(Lit("huf", skew(k, 1, 3), sf=1)), k)
    s = skew(300, 3)
    add("huffman-stream-zero-last-byte", Frame().compressed(Lit("huf", s, sf=0, stream_defect="zero_last")), 300)
    add("huffman-stream-bits-left-over", Frame().compressed(Lit("huf", s, sf=0, stream_defect="leftover")), 300)
    add("huffman-stream-too-short", Frame().compressed(Lit("huf", s, sf=0, stream_defect="short")), 300)
    # libzstd checks that each of 4 streams ends at its start only in its plain loop, which it takes
    # when a stream is shorter than 8 bytes; its fast loop lets all three defects through
    tiny = skew(44, 3, 6)
    for sdef in ("zero_last", "leftover", "short"):
        add(f"huffman-4-streams-{sdef.replace('_', '-')}", Frame().compressed(Lit("huf", tiny, sf=1, stream_defect=sdef)), 44)
        add(f"huffman-4-long-streams-{sdef.replace('_', '-')}", Frame().compressed(Lit("huf", s, sf=1, stream_defect=sdef)), 300, libzstd=False)
    add("huffman-jump-table-past-section", Frame().compressed(Lit("huf", s, sf=1, jump=[60, 60, 400])), 300)
    # ---- sequences
    add("offset-zero-from-rep0-minus-1", Frame(check=False).raw(rnd(20)).compressed(Lit("raw", b""), [(0, 3, 3)]), 23)
    add("offset-past-frame-start", Frame(check=False).raw(rnd(8)).compressed(Lit("raw", b"ab"), [(2, 4, 3 + 11)]), 14)
    add("offset-into-previous-frame",
        Frame().raw(rnd(20)).finish()[0] + Frame(check=False).raw(rnd(3)).compressed(Lit("raw", b"ab"), [(2, 4, 3 + 10)]).finish()[0], 29)
    add("sequences-use-more-literals-than-block-has", Frame(check=False).raw(rnd(8)).compressed(Lit("raw", b"ab"), [(3, 4, 3 + 2)]), 15)
    three = [(2, 4, 3 + 5), (1, 40, 3 + 9), (0, 7, 2)]
    for sdef in ("leftover", "zero_last", "overrun"):
        add(f"sequence-stream-{sdef.replace('_', '-')}", Frame().raw(rnd(16)).compressed(Lit("raw", rnd(5)), three, seq_defect=sdef), 72)
    ids = [c.id for c in cases]
    assert len(set(ids)) == len(ids)
    return cases


@functools.lru_cache(maxsize=None)
def legal_cases():
    return tuple(_legal())


@functools.lru_cache(maxsize=None)
def illegal_cases():
    return tuple(_illegal())
