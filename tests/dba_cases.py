"""The named hand-built DELTA_BYTE_ARRAY pages (dba_build.py), in groups named by the part of the value
copy (csrc/pqgpu_binary.hip) they aim at. Each case is (name, prefixes, suffixes, kind) plus what its
column needs; tests/test_dba_build.py holds every one against dba_build.unroll and the oracle and
asserts from dba_build.paths that it reaches its seam; tests/test_gpu_dba_forms.py runs them on the device.

Prefix shapes, over the values of a batch (64), of a chunk (256) or over the chunk minima of a page:
    ladder_up        the prefix grows with the index: every byte has its own donor, at its own distance
    ladder_down      the prefix shrinks with the index: the low bytes all come from the unit's first
    all_inherit      prefix = the whole previous value, no suffix
    ties             long runs of one prefix, then a strictly smaller one
    random           uniform in [0, len(previous)]
    short_of_common  the prefix stops r bytes short of the common prefix; the suffix repeats those bytes
Suffix bytes are fresh random bytes (0..255) per value, except those short_of_common repeats.
"""
import functools
import random
from dataclasses import dataclass, field

import numpy as np

from pqgpu import abi
from pqgpu.batch import ColumnChunk, Page
from tools.synth import writer  # (level sections only)

import dba_build as B

SHAPES = ["ladder_up", "ladder_down", "all_inherit", "ties", "random", "short_of_common"]
GROUPS = ["batch", "tail", "chain_par", "chain_serial", "vb", "lds", "flba", "carry"]
BATCH_SIZES = [1, 2, 63, 64, 65, 127, 128, 129]
TAIL_SIZES = [255, 256, 257, 511, 512, 513]
CHAIN_PAR_CHUNKS = [2, 3, 64, 65, 128, 129, 255, 256]
CHAIN_SHAPES = ["ladder_up", "ladder_down", "all_inherit"]
CHAIN_SERIAL_VALUES = [256 * 256 + 1, 257 * 256]
VB_LENGTHS = [2047, 2048, 2049]
FLBA_WIDTHS = [1, 16, 33, 2048, 2049]
CARRY_LENGTHS = [0, 1, 2047, 2048, 2049]
ILLEGAL_AT = [0, 63, 64, 255, 256, 257]
CONFIGS = [((128, 4), (128, 4)), ((8, 1), (2048, 8)), ((360, 5), (128, 16)), ((2048, 8), (24, 3))]


@dataclass
class Case:
    name: str
    prefixes: list
    suffixes: list
    kind: str                   # "legal" | "illegal"
    group: str = ""
    ptype: int = abi.BYTE_ARRAY
    type_length: int = 0
    cfg: tuple = CONFIGS[0]
    before: tuple = None        # carry: (prefixes, suffixes) of the page before this one
    null_between: bool = False  # carry: a null-only page between the two
    cut: int = 0                # bytes dropped from the page's end
    bad: tuple = None           # illegal: (error code, value index) by construction
    _page: bytes = field(default=None, repr=False)

    @property
    def page(self):
        if self._page is None:
            pg = B.page(self.prefixes, self.suffixes, *self.cfg)
            self._page = pg[:len(pg) - self.cut] if self.cut else pg
        return self._page

    @property
    def previous(self):
        """The value before the page's first (carry cases: the last value of the page before)."""
        return B.unroll(*self.before)[-1] if self.before and self.before[0] else b""

    def values(self):
        return B.unroll(self.prefixes, self.suffixes, self.previous)

    def lengths(self):
        return [len(v) for v in self.values()]


# ---- value sequences ----------------------------------------------------------------------------------

class Seq:
    def __init__(self, seed, previous=b""):
        self.rnd = random.Random(seed)
        self.prev, self.P, self.S = previous, [], []

    def add(self, p, s, repeat=0):
        """A value of prefix min(p, len(previous)) (None: all of it) whose suffix is `repeat` bytes
        that repeat the previous value's next bytes, then s fresh random bytes."""
        lp = len(self.prev)
        p = lp if p is None else min(p, lp)
        suf = self.prev[p:p + repeat] + (self.rnd.randbytes(s) if s else b"")
        self.P.append(p)
        self.S.append(suf)
        self.prev = self.prev[:p] + suf if p else suf

    def small(self, n):
        """n short values (prefix at most 6, 1..4 fresh bytes)."""
        for _ in range(n):
            self.add(self.rnd.randint(0, 6), self.rnd.randint(1, 4))


def fill(seq, n, shape, span, num=1, den=1, empties=()):
    """n values of the shape, the shape's index running over spans of `span` values; ladder steps are
    num / den of a byte per value; `empties`: indices that hold an empty value (prefix 0, no suffix)."""
    r = seq.rnd
    top = span * num // den
    q, run = 20, 0
    for i in range(n):
        if i in empties:
            seq.add(0, 0)
            continue
        j, lp = i % span, len(seq.prev)
        if shape == "ladder_up":
            seq.add(j * num // den, r.randint(1, 3) + (num // den if num > den else 0))
        elif shape == "ladder_down":
            p = (span - j) * num // den
            seq.add(p, (max(top - min(p, lp), 0) if j == 0 else 0) + r.randint(0, 2))
        elif shape == "all_inherit":
            seq.add(None, 0) if i else seq.add(0, 40)
        elif shape == "ties":
            if run == 0:
                q = q - r.randint(1, 3) if q - 3 >= 0 else 20
                run = r.randint(3, 70)
            run -= 1
            seq.add(q, max(20 - min(q, lp), 0) + r.randint(1, 3))
        elif shape == "random":
            seq.add(r.randint(0, lp), r.randint(0, 8))
        elif shape == "short_of_common":
            c = max(lp - r.randint(0, 4), 0)
            rep = min(r.randint(1, 3), c)
            seq.add(c - rep, r.randint(0, 6) if lp < 48 else 0, repeat=rep)
        else:
            raise ValueError(shape)


def chain_page(seed, n, shape, vlen=64):
    """n values of vlen bytes whose chunk minima follow the shape: one value per chunk (anywhere in
    it) takes the chunk's minimum prefix k_c and vlen - k_c fresh bytes; every other value inherits
    all but 0..3 bytes."""
    seq = Seq(seed)
    r = seq.rnd
    nch = (n + B.BIN_CHUNK - 1) // B.BIN_CHUNK
    seq.add(0, vlen)
    for c in range(nch):
        lo, hi = c * B.BIN_CHUNK, min((c + 1) * B.BIN_CHUNK, n)
        pos = r.randrange(max(lo, 1), hi) if hi > max(lo, 1) else -1
        k = 1 + c * (vlen - 6) // nch if shape == "ladder_up" else (vlen - 4) - c * (vlen - 6) // nch
        for i in range(max(lo, 1), hi):
            if shape == "all_inherit":
                seq.add(None, 0)
            elif i == pos:
                seq.add(k, vlen - k)
            else:
                t = r.randint(1, 3) if r.random() < 0.125 else 0
                seq.add(vlen - t, t)
    return seq


# ---- the groups -------------------------------------------------------------------------------------------

def group_batch(add):
    k = 0
    for n in BATCH_SIZES:
        for shape in SHAPES:
            seq = Seq(1000 + k)
            fill(seq, n, shape, B.WAVE)
            add(f"batch-{shape}-{n}", seq, cfg=CONFIGS[k % 4])
            k += 1
    # empty values: the page's first, inside a chain, a batch's last, a batch's first, the page's last
    for shape in ("ladder_up", "random"):
        seq = Seq(1100 + k)
        fill(seq, 129, shape, B.WAVE, empties={0, 20, 63, 64, 100, 128})
        add(f"batch-empties-{shape}-129", seq)
        k += 1


def pow2_chunk(seq, n):
    """A chunk of n values whose last value takes bytes 0, 1, ..., 8 from the values 255 (the chunk's
    first), 128, 64, ..., 2 and 1 before it; every other value inherits the previous one whole."""
    last = n - 1
    donors = {last - d: b for b, d in enumerate([last] + [1 << s for s in range(7, -1, -1) if (1 << s) < last])}
    for y in range(n):
        if y in donors:
            seq.add(donors[y], 24 - min(donors[y], len(seq.prev)) + 8)  # 32 bytes or so
        elif y == last:
            seq.add(len(donors), 3)
        else:
            seq.add(None, 0)


def group_tail(add):
    k = 0
    for n in TAIL_SIZES:
        for shape in SHAPES:
            seq = Seq(2000 + k)
            fill(seq, n, shape, B.BIN_CHUNK, num=48, den=B.BIN_CHUNK)
            add(f"tail-{shape}-{n}", seq, cfg=CONFIGS[k % 4])
            k += 1
    for n in (256, 513):  # chunk 0 (and chunk 1): donors at every power-of-two distance and at 255
        seq = Seq(2100 + n)
        for lo in range(0, n, B.BIN_CHUNK):
            pow2_chunk(seq, min(B.BIN_CHUNK, n - lo))
        add(f"tail-pow2-{n}", seq)
    for shape in ("ladder_up", "ladder_down"):  # 7 bytes a step: chunk-last values of up to 1800 bytes
        seq = Seq(2150 + len(shape))
        fill(seq, 513, shape, B.BIN_CHUNK, num=7)
        add(f"tail-long-{shape}-513", seq)
    # a chunk-last value of 1800 bytes that the next chunks inherit almost whole, then up to byte 1000
    seq = Seq(2160)
    fill(seq, B.BIN_CHUNK, "ladder_up", B.BIN_CHUNK, num=7)
    for i in range(2 * B.BIN_CHUNK + 100):
        t = seq.rnd.randint(0, 2)
        if i == B.BIN_CHUNK + 9:
            seq.add(1000, len(seq.prev) - 1000)
        else:
            seq.add(len(seq.prev) - t, t)
    add("tail-long-inherited-868", seq)
    seq = Seq(2200)  # chunk 0's last value is empty; chunk 1's last value too
    fill(seq, 600, "short_of_common", B.BIN_CHUNK, empties={255, 511})
    add("tail-empty-chunk-last-600", seq)
    seq = Seq(2201)  # chunk 1 and 2 inherit everything: m_c = |T_c|, no own bytes
    fill(seq, 700, "all_inherit", B.BIN_CHUNK)
    add("tail-no-own-bytes-700", seq)


def group_chain_par(add):
    k = 0
    for nch in CHAIN_PAR_CHUNKS:
        for shape in CHAIN_SHAPES:
            n = nch * B.BIN_CHUNK - (k * 37) % 200  # a partial last chunk, of another size each time
            if nch == B.DCP and shape == "ladder_down":
                n = nch * B.BIN_CHUNK  # exactly 65 536 values
            add(f"chain_par-{shape}-{nch}", chain_page(3000 + k, n, shape), cfg=(CONFIGS[0], CONFIGS[3])[k % 2])
            k += 1


def group_chain_serial(add):
    k = 0
    for n in CHAIN_SERIAL_VALUES:
        for shape in CHAIN_SHAPES:
            add(f"chain_serial-{shape}-{n}", chain_page(4000 + k, n, shape), cfg=(CONFIGS[0], CONFIGS[3])[k % 2])
            k += 1


def vb_page(seed, longest, nxt):
    """300 values or so, none longer than `longest`: short ones, one of `longest` bytes, a value that
    takes `nxt` bytes of it, one that takes all of that, one of `longest` bytes again with 9 new
    bytes at its end, short ones."""
    seq = Seq(seed)
    seq.small(130)
    seq.add(3, longest - min(3, len(seq.prev)))
    seq.add(nxt, min(5, longest - nxt))
    seq.add(None, 0)
    seq.add(min(longest - 9, len(seq.prev)), longest - min(longest - 9, len(seq.prev)))
    seq.small(170)
    return seq


def group_vb(add):
    for ln in VB_LENGTHS[:2]:
        add(f"vb-{ln}", vb_page(5000 + ln, ln, ln))
    for nxt in (2049, 2048, 1):
        add(f"vb-2049-next-{nxt}", vb_page(5100 + nxt, 2049, nxt))


def lds_page(seed, build):
    """Chunk 0: 256 short values; chunk 1: built by build(seq, batch index) per batch; 40 short values."""
    seq = Seq(seed)
    seq.small(B.BIN_CHUNK)
    for q in range(4):
        build(seq, q)
    seq.small(40)
    return seq


def group_lds(add):
    r = random.Random(6000)

    def chunk_total(extra):
        def build(seq, q):
            for t in range(B.WAVE):
                seq.add(r.randint(0, 4), 12 + (extra if q == 3 and t == 63 else 0))
        return build

    def batch_total(at, extra):
        def build(seq, q):
            if q != at:
                return seq.small(B.WAVE)
            for t in range(B.WAVE):
                p = min(r.randint(40, 64) if t else r.randint(0, 6), len(seq.prev))
                seq.add(p, 64 - p + (extra if t == 63 else 0))
        return build

    def batch_suffix(at, extra):
        def build(seq, q):
            if q != at:
                return seq.small(B.WAVE)
            for t in range(B.WAVE):
                seq.add(r.randint(0, 8), 48 + (extra if t == 31 else 0))
        return build
    for extra in (0, 1):
        add(f"lds-chunk-suffix-{B.DBA_SB + extra}", lds_page(6001 + extra, chunk_total(extra)))
    add(f"lds-batch-total-{B.DBA_OB}-at-1", lds_page(6010, batch_total(1, 0)))
    for at in (0, 2, 3):
        add(f"lds-batch-total-{B.DBA_OB + 1}-at-{at}", lds_page(6011 + at, batch_total(at, 1)))
    add(f"lds-batch-suffix-{B.DBA_SB}-at-1", lds_page(6020, batch_suffix(1, 0)))
    for at in (0, 2, 3):
        add(f"lds-batch-suffix-{B.DBA_SB + 1}-at-{at}", lds_page(6021 + at, batch_suffix(at, 1)))


def group_flba(add):
    for w in FLBA_WIDTHS:
        n = 300 if w >= 2048 else 600
        for shape in ("ladder_up", "ladder_down"):
            seq = Seq(7000 + w)
            for i in range(n):
                j = i % B.WAVE
                p = j * w // (B.WAVE - 1)
                p = min(p if shape == "ladder_up" else w - p, len(seq.prev))
                seq.add(p, w - p)
            add(f"flba-{shape}-{w}", seq, ptype=abi.FIXED_LEN_BYTE_ARRAY, type_length=w)


def carry_pages(seed, last_len, first_prefix):
    a = Seq(seed)
    a.small(100)
    if last_len:
        a.add(1, last_len - 1)
    else:
        a.add(0, 0)
    assert len(a.prev) == last_len
    b = Seq(seed + 1, previous=a.prev)
    b.P.append(first_prefix)  # (as written: an illegal one is longer than the previous value)
    b.S.append(b.rnd.randbytes(3))
    b.prev = a.prev[:first_prefix] + b.S[0]
    fill(b, 100, "random", B.WAVE)
    return (a.P, a.S), b


def group_carry(add, add_illegal):
    k = 0
    for ln in CARRY_LENGTHS:
        for fp in sorted({0, ln}):
            before, b = carry_pages(8000 + 2 * k, ln, fp)
            add(f"carry-last-{ln}-first-{fp}", b, before=before)
            k += 1
        before, b = carry_pages(8100 + 2 * k, ln, ln + 1)
        add_illegal(f"carry-last-{ln}-first-{ln + 1}", b, (abi.ERR_CORRUPT, 0), before=before, group="carry")
    before, b = carry_pages(8200, 2049, 2049)
    add("carry-null-page-between-2049", b, before=before, null_between=True)
    before, b = carry_pages(8202, 0, 0)
    add("carry-null-page-between-0", b, before=before, null_between=True)


def group_illegal(add_illegal):
    def base(seed, n=600, empties=()):
        seq = Seq(seed)
        fill(seq, n, "ties", B.BIN_CHUNK, empties=empties)
        return seq, [len(v) for v in B.unroll(seq.P, seq.S)]
    for at in ILLEGAL_AT:
        seq, lens = base(9000 + at)
        seq.P[at] = (lens[at - 1] if at else 0) + 1
        add_illegal(f"illegal-prefix-at-{at}", seq, (abi.ERR_CORRUPT, at))
    # chunk 256 (the 257th, one value) of a 257-chunk page: value 256 * 256
    seq = chain_page(9100, 256 * 256 + 1, "ladder_up")
    seq.P[256 * 256] = 65
    add_illegal("illegal-prefix-at-65536-chunk-256", seq, (abi.ERR_CORRUPT, 256 * 256))
    seq, lens = base(9200, empties={100})
    seq.P[101] = 1
    add_illegal("illegal-prefix-after-empty", seq, (abi.ERR_CORRUPT, 101))
    seq, lens = base(9300)
    seq.P[77] = -1
    add_illegal("illegal-negative-prefix", seq, (abi.ERR_CORRUPT, 77))
    seq, lens = base(9400)
    last = max(i for i, s in enumerate(seq.S) if s)
    add_illegal("illegal-suffix-bytes-one-short", seq, (abi.ERR_EOF, last), cut=1)


# ---- the lists -----------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _built():
    legal, illegal = [], []

    def adder(group):
        def add(name, seq, **kw):
            legal.append(Case(name, seq.P, seq.S, "legal", group=group, **kw))

        def add_illegal(name, seq, bad, **kw):
            kw.setdefault("group", "illegal")
            illegal.append(Case(name, seq.P, seq.S, "illegal", bad=bad, **kw))
        return add, add_illegal
    group_batch(adder("batch")[0])
    group_tail(adder("tail")[0])
    group_chain_par(adder("chain_par")[0])
    group_chain_serial(adder("chain_serial")[0])
    group_vb(adder("vb")[0])
    group_lds(adder("lds")[0])
    group_flba(adder("flba")[0])
    group_carry(*adder("carry"))
    group_illegal(adder("illegal")[1])
    names = [c.name for c in legal + illegal]
    assert len(names) == len(set(names))
    return tuple(legal), tuple(illegal)


def legal_cases(group=None):
    return [c for c in _built()[0] if group is None or c.group == group]


def illegal_cases(group=None):
    return [c for c in _built()[1] if group is None or c.group == group]


def case(name):
    return next(c for c in _built()[0] + _built()[1] if c.name == name)


# ---- columns --------------------------------------------------------------------------------------------------

def dba_page(body, n):
    return Page(body=body, num_values=n, encoding=abi.DELTA_BYTE_ARRAY, num_rows=n)


def filler(k, seed=0):
    """A one-value page of k bytes: moves what follows it by k bytes in the column's byte buffer."""
    s = random.Random(seed + k).randbytes(k)
    return dba_page(B.page([0], [s]), 1), [s]


def optional_page(rng, body, n_values, n_nulls, version=2):
    """The data section behind definition levels with n_nulls nulls among n_values + n_nulls slots."""
    dl = np.ones(n_values + n_nulls, dtype=np.uint8)
    dl[rng.permutation(dl.size)[:n_nulls]] = 0
    dls = writer.rle_encode_levels(dl, 1)
    if version == 1:
        pg = Page(body=len(dls).to_bytes(4, "little") + dls + body, num_values=dl.size, encoding=abi.DELTA_BYTE_ARRAY,
                  num_rows=dl.size)
    else:
        pg = Page(body=dls + body, num_values=dl.size, encoding=abi.DELTA_BYTE_ARRAY, version=2, num_nulls=n_nulls,
                  num_rows=dl.size)
        pg.dl_byte_length = len(dls)
    return pg, dl


def column_of(c, k=None, optional=0, seed=0):
    """-> (ColumnChunk, expected values, expected definition levels or None).
    The case's page, last in its column; before it a filler page of k bytes (k not None) or, for a
    carry case, the page it continues (and a null-only page). optional: 2 or 1: the pages as V2 / V1
    pages of an optional column with about 20 % nulls."""
    rng = np.random.default_rng(seed)
    ch = ColumnChunk(physical_type=c.ptype, type_length=c.type_length, max_def=1 if (optional or c.null_between) else 0)
    parts, dls = [], []  # [(body, values)]
    if c.before is not None:
        parts.append((B.page(*c.before), B.unroll(*c.before)))
        ch.dba_carry = True
    elif k is not None:
        assert c.ptype == abi.BYTE_ARRAY
        pg, v = filler(k, seed)
        parts.append((pg.body, v))
    try:
        vals = c.values()
    except B.Illegal as e:
        vals = B.unroll(c.prefixes[:e.index], c.suffixes[:e.index], c.previous)
    parts.append((c.page, vals))
    for i, (body, v) in enumerate(parts):
        n = len(v) if (c.kind == "legal" or i + 1 < len(parts)) else len(c.prefixes)
        if optional or c.null_between:
            pg, dl = optional_page(rng, body, n, max(n // 4, 3) if optional else 0, version=optional or 2)
            ch.pages.append(pg)
            dls.append(dl)
            if c.null_between and i + 2 == len(parts):
                pg, dl = optional_page(rng, B.page([], []), 0, 5, version=optional or 2)
                ch.pages.append(pg)
                dls.append(dl)
        else:
            ch.pages.append(dba_page(body, n))
    want = [v for _, vs in parts for v in vs]
    ch.n_values_hint = len(want)
    return ch, want, (np.concatenate(dls) if dls else None)
