"""GPU parity of the dictionary expansion (dict_tiles_body in csrc/pqgpu_dict.hip, run by
k_dict_fused<W> / k_dict_tiles<W> and their IDS variants) on hand-built run shapes: the counterpart of
test_gpu_dict_walk_forms.py, which puts *headers* on the walk's window edges; the pages here put *values*
on the expansion's output seams.

The seams (constants below, each with the source line it restates):
  shift     sh = out_offset % E: a page's slots start sh elements into its first 16-byte store;
  chunks    CH values counted in shifted slots, chunk j's first run from chunk_run[chunk_base + j];
  rounds    at most ROUND runs per sweep, the round ending at the start of run ROUND of the round, which can
            lie inside a tile and inside a lane's E elements;
  records   indices below PREFETCH come from the hand-off prefetch (pf0 / pf1 by __shfl), the others from
            memory; lane 63's run end (nx63, record k + t0 + 64) from pf1 or memory (its pf0 arm needs
            k + t0 + 64 < 64 and is never taken: no case can reach it);
  lanes     a lane whose E elements belong to 2, 3, 4 runs ("the element starts a later run");
  staging   a round's packed bytes [lo & ~15, hi + 8) in XT_SEG LDS bytes, the global sweep above that, the
            section staged before the hand-off when sec_end + 8 - (data_begin & ~15) <= XT_SEG, and its
            invalidation by a round that it does not cover;
  dictionary  LDS-resident when dict_n * W <= DICT_LDS and the workgroup's WPB chunks are of one column;
  stores    16-byte stores for whole tiles of a 16-byte aligned column, element stores otherwise.

Every case is a list of columns whose pages are built from a run list. The device is compared with two
independent expectations: the oracle (pqref.decode_batch, as test_gpu_parity.run_both does: values, counts,
first error) and a plain Python expansion of the run list (dictionary[id] per run), which owes nothing to
the oracle. Every case runs for INT64 (W = 8) and INT32 (W = 4), fused and split (DISPATCH_DICT_FUSED 1 / 0).

expansion_facts() restates, from a page's bytes alone, what the walk writes (one record per run header it
consumes: dict_walk_ls stores one record per emitted chain position, and put_record stores one for a header
taken by the 32-byte scalar shortcut or the scalar re-decode) and how the expansion cuts the page into
chunks and rounds; test_cases_reach_the_seams checks without a GPU that the cases reach every seam above,
that the oracle gives the stated status, and that the Python expansion equals the oracle's values.

Notes on the issue's list: a run cannot span a round seam (a round ends where a run starts), so the error
cases put the bad run last in a round and first in the next one; two packed runs of one round are at most
ROUND - 2 headers apart, so the round whose byte span exceeds XT_SEG "although each run is short" pads the
RLE headers between them with 0x80 continuation bytes (readUnsignedVarInt takes them; the walk's scalar
path). Every alignment data_begin & 15 in {0, 1, 15} is reached (V1 definition-level sections of 12, 13, 11
bytes after their 4-byte length).
"""
import bisect
import functools

import numpy as np
import pytest

from oracle import pqref
from pqgpu import abi
from tools.synth import writer

from helpers import assert_same
from test_gpu_dict_walk_forms import CARD, chunk, packed, rle, uvarint

PTYPE = {8: abi.INT64, 4: abi.INT32}
ROUND = 127      # `k += XT_RUNS - 1;`, constexpr uint32_t XT_RUNS = 128 (run table entries per wave)
PREFETCH = 128   # `pf0 = sld(rec + pw.rec_base + lane); pf1 = sld(rec + pw.rec_base + WAVE + lane);`
XT_SEG = 2560    # constexpr uint32_t XT_SEG = 2560 (LDS bytes for the packed data of one round)
DICT_LDS = 8192  # constexpr uint32_t DICT_LDS_BYTES = 8192 (dictionary staged in LDS per workgroup)
WPB = 4          # constexpr int WPB = 4 (pqgpu_device.h), DICT_WPB (pqgpu_plan.h): chunks per workgroup


def geom(W):
    """E = 16 / W (`constexpr uint32_t E = 16 / W`), TV = 64 E (`TV = WAVE * E`), CH = 16 TV
    (`CH = CH_TILES * TV`, DICT_CHUNK_TILES = 16)."""
    E = 16 // W
    return E, 64 * E, 16 * 64 * E


# ---- pages from run lists -----------------------------------------------------------------------------

def pack_ids(groups, ids, w):
    """packed() of test_gpu_dict_walk_forms for long runs (numpy instead of one big integer)."""
    if len(ids) <= 64:
        return packed(groups, ids, w)
    a = np.asarray(ids, dtype=np.uint64)
    bits = ((a[:, None] >> np.arange(w, dtype=np.uint64)) & np.uint64(1)).astype(np.uint8).ravel()
    return uvarint((groups << 1) | 1) + np.packbits(bits, bitorder="little").tobytes()


class Pg:
    """A page from runs ("rle", count, id[, header bytes]) / ("packed", ids, groups): ids shorter than
    8 * groups end the data early (a run cut by the section end: the missing ids read as 0). n: the page's
    value count (default: all of the runs'). lv: a V1 level section in front of the data."""

    def __init__(self, w, runs, n=None, lv=b""):
        body = bytearray([w])
        for r in runs:
            if r[0] == "rle":
                body += (r[3] + int(r[2]).to_bytes((w + 7) // 8, "little")) if len(r) > 3 else rle(r[1], r[2], w)
            else:
                assert len(r[1]) <= 8 * r[2] and all(0 <= v < 1 << w for v in r[1])
                body += pack_ids(r[2], r[1], w)
        self.w, self.runs, self.lv = w, runs, bytes(lv)
        self.n = sum(r[1] if r[0] == "rle" else 8 * r[2] for r in runs) if n is None else n
        self.body = self.lv + bytes(body)
        self.data_begin = len(self.lv)

    def ids(self):
        """The plain expansion of the run list: the page's n ids."""
        out = []
        for r in self.runs:
            out += [r[2]] * r[1] if r[0] == "rle" else list(r[1]) + [0] * (8 * r[2] - len(r[1]))
        assert len(out) >= self.n
        return np.array(out[:self.n], dtype=np.int64)


class Col:
    def __init__(self, pages, card=CARD, salt=0, nullable=False, dict_cut=0):
        self.pages, self.card, self.salt, self.nullable, self.dict_cut = pages, card, salt, nullable, dict_cut


class Case:
    """cols: the columns; code / err: the oracle's first error (code, page of the batch, value index)."""

    def __init__(self, cols, code=0, err=None):
        self.cols, self.code, self.err = cols if isinstance(cols, list) else [cols], code, err


def dictionary(card, W, salt=0):
    """card distinct entries, none of them small or regular (an odd multiplier is a bijection mod 2^k)."""
    i = np.arange(1, card + 1, dtype=np.uint64) + np.uint64(1000003 * salt)
    if W == 8:
        return (i * np.uint64(0x9E3779B97F4A7C15)).view(np.int64)
    return ((i * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32)


def build_chunks(case, W):
    out = []
    for c in case.cols:
        ch = chunk([(p.body, p.n) for p in c.pages], PTYPE[W], dictionary=dictionary(c.card, W, c.salt))
        assert ch.dict_page == dictionary(c.card, W, c.salt).tobytes()
        if c.nullable:
            ch.max_def = 1
        if c.dict_cut:
            ch.dict_page = ch.dict_page[:-c.dict_cut]
        out.append(ch)
    return out


def expected(case, W):
    """Per column the values of the Python expansion, or the first (batch page, value index) whose id is
    past the dictionary."""
    vals, page = [], 0
    for c in case.cols:
        d, col = dictionary(c.card, W, c.salt), []
        for p in c.pages:
            ids = p.ids()
            bad = np.nonzero(ids >= c.card)[0]
            if bad.size:
                return None, (page, int(bad[0]))
            col.append(d[ids])
            page += 1
        vals.append(np.concatenate(col) if col else d[:0])
    return vals, None


def levels_v1(n, nbytes):
    """A V1 definition-level section (4-byte length, RLE runs of level 1) of 4 + nbytes bytes for n slots."""
    two = {11: 1, 12: 0, 13: 2}[nbytes]
    three = (nbytes - 2 * two) // 3
    counts = [1] * two + [64] * (three - 1)
    counts.append(n - sum(counts))
    assert 64 <= counts[-1] < 8192
    runs = b"".join(uvarint(c << 1) + b"\x01" for c in counts)
    assert len(runs) == nbytes
    return len(runs).to_bytes(4, "little") + runs


# ---- what the walk and the expansion make of a page ---------------------------------------------------

def parse_headers(body, n, data_begin=0):
    """The walk's records, one per run header it consumes: (first value, end, packed, payload), payload =
    the raw RLE id or the page offset of the packed data (RunLengthBitPackingHybridDecoder.readNext)."""
    w, pos, end, produced, recs = body[data_begin], data_begin + 1, len(body), 0, []
    nb = (w + 7) // 8
    while produced < n and pos < end:
        h = hl = shift = 0
        while True:
            if pos + hl >= end:
                return recs
            b = body[pos + hl]
            h = (h | ((b & 0x7F) << (shift & 31))) & 0xFFFFFFFF
            shift, hl = shift + 7, hl + 1
            if b < 0x80:
                break
        if h & 1:
            g = h >> 1
            assert 0 < g < 1 << 28
            c, pk, payload, nx = 8 * g, True, pos + hl, min(pos + hl + g * w, end)
        else:
            c, pk, nx = (h >> 1) or n - produced, False, pos + hl + nb
            assert nx <= end
            payload = int.from_bytes(body[pos + hl:nx], "little")
        take = min(c, n - produced)
        recs.append((produced, produced + take, pk, payload))
        produced, pos = produced + take, nx
    return recs


def expansion_facts(body, n, W, out_offset, data_begin=0):
    """How dict_tiles_body cuts a page of n values at dense offset out_offset: the shift, the pre-stage
    size, the records, and per chunk its first record (chunk_run), the runs that intersect it, its rounds
    (b_lo, b_hi, the packed byte span (lo & ~15, hi + 8) or None, where the bytes come from: "pre" the
    section staged before the hand-off, "lds" a round's own staging, "global" the FAST = false sweep, the
    round's first record and the record whose end sets the span's end) and the numbers of runs that the E
    elements of its lanes belong to."""
    E, TV, CH = geom(W)
    sh = out_offset % E
    recs = parse_headers(body, n, data_begin)
    starts = [r[0] for r in recs]
    N = recs[-1][1] if recs else 0
    w, sec_end = body[data_begin], len(body)
    prestage = sec_end + 8 - (data_begin & ~15)
    pre_lo, pre_hi = (data_begin & ~15, sec_end + 8) if sec_end > data_begin and prestage <= XT_SEG else (1 << 32, 0)
    chunks = []
    for j in range((N + sh + CH - 1) // CH):
        v_lo, v_hi = max(j * CH, sh) - sh, min((j + 1) * CH, N + sh) - sh
        first = bisect.bisect_right(starts, v_lo) - 1
        n_runs = bisect.bisect_left(starts, v_hi) - first
        rounds, k, b_lo, p_hi = [], first, v_lo, pre_hi
        while True:
            live = [r for r in recs[k:k + ROUND] if r[0] < v_hi]
            b_hi = v_hi
            if len(live) >= ROUND:
                b_hi = min(starts[k + ROUND] if k + ROUND < len(recs) else N, v_hi)
            lo = min((pl + (((max(st, b_lo) - st) * w) >> 3) for st, en, pk, pl in live if pk), default=None)
            his = [pl + (((min(en, v_hi) - st) * w + 7) >> 3) + 8 if pk else 0 for st, en, pk, pl in live]
            hi = max(his) if lo is not None else None
            span = src = None
            if lo is not None:
                span = (lo & ~15, hi)
                if span[0] >= pre_lo and hi <= p_hi:
                    src = "pre"
                else:
                    p_hi = 0
                    src = "lds" if hi - span[0] <= XT_SEG else "global"
            rounds.append((b_lo, b_hi, span, src, k, k + his.index(hi) if span else None))
            if b_hi >= v_hi:
                break
            k, b_lo = k + ROUND, b_hi
        v = np.arange(v_lo, v_hi)
        run = np.searchsorted(starts, v, side="right")
        lane = (v + sh) // E
        _, at = np.unique(lane, return_index=True)
        per_lane = run[np.append(at[1:] - 1, len(v) - 1)] - run[at] + 1
        chunks.append(dict(first=first, n_runs=n_runs, rounds=rounds, lane_runs=set(per_lane.tolist()),
                           full=v_hi - v_lo == CH))
    return dict(sh=sh, prestage=prestage, staged_before=pre_hi > 0, records=recs, chunks=chunks)


def planned_chunks(batch, W):
    """The expansion's chunk list of the W-byte dictionary pages, as the plan orders it (batch page order,
    dict_page_chunks(slots) chunks per page): the column of every chunk, WPB per workgroup."""
    E, TV, CH = geom(W)
    cols = []
    for pg in batch.pages:
        if abi.elem_width(batch.columns[int(pg["column"])]["physical_type"], 0) == W:
            cols += [int(pg["column"])] * ((int(pg["num_values"]) + E - 1 + CH - 1) // CH)
    return [cols[i:i + WPB] for i in range(0, len(cols), WPB)]


# ---- the cases ----------------------------------------------------------------------------------------

def _cycle(k, top, seed):
    return np.random.default_rng(seed).integers(0, top, size=k).tolist()


def _aligned(pages_of, sh, W):
    """Pages with an aligner page of 1 .. E - 1 values in front of each page that would not start at
    shift sh otherwise. pages_of: [function(sh) -> Pg]."""
    E = geom(W)[0]
    out, off = [], 0
    for make_page in pages_of:
        fix = (sh - off) % E
        if fix:
            out.append(Pg(3, [("rle", fix, 2)]))
        out.append(make_page(sh))
        off += fix + out[-1].n
        assert (off - out[-1].n) % E == sh
    return out


def _a_page(form, N, sh, W, seed):
    E, TV, CH = geom(W)
    if form == "rle":  # one record serves every chunk
        return Pg(3, [("rle", N, seed % CARD)])
    if form == "seam":  # run boundaries at each chunk seam, one value before it and one after
        cuts = sorted({c for s in range(CH - sh, N + 2, CH) for c in (s - 1, s, s + 1) if 0 < c < N}) or \
            ([N // 2] if N >= 2 else [])
        edges = [0] + cuts + [N]
        return Pg(3, [("rle", b - a, (seed + i) % CARD) for i, (a, b) in enumerate(zip(edges, edges[1:]))])
    w = int(form[1:])  # one packed run of odd width: chunk j starts inside a byte
    g = (N + 7) // 8
    return Pg(w, [("packed", _cycle(8 * g, min(1 << w, DICT_LDS // W), seed), g)], n=N)


def _group_a(W, sh, form, half):
    E, TV, CH = geom(W)
    targets = [1, E - 1, E, E + 1, TV - 1, TV, TV + 1] if half == "lo" else [CH - 1, CH, CH + 1, 2 * CH, 2 * CH + 1]
    sizes = [t - sh for t in dict.fromkeys(targets) if t - sh >= 1]
    if half == "hi":
        sizes.append(CH + 1 - sh)  # the column's last page: its last chunk holds one value
    pages = _aligned([functools.partial(_a_page, form, N, W=W, seed=7 * i + sh) for i, N in enumerate(sizes)], sh, W)
    return Case(Col(pages, card=CARD if form in ("rle", "seam") else min(1 << int(form[1:]), DICT_LDS // W)))


def _short_runs(total, seed, every=0):
    """Runs of 1, 2, 3 values (a packed group of 8 after every `every` runs) of `total` values."""
    rng, runs, left, i = np.random.default_rng(seed), [], total, 0
    while left:
        i += 1
        if every and i % every == 0 and left >= 8:
            runs.append(("packed", rng.integers(0, CARD, size=8).tolist(), 1))
            left -= 8
        else:
            c = min(int(rng.integers(1, 4)), left)
            runs.append(("rle", c, (i * 3) % CARD))
            left -= c
    return runs


def _group_b(W):
    E, TV, CH = geom(W)
    one = [("rle", 1, i % 2 + 1) for i in range(2 * TV)]               # two tiles of runs of one value
    mixed = _short_runs(CH + TV + 5, seed=W, every=23)
    three = [("rle", c, (i + i // 3) % CARD) for i, c in enumerate([1, 2, 1] * (TV // 2))]  # W = 4: 3 runs per lane
    pages = [Pg(3, one), Pg(3, mixed), Pg(3, three)]
    lead = Pg(3, [("rle", E + 1, 4)])                                # the same pages at shift 1
    return Case(Col(pages + [lead] + [Pg(3, list(r)) for r in (one, mixed, three)]))


PACKED_AT = (60, 61, 130, 200, 201)  # C: records of both sources carry packed payloads too


def _runs_c(k, first=0):
    """k runs of 3 values (8 for the packed groups at PACKED_AT), numbered from `first`."""
    return [("packed", _cycle(8, 8, i), 1) if i in PACKED_AT else ("rle", 3, i % 8) for i in range(first, first + k)]


def _len(runs):
    return sum(r[1] if r[0] == "rle" else 8 * r[2] for r in runs)


def _group_c_runs(W):
    """Full chunks of exactly R runs."""
    CH = geom(W)[2]
    pages = []
    for R in (126, 127, 128, 129, 253, 254, 255):
        runs = _runs_c(R - 1)
        pages.append(Pg(3, runs + [("rle", CH - _len(runs), 7)]))
        assert pages[-1].n == CH
    return Case(Col(pages, card=8))


def _group_c_first(W, sh):
    """Pages whose second chunk starts with record K, which begins at the seam ("edge") or two values
    before it ("cross"); more than 64 runs in the second chunk."""
    E, TV, CH = geom(W)
    pages = [Pg(3, [("rle", E + sh, 1)])] if sh else []
    for K in (63, 64, 65, 127, 128, 129):
        for back in (0, 2):
            runs = _runs_c(K - 1)
            runs.append(("rle", CH - sh - back - _len(runs), 6))       # record K - 1 ends at the seam (- 2)
            runs += _runs_c(100, first=K)
            runs.append(("rle", 3 + (-(_len(runs) + 3)) % E, 5))       # a multiple of E values: the shift stays
            pages.append(Pg(3, runs))
    return Case(Col(pages, card=8))


def _group_c_nx63(W):
    """Lane 63's run end (record k + 64 = 127: pf1; 128, 129: memory) decides how many packed bytes the round
    stages: the second chunk starts with record K, its record K + 63 is a packed run of 400 values, the
    round's last, in a section too long to be staged before the hand-off."""
    E, TV, CH = geom(W)
    w, top, pages = 17, DICT_LDS // W, []
    for K in (63, 64, 65):
        runs = [("rle", 3, i % CARD) for i in range(K - 1)]
        runs[5] = ("packed", _cycle(1000, top, K), 125)
        runs.append(("rle", CH - _len(runs), 6))
        runs += [("rle", 3, i % CARD) for i in range(63)] + [("packed", _cycle(400, top, K + 1), 50)]
        runs += [("rle", 3, i % CARD) for i in range(9)]
        runs.append(("rle", 3 + (-(_len(runs) + 3)) % E, 5))
        pages.append(Pg(w, runs))
    return Case(Col(pages, card=top))


def _full_packed(W, w, n=None, seed=0, short=0):
    CH = geom(W)[2]
    n = CH if n is None else n
    g = (n + 7) // 8
    ids = _cycle(8 * g, min(1 << w, DICT_LDS // W), seed + w)
    return ("packed", ids[:len(ids) - short], g)


def _group_d_full(W):
    """A full chunk of one packed run: under XT_SEG, 8 bytes over it, and far over it."""
    pages = [Pg(w, [_full_packed(W, w)]) for w in ((9, 10, 16, 32) if W == 8 else (4, 5, 6))]
    # a round that stages exactly XT_SEG bytes, and one id more: 15 RLE runs of 3 bytes and a 2-byte header put the
    # packed data at page offset 48; 1,856 (1,857) ids of 11 bits take 2,552 (2,554) bytes, + 8
    for n in (1856, 1857):
        pages.append(Pg(11, [("rle", 1, i % CARD) for i in range(15)] + [_full_packed(W, 11, n=n)], n=15 + n))
    return Case(Col(pages, card=DICT_LDS // W))


def _group_d_three(W):
    """Three chunks: RLE runs with a packed group, one packed run over XT_SEG, RLE runs again; and one
    chunk of three rounds: staged, global, staged."""
    E, TV, CH = geom(W)
    w = 12 if W == 8 else 6
    top = min(1 << w, DICT_LDS // W)
    side = [("rle", 5, i % CARD) if i % 40 else ("packed", _cycle(8, top, i), 1) for i in range(CH // 8)]
    side.append(("rle", CH - _len(side), 1))
    a = Pg(w, side + [_full_packed(W, w)] + side)
    small = [("rle", 1, i % CARD) for i in range(ROUND - 1)]
    big = CH - 2 * (ROUND - 1) - 8 - 24
    b = Pg(w, small[:50] + [("packed", _cycle(8, top, 3), 1)] + small[50:] + [_full_packed(W, w, big - big % 8, seed=1)] +
           small + [("packed", _cycle(8, top, 4), 1), ("rle", 16 + big % 8, 2)])
    assert b.n == CH
    return Case(Col([a, b], card=top))


def _rle_fill(nbytes, seed):
    """RLE runs of 1-3 values at w = 8 (2 bytes each, one of 64 values and 3 bytes when nbytes is odd)."""
    runs = [("rle", 64, 3)] if nbytes % 2 else []
    return runs + [("rle", 1 + (i + seed) % 3, (i + seed) % CARD) for i in range((nbytes - 3 * len(runs)) // 2)]


def _group_d_prestage(W):
    """Nullable V1 pages whose data section makes sec_end + 8 - (data_begin & ~15) 2559, 2560, 2561 at
    data_begin & 15 = 0, 1, 15: a packed run of 1,600 values ends the section."""
    pages = []
    for size in (2559, 2560, 2561):
        for lv_bytes in (12, 13, 11):
            db = 4 + lv_bytes
            data = size - 8 + (db & ~15) - db            # bytes of the data section
            tail = ("packed", _cycle(1600, 200, size + lv_bytes), 200)
            runs = _rle_fill(data - 1 - 2 - 1600, size) + [tail]
            n = _len(runs)
            pages.append(Pg(8, runs, lv=levels_v1(n, lv_bytes)))
            assert len(pages[-1].body) + 8 - (db & ~15) == size and db & 15 == (0, 1, 15)[(12, 13, 11).index(lv_bytes)]
    return Case(Col(pages, card=200, nullable=True))


def _group_d_cut(W):
    """A packed run cut by the section end in the page's last chunk: in a section staged before the
    hand-off (the round reaches past it: staged again), staged per round, and under the global sweep."""
    E, TV, CH = geom(W)
    pages = []
    for w, lead, cut in ((3, 40, 15), (3, CH, CH // 4), (32, CH, CH // 4)):
        top = min(1 << w, DICT_LDS // W)
        runs = [("rle", 5, i % CARD) for i in range(lead // 5)]
        runs.append(_full_packed(W, w, n=CH // 2 if lead == CH else 64, seed=lead, short=cut))
        pages.append(Pg(w, runs))
    return Case(Col(pages, card=DICT_LDS // W))


def _group_d_apart(W):
    """Two packed groups of one round more than XT_SEG bytes apart: the RLE headers between them are
    varints padded with continuation bytes (30 bytes each)."""
    pad = lambda c: bytes([0x80 | (c << 1)]) + b"\x80" * 28 + b"\x00"
    runs = [("packed", _cycle(8, 8, 1), 1)] + [("rle", 2, i % CARD, pad(2)) for i in range(100)] + \
        [("packed", _cycle(8, 8, 2), 1), ("rle", 9, 1)]
    return Case(Col([Pg(3, runs), Pg(3, [("rle", 3, 0)] + runs)], card=8))


def _group_e_dict(W, over):
    """A dictionary of exactly DICT_LDS bytes, or one entry more: ids that touch entry 0 and the last."""
    card = DICT_LDS // W + over
    w = card.bit_length() if over else (card - 1).bit_length()
    ids = _cycle(512, card, over)
    ids[0], ids[1], ids[-1] = card - 1, 0, card - 1
    runs = [("rle", 3, card - 1), ("rle", 2, 0), ("packed", ids, 64), ("rle", 70, card - 1), ("rle", 1, 0)]
    return Case(Col([Pg(w, runs), Pg(w, list(reversed(runs)))], card=card))


def _group_e_mix(W, chunks_per_col):
    """Columns of 1-3 chunks each, back to back in the chunk list: workgroups whose WPB chunks belong to
    different columns (no dictionary in LDS: every value is gathered from memory)."""
    CH = geom(W)[2]
    cols = []
    for i, nch in enumerate(chunks_per_col):
        runs = _short_runs(nch * CH - 9 - i, seed=10 * W + i, every=11)
        cols.append(Col([Pg(3, runs)], card=CARD + i, salt=i + 1))
    return Case(cols)


def _group_e_short(W):
    """The dictionary page is 3 bytes short of dict_num_values entries (PlainValuesDictionary ctor)."""
    return Case(Col([Pg(3, [("rle", 9, 1)])], dict_cut=3), code=abi.ERR_EOF, err=(0, -1))


def _group_f(W, form):
    """[good page, bad page, good page]; the good page in front leaves shift 1."""
    E, TV, CH = geom(W)
    sh, BAD = 1, 6
    good = Pg(3, [("rle", E + 1, 2), ("packed", _cycle(8, CARD, 5), 1)], n=E + 1)
    if form in ("rle_chunk", "rle_round_last", "rle_round_first"):
        if form == "rle_chunk":   # the bad run spans the chunk seam: both chunks report its first value
            at = CH - sh - 10
            runs = [("rle", at, 1), ("rle", 20, BAD), ("rle", 30, 2)]
        else:                     # record ROUND - 1 (last of round one) / ROUND (first of round two)
            k = ROUND - 1 if form == "rle_round_last" else ROUND
            runs = [("rle", 3, i % CARD) for i in range(k)] + [("rle", 5, BAD)] + [("rle", 3, i % CARD) for i in range(20)]
            at = 3 * k
        return Case(Col([good, Pg(3, runs), good]), code=abi.ERR_DICT_ID, err=(1, at))
    N = CH + 100 - 3
    ids = _cycle(CH + 104, CARD, 9)
    at = {"packed_chunk_first": CH - sh, "packed_chunk_last": CH - sh - 1, "packed_last": N - 1, "packed_padding": N}[form]
    ids[at] = 7
    if form == "packed_padding":  # ids past N are never read: no error
        ids[N + 1] = ids[N + 2] = 7
        return Case(Col([good, Pg(3, [("packed", ids, (CH + 104) // 8)], n=N), good], card=CARD))
    return Case(Col([good, Pg(3, [("packed", ids, (CH + 104) // 8)], n=N), good]), code=abi.ERR_DICT_ID, err=(1, at))


def _groups(W):
    E = geom(W)[0]
    g = {}
    for sh in range(E):
        for form in ("rle", "seam", "w3", "w11"):
            for half in ("lo", "hi"):
                g[f"A_{half}_sh{sh}_{form}"] = functools.partial(_group_a, W, sh, form, half)
    g["B_lanes"] = functools.partial(_group_b, W)
    g["C_runs"] = functools.partial(_group_c_runs, W)
    for sh in (0, E - 1):
        g[f"C_first_sh{'0' if sh == 0 else 'max'}"] = functools.partial(_group_c_first, W, sh)
    g["C_nx63"] = functools.partial(_group_c_nx63, W)
    g["D_full"] = functools.partial(_group_d_full, W)
    g["D_three"] = functools.partial(_group_d_three, W)
    g["D_prestage"] = functools.partial(_group_d_prestage, W)
    g["D_cut"] = functools.partial(_group_d_cut, W)
    g["D_apart"] = functools.partial(_group_d_apart, W)
    g["E_dict_fits"] = functools.partial(_group_e_dict, W, 0)
    g["E_dict_over"] = functools.partial(_group_e_dict, W, 1)
    g["E_mix2"] = functools.partial(_group_e_mix, W, (3, 3))
    g["E_mix3"] = functools.partial(_group_e_mix, W, (1, 2, 3))
    g["E_dict_short"] = functools.partial(_group_e_short, W)
    for form in ("rle_chunk", "rle_round_last", "rle_round_first", "packed_chunk_first", "packed_chunk_last",
                 "packed_last", "packed_padding"):
        g[f"F_{form}"] = functools.partial(_group_f, W, form)
    return g


GROUPS = {W: _groups(W) for W in (8, 4)}
PARAMS = [pytest.param(W, name, id=f"W{W}-{name}") for W in (8, 4) for name in GROUPS[W]]


@functools.lru_cache(maxsize=None)
def case(W, name):
    return GROUPS[W][name]()


@functools.lru_cache(maxsize=None)
def reference(W, name):
    """(batch, oracle result, Python expansion per column or None, its first bad (page, index) or None):
    computed once per case and shared; nothing changes it."""
    c = case(W, name)
    batch = writer.build_batch(build_chunks(c, W))
    vals, bad = expected(c, W)
    return batch, pqref.decode_batch(batch), vals, bad


def case_facts(W, name):
    """expansion_facts of every page of the case, at the dense offset its column has reached."""
    out = []
    for c in case(W, name).cols:
        off = 0
        for p in c.pages:
            out.append(expansion_facts(p.body, p.n, W, off, p.data_begin))
            off += p.n
    return out


# ---- no GPU: the cases reach the seams, the two expectations agree ------------------------------------

def test_builders_agree():
    rng = np.random.default_rng(1)
    for w in (1, 3, 11, 32):
        ids = rng.integers(0, 1 << w, size=8 * 20).tolist()
        assert pack_ids(20, ids, w) == packed(20, ids, w)
        assert pack_ids(20, ids[:-13], w) == packed(20, ids[:-13], w)
    p = Pg(3, [("rle", 5, 4), ("packed", [1, 2, 3], 1), ("rle", 2, 1, b"\x84\x80\x00")], n=14)
    assert p.ids().tolist() == [4] * 5 + [1, 2, 3, 0, 0, 0, 0, 0] + [1]
    assert parse_headers(p.body, p.n) == [(0, 5, False, 4), (5, 13, True, 4), (13, 14, False, 1)]


@pytest.mark.parametrize("W", [8, 4])
def test_cases_reach_the_seams(W):
    """No GPU. The oracle's verdict and the Python expansion on every case, and the seams the cases reach
    (expansion_facts): a seam taken out of the cases fails here."""
    E, TV, CH = geom(W)
    shifts, runs_full, firsts, lane_runs, spans, prestages, dict_bytes = set(), set(), set(), set(), set(), set(), set()
    sources, off_boundary, nx63 = set(), False, set()
    for name in GROUPS[W]:
        c = case(W, name)
        batch, ref, vals, bad = reference(W, name)
        assert len(batch.pages) <= 26, name
        if c.code:
            assert ref.code == c.code and ref.status[1:] == c.err, (name, ref.status)
            assert c.cols[0].dict_cut or bad == c.err, (name, bad)
            continue
        assert ref.code == 0 and bad is None, (name, ref.status, bad)
        for i, col in enumerate(c.cols):
            assert ref.columns[i]["n_values"] == len(vals[i]), name
            assert_same(vals[i], ref.columns[i]["values"], PTYPE[W])
            dict_bytes.add(col.card * W)
        mixed = sum(len(set(wg)) > 1 for wg in planned_chunks(batch, W))
        assert (mixed > 0) == name.startswith("E_mix"), name  # one expansion workgroup, chunks of several columns
        for p, f in zip([p for col in c.cols for p in col.pages], case_facts(W, name)):
            assert p.n <= 3 * CH, name
            shifts.add(f["sh"])
            if p.lv:
                prestages.add((f["prestage"], p.data_begin & 15))
            for ch in f["chunks"]:
                firsts.add(ch["first"])
                lane_runs |= ch["lane_runs"]
                if ch["full"]:
                    runs_full.add(ch["n_runs"])
                for b_lo, b_hi, span, src, k, k_hi in ch["rounds"]:
                    sources.add((src, f["staged_before"]))
                    if src == "lds" and k_hi == k + 63 and span[1] - span[0] > 64:
                        nx63.add(k + 64)  # lane 63's run end decides how many bytes the round stages
                    if span and src != "pre":
                        spans.add(min(max(span[1] - span[0], XT_SEG - 1), XT_SEG + 1))
                    if b_hi < CH * (1 + b_hi // CH) and ch["rounds"][-1][1] != b_hi:
                        off_boundary |= (b_hi + f["sh"]) % TV != 0 and (b_hi + f["sh"]) % E != 0
    assert shifts == set(range(E))
    assert runs_full >= {126, 127, 128, 129, 253, 254, 255}
    assert firsts >= {63, 64, 65, 127, 128, 129}
    assert nx63 >= {PREFETCH - 1, PREFETCH, PREFETCH + 1}  # nx63 from pf1, and from memory
    assert off_boundary
    assert spans == {XT_SEG - 1, XT_SEG, XT_SEG + 1}   # below (clamped), equal, above (clamped)
    assert prestages == {(s, a) for s in (2559, 2560, 2561) for a in (0, 1, 15)}
    assert lane_runs >= set(range(1, E + 1))
    assert {DICT_LDS, DICT_LDS + W} <= dict_bytes
    # a section staged before the hand-off that a round reaches past (staged again), and the three sources
    assert {("pre", True), ("lds", True), ("lds", False), ("global", False), (None, False)} <= sources


def test_exact_round_span():
    """Rounds whose packed bytes take exactly XT_SEG bytes, and one id (2 bytes) more: the numbers themselves,
    not the clamped classes of test_cases_reach_the_seams."""
    for W in (8, 4):
        got = {span[1] - span[0] for f in case_facts(W, "D_full") + case_facts(W, "D_prestage")
               for ch in f["chunks"] for _, _, span, src, _, _ in ch["rounds"] if span and src != "pre"}
        assert {XT_SEG, XT_SEG + 2} <= got, sorted(got)


# ---- GPU ----------------------------------------------------------------------------------------------

@pytest.fixture(params=[1, 0], ids=["fused", "split"])
def dict_fused(decoder, request):
    """PQG_DISPATCH_DICT_FUSED: 1 = walk + expansion in one launch (k_dict_fused), 0 = k_dict_runs +
    k_dict_tiles, which the timeout re-run falls back to."""
    decoder.set_dispatch(abi.DISPATCH_DICT_FUSED, request.param)
    yield request.param
    decoder.set_dispatch(abi.DISPATCH_DICT_FUSED, 1)


def check_columns(W, name, cols_numpy, n_values):
    """Device values against the oracle and against the Python expansion."""
    batch, ref, vals, bad = reference(W, name)
    for i, cd in enumerate(batch.columns):
        assert n_values[i] == ref.columns[i]["n_values"] == len(vals[i])
        assert_same(cols_numpy[i], ref.columns[i]["values"], cd["physical_type"])
        assert_same(cols_numpy[i], vals[i], cd["physical_type"])


@pytest.mark.gpu
@pytest.mark.parametrize("W,name", PARAMS)
def test_dict_expand_forms(decoder, dict_fused, W, name):
    c = case(W, name)
    batch, ref, vals, bad = reference(W, name)
    dcols, st = decoder.decode(decoder.upload(batch), check=False)
    assert (int(st.code), int(st.page), int(st.value_index)) == ref.status, \
        f"gpu status {st.code, st.page, st.value_index} {st.message} vs oracle {ref.status}"
    assert ref.code == c.code
    if c.code:
        return
    check_columns(W, name, [d.numpy() for d in dcols], [d.n_values for d in dcols])
    for i, cd in enumerate(batch.columns):
        if cd["max_def"] > 0:
            assert np.array_equal(dcols[i].def_levels[:batch.column_slots[i]].cpu().numpy(), ref.columns[i]["def_levels"])


IDS_NAMES = [n for n in GROUPS[4] if n.startswith(("A_", "C_"))]


@pytest.mark.gpu
@pytest.mark.parametrize("name", IDS_NAMES)
def test_dict_expand_ids(decoder, dict_fused, name):
    """The ids variant (k_dict_fused<4, true> / k_dict_tiles<4, true>: a COLUMN_DICTIONARY_IDS column gets
    uint32 ids, whatever its type): the INT32 cases of A and C, whose seams are those of 4-byte elements,
    against the ids of the run lists (the oracle has no id output)."""
    import copy
    batch, ref, vals, bad = reference(4, name)
    ibatch = copy.copy(batch)
    ibatch.columns = [dict(cd, flags=abi.COLUMN_DICTIONARY_IDS) for cd in batch.columns]
    dcols, st = decoder.decode(decoder.upload(ibatch), check=False)
    assert int(st.code) == 0, st.message
    for col, d in zip(case(4, name).cols, dcols):
        want = np.concatenate([p.ids() for p in col.pages]).astype(np.uint32)
        assert d.n_values == len(want)
        got = d.values[:4 * d.n_values].cpu().numpy().view(np.uint32)
        bad_at = np.nonzero(got != want)[0]
        assert bad_at.size == 0, f"{bad_at.size} ids differ, first at {bad_at[:5]}: {got[bad_at[:5]]} vs {want[bad_at[:5]]}"


@pytest.mark.gpu
@pytest.mark.parametrize("W", [8, 4])
@pytest.mark.parametrize("name", ["A_hi_sh1_seam", "C_first_shmax"])
def test_dict_expand_relaunch(decoder, dict_fused, W, name):
    """A plan launched twice (flags and epochs of a second launch), the outputs poisoned in between."""
    import torch
    batch, ref, vals, bad = reference(W, name)
    plan = decoder.plan(decoder.upload(batch))
    try:
        for _ in range(2):
            for col in plan.columns:
                col.values.fill_(0x5A)
            decoder.stream.wait_stream(torch.cuda.current_stream(decoder.device))  # the fills first
            plan.launch()
            rc, st = plan.sync()
            assert rc == 0, st.message
            check_columns(W, name, [col.numpy() for col in plan.columns], [col.n_values for col in plan.columns])
    finally:
        plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("W", [8, 4])
@pytest.mark.parametrize("skew", [0, 1], ids=["aligned16", "element_aligned"])
@pytest.mark.parametrize("name", ["A_hi_sh1_w11", "A_lo_sh0_rle"])
def test_dict_expand_output_guard(decoder, dict_fused, W, skew, name):
    """The column's values in a slice of a canary-filled tensor: 16-byte aligned (whole tiles take 16-byte
    stores) and W bytes further (out16 is false: every tile takes element stores; the C ABI accepts an
    element-aligned pointer). No byte before or after the column changes."""
    import torch
    batch, ref, vals, bad = reference(W, name)
    n = batch.column_slots[0]
    cols = decoder.alloc_columns(batch)
    big = torch.full((n * W + 512,), 0xC3, dtype=torch.uint8, device=decoder.device)
    assert big.data_ptr() % 16 == 0
    lo = 256 + skew * W
    cols[0].values = big[lo:lo + n * W]
    cols[0].values.fill_(0xA5)
    dcols, st = decoder.decode(decoder.upload(batch), cols=cols, check=False)
    assert int(st.code) == 0, st.message
    check_columns(W, name, [d.numpy() for d in dcols], [d.n_values for d in dcols])
    host = big.cpu().numpy()
    assert (host[:lo] == 0xC3).all() and (host[lo + n * W:] == 0xC3).all()
