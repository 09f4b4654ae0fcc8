"""Hand-assembled Zstandard frames (RFC 8878) for tests: a frame BUILDER, not a compressor.

The caller describes a frame piece by piece (frame header fields, blocks, the literals section, the
sequences as explicit (literal_length, match_length, offset_value) triples, the mode and content of
every table), and gets the frame's bytes and the bytes it must decode to. The expected output comes
from executing the described blocks here (literal copy, match copy, repeat-offset rules): it is known
by construction and owes nothing to the oracle (oracle/zstd_ref.c) or the device decoder.
tests/test_zstd_build.py holds every frame of `legal_cases()` / `illegal_cases()` against libzstd.

Pure Python + numpy, deterministic.
"""
import heapq

import numpy as np

from oracle import pqref

MAGIC = 0xFD2FB528
LL_BASE = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 18, 20, 22, 24, 28, 32, 40,
           48, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536]
LL_BITS = [0] * 16 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
ML_BASE = list(range(3, 35)) + [35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099,
                                8195, 16387, 32771, 65539]
ML_BITS = [0] * 32 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
LL_DEF = [4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1]
ML_DEF = [1, 4, 3, 2, 2, 2, 2, 2, 2] + [1] * 37 + [-1] * 7
OF_DEF = [1, 1, 1, 1, 1, 1, 2, 2, 2] + [1] * 15 + [-1] * 5
# per table kind: (predefined counts, predefined log, largest log, largest symbol)
KINDS = {"ll": (LL_DEF, 6, 9, 35), "of": (OF_DEF, 5, 8, 31), "ml": (ML_DEF, 6, 9, 52)}
PREDEF, RLE, FSE, REPEAT = 0, 1, 2, 3


def ll_code(v):
    return max(c for c in range(36) if LL_BASE[c] <= v)


def ml_code(v):
    return max(c for c in range(53) if ML_BASE[c] <= v)


def of_code(v):
    return v.bit_length() - 1


# ---- bit streams ------------------------------------------------------------------------------------
class Bits:
    """Little-endian bit writer. A backward stream (RFC 8878 4.1) is written in the reverse of the
    order it is read and closed with `backward()`: the padding 1 bit goes above the last field."""

    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def put(self, v, k):
        assert 0 <= v < (1 << k) or k == 0 and v == 0, (v, k)
        self.acc |= v << self.n
        self.n += k
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def forward(self):
        """Bytes of a forward stream (zero padded to a byte)."""
        return bytes(self.out) + (bytes([self.acc]) if self.n else b"")

    def backward(self, pad=True):
        if pad:
            self.put(1, 1)
        return self.forward()


# ---- FSE ----------------------------------------------------------------------------------------------
def fse_table(norm, log):
    """Decoding table of normalized counts: per state (symbol, bits, baseline), RFC 8878 4.1.1."""
    size = 1 << log
    sym = [0] * size
    high = size - 1
    for s, c in enumerate(norm):
        if c == -1:
            sym[high] = s
            high -= 1
    step, pos = (size >> 1) + (size >> 3) + 3, 0
    for s, c in enumerate(norm):
        for _ in range(max(c, 0)):
            sym[pos] = s
            pos = (pos + step) & (size - 1)
            while pos > high:
                pos = (pos + step) & (size - 1)
    assert pos == 0, "counts do not fill the table"
    nxt = [1 if c == -1 else c for c in norm]
    tab = []
    for u in range(size):
        s = sym[u]
        ns = nxt[s]
        nxt[s] += 1
        nb = log - (ns.bit_length() - 1)
        tab.append((s, nb, (ns << nb) - size))
    return tab


def rle_table(sym):
    return [(sym, 0, 0)]


def ncount_bytes(norm, log, raw_log=None):
    """FSE table description (RFC 8878 4.1.1): accuracy log and the normalized counts, with the
    2-bit zero-run repeat flags after every zero count. `norm` ends at its last non-zero count."""
    b = Bits()
    b.put((log if raw_log is None else raw_log) - 5, 4)
    remaining = (1 << log) + 1
    i = 0
    while i < len(norm):
        v = norm[i] + 1
        nbits = remaining.bit_length()
        maxv = (1 << nbits) - 1 - remaining
        if v < maxv:
            b.put(v, nbits - 1)
        elif v < (1 << (nbits - 1)):
            b.put(v, nbits)
        else:
            b.put(v + maxv, nbits)
        remaining -= abs(norm[i])
        i += 1
        if norm[i - 1] == 0:
            z = 0
            while i < len(norm) and norm[i] == 0:
                z += 1
                i += 1
            while z >= 3:
                b.put(3, 2)
                z -= 3
            b.put(z, 2)
    return b.forward()


def derive_norm(symbols, log, lt1=False):
    """Normalized counts of accuracy `log` for the symbols used (every used symbol gets a state; with
    lt1 the rarest ones get the "less than 1" count -1)."""
    size = 1 << log
    hist = {}
    for s in symbols:
        hist[s] = hist.get(s, 0) + 1
    assert hist and len(hist) <= size
    norm = [0] * (max(hist) + 1)
    total = sum(hist.values())
    left = size
    order = sorted(hist, key=lambda s: (hist[s], s))
    for s in order:
        norm[s] = 1
        left -= 1
    for s in order[::-1]:  # proportional shares, the most frequent first
        add = min(left, hist[s] * (size - len(hist)) // total)
        norm[s] += add
        left -= add
    norm[order[-1]] += left
    if lt1:
        for s in order[:-1]:
            if norm[s] == 1:
                norm[s] = -1
    assert sum(abs(c) for c in norm) == size
    return norm


def _state_for(tab, sym, nxt, need_bits=False):
    """The state holding `sym` from which the decoder moves to state `nxt` (nxt None: any state of
    the symbol; need_bits: one that reads at least one bit)."""
    for u, (s, nb, base) in enumerate(tab):
        if s != sym:
            continue
        if nxt is None:
            if not need_bits or nb:
                return u
        elif base <= nxt < base + (1 << nb):
            return u
    raise ValueError(f"symbol {sym} has no state in the table")


# ---- Huffman -------------------------------------------------------------------------------------------
def derive_weights(data):
    """Huffman weights (RFC 8878 4.2.1) for symbols 0..max(data) from the bytes' histogram, code
    lengths limited to 11 bits. At least two symbols get a code."""
    hist = np.bincount(np.frombuffer(bytes(data), dtype=np.uint8), minlength=2).astype(np.int64)
    for i in (0, 1):  # a tree has at least two leaves
        if np.count_nonzero(hist) < 2 and hist[i] == 0:
            hist[i] = 1
    while True:
        heap = [(int(c), i, (i,)) for i, c in enumerate(hist) if c]
        heapq.heapify(heap)
        depth = dict.fromkeys((i for i, c in enumerate(hist) if c), 0)
        while len(heap) > 1:
            a, b = heapq.heappop(heap), heapq.heappop(heap)
            for s in a[2] + b[2]:
                depth[s] += 1
            heapq.heappush(heap, (a[0] + b[0], min(a[1], b[1]), a[2] + b[2]))
        mx = max(depth.values())
        if mx <= 11:
            break
        hist = np.where(hist > 0, np.maximum(hist // 2, 1), 0)  # flatten and retry
    return [mx + 1 - depth[s] if s in depth else 0 for s in range(max(depth) + 1)]


def huf_codes(weights):
    """weights of symbols 0..k (all of them: the last is the one the tree description leaves out) ->
    (max_bits, {symbol: (code, bits)}), the canonical codes of RFC 8878 4.2.1.3."""
    total = sum(1 << (w - 1) for w in weights if w)
    max_bits = total.bit_length() - 1
    assert total == 1 << max_bits, "weights do not sum to a power of two"
    codes, nxt = {}, 0
    for wt in range(1, max_bits + 1):
        for s, w in enumerate(weights):
            if w == wt:
                codes[s] = (nxt >> (wt - 1), max_bits + 1 - wt)
                nxt += 1 << (wt - 1)
    return max_bits, codes


def huf_stream(codes, data, defect=None):
    b = Bits()
    if defect == "leftover":
        b.put(0, 1)
    for s in reversed(bytes(data)):
        c, k = codes[s]
        b.put(c, k)
    out = b.backward()
    if defect == "zero_last":
        out += b"\0"
    if defect == "short":
        assert len(out) > 1
        out = out[1:]
    return out


def tree_direct(weights):
    """Tree description with 4-bit weights; `weights` leaves out the last symbol's."""
    assert 1 <= len(weights) <= 128
    w = list(weights) + [0]
    return bytes([127 + len(weights)]) + bytes((w[i] << 4) | w[i + 1] for i in range(0, len(weights), 2))


def tree_fse(weights, log=6, norm=None):
    """Tree description with FSE-compressed weights (two interleaved states)."""
    n = len(weights)
    assert 2 <= n <= 255
    norm = norm or derive_norm(weights, log)
    tab = fse_table(norm, log)
    b = Bits()
    # decoding order: weight i comes from state (i & 1); the update after weight n - 2 finds the
    # stream empty, which ends the decoding (so it must ask for at least one bit)
    nxt = [None, None]
    first = [0, 0]
    for i in range(n - 1, -1, -1):
        u = _state_for(tab, weights[i], nxt[i & 1], need_bits=(i == n - 2))
        if nxt[i & 1] is not None:
            b.put(nxt[i & 1] - tab[u][2], tab[u][1])
        nxt[i & 1] = u
        first[i & 1] = u
    b.put(first[1], log)
    b.put(first[0], log)
    body = ncount_bytes(norm, log) + b.backward()
    assert len(body) < 128
    return bytes([len(body)]) + body


# ---- literals section ----------------------------------------------------------------------------------
class Lit:
    """The literals section of a compressed block.
    kind: "raw", "rle", "huf" (Compressed_Literals_Block), "treeless"; sf: Size_Format 0..3;
    data: the literal bytes (rle: data[0] repeated len(data) times);
    weights: Huffman weights of symbols 0..k-1 (symbol k's is implied), None: from the data;
    tree: "direct" / "fse" / None (direct while it fits), fse_log: accuracy of the weights' table;
    stream_defect: "zero_last" / "leftover" / "short" (first stream); jump: override of the jump
    table's three sizes; tree_bytes: a tree description taken as it is."""

    def __init__(self, kind="raw", data=b"", sf=None, weights=None, tree=None, fse_log=6, stream_defect=None, jump=None,
                 tree_bytes=None, regen=None):
        self.kind, self.data, self.sf, self.weights, self.tree = kind, bytes(data), sf, weights, tree
        self.fse_log, self.stream_defect, self.jump, self.tree_bytes, self.regen = fse_log, stream_defect, jump, tree_bytes, regen


def _lit_bytes(lit, st):
    n = len(lit.data) if lit.regen is None else lit.regen
    if lit.kind in ("raw", "rle"):
        lt = 0 if lit.kind == "raw" else 1
        sf = lit.sf if lit.sf is not None else ((n & 1) << 1 if n < 32 else 1 if n < 4096 else 3)
        if sf in (0, 2):  # one Size_Format bit: the field's upper bit is the size's lowest (2: an odd size)
            assert n < 32 and (n & 1) == sf >> 1, "a 1-byte header reads as Size_Format 0 (even size) or 2 (odd)"
            hdr = bytes([(n << 3) | lt])
        elif sf == 1:
            assert n < 4096
            hdr = bytes([((n & 15) << 4) | (1 << 2) | lt, n >> 4])
        else:
            assert n < (1 << 20)
            hdr = bytes([((n & 15) << 4) | (3 << 2) | lt, (n >> 4) & 255, n >> 12])
        return hdr + (lit.data if lt == 0 else lit.data[:1] or b"\0")
    lt = 2 if lit.kind == "huf" else 3
    if lt == 2:
        if lit.tree_bytes is not None:
            tree = lit.tree_bytes
            weights = lit.weights
        else:
            if lit.weights is None:
                weights = derive_weights(lit.data)
                listed = weights[:-1]
            else:
                listed = lit.weights
                total = sum(1 << (w - 1) for w in listed if w)
                left = (1 << total.bit_length()) - total
                weights = list(listed) + [left.bit_length()]
            how = lit.tree or ("direct" if len(listed) <= 128 else "fse")
            tree = tree_direct(listed) if how == "direct" else tree_fse(listed, lit.fse_log)
        if weights is not None:
            st["huf"] = huf_codes(weights)[1]
    else:
        tree = b""
    codes = st.get("huf")
    if codes is None:  # treeless with nothing to repeat (an illegal frame): any stream will do
        codes = {s: (s & 1, 1) for s in range(256)}
    sf = lit.sf if lit.sf is not None else (0 if n < 6 else 1 if n < 1024 else 2 if n < 16384 else 3)
    if sf == 0:
        body = tree + huf_stream(codes, lit.data, lit.stream_defect)
    else:
        seg = (n + 3) // 4
        parts = [huf_stream(codes, lit.data[i * seg:(i + 1) * seg], lit.stream_defect if i == 0 else None) for i in range(4)]
        jump = lit.jump or [len(p) for p in parts[:3]]
        body = tree + b"".join(j.to_bytes(2, "little") for j in jump) + b"".join(parts)
    c = len(body)
    width = {0: 10, 1: 10, 2: 14, 3: 18}[sf]
    assert n < (1 << width) and c < (1 << width), (n, c, sf)
    v = lt | (sf << 2) | (n << 4) | (c << (4 + width))
    return v.to_bytes({0: 3, 1: 3, 2: 4, 3: 5}[sf], "little") + body


# ---- sequences section ---------------------------------------------------------------------------------
def nseq_bytes(n, form=None):
    """Number_of_Sequences in its 1-, 2- or 3-byte form (form None: the shortest)."""
    form = form or (1 if n < 128 else 2 if n < 0x7F00 else 3)
    if form == 1:
        assert n < 128
        return bytes([n])
    if form == 2:
        assert n < 0x7F00
        return bytes([128 + (n >> 8), n & 255])
    assert n >= 0x7F00
    return bytes([255]) + (n - 0x7F00).to_bytes(2, "little")


class Tab:
    """One sequence table: mode PREDEF / RLE / FSE / REPEAT; FSE: accuracy `log` and the normalized
    counts `norm` (None: derived from the block's codes; lt1: rare symbols get -1); RLE: the symbol
    (None: the block's). raw_log writes another accuracy log than the table has (a defect)."""

    def __init__(self, mode=PREDEF, log=None, norm=None, lt1=False, sym=None, raw_log=None):
        self.mode, self.log, self.norm, self.lt1, self.sym, self.raw_log = mode, log, norm, lt1, sym, raw_log


def _seq_codes(seqs):
    out = []
    for ll, ml, ofv in seqs:
        lc, mc, oc = ll_code(ll), ml_code(ml), of_code(ofv)
        out.append((lc, ll - LL_BASE[lc], LL_BITS[lc], oc, ofv - (1 << oc), oc, mc, ml - ML_BASE[mc], ML_BITS[mc]))
    return out


def seq_bits(seqs, tabs):
    """Stream bits each sequence consumes (extra bits + the state updates after it), given the
    decoding tables {kind: table} and the states the encoder picks."""
    return _seq_stream(seqs, tabs)[1]


def _seq_stream(seqs, tabs, defect=None):
    codes = _seq_codes(seqs)
    n = len(codes)
    logs = {k: (len(tabs[k]).bit_length() - 1) for k in tabs}
    b = Bits()
    if defect == "leftover":
        b.put(0, 1)
    nxt = {"ll": None, "of": None, "ml": None}
    cost = [0] * n
    for i in range(n - 1, -1, -1):
        lc, lx, lb, oc, ox, ob, mc, mx, mb = codes[i]
        st = {}
        for k, c in (("ll", lc), ("ml", mc), ("of", oc)):
            st[k] = _state_for(tabs[k], c, nxt[k])
        if i < n - 1:  # updates are read LL, ML, OF: written OF, ML, LL
            for k in ("of", "ml", "ll"):
                _, nb, base = tabs[k][st[k]]
                b.put(nxt[k] - base, nb)
                cost[i] += nb
        b.put(lx, lb)  # extra bits are read OF, ML, LL
        b.put(mx, mb)
        b.put(ox, ob)
        cost[i] += lb + mb + ob
        nxt = st
    b.put(nxt["ml"], logs["ml"])  # initial states are read LL, OF, ML
    b.put(nxt["of"], logs["of"])
    b.put(nxt["ll"], logs["ll"])
    out = b.backward()
    if defect == "zero_last":
        out += b"\0"
    if defect == "overrun":
        assert len(out) > 1
        out = out[1:]
    return out, cost


def _seq_section(seqs, tabs, st, nseq_form=None, modes_reserved=0, defect=None, nseq_override=None):
    """Sequences_Section bytes; `tabs` {kind: Tab}; st carries the previous block's tables."""
    if not seqs:
        return nseq_bytes(0, nseq_form)
    codes = _seq_codes(seqs)
    used = {"ll": [c[0] for c in codes], "of": [c[3] for c in codes], "ml": [c[6] for c in codes]}
    desc, modes, dec = b"", 0, {}
    for k, shift in (("ll", 6), ("of", 4), ("ml", 2)):
        t = tabs.get(k) or Tab()
        defn, deflog, maxlog, _ = KINDS[k]
        modes |= t.mode << shift
        if t.mode == PREDEF:
            dec[k] = fse_table(defn, deflog)
        elif t.mode == RLE:
            sym = used[k][0] if t.sym is None else t.sym
            desc += bytes([sym])
            dec[k] = rle_table(sym)
        elif t.mode == FSE:
            log = t.log or 5
            norm = t.norm or derive_norm(used[k], log, t.lt1)
            desc += ncount_bytes(norm, log, t.raw_log)
            dec[k] = fse_table(norm, log)
        else:
            dec[k] = st["tabs"].get(k) or fse_table(defn, deflog)  # (nothing to repeat: an illegal frame)
        st["tabs"][k] = dec[k]
    stream, cost = _seq_stream(seqs, dec, defect)
    st["seq_bits"] = max(st.get("seq_bits", 0), max(cost))
    n = len(seqs) if nseq_override is None else nseq_override
    return nseq_bytes(n, nseq_form) + bytes([modes | modes_reserved]) + desc + stream


# ---- execution (the expected output) -------------------------------------------------------------------
def execute(out, frame0, lits, seqs, rep):
    """Run one block's sequences over `out` (bytearray; the frame began at frame0): literal copy,
    match copy, repeat offsets (RFC 8878 3.1.1.5)."""
    lp = 0
    for ll, ml, ofv in seqs:
        assert lp + ll <= len(lits), "sequences use more literals than the block has"
        out += lits[lp:lp + ll]
        lp += ll
        if ofv > 3:
            off = ofv - 3
            rep[:] = [off, rep[0], rep[1]]
        else:
            idx = ofv - 1 + (1 if ll == 0 else 0)
            if idx == 0:
                off = rep[0]
            elif idx == 3:
                off = rep[0] - 1
                rep[:] = [off, rep[0], rep[1]]
            elif idx == 1:
                off = rep[1]
                rep[:] = [off, rep[0], rep[2]]
            else:
                off = rep[2]
                rep[:] = [off, rep[0], rep[1]]
        assert 0 < off <= len(out) - frame0, "offset outside the frame"
        if off >= ml:
            start = len(out) - off
            out += out[start:start + ml]
        else:
            pat = bytes(out[len(out) - off:])
            out += (pat * (ml // off + 1))[:ml]
    out += lits[lp:]


# ---- frames ---------------------------------------------------------------------------------------------
class Frame:
    """One Zstandard frame under construction.

    single: Single_Segment (no Window_Descriptor); window: (exponent, mantissa) of the descriptor
    (default (7, 0): 128 KiB, so blocks of any legal size pass Block_Maximum_Size);
    fcs_bytes: width of Frame_Content_Size, 0 / 1 / 2 / 4 / 8 (None: the smallest that holds the
    content with Single_Segment, else no field; 0 needs a Window_Descriptor); fcs: the value written (None: the content's size);
    did_bytes / did: the Dictionary_ID field; checksum: XXH64 content checksum; reserved: the
    reserved bit of the frame header descriptor.
    `check=False` skips the executor's legality asserts (for frames that are illegal on purpose; their
    expected output is meaningless)."""

    def __init__(self, single=False, window=(7, 0), fcs_bytes=None, fcs=None, did_bytes=0, did=0, checksum=False,
                 reserved=False, check=True):
        self.single, self.window, self.fcs_bytes, self.fcs = single, window, fcs_bytes, fcs
        self.did_bytes, self.did, self.checksum, self.reserved, self.check = did_bytes, did, checksum, reserved, check
        self.body = bytearray()
        self.out = bytearray()
        self.rep = [1, 4, 8]
        self.st = {"tabs": {}}
        self.closed = False

    def _block(self, btype, size, payload, last):
        self.body += ((size << 3) | (btype << 1) | int(last)).to_bytes(3, "little") + payload
        self.closed = self.closed or last
        return self

    def raw(self, data, last=False):
        self.out += data
        return self._block(0, len(data), bytes(data), last)

    def rle(self, byte, n, last=False):
        self.out += bytes([byte]) * n
        return self._block(1, n, bytes([byte]), last)

    def reserved_block(self, size=1, payload=b"\0", last=False):
        return self._block(3, size, payload, last)

    def compressed(self, lits=None, seqs=(), ll=None, of=None, ml=None, last=False, nseq_form=None, modes_reserved=0,
                   seq_defect=None, nseq_override=None, trailing=b""):
        """A Compressed_Block: `lits` (Lit), `seqs` [(literal_length, match_length, offset_value)],
        the three tables (Tab; default predefined). trailing: bytes appended to the block."""
        lits = lits or Lit()
        seqs = list(seqs)
        payload = _lit_bytes(lits, self.st)
        payload += _seq_section(seqs, {"ll": ll, "of": of, "ml": ml}, self.st, nseq_form, modes_reserved, seq_defect,
                                nseq_override) + trailing
        data = lits.data if lits.kind != "rle" else lits.data[:1] * len(lits.data)
        if self.check:
            before = len(self.out)
            execute(self.out, 0, data, seqs, self.rep)
            assert len(self.out) - before <= 131072, "a block regenerates at most 128 KiB"
        return self._block(2, len(payload), payload, last)

    def raw_compressed(self, payload, last=False):
        """A Compressed_Block whose content is given byte for byte."""
        return self._block(2, len(payload), bytes(payload), last)

    @property
    def seq_bits(self):
        """The most stream bits one sequence of the frame consumes."""
        return self.st.get("seq_bits", 0)

    def finish(self):
        """-> (frame bytes, expected output)."""
        if not self.closed:  # mark the last block
            assert self.body, "a frame needs a block"
            # find the last block header by re-walking the body
            p = 0
            while True:
                h = int.from_bytes(self.body[p:p + 3], "little")
                size = 1 if (h >> 1) & 3 == 1 else h >> 3
                if p + 3 + size >= len(self.body):
                    break
                p += 3 + size
            self.body[p] |= 1
        n = len(self.out)
        fb = self.fcs_bytes
        if fb is None:  # Single_Segment: the smallest field; else none
            fb = 0 if not self.single else 1 if n < 256 else 2 if n < 65792 else 4
        assert fb or not self.single, "Single_Segment always carries a Frame_Content_Size"
        if fb == 1:
            assert self.single, "a 1-byte Frame_Content_Size exists only with Single_Segment"
        flag = {0: 0, 1: 0, 2: 1, 4: 2, 8: 3}[fb]
        didf = {0: 0, 1: 1, 2: 2, 4: 3}[self.did_bytes]
        fhd = (flag << 6) | (int(self.single) << 5) | (int(self.reserved) << 3) | (int(self.checksum) << 2) | didf
        hdr = MAGIC.to_bytes(4, "little") + bytes([fhd])
        if not self.single:
            hdr += bytes([(self.window[0] << 3) | self.window[1]])
        hdr += self.did.to_bytes(self.did_bytes, "little")
        v = n if self.fcs is None else self.fcs
        if fb:
            hdr += (v - 256 if fb == 2 else v).to_bytes(fb, "little")
        tail = (pqref.xxh64(bytes(self.out)) & 0xFFFFFFFF).to_bytes(4, "little") if self.checksum else b""
        return hdr + bytes(self.body) + tail, bytes(self.out)


def skippable(n=5, nibble=3):
    return (0x184D2A50 | nibble).to_bytes(4, "little") + n.to_bytes(4, "little") + bytes(range(n))


def concat(*parts):
    """Frames (as (bytes, expected) pairs) and skippable frames (bytes) one after another."""
    f, e = b"", b""
    for p in parts:
        if isinstance(p, tuple):
            f += p[0]
            e += p[1]
        else:
            f += p
    return f, e


def window_size(exp, mant):
    base = 1 << (10 + exp)
    return base + base // 8 * mant
