"""Hand-built DELTA_BINARY_PACKED pages: a byte-level page builder and an independent reader.

build() writes any page DeltaBinaryPackingValuesReader accepts (and pages it refuses): declared widths
that are not minimal, arbitrary width bytes for the unread miniblocks of a last block, over-long
varints, bytes after the last used miniblock, a header count unrelated to the blocks written. It does
not use tools/synth/writer.py.

read() is the plain restatement of the reader in Python integers: DeltaBinaryPackingValuesReader
.initFromPage (parquet-column/.../delta/DeltaBinaryPackingValuesReader.java:59-172),
DeltaBinaryPackingConfig (:30-51), BytesUtils.readUnsignedVarInt / readUnsignedVarLong /
readZigZagVarLong (parquet-common/.../bytes/BytesUtils.java:202-211, 254-269), with Java's int and
long wrap-around and shift masking applied at each step. It does not call the oracle: it is the second
opinion on oracle/pqref.c (tests/test_delta_build.py compares the two on every case).
"""
import math

import numpy as np

from pqgpu.abi import ERR_CORRUPT, ERR_DELTA_CONFIG, ERR_EOF  # error code numbers only

M32, M64 = (1 << 32) - 1, (1 << 64) - 1


def i32(v):
    v &= M32
    return v - (1 << 32) if v >> 31 else v


def i64(v):
    v &= M64
    return v - (1 << 64) if v >> 63 else v


def zigzag64(v):
    """BytesUtils.writeZigZagVarLong's mapping: (v << 1) ^ (v >> 63) as an unsigned 64-bit number."""
    return ((v << 1) ^ (v >> 63)) & M64


# ---- builder ------------------------------------------------------------------------------------------

def varint(u, extra=0):
    """Unsigned LEB128 of u, shortest form, then `extra` more bytes: the last byte gets its
    continuation bit, extra - 1 bytes of 0x80 follow and 0x00 closes (the same value to a reader
    that masks its shifts or not: the added payload bits are all 0)."""
    assert u >= 0 and extra >= 0
    out = bytearray()
    while True:
        b = u & 0x7F
        u >>= 7
        if u:
            out.append(b | 0x80)
        else:
            out.append(b)
            break
    if extra:
        out[-1] |= 0x80
        out += b"\x80" * (extra - 1) + b"\x00"
    return bytes(out)


def _field(u, pad):
    """A header field: `pad` is a number of extra bytes or the field's raw bytes."""
    if isinstance(pad, (bytes, bytearray)):
        return bytes(pad)
    return varint(u, int(pad or 0))


def pack(vals, w):
    """Packer.LITTLE_ENDIAN: value i in bits [i * w, (i + 1) * w), byte 0 bit 0 first."""
    if w == 0:
        return b""
    bits = 0
    for i, v in enumerate(vals):
        assert 0 <= v < (1 << w), (v, w)
        bits |= v << (i * w)
    return bits.to_bytes(len(vals) * w // 8, "little")


def build_ex(block, mbn, total, first, blocks, *, pad=None, trailing=b""):
    """-> (page bytes, [byte offset of each block header]).

    blocks: [(min_delta, widths, deltas)]: `widths` are all mbn width bytes as written (the caller
    chooses what the unused ones hold), `deltas` one list of block / mbn unsigned integers below
    2 ** width per miniblock WRITTEN (the used ones; more, to write out unused miniblocks' data too),
    padding deltas past `total` included.
    pad: {"block" | "mbn" | "total" | "first": extra bytes or raw bytes, "min": {block index: the
    same}} (see varint()). Raw bytes let a field be any byte string, e.g. a varint of 11 or more bytes
    whose late bytes land on Java's masked shifts.
    """
    pad = pad or {}
    mbs = block // mbn if mbn else 0
    out = bytearray()
    out += _field(block, pad.get("block"))
    out += _field(mbn, pad.get("mbn"))
    out += _field(total, pad.get("total"))
    out += _field(zigzag64(first), pad.get("first"))
    pmin = pad.get("min", {})
    offs = []
    for b, (min_delta, widths, deltas) in enumerate(blocks):
        assert len(widths) == mbn and len(deltas) <= mbn
        offs.append(len(out))
        out += _field(zigzag64(min_delta), pmin.get(b))
        out += bytes(widths)
        for m, d in enumerate(deltas):
            assert len(d) == mbs
            out += pack(d, widths[m])
    out += trailing
    return bytes(out), offs


def build(block, mbn, total, first, blocks, *, pad=None, trailing=b""):
    return build_ex(block, mbn, total, first, blocks, pad=pad, trailing=trailing)[0]


# ---- reader -------------------------------------------------------------------------------------------

class _Err(Exception):
    def __init__(self, code):
        self.code = code


class _In:
    """ByteBufferInputStream over one buffer: read() and slice() throw EOFException when short
    (SingleBufferInputStream.java:49-55, 113-125)."""

    def __init__(self, buf, pos):
        self.buf, self.pos = buf, pos

    def read(self):
        if self.pos >= len(self.buf):
            raise _Err(ERR_EOF)
        self.pos += 1
        return self.buf[self.pos - 1]

    def slice(self, n):
        if len(self.buf) - self.pos < n:
            raise _Err(ERR_EOF)
        self.pos += n
        return self.buf[self.pos - n:self.pos]


def read_unsigned_var_int(s):
    """BytesUtils.readUnsignedVarInt :202-211 (int arithmetic: << takes its count mod 32)."""
    value, i = 0, 0
    b = s.read()
    while b & 0x80:
        value = i32(value | ((b & 0x7F) << (i & 31)))
        i += 7
        b = s.read()
    return i32(value | (b << (i & 31)))


def read_unsigned_var_long(s):
    """BytesUtils.readUnsignedVarLong :260-269 (long arithmetic: << takes its count mod 64)."""
    value, i = 0, 0
    b = s.read()
    while b & 0x80:
        value = i64(value | ((b & 0x7F) << (i & 63)))
        i += 7
        b = s.read()
    return i64(value | (b << (i & 63)))


def read_zigzag_var_long(s):
    """BytesUtils.readZigZagVarLong :254-258."""
    raw = read_unsigned_var_long(s)
    temp = i64(i64(raw << 63) >> 63 ^ raw) >> 1
    return i64(temp ^ (raw & i64(1 << 63)))


def _java_int_of_double(x):
    """(int) of a double: NaN -> 0, saturating."""
    if x != x:
        return 0
    return int(max(-2.0**31, min(2.0**31 - 1, x)))


def _init_from_page(s):
    # DeltaBinaryPackingConfig.readConfig :43-45, ctor :34-41
    block = read_unsigned_var_int(s)
    mbn = read_unsigned_var_int(s)
    if mbn == 0:
        mini = math.nan if block == 0 else math.copysign(math.inf, block)
    else:
        mini = block / mbn
    if mini != mini or math.isinf(mini) or math.fmod(mini, 8.0) != 0:
        raise _Err(ERR_DELTA_CONFIG)  # Preconditions.checkArgument(miniSize % 8 == 0)
    mbs = _java_int_of_double(mini)
    total = read_unsigned_var_int(s)
    # allocateValuesBuffer :83-87
    if mbs == 0:
        q = math.nan if total == 0 else math.copysign(math.inf, total)
    else:
        q = total / mbs
    count = _java_int_of_double(q if q != q or math.isinf(q) else float(math.ceil(q)))
    size = i32(count * mbs + 1)
    if size < 0:
        raise _Err(ERR_CORRUPT)  # NegativeArraySizeException
    if mbn < 0:
        raise _Err(ERR_CORRUPT)  # new int[miniBlockNumInABlock]
    buf = [0] * size
    buffered = 0
    buf[buffered] = read_zigzag_var_long(s)
    buffered += 1
    while buffered < total:
        # loadNewBlockToBuffer :121-143
        min_delta = read_zigzag_var_long(s)
        widths = [s.read() for _ in range(mbn)]  # readBitWidthsForMiniBlocks :164-172
        i = 0
        while i < mbn and buffered < total:
            w = widths[i]
            if w > 64:
                raise _Err(ERR_CORRUPT)  # Packer.newBytePackerForLong: no packer of that width
            mask = (1 << w) - 1
            for _ in range(0, mbs, 8):  # unpackMiniBlock :150-154, unpack8Values :156-162
                bits = int.from_bytes(s.slice(w), "little")
                if w:
                    for k in range(8):
                        buf[buffered + k] = i64((bits >> (k * w)) & mask)
                buffered += 8
            i += 1
        unpacked = i * mbs
        for j in range(buffered - unpacked, buffered):
            buf[j] = i64(buf[j] + i64(min_delta + buf[j - 1]))
        if mbs <= 0:  # (valuesBuffered never grows: the real reader loops until the stream ends)
            continue
    return buf[:max(total, 0)]


def read(page, pos=0):
    """initFromPage on page[pos:]: (values as int64, bytes consumed) or the error code the reader's
    exception maps to (EOFException: EOF; the config precondition: DELTA_CONFIG; a negative array
    size or a width without a packer: CORRUPT)."""
    s = _In(bytes(page), pos)
    try:
        vals = _init_from_page(s)
    except _Err as e:
        return e.code
    return np.array(vals, dtype=np.int64), s.pos - pos
