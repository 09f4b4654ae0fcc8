"""The arithmetic of k_crc_tiles and k_crc_fold (csrc/pqgpu_crc.hip, csrc/pqgpu_crc.h) restated lane by lane in
plain Python and held against zlib.crc32: four states per lane, rows of 1 KiB from the 16-byte boundary below the
tile, bytes masked to zero before the first and after the last byte, the start value as data on the first four
byte positions, the move of every lane's value to the tile's nominal end (backwards where that lies before the
lane's position), Horner's rule over more than 64 partials and the final move back to the job's end. No device
and no library: it pins the algebra the kernels rely on, at T = 4096 so that many-tile jobs stay small."""
import os
import zlib

POLY, X0, ORDER, ROW = 0xEDB88320, 0x80000000, 0xFFFFFFFF, 1024


def mul(a, b):
    """a * b modulo P, reflected bit order (bit 31 = x^0)."""
    p, m = 0, X0
    while m:
        if a & m:
            p ^= b
        b = (b >> 1) ^ POLY if b & 1 else b >> 1
        m >>= 1
    return p


X2N = [X0 >> 1]  # x^(2^k)
for _ in range(31):
    X2N.append(mul(X2N[-1], X2N[-1]))


def x8n(n):
    """x^(8 n); exponents count modulo the order of x, 2^32 - 1."""
    n %= ORDER
    p, k = X0, 3
    while n:
        if n & 1:
            p = mul(X2N[k & 31], p)
        n >>= 1
        k += 1
    return p


def x8n_back(n):
    return x8n(ORDER - n % ORDER)


def tables(T):
    """crc_build_tables: step4, row, xp8, xt."""
    x32, xrow, x8, xtile = x8n(4), x8n(ROW), x8n(1), x8n(T)
    step4 = [mul(b << (8 * k), x32) for k in range(4) for b in range(256)]
    row = [mul(b << (8 * k), xrow) for k in range(4) for b in range(256)]
    xp8, p = [], x8n_back(T)
    for _ in range(2 * T):
        xp8.append(p)
        p = mul(p, x8)
    xt, p = [], X0
    for _ in range(65):
        xt.append(p)
        p = mul(p, xtile)
    return step4, row, xp8, xt


def lookup4(t, v):
    return t[v & 255] ^ t[256 + ((v >> 8) & 255)] ^ t[512 + ((v >> 16) & 255)] ^ t[768 + (v >> 24)]


def byte_mask(lo, hi):
    lo, hi = max(lo, 0), min(hi, 4)
    if hi <= lo:
        return 0
    return (0xFFFFFFFF >> (8 * (4 - hi))) & (0xFFFFFFFF << (8 * lo)) & 0xFFFFFFFF


def tile_partial(buf, base_addr, start, size, first, T, tabs):
    """k_crc_tiles for one tile; base_addr stands for the address of d_bytes."""
    step4, row, xp8, _ = tabs
    n4 = (len(buf) + 3) & ~3
    pa = base_addr + start
    base = max(pa & ~15, base_addr)
    lead = pa - base
    span = lead + size
    n_rows = (span + ROW - 1) // ROW
    n_rec = min(n4 - (base - base_addr), n_rows * ROW)
    at = base - base_addr

    def ld32(o):  # range-checked: nothing at or past n_rec is read
        if o + 4 > n_rec:
            return 0
        b = buf[at + o: at + o + 4]
        return int.from_bytes(b + bytes(4 - len(b)), "little")
    total = 0
    for lane in range(64):
        s = [0, 0, 0, 0]
        for r in range(n_rows):
            o = r * ROW + 16 * lane
            d = [ld32(o + 4 * k) for k in range(4)]
            if o < lead or o + 16 > span:
                d = [d[k] & byte_mask(lead - o - 4 * k, span - o - 4 * k) for k in range(4)]
            if first and r == 0 and lane < 2:
                d = [d[k] ^ byte_mask(lead - o - 4 * k, lead - o - 4 * k + 4) for k in range(4)]
            s = [lookup4(row, s[k] ^ d[k]) for k in range(4)]
        c = lookup4(step4, s[0]) ^ s[1]
        c = lookup4(step4, c) ^ s[2]
        c = lookup4(step4, c) ^ s[3]
        move = lead + T - n_rows * ROW - 16 * lane - 12
        assert -2044 <= move <= T - 1021
        total ^= mul(c, xp8[move + T])
    return total


def job_crc(buf, base_addr, off, size, T, tabs):
    """k_crc_fold over the job's tile partials."""
    _, _, xp8, xt = tabs
    nt = (size + T - 1) // T
    if nt == 0:
        return 0
    parts = [tile_partial(buf, base_addr, off + t * T, min(T, size - t * T), t == 0, T, tabs) for t in range(nt)]
    total = 0
    for lane in range(64):
        acc, last = 0, lane
        for t in range(lane, nt, 64):
            acc = (0 if t == lane else mul(acc, xt[64])) ^ parts[t]
            last = t
        if lane < nt:
            acc = mul(acc, xt[nt - 1 - last])
        total ^= acc
    return mul(total, xp8[size - nt * T + T]) ^ 0xFFFFFFFF


def test_moves_backwards():
    assert mul(x8n(5), x8n_back(5)) == X0 and mul(x8n(2**33 + 7), x8n_back(2**33 + 7)) == X0
    assert x8n(ORDER) == X0  # the order of x divides 2^32 - 1


def test_tiles_and_fold_against_zlib():
    T = 4096
    tabs = tables(T)
    buf = os.urandom(70 * T + 100)
    cases = [(o, s) for s in (0, 1, 2, 3, 4, 5, 7, 15, 16, 17, 1023, 1024, 1025, T - 1, T, T + 1, 2 * T + 1)
             for o in (0, 1, 3, 13, 15, 16, 29)]
    cases += [(7, 66 * T + 3), (len(buf) - 5, 5), (len(buf) - 1, 1), (len(buf), 0)]
    for base_addr in (0x1000, 0x1004, 0x100C):  # d_bytes is 4-byte aligned, not more
        for o, s in cases:
            got, ref = job_crc(buf, base_addr, o, s, T, tabs), zlib.crc32(buf[o:o + s])
            assert got == ref, (base_addr, o, s, hex(got), hex(ref))
