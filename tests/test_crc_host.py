"""Page checksums, host side (include/pqgpu.h, "page checksums"): pqg_crc32_combine against zlib and against
an independent GF(2) square-and-multiply, pqg_crc_jobs_from_headers on reference-written and writer-made
chunks, the crc fields framing.read_column_chunk keeps, and the job struct's size. No device is needed."""
import ctypes as C
import os
import zlib

import numpy as np
import pytest

import fixtures
import thrift_compact
from pqgpu import abi, framing, native
from tools.synth import writer

T = abi.CRC_TILE_BYTES
POLY = 0xEDB88320


# ---- an independent reference for lengths no buffer can have: polynomials over GF(2) modulo P in the
# reflected bit order (bit 31 = x^0), x^(8 n) by square-and-multiply on the exponent's bits
def gf_mul(a, b):
    p = 0
    for i in range(32):
        if (a >> (31 - i)) & 1:
            p ^= b
        b = (b >> 1) ^ (POLY if b & 1 else 0)
    return p


def gf_x_pow(e):
    r, sq = 0x80000000, 0x40000000  # x^0, x^1
    while e:
        if e & 1:
            r = gf_mul(r, sq)
        sq = gf_mul(sq, sq)
        e >>= 1
    return r


def ref_combine(crc_a, crc_b, len_b):
    return gf_mul(crc_a, gf_x_pow(8 * len_b)) ^ crc_b


def combine(a, b, n):
    return native.lib().pqg_crc32_combine(a, b, n)


def test_abi_has_the_crc_job():
    assert C.sizeof(abi.CrcJob) == 24 and abi.CRC_JOB_DTYPE.itemsize == 24
    assert [f[0] for f in abi.CrcJob._fields_] == list(abi.CRC_JOB_DTYPE.names)
    assert T in (4096, 8192, 16384, 32768) and abi.CRC_VERIFY == 1
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pqgpu.h")) as f:
        assert f"#define PQG_CRC_TILE_BYTES {T} " in f.read()


def test_combine_random_splits():
    rng = np.random.default_rng(5)
    for _ in range(200):
        buf = rng.integers(0, 256, size=int(rng.integers(0, 5000)), dtype=np.uint8).tobytes()
        cut = int(rng.integers(0, len(buf) + 1))
        a, b = buf[:cut], buf[cut:]
        assert combine(zlib.crc32(a), zlib.crc32(b), len(b)) == zlib.crc32(buf)


@pytest.mark.parametrize("fill", [None, 0x00, 0xFF])
def test_combine_lengths_around_the_tile(fill):
    rng = np.random.default_rng(6)
    for len_b in (0, 1, 3, 4, 5, T - 1, T, T + 1):
        for len_a in (0, 1, 7, T + 3):
            n = len_a + len_b
            buf = rng.integers(0, 256, size=n, dtype=np.uint8).tobytes() if fill is None else bytes([fill]) * n
            a, b = buf[:len_a], buf[len_a:]
            assert combine(zlib.crc32(a), zlib.crc32(b), len_b) == zlib.crc32(buf), (len_a, len_b)
    assert combine(0x12345678, 0x0BADF00D, 0) == 0x12345678 ^ 0x0BADF00D  # zlib's identity for an empty B


def test_combine_beyond_memory():
    """Lengths no buffer here can have, against the square-and-multiply above (itself checked against zlib)."""
    rng = np.random.default_rng(7)
    for n in (1, 5, 1000, 70001):
        a, b = os.urandom(33), bytes(rng.integers(0, 256, size=n, dtype=np.uint8))
        assert ref_combine(zlib.crc32(a), zlib.crc32(b), n) == zlib.crc32(a + b)
    for len_b in (2**32 - 1, 2**35 + 3, 2**32 - 2, 2**32, 2**63 + 11):
        for _ in range(4):
            ca, cb = (int(v) for v in rng.integers(0, 2**32, size=2))
            assert combine(ca, cb, len_b) == ref_combine(ca, cb, len_b), len_b


# ---- pqg_crc_jobs_from_headers ------------------------------------------------------------------------
def raw_chunk(name, c):
    buf = np.fromfile(os.path.join(fixtures.GOLDEN, name + ".parquet"), dtype=np.uint8).tobytes()
    return buf[c["start"]: c["start"] + c["length"]]


def written_chunks():
    """Writer-made chunks, V1 and V2, with a dictionary page."""
    rng = np.random.default_rng(8)
    dl = (rng.random(3000) > 0.25).astype(np.uint8)
    vals = rng.integers(0, 40, size=int(dl.sum())).astype(np.int64) * 1000003
    return [writer.write_column_chunk(abi.INT64, vals, abi.RLE_DICTIONARY, def_levels=dl, max_def=1, version=ver,
                                      page_rows=700) for ver in (1, 2)]


def chunk_inputs():
    """(label, raw chunk bytes, value count, carries CRCs)"""
    out = []
    for name, c in fixtures.chunk_cases():
        if name in ("test-append_1", "test-append_2"):
            out.append((f"{name}/{c['key']}", raw_chunk(name, c), c["num_values"], True))
    for ch in written_chunks():
        for crc in (True, False):
            out.append((f"written v{ch.pages[0].version} crc={crc}", thrift_compact.chunk_bytes(ch, with_crc=crc),
                        ch.num_slots, crc))
    return out


def jobs_from_headers(hdrs, chunk_offset=0, capacity=None):
    L = native.lib()
    arr = (abi.PageHeader * max(len(hdrs), 1))(*hdrs)
    cap = len(hdrs) if capacity is None else capacity
    jobs = (abi.CrcJob * max(cap, 1))()
    hoj = (C.c_int32 * max(cap, 1))()
    n, st = C.c_int(-1), abi.Status()
    rc = L.pqg_crc_jobs_from_headers(C.addressof(arr), len(hdrs), chunk_offset, C.addressof(jobs), C.addressof(hoj), cap,
                                     C.byref(n), C.byref(st))
    return rc, st, n.value, jobs, hoj


def test_jobs_from_headers():
    inputs = chunk_inputs()
    assert sum(1 for i in inputs if i[3]) >= 6
    for label, raw, nv, has_crc in inputs:
        rc, st, hdrs = framing.frame_chunk_native(raw, nv, verify_crc=False)
        assert rc == abi.OK, (label, st.message)
        want = [(i, h) for i, h in enumerate(hdrs) if h.has_crc]
        assert bool(want) == has_crc, label
        if has_crc:
            assert len(want) == len(hdrs)  # the dictionary page too
        base = 4096 + 7
        rc, st, n, jobs, hoj = jobs_from_headers(hdrs, chunk_offset=base)
        assert rc == abi.OK and n == len(want), label
        for j, (i, h) in enumerate(want):
            J = jobs[j]
            assert (J.offset, J.size, J.expected, J.flags, J.reserved) == (base + h.body_offset, h.compressed_page_size,
                                                                           h.crc, abi.CRC_VERIFY, 0), (label, j)
            assert hoj[j] == i
            body = raw[h.body_offset: h.body_offset + h.compressed_page_size]
            assert zlib.crc32(body) == J.expected, (label, j)
        # the capacity protocol: too small -> INVALID_ARG with the count needed; NULL header_of_job is fine
        if want:
            rc, st, n, _, _ = jobs_from_headers(hdrs, capacity=len(want) - 1)
            assert rc == abi.ERR_INVALID_ARG and n == len(want) and st.value_index == len(want), label
            rc, st, n, _, _ = jobs_from_headers(hdrs, capacity=0)
            assert rc == abi.ERR_INVALID_ARG and st.value_index == len(want)
        jobs2 = (abi.CrcJob * max(len(want), 1))()
        n2 = C.c_int(0)
        arr = (abi.PageHeader * max(len(hdrs), 1))(*hdrs)
        assert native.lib().pqg_crc_jobs_from_headers(C.addressof(arr), len(hdrs), 0, C.addressof(jobs2), None, len(want),
                                                      C.byref(n2), None) == abi.OK and n2.value == len(want)


def test_jobs_from_headers_mixed_and_refusals():
    ch = written_chunks()[1]
    raw = thrift_compact.chunk_bytes(ch, with_crc=True)
    _, _, hdrs = framing.frame_chunk_native(raw, ch.num_slots, verify_crc=False)
    assert len(hdrs) >= 4
    hdrs[1].has_crc = 0
    hdrs[3].has_crc = 0
    rc, _, n, jobs, hoj = jobs_from_headers(hdrs)
    keep = [i for i in range(len(hdrs)) if i not in (1, 3)]
    assert rc == abi.OK and n == len(keep) and [hoj[j] for j in range(n)] == keep
    assert jobs_from_headers([])[:3:2] == (abi.OK, 0)
    L = native.lib()
    n = C.c_int(0)
    assert L.pqg_crc_jobs_from_headers(None, 2, 0, None, None, 0, C.byref(n), None) == abi.ERR_INVALID_ARG
    arr = (abi.PageHeader * len(hdrs))(*hdrs)
    assert L.pqg_crc_jobs_from_headers(C.addressof(arr), len(hdrs), 0, None, None, 4, C.byref(n), None) == abi.ERR_INVALID_ARG
    assert L.pqg_crc_jobs_from_headers(C.addressof(arr), len(hdrs), 0, None, None, 0, None, None) == abi.ERR_INVALID_ARG


# ---- framing.read_column_chunk keeps the header's crc ---------------------------------------------------
def test_read_column_chunk_keeps_crc():
    seen = 0
    for name, c in fixtures.chunk_cases():
        if name not in ("test-append_1", "test-append_2"):
            continue
        ch, _ = fixtures.load_chunk(name, c)
        if ch.dict_page is not None:
            assert ch.dict_crc == zlib.crc32(ch.dict_page)
        for pg in ch.pages:
            assert pg.crc == zlib.crc32(pg.body)
            assert 0 <= pg.crc < 2**32
            seen += 1
    assert seen >= 4
    for ch in written_chunks():
        for crc in (True, False):
            raw = thrift_compact.chunk_bytes(ch, with_crc=crc)
            got = framing.read_column_chunk(raw, 0, len(raw), abi.INT64, max_def=1, num_values=ch.num_slots)
            assert len(got.pages) == len(ch.pages) and got.dict_page == ch.dict_page
            assert got.dict_crc == (zlib.crc32(ch.dict_page) if crc else None)
            assert [p.crc for p in got.pages] == [zlib.crc32(p.body) if crc else None for p in ch.pages]
    # a checksum with the top bit set comes back unsigned
    pg = ch.pages[0]
    body = bytearray(pg.body)
    while zlib.crc32(bytes(body)) < 2**31:
        body[-1] = (body[-1] + 1) & 0xFF
    import copy
    q = copy.copy(pg)
    q.body = bytes(body)
    raw = thrift_compact.page_header_of(q, zlib.crc32(q.body)) + q.body
    got = framing.read_column_chunk(raw, 0, len(raw), abi.INT64, max_def=1)
    assert got.pages[0].crc == zlib.crc32(q.body) >= 2**31
