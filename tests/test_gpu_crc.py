"""Page checksums on the device (pqg_crc32_pages / pqg_crc32_sync, Decoder.crc32, Decoder.upload_chunks(verify_crc=True))
against zlib.crc32, which is java.util.zip.CRC32. Sizes are chosen around the kernel's own seams: its 16-byte lane
slices, its 1 KiB rows, and the tile T = PQG_CRC_TILE_BYTES one wave checksums; more than 64 tiles make the fold's
lanes take a second partial."""
import copy
import ctypes as C
import os
import zlib

import numpy as np
import pytest
import torch

import fixtures
import thrift_compact
from helpers import assert_same
from pqgpu import abi, framing, native
from test_crc_host import jobs_from_headers, raw_chunk, written_chunks
from test_gpu_take import busy_stream
from tools.synth import writer

pytestmark = pytest.mark.gpu
T = abi.CRC_TILE_BYTES
SIZES = [0, 1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, T - 1, T, T + 1, 2 * T - 1, 2 * T,
         2 * T + 1, 3 * T + 5]


def job_table(rows):
    """rows: (offset, size[, expected[, flags[, reserved]]])"""
    t = np.zeros(len(rows), dtype=abi.CRC_JOB_DTYPE)
    for j, r in enumerate(rows):
        r = tuple(r) + (0,) * (5 - len(r))
        t[j] = r
    return t


def crc_pages(decoder, d_bytes, table, want_crc=True, n_bytes=None):
    """One pqg_crc32_pages + pqg_crc32_sync. Returns (rc of the call, crcs, statuses, rc of the sync, status)."""
    n = len(table)
    d_crc = torch.full((max(n, 1),), 0x5A5A5A5A, dtype=torch.int32, device=decoder.device)
    d_status = torch.full((max(n, 1),), -7, dtype=torch.int32, device=decoder.device)
    torch.cuda.synchronize()
    L = native.lib()
    rc = L.pqg_crc32_pages(decoder.ctx, d_bytes.data_ptr(), d_bytes.numel() if n_bytes is None else n_bytes,
                           table.ctypes.data if n else None, n, d_crc.data_ptr() if want_crc else None, d_status.data_ptr())
    st = abi.Status()
    rc_sync = L.pqg_crc32_sync(decoder.ctx, d_status.data_ptr(), n, C.byref(st))
    return rc, d_crc[:n].cpu().numpy().view(np.uint32), d_status[:n].cpu().numpy(), rc_sync, st


def upload(decoder, buf):
    return torch.from_numpy(np.frombuffer(bytes(buf), dtype=np.uint8).copy()).to(decoder.device)


def want_crcs(buf, table):
    return np.array([zlib.crc32(buf[int(o): int(o) + int(s)]) for o, s in zip(table["offset"], table["size"])], dtype=np.uint32)


def packed_matrix():
    """Every size at every start residue mod 16, packed into one buffer with a gap between jobs."""
    rows, pos = [], 0
    for s in SIZES:
        for r in range(16):
            base = (pos + 15) // 16 * 16
            rows.append((base + r, s))
            pos = base + r + s + 1
    return job_table(rows), pos


@pytest.mark.parametrize("fill", ["random", 0x00, 0xFF])
def test_size_alignment_matrix(decoder, fill):
    table, n = packed_matrix()
    assert len(table) == len(SIZES) * 16
    buf = np.random.default_rng(1).integers(0, 256, size=n, dtype=np.uint8).tobytes() if fill == "random" else bytes([fill]) * n
    rc, crcs, status, rc_sync, _ = crc_pages(decoder, upload(decoder, buf), table)
    assert rc == abi.OK and rc_sync == abi.OK
    want = want_crcs(buf, table)
    bad = np.flatnonzero(crcs != want)
    assert bad.size == 0, [(int(table["offset"][j]) % 16, int(table["size"][j]), hex(crcs[j]), hex(want[j])) for j in bad[:8]]
    assert not status.any()


def test_buffer_end_and_odd_length(decoder):
    """Jobs that end at the buffer's last byte, for buffer lengths of every residue mod 4 (the buffer is readable up to
    its length rounded up to 4 and no further), through Decoder.crc32."""
    rng = np.random.default_rng(2)
    for n in (1, 2, 3, 5, 1023, 1026, T + 1, T + 18, 2 * T + 7):
        buf = rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()
        offs = sorted({0, 1, n // 2, max(n - 17, 0), n - 1, n})
        d_crc, codes, st = decoder.crc32(upload(decoder, buf), offs, [n - o for o in offs])
        assert st.code == abi.OK and not codes.any()
        got = d_crc.cpu().numpy().view(np.uint32)
        assert [int(g) for g in got] == [zlib.crc32(buf[o:]) for o in offs], n


def test_many_tiles(decoder):
    n = 70 * T + 3
    buf = os.urandom(5) + np.random.default_rng(3).integers(0, 256, size=n, dtype=np.uint8).tobytes() + os.urandom(9)
    rows = [(5, n)] + [(5 + k * T, min(T, n - k * T)) for k in range(71)]
    rc, crcs, status, rc_sync, _ = crc_pages(decoder, upload(decoder, buf), job_table(rows))
    assert rc == abi.OK and rc_sync == abi.OK and not status.any()
    assert int(crcs[0]) == zlib.crc32(buf[5: 5 + n])
    chained = 0
    for (_, size), c in zip(rows[1:], crcs[1:]):
        chained = native.lib().pqg_crc32_combine(chained, int(c), size)
    assert chained == int(crcs[0])


def test_slot_reuse_in_queued_calls(decoder):
    """2 * CRC_SLOTS + 1 calls of pqg_crc32_pages queued on one context with no wait between them, each with a job
    list of its own: one job of T + 1 bytes (two tiles and a fold) at its own offset. The job and tile tables go
    up through a pinned slot that the call CRC_SLOTS later reuses: a slot overwritten before the fold that reads
    it has run shows as a call that gave another call's checksum."""
    calls, size = 5, T + 1
    buf = np.random.default_rng(5).integers(0, 256, size=calls * (size + 3) + 8, dtype=np.uint8).tobytes()
    tables = [job_table([(k * (size + 3) + k % 4, size)]) for k in range(calls)]
    d_bytes = upload(decoder, buf)
    d_crc = [torch.full((1,), 0x5A5A5A5A, dtype=torch.int32, device=decoder.device) for _ in range(calls)]
    d_status = [torch.full((1,), -7, dtype=torch.int32, device=decoder.device) for _ in range(calls)]
    held = busy_stream(decoder)
    L = native.lib()
    for t, c, s in zip(tables, d_crc, d_status):
        assert L.pqg_crc32_pages(decoder.ctx, d_bytes.data_ptr(), d_bytes.numel(), t.ctypes.data, 1, c.data_ptr(),
                                 s.data_ptr()) == abi.OK
    st = abi.Status()
    for s in d_status:
        assert L.pqg_crc32_sync(decoder.ctx, s.data_ptr(), 1, C.byref(st)) == abi.OK
    want = [int(want_crcs(buf, t)[0]) for t in tables]
    assert len(set(want)) == calls
    assert [int(c.cpu().numpy().view(np.uint32)[0]) for c in d_crc] == want
    del held


def test_isolation(decoder):
    rng = np.random.default_rng(4)
    sizes = [1, 3, 16, 17, 1024, T - 1, T, T + 1, 2 * T + 5, 0, 40]
    rows, pos = [], 3
    for s in sizes:
        rows.append((pos, s))
        pos += s + 2  # two bytes between neighbours: one after this job, one before the next
    buf = bytearray(rng.integers(0, 256, size=pos + 1, dtype=np.uint8).tobytes())
    table = job_table(rows)
    want = want_crcs(bytes(buf), table)
    flipped = bytearray(buf)
    for o, s in rows:
        flipped[o - 1] ^= 0xFF
        flipped[o + s] ^= 0xFF
    _, crcs, _, _, _ = crc_pages(decoder, upload(decoder, flipped), table)
    assert np.array_equal(crcs, want)
    # overlapping and duplicate jobs, then the same jobs in reverse order
    lap = [(0, len(buf)), (1, len(buf) - 1), (T - 8, 16), (T - 8, 16), (100, 2 * T), (101, 2 * T), (100, 2 * T), (7, 0), (7, 0)]
    table = job_table(lap)
    want = want_crcs(bytes(buf), table)
    d = upload(decoder, buf)
    _, crcs, _, _, _ = crc_pages(decoder, d, table)
    assert np.array_equal(crcs, want)
    _, crcs, _, _, _ = crc_pages(decoder, d, table[::-1].copy())
    assert np.array_equal(crcs, want[::-1])


def test_verdicts(decoder):
    rng = np.random.default_rng(5)
    sizes = [1, 2, 5, 16, 1025, T, T + 1, 2 * T, 2 * T + 9, 3 * T + 1, 0, 64]
    rows, pos = [], 1
    for s in sizes:
        rows.append((pos, s))
        pos += s + 3
    buf = bytearray(rng.integers(0, 256, size=pos, dtype=np.uint8).tobytes())
    good = want_crcs(bytes(buf), job_table(rows))
    table = job_table([(o, s, int(c), abi.CRC_VERIFY) for (o, s), c in zip(rows, good)])
    rc, crcs, status, rc_sync, st = crc_pages(decoder, upload(decoder, buf), table)
    assert rc == abi.OK and rc_sync == abi.OK and st.code == abi.OK and not status.any() and np.array_equal(crcs, good)
    # no d_crc: the verdicts alone
    rc, _, status, rc_sync, _ = crc_pages(decoder, upload(decoder, buf), table, want_crc=False)
    assert rc == abi.OK and rc_sync == abi.OK and not status.any()
    # one bit at the first byte, the last byte, and on each side of a tile seam
    hits = {0: 0, 3: 15, 5: T - 1, 6: T, 7: T - 1, 8: 2 * T, 9: 3 * T, 11: 63}  # job -> byte of the job
    bad = bytearray(buf)
    for j, at in hits.items():
        assert at < rows[j][1]
        bad[rows[j][0] + at] ^= 1 << (j % 8)
    rc, crcs, status, rc_sync, st = crc_pages(decoder, upload(decoder, bad), table)
    assert rc == abi.OK
    assert [j for j in range(len(rows)) if status[j]] == sorted(hits) and set(status[sorted(hits)]) == {abi.ERR_CRC}
    assert np.array_equal(crcs, want_crcs(bytes(bad), table))
    assert rc_sync == abi.ERR_CRC and st.code == abi.ERR_CRC and st.page == min(hits)
    assert b"CRC checksum verification failed" in st.message
    # a high-bit expected value compares unsigned; without the flag a wrong expected value is ignored
    table2 = job_table([(o, s, int(c) ^ 0x80000001, 0) for (o, s), c in zip(rows, good)])
    rc, crcs, status, rc_sync, _ = crc_pages(decoder, upload(decoder, buf), table2)
    assert rc == abi.OK and rc_sync == abi.OK and not status.any() and np.array_equal(crcs, good)
    table2["flags"] = abi.CRC_VERIFY
    _, _, status, rc_sync, st = crc_pages(decoder, upload(decoder, buf), table2)
    assert status.all() and rc_sync == abi.ERR_CRC and st.page == 0


def test_refusals(decoder):
    """Every refusal is made on the host, before any launch: the status words keep what they held."""
    buf = upload(decoder, os.urandom(1000))
    L = native.lib()

    def call(rows, **kw):
        rc, _, status, _, _ = crc_pages(decoder, buf, job_table(rows), **kw)
        assert (status == -7).all()
        return rc
    assert call([(0, 1000), (1, 1000)]) == abi.ERR_INVALID_ARG                  # one byte past n_bytes
    assert call([(1001, 0)]) == abi.ERR_INVALID_ARG
    assert call([(2**64 - 1, 2)]) == abi.ERR_INVALID_ARG                        # offset + size wraps
    assert call([(0, 10, 0, 0, 1)]) == abi.ERR_INVALID_ARG                      # reserved
    assert call([(0, 10, 0, 2)]) == abi.ERR_INVALID_ARG                         # unknown flag
    assert call([(0, 10, 0, abi.CRC_VERIFY | 4)]) == abi.ERR_INVALID_ARG
    table = job_table([(0, 10)])
    d_status = torch.full((1,), -7, dtype=torch.int32, device=decoder.device)
    torch.cuda.synchronize()
    args = [decoder.ctx, buf.data_ptr(), 1000, table.ctypes.data, 1, None, d_status.data_ptr()]
    for null in (0, 1, 3, 6):
        a = list(args)
        a[null] = None
        assert L.pqg_crc32_pages(*a) == abi.ERR_INVALID_ARG, null
    a = list(args)
    a[4] = -1
    assert L.pqg_crc32_pages(*a) == abi.ERR_INVALID_ARG
    assert L.pqg_crc32_sync(None, d_status.data_ptr(), 1, None) == abi.ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert int(d_status.cpu()[0]) == -7
    # n_jobs == 0 is valid, with or without pointers
    assert L.pqg_crc32_pages(decoder.ctx, None, 0, None, 0, None, None) == abi.OK
    assert L.pqg_crc32_pages(decoder.ctx, buf.data_ptr(), 1000, table.ctypes.data, 0, None, d_status.data_ptr()) == abi.OK
    assert L.pqg_crc32_sync(decoder.ctx, d_status.data_ptr(), 0, None) == abi.OK
    rc, crcs, status, rc_sync, _ = crc_pages(decoder, buf, job_table([(0, 1000), (999, 1), (1000, 0)]))
    assert rc == abi.OK and rc_sync == abi.OK and not status.any() and int(crcs[2]) == 0


def file_chunks():
    """(raw chunk bytes, value count): the reference-written chunks that carry CRCs, and writer-made V1 / V2 chunks
    with a dictionary page."""
    out = [(raw_chunk(name, c), c["num_values"]) for name, c in fixtures.chunk_cases() if name in ("test-append_1", "test-append_2")]
    out += [(thrift_compact.chunk_bytes(ch, with_crc=True), ch.num_slots) for ch in written_chunks()]
    return out


def test_file_bytes_in(decoder):
    chunks = file_chunks()
    assert len(chunks) >= 6

    def pipeline(raws):
        """pqg_frame_chunk(verify_crc=0) -> pqg_crc_jobs_from_headers -> one pqg_crc32_pages over all chunks.
        Returns per chunk (statuses by job, header_of_job, headers)."""
        data, tables, per = bytearray(), [], []
        for k, (raw, nv) in enumerate(raws):
            data += bytes(1 + k % 5)  # chunks start at any alignment
            base = len(data)
            data += raw
            rc, st, hdrs = framing.frame_chunk_native(raw, nv, verify_crc=False)
            assert rc == abi.OK, st.message
            rc, _, n, jobs, hoj = jobs_from_headers(hdrs, chunk_offset=base)
            assert rc == abi.OK and n == len(hdrs) > 0
            tables.append(np.frombuffer(bytes(jobs), dtype=abi.CRC_JOB_DTYPE)[:n])
            per.append((n, [hoj[j] for j in range(n)], hdrs))
        table = np.concatenate(tables)
        rc, crcs, status, _, _ = crc_pages(decoder, upload(decoder, data), table)
        assert rc == abi.OK and np.array_equal(crcs, want_crcs(bytes(data), table))
        out, at = [], 0
        for n, hoj, hdrs in per:
            out.append((status[at: at + n], hoj, hdrs))
            at += n
        return out
    for (raw, nv), (status, hoj, hdrs) in zip(chunks, pipeline(chunks)):
        assert not status.any()
        assert framing.frame_chunk_native(raw, nv, verify_crc=True)[0] == abi.OK
    # a flipped byte in the middle of page k's body
    damaged, ks = [], []
    for i, (raw, nv) in enumerate(chunks):
        _, _, hdrs = framing.frame_chunk_native(raw, nv, verify_crc=False)
        k = i % len(hdrs)
        b = bytearray(raw)
        b[hdrs[k].body_offset + hdrs[k].compressed_page_size // 2] ^= 0x10
        damaged.append((bytes(b), nv))
        ks.append(k)
    assert 0 in ks and max(ks) > 0  # a dictionary or first page, and later ones
    for (raw, nv), k, (status, hoj, hdrs) in zip(damaged, ks, pipeline(damaged)):
        assert [hoj[j] for j in np.flatnonzero(status)] == [k] and status[hoj.index(k)] == abi.ERR_CRC
        rc, st, _ = framing.frame_chunk_native(raw, nv, verify_crc=True)
        assert rc == abi.ERR_CRC and st.page == k and b"CRC checksum verification failed" in st.message


# ---- Decoder.upload_chunks(verify_crc=True) ---------------------------------------------------------------
def with_crcs(ch):
    """The chunk with the checksums a writer would have put into its page headers."""
    ch = copy.deepcopy(ch)
    if ch.dict_page is not None:
        ch.dict_crc = zlib.crc32(ch.dict_page)
    for pg in ch.pages:
        pg.crc = zlib.crc32(pg.body)
    return ch


def codec_chunks():
    """Fixture chunks of every codec, V1 and V2: (chunk with crcs, expected values)."""
    picked = []
    for fx in ("arrow_encodings", "arrow_binary", "arrow_snappy", "arrow_zstd", "arrow_gzip", "arrow_lz4raw"):
        for ver in ("_v1", "_v2"):
            cases = [(n, c) for n, c in fixtures.chunk_cases() if n == fx + ver]
            assert cases, fx + ver
            for n, c in cases:
                ch, exp = fixtures.load_chunk(n, c)
                picked.append((with_crcs(ch), exp))
    return picked


def test_upload_chunks_verifies(decoder):
    picked = codec_chunks()
    chunks = [ch for ch, _ in picked]
    codecs = {p.codec for ch in chunks for p in ch.pages}
    assert codecs == {writer.UNCOMPRESSED, writer.SNAPPY, writer.ZSTD, writer.GZIP, writer.LZ4_RAW}
    assert any(p.version == 2 and p.codec and p.rl_byte_length + p.dl_byte_length for ch in chunks for p in ch.pages)
    assert any(ch.dict_codec for ch in chunks) and any(ch.dict_page is not None and not ch.dict_codec for ch in chunks)
    dbatch = decoder.upload_chunks(chunks, verify_crc=True)
    plain = decoder.upload_chunks(chunks)
    assert np.array_equal(dbatch.bytes.cpu().numpy(), plain.bytes.cpu().numpy())
    cols, st = decoder.decode(dbatch)
    for col, (ch, exp) in zip(cols, picked):
        assert_same(col.numpy(), exp, ch.physical_type)


def fixture_chunk(name, key):
    (c,) = [c for n, c in fixtures.chunk_cases() if n == name and c["key"] == key]
    return with_crcs(fixtures.load_chunk(name, c)[0])


def outcome(decoder, chunks, **kw):
    """What an upload + decode ends in: the error code raised, or the decoded bytes."""
    try:
        cols, st = decoder.decode(decoder.upload_chunks(chunks, **kw), check=False)
    except native.PqgError as e:
        return ("raised", e.code)
    return ("decoded", st.code, [c.values.cpu().numpy().tobytes() for c in cols],
            [c.def_levels.cpu().numpy().tobytes() for c in cols if c.def_levels is not None])


def test_upload_chunks_damage(decoder):
    first = fixture_chunk("arrow_snappy_v2", "rg0_c0")  # a SNAPPY dictionary page
    assert first.dict_codec == writer.SNAPPY
    good = fixture_chunk("arrow_snappy_v2", "rg0_c4")   # SNAPPY V2 pages behind their definition levels
    k = 2
    lv = good.pages[k].rl_byte_length + good.pages[k].dl_byte_length
    assert good.pages[k].version == 2 and good.pages[k].codec == writer.SNAPPY and lv > 16

    def damaged(at, drop_crc=False):
        ch = copy.deepcopy(good)
        b = bytearray(ch.pages[k].body)
        b[at] ^= 0x55
        ch.pages[k].body = bytes(b)
        if drop_crc:
            ch.pages[k].crc = None
        return [first, ch]
    assert outcome(decoder, [first, good], verify_crc=True)[:2] == ("decoded", abi.OK)
    # the data section's first byte is the Snappy block's length: today the codec reports CORRUPT
    assert outcome(decoder, damaged(lv)) == ("raised", abi.ERR_CORRUPT)
    for at in (lv, len(good.pages[k].body) - 1, 0, lv - 1):  # data bytes, then level bytes
        with pytest.raises(native.PqgError) as ei:
            decoder.upload_chunks(damaged(at), verify_crc=True)
        assert ei.value.code == abi.ERR_CRC, at
        assert f"chunk 1, page {k}:" in str(ei.value) and "CRC checksum verification failed" in str(ei.value)
        # without a crc on the damaged page nothing checks it: the outcome is that of verify_crc=False
        assert outcome(decoder, damaged(at, drop_crc=True), verify_crc=True) == outcome(decoder, damaged(at))
    # a damaged dictionary page is named as one, and comes before a damaged data page of a later chunk
    bad_dict = copy.deepcopy(first)
    bad_dict.dict_page = bad_dict.dict_page[:-1] + bytes([bad_dict.dict_page[-1] ^ 1])
    with pytest.raises(native.PqgError) as ei:
        decoder.upload_chunks([bad_dict, damaged(lv)[1]], verify_crc=True)
    assert ei.value.code == abi.ERR_CRC and "chunk 0, dictionary page:" in str(ei.value)
    # uncompressed pages are checked in the batch itself
    flat = with_crcs(writer.write_column_chunk(abi.INT32, np.arange(3000, dtype=np.int32), abi.PLAIN, page_rows=1000))
    assert outcome(decoder, [flat], verify_crc=True)[:2] == ("decoded", abi.OK)
    flat.pages[1].body = flat.pages[1].body[:8] + bytes([flat.pages[1].body[8] ^ 1]) + flat.pages[1].body[9:]
    assert flat.pages[1].crc != zlib.crc32(flat.pages[1].body)
    with pytest.raises(native.PqgError) as ei:
        decoder.upload_chunks([flat], verify_crc=True)
    assert ei.value.code == abi.ERR_CRC and "chunk 0, page 1:" in str(ei.value)
    assert outcome(decoder, [flat])[:2] == ("decoded", abi.OK)
