"""Time pqg_decrypt_pages on the pages of the benchmark workloads, encrypted in both modes, beside the local
libcrypto on the host and the plain decode of the same pages.

    python tools/bench_decrypt.py [--workloads c2,c4] [--c2-rows 100000000] [--c4-rows 125000000]
                                  [--tiles 4096,16384,32768] [--repeats 5] [--launches 10] [--warmup 2]

Workloads: C2's pages (bench.py's input) and one GPU's C4 shard (lineitem, about 100,000 smaller pages). Every data
page and dictionary page of the host batch becomes one module, [length][nonce][ciphertext][tag] (AES_GCM_V1) or
without the tag (the page modules of AES_GCM_CTR_V1), encrypted here with libcrypto under one 128-bit key per
column with AesCipher.createModuleAAD's AADs; the modules are uploaded once and every job's plaintext goes to the
page's place in the device batch, where the decoder reads it.

Each repeat times `launches` back-to-back calls between two device events on the decoder's stream: decrypt alone
(a call includes the host's table build and its copy through pinned memory), decrypt + decode (one prepared plan
launch behind each decrypt call) and the plain decode. The batch is compared with the plaintext batch before and
after timing. Reported per (workload, mode, tile): median / min / max ms per call, plaintext bytes/s, the fraction
of the 8 TB/s HBM roofline counted over read + write (ciphertext in, plaintext out), decrypt + decode against the
decode. Per (workload, mode): libcrypto's EVP decryption of the same modules on 1 and 16 host threads. One JSON
line each. Needs a libcrypto (ctypes.util.find_library)."""
import argparse
import ctypes as C
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "parquet-mr_amd"), os.path.join(REPO, "tools"), os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import aes_ref  # noqa: E402  (tests/: the module framing and the libcrypto binding)
from pqgpu import abi, crypto, decoder, native  # noqa: E402

PEAK_BYTES_PER_S = 8e12
HOST_THREADS = 16
FILE_AAD = bytes(range(8))


def timed(stream, fn, launches):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        start.record()
        for _ in range(launches):
            fn()
        stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / launches


def encrypt_batch(batch, mode, lib, rng):
    """-> (module buffer, job table, keys, AAD blob, per job (key, aad)) for every page and dictionary page."""
    cols = batch.columns
    keys = [rng.bytes(16) for _ in cols]
    page_no = {}
    items = []  # (offset in the batch, size, column, aad)
    for i, c in enumerate(cols):
        if c["dict_offset"] >= 0:
            items.append((int(c["dict_offset"]), int(c["dict_size"]), i, crypto.module_aad(FILE_AAD, crypto.DICTIONARY_PAGE, 0, i)))
    for o, s, col in zip(batch.pages["offset"].tolist(), batch.pages["size"].tolist(), batch.pages["column"].tolist()):
        k = page_no.get(col, 0)
        page_no[col] = k + 1
        items.append((o, s, col, crypto.module_aad(FILE_AAD, crypto.DATA_PAGE, 0, col, k % 32768)))
    view = memoryview(batch.data)
    table = np.zeros(len(items), dtype=abi.DECRYPT_JOB_DTYPE)
    mods, aads, pos, apos = [], [], 0, 0
    for j, (o, s, col, aad) in enumerate(items):
        m = aes_ref.encrypt_module(keys[col], mode, rng.bytes(12), bytes(view[o:o + s]), aad, backend=lib)
        table[j] = (pos, o, len(m), apos, len(aad), mode, col, 0)
        mods.append(m)
        aads.append(aad)
        pos += len(m)
        apos += len(aad)
    src = np.frombuffer(b"".join(mods) + bytes(16), dtype=np.uint8).copy()
    return src, table, keys, b"".join(aads), [(keys[it[2]], it[3]) for it in items]


def host_rate(lib, src, table, owners, mode, threads):
    """Plaintext bytes/s of libcrypto's EVP decryption of the modules, split into `threads` shares of equal bytes."""
    L, vp = lib.lib, C.c_void_p
    base = src.ctypes.data
    offs, sizes = table["src_offset"].tolist(), table["src_size"].tolist()
    cum = np.cumsum(table["src_size"].astype(np.int64))
    cuts = [0] + [int(np.searchsorted(cum, cum[-1] * (k + 1) // threads, side="left")) + 1 for k in range(threads)]
    cuts[-1] = len(offs)
    cipher = vp(getattr(L, "EVP_aes_128_gcm" if mode == abi.DECRYPT_GCM else "EVP_aes_128_ctr")())
    ok = [True] * threads

    def share(k):
        ctx = vp(L.EVP_CIPHER_CTX_new())
        out = C.create_string_buffer(int(max(sizes)) + 32)
        n = C.c_int()
        for j in range(cuts[k], max(cuts[k], cuts[k + 1])):
            key, aad = owners[j]
            m, size = base + offs[j], sizes[j]
            if mode == abi.DECRYPT_GCM:
                L.EVP_DecryptInit_ex(ctx, cipher, None, None, None)
                L.EVP_DecryptInit_ex(ctx, None, None, key, vp(m + 4))
                L.EVP_DecryptUpdate(ctx, None, C.byref(n), aad, len(aad))
                L.EVP_DecryptUpdate(ctx, out, C.byref(n), vp(m + 16), size - 32)
                L.EVP_CIPHER_CTX_ctrl(ctx, 0x11, 16, vp(m + size - 16))  # EVP_CTRL_GCM_SET_TAG
                ok[k] = ok[k] and L.EVP_DecryptFinal_ex(ctx, C.byref(out, n.value), C.byref(n)) == 1
            else:
                iv = C.string_at(m + 4, 12) + b"\0\0\0\1"
                L.EVP_DecryptInit_ex(ctx, cipher, None, key, iv)
                L.EVP_DecryptUpdate(ctx, out, C.byref(n), vp(m + 16), size - 16)
        L.EVP_CIPHER_CTX_free(ctx)
    t0 = time.perf_counter()
    if threads == 1:
        share(0)
    else:
        with ThreadPoolExecutor(threads) as ex:
            list(ex.map(share, range(threads)))
    dt = time.perf_counter() - t0
    assert all(ok), "libcrypto refused a tag"
    overhead = 32 if mode == abi.DECRYPT_GCM else 16
    return float(cum[-1] - overhead * len(offs)) / dt


def run(name, batch, args, lib):
    dec = decoder.Decoder(0)
    rng = np.random.default_rng(1)
    dbatch = dec.upload(batch)
    cols, st = dec.decode(dbatch)
    plan = dec.plan(dbatch, cols)
    want = batch.data
    tiles = [int(t) for t in args.tiles.split(",")]
    ms_decode = []
    for mode, mode_name in ((abi.DECRYPT_GCM, "gcm"), (abi.DECRYPT_CTR, "ctr")):
        src, table, keys, aad, owners = encrypt_batch(batch, mode, lib, rng)
        d_src = torch.from_numpy(src).to(dec.device)
        n = len(table)
        d_status = torch.zeros(n, dtype=torch.int32, device=dec.device)
        plain = int(table["src_size"].sum()) - (32 if mode == abi.DECRYPT_GCM else 16) * n
        moved = int(table["src_size"].sum()) + plain
        torch.cuda.synchronize()

        def decrypt():
            dec.decrypt(d_src, dbatch.bytes, table, keys, aad, d_status=d_status, sync=False)

        def both():
            decrypt()
            plan.launch()

        def check(what):
            st = abi.Status()
            rc = native.lib().pqg_decrypt_sync(dec.ctx, d_status.data_ptr(), n, C.byref(st))
            assert rc == abi.OK, (what, st.message)
            assert np.array_equal(dbatch.bytes.cpu().numpy(), want), what

        ms = {t: [] for t in tiles}
        ms_both = {t: [] for t in tiles}
        for t in tiles:  # checked before anything is timed
            dec.set_dispatch(abi.DISPATCH_AES_TILE_BYTES, t)
            dbatch.bytes.zero_()
            torch.cuda.synchronize()
            decrypt()
            check(f"{name} {mode_name} tile {t} before")
        for _ in range(args.repeats):
            for t in tiles:
                dec.set_dispatch(abi.DISPATCH_AES_TILE_BYTES, t)
                for _ in range(args.warmup):
                    both()
                ms[t].append(timed(dec.stream, decrypt, args.launches))
                ms_both[t].append(timed(dec.stream, both, args.launches))
            for _ in range(args.warmup):
                plan.launch()
            ms_decode.append(timed(dec.stream, plan.launch, args.launches))
            rc, st = plan.sync()
            assert rc == abi.OK, st.message
        check(f"{name} {mode_name} after")
        dms = float(np.median(ms_decode))
        best = 0.0
        for t in tiles:
            m, mb = float(np.median(ms[t])), float(np.median(ms_both[t]))
            rate = plain / (m * 1e-3)
            best = max(best, rate)
            print(json.dumps({"workload": name, "mode": mode_name, "tile_bytes": t, "jobs": n, "plaintext_bytes": plain,
                              "ms_per_call": round(m, 4), "ms_min": round(min(ms[t]), 4), "ms_max": round(max(ms[t]), 4),
                              "plaintext_bytes_per_s": round(rate, 0),
                              "hbm_read_write_roofline_fraction": round(moved / (m * 1e-3) / PEAK_BYTES_PER_S, 4),
                              "decrypt_plus_decode_ms": round(mb, 4), "decode_ms_per_launch": round(dms, 4),
                              "decrypt_plus_decode_over_decode": round(mb / dms, 3)}), flush=True)
        for threads in (1, HOST_THREADS):
            rate = host_rate(lib, src, table, owners, mode, threads)
            print(json.dumps({"workload": name, "mode": mode_name, "libcrypto_threads": threads, "plaintext_bytes": plain,
                              "plaintext_bytes_per_s": round(rate, 0), "best_device_over_host": round(best / rate, 2)}), flush=True)
    plan.close()
    dec.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="c2,c4")
    ap.add_argument("--c2-rows", type=int, default=100_000_000)
    ap.add_argument("--c4-rows", type=int, default=125_000_000)
    ap.add_argument("--tiles", default="4096,16384,32768")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_decrypt.py needs a GPU"
    lib = aes_ref.Libcrypto.load()
    assert lib is not None, "bench_decrypt.py needs a libcrypto"
    from tools.synth import writer
    for w in args.workloads.split(","):
        if w == "c2":
            import workloads
            chunk, _, _ = workloads.make_c2(args.c2_rows, 42, 43, 1.5, 1000, 4096, 20000)
            run("c2", writer.build_batch([chunk]), args, lib)
        elif w == "c4":
            import lineitem
            run("c4", lineitem.Shard(args.c4_rows).batch, args, lib)
        else:
            raise SystemExit(f"unknown workload {w}")


if __name__ == "__main__":
    main()
