"""Time pqg_take on decoded-column-shaped device data and the torch composition beside it.

    python tools/bench_take.py [--rows 100000000] [--binary-rows 20000000] [--repeats 5] [--launches 20] [--direct]

Cases:
  (a)  required int64, the bitmap of lt(c, x) at about 10 % selected; yardstick on the same tensors:
       values[row_ids] with the row ids the filter already produced
  (b)  nullable int64 and nullable double, 10 % nulls each, taken in one call with the same bitmap;
       yardstick: the torch composition a user would write today (cumsum of validity -> source index
       -> index_select, plus def_levels[row_ids]) for both columns
  (c)  a required BYTE_ARRAY column of 8-24 byte values (--binary-rows), a random 10 % bitmap
  (a') case (a) at about 90 % selected
  (r)  pqg_take_records on a list<int64> leaf of --rows slots: record lengths uniform 0..8, an empty list
       as one null slot, a random 10 % of the records kept; (r90): the same at 90 %. Beside each:
       `_floor`, pqg_take on the same definition bytes and values as a flat nullable column plus the
       repetition bytes as a required 1-byte column, with the slot bitmap computed outside the timed
       region (what the record call costs beyond it is the count / scan / expansion of the record
       bitmap); `_torch`, the composition cumsum(rep == 0) - 1 -> bit lookup -> nonzero -> index_select
       of the levels, with the nullable value gather of case (b)
--direct adds every HIP case again with PQG_DISPATCH_TAKE_STAGED = 0 (one store per kept lane).

Timing as tools/bench_filter.py: each repeat times `launches` back-to-back launches between two device
events on the decoder's stream (after warm-up launches of the same shape) and the cases alternate
inside a repeat. Reported per case: the median over the repeats of ms per launch, the smallest and
largest repeat, and the fraction of 8 TB/s reached on the algorithmic bytes (bitmap, level bytes and
kept values read, plus everything written). The results are checked against torch before anything is
timed. One JSON line per case."""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "parquet-mr_amd"))
sys.path.insert(0, REPO)

from pqgpu import abi, decoder  # noqa: E402
from pqgpu import filter as F  # noqa: E402
from pqgpu import take as T  # noqa: E402
from tools.bench_filter import PEAK_BYTES_PER_S, device_column, timed  # noqa: E402


def pack_bitmap(mask):
    """bool[n] (n a multiple of 64) -> int64 words, row r = bit r & 63 of word r >> 6."""
    bits = mask.view(-1, 64).to(torch.int64) << torch.arange(64, device=mask.device, dtype=torch.int64)
    return bits.sum(dim=1)  # distinct bits: the wrapping sum is their union


def torch_take_nullable(values, dl, row_ids):
    """What a user composes today for one nullable column: (dense kept values, kept level bytes)."""
    valid = dl == 1
    src = torch.cumsum(valid, dim=0) - 1  # dense index of a row that has a value
    kept_valid = row_ids[valid[row_ids]]
    return values.index_select(0, src[kept_valid]), dl[row_ids]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--binary-rows", type=int, default=20_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--direct", action="store_true", help="also time the one-store-per-lane variant")
    ap.add_argument("--cases", default="a,b,c,a90", help="cases to check and time, of a,b,c,a90,r,r90 (a profiler run takes one at a time)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_take needs a GPU"
    n, nb = args.rows, args.binary_rows // 64 * 64
    cases = args.cases.split(",")
    dec = decoder.Decoder(0)
    dev = dec.device
    g = torch.Generator(device=dev)
    g.manual_seed(1)

    # (a), (a'): required int64 uniform in [0, 1000): lt(c, 100) keeps about 10 %, lt(c, 900) about 90 %
    a_vals = torch.randint(0, 1000, (n,), generator=g, device=dev, dtype=torch.int64)
    a_cols = [device_column(abi.INT64, a_vals)]
    sels = {}
    for name, x in (("a", 100), ("a90", 900)):
        sel = dec.filter(F.lt(F.col(0), x), a_cols, n)
        sels[name] = (sel.bitmap, sel.row_ids.clone(), sel.count)
    # (b): two nullable columns, 10 % nulls each, taken with (a)'s bitmap
    dl0 = (torch.rand(n, generator=g, device=dev) >= 0.1).to(torch.uint8)
    dl1 = (torch.rand(n, generator=g, device=dev) >= 0.1).to(torch.uint8)
    b_i = torch.randint(0, 1000, (int(dl0.sum()),), generator=g, device=dev, dtype=torch.int64)
    b_d = torch.rand(int(dl1.sum()), generator=g, device=dev, dtype=torch.float64)
    b_cols = [device_column(abi.INT64, b_i, dl0), device_column(abi.DOUBLE, b_d, dl1)]
    # (c): 8-24 byte values, a random 10 % of the rows
    lens = torch.randint(8, 25, (nb,), generator=g, device=dev, dtype=torch.int64)
    c_off = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(lens, 0)])
    c_bytes = torch.randint(0, 256, (int(c_off[-1]),), generator=g, device=dev, dtype=torch.uint8)
    c_col = decoder.DeviceColumn(abi.BYTE_ARRAY, c_off.view(torch.uint8), None, binary_data=c_bytes)
    c_col.n_values = nb
    c_mask = torch.rand(nb, generator=g, device=dev) < 0.1
    c_bitmap = pack_bitmap(c_mask)

    a_bm, a_ids, a_count = sels["a"]
    a90_bm, a90_ids, a90_count = sels["a90"]
    outs = {"a": [T.alloc_output(dev, a_cols[0], n, a_count)], "a90": [T.alloc_output(dev, a_cols[0], n, a90_count)],
            "b": [T.alloc_output(dev, c, n, a_count) for c in b_cols], "c": [T.alloc_output(dev, c_col, nb, nb)]}
    torch.cuda.synchronize()

    # results first: against torch on the same tensors
    for name, (bm, ids, count) in sels.items():
        if name not in cases:
            continue
        t = dec.take(bm, a_cols, n_rows=n, rows_capacity=count, out=outs[name])
        assert t.n_rows == count and torch.equal(t.columns[0].typed(), a_vals[ids]), f"case ({name}) differs from torch"
    b_kept, c_count, c_nbytes = [], 0, 0
    if "b" in cases:
        t = dec.take(a_bm, b_cols, n_rows=n, rows_capacity=a_count, out=outs["b"])
        for col, src in zip(t.columns, b_cols):
            want_v, want_dl = torch_take_nullable(src.typed(), src.def_levels, a_ids)
            assert torch.equal(col.typed(), want_v) and torch.equal(col.def_levels[:t.n_rows], want_dl), "case (b) differs from torch"
            b_kept.append(col.n_values)
        del want_v, want_dl
    if "c" in cases:
        t = dec.take(c_bitmap, [c_col], n_rows=nb, out=outs["c"])
        c_ids = torch.nonzero(c_mask).flatten()
        k_len = lens[c_ids]
        want_off = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(k_len, 0)])
        assert t.n_rows == c_ids.numel() and torch.equal(t.columns[0].offsets(), want_off), "case (c) offsets differ from torch"
        src_idx = torch.repeat_interleave(c_off[c_ids] - want_off[:-1], k_len) + torch.arange(int(want_off[-1]), device=dev)
        assert torch.equal(t.columns[0].binary_data[:int(want_off[-1])], c_bytes[src_idx]), "case (c) bytes differ from torch"
        c_count, c_nbytes = t.n_rows, int(want_off[-1])
        del src_idx, want_off, k_len, c_ids

    # (r), (r90): a list<int64> leaf; max_def 2: an element slot has def 2, the slot of an empty list def 1
    rec = {}
    if "r" in cases or "r90" in cases:
        n_rec = n * 9 // 37 // 64 * 64  # lengths 0..8 take (1 + 1 + 2 + ... + 8) / 9 slots on average
        r_lens = torch.randint(0, 9, (n_rec,), generator=g, device=dev, dtype=torch.int64)
        r_slots = torch.clamp(r_lens, min=1)
        r_starts = torch.cumsum(r_slots, 0) - r_slots
        n_slots = int(r_slots.sum())
        r_rl = torch.ones(n_slots, dtype=torch.uint8, device=dev)
        r_rl[r_starts] = 0
        r_dl = torch.full((n_slots,), 2, dtype=torch.uint8, device=dev)
        r_dl[r_starts[r_lens == 0]] = 1
        r_vals = torch.randint(0, 1000, (int((r_dl == 2).sum()),), generator=g, device=dev, dtype=torch.int64)
        r_col = decoder.DeviceColumn(abi.INT64, r_vals.view(torch.uint8), r_dl, r_rl)
        r_col.n_values, r_col.max_def, r_col.max_rep, r_col.n_slots = r_vals.numel(), 2, 1, n_slots
        flat_cols = [decoder.DeviceColumn(abi.INT64, r_vals.view(torch.uint8), r_dl), device_column(abi.BOOLEAN, r_rl)]
        flat_cols[0].n_values, flat_cols[0].max_def = r_vals.numel(), 2
        del r_slots, r_starts
        for name, p in (("r", 0.1), ("r90", 0.9)):
            if name not in cases:
                continue
            mask = torch.rand(n_rec, generator=g, device=dev) < p
            bm = pack_bitmap(mask)
            rec_of = torch.cumsum(r_rl == 0, 0) - 1
            slot_mask = mask[rec_of]
            ids = torch.nonzero(slot_mask).flatten()
            pad = torch.zeros((n_slots + 63) // 64 * 64, dtype=torch.bool, device=dev)
            pad[:n_slots] = slot_mask
            out_r = [T.alloc_record_output(dev, r_col, n_rec, n_rec)]
            out_f = [T.alloc_output(dev, c, n_slots, int(ids.numel())) for c in flat_cols]
            t = dec.take_records(bm, [r_col], n_rows=n_rec, out=out_r)
            got = t.columns[0]
            want_v, want_dl = torch_take_nullable(r_vals, (r_dl == 2).to(torch.uint8), ids)
            assert t.n_rows == int(mask.sum()) and got.n_slots == ids.numel(), f"case ({name}) counts differ from torch"
            assert torch.equal(got.typed(), want_v) and torch.equal(got.def_levels[:got.n_slots], r_dl[ids]) and \
                torch.equal(got.rep_levels[:got.n_slots], r_rl[ids]), f"case ({name}) differs from torch"
            f = dec.take(pack_bitmap(pad), flat_cols, n_rows=n_slots, rows_capacity=int(ids.numel()), out=out_f)
            assert f.n_rows == ids.numel() and torch.equal(f.columns[0].typed(), want_v), f"case ({name}) floor differs from torch"
            rec[name] = dict(bitmap=bm, slot_bitmap=pack_bitmap(pad), out=out_r, out_flat=out_f, kept_records=t.n_rows,
                             kept_slots=int(ids.numel()), kept_values=got.n_values, n_rec=n_rec, n_slots=n_slots)
            del mask, rec_of, slot_mask, ids, pad, want_v, want_dl

    def rec_hip(r, staged=1):
        def fn():
            dec.set_dispatch(abi.DISPATCH_TAKE_STAGED, staged)
            dec.take_records(r["bitmap"], [r_col], n_rows=r["n_rec"], out=r["out"])
        return fn

    def rec_floor(r):
        def fn():
            dec.set_dispatch(abi.DISPATCH_TAKE_STAGED, 1)
            dec.take(r["slot_bitmap"], flat_cols, n_rows=r["n_slots"], rows_capacity=r["kept_slots"], out=r["out_flat"])
        return fn

    def rec_torch(r):
        def fn():
            rec_of = torch.cumsum(r_rl == 0, 0) - 1
            keep = (r["bitmap"][rec_of >> 6] >> (rec_of & 63)) & 1
            ids = torch.nonzero(keep).flatten()
            r_rl.index_select(0, ids)
            torch_take_nullable(r_vals, (r_dl == 2).to(torch.uint8), ids)
        return fn

    def hip(bm, cols, rows, cap, out, staged=1):
        def fn():
            dec.set_dispatch(abi.DISPATCH_TAKE_STAGED, staged)
            dec.take(bm, cols, n_rows=rows, rows_capacity=cap, out=out)
        return fn

    def torch_b():
        for src in b_cols:
            torch_take_nullable(src.typed(), src.def_levels, a_ids)

    hip_cases = {"a": (a_bm, a_cols, n, a_count, outs["a"]), "b": (a_bm, b_cols, n, a_count, outs["b"]),
                 "c": (c_bitmap, [c_col], nb, nb, outs["c"]), "a90": (a90_bm, a_cols, n, a90_count, outs["a90"])}
    runs = {}
    for k, v in hip_cases.items():
        runs[k + "_hip"] = hip(*v)
        if args.direct:
            runs[k + "_hip_direct"] = hip(*v, staged=0)
    runs["a_torch"] = lambda: a_vals[a_ids]
    runs["b_torch"] = torch_b
    runs["a90_torch"] = lambda: a_vals[a90_ids]
    for name, r in rec.items():
        runs[name + "_hip"] = rec_hip(r)
        if args.direct:
            runs[name + "_hip_direct"] = rec_hip(r, staged=0)
        runs[name + "_floor"] = rec_floor(r)
        runs[name + "_torch"] = rec_torch(r)
    runs = {k: fn for k, fn in runs.items() if k.split("_")[0] in cases}
    times = {k: [] for k in runs}
    for k, fn in runs.items():
        timed(dec.stream, fn, args.warmup)
    for _ in range(args.repeats):
        for k, fn in runs.items():
            times[k].append(timed(dec.stream, fn, args.launches))
    dec.set_dispatch(abi.DISPATCH_TAKE_STAGED, 1)

    n_words = (n + 63) // 64
    nbytes = {"a": 8 * n_words + 16 * a_count, "a90": 8 * n_words + 16 * a90_count,
              "b": 8 * n_words + 2 * n + 16 * sum(b_kept) + 2 * a_count,
              "c": nb // 8 + 16 * c_count + 8 * (c_count + 1) + 2 * c_nbytes}  # offsets: two read, one written per kept value
    what = {"a": "required int64, ~10 % kept", "a90": "required int64, ~90 % kept",
            "b": "nullable int64 + nullable double, 10 % nulls, ~10 % kept, one call",
            "c": "required BYTE_ARRAY of 8-24 byte values, ~10 % kept"}
    kept = {"a": a_count, "a90": a90_count, "b": a_count, "c": c_count}
    for name, r in rec.items():  # the record bitmap, both level bytes and the kept values read; the three outputs written
        nbytes[name] = r["n_rec"] // 8 + 2 * r["n_slots"] + 16 * r["kept_values"] + 2 * r["kept_slots"]
        what[name] = f"list<int64>, record lengths 0..8, ~{90 if name == 'r90' else 10} % of {r['n_rec']} records kept"
        kept[name] = r["kept_records"]
    for k, ts in times.items():
        case = k.split("_")[0]
        ms = float(np.median(ts))
        rows = nb if case == "c" else rec[case]["n_slots"] if case in rec else n
        print(json.dumps({"case": k, "what": what[case], "rows": rows, "kept": kept[case],
                          "ms_per_launch": round(ms, 4), "ms_min": round(min(ts), 4), "ms_max": round(max(ts), 4),
                          "repeats": len(ts), "launches_per_repeat": args.launches, "algorithmic_bytes": nbytes[case],
                          "fraction_of_8TBps": round(nbytes[case] / (ms * 1e-3) / PEAK_BYTES_PER_S, 4)}), flush=True)
    dec.close()


if __name__ == "__main__":
    main()
