"""Time pqg_filter_run on decoded-column-shaped device data and the torch composition beside it.

    python tools/bench_filter.py [--rows 100000000] [--repeats 5] [--launches 20] [--cases abde]

Four cases, all with row ids:
  (a) lt(required int64, x) at about 10 % selectivity; yardstick on the same tensors:
      torch.nonzero(values < x)
  (b) and_(lt_eq(nullable int64, x), not_eq(nullable double, y)), 10 % nulls in each column
  (d) eq(required BYTE_ARRAY, s) over a 7-entry dictionary of 10-20-byte entries: the uint32 ids + the
      dictionary (pqg_filter_run_dict) against pqg_filter_run on the materialised column (offsets + bytes),
      and against torch on the ids: torch.nonzero(table[ids]) with the verdicts of the 7 entries in `table`
  (e) lt(required int64, x) over a 1,000-entry dictionary at about 10 % selectivity: ids against values

Each repeat times `launches` back-to-back launches between two device events on the decoder's stream
(after warm-up launches of the same shape) and the cases alternate inside a repeat, so a drift of the
machine shows up as spread, not as a difference. Reported per case: the median over the repeats of ms
per launch, the smallest and largest repeat, and the fraction of 8 TB/s reached on the algorithmic
bytes (referenced values (for an id column its 4-byte ids) + definition levels read, bitmap + row ids written).
The results are checked
against torch before anything is timed. One JSON line per case."""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "parquet-mr_amd"))

from pqgpu import abi, decoder  # noqa: E402
from pqgpu import filter as F  # noqa: E402

PEAK_BYTES_PER_S = 8e12


def device_column(physical_type, values, def_levels=None):
    """A DeviceColumn over existing tensors, laid out as decode() leaves it."""
    col = decoder.DeviceColumn(physical_type, values.view(torch.uint8), def_levels)
    col.n_values = values.numel()
    col.max_def = 0 if def_levels is None else 1
    return col


def timed(stream, fn, launches):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        start.record()
        for _ in range(launches):
            fn()
        stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cases", default="abde", help="letters of the cases to time (all are set up and checked)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_filter needs a GPU"
    n = args.rows
    dec = decoder.Decoder(0)
    dev = dec.device
    g = torch.Generator(device=dev)
    g.manual_seed(1)

    # (a) required int64, values uniform in [0, 1000): lt(c, 100) selects about 10 %
    a_vals = torch.randint(0, 1000, (n,), generator=g, device=dev, dtype=torch.int64)
    a_cols = [device_column(abi.INT64, a_vals)]
    a_filter = F.Filter(F.lt(F.col(0), 100), a_cols)
    # (b) two nullable columns, 10 % nulls each: dense values of the non-null rows + one level byte per row
    dl0 = (torch.rand(n, generator=g, device=dev) >= 0.1).to(torch.uint8)
    dl1 = (torch.rand(n, generator=g, device=dev) >= 0.1).to(torch.uint8)
    row_i = torch.randint(0, 1000, (n,), generator=g, device=dev, dtype=torch.int64)
    row_d = torch.randint(0, 50, (n,), generator=g, device=dev, dtype=torch.int64).to(torch.float64)
    b_i, b_d = row_i[dl0 == 1].contiguous(), row_d[dl1 == 1].contiguous()
    b_cols = [device_column(abi.INT64, b_i, dl0), device_column(abi.DOUBLE, b_d, dl1)]
    b_filter = F.Filter(F.and_(F.lt_eq(F.col(0), 110), F.not_eq(F.col(1), 7.0)), b_cols)

    # (d) 7 entries of 10-20 bytes (the l_shipmode shape); the materialised column is dictionary[ids]
    words = [b"REG AIR...", b"AIR.........", b"RAIL...........", b"SHIP.............", b"TRUCK..............",
             b"MAIL.........xyz", b"FOB................."]
    assert len(words) == 7 and all(10 <= len(w) <= 20 for w in words)
    d_ids = torch.randint(0, 7, (n,), generator=g, device=dev, dtype=torch.int32)
    lens = torch.tensor([len(w) for w in words], dtype=torch.int64, device=dev)
    pad = torch.tensor([list(w.ljust(20, b"\0")) for w in words], dtype=torch.uint8, device=dev)
    d_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    torch.cumsum(lens[d_ids], 0, out=d_off[1:])
    d_bytes = pad[d_ids][(torch.arange(20, device=dev)[None, :] < lens[:, None])[d_ids]].contiguous()
    assert d_bytes.numel() == int(d_off[-1])
    d_val_cols = [decoder.DeviceColumn(abi.BYTE_ARRAY, d_off.view(torch.uint8), binary_data=d_bytes)]
    d_val_cols[0].n_values = n
    d_dict = decoder.DeviceColumn(abi.BYTE_ARRAY, torch.tensor([0] + list(np.cumsum([len(w) for w in words])), dtype=torch.int64,
                                                               device=dev).view(torch.uint8),
                                  binary_data=torch.tensor(list(b"".join(words)), dtype=torch.uint8, device=dev))
    d_dict.n_values = 7
    d_id_cols = [device_column(abi.BYTE_ARRAY, d_ids)]
    d_id_cols[0].flags, d_id_cols[0].dictionary = abi.COLUMN_DICTIONARY_IDS, d_dict
    d_pred = F.eq(F.col(0), words[1])
    d_filter_ids, d_filter_vals = F.Filter(d_pred, d_id_cols), F.Filter(d_pred, d_val_cols)
    d_table = torch.tensor([w == words[1] for w in words], dtype=torch.bool, device=dev)
    # (e) 1,000 distinct int64 entries in random order; lt(c, x) holds on 100 of them
    e_dict_vals = torch.randperm(1000, generator=g, device=dev).to(torch.int64) * 1_000_003
    e_ids = torch.randint(0, 1000, (n,), generator=g, device=dev, dtype=torch.int32)
    e_vals = e_dict_vals[e_ids].contiguous()
    e_val_cols = [device_column(abi.INT64, e_vals)]
    e_dict = device_column(abi.INT64, e_dict_vals)
    e_id_cols = [device_column(abi.INT64, e_ids)]
    e_id_cols[0].flags, e_id_cols[0].dictionary = abi.COLUMN_DICTIONARY_IDS, e_dict
    e_pred = F.lt(F.col(0), 100 * 1_000_003)
    e_filter_ids, e_filter_vals = F.Filter(e_pred, e_id_cols), F.Filter(e_pred, e_val_cols)

    n_words = (n + 63) // 64
    out = (torch.empty(n_words, dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.int64, device=dev),
           torch.empty(16, dtype=torch.uint8, device=dev))
    torch.cuda.synchronize()

    # results first: against torch on the same tensors
    sel = dec.filter(a_filter, a_cols, n, out=out)
    want = torch.nonzero(a_vals < 100).flatten()
    assert sel.count == want.numel() and torch.equal(sel.row_ids, want), "case (a) differs from torch"
    a_count = sel.count
    sel = dec.filter(b_filter, b_cols, n, out=out)
    # not_eq is true on a null row, lt_eq false
    want = torch.nonzero(((dl0 == 1) & (row_i <= 110)) & ((dl1 == 0) | (row_d != 7.0))).flatten()
    assert sel.count == want.numel() and torch.equal(sel.row_ids, want), "case (b) differs from torch"
    b_count = sel.count
    want = torch.nonzero(d_table[d_ids]).flatten()
    for flt, cols in ((d_filter_ids, d_id_cols), (d_filter_vals, d_val_cols)):
        sel = dec.filter(flt, cols, n, out=out)
        assert sel.count == want.numel() and torch.equal(sel.row_ids, want), "case (d) differs from torch"
    d_count = sel.count
    want = torch.nonzero(e_vals < 100 * 1_000_003).flatten()
    for flt, cols in ((e_filter_ids, e_id_cols), (e_filter_vals, e_val_cols)):
        sel = dec.filter(flt, cols, n, out=out)
        assert sel.count == want.numel() and torch.equal(sel.row_ids, want), "case (e) differs from torch"
    e_count = sel.count
    del want, row_i, row_d

    runs = {
        "a_hip": lambda: dec.filter(a_filter, a_cols, n, out=out),
        "a_torch": lambda: torch.nonzero(a_vals < 100),
        "b_hip": lambda: dec.filter(b_filter, b_cols, n, out=out),
        "d_ids": lambda: dec.filter(d_filter_ids, d_id_cols, n, out=out),
        "d_values": lambda: dec.filter(d_filter_vals, d_val_cols, n, out=out),
        "d_torch": lambda: torch.nonzero(d_table[d_ids]),
        "e_ids": lambda: dec.filter(e_filter_ids, e_id_cols, n, out=out),
        "e_values": lambda: dec.filter(e_filter_vals, e_val_cols, n, out=out),
    }
    runs = {k: fn for k, fn in runs.items() if k[0] in args.cases}
    times = {k: [] for k in runs}
    for k, fn in runs.items():
        timed(dec.stream, fn, args.warmup)
    for _ in range(args.repeats):
        for k, fn in runs.items():
            times[k].append(timed(dec.stream, fn, args.launches))

    a_bytes = 8 * n + 8 * n_words + 8 * a_count
    b_bytes = 8 * (b_i.numel() + b_d.numel()) + 2 * n + 8 * n_words + 8 * b_count
    meta = {"a_hip": ("lt(required int64)", a_bytes, a_count), "a_torch": ("torch.nonzero(values < x)", a_bytes, a_count),
            "b_hip": ("and_(lt_eq(nullable int64), not_eq(nullable double))", b_bytes, b_count)}
    out_bytes = lambda count: 8 * n_words + 8 * count  # noqa: E731
    meta.update({
        "d_ids": ("eq(BYTE_ARRAY) on uint32 ids + 7-entry dictionary", 4 * n + out_bytes(d_count), d_count),
        "d_values": ("eq(BYTE_ARRAY) on the materialised column", 8 * (n + 1) + d_bytes.numel() + out_bytes(d_count), d_count),
        "d_torch": ("torch.nonzero(table[ids])", 4 * n + out_bytes(d_count), d_count),
        "e_ids": ("lt(int64) on uint32 ids + 1,000-entry dictionary", 4 * n + out_bytes(e_count), e_count),
        "e_values": ("lt(int64) on the materialised column", 8 * n + out_bytes(e_count), e_count)})
    for k, ts in times.items():
        what, nbytes, count = meta[k]
        ms = float(np.median(ts))
        print(json.dumps({"case": k, "what": what, "rows": n, "selected": count, "ms_per_launch": round(ms, 4),
                          "ms_min": round(min(ts), 4), "ms_max": round(max(ts), 4), "repeats": len(ts),
                          "launches_per_repeat": args.launches, "algorithmic_bytes": nbytes,
                          "fraction_of_8TBps": round(nbytes / (ms * 1e-3) / PEAK_BYTES_PER_S, 4)}), flush=True)
    dec.close()


if __name__ == "__main__":
    main()
