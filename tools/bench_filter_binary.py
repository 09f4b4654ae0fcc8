"""Time record filters on DECIMAL columns (pqg_filter_create_typed filters) beside case (a) of
tools/bench_filter.py, in one process.

    python tools/bench_filter_binary.py [--rows 100000000] [--repeats 5] [--launches 20] [--cases afghi]

All with row ids, at about 10 % selected:
  (a) lt(required int64, x): the yardstick, as in tools/bench_filter.py
  (f) lt(required FLBA(16) DECIMAL, x) under the signed-integer order
  (g) the same on FLBA(5)
  (h) lt on a required BYTE_ARRAY DECIMAL column (value lengths 2 .. 16) under the signed-integer order
  (i) (f) on uint32 ids over a 1,000-entry FLBA(16) dictionary (pqg_filter_run_dict)
The values are int64 draws in [0, 1000) written as big-endian two's complement (for (h) sign-extended to a
length drawn per value); the results are checked against torch on those integers before anything is
timed. Timing and reporting are tools/bench_filter.py's: per repeat `launches` launches between two events,
the cases alternating inside a repeat; median, min and max of ms per launch, the algorithmic bytes (values +
offsets read, bitmap + row ids written) and their fraction of 8 TB/s. One JSON line per case."""
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
from tools.bench_filter import PEAK_BYTES_PER_S, device_column, timed  # noqa: E402


def big_endian(ints, width):
    """int64 tensor -> uint8 tensor [n, width]: big-endian two's complement, sign-extended."""
    shifts = torch.arange(width - 1, -1, -1, device=ints.device, dtype=torch.int64) * 8
    return ((ints[:, None] >> shifts.clamp(max=63)[None, :]) & 0xFF).to(torch.uint8)


def fixed_column(raw, width):
    col = decoder.DeviceColumn(abi.FIXED_LEN_BYTE_ARRAY, raw.reshape(-1), type_length=width)
    col.n_values = raw.shape[0]
    return col


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cases", default="afghi")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_filter_binary needs a GPU"
    n = args.rows
    dec = decoder.Decoder(0)
    dev = dec.device
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    signed = lambda i: F.col(i, order="signed_integer")  # noqa: E731

    a_vals = torch.randint(0, 1000, (n,), generator=g, device=dev, dtype=torch.int64)
    want = torch.nonzero(a_vals < 100).flatten()
    a_cols = [device_column(abi.INT64, a_vals)]
    f_cols = [fixed_column(big_endian(a_vals, 16), 16)]
    g_cols = [fixed_column(big_endian(a_vals, 5), 5)]
    # (h) the same integers, each sign-extended to a length of its own, 2 .. 16 bytes
    lens = torch.randint(2, 17, (n,), generator=g, device=dev, dtype=torch.int64)
    h_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    torch.cumsum(lens, 0, out=h_off[1:])
    wide = big_endian(a_vals, 16)
    h_bytes = wide[(torch.arange(16, device=dev)[None, :] >= (16 - lens)[:, None])].contiguous()
    del wide
    assert h_bytes.numel() == int(h_off[-1])
    h_cols = [decoder.DeviceColumn(abi.BYTE_ARRAY, h_off.view(torch.uint8), binary_data=h_bytes)]
    h_cols[0].n_values = n
    # (i) 1,000 entries in random order
    entry_ints = torch.randperm(1000, generator=g, device=dev).to(torch.int64)
    i_ids = torch.randint(0, 1000, (n,), generator=g, device=dev, dtype=torch.int32)
    i_want = torch.nonzero(entry_ints[i_ids.long()] < 100).flatten()
    i_cols = [device_column(abi.FIXED_LEN_BYTE_ARRAY, i_ids)]
    i_cols[0].flags, i_cols[0].dictionary = abi.COLUMN_DICTIONARY_IDS, fixed_column(big_endian(entry_ints, 16), 16)

    lit = F.decimal_bytes(100)
    filters = {"a": (F.Filter(F.lt(F.col(0), 100), a_cols), a_cols, want),
               "f": (F.Filter(F.lt(signed(0), lit), f_cols), f_cols, want),
               "g": (F.Filter(F.lt(signed(0), lit), g_cols), g_cols, want),
               "h": (F.Filter(F.lt(signed(0), lit), h_cols), h_cols, want),
               "i": (F.Filter(F.lt(signed(0), lit), i_cols), i_cols, i_want)}
    n_words = (n + 63) // 64
    out = (torch.empty(n_words, dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.int64, device=dev),
           torch.empty(16, dtype=torch.uint8, device=dev))
    torch.cuda.synchronize()
    counts = {}
    for name, (flt, cols, expect) in filters.items():
        sel = dec.filter(flt, cols, n, out=out)
        assert sel.count == expect.numel() and torch.equal(sel.row_ids, expect), f"case ({name}) differs from torch"
        counts[name] = sel.count
    del want, i_want

    runs = {name: (lambda flt=flt, cols=cols: dec.filter(flt, cols, n, out=out))
            for name, (flt, cols, _) in filters.items() if name in args.cases}
    times = {name: [] for name in runs}
    for fn in runs.values():
        timed(dec.stream, fn, args.warmup)
    for _ in range(args.repeats):
        for name, fn in runs.items():
            times[name].append(timed(dec.stream, fn, args.launches))

    out_bytes = lambda c: 8 * n_words + 8 * c  # noqa: E731
    meta = {"a": ("lt(required int64)", 8 * n), "f": ("lt(required FLBA(16) DECIMAL)", 16 * n),
            "g": ("lt(required FLBA(5) DECIMAL)", 5 * n),
            "h": ("lt(required BYTE_ARRAY DECIMAL, signed order)", 8 * (n + 1) + h_bytes.numel()),
            "i": ("lt(FLBA(16) DECIMAL) on uint32 ids + 1,000-entry dictionary", 4 * n)}
    for name, ts in times.items():
        what, read = meta[name]
        nbytes = read + out_bytes(counts[name])
        ms = float(np.median(ts))
        print(json.dumps({"case": name, "what": what, "rows": n, "selected": counts[name], "ms_per_launch": round(ms, 4),
                          "ms_min": round(min(ts), 4), "ms_max": round(max(ts), 4), "repeats": len(ts),
                          "launches_per_repeat": args.launches, "algorithmic_bytes": nbytes,
                          "fraction_of_8TBps": round(nbytes / (ms * 1e-3) / PEAK_BYTES_PER_S, 4)}), flush=True)
    dec.close()


if __name__ == "__main__":
    main()
