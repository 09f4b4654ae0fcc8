"""Throughput of contains() on a list column (pqg_filter_run_records) on one MI355X.

    python tools/bench_filter_records.py [--slots 100000000] [--repeats 5] [--launches 20] [--cases eq1,eq50,in20]

The input is the list<int64> leaf of tools/bench_take.py case (r): about --slots slots in slots * 9 / 37
records, record lengths uniform 0..8, an empty list one slot at def 1 (max_def 2, max_rep 1). Predicates:
  eq1   contains(eq(c, x)) over values uniform in [0, 400): about 1 % of the records selected
  eq50  contains(eq(c, x)) over values uniform in [0, 5): about 50 %
  in20  contains(in(c, 20 members)) over values uniform in [0, 1000): about 7 %
Per predicate three runs on the same tensors, all with row ids:
  _hip    Decoder.filter_records
  _floor  (i) Decoder.filter on the same slots as a flat nullable column with the same leaf: the leaf
          evaluated per slot, no records (a bitmap and row ids per slot)
  _torch  (ii) what a user composes today: cumsum(rep == 0) - 1, the comparison on the dense values,
          index_reduce amax per record, packed to a bitmap, nonzero for the row ids
Every result is checked against the torch composition before anything is timed. Timing and reporting are
tools/bench_filter.py's: device events on the decoder's stream after warm-up launches, the runs alternate
inside a repeat, the median over the repeats of ms per launch with the smallest and largest repeat. One
JSON line per run; algorithmic bytes: both level bytes of every slot and the dense values read, the record
bitmap and the row ids written."""
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
from tools.bench_filter import PEAK_BYTES_PER_S, timed  # noqa: E402
from tools.bench_take import pack_bitmap  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=100_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cases", default="eq1,eq50,in20", help="of eq1,eq50,in20 (a profiler run takes one at a time)")
    ap.add_argument("--only", default="hip,floor,torch", help="runs to time, of hip,floor,torch")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_filter_records needs a GPU"
    cases, only = args.cases.split(","), args.only.split(",")
    dec = decoder.Decoder(0)
    dev = dec.device
    g = torch.Generator(device=dev)
    g.manual_seed(1)

    n_rec = args.slots * 9 // 37 // 64 * 64  # lengths 0..8 take (1 + 1 + 2 + ... + 8) / 9 slots on average
    lens = torch.randint(0, 9, (n_rec,), generator=g, device=dev, dtype=torch.int64)
    slots = torch.clamp(lens, min=1)
    starts = torch.cumsum(slots, 0) - slots
    n_slots = int(slots.sum())
    rl = torch.ones(n_slots, dtype=torch.uint8, device=dev)
    rl[starts] = 0
    dl = torch.full((n_slots,), 2, dtype=torch.uint8, device=dev)
    dl[starts[lens == 0]] = 1
    base = torch.randint(0, 1000, (int((dl == 2).sum()),), generator=g, device=dev, dtype=torch.int64)
    del slots, starts, lens
    members = [int(x) for x in np.random.default_rng(2).permutation(1000)[:20]]
    spec = {"eq1": (base % 400, F.eq(F.col(0), 7), "contains(eq), ~1 % of the records"),
            "eq50": (base % 5, F.eq(F.col(0), 3), "contains(eq), ~50 % of the records"),
            "in20": (base, F.in_(F.col(0), members), "contains(in) with 20 members")}

    acc = torch.uint8  # the narrowest type index_reduce takes here
    try:
        torch.zeros(2, dtype=acc, device=dev).index_reduce_(0, torch.zeros(1, dtype=torch.int64, device=dev),
                                                            torch.ones(1, dtype=acc, device=dev), "amax")
    except RuntimeError:
        acc = torch.int32

    def torch_contains(vals, leaf):
        rec_of = torch.cumsum(rl == 0, 0) - 1
        hit = torch.isin(vals, torch.tensor(leaf.values, device=dev)) if leaf.op == abi.FILTER_IN else vals == leaf.values[0]
        out = torch.zeros(n_rec, dtype=acc, device=dev)
        out.index_reduce_(0, rec_of[dl == 2], hit.to(acc), "amax")
        return pack_bitmap(out.bool()), torch.nonzero(out).flatten()

    runs, info = {}, {}
    for name in cases:
        vals, leaf, what = spec[name]
        vals = vals.contiguous()
        col = decoder.DeviceColumn(abi.INT64, vals.view(torch.uint8), dl, rl)
        col.n_values, col.max_def, col.max_rep, col.n_slots = vals.numel(), 2, 1, n_slots
        flat = decoder.DeviceColumn(abi.INT64, vals.view(torch.uint8), dl)
        flat.n_values, flat.max_def = vals.numel(), 2
        pred = F.Filter(F.contains(leaf), [col])
        flat_pred = F.Filter(leaf, [flat])
        out = (torch.empty(n_rec // 64, dtype=torch.int64, device=dev), torch.empty(n_rec, dtype=torch.int64, device=dev),
               torch.empty(16, dtype=torch.uint8, device=dev))
        flat_out = (torch.empty((n_slots + 63) // 64, dtype=torch.int64, device=dev),
                    torch.empty(n_slots, dtype=torch.int64, device=dev), torch.empty(16, dtype=torch.uint8, device=dev))
        # the result first
        want_bm, want_ids = torch_contains(vals, leaf)
        sel = dec.filter_records(pred, [col], n_rec, out=out)
        assert sel.count == want_ids.numel() and torch.equal(sel.bitmap, want_bm) and torch.equal(sel.row_ids, want_ids), \
            f"case {name} differs from torch"
        fsel = dec.filter(flat_pred, [flat], n_slots, out=flat_out)
        hit = torch.isin(vals, torch.tensor(leaf.values, device=dev)) if leaf.op == abi.FILTER_IN else vals == leaf.values[0]
        assert fsel.count == int(hit.sum()), f"case {name}: the floor differs from torch"
        info[name] = dict(what=what, selected=sel.count, values=vals.numel())
        del want_bm, want_ids, hit
        torch.cuda.synchronize()

        def hip(pred=pred, col=col, out=out):
            dec.filter_records(pred, [col], n_rec, out=out)

        def floor(flat_pred=flat_pred, flat=flat, flat_out=flat_out):
            dec.filter(flat_pred, [flat], n_slots, out=flat_out)

        def composed(vals=vals, leaf=leaf):
            torch_contains(vals, leaf)

        for kind, fn in (("hip", hip), ("floor", floor), ("torch", composed)):
            if kind in only:
                runs[f"{name}_{kind}"] = fn

    times = {k: [] for k in runs}
    for k, fn in runs.items():
        timed(dec.stream, fn, args.warmup)
    for _ in range(args.repeats):
        for k, fn in runs.items():
            times[k].append(timed(dec.stream, fn, args.launches))
    for k, ts in times.items():
        name = k.split("_")[0]
        i = info[name]
        nbytes = 2 * n_slots + 8 * i["values"] + n_rec // 8 + 8 * i["selected"]
        ms = float(np.median(ts))
        print(json.dumps({"case": k, "what": i["what"], "slots": n_slots, "records": n_rec, "selected": i["selected"],
                          "ms_per_launch": round(ms, 4), "ms_min": round(min(ts), 4), "ms_max": round(max(ts), 4),
                          "repeats": len(ts), "launches_per_repeat": args.launches, "algorithmic_bytes": nbytes,
                          "fraction_of_8TBps": round(nbytes / (ms * 1e-3) / PEAK_BYTES_PER_S, 4)}), flush=True)
    dec.close()


if __name__ == "__main__":
    main()
