"""Row-group dictionary filter: one call for a whole file against the per-group loop it replaces.

    python tools/bench_rowgroups.py [--groups 1000] [--entries 1000] [--reps 20] [--out out/rowgroups.json]

For 1,000 row groups of one int64 column (1k-entry dictionaries, the C2 shape) and of one string column, and
and(eq, in) predicates chosen to drop none, half and all of the groups, three ways to the same answer:

  new    Decoder.decode_dictionaries on the dictionary pages of every row group + Decoder.filter_row_groups:
         one plan and one filter call, whatever the number of row groups
  loop   what the calls before this feature allow: per row group decode_dictionary, then Decoder.filter on the
         dictionary as a column ("does the predicate hold on some entry"), one count read back per group. It
         answers this predicate shape (no nulls, eq / in) only; it is here for the launch and sync cost
  cpu    the NumPy restatement of DictionaryFilter on the host dictionaries (np.isin per group)

Times are host clocks around work that ends in a stream synchronise, median over --reps after a warm-up, with
the dictionary upload outside the window. Launch counts are stated from the code, not measured: the new path
queues the launches of one decode plan plus one memset and four launches for the filter, independent of the
number of row groups; the loop queues a plan, a filter (three launches here) and two synchronisations per group.
Every variant's drop bits are compared before anything is timed. Prints one JSON object."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "parquet-mr_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from pqgpu import abi, batch  # noqa: E402
from pqgpu import decoder as D  # noqa: E402
from pqgpu import filter as F  # noqa: E402
from tools.synth import writer  # noqa: E402


PROBES = {"none": 13, "half": 7, "all": 5}   # eq literal: held by every group, by the even groups, by no group
MEMBERS = (11, 1, 2)                          # in set: 11 is held by every group


def make_groups(kind, n_groups, n_entries, rng):
    """Per row group the dictionary entries (host) of one column: distinct values from 1,000 up, with 11 and 13
    in every group and 7 in the even ones."""
    assert n_entries >= 3
    groups = []
    for g in range(n_groups):
        vals = rng.choice(np.arange(1_000, 1_000_000), size=n_entries, replace=False).astype(np.int64)
        vals[:2] = (11, 13)
        if g % 2 == 0:
            vals[2] = 7
        rng.shuffle(vals)
        groups.append(vals if kind == "int64" else [b"key-%012d" % int(v) for v in vals])
    return groups


def lit(kind, v):
    return int(v) if kind == "int64" else b"key-%012d" % int(v)


def predicates(kind):
    """name -> and(eq, in) that drops none, half, all of the groups."""
    c = F.col(0)
    return {name: F.and_(F.eq(c, lit(kind, probe)), F.in_(c, [lit(kind, m) for m in MEMBERS]))
            for name, probe in PROBES.items()}


def cpu_reference(kind, name, groups):
    """DictionaryFilter on the host dictionaries: the drop bit per group (no nulls, every page dictionary-encoded):
    eq cannot match without its literal among the entries, in without a member; and drops on either."""
    probe, members = lit(kind, PROBES[name]), [lit(kind, m) for m in MEMBERS]
    drops = np.zeros(len(groups), dtype=bool)
    for g, entries in enumerate(groups):
        if kind == "int64":
            drops[g] = not (entries == probe).any() or not np.isin(entries, members).any()
        else:
            have = set(entries)
            drops[g] = probe not in have or not any(m in have for m in members)
    return drops


def timed(fn, sync, reps):
    fn()
    sync()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        sync()
        times.append(time.perf_counter() - t0)
    return float(np.median(times)) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=1000)
    ap.add_argument("--entries", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--loop-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dec = D.Decoder(0)
    rng = np.random.default_rng(1)
    report = {"groups": args.groups, "entries": args.entries, "cases": []}
    for kind, t in (("int64", abi.INT64), ("string", abi.BYTE_ARRAY)):
        groups = make_groups(kind, args.groups, args.entries, rng)
        chunks = [batch.ColumnChunk(physical_type=t, pages=[], dict_page=writer.plain_encode(e, t), dict_num_values=len(e),
                                    dict_encoding=abi.PLAIN) for e in groups]
        dbatch = dec.upload_chunks(chunks)  # dictionary pages only
        n = args.groups
        for name, pred in predicates(kind).items():
            flt = F.Filter(pred, [t])
            state = {}

            def new():
                dicts = dec.decode_dictionaries(dbatch, range(n))
                state["sel"] = dec.filter_row_groups(flt, [[F.RowGroupColumn(d, may_contain_null=False)] for d in dicts])

            def loop():
                # per group: the dictionary as a required column; a group drops when either side of the and holds
                # on no entry (the leaf selects no "row" of it)
                drops = np.zeros(n, dtype=bool)
                for g in range(n):
                    d = dec.decode_dictionary(dbatch, g)
                    cannot = False
                    for leaf in pred.children:
                        cannot = cannot or dec.filter(leaf, [d], d.n_values, row_ids=False).count == 0
                    drops[g] = cannot
                state["loop"] = drops

            new()
            loop()
            want = cpu_reference(kind, name, groups)
            got = state["sel"].drop.cpu().numpy()
            assert np.array_equal(got, want), (kind, name, "filter_row_groups differs from the CPU reference")
            assert np.array_equal(state["loop"], want), (kind, name, "the per-group loop differs from the CPU reference")
            sync = dec.stream.synchronize
            case = {"column": kind, "predicate": name, "dropped": int(want.sum()),
                    "new_ms": timed(new, lambda: state["sel"].count, args.reps),
                    "filter_only_ms": None,
                    "loop_ms": timed(loop, sync, args.loop_reps),
                    "cpu_ms": timed(lambda: cpu_reference(kind, name, groups), lambda: None, max(args.loop_reps, 3))}
            dicts = dec.decode_dictionaries(dbatch, range(n))
            table = [[F.RowGroupColumn(d, may_contain_null=False)] for d in dicts]
            case["filter_only_ms"] = timed(lambda: state.__setitem__("sel", dec.filter_row_groups(flt, table)),
                                           lambda: state["sel"].count, args.reps)
            report["cases"].append(case)
            print(json.dumps(case), file=sys.stderr, flush=True)
    text = json.dumps(report)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)
    dec.close()


if __name__ == "__main__":
    main()
