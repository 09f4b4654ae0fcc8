#!/usr/bin/env python3
"""Compare the gfx950 machine code of two builds, function by function.

    tools/isa_diff.py A B

A and B are device listings (hipcc ... --cuda-device-only -S -o x.s x.hip) or directories of them (*.s).
A function is matched by its mangled name, whichever file of a directory holds it. Compared: the
instructions between the entry label and .Lfunc_end, with comments stripped and .LBB<n>_ labels reduced to
.LBB_ (the function's index in its file), and, for kernels, vgpr_count, sgpr_count,
group_segment_fixed_size and private_segment_fixed_size of the code object's metadata.

Prints one line per function and exits 1 when a function differs or is on one side only.
"""
import os
import re
import sys

FIGURES = ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")


def listings(path):
    if os.path.isdir(path):
        return [os.path.join(path, f) for f in sorted(os.listdir(path)) if f.endswith(".s")]
    return [path]


def parse(path):
    """{name: (body lines, figures or None)} over the listing(s) at path."""
    bodies, figures = {}, {}
    for file in listings(path):
        with open(file) as f:
            lines = f.read().split("\n")
        name, body, entry = None, None, {}
        for line in lines:
            m = re.match(r"\s*\.type\s+(\S+),@function", line)
            if m:
                name, body = m.group(1), None
                continue
            if name and body is None:
                if line.startswith(name + ":"):
                    body = []
                continue
            if name:
                if re.match(r"\.Lfunc_end\d+:", line):
                    bodies[name], name, body = body, None, None
                    continue
                text = re.sub(r"\.LBB\d+_", ".LBB_", line.split(";")[0]).strip()
                if text:
                    body.append(text)
                continue
            # code object metadata: one "  - .key: value" entry per kernel, keys one per line
            if re.match(r"  - \.", line):
                entry = {}
            m = re.match(r"\s+(?:- )?\.(\w+):\s+(\S+)\s*$", line)
            if m:
                entry[m.group(1)] = m.group(2)
                if "name" in entry and all(k in entry for k in FIGURES):
                    figures[entry["name"]] = tuple(int(entry[k]) for k in FIGURES)
    return {n: (b, figures.get(n)) for n, b in bodies.items()}


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    a, b = parse(sys.argv[1]), parse(sys.argv[2])
    bad = 0
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            print(f"only in {'A' if name in a else 'B'}: {name}")
            bad += 1
            continue
        (body_a, fig_a), (body_b, fig_b) = a[name], b[name]
        same = body_a == body_b and fig_a == fig_b
        bad += not same
        fig = "" if fig_a is None else " " + " ".join(f"{k}={x}" + ("" if x == y else f"->{y}")
                                                      for k, x, y in zip(FIGURES, fig_a, fig_b or fig_a))
        print(f"{'equal    ' if same else 'DIFFERENT'} {len(body_a)} lines{fig} {name}")
        if body_a != body_b:
            first = next((i for i, (x, y) in enumerate(zip(body_a, body_b)) if x != y), min(len(body_a), len(body_b)))
            print(f"    first difference at instruction {first}: {body_a[first:first + 1]} / {body_b[first:first + 1]}")
    print(f"{len(set(a) | set(b))} functions, {bad} different")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
