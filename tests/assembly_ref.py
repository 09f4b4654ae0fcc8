"""A vectorised reference for record assembly, and level generators for sizes the per-slot automaton
(oracle/assembly.py) cannot reach in a test's time.

closed_form() restates the definition in the header comment of csrc/pqgpu_assembly.hip with numpy
(int64 cumulative sums and boolean indexing, nothing of the kernel's structure):
  slot i begins an entry of depth q   when rl[i] <= q and dl[i] >= DR[q]
  (DR[0] = 0, DR[r] = definition level of the r-th REPEATED node);
  OPTIONAL node k at depth q:  validity = dl[i] >= D(k) over the depth-q entry slots;
  REPEATED node at depth q:    offsets = exclusive count of depth-q entries at every depth-(q - 1) entry
                               slot, then the total;
  records = depth-0 entries.
tests/test_assembly_ref.py pins it to the automaton on every path and generator below.

is_valid_levels() is the predicate "a sequence a writer produces"; every generator asserts it on
what it returns."""
import numpy as np

from oracle import assembly as A

from test_gpu_assembly import PATHS, random_levels

R, O, P = A.REQUIRED, A.OPTIONAL, A.REPEATED

B = 8192  # slots of a one-pass block (k_asm_onepass)
C = 4096  # slots of a count-pass block (k_asm_count)

PATH_15 = [O, P] * 7 + [O]        # 15 nodes, max_rep 7, max_def 15
PATHS_DEEP = PATHS + [
    [P, O],                       # max_rep 1 (MD 2)
    [P, P],                       # max_rep 2 (MD 4)
    [P, P, P, R],                 # max_rep 3 (MD 4)
    [P, P, P, P, O],              # max_rep 4 (MD 8)
    [O, P, P, O, P, P, R, P, O],  # max_rep 5
    [P] * 7,                      # max_rep 7
    PATH_15,
    [R] + PATH_15,                # 16 nodes = ASM_MAX_NODES
]


def path_id(path):
    return "".join("ROP"[rp] for rp in path)


def path_levels(path):
    """(max_rep, max_def, DR, depth of every node, definition level of every node)."""
    lv = A.levels_of(path)
    DR = [0] + [lv[k][1] for k in range(len(path)) if path[k] == P]
    return lv[-1][0], lv[-1][1], DR, [r for r, _ in lv], [d for _, d in lv]


def closed_form(path, rl, dl):
    """Columnar form of the records: {"records", "n_entries": [per node], "validity": {k: uint8 array},
    "offsets": {k: int64 array}}. A level that the path does not have (max 0) counts as all zeros."""
    max_r, max_d, DR, depth, D = path_levels(path)
    dl = np.asarray(dl).astype(np.int64)
    n = dl.size
    rl = np.asarray(rl).astype(np.int64) if max_r > 0 else np.zeros(n, dtype=np.int64)
    if max_d == 0:
        dl = np.zeros(n, dtype=np.int64)
    begins = [(rl <= q) & (dl >= DR[q]) for q in range(max_r + 1)]
    count = [int(b.sum(dtype=np.int64)) for b in begins]
    validity, offsets = {}, {}
    for k, rp in enumerate(path):
        q = depth[k]
        if rp == O:
            validity[k] = (dl[begins[q]] >= D[k]).astype(np.uint8)
        elif rp == P:
            before = np.cumsum(begins[q], dtype=np.int64) - begins[q]
            offsets[k] = np.concatenate([before[begins[q - 1]], np.array([count[q]], dtype=np.int64)])
    return {"records": count[0], "n_entries": [count[q] for q in depth], "validity": validity, "offsets": offsets}


def is_valid_levels(path, rl, dl):
    """r_0 = 0; levels within their maxima; a slot of repetition level r has the r-th REPEATED node
    defined (d >= DR[r]) and follows a slot that reached it (DR[r] <= d of the slot before)."""
    max_r, max_d, DR, _, _ = path_levels(path)
    rl = np.asarray(rl).astype(np.int64)
    dl = np.asarray(dl).astype(np.int64)
    if rl.size != dl.size:
        return False
    if rl.size == 0:
        return True
    if rl[0] != 0 or rl.max() > max_r or dl.max() > max_d or rl.min() < 0 or dl.min() < 0:
        return False
    dr = np.asarray(DR, dtype=np.int64)
    if not (dl >= dr[rl]).all():
        return False
    reach = np.searchsorted(dr, dl[:-1], side="right") - 1  # deepest q with DR[q] <= d of the slot before
    return bool((rl[1:] <= reach).all())


def _checked(path, rl, dl):
    rl = np.ascontiguousarray(rl, dtype=np.uint8)
    dl = np.ascontiguousarray(dl, dtype=np.uint8)
    assert is_valid_levels(path, rl, dl)
    return rl, dl


def pooled(path, n, rng):
    """Random picks from a pool of about 64 short valid sequences (1..40 slots each, per-slot
    random_levels), concatenated to exactly n slots; the last pick is cut (a prefix of a valid
    sequence is valid, and every piece begins a record)."""
    lens = rng.integers(1, 41, size=64)
    pieces = [random_levels(path, int(L), rng) for L in lens]
    pool_r = np.concatenate([p[0] for p in pieces])
    pool_d = np.concatenate([p[1] for p in pieces])
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]])
    picks = np.empty(0, dtype=np.int64)
    while int(lens[picks].sum()) < n:
        picks = np.concatenate([picks, rng.integers(0, 64, size=n // 16 + 8)])
    L = lens[picks]
    out0 = np.cumsum(L) - L                                   # first output slot of every pick
    idx = (np.repeat(starts[picks] - out0, L) + np.arange(int(L.sum())))[:n]
    return _checked(path, pool_r[idx], pool_d[idx])


def one_record(path, n, rng):
    """One record over all n slots: a pooled sequence whose later record starts become
    continuations of the first REPEATED node (r = 1), every slot having that node defined."""
    max_r, _, DR, _, _ = path_levels(path)
    assert max_r >= 1
    rl, dl = pooled(path, n, rng)
    rl = rl.copy()
    rl[1:][rl[1:] == 0] = 1
    return _checked(path, rl, np.maximum(dl, DR[1]))


def all_null(path, n):
    return _checked(path, np.zeros(n), np.zeros(n))


def dense(path, n):
    """Every slot begins an entry of every depth."""
    return _checked(path, np.zeros(n), np.full(n, path_levels(path)[1]))


def deepest_only(path, n):
    """One entry of every depth but the deepest, which has n."""
    max_r, max_d, _, _, _ = path_levels(path)
    rl = np.full(n, max_r)
    rl[:1] = 0
    return _checked(path, rl, np.full(n, max_d))


KINDS = ("pooled", "one_record", "all_null", "dense", "deepest_only")


def make(kind, path, n, rng):
    if kind == "pooled":
        return pooled(path, n, rng)
    if kind == "one_record":
        return one_record(path, n, rng)
    return {"all_null": all_null, "dense": dense, "deepest_only": deepest_only}[kind](path, n)


def blocks_of(kinds, path, rng, lengths=None):
    """Segments of the given kinds back to back, B slots each unless `lengths` says otherwise. Every
    kind begins with r = 0, so the joined sequence stays valid; neighbouring segments then have zero
    and full counts per depth."""
    lengths = [B] * len(kinds) if lengths is None else lengths
    parts = [make(kind, path, int(L), rng) for kind, L in zip(kinds, lengths)]
    return _checked(path, np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]))


MIXTURES = [
    ("dense", "all_null", "all_null", "dense"),
    ("one_record", "all_null", "one_record"),
    ("all_null", "deepest_only", "pooled", "all_null"),
    ("deepest_only", "dense", "one_record", "deepest_only"),
    ("all_null", "all_null", "dense"),
]
