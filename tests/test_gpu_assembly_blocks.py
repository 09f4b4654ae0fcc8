"""pqg_assemble at its seams, bit-exact against the vectorised closed form (tests/assembly_ref.py, pinned
to the automaton by tests/test_assembly_ref.py): the three depth classes of k_asm_onepass (MD = 2, 4, 8),
sizes on thread / count-block / one-pass-block boundaries, blocks with zero and with full counts per
depth, more than 64 predecessor blocks, more than 1,024 count blocks, level and output arrays off their
natural alignment, and the capacity contract of include/pqgpu.h with guard bytes round every output.

Two routes reach the output kernel and every correctness case takes both: decoder.assemble (count pass,
capacity check, then the one-pass kernel) and decoder.assemble_schema with a single leaf (capacities at
the bound, the one-pass kernel alone). raw_assemble() calls pqg_assemble itself where a test needs
capacities, NULL outputs or output addresses the wrappers do not give."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from pqgpu import abi, native

import assembly_ref as AR
from assembly_ref import B, C as CB, O, P, PATHS_DEEP, PATH_15, R, path_id

pytestmark = pytest.mark.gpu

GUARD = 64
POISON = 0xA5
P7 = [P] * 7
OPO = [O, P, O]
PPPR = [P, P, P, R]
PPPPO = [P, P, P, P, O]
CAP_PATH = [O, P, P, O, P, P, R, P, O]
LONG = 66 * B + 17  # more than 64 predecessor blocks


# ---- inputs and references (computed once per case, read-only) -----------------------------------

@functools.lru_cache(maxsize=16)
def case(pid, kind, n, seed=0):
    """(rl, dl, closed form) of a generated case; kind: a generator's name, a tuple of block kinds
    (whole blocks; (kinds, lengths) for other lengths), "bytes" / "bytes_max1" for arbitrary bytes."""
    path = PATHS_DEEP[pid]
    rng = np.random.default_rng([pid, n, seed])
    if kind == "bytes":
        rl, dl = (rng.integers(0, 256, size=n, dtype=np.uint8) for _ in range(2))
    elif kind == "bytes_max1":
        max_r, max_d = AR.path_levels(path)[:2]
        rl = rng.integers(0, max_r + 2, size=n, dtype=np.uint8)
        dl = rng.integers(0, max_d + 2, size=n, dtype=np.uint8)
    elif isinstance(kind, tuple):
        kinds, lengths = kind if isinstance(kind[0], tuple) else (kind, None)
        rl, dl = AR.blocks_of(kinds, path, rng, lengths)
        assert rl.size == n
    else:
        rl, dl = AR.make(kind, path, n, rng)
    exp = AR.closed_form(path, rl, dl)
    for a in [rl, dl, *exp["validity"].values(), *exp["offsets"].values()]:
        a.flags.writeable = False
    return rl, dl, exp


def pid_of(path):
    return PATHS_DEEP.index(path)


def upload(decoder, path, rl, dl, o_def=0, o_rep=0):
    """Device level tensors (None where the path has no such level), starting o_def / o_rep bytes
    into their allocations."""
    max_r, max_d = AR.path_levels(path)[:2]

    def dev(a, o):
        buf = torch.zeros(o + max(a.size, 1) + 16, dtype=torch.uint8, device=decoder.device)
        buf[o:o + a.size].copy_(torch.from_numpy(np.array(a)))
        t = buf[o:o + max(a.size, 1)]
        assert t.data_ptr() % 256 == o % 256
        return t
    return (dev(dl, o_def) if max_d > 0 else None), (dev(rl, o_rep) if max_r > 0 else None)


# ---- the two routes of the wrappers --------------------------------------------------------------

def normal(path, got):
    out = {"records": got["records"], "n_entries": [nd["n_entries"] for nd in got["nodes"]], "validity": {}, "offsets": {}}
    for k, rp in enumerate(path):
        if rp == O:
            out["validity"][k] = got["nodes"][k]["validity"].cpu().numpy()
        if rp == P:
            out["offsets"][k] = got["nodes"][k]["offsets"].cpu().numpy()
    return out


def counted_route(decoder, path, n, dt, rt):
    return normal(path, decoder.assemble(path, n, dt, rt))


def onepass_route(decoder, path, n, dt, rt):
    nodes = [(k - 1, rp) for k, rp in enumerate(path)]
    return normal(path, decoder.assemble_schema(nodes, [(len(path) - 1, dt, rt, n)]))


def same(path, got, exp, what):
    assert got["records"] == exp["records"], what
    assert got["n_entries"] == exp["n_entries"], what
    for key, dt in (("validity", np.uint8), ("offsets", np.int64)):
        for k, e in exp[key].items():
            g = got[key][k]
            assert g.dtype == dt and g.shape == e.shape and np.array_equal(g, e), f"{what}: {key} of node {k}"


def both_routes(decoder, path, rl, dl, exp, o_def=0, o_rep=0, routes=(counted_route, onepass_route)):
    dt, rt = upload(decoder, path, rl, dl, o_def, o_rep)
    got = [route(decoder, path, rl.size, dt, rt) for route in routes]
    for route, g in zip(routes, got):
        same(path, g, exp, route.__name__)
    for g in got[1:]:  # (implied by the above; the routes count in different kernels)
        assert g["records"] == got[0]["records"] and g["n_entries"] == got[0]["n_entries"]


# ---- pqg_assemble itself -------------------------------------------------------------------------

class Raw:
    pass


def raw_assemble(decoder, path, n, dt, rt, outs):
    """pqg_assemble through ctypes. outs[k]: None (a NULL output) or (capacity, byte offset): the
    output starts GUARD + byte offset bytes into a 256-byte aligned allocation filled with 0xA5 that
    ends GUARD bytes after the capacity. Returns rc, the status, records, n_entries, per node the
    output's elements (offsets decoded from bytes: they may sit off 8-byte alignment), the output's bytes
    and the bytes round it."""
    depth = len(path)
    nodes = (abi.AssemblyNode * depth)()
    bufs = [None] * depth
    for k, rp in enumerate(path):
        nodes[k].repetition = rp
        if outs[k] is None:
            continue
        cap, off = outs[k]
        size = cap * (8 if rp == P else 1)
        bufs[k] = torch.full((GUARD + off + size + GUARD,), POISON, dtype=torch.uint8, device=decoder.device)
        assert bufs[k].data_ptr() % 256 == 0
        ptr = bufs[k].data_ptr() + GUARD + off
        if rp == P:
            nodes[k].offsets = ptr
        else:
            nodes[k].validity = ptr
        nodes[k].capacity = cap
    torch.cuda.synchronize(decoder.device)
    n_rec = C.c_uint64(0)
    st = abi.Status()
    res = Raw()
    res.rc = native.lib().pqg_assemble(decoder.ctx, dt.data_ptr() if dt is not None else None,
                                       rt.data_ptr() if rt is not None else None, n, C.addressof(nodes), depth,
                                       C.byref(n_rec), C.byref(st))
    res.code, res.page, res.value_index, res.message = st.code, st.page, st.value_index, st.message
    res.records = int(n_rec.value)
    res.n_entries = [int(nodes[k].n_entries) for k in range(depth)]
    res.out, res.bytes, res.around = [None] * depth, [None] * depth, [None] * depth
    for k, rp in enumerate(path):
        if outs[k] is None:
            continue
        cap, off = outs[k]
        whole = bufs[k].cpu().numpy()
        lo, hi = GUARD + off, whole.size - GUARD
        res.bytes[k] = whole[lo:hi]
        res.around[k] = np.concatenate([whole[:lo], whole[hi:]])
        res.out[k] = np.frombuffer(whole[lo:hi].tobytes(), dtype=np.int64) if rp == P else whole[lo:hi]
        assert res.out[k].size == cap
    return res


def needs(path, exp):
    """Elements every node's output needs (0 for REQUIRED nodes)."""
    return [exp["validity"][k].size if rp == O else exp["offsets"][k].size if rp == P else 0 for k, rp in enumerate(path)]


def untouched(a):
    return bool((a == POISON).all())


def raw_ok(path, res, exp, outs, what=""):
    """PQG_OK, the counts, every given output equal to the closed form in its needed range and 0xA5
    past it, every guard byte 0xA5."""
    assert res.rc == abi.OK and res.code == abi.OK, (what, res.rc, res.message)
    assert res.records == exp["records"] and res.n_entries == exp["n_entries"], what
    need = needs(path, exp)
    for k, rp in enumerate(path):
        if outs[k] is None:
            continue
        e = exp["offsets"][k] if rp == P else exp["validity"][k]
        assert np.array_equal(res.out[k][:need[k]], e), f"{what}: output of node {k}"
        assert untouched(res.bytes[k][need[k] * (8 if rp == P else 1):]), f"{what}: node {k} written past its entries"
        assert untouched(res.around[k]), f"{what}: guard bytes of node {k}"


def raw_counts_only(path, res, exp):
    assert res.records == exp["records"] and res.n_entries == exp["n_entries"]


# ---- 1. depth classes x sizes on every boundary --------------------------------------------------

SIZES = [1, 15, 16, 17, CB - 1, CB, CB + 1, B - 1, B, B + 1, 2 * B - 1, 2 * B, 2 * B + 1, 3 * B + 5]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("pid", range(len(PATHS_DEEP)), ids=[path_id(p) for p in PATHS_DEEP])
def test_depth_classes_at_boundaries(decoder, pid, n):
    rl, dl, exp = case(pid, "pooled", n)
    both_routes(decoder, PATHS_DEEP[pid], rl, dl, exp)


# ---- 2. shapes: blocks with zero and with full counts per depth ----------------------------------

SHAPE_PATHS = [OPO, PPPR, PPPPO, P7, PATH_15]
SEAMS = [(("one_record", "all_null"), (2 * B + e, B + 3)) for e in (0, -1, 1)]  # the record ends at / before / after a block end
SHAPE_CASES = ([(kind, n) for kind in ("one_record", "all_null", "dense", "deepest_only") for n in (B, 3 * B + 5)]
               + [(mix, len(mix) * B) for mix in AR.MIXTURES]
               + [((mix, (B,) * (len(mix) - 1) + (B + 5,)), len(mix) * B + 5) for mix in AR.MIXTURES]
               + [(seam, sum(seam[1])) for seam in SEAMS])


def shape_id(c):
    kind, n = c
    if isinstance(kind, str):
        return f"{kind}-{n}"
    kinds, lengths = kind if isinstance(kind[0], tuple) else (kind, None)
    return "+".join(kinds) + (f"-{n}" if lengths else "")


@pytest.mark.parametrize("shape", SHAPE_CASES, ids=shape_id)
@pytest.mark.parametrize("path", SHAPE_PATHS, ids=path_id)
def test_shapes(decoder, path, shape):
    kind, n = shape
    rl, dl, exp = case(pid_of(path), kind, n)
    both_routes(decoder, path, rl, dl, exp)


# ---- 3. more than 64 predecessor blocks ----------------------------------------------------------

@pytest.mark.parametrize("kind", ["pooled", "one_record"])
@pytest.mark.parametrize("path", [OPO, PPPR, P7], ids=path_id)
def test_long_look_back(decoder, path, kind):
    """67 one-pass blocks: the last ones have more than 64 predecessors. In one_record only block 0 has
    a depth-0 entry, so a depth-0 look-back that finds no nearer inclusive count walks past 64 aggregates
    of 0 (the word 'published, count 0' differs from 'not published' by its flag alone). Whether a
    look-back takes its second step depends on how far the predecessors have got when it reads them
    (a predecessor that has published its inclusive count ends the walk at once) and cannot be forced;
    these sizes make it possible."""
    rl, dl, exp = case(pid_of(path), kind, LONG)
    if kind == "one_record":
        assert exp["records"] == 1
    both_routes(decoder, path, rl, dl, exp)


# ---- 4. more than 1,024 count blocks: k_asm_scan with two blocks per thread ----------------------

@pytest.mark.parametrize("path", [OPO, PPPPO], ids=path_id)
def test_scan_segments(decoder, path):
    """1,027 count blocks: seg = 2, threads 0..513 hold blocks, the rest none."""
    n = 1026 * CB + 1
    rl, dl, exp = case(pid_of(path), "pooled", n)
    both_routes(decoder, path, rl, dl, exp, routes=(counted_route,))
    # the counts alone (no outputs: count pass and scan only)
    dt, rt = upload(decoder, path, rl, dl)
    raw_counts_only(path, raw_assemble(decoder, path, n, dt, rt, [None] * len(path)), exp)


# ---- 5. level arrays off 16-byte alignment -------------------------------------------------------

@pytest.mark.parametrize("o_def,o_rep", [(1, 8), (8, 15), (15, 1), (0, 1), (8, 0)])
@pytest.mark.parametrize("path", [OPO, PPPPO], ids=path_id)
def test_input_alignment(decoder, path, o_def, o_rep):
    rl, dl, exp = case(pid_of(path), "pooled", 2 * B + 3)
    both_routes(decoder, path, rl, dl, exp, o_def, o_rep)


# ---- 6. output arrays off their alignment --------------------------------------------------------

@pytest.mark.parametrize("off_o", [8, 4])
@pytest.mark.parametrize("off_v", [1, 3, 15])
@pytest.mark.parametrize("kind", ["pooled", "dense"])
@pytest.mark.parametrize("path", [OPO, CAP_PATH], ids=path_id)
def test_output_alignment(decoder, path, kind, off_v, off_o):
    """Validity from byte 1, 3 or 15 of a 16-byte line (block 0 has a head of bytes); offsets from byte 8
    (8- but not 16-byte aligned: block 0 stores one entry before its pairs) or byte 4 (one entry per store)."""
    n = 2 * B + 3
    rl, dl, exp = case(pid_of(path), kind, n)
    dt, rt = upload(decoder, path, rl, dl)
    need = needs(path, exp)
    off = [off_o if rp == P else off_v for rp in path]
    exact = [None if rp == R else (need[k], off[k]) for k, rp in enumerate(path)]
    bound = [None if rp == R else (n + 1 if rp == P else n, off[k]) for k, rp in enumerate(path)]
    raw_ok(path, raw_assemble(decoder, path, n, dt, rt, exact), exp, exact, "exact capacities")
    raw_ok(path, raw_assemble(decoder, path, n, dt, rt, bound), exp, bound, "capacities at the bound")


# ---- 7. the capacity contract --------------------------------------------------------------------

CAP_N = 2 * B + 3
CAP_OUT = [k for k, rp in enumerate(CAP_PATH) if rp != R]


def cap_case(decoder):
    rl, dl, exp = case(pid_of(CAP_PATH), "pooled", CAP_N)
    dt, rt = upload(decoder, CAP_PATH, rl, dl)
    need = needs(CAP_PATH, exp)
    assert all(0 < need[k] < CAP_N for k in CAP_OUT)  # every output is smaller than its bound
    return exp, dt, rt, need


def test_capacity_exact(decoder):
    exp, dt, rt, need = cap_case(decoder)
    outs = [(need[k], 0) if k in CAP_OUT else None for k in range(len(CAP_PATH))]
    raw_ok(CAP_PATH, raw_assemble(decoder, CAP_PATH, CAP_N, dt, rt, outs), exp, outs)


@pytest.mark.parametrize("short", CAP_OUT)
def test_capacity_one_short_writes_nothing(decoder, short):
    """One output an element short, the others exact: PQG_ERR_INVALID_ARG naming the node, every count
    filled in, and not one byte of any output or guard written."""
    exp, dt, rt, need = cap_case(decoder)
    outs = [(need[k] - (k == short), 0) if k in CAP_OUT else None for k in range(len(CAP_PATH))]
    res = raw_assemble(decoder, CAP_PATH, CAP_N, dt, rt, outs)
    assert res.rc == abi.ERR_INVALID_ARG and res.code == abi.ERR_INVALID_ARG
    assert res.value_index == short and res.page == -1
    raw_counts_only(CAP_PATH, res, exp)
    for k in CAP_OUT:
        assert untouched(res.bytes[k]) and untouched(res.around[k]), f"node {k} written"


def test_capacity_at_the_bound(decoder):
    exp, dt, rt, need = cap_case(decoder)
    outs = [(CAP_N + (CAP_PATH[k] == P), 0) if k in CAP_OUT else None for k in range(len(CAP_PATH))]
    raw_ok(CAP_PATH, raw_assemble(decoder, CAP_PATH, CAP_N, dt, rt, outs), exp, outs)


@pytest.mark.parametrize("at_bound", [0, 1, 8])
def test_capacity_mixed(decoder, at_bound):
    """One node at the bound, the others exact: not sized for any content, so counted first."""
    exp, dt, rt, need = cap_case(decoder)
    outs = [(need[k], 0) if k in CAP_OUT else None for k in range(len(CAP_PATH))]
    outs[at_bound] = (CAP_N + (CAP_PATH[at_bound] == P), 0)
    raw_ok(CAP_PATH, raw_assemble(decoder, CAP_PATH, CAP_N, dt, rt, outs), exp, outs)


@pytest.mark.parametrize("only", [(k,) for k in CAP_OUT] + [tuple(k for k in CAP_OUT if CAP_PATH[k] == O), ()],
                         ids=lambda t: "none" if not t else "node" + "_".join(map(str, t)))
def test_capacity_some_outputs(decoder, only):
    """NULL outputs for all nodes but some (one node alone; every OPTIONAL node and no REPEATED one;
    none at all: counts only), at exact capacities and at the bound."""
    exp, dt, rt, need = cap_case(decoder)
    for cap in (lambda k: need[k], lambda k: CAP_N + (CAP_PATH[k] == P)):
        outs = [(cap(k), 0) if k in only else None for k in range(len(CAP_PATH))]
        raw_ok(CAP_PATH, raw_assemble(decoder, CAP_PATH, CAP_N, dt, rt, outs), exp, outs)


# ---- 8. argument errors (before any launch) and empty columns ------------------------------------

def test_argument_errors(decoder):
    rl, dl, _ = case(pid_of(OPO), "pooled", 17)
    dt, rt = upload(decoder, OPO, rl, dl)

    def call(path, d=dt, r=rt, n=17):
        return raw_assemble(decoder, path, n, d, r, [None] * len(path))
    res = call([O] * 17)
    assert res.rc == abi.ERR_INVALID_ARG and res.code == abi.ERR_INVALID_ARG
    res = call([P] * 8)
    assert res.rc == abi.ERR_UNSUPPORTED and res.code == abi.ERR_UNSUPPORTED and res.value_index == 7
    res = call([O, 3, O])
    assert res.rc == abi.ERR_INVALID_ARG and res.value_index == 1
    res = call(OPO, d=None)
    assert res.rc == abi.ERR_INVALID_ARG and res.code == abi.ERR_INVALID_ARG
    res = call(OPO, r=None)
    assert res.rc == abi.ERR_INVALID_ARG and res.code == abi.ERR_INVALID_ARG
    assert call([R], d=None, r=None).rc == abi.OK        # no levels to give: max_def = max_rep = 0
    assert call(OPO, d=None, r=None, n=0).rc == abi.OK   # nor for no slots


@pytest.mark.parametrize("pid", range(len(PATHS_DEEP)), ids=[path_id(p) for p in PATHS_DEEP])
def test_no_slots(decoder, pid):
    path = PATHS_DEEP[pid]
    rl, dl, exp = case(pid, "pooled", 0)
    assert exp["records"] == 0 and all(o.tolist() == [0] for o in exp["offsets"].values())
    both_routes(decoder, path, rl, dl, exp)
    dt, rt = upload(decoder, path, rl, dl)
    outs = [None if rp == R else (1 if rp == P else 0, 0) for rp in path]
    res = raw_assemble(decoder, path, 0, dt, rt, outs)
    raw_ok(path, res, exp, outs)
    assert all(res.out[k].tolist() == [0] for k, rp in enumerate(path) if rp == P)


# ---- 9. one context, long and short calls in turn ------------------------------------------------

def test_scratch_reuse(decoder):
    """The status words and totals of a long call must not reach a shorter one after it."""
    for path, n in [(P7, LONG), (OPO, 5), (P7, B + 1), (OPO, LONG), (P7, 5), (OPO, B + 1), (P7, LONG)]:
        rl, dl, exp = case(pid_of(path), "pooled", n)
        both_routes(decoder, path, rl, dl, exp)


# ---- 10. arbitrary level bytes -------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["bytes", "bytes_max1"])
@pytest.mark.parametrize("path", [OPO, P7], ids=path_id)
def test_arbitrary_bytes(decoder, path, kind):
    """Levels uniform in 0..255, and in 0..max + 1: no writer's sequence, so the automaton says nothing,
    but the kernel's stated definition (rep <= q and def >= DR[q], validity def >= D) is total and the
    levels pqg_take_records hands over are not validated again: equality with the closed form, and
    nothing written outside the outputs."""
    n = 2 * B + 3
    rl, dl, exp = case(pid_of(path), kind, n)
    assert not AR.is_valid_levels(path, rl, dl)
    both_routes(decoder, path, rl, dl, exp)
    dt, rt = upload(decoder, path, rl, dl)
    need = needs(path, exp)
    for cap in (lambda k: need[k], lambda k: n + (path[k] == P)):
        outs = [None if rp == R else (cap(k), 0) for k, rp in enumerate(path)]
        raw_ok(path, raw_assemble(decoder, path, n, dt, rt, outs), exp, outs)
