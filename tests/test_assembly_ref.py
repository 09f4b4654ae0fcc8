"""The vectorised assembly reference (tests/assembly_ref.py) against the automaton
(oracle/assembly.py, pinned to TestColumnIO.expectedEventsForR1): closed_form() equals
columnar(fsm_events()) on every path of PATHS_DEEP and every generator; the generators produce
sequences a writer produces, and is_valid_levels() rejects ones it does not."""
import numpy as np
import pytest

from oracle import assembly as A

import assembly_ref as AR
from assembly_ref import B, O, P, PATHS_DEEP, path_id
from test_oracle_assembly import PAPER, stripes

SHAPES = list(AR.KINDS) + ["blocks"]


def automaton(path, rl, dl):
    names = [f"n{k}" for k in range(len(path))]
    max_d = A.levels_of(path)[-1][1]
    vals = [0] * int((np.asarray(dl) >= max_d).sum())
    return A.columnar(path, A.fsm_events(path, names, list(map(int, rl)), list(map(int, dl)), vals))


def same(path, got, exp):
    assert got["records"] == exp["records"]
    for k, rp in enumerate(path):
        if rp == O:
            assert got["validity"][k].dtype == np.uint8
            assert got["validity"][k].tolist() == exp["validity"][k], f"validity of node {k}"
            assert got["n_entries"][k] == len(exp["validity"][k])
        if rp == P:
            assert got["offsets"][k].dtype == np.int64
            assert got["offsets"][k].tolist() == exp["offsets"][k], f"offsets of node {k}"
            assert got["n_entries"][k] == exp["offsets"][k][-1]


def shape(kind, path, n, rng):
    max_r = AR.path_levels(path)[0]
    if kind == "one_record" and max_r == 0:
        kind = "pooled"  # a path without a REPEATED node has one slot per record
    if kind != "blocks":
        return AR.make(kind, path, n, rng)
    kinds = ["dense", "all_null", "one_record" if max_r else "pooled", "all_null", "deepest_only"]
    cut = np.sort(rng.integers(0, n + 1, size=len(kinds) - 1))  # segment lengths (some empty at small n)
    lengths = np.diff(np.concatenate([[0], cut, [n]]))
    return AR.blocks_of(kinds, path, rng, lengths)


@pytest.mark.parametrize("path", PATHS_DEEP, ids=path_id)
@pytest.mark.parametrize("kind", SHAPES)
def test_closed_form_equals_the_automaton(path, kind):
    for n in (1, 17, 777, 5000):
        rng = np.random.default_rng(n + len(path))
        rl, dl = shape(kind, path, n, rng)
        assert rl.dtype == np.uint8 and dl.dtype == np.uint8 and rl.size == dl.size == n
        same(path, AR.closed_form(path, rl, dl), automaton(path, rl, dl))


@pytest.mark.parametrize("leaf", list(PAPER))
def test_closed_form_reproduces_the_paper_records(leaf):
    names, path, r1, r2 = PAPER[leaf]
    rl, dl, vals = stripes(r1 + r2)
    assert AR.is_valid_levels(path, rl, dl)
    same(path, AR.closed_form(path, rl, dl), A.columnar(path, A.fsm_events(path, names, rl, dl, vals)))


def test_closed_form_name_language_country():
    """The figures test_oracle_assembly pins by hand."""
    _, path, r1, r2 = PAPER["Name.Language.Country"]
    rl, dl, _ = stripes(r1 + r2)
    c = AR.closed_form(path, rl, dl)
    assert c["records"] == 2 and c["n_entries"] == [4, 3, 3]
    assert c["offsets"][0].tolist() == [0, 3, 4] and c["offsets"][1].tolist() == [0, 2, 2, 3, 3]
    assert c["validity"][2].tolist() == [1, 0, 1]


@pytest.mark.parametrize("path", PATHS_DEEP, ids=path_id)
def test_generators_produce_valid_levels_at_block_seams(path):
    max_r = AR.path_levels(path)[0]
    for n in (B - 1, B, B + 1):
        rng = np.random.default_rng(n)
        for kind in AR.KINDS:
            if kind == "one_record" and max_r == 0:
                continue
            rl, dl = AR.make(kind, path, n, rng)  # (asserts is_valid_levels itself)
            assert rl.size == dl.size == n and AR.is_valid_levels(path, rl, dl)
    for kinds in AR.MIXTURES:
        if max_r == 0 and "one_record" in kinds:
            continue
        rl, dl = AR.blocks_of(kinds, path, np.random.default_rng(3))
        assert rl.size == len(kinds) * B and AR.is_valid_levels(path, rl, dl)


def test_one_record_is_one_record():
    for path in PATHS_DEEP:
        if AR.path_levels(path)[0]:
            rl, dl = AR.one_record(path, 3 * B + 5, np.random.default_rng(1))
            assert AR.closed_form(path, rl, dl)["records"] == 1


def test_broken_sequences_are_rejected():
    path = [O, P, O, P, O]  # DR = [0, 2, 4], max_def 5
    ok = ([0, 1, 2, 2, 0, 0], [5, 4, 4, 5, 0, 1])
    assert AR.is_valid_levels(path, *ok)

    def broken(i, r=None, d=None):
        rl, dl = list(ok[0]), list(ok[1])
        if r is not None:
            rl[i] = r
        if d is not None:
            dl[i] = d
        return AR.is_valid_levels(path, rl, dl)

    assert not broken(0, r=1)            # the first slot continues a list
    assert not broken(2, r=3)            # repetition level above the maximum
    assert not broken(3, d=6)            # definition level above the maximum
    assert not broken(2, d=3)            # r = 2 with d < DR[2]: the list it continues is not defined
    assert not broken(5, r=1, d=2)       # r = 1 after a slot with d = 0 < DR[1]: nothing to continue
    assert broken(1, r=2)                # (r = 2 after d = 5 with d = 4 >= DR[2] is a writer's sequence)
    assert not AR.is_valid_levels(path, [0, 0], [1])
    rl, dl = AR.pooled(path, 500, np.random.default_rng(0))
    rl = rl.copy()
    rl[0] = 1
    assert not AR.is_valid_levels(path, rl, dl)
