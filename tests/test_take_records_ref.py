"""tests/take_records_ref.py against itself, against the oracle's record assembly and against tests/take_ref.py
(CPU): the slot-by-slot form and the vectorised form agree; records rebuilt by the oracle's automaton from
the taken stripes are the kept records of the original list (what RecordReaderImplementation hands back
after FilteringRecordMaterializer dropped the others); on flat columns the outcome is take_ref's."""
import numpy as np
import pytest

import filter_ref as R
import take_records_ref as KR
import take_ref as K
from oracle import assembly as A
from pqgpu import abi
from records import random_record, rebuild, shred

RQ, O, P = A.REQUIRED, A.OPTIONAL, A.REPEATED
N = A.Node

# flat leaves beside lists, two nested REPEATED levels, optional groups around and inside lists
SCHEMA_LISTS = [N("id", RQ), N("tag", O), N("xs", P), N("grid", P, [N("row", P)]),
                N("box", O, [N("items", P, [N("v", O), N("w", RQ)]), N("note", O)])]
SCHEMA_DEEP = [N("a", O, [N("b", P, [N("c", O), N("d", RQ)]), N("e", O)]),
               N("f", P, [N("g", P, [N("h", P)]), N("i", RQ)]), N("j", RQ)]


def stripes_of(roots, recs):
    out = []
    for chain, (rl, dl, vals) in zip(A.schema_leaves(roots), shred(roots, recs)):
        max_d = A.levels_of([n.repetition for n in chain])[-1][1]
        out.append((rl, dl, vals, max_d))
    return out


def random_stripe(rng, n_rec, max_rep, max_def, p_null=0.3):
    """Records of 1..5 slots; repetition values 1..max_rep inside a record are free (they are only copied)."""
    lens = rng.integers(1, 6, size=n_rec)
    rl = rng.integers(1, max_rep + 1, size=int(lens.sum())).astype(np.uint8)
    rl[np.cumsum(lens) - lens] = 0
    dl = np.where(rng.random(rl.size) < p_null, rng.integers(0, max_def, size=rl.size), max_def).astype(np.uint8)
    vals = rng.integers(-1000, 1000, size=int((dl == max_def).sum())).astype(np.int64)
    return rl, dl, vals, max_def


def same(a, b):
    assert len(a) == len(b)
    for (rla, dla, va), (rlb, dlb, vb) in zip(a, b):
        assert rla.dtype == np.uint8 and np.array_equal(rla, rlb)
        assert dla.dtype == np.uint8 and np.array_equal(dla, dlb)
        assert list(va) == list(vb)


@pytest.mark.parametrize("n,p", [(0, 0.5), (1, 1.0), (1, 0.0), (300, 0.0), (300, 1.0), (500, 0.1), (500, 0.9)])
def test_the_two_forms_agree(n, p):
    rng = np.random.default_rng(n + int(p * 10))
    stripes = [random_stripe(rng, n, 1, 2), random_stripe(rng, n, 2, 3), random_stripe(rng, n, 3, 5, 0.6)]
    keep = rng.random(n) < p
    same(KR.take_slots(stripes, keep), KR.take(stripes, keep))


def test_slots_outside_the_mask_are_not_kept():
    """A stripe that begins inside a record (record -1) and one with more records than the mask."""
    rl = np.array([1, 1, 0, 1, 0, 0, 1], dtype=np.uint8)
    dl = np.array([1, 1, 1, 0, 1, 1, 1], dtype=np.uint8)
    vals = np.arange(6, dtype=np.int64)
    for fn in (KR.take_slots, KR.take):
        (orl, odl, ov), = fn([(rl, dl, vals, 1)], [True, True])  # records 0 and 1 of 3; two slots of record -1
        assert orl.tolist() == [0, 1, 0] and odl.tolist() == [1, 0, 1] and list(ov) == [2, 3]


def test_hand_written_example():
    """list<int>: [1, 2], [], null-ish (def 0), [3]; keep records 0 and 3, then 1 and 2."""
    rl = np.array([0, 1, 0, 0, 0], dtype=np.uint8)
    dl = np.array([2, 2, 1, 0, 2], dtype=np.uint8)
    vals = np.array([1, 2, 3], dtype=np.int64)
    for fn in (KR.take_slots, KR.take):
        (orl, odl, ov), = fn([(rl, dl, vals, 2)], [True, False, False, True])
        assert orl.tolist() == [0, 1, 0] and odl.tolist() == [2, 2, 2] and list(ov) == [1, 2, 3]
        (orl, odl, ov), = fn([(rl, dl, vals, 2)], [False, True, True, False])
        assert orl.tolist() == [0, 0] and odl.tolist() == [1, 0] and list(ov) == []


@pytest.mark.parametrize("roots", [SCHEMA_LISTS, SCHEMA_DEEP], ids=["lists", "deep"])
@pytest.mark.parametrize("p", [0.0, 0.3, 1.0])
def test_the_oracle_rebuilds_the_kept_records(roots, p):
    rng = np.random.default_rng(len(roots) + int(p * 10))
    recs = [random_record(roots, rng) for _ in range(250)]
    keep = rng.random(len(recs)) < p
    stripes = stripes_of(roots, recs)
    assert all(KR.n_records(s[0]) == len(recs) for s in stripes)
    assert any(s[0].max() >= 2 for s in stripes)  # at least two nested REPEATED levels
    for fn in (KR.take_slots, KR.take):
        taken = [(rl, dl, list(v)) for rl, dl, v in fn(stripes, keep)]
        ev = A.fsm_events_multi(roots, taken)
        assert rebuild(roots, ev) == [r for r, k in zip(recs, keep) if k]


def test_flat_columns_are_take_ref():
    rng = np.random.default_rng(9)
    n = 400
    keep = rng.random(n) < 0.4
    for md in (0, 1, 3):
        dl = np.where(rng.random(n) < 0.3, rng.integers(0, max(md, 1), size=n), md).astype(np.uint8)
        vals = rng.integers(-1000, 1000, size=int((dl == md).sum())).astype(np.int64)
        (wdl, wv), = K.take([R.RefColumn(abi.INT64, vals, dl if md else None, md)], keep)
        for fn in (KR.take_slots, KR.take):
            (orl, odl, ov), = fn([(np.zeros(n, dtype=np.uint8), dl, vals, md)], keep)
            assert not orl.any() and orl.size == int(keep.sum())
            assert np.array_equal(odl, dl[keep]) and (wdl is None or np.array_equal(odl, wdl))
            assert list(ov) == list(wv)


def test_take_of_take_is_the_take_of_the_composed_mask():
    rng = np.random.default_rng(5)
    n = 300
    stripes = [random_stripe(rng, n, 2, 3), random_stripe(rng, n, 1, 1)]
    m1 = rng.random(n) < 0.6
    m2 = rng.random(int(m1.sum())) < 0.4
    first = KR.take(stripes, m1)
    again = [(rl, dl, v, s[3]) for (rl, dl, v), s in zip(first, stripes)]
    same(KR.take(again, m2), KR.take(stripes, K.compose(m1, m2)))
