"""tests/filter_records_ref.py pinned: the contains() reference the device is compared with.
(b) the value-by-value inspectors equal (c) the array form on random schemas; (b) reproduces the known
answers of TestRecordLevelFilters (tests/golden/filter_contains_phonebook.json); (a) the rewriters'
outcome reproduces TestContainsRewriter and the refusals of LogicalInverter / ContainsRewriter /
Operators.Contains. No device, no native library."""
import json
import os

import numpy as np
import pytest

import filter_records_ref as RR
import filter_ref as R
from pqgpu import abi
from pqgpu import filter as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "filter_contains_phonebook.json")
TYPES = {"INT64": abi.INT64, "BYTE_ARRAY": abi.BYTE_ARRAY, "DOUBLE": abi.DOUBLE}
NAMES = ["number", "kind", "key", "value"]
MK = {"eq": F.eq, "not_eq": F.not_eq, "lt": F.lt, "lt_eq": F.lt_eq, "gt": F.gt, "gt_eq": F.gt_eq, "in": F.in_,
      "not_in": F.not_in}


def phonebook():
    """(columns, ids, cases) of the golden phone book: the four repeated leaves of PhoneBookWriter's schema."""
    doc = json.load(open(GOLDEN))
    number, kind, key, value = [], [], [], []
    for u in doc["users"]:
        ph = u["phones"]
        number.append(None if ph is None else [p[0] for p in ph])
        kind.append(None if ph is None else [None if p[1] is None else p[1].encode() for p in ph])
        ac = u["accounts"]
        key.append(None if ac is None else [k.encode() for k, _ in ac])
        value.append(None if ac is None else [v for _, v in ac])
    spec = doc["columns"]
    cols = [RR.from_lists(TYPES[spec[n]["type"]], lists, max_def=spec[n]["max_def"])
            for n, lists in zip(NAMES, (number, kind, key, value))]
    for n, c in zip(NAMES, cols):
        assert c.max_rep == spec[n]["max_rep"]
    return cols, np.array([u["id"] for u in doc["users"]]), doc["cases"]


def phonebook_predicate(p):
    if p[0] in ("and", "or"):
        return (F.and_ if p[0] == "and" else F.or_)(phonebook_predicate(p[1]), phonebook_predicate(p[2]))
    if p[0] == "contains":
        return F.contains(phonebook_predicate(p[1]))
    c = NAMES.index(p[1])
    enc = (lambda v: v.encode()) if c in (1, 2) else (lambda v: v)
    return MK[p[0]](F.col(c), [enc(v) for v in p[2]] if isinstance(p[2], list) else enc(p[2]))


def test_phonebook_known_answers():
    cols, ids, cases = phonebook()
    assert len(ids) == 107 and len(cases) == 16
    assert {c["test"] for c in cases} == {
        "testArrayContains", "testArrayContainsSimpleAndFilter", "testArrayContainsNestedAndFilter",
        "testArrayContainsSimpleOrFilter", "testArrayContainsNestedOrFilter", "testMapContains"}
    for case in cases:
        pred = phonebook_predicate(case["pred"])
        assert RR.outcome(pred) == (RR.OK, -1)
        got = RR.evaluate_records(pred, cols, len(ids))
        assert ids[got].tolist() == case["ids"], case
        assert np.array_equal(RR.evaluate(pred, cols, len(ids)), got), case


def test_not_eq_is_false_without_a_value():
    """contains(notEq(kind, "cell")) keeps 27, 28, 30 and none of 17-20 (no value in the record)."""
    cols, ids, _ = phonebook()
    for pred in (F.contains(F.not_eq(F.col(1), b"cell")), F.contains(F.not_in(F.col(1), [b"cell"]))):
        got = ids[RR.evaluate_records(pred, cols, len(ids))].tolist()
        assert got == [27, 28, 30]


def random_lists(rng, t, n_rows, max_def):
    lists = []
    for _ in range(n_rows):
        r = rng.random()
        if r < 0.1:
            lists.append(None)
        elif r < 0.2:
            lists.append([])
        else:
            k = int(rng.integers(1, 6))
            lists.append([None if max_def == 3 and rng.random() < 0.2 else R.random_literal(rng, t) for _ in range(k)])
    return lists


def random_flat(rng, t, n_rows):
    valid = rng.random(n_rows) < 0.8
    vals = [R.random_literal(rng, t) for _ in range(int(valid.sum()))]
    if t != abi.BYTE_ARRAY:
        vals = np.asarray(vals, dtype=abi.numpy_dtype(t) if t != abi.BOOLEAN else np.uint8)
    return R.RefColumn(t, vals, valid.astype(np.uint8), max_def=1)


ALL_TYPES = [abi.BOOLEAN, abi.INT32, abi.INT64, abi.FLOAT, abi.DOUBLE, abi.BYTE_ARRAY]


@pytest.mark.parametrize("seed", range(12))
def test_inspectors_equal_arrays_on_random_schemas(seed):
    rng = np.random.default_rng(1000 + seed)
    n_rows = int(rng.integers(1, 60))
    types = [ALL_TYPES[int(rng.integers(0, 6))] for _ in range(4)]
    repeated = [True, True, False, bool(rng.random() < 0.5)]
    cols = []
    for t, rep in zip(types, repeated):
        md = int(rng.integers(2, 4))
        cols.append(RR.from_lists(t, random_lists(rng, t, n_rows, md), max_def=md) if rep else random_flat(rng, t, n_rows))
    if seed % 4 == 0:
        cols[1] = RR.RefListColumn(types[1], missing=True)
    n_ok = 0
    for _ in range(40):
        pred = RR.random_tree(rng, types, repeated, depth=4)
        if RR.outcome(pred)[0] != RR.OK:
            continue
        n_ok += 1
        assert np.array_equal(RR.evaluate_records(pred, cols, n_rows), RR.evaluate(pred, cols, n_rows)), repr(pred)
    assert n_ok >= 10


# ---- (a) the rewriters --------------------------------------------------------------------------------------

def c_(v, col=0):
    return F.contains(F.eq(F.col(col), v))


def shape(p):
    """The merged tree as nested tuples."""
    if isinstance(p, RR.Merged):
        return ("and" if p.op == abi.FILTER_AND else "or", shape(p.left), shape(p.right))
    if p.op == abi.FILTER_CONTAINS:
        return p.children[0].values[0]
    return repr(p)


def test_contains_rewriter_cases():
    """TestContainsRewriter.testBaseCases and testNested."""
    a, d = F.col(0), F.col(1)
    for p in (F.eq(a, 17), F.not_eq(a, 17), F.lt(a, 17), F.lt_eq(a, 17), F.gt(a, 17), F.gt_eq(a, 17),
              F.and_(F.eq(a, 17), F.eq(d, 12.0)), F.or_(F.eq(a, 17), F.eq(d, 12.0)), c_(17)):
        assert RR.contains_rewrite(p) is p
    assert shape(RR.contains_rewrite(F.and_(c_(17), c_(7)))) == ("and", 17, 7)
    assert shape(RR.contains_rewrite(F.or_(c_(17), c_(7)))) == ("or", 17, 7)
    c1, c2, c3, c4 = c_(1), c_(2), c_(3), c_(4)
    assert shape(RR.contains_rewrite(F.and_(c1, F.or_(c2, c3)))) == ("and", 1, ("or", 2, 3))
    assert shape(RR.contains_rewrite(F.or_(F.and_(c1, c2), c3))) == ("or", ("and", 1, 2), 3)
    assert shape(RR.contains_rewrite(F.and_(F.and_(c1, c2), F.or_(c2, c3)))) == ("and", ("and", 1, 2), ("or", 2, 3))
    assert shape(RR.contains_rewrite(F.or_(F.and_(c1, c2), F.or_(c3, c4)))) == ("or", ("and", 1, 2), ("or", 3, 4))


def test_outcome_refusals():
    flat = F.eq(F.col(2), 5)
    # LogicalInverter.visit(Contains): any not() above a contains, however many
    assert RR.outcome(F.not_(c_(1))) == (RR.UNSUPPORTED, 1)
    assert RR.outcome(F.not_(F.not_(c_(1)))) == (RR.UNSUPPORTED, 1)
    assert RR.outcome(F.and_(flat, F.not_(F.or_(flat, c_(1))))) == (RR.UNSUPPORTED, 3)
    # the innermost not() throws first, at the first contains its inversion meets
    assert RR.outcome(F.not_(F.and_(c_(1), F.not_(c_(2))))) == (RR.UNSUPPORTED, 3)
    # ContainsRewriter: left Contains, right not -> refused; the mirror case and a leaf on either side pass
    assert RR.outcome(F.and_(c_(1), F.and_(flat, flat))) == (RR.UNSUPPORTED, 5)
    assert RR.outcome(F.and_(F.and_(flat, flat), c_(1))) == (RR.OK, -1)
    assert RR.outcome(F.or_(flat, c_(1))) == (RR.OK, -1)
    assert RR.outcome(F.or_(c_(1), flat)) == (RR.OK, -1)
    # the early return leaves the other side unexamined: its refusal is never met
    bad = F.and_(c_(1), F.and_(flat, flat))
    assert RR.outcome(F.and_(flat, bad)) == (RR.OK, -1)
    assert RR.outcome(F.and_(bad, flat))[0] == RR.UNSUPPORTED
    # two Contains sides on different columns
    assert RR.outcome(F.and_(c_(1, 0), c_(1, 1))) == (RR.INVALID, 4)
    assert RR.outcome(F.and_(F.and_(flat, c_(1, 0)), c_(1, 1))) == (RR.OK, -1)
    # Operators.Contains: no null element values, a single-column predicate
    assert RR.outcome(F.contains(F.eq(F.col(0), None))) == (RR.INVALID, 1)
    assert RR.outcome(F.contains(F.in_(F.col(0), [1, None]))) == (RR.INVALID, 1)
    assert RR.outcome(F.contains(F.and_(F.eq(F.col(0), 1), F.eq(F.col(0), 2)))) == (RR.INVALID, 3)
