"""pqg_filter_create / pqg_filter_program with PQG_FILTER_CONTAINS (host only, no device): a contains node
is accepted and reported as it is, every refusal of Operators.Contains, LogicalInverter and ContainsRewriter
returns its code and node (tests/filter_records_ref.py, outcome) on seeded random trees, the rewriter's
left / right asymmetry and early return are covered explicitly, and pqg_filter_record_column has the layout
the header states."""
import ctypes as C

import numpy as np

import filter_records_ref as RR
import filter_ref as R
from pqgpu import abi, native
from pqgpu import filter as F

TYPES = [abi.INT64, abi.BYTE_ARRAY, abi.INT32, abi.DOUBLE, abi.BOOLEAN]
REPEATED = [True, True, False, False, True]
CODES = {RR.OK: abi.OK, RR.UNSUPPORTED: abi.ERR_UNSUPPORTED, RR.INVALID: abi.ERR_INVALID_ARG}


def created(pred, types=TYPES):
    """(rc, node the status names, program or None)."""
    c = F.compile(pred, types)
    rc, h, st = F.create(c.nodes, c.literals, c.literal_bytes, c.column_types)
    if rc != abi.OK:
        assert not h.value and st.code == rc
        return rc, st.value_index, None
    try:
        return rc, st.value_index, F.program(h)
    finally:
        native.lib().pqg_filter_destroy(h)


def shape(prog):
    return [(op, column, left, right, flags, n) for (op, column, left, right, flags, _, n) in prog]


def c_(v, col=0):
    return F.contains(F.eq(F.col(col), v))


def test_contains_is_accepted_and_reported():
    assert abi.FILTER_CONTAINS == 11
    rc, _, prog = created(c_(7))
    assert rc == abi.OK
    assert shape(prog) == [(abi.FILTER_EQ, 0, -1, -1, 0, 1), (abi.FILTER_CONTAINS, -1, 0, -1, 0, 0)]
    p = F.or_(F.not_(F.lt(F.col(2), 5)), F.and_(c_(7), F.contains(F.in_(F.col(0), [1, 2, 3]))))
    rc, _, prog = created(p)
    assert rc == abi.OK
    assert shape(prog) == R.flatten(RR.li_rewrite(p))
    assert [nd[0] for nd in prog].count(abi.FILTER_CONTAINS) == 2
    assert repr(c_(7)) == "contains(eq(col0, 7))"


def test_contains_counts_against_the_node_limit():
    p = c_(0)
    for i in range(1, 22):  # 22 contains + 22 leaves + 21 ands = 65 nodes
        p = F.and_(p, c_(i))
    assert created(p)[0] == abi.ERR_UNSUPPORTED
    q = c_(0)
    for i in range(1, 21):  # 62 nodes
        q = F.and_(q, c_(i))
    rc, _, prog = created(q)
    assert rc == abi.OK and len(prog) == 62


def test_malformed_contains_nodes():
    leaf = (abi.FILTER_EQ, 0, -1, -1, 0, 0, 1)
    other = (abi.FILTER_EQ, 0, -1, -1, 0, 1, 1)
    cont = (abi.FILTER_CONTAINS, -1, 0, -1, 0, 0, 0)

    def rc_node(nodes, literals=(5, 6)):
        rc, h, st = F.create(list(nodes), list(literals), b"", TYPES)
        if rc == abi.OK:
            native.lib().pqg_filter_destroy(h)
        return rc, st.value_index

    assert rc_node([leaf, cont]) == (abi.OK, -1)
    assert rc_node([cont]) == (abi.ERR_INVALID_ARG, 0)                                      # childless
    assert rc_node([leaf, other, (abi.FILTER_CONTAINS, -1, 0, 1, 0, 0, 0)]) == (abi.ERR_INVALID_ARG, 2)  # right != -1
    assert rc_node([leaf, (abi.FILTER_CONTAINS, -1, 0, -1, abi.FILTER_UNSIGNED, 0, 0)]) == (abi.ERR_INVALID_ARG, 1)
    assert rc_node([leaf, (abi.FILTER_CONTAINS, -1, 0, -1, 0, 0, 1)]) == (abi.ERR_INVALID_ARG, 1)      # literals
    assert rc_node([leaf, other, (abi.FILTER_AND, -1, 0, 1, 0, 0, 0),
                    (abi.FILTER_CONTAINS, -1, 2, -1, 0, 0, 0)]) == (abi.ERR_INVALID_ARG, 3)            # child not a leaf
    assert rc_node([leaf, cont, (abi.FILTER_CONTAINS, -1, 1, -1, 0, 0, 0)]) == (abi.ERR_INVALID_ARG, 2)
    null_leaf = (abi.FILTER_EQ, 0, -1, -1, abi.FILTER_NULL_LITERAL, 0, 0)
    assert rc_node([null_leaf, cont]) == (abi.ERR_INVALID_ARG, 1)
    null_set = (abi.FILTER_IN, 0, -1, -1, abi.FILTER_NULL_LITERAL, 0, 1)
    assert rc_node([null_set, cont]) == (abi.ERR_INVALID_ARG, 1)
    # lt on BOOLEAN under a contains: refused at the leaf, as without one
    assert rc_node([(abi.FILTER_LT, 4, -1, -1, 0, 0, 1), cont]) == (abi.ERR_INVALID_ARG, 0)
    assert rc_node([leaf, (12, -1, 0, -1, 0, 0, 0)]) == (abi.ERR_INVALID_ARG, 1)            # op past CONTAINS


def test_not_above_contains():
    flat = lambda: F.eq(F.col(2), 5)  # noqa: E731
    for p in (F.not_(c_(1)), F.not_(F.not_(c_(1))), F.and_(flat(), F.not_(F.or_(flat(), c_(1)))),
              F.not_(F.and_(c_(1), F.not_(c_(2)))), F.or_(F.not_(F.and_(flat(), c_(1))), F.not_(c_(2)))):
        code, node = RR.outcome(p)
        assert code == RR.UNSUPPORTED
        assert created(p)[:2] == (abi.ERR_UNSUPPORTED, node), repr(p)
    assert created(F.not_(F.and_(c_(1), F.not_(c_(2)))))[1] == 3  # the innermost not() throws first


def test_contains_rewriter_asymmetry_and_early_return():
    flat = lambda: F.eq(F.col(2), 5)  # noqa: E731
    two = lambda: F.and_(flat(), flat())  # noqa: E731
    # a Contains on the left needs one on the right ...
    assert created(F.and_(c_(1), two()))[:2] == (abi.ERR_UNSUPPORTED, 5)
    assert created(F.or_(c_(1), two()))[:2] == (abi.ERR_UNSUPPORTED, 5)
    assert created(F.or_(F.and_(c_(1), c_(2)), two()))[:2] == (abi.ERR_UNSUPPORTED, 8)
    # ... the mirror case is accepted, and so is a plain leaf on either side
    for p in (F.and_(two(), c_(1)), F.or_(two(), F.and_(c_(1), c_(2))), F.or_(flat(), c_(1)), F.or_(c_(1), flat()),
              F.and_(F.and_(flat(), c_(1, 0)), c_(1, 1))):
        assert RR.outcome(p) == (RR.OK, -1)
        rc, _, prog = created(p)
        assert rc == abi.OK and shape(prog) == R.flatten(p), repr(p)
    # the early return: a plain leaf on the left leaves the right side unexamined, refusals included
    bad = lambda: F.and_(c_(1), two())  # noqa: E731
    assert created(F.and_(flat(), bad()))[0] == abi.OK
    assert created(F.and_(bad(), flat()))[:2] == (abi.ERR_UNSUPPORTED, 5)
    mixed = lambda: F.and_(c_(1, 0), c_(1, 1))  # noqa: E731
    assert created(F.or_(flat(), mixed()))[0] == abi.OK
    # two Contains sides on different columns
    assert created(mixed())[:2] == (abi.ERR_INVALID_ARG, 4)
    assert created(F.or_(c_(1, 0), F.or_(c_(2, 0), c_(3, 1))))[:2] == (abi.ERR_INVALID_ARG, 6)
    assert created(F.or_(F.and_(c_(1, 0), c_(2, 0)), c_(3, 1)))[:2] == (abi.ERR_INVALID_ARG, 7)
    # after the inversion the same rules hold: not(or(flat, flat)) is an and of two leaves
    assert created(F.and_(c_(1), F.not_(F.or_(flat(), flat()))))[:2] == (abi.ERR_UNSUPPORTED, 6)


def test_random_trees_against_the_reference():
    rng = np.random.default_rng(29)
    seen = {RR.OK: 0, RR.UNSUPPORTED: 0, RR.INVALID: 0}
    for i in range(400):
        p = RR.random_tree(rng, TYPES, REPEATED, depth=int(rng.integers(2, 6)), p_not=0.08, p_bad=0.03)
        code, node = RR.outcome(p)
        seen[code] += 1
        rc, got_node, prog = created(p)
        assert rc == CODES[code], (i, repr(p))
        if code == RR.OK:
            assert shape(prog) == R.flatten(RR.li_rewrite(p)), repr(p)
        else:
            assert got_node == node, (i, repr(p))
    assert min(seen.values()) >= 20, seen


def test_record_column_layout():
    T = abi.FilterRecordColumn
    assert C.sizeof(T) == 64
    assert (T.col.offset, T.max_rep.offset, T.reserved.offset, T.rep_levels.offset, T.n_slots.offset) == (0, 40, 44, 48, 56)
    assert C.sizeof(abi.FilterColumn) == 40
    assert "pqg_filter_run_records" in native.EXPORTS and hasattr(native.lib(), "pqg_filter_run_records")
