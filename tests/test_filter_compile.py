"""pqg_filter_create / pqg_filter_program (host only, no device): the rewritten, NOT-free program
equals tests/filter_ref.py's LogicalInverseRewriter on parquet-mr's known answers and on seeded random
trees, and malformed or out-of-scope tables are rejected with their exact codes."""
import numpy as np
import pytest

import filter_ref as R
from pqgpu import abi, native
from pqgpu import filter as F
from test_filter_ref import rewriter_complex

TYPES = [abi.INT32, abi.DOUBLE, abi.BOOLEAN, abi.INT64, abi.FLOAT, abi.BYTE_ARRAY]


def program_shape(pred, types):
    flt = F.Filter(pred, types)
    try:
        prog = flt.program()
    finally:
        flt.close()
    return [(op, column, left, right, flags, n) for (op, column, left, right, flags, _, n) in prog], prog


def test_known_answers():
    INT, DBL = F.col(0), F.col(1)
    cases = [F.eq(INT, 17), F.not_(F.eq(INT, 17)), F.not_(F.not_eq(INT, 17)), F.not_(F.lt(INT, 17)),
             F.not_(F.lt_eq(INT, 17)), F.not_(F.gt(INT, 17)), F.not_(F.gt_eq(INT, 17)), F.not_(F.in_(INT, [1, 2])),
             F.not_(F.not_(F.eq(INT, 17))), F.not_(F.and_(F.eq(INT, 17), F.eq(DBL, 12.0))),
             F.and_(F.not_(F.gt_eq(INT, 17)), F.lt(INT, 7)), rewriter_complex()[0]]
    for p in cases:
        got, _ = program_shape(p, TYPES)
        assert got == R.flatten(R.rewrite(p)), repr(p)
        assert all(nd[0] != abi.FILTER_NOT for nd in got)
    got, _ = program_shape(rewriter_complex()[0], TYPES)
    assert got == R.flatten(rewriter_complex()[1])  # complexCollapsed


def test_random_trees():
    rng = np.random.default_rng(11)
    for _ in range(200):
        p = R.random_predicate(rng, TYPES, 5)
        got, prog = program_shape(p, TYPES)
        assert got == R.flatten(R.rewrite(p)), repr(p)
        # every leaf owns a literal range of its own, inside the table
        end = 0
        for (op, _, _, _, _, begin, n) in prog:
            if op <= abi.FILTER_NOTIN:
                assert begin == end
                end = begin + n


def test_null_set_members_are_dropped():
    got, _ = program_shape(F.in_(F.col(0), [1, None, 3]), TYPES)
    assert got == [(abi.FILTER_IN, 0, -1, -1, abi.FILTER_NULL_LITERAL, 0)]


def rc_of(nodes, literals=(), blob=b"", types=TYPES, **kw):
    rc, h, st = F.create(list(nodes), list(literals), blob, list(types), **kw)
    if rc == abi.OK:
        native.lib().pqg_filter_destroy(h)
    else:
        assert not h.value
        assert st.code == rc
    return rc


def leaf(op, column, begin=0, n=1, flags=0):
    return (op, column, -1, -1, flags, begin, n)


def test_rejections():
    eq0 = leaf(abi.FILTER_EQ, 0)
    assert rc_of([eq0], [17]) == abi.OK
    # BOOLEAN inequalities: IllegalArgumentException in the reference
    for op in (abi.FILTER_LT, abi.FILTER_LTEQ, abi.FILTER_GT, abi.FILTER_GTEQ):
        assert rc_of([leaf(op, 2)], [1]) == abi.ERR_INVALID_ARG
    assert rc_of([leaf(abi.FILTER_EQ, 2)], [1]) == abi.OK
    # forward and self child indices
    assert rc_of([eq0, (abi.FILTER_AND, -1, 0, 2, 0, 0, 0), eq0], [17]) == abi.ERR_INVALID_ARG
    assert rc_of([eq0, (abi.FILTER_NOT, -1, 1, -1, 0, 0, 0)], [17]) == abi.ERR_INVALID_ARG
    assert rc_of([eq0, (abi.FILTER_AND, -1, 0, 0, 0, 0, 0)], [17]) == abi.ERR_INVALID_ARG
    assert rc_of([eq0, (abi.FILTER_NOT, -1, -1, -1, 0, 0, 0)], [17]) == abi.ERR_INVALID_ARG
    # two roots
    assert rc_of([eq0, eq0], [17]) == abi.ERR_INVALID_ARG
    assert rc_of([eq0, eq0, eq0, (abi.FILTER_AND, -1, 0, 1, 0, 0, 0)], [17]) == abi.ERR_INVALID_ARG
    # a node with two parents
    assert rc_of([eq0, (abi.FILTER_NOT, -1, 0, -1, 0, 0, 0), (abi.FILTER_AND, -1, 0, 1, 0, 0, 0)], [17]) == abi.ERR_INVALID_ARG
    # column out of range
    assert rc_of([leaf(abi.FILTER_EQ, len(TYPES))], [17]) == abi.ERR_INVALID_ARG
    assert rc_of([leaf(abi.FILTER_EQ, -1)], [17]) == abi.ERR_INVALID_ARG
    # literal range past the table
    assert rc_of([leaf(abi.FILTER_EQ, 0, begin=1)], [17]) == abi.ERR_INVALID_ARG
    assert rc_of([leaf(abi.FILTER_IN, 0, begin=0, n=3)], [1, 2]) == abi.ERR_INVALID_ARG
    assert rc_of([leaf(abi.FILTER_IN, 0, begin=0xFFFFFFFF, n=2)], [1, 2]) == abi.ERR_INVALID_ARG
    # byte-array cell past the blob
    assert rc_of([leaf(abi.FILTER_EQ, 5)], [0 | (3 << 32)], b"abc") == abi.OK
    assert rc_of([leaf(abi.FILTER_EQ, 5)], [1 | (3 << 32)], b"abc") == abi.ERR_INVALID_ARG
    assert rc_of([leaf(abi.FILTER_EQ, 5)], [0xFFFFFFFF | (0xFFFFFFFF << 32)], b"abc") == abi.ERR_INVALID_ARG
    # wrong literal counts, null against an inequality, unknown op / flags, unsigned on a double
    assert rc_of([leaf(abi.FILTER_EQ, 0, n=2)], [1, 2]) == abi.ERR_INVALID_ARG
    assert rc_of([leaf(abi.FILTER_IN, 0, n=0)], [1]) == abi.ERR_INVALID_ARG
    assert rc_of([leaf(abi.FILTER_LT, 0, n=0, flags=abi.FILTER_NULL_LITERAL)], [1]) == abi.ERR_INVALID_ARG
    assert rc_of([leaf(abi.FILTER_EQ, 0, n=0, flags=abi.FILTER_NULL_LITERAL)], []) == abi.OK
    assert rc_of([leaf(11, 0)], [1]) == abi.ERR_INVALID_ARG
    assert rc_of([leaf(abi.FILTER_EQ, 0, flags=4)], [1]) == abi.ERR_INVALID_ARG
    assert rc_of([leaf(abi.FILTER_EQ, 1, flags=abi.FILTER_UNSIGNED)], [1]) == abi.ERR_INVALID_ARG
    assert rc_of([], []) == abi.ERR_INVALID_ARG
    # out of scope: INT96 / FIXED_LEN_BYTE_ARRAY columns
    for t in (abi.INT96, abi.FIXED_LEN_BYTE_ARRAY):
        assert rc_of([leaf(abi.FILTER_EQ, 0)], [1], types=[t]) == abi.ERR_UNSUPPORTED
    assert rc_of([leaf(abi.FILTER_EQ, 0)], [1], types=[8]) == abi.ERR_INVALID_ARG


def chain(n_leaves, nots=0):
    """n_leaves eq leaves joined by and nodes (2 n_leaves - 1 nodes), then `nots` not nodes on top."""
    nodes = [leaf(abi.FILTER_EQ, 0)]
    for _ in range(n_leaves - 1):
        nodes.append(leaf(abi.FILTER_EQ, 0))
        nodes.append((abi.FILTER_AND, -1, len(nodes) - 2, len(nodes) - 1, 0, 0, 0))
    for _ in range(nots):
        nodes.append((abi.FILTER_NOT, -1, len(nodes) - 1, -1, 0, 0, 0))
    return nodes


def test_limits():
    assert len(chain(32)) == 63 and rc_of(chain(32), [17]) == abi.OK
    assert len(chain(33)) == 65 and rc_of(chain(33), [17]) == abi.ERR_UNSUPPORTED  # 65 nodes after the rewrite
    assert rc_of(chain(32, nots=40), [17]) == abi.OK  # 103 nodes before it, 63 after
    nodes = chain(32)
    nodes.append(leaf(abi.FILTER_EQ, 0))
    nodes.append((abi.FILTER_OR, -1, len(nodes) - 2, len(nodes) - 1, 0, 0, 0))
    assert len(nodes) == 65 and rc_of(nodes, [17]) == abi.ERR_UNSUPPORTED
    # literal cells and literal bytes
    assert rc_of([leaf(abi.FILTER_IN, 0, n=4096)], list(range(4096))) == abi.OK
    assert rc_of([leaf(abi.FILTER_IN, 0, n=4096)], list(range(4097))) == abi.ERR_UNSUPPORTED
    assert rc_of([leaf(abi.FILTER_EQ, 5)], [0 | (16384 << 32)], bytes(16384)) == abi.OK
    assert rc_of([leaf(abi.FILTER_EQ, 5)], [0], bytes(16385)) == abi.ERR_UNSUPPORTED
    # leaves that share one literal range each get their own copy: 4,097 cells after the rewrite
    two = [leaf(abi.FILTER_IN, 0, n=4096), leaf(abi.FILTER_EQ, 0), (abi.FILTER_AND, -1, 0, 1, 0, 0, 0)]
    assert rc_of(two, list(range(4096))) == abi.ERR_UNSUPPORTED


def test_dictionary_id_columns_are_refused():
    class Ids:
        physical_type = abi.INT64
        flags = abi.COLUMN_DICTIONARY_IDS
    with pytest.raises(native.PqgError) as e:
        F.Filter(F.eq(F.col(0), 1), [Ids()])
    assert e.value.code == abi.ERR_UNSUPPORTED
