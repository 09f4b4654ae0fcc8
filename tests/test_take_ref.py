"""tests/take_ref.py against itself and a hand-written example (CPU): the row-by-row form and the
vectorised form agree, and a take of a take is the take of the composed mask."""
import numpy as np
import pytest

import filter_ref as R
import take_ref as K
from pqgpu import abi


def random_columns(rng, n):
    cols = []
    for t, md in [(abi.INT32, 0), (abi.DOUBLE, 1), (abi.BOOLEAN, 1), (abi.INT64, 3), (abi.BYTE_ARRAY, 2), (abi.BYTE_ARRAY, 0)]:
        dl = None
        if md:
            dl = np.where(rng.random(n) < 0.3, rng.integers(0, md, size=n), md).astype(np.uint8)
        k = n if dl is None else int((dl == md).sum())
        if t == abi.BYTE_ARRAY:
            vals = [bytes(rng.integers(0, 256, size=int(rng.integers(0, 6)), dtype=np.uint8)) for _ in range(k)]
        elif t == abi.BOOLEAN:
            vals = rng.integers(0, 2, size=k).astype(np.uint8)
        else:
            vals = rng.integers(-1000, 1000, size=k).astype(abi.numpy_dtype(t))
        cols.append(R.RefColumn(t, vals, dl, md))
    cols.append(R.RefColumn(abi.INT32, max_def=1, missing=True))
    return cols


def same(cols, a, b):
    for col, (dla, va), (dlb, vb) in zip(cols, a, b):
        assert (dla is None) == (dlb is None)
        if dla is not None:
            assert dla.dtype == np.uint8 and np.array_equal(dla, dlb)
        assert K.values_equal(col.physical_type, va, vb)


@pytest.mark.parametrize("n,p", [(0, 0.5), (1, 0.5), (200, 0.0), (200, 1.0), (777, 0.3), (777, 0.9)])
def test_the_two_forms_agree(n, p):
    rng = np.random.default_rng(n + int(p * 10))
    cols = random_columns(rng, n)
    keep = rng.random(n) < p
    same(cols, K.take_rows(cols, keep), K.take(cols, keep))


def test_hand_written_example():
    """6 rows, keep mask 010110: rows 1, 3 and 4."""
    req = R.RefColumn(abi.INT32, np.array([10, 11, 12, 13, 14, 15], dtype=np.int32))
    # levels 3 0 3 2 3 1: rows 0, 2 and 4 hold "a", "bb", "" — the kept rows are null, null (level 2), ""
    opt = R.RefColumn(abi.BYTE_ARRAY, [b"a", b"bb", b""], np.array([3, 0, 3, 2, 3, 1], dtype=np.uint8), 3)
    keep = np.array([0, 1, 0, 1, 1, 0], dtype=bool)
    for fn in (K.take_rows, K.take):
        (dl0, v0), (dl1, v1) = fn([req, opt], keep)
        assert dl0 is None and list(v0) == [11, 13, 14]
        assert dl1.tolist() == [0, 2, 3] and [bytes(x) for x in v1] == [b""]
    # row 2's "bb" survives a mask that keeps it, at the dense position its kept predecessors leave
    (_, v0), (dl1, v1) = K.take_rows([req, opt], np.array([0, 0, 1, 0, 1, 1], dtype=bool))
    assert list(v0) == [12, 14, 15] and dl1.tolist() == [3, 3, 1] and [bytes(x) for x in v1] == [b"bb", b""]


def test_take_of_take_is_the_take_of_the_composed_mask():
    rng = np.random.default_rng(5)
    n = 500
    cols = random_columns(rng, n)
    m1 = rng.random(n) < 0.6
    m2 = rng.random(int(m1.sum())) < 0.4
    first = K.take(cols, m1)
    second = K.take(K.as_ref_columns(cols, first), m2)
    m = K.compose(m1, m2)
    assert int(m.sum()) == int(m2.sum())
    same(cols, second, K.take(cols, m))
    same(cols, second, K.take_rows(cols, m))
