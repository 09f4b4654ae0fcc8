"""Reference semantics of parquet-mr's contains() record filter, restated in Python / numpy.
Test infrastructure only (the product is csrc/pqgpu_filter*.{cpp,hip}); flat leaves come from
tests/filter_ref.py.

What is restated (paths under parquet-column/src/main/java/org/apache/parquet/ unless noted):
  outcome            what FilterCompat.get (filter2/compat/FilterCompat.java:80-91) does with a predicate
                     that holds contains(): FilterApi.contains / Operators.Contains (Operators.java:326-462),
                     LogicalInverseRewriter with LogicalInverter.java:97-99, then ContainsRewriter.java:100-168
                     with its left / right asymmetry and early returns -> OK, UNSUPPORTED or INVALID and the
                     offending node (post-order index, as pqgpu.filter.compile numbers the nodes)
  evaluate_records   value by value with explicit inspector state (isKnown, setResult only when unknown,
                     updateNull at record end): the expectMultipleResults inspectors and ContainsPredicate /
                     ContainsAndPredicate / ContainsOrPredicate of parquet-generator/.../
                     IncrementallyUpdatedFilterPredicateGenerator.java:198-327, 339-537, on the tree
                     ContainsRewriter merged; flat leaves through filter_ref.leaf_row
  evaluate           the same over numpy arrays, with and / or kept as they are above every contains

notIn: the generated loop (:312-320) accepts a value that differs from any one member of the set; the flat
filter reads notIn as "not a member", and contains(notIn) uses that reading here as on the device."""
import numpy as np

from pqgpu import abi
from pqgpu import filter as F

import filter_ref as R

OK, UNSUPPORTED, INVALID = "OK", "UNSUPPORTED", "INVALID"
_LOGICAL = (abi.FILTER_AND, abi.FILTER_OR)


def is_leaf(p):
    return p.op <= abi.FILTER_NOTIN


class Refused(Exception):
    def __init__(self, code, node):
        super().__init__(code)
        self.code = code
        self.node = node  # the original predicate object


# ---- outcome ---------------------------------------------------------------------------------------------

def post_order(pred):
    """id(node) -> index, numbering left, right, node (pqgpu.filter.compile)."""
    index, n = {}, [0]

    def walk(p):
        for k in p.children:
            walk(k)
        index[id(p)] = n[0]  # an object used twice keeps its last place
        n[0] += 1

    walk(pred)
    return index


def _origin(p):
    return getattr(p, "_origin", p)


def _made(new, old):
    new._origin = _origin(old)
    return new


def li_invert(p):
    """LogicalInverter.invert with visit(Contains): UnsupportedOperationException."""
    if p.op == abi.FILTER_CONTAINS:
        raise Refused(UNSUPPORTED, _origin(p))
    if p.op == abi.FILTER_AND:
        left = li_invert(p.children[0])
        return _made(F.or_(left, li_invert(p.children[1])), p)
    if p.op == abi.FILTER_OR:
        left = li_invert(p.children[0])
        return _made(F.and_(left, li_invert(p.children[1])), p)
    if p.op == abi.FILTER_NOT:
        return p.children[0]
    return _made(F.Predicate(R.INVERSE[p.op], p.column, p.values), p)


def li_rewrite(p):
    """LogicalInverseRewriter.rewrite; a contains is returned as it is."""
    if p.op in _LOGICAL:
        left = li_rewrite(p.children[0])
        right = li_rewrite(p.children[1])
        return _made(F.Predicate(p.op, children=(left, right)), p)
    if p.op == abi.FILTER_NOT:
        return li_invert(li_rewrite(p.children[0]))
    return p


class Merged:
    """ContainsComposedPredicate: and / or of two Contains on one column."""

    def __init__(self, op, left, right):
        lc, rc = contains_column(left), contains_column(right)
        if lc != rc:
            raise ValueError("Composed Contains predicates must reference the same column name")
        self.op, self.left, self.right, self.column = op, left, right, lc


def is_contains(p):
    return isinstance(p, Merged) or p.op == abi.FILTER_CONTAINS


def contains_column(p):
    return p.column if isinstance(p, Merged) else p.children[0].column.index


def cr_visit(p):
    """ContainsRewriter.visit(And) / visit(Or): returns a Merged, or the node as it is. The rewritten children
    of a node that stays are dropped, as in the reference (`return and`)."""
    sides = []
    for k in p.children:
        if k.op in _LOGICAL:
            sides.append(cr_visit(k))
        elif k.op == abi.FILTER_CONTAINS:
            sides.append(k)
        else:
            return p
    left, right = sides
    if is_contains(left):
        if not is_contains(right):
            raise Refused(UNSUPPORTED, _origin(p))
        try:
            return Merged(p.op, left, right)
        except ValueError:
            raise Refused(INVALID, _origin(p))
    return p


def contains_rewrite(p):
    """ContainsRewriter.rewrite of a NOT-free predicate."""
    return cr_visit(p) if p.op in _LOGICAL else p


def compat(pred):
    """FilterCompat.get: the predicate the record filter runs, or Refused. FilterApi.contains' own checks
    come first (the predicate could not have been built): first offender in post-order."""
    def build(p):
        for k in p.children:
            build(k)
        if p.op == abi.FILTER_CONTAINS:
            k = p.children[0]
            if not is_leaf(k) or any(v is None for v in k.values):
                raise Refused(INVALID, p)

    build(pred)
    return contains_rewrite(li_rewrite(pred))


def outcome(pred):
    """(OK, -1), or (UNSUPPORTED | INVALID, post-order index of the offending node)."""
    try:
        compat(pred)
    except Refused as e:
        return e.code, post_order(pred)[id(e.node)]
    return OK, -1


# ---- columns ---------------------------------------------------------------------------------------------

class RefListColumn:
    """A decoded repeated leaf: one repetition and one definition byte per slot, dense values for the slots
    with def == max_def. Record i runs from the i-th slot with rep == 0 to the next. missing=True: a column
    no value reaches."""

    def __init__(self, physical_type, values=(), def_levels=(), rep_levels=(), max_def=1, max_rep=1, missing=False):
        self.physical_type = physical_type
        self.values = values
        self.def_levels = np.asarray(def_levels, dtype=np.uint8)
        self.rep_levels = np.asarray(rep_levels, dtype=np.uint8)
        self.max_def, self.max_rep, self.missing = max_def, max_rep, missing

    def record_values(self, n_rows):
        """Per record: the list of its values (the slots with def == max_def), in order."""
        out = [[] for _ in range(n_rows)]
        if self.missing:
            return out
        r, k = -1, 0
        for rep, d in zip(self.rep_levels, self.def_levels):
            if rep == 0:
                r += 1
            if d == self.max_def:
                out[r].append(self.values[k])
                k += 1
        assert r == n_rows - 1, (r, n_rows)
        return out


def from_lists(physical_type, lists, max_def=2):
    """A RefListColumn of an optional list of required elements (max_def 2: 0 null list, 1 empty list), or
    with max_def 3 of optional elements (None inside a list: def 2). lists[i]: None, [] or a list."""
    vals, dl, rl = [], [], []
    for lst in lists:
        if lst is None or len(lst) == 0:
            dl.append(0 if lst is None else 1)
            rl.append(0)
            continue
        for j, v in enumerate(lst):
            rl.append(0 if j == 0 else 1)
            if v is None:
                assert max_def >= 3
                dl.append(max_def - 1)
            else:
                dl.append(max_def)
                vals.append(v)
    if physical_type != abi.BYTE_ARRAY:
        vals = np.asarray(vals, dtype=abi.numpy_dtype(physical_type) if physical_type != abi.BOOLEAN else np.uint8)
    return RefListColumn(physical_type, vals, dl, rl, max_def=max_def, max_rep=1)


# ---- inspectors, value by value ----------------------------------------------------------------------------

class Inspector:
    def __init__(self):
        self.known = self.result = False

    def set_result(self, r):
        assert not self.known, "setResult() called on a ValueInspector whose result is already known"
        self.known, self.result = True, r

    def reset(self):
        self.known = self.result = False


class LeafInspector(Inspector):
    """The expectMultipleResults form: update() sets true once, and only while unknown."""

    def __init__(self, leaf, physical_type):
        super().__init__()
        self.leaf, self.type = leaf, physical_type

    def update(self, value):
        if not self.known and R.leaf_row(self.leaf, self.type, value):
            self.set_result(True)


class ComposedInspector(Inspector):
    """ContainsAndPredicate / ContainsOrPredicate."""

    def __init__(self, op, left, right):
        super().__init__()
        self.op, self.left, self.right = op, left, right

    def update(self, value):
        self.left.update(value)
        self.right.update(value)
        if self.known:
            return
        lt = self.left.known and self.left.result
        rt = self.right.known and self.right.result
        if (lt and rt) if self.op == abi.FILTER_AND else (lt or rt):
            self.set_result(True)

    def reset(self):
        super().reset()
        self.left.reset()
        self.right.reset()


class ContainsInspector(Inspector):
    """ContainsPredicate around the inspector ContainsInspectorVisitor built."""

    def __init__(self, inner):
        super().__init__()
        self.inner = inner

    def update(self, value):
        self.inner.update(value)
        if not self.known and self.inner.known and self.inner.result:
            self.set_result(True)

    def update_null(self):
        self.set_result(False)

    def reset(self):
        super().reset()
        self.inner.reset()


def _inner(p, columns):
    if isinstance(p, Merged):
        return ComposedInspector(p.op, _inner(p.left, columns), _inner(p.right, columns))
    leaf = p.children[0]
    return LeafInspector(leaf, columns[leaf.column.index].physical_type)


def evaluate_records(pred, columns, n_rows):
    """compat(pred) on every record -> bool array. columns[c]: RefListColumn or filter_ref.RefColumn."""
    tree = compat(pred)
    lists, rows, inspectors = {}, {}, {}

    def ev(p, r):
        if is_contains(p):
            c = contains_column(p)
            if c not in lists:
                lists[c] = columns[c].record_values(n_rows)
            insp = inspectors.setdefault(id(p), ContainsInspector(_inner(p, columns)))
            insp.reset()
            for v in lists[c][r]:
                insp.update(v)
            if not insp.known:  # the end of the record: every inspector still unknown gets updateNull()
                insp.update_null()
            return insp.result
        if p.op == abi.FILTER_AND:
            return ev(p.children[0], r) and ev(p.children[1], r)
        if p.op == abi.FILTER_OR:
            return ev(p.children[0], r) or ev(p.children[1], r)
        c = p.column.index
        if c not in rows:
            rows[c] = columns[c].row_values(n_rows)
        return R.leaf_row(p, columns[c].physical_type, rows[c][r])

    return np.array([ev(tree, r) for r in range(n_rows)], dtype=bool)


# ---- the same over arrays ---------------------------------------------------------------------------------

def contains_array(leaf, col, n_rows):
    """contains(leaf) per record: some slot with a value satisfies the leaf."""
    out = np.zeros(n_rows, dtype=bool)
    if col.missing or len(col.rep_levels) == 0:
        return out
    rec = np.cumsum(col.rep_levels == 0) - 1
    has = col.def_levels == col.max_def
    n = int(has.sum())
    dense = R._leaf_array(leaf, R.RefColumn(col.physical_type, col.values, max_def=0), n)
    hit_rec = rec[has][dense]
    out[hit_rec[(hit_rec >= 0) & (hit_rec < n_rows)]] = True
    return out


def evaluate(pred, columns, n_rows):
    """evaluate_records over arrays: plain and / or above every contains (no ContainsRewriter merge)."""
    def ev(p):
        if p.op == abi.FILTER_AND:
            return ev(p.children[0]) & ev(p.children[1])
        if p.op == abi.FILTER_OR:
            return ev(p.children[0]) | ev(p.children[1])
        if p.op == abi.FILTER_CONTAINS:
            leaf = p.children[0]
            return contains_array(leaf, columns[leaf.column.index], n_rows)
        return R._leaf_array(p, columns[p.column.index], n_rows)

    return ev(li_rewrite(pred))


# ---- seeded random predicates -----------------------------------------------------------------------------

def random_leaf(rng, c, t, null_ok=False):
    column = F.col(c, unsigned=bool(t in (abi.INT32, abi.INT64) and rng.random() < 0.3))
    ops = [F.eq, F.not_eq, F.in_, F.not_in] + ([] if t == abi.BOOLEAN else [F.lt, F.lt_eq, F.gt, F.gt_eq])
    mk = ops[int(rng.integers(0, len(ops)))]
    if mk in (F.in_, F.not_in):
        vals = [R.random_literal(rng, t) for _ in range(int(rng.integers(1, 12)))]
        if null_ok and rng.random() < 0.15:
            vals.append(None)
        return mk(column, vals)
    if null_ok and mk in (F.eq, F.not_eq) and rng.random() < 0.15:
        return mk(column, None)
    return mk(column, R.random_literal(rng, t))


def random_tree(rng, types, repeated, depth, p_not=0.12, p_bad=0.0):
    """A random tree over flat columns (plain leaves) and repeated columns (contains), with not() anywhere.
    p_bad: the chance that a contains gets a null literal or a non-leaf child."""
    r = rng.random()
    if depth > 1 and r < 0.65:
        if r < p_not:
            return F.not_(random_tree(rng, types, repeated, depth - 1, p_not, p_bad))
        mk = F.and_ if rng.random() < 0.5 else F.or_
        return mk(random_tree(rng, types, repeated, depth - 1, p_not, p_bad),
                  random_tree(rng, types, repeated, depth - 1, p_not, p_bad))
    c = int(rng.integers(0, len(types)))
    if not repeated[c]:
        return random_leaf(rng, c, types[c], null_ok=True)
    if rng.random() < p_bad:
        if rng.random() < 0.5:
            return F.contains(F.eq(F.col(c), None))
        return F.contains(F.and_(random_leaf(rng, c, types[c]), random_leaf(rng, c, types[c])))
    return F.contains(random_leaf(rng, c, types[c]))
