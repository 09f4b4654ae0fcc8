"""Filters over columns decoded as dictionary ids (host only, no device): an id column that carries its
decoded dictionary compiles to the dictionary's physical type, with the literal cells of that type; INT96
and FIXED_LEN_BYTE_ARRAY dictionaries stay refused at filter creation."""
import pytest

from pqgpu import abi, native
from pqgpu import filter as F


class Dictionary:
    def __init__(self, physical_type):
        self.physical_type = physical_type


class Ids:
    """What Decoder.decode leaves of a COLUMN_DICTIONARY_IDS column, as far as compile looks."""

    def __init__(self, physical_type, dictionary=None):
        self.physical_type = physical_type
        self.flags = abi.COLUMN_DICTIONARY_IDS
        self.dictionary = dictionary


@pytest.mark.parametrize("t,lit", [(abi.INT32, -7), (abi.INT64, 1 << 40), (abi.FLOAT, 1.5), (abi.DOUBLE, -0.0),
                                   (abi.BOOLEAN, True), (abi.BYTE_ARRAY, b"AIR")])
def test_an_id_column_with_a_dictionary_compiles_to_the_dictionarys_type(t, lit):
    cols = [abi.INT32, Ids(t, Dictionary(t))]
    assert F.column_types(cols) == [abi.INT32, t]
    got = F.compile(F.eq(F.col(1), lit), cols)
    want = F.compile(F.eq(F.col(1), lit), [abi.INT32, t])  # the same predicate over a value column
    assert (got.nodes, got.literals, got.literal_bytes, got.column_types) == \
           (want.nodes, want.literals, want.literal_bytes, want.column_types)
    flt = F.Filter(F.not_(F.eq(F.col(1), lit)), cols)
    assert [nd[0] for nd in flt.program()] == [abi.FILTER_NOTEQ] and flt.n_cols == 2
    flt.close()


def test_the_dictionarys_type_is_the_one_that_counts():
    """column_types reads the type off the dictionary the column carries."""
    assert F.column_types([Ids(abi.INT64, Dictionary(abi.BYTE_ARRAY))]) == [abi.BYTE_ARRAY]


def test_without_a_dictionary_an_id_column_is_still_refused():
    with pytest.raises(native.PqgError) as e:
        F.Filter(F.eq(F.col(0), 1), [Ids(abi.INT64)])
    assert e.value.code == abi.ERR_UNSUPPORTED


@pytest.mark.parametrize("t", [abi.INT96, abi.FIXED_LEN_BYTE_ARRAY])
def test_int96_and_flba_dictionaries_are_refused(t):
    with pytest.raises(native.PqgError) as e:
        F.Filter(F.eq(F.col(0), b"\0" * 12), [Ids(t, Dictionary(t))])
    assert e.value.code == abi.ERR_UNSUPPORTED
