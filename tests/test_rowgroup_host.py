"""pqg_chunk_has_non_dictionary_pages (csrc/pqgpu_rowgroup_host.cpp, host only) through framing.has_non_dictionary_pages:
DictionaryFilter.hasNonDictionaryPages over a chunk's encoding_stats and encodings list, case by case and against
tests/rowgroup_filter_ref.py over every small combination. No GPU."""
import itertools

import rowgroup_filter_ref as G
from pqgpu import abi, framing

D, V2, DICT, INDEX = abi.DATA_PAGE, abi.DATA_PAGE_V2, abi.DICTIONARY_PAGE, abi.INDEX_PAGE
PD, RD, PLAIN, RLE, BP = abi.PLAIN_DICTIONARY, abi.RLE_DICTIONARY, abi.PLAIN, abi.RLE, abi.BIT_PACKED


def test_stats_present():
    assert framing.has_non_dictionary_pages([(DICT, PLAIN, 1), (D, RD, 4)], [PLAIN, RD, RLE]) is False
    assert framing.has_non_dictionary_pages([(DICT, PD, 1), (V2, PD, 4)], []) is False
    assert framing.has_non_dictionary_pages([(DICT, PLAIN, 1), (D, RD, 4), (D, PLAIN, 2)], []) is True
    assert framing.has_non_dictionary_pages([(D, PLAIN, 2)], [PD, RLE, BP]) is True  # the stats win over the list
    assert framing.has_non_dictionary_pages([(D, abi.DELTA_BINARY_PACKED, 1)], []) is True


def test_count_zero_entry_still_counts():
    assert framing.has_non_dictionary_pages([(D, RD, 4), (V2, PLAIN, 0)], []) is True
    assert framing.has_non_dictionary_pages([(D, RD, 0)], []) is False


def test_both_dictionary_encodings_listed():
    # RLE_DICTIONARY is removed first and PLAIN_DICTIONARY only when it was absent: one stays behind
    assert framing.has_non_dictionary_pages([(D, RD, 1), (D, PD, 1)], []) is True
    assert framing.has_non_dictionary_pages([(V2, PD, 1), (D, RD, 1)], []) is True


def test_empty_data_set():
    assert framing.has_non_dictionary_pages([], [PLAIN]) is False
    assert framing.has_non_dictionary_pages([(DICT, PLAIN, 1), (INDEX, PLAIN, 3)], [PLAIN]) is False


def test_fallback_on_the_encodings_list():
    assert framing.has_non_dictionary_pages(None, [PD, RLE, BP]) is False
    assert framing.has_non_dictionary_pages(None, [PD]) is False
    assert framing.has_non_dictionary_pages(None, [PD, PD, RLE]) is False  # a list, read as a set
    assert framing.has_non_dictionary_pages(None, [PD, RLE, PLAIN]) is True
    assert framing.has_non_dictionary_pages(None, [RD]) is True            # 2.0 without stats cannot tell
    assert framing.has_non_dictionary_pages(None, [RD, RLE, BP]) is True
    assert framing.has_non_dictionary_pages(None, [PD, RD]) is True
    assert framing.has_non_dictionary_pages(None, []) is True


def test_against_the_reference_exhaustively():
    encs = (PLAIN, PD, RLE, RD, abi.DELTA_BYTE_ARRAY)
    n = 0
    for k in range(4):
        for combo in itertools.product(encs, repeat=k):
            assert framing.has_non_dictionary_pages(None, combo) == G.has_non_dictionary_pages(None, combo), combo
            for types in itertools.product((D, V2, DICT), repeat=k):
                stats = [(t, e, i % 2) for i, (t, e) in enumerate(zip(types, combo))]
                assert framing.has_non_dictionary_pages(stats, [PD]) == G.has_non_dictionary_pages(stats, [PD]), stats
                n += 1
    assert n == sum((5 * 3) ** k for k in range(4))
