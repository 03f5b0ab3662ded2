"""CPU tier: tests/pivot_model.py -- the numpy model of sjgpu_pivot_fields_device and the fold rule of at_key_case_insensitive -- against tests/golden/pivot.json,
what the REAL reference answers for element::at_key(k) and element::at_key_case_insensitive(k) (tests/golden/make_pivot_golden.py).  The records go through
Python's json into the long format (parent row, key, value), the keys into codes in order of first occurrence, the listed keys into a map from codes to columns,
and the model's table must be the reference's answers, plain and folded.  simdjson_amd/pivot.py's fold_key and column_map are held to the same fixture."""
import numpy as np

import pivot_model
from simdjson_amd import pivot


def test_the_fixture_holds_what_it_was_made_for():
    sets = pivot_model.fixture()
    records = b"\n".join(r for s in sets for r in s[0])
    for needle in (b'{"a":1,"a":2}', b'"\\u0041"', b'"":', b'"/"', b'"~"', b'"a\\u0000b"', b'"A\\u0000c"', b'"ID":1,"Id":2,"id":3', b'"\xc3\xa9"', b'"\xc3\x89"', b"[1,2]", b'"str"',
                   b"null", b"{}", b'{"p":{"q":[]}}'):
        assert needle in records, needle
    answers = {a for s in sets for table in s[2:] for row in table for a in row}
    assert {"E 17", "E 20", "V 1", 'V {"p":{"q":[]}}'} <= answers
    for _, keys, plain, folded in sets:
        assert b"absent" in keys and all(len(row) == len(keys) for row in plain + folded)


def test_the_model_answers_what_the_reference_answers():
    differ = 0
    for records, keys, plain, folded in pivot_model.fixture():
        assert pivot_model.answers(records, keys, False) == plain
        assert pivot_model.answers(records, keys, True) == folded
        differ += plain != folded
    assert differ >= 2  # the fold is seen: ID / Id / id, NAME / Name


def test_the_fold_rule():
    f = pivot_model.fold_class
    assert f(b"a\0b") == f(b"A\0c") == f(b"a\0c") != f(b"a\0") and f(b"ID") == f(b"id") == f(b"Id") != f(b"ID ")
    assert f(b"\xc3\xa9") != f(b"\xc3\x89") and f(b"\xc3\xa9X") == f(b"\xc3\xa9x") and f(b"") == f(b"") != f(b"\0")
    for _, keys, _, _ in pivot_model.fixture():
        for a in keys:
            assert pivot.fold_key(a) == f(a)


def test_column_map_of_the_package():
    """records_many's map: every key in order of first occurrence, min_count, a list with unknown and repeated keys, the classes named by their first spelling"""
    for records, keys, plain, folded in pivot_model.fixture():
        _, _, slot_keys, _ = pivot_model.long_format(records)
        codes, dictionary = pivot_model.encode(slot_keys)
        counts = np.bincount(codes, minlength=len(dictionary))
        for fold in (False, True):
            names, column_of_code, pick = pivot.column_map(dictionary, counts, keys, 1, fold)
            want_map, want_pick = pivot_model.column_map(dictionary, keys, fold)
            assert names == keys and np.array_equal(column_of_code, want_map) and (pick or list(range(len(keys)))) == want_pick
        names, column_of_code, pick = pivot.column_map(dictionary, counts)
        assert names == dictionary and column_of_code.tolist() == list(range(len(dictionary))) and pick is None
        names, column_of_code, pick = pivot.column_map(dictionary, counts, None, 2)
        assert names == [k for k, n in zip(dictionary, counts) if n >= 2] and pick is None
        assert [names[c] if c >= 0 else None for c in column_of_code] == [k if n >= 2 else None for k, n in zip(dictionary, counts)]
        names, column_of_code, pick = pivot.column_map(dictionary, counts, None, 1, True)
        classes = {}
        for k in dictionary:
            classes.setdefault(pivot_model.fold_class(k), k)
        assert names == list(classes.values()) and pick is None
        assert [names[c] for c in column_of_code] == [classes[pivot_model.fold_class(k)] for k in dictionary]
