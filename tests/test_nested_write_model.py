"""CPU tier: tests/nested_write_model.py -- the Python model the emulation and the device are compared with -- pinned against tests/golden/nested_write.json, the
texts of the reference's builder::string_builder: every row of every table under every legal combination of the four flags, none skipped; the tables the fixture was
made from are the tables of tests/nested_write_cases.py, by their digest; and what the fixture cannot hold, by rule: doubles without a text, status 19, the counts,
BARE | OMIT_NULLS, and what lies under a validity bit of 0."""
import hashlib
import json
import os

import numpy as np
import pytest

import nested_write_cases as cases
import nested_write_model as model
import write_records_cases as plain_cases
import write_records_model as plain_model

FIXTURE = cases.fixture()
TABLES = cases.fixture_tables()
NEWLINE, OMIT_NULLS, ARRAY_ROWS, BARE = cases.NEWLINE, cases.OMIT_NULLS, cases.ARRAY_ROWS, cases.BARE


def test_the_fixture_was_made_from_these_tables():
    assert sorted(FIXTURE) == sorted(t["name"] for t in TABLES) and len(TABLES) == 10
    for t in TABLES:
        assert hashlib.sha256(cases.table_blob(t)).hexdigest() == FIXTURE[t["name"]]["blob_sha256"], t["name"]
        assert sorted(k for k in FIXTURE[t["name"]] if k != "blob_sha256") == sorted(cases.legal_flags(len(t["fields"]))), t["name"]
    kinds = {f["kind"] for t in TABLES for f in t["fields"] if cases.is_list(f)}
    assert kinds == {cases.INT64, cases.UINT64, cases.DOUBLE, cases.BOOL, cases.STRING, cases.JSON, cases.STRING_CELLS}
    lengths = {len(x) for t in TABLES for f in t["fields"] if cases.is_list(f) for x in f["lists"] if x is not None}
    assert set(cases.LIST_LENGTHS) <= lengths and any(x is None for t in TABLES for f in t["fields"] if cases.is_list(f) for x in f["lists"])
    strings = [e for f in cases._string_lengths()["fields"] for x in f["lists"] for e in x]
    assert {len(e) for e in strings} == set(plain_cases.STRING_LENGTHS)
    assert os.path.getsize(cases.GOLDEN) <= os.path.getsize(plain_cases.GOLDEN)
    assert {f for t in TABLES for f in cases.legal_flags(len(t["fields"]))} == {0, 1, 2, 3, 4, 6, 8, 9, 10, 11}


@pytest.mark.parametrize("table", TABLES, ids=[t["name"] for t in TABLES])
def test_every_row_is_the_references(table):
    for flags in cases.legal_flags(len(table["fields"])):
        for tail_ones, lead in ((False, 0), (True, 7)):
            offsets, chars, status, counts = model.records(cases.arrays_of(table, tail_ones=tail_ones, lead=lead), flags)
            assert not status.any() and int(offsets[-1]) == len(chars)
            cases.assert_rows_are_the_fixtures(FIXTURE[table["name"]][flags], cases.split(offsets, chars), (table["name"], flags))
            lists = [x for f in table["fields"] if cases.is_list(f) for x in f["lists"]]
            invalid = sum(x is None for x in lists) + sum(1 for f in table["fields"] if not cases.is_list(f) for x in f["cells"] if x is None or (f["kind"] == cases.JSON and x == b""))
            elements = [(f["kind"], e) for f in table["fields"] if cases.is_list(f) for x in f["lists"] if x is not None for e in x]
            assert counts.tolist() == [table["n"], 0, invalid, 0, len(elements), sum(1 for k, e in elements if e is None or (k == cases.JSON and e == b""))]


def test_the_issues_own_examples():
    """what the reference writes for the calls the feature's request names"""
    t = {"name": "t", "n": 4, "fields": [cases.list_field(b"a", cases.INT64, [[1, None, (1 << 64) - 3], [], None, [5]])]}
    offsets, chars, _, _ = model.records(cases.arrays_of(t), 0)
    assert cases.split(offsets, chars) == [b'{"a":[1,null,-3]}', b'{"a":[]}', b'{"a":null}', b'{"a":[5]}']
    d = {"name": "t", "n": 1, "fields": [cases.list_field(b"a", cases.DOUBLE, [[cases.bits_of(1.0), cases.bits_of(-0.0), cases.bits_of(1e300)]])]}
    assert model.records(cases.arrays_of(d), BARE)[1] == b"[1.0,-0.0,1e+300]"
    s = {"name": "t", "n": 1, "fields": [cases.list_field(b"a", cases.STRING, [[b'q"', b"\n"]]), cases.column(b"b", cases.BOOL, [1])]}
    assert model.records(cases.arrays_of(s), ARRAY_ROWS | NEWLINE)[1] == b'[["q\\"","\\n"],true]\n'


def test_the_rows_are_what_a_json_parser_reads():
    t = TABLES[0]
    offsets, chars, _, _ = model.records(cases.arrays_of(t), NEWLINE)
    rows = [json.loads(line) for line in chars.split(b"\n") if line]
    assert len(rows) == t["n"] and rows[0]["i"] == [1, None, -3] and rows[0]["j"] == [{"a": [1, 2, {"b": None}]}, None, 7] and rows[2]["i"] is None and rows[1]["u"] == [1, 2]
    offsets, chars, _, _ = model.records(cases.arrays_of(t), ARRAY_ROWS | NEWLINE)
    rows = [json.loads(line) for line in chars.split(b"\n") if line]
    assert rows[5] == [5, [None, 7, None], [3], [1e21, None], [False], ["0123456789abcdef", None, "\x00\x1f"], ["\x7f"], [{}], "f"]


def test_without_lists_and_new_flags_it_is_the_plain_model():
    for t in plain_cases.fixture_tables() + [plain_cases.mixed_table(130), plain_cases.nonfinite_table()]:
        arrays = cases.arrays_of({"name": t["name"], "n": t["n"], "fields": t["columns"]}, tail_ones=True)
        for flags in plain_cases.ALL_FLAGS:
            a, b = model.records(arrays, flags), plain_model.records(cases.as_plain_arrays(arrays), flags)
            assert a[1] == b[1] and np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2]) and a[3].tolist() == b[3].tolist() + [0, 0]


def test_doubles_without_a_text_are_null_by_our_rule_in_a_list_under_omit_nulls_too():
    inf, nan = 0x7FF0000000000000, 0x7FF8000000000ABC
    t = {"name": "t", "n": 3, "fields": [cases.list_field(b"d", cases.DOUBLE, [[cases.bits_of(1.5), inf, None], [nan], []]), cases.column(b"p", cases.DOUBLE, [nan, 0, inf])]}
    for flags, want in ((0, b'{"d":[1.5,null,null],"p":null}{"d":[null],"p":0.0}{"d":[],"p":null}'), (OMIT_NULLS, b'{"d":[1.5,null,null]}{"d":[null],"p":0.0}{"d":[]}'),
                        (ARRAY_ROWS, b"[[1.5,null,null],null][[null],0.0][[],null]")):
        offsets, chars, status, counts = model.records(cases.arrays_of(t), flags)
        assert chars == want and counts.tolist() == [3, 0, 2, 4, 4, 3]


def test_bare_rows_that_are_left_out_are_empty_without_their_newline():
    t = cases._bare_strings()
    offsets, chars, status, counts = model.records(cases.arrays_of(t), BARE | OMIT_NULLS | NEWLINE)
    assert chars == b'["a","\\"",null]\n[]\n["zzzzzzzzzzzzzzzzzzzz"]\n' and np.diff(offsets.astype(np.int64)).tolist() == [16, 0, 3, 0, 0, 25]
    assert not status.any() and counts.tolist() == [6, 0, 3, 0, 4, 1]
    assert model.records(cases.arrays_of(t), BARE | NEWLINE)[1].split(b"\n") == [b'["a","\\"",null]', b"null", b"[]", b"null", b"null", b'["zzzzzzzzzzzzzzzzzzzz"]', b""]
    # fed back as JSON elements, the empty rows are nulls again: composition keeps them
    inner = model.records(cases.arrays_of(t), BARE | OMIT_NULLS)  # (a caller composes WITHOUT the newline)
    outer = {"n": 2, "fields": [{"key": b"ll", "kind": cases.JSON, "values": None, "valid": None, "offsets": inner[0], "chars": np.frombuffer(inner[1], np.uint8),
                                 "chars_bytes": len(inner[1]), "list_offsets": np.array([0, 4, 6], np.uint32), "list_valid": None, "elements": 6}]}
    assert model.records(outer, 0)[1] == b'{"ll":[["a","\\"",null],null,[],null]}{"ll":[null,["zzzzzzzzzzzzzzzzzzzz"]]}'


def test_status_19_empties_the_row_and_a_validity_bit_of_0_hides_the_words():
    a, bad = cases.bad_lists()
    assert bad == [1, 3, 5, 6, 7, 8, 9]
    for flags in (0, 1, 2, 3, ARRAY_ROWS, ARRAY_ROWS | NEWLINE):
        offsets, chars, status, counts = model.records(a, flags)
        assert [r for r in range(a["n"]) if status[r]] == bad and set(status[bad].tolist()) == {19}
        assert all(offsets[r] == offsets[r + 1] for r in bad) and counts.tolist()[:3] == [3, 7, 0] and counts.tolist()[4:] == [5 + 8 + 5, 0]
    assert cases.split(offsets, chars)[2] == b'[[2,3,3,4,4],["s2","t"],["c2"],2]\n'  # (row 2 is longer for row 3's bad offset -- five elements --, and served)
    offsets, chars, status, counts = model.records(cases.hidden_bad_lists(), 0)
    assert not status.any() and counts.tolist() == [10, 0, 2, 0, 49, 10]
    assert cases.split(offsets, chars)[3] == b'{"i":null,"s":["s3","t"],"c":["c3"],"r":3}' and cases.split(offsets, chars)[1] == b'{"i":[1,2],"s":["s1","t"],"c":[null],"r":1}'


def test_the_refusals_that_stand_on_the_flags():
    one, two = cases.arrays_of(cases._bare_strings()), cases.arrays_of(cases._integers())
    assert not any(model.refused(one, f) for f in cases.legal_flags(1)) and not any(model.refused(two, f) for f in cases.legal_flags(2))
    assert all(model.refused(two, f) for f in (BARE, 16, ARRAY_ROWS | OMIT_NULLS, ARRAY_ROWS | BARE)) and model.refused(one, ARRAY_ROWS | BARE)


def test_the_grouping_cases_take_the_road_they_name():
    for name, (t, group) in cases.grouping_cases().items():
        offsets, _, _, _ = model.records(cases.arrays_of(t), NEWLINE)
        assert cases.group_rows(offsets, 0) == group, name
    assert [int(x) for x in np.diff(model.records(cases.arrays_of(cases.digits_table([10, 19, 20, 21, 117])), NEWLINE)[0].astype(np.int64))] == [10, 19, 20, 21, 117]
