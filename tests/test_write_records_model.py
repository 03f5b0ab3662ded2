"""CPU tier: tests/write_records_model.py -- the Python model the emulation and the device are compared with -- pinned against tests/golden/write_records.json, the
texts of the reference's builder::string_builder: every row of every table under all four combinations of the flags, none skipped; the tables the fixture was
made from are the tables of tests/write_records_cases.py, by their digest; and what the fixture cannot hold, by rule: doubles without a text, status 19, the counts,
validity bits beyond n."""
import hashlib

import numpy as np
import pytest

import write_records_cases as cases
import write_records_model as model

FIXTURE = cases.fixture()
TABLES = cases.fixture_tables()


def test_the_fixture_was_made_from_these_tables():
    assert sorted(FIXTURE) == sorted(t["name"] for t in TABLES) and len(TABLES) == 8
    for t in TABLES:
        assert hashlib.sha256(cases.table_blob(t)).hexdigest() == FIXTURE[t["name"]]["blob_sha256"], t["name"]
    kinds = {c["kind"] for t in TABLES for c in t["columns"]}
    assert kinds == {cases.INT64, cases.UINT64, cases.DOUBLE, cases.BOOL, cases.STRING, cases.JSON, cases.STRING_CELLS}
    assert any(len(c["key"]) == 1024 for t in TABLES for c in t["columns"]) and any(c["key"] == b"" for t in TABLES for c in t["columns"])
    assert set(b"".join(c for c in TABLES[3]["columns"][0]["cells"])) == set(range(256))


@pytest.mark.parametrize("table", TABLES, ids=[t["name"] for t in TABLES])
@pytest.mark.parametrize("flags", cases.ALL_FLAGS)
def test_every_row_is_the_references(table, flags):
    for tail_ones in (False, True):
        offsets, chars, status, counts = model.records(cases.arrays_of(table, tail_ones=tail_ones), flags)
        assert not status.any() and int(offsets[-1]) == len(chars)
        cases.assert_rows_are_the_fixtures(FIXTURE[table["name"]][flags], cases.split(offsets, chars), (table["name"], flags))
        invalid = sum(1 for c in table["columns"] for x in c["cells"] if x is None or (c["kind"] == cases.JSON and x == b""))
        assert counts.tolist() == [table["n"], 0, invalid, 0]


def test_the_rows_are_what_a_json_parser_reads():
    import json
    t = TABLES[0]
    offsets, chars, _, _ = model.records(cases.arrays_of(t), cases.NEWLINE)
    rows = [json.loads(line) for line in chars.split(b"\n") if line]
    assert len(rows) == t["n"] and rows[0] == {"i": 0, "u": 0, "d": 0.0, "b": False, "s": "", "c": "cell", "j": {"a": [1, 2, {"b": None}]}}
    offsets, chars, _, _ = model.records(cases.arrays_of(t), cases.NEWLINE | cases.OMIT_NULLS)
    assert json.loads(chars.split(b"\n")[2]) == {"i": -1, "u": (1 << 64) - 1, "b": True, "c": ""}


def test_doubles_without_a_text_are_null_by_our_rule():
    t = cases.nonfinite_table()
    a = cases.arrays_of(t)
    offsets, chars, status, counts = model.records(a, 0)
    rows = cases.split(offsets, chars)
    assert rows[0] == b'{"d":1.0,"r":0}' and rows[7] == b'{"d":-0.0,"r":7}' and rows[9] == b'{"d":1.7976931348623157e+308,"r":9}'
    assert all(rows[r] == b'{"d":null,"r":%d}' % r for r in (1, 2, 3, 4, 5, 6, 8)) and not status.any()
    assert counts.tolist() == [10, 0, 7, 6]
    offsets, chars, status, counts = model.records(a, cases.OMIT_NULLS)
    assert all(cases.split(offsets, chars)[r] == b'{"r":%d}' % r for r in (1, 2, 3, 4, 5, 6, 8)) and counts.tolist() == [10, 0, 7, 6]


def test_a_row_whose_fields_are_all_left_out_and_no_columns_at_all():
    t = {"name": "t", "n": 2, "columns": [cases.column(b"a", cases.INT64, [None, 5]), cases.column(b"j", cases.JSON, [b"", None])]}
    for flags, want in ((cases.OMIT_NULLS, b'{}{"a":5}'), (cases.OMIT_NULLS | cases.NEWLINE, b'{}\n{"a":5}\n'), (0, b'{"a":null,"j":null}{"a":5,"j":null}')):
        assert model.records(cases.arrays_of(t), flags)[1] == want
    offsets, chars, status, counts = model.records({"n": 3, "columns": []}, cases.NEWLINE)
    assert chars == b"{}\n{}\n{}\n" and offsets.tolist() == [0, 3, 6, 9] and counts.tolist() == [3, 0, 0, 0]
    offsets, chars, status, counts = model.records({"n": 0, "columns": []}, 0)
    assert chars == b"" and offsets.tolist() == [0] and counts.tolist() == [0, 0, 0, 0] and len(status) == 0


def test_status_19_empties_the_row_and_a_validity_bit_of_0_hides_the_cell():
    a, bad = cases.bad_offsets()
    assert bad == [3, 6, 7, 9, 10, 11]
    for flags in cases.ALL_FLAGS:
        offsets, chars, status, counts = model.records(a, flags)
        assert [r for r in range(a["n"]) if status[r]] == bad and set(status[bad].tolist()) == {19}
        assert all(offsets[r] == offsets[r + 1] for r in bad) and counts.tolist() == [a["n"] - len(bad), len(bad), 0, 0]
    assert cases.split(offsets, chars)[2] == b'{"s":"s2s3s4","j":2,"c":"s2","i":2}\n'
    a, bad = cases.bad_offsets(arrays_under_valid_bits=True)
    offsets, chars, status, counts = model.records(a, 0)
    assert bad == [] and not status.any() and counts.tolist() == [a["n"], 0, 6, 0]
    assert cases.split(offsets, chars)[3] == b'{"s":null,"j":3,"c":"s3","i":3}' and cases.split(offsets, chars)[10] == b'{"s":"s10","j":10,"c":null,"i":10}'


def test_validity_bits_beyond_n_are_not_looked_at():
    t = cases.mixed_table(70)
    plain, ones = cases.arrays_of(t), cases.arrays_of(t, tail_ones=True)
    assert any(c["valid"] is not None and int(c["valid"][-1]) >> 6 == (1 << 58) - 1 for c in ones["columns"])
    a, b = model.records(plain, cases.NEWLINE), model.records(ones, cases.NEWLINE)
    assert a[1] == b[1] and np.array_equal(a[0], b[0]) and np.array_equal(a[3], b[3]) and a[3][3] > 0


def test_the_span_tables_take_what_they_say():
    for total in (cases.WINDOW - 1, cases.WINDOW, cases.WINDOW + 1):
        offsets, chars, _, _ = model.records(cases.arrays_of(cases.span_table(total, rows_after=3)), cases.NEWLINE)
        assert int(offsets[cases.ROWS_PER_STEP]) == total and len(offsets) == cases.ROWS_PER_STEP + 4
