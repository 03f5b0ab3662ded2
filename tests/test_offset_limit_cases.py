"""CPU tier: what tests/offset_limit_cases.py -- the plan of tests/test_gpu_offset_limits.py -- claims about itself.  Every total is the sum of its runs and
lies where its level says (inside (2^31, 2^32), on 2^32 - 1, on 2^32 or on the first total above it the rows allow); the length the plan assumes for each distinct
row is the length of that row's text, matches or fields in the Python models (each pinned against the real reference on this tier); and every case, scaled down
to a handful of rows, gives offsets in the models that are the plan's arithmetic progression.  The document's tape is the oracle's."""
import numpy as np
import pytest

import checkers
import fields_model
import json_text_model
import lists_model
import nested_write_model
import offset_limit_cases as C
import pointer_model
import query_cases
import write_records_model


@pytest.fixture(scope="module")
def stream():
    """the document's tape, string buffer and table (the oracle's parse), and the root cell of every pointer (tests/pointer_model.py)"""
    doc = np.frombuffer(C.document(), np.uint8)
    err, tape, sbuf = checkers.Oracle().dom_parse(doc)
    assert err == 0
    tape, sbuf, table = query_cases.lay_out([(tape, sbuf)])
    tape_list, sbuf_bytes = tape.tolist(), sbuf.tobytes()
    cells = {name: pointer_model.walk(tape_list, sbuf_bytes, ptr) for name, ptr in C.ROOT_POINTERS.items()}
    return tape, sbuf, table, cells


def test_every_total_is_the_sum_of_its_runs_and_lies_at_its_level():
    seen = set()
    for case in C.ALL_CASES:
        lengths = C.LENGTHS[case.call]
        total = C.total_of(case, lengths)
        assert total == case.total, (case.call, case.name, total)
        assert rows_in_32_bits(C.rows_of(case))
        if case.level == "T1":
            assert C.HALF < total < C.LIMIT
            # the offsets of a served case: a progression of equal rows that ends on the total; the last row ends beyond 2^31, so bytes of it are written at
            # positions with bit 31 set (these are the smallest such totals: the T2 cases have half of their offsets up there, count only)
            offsets = C.offsets_of(case, lengths)
            assert int(offsets[-1]) == total and int(offsets[-2]) < total - 1 and len(set(np.diff(offsets).tolist())) == 1
        elif case.level == "T2":
            assert total == C.T2 == 0xFFFFFFFF and int(C.offsets_of(case, lengths)[-1]) == 0xFFFFFFFF
        else:
            assert total >= C.T3
            if total != C.T3:  # rows of 65 536 bytes alone: one row beyond the 65 536 that make 2^32 exactly -- the total wraps to one row, not to 0
                assert total - min(lengths[name] for name, _ in case.runs) == C.LIMIT
        seen.add((case.call, case.level))
    assert seen == {(call, level) for call in C.LENGTHS for level in ("T1", "T2", "T3")}
    # the products the plan is built on
    assert 65535 * 65537 == C.T2 and 65535 * 65536 + 65535 == C.T2 and 32768 * 65538 == 2147549184


def rows_in_32_bits(rows):
    return 0 < rows < 0xFFFFFFF0


def test_the_single_row_beyond_32_bits():
    """64 columns over one cell of 64 MiB: the row's own length wraps 32 bits.  The model writes the row for cells of 5 and 70 bytes: its length is the
    plan's formula at both, the formula is linear in the cell, and at 64 MiB it is 2^32 + 449"""
    for cell in (5, 70):
        offsets, chars, status, counts = write_records_model.records(C.wide_columns(cell), 0)
        assert offsets.tolist() == [0, C.wide_row_bytes(cell)] and status.tolist() == [0] and len(chars) == C.wide_row_bytes(cell)
        assert chars.startswith(b'{"k00":' + b"1" * cell + b',"k01":') and chars.endswith(b'"k63":' + b"1" * cell + b"}")
    assert C.wide_row_bytes(70) - C.wide_row_bytes(5) == 64 * 65
    assert C.WIDE_ROW_TOTAL == C.wide_row_bytes(64 << 20) == (1 << 32) + 449
    assert C.WIDE_ROW_TOTAL & 0xFFFFFFFF == 449  # what a 32-bit length would hold


def test_the_gather_s_cells_have_the_lengths_assumed():
    sbuf, cells = C.gather_buffer()
    assert len(sbuf) == sum(C.GATHER_LENGTHS.values())
    texts = {name: pointer_model.string_of(sbuf, value) for name, (tag, value) in cells.items()}
    assert {name: len(t) for name, t in texts.items()} == C.GATHER_LENGTHS and all(tag == C.QUOTE for tag, _ in cells.values())
    assert len({t[:1] for t in texts.values()}) == 3  # three different letters: a byte of the wrong record shows
    for case in C.GATHER:
        few = C.scaled(case)
        want = b"".join(texts[name] for name in C.row_names(few))
        assert len(want) == int(C.offsets_of(few, C.GATHER_LENGTHS)[-1])


def test_the_document_s_cells_have_the_lengths_assumed(stream):
    tape, sbuf, table, cells = stream
    assert [chr(cells[n][0]) for n in ("a", "b", "c", "oa", "ob", "oc", "s", "t", "one", "arr")] == list('[[[{{{""l[')
    L = lists_model.Stream(tape, sbuf, table)
    for name, want in C.PATH_LENGTHS.items():
        code, found = L.matches_from(cells[name], C.PATH)
        assert code == 0 and len(found) == want and set(found) == {(C.INT64, 1)}, name
    F = fields_model.Stream(tape, sbuf, table)
    for name, want in C.FIELD_LENGTHS.items():
        code, found = F.fields_from(cells[name])
        assert code == 0 and len(found) == want < fields_model.SATURATED, name
        assert fields_model.count_field(tape[cells[name][1] & 0xFFFFFFFF]) == want  # the count the device reads
        assert {(kt, t, v) for kt, _, t, v in found} == {(C.QUOTE, C.INT64, 1)}, name
    J = json_text_model.Stream(tape, sbuf, table)
    for name, want in C.TEXT_LENGTHS.items():
        code, text = J.text_of(cells[name])
        assert code == 0 and len(text) == want, (name, len(text))
    assert J.text_of(cells["one"])[1] == b"1" and J.text_of(cells["arr"])[1] == b"[10" + b",1" * (C.ARR_ELEMENTS - 1) + b"]"
    assert J.text_of(cells["t"])[1] == b'"' + b"y" * 65536 + b'"'


def test_the_cases_rooted_at_cells_scaled_down(stream):
    tape, sbuf, table, cells = stream

    def roots(case):
        names = C.row_names(case)
        return np.array([cells[n][0] for n in names], np.uint8), np.array([cells[n][1] for n in names], np.uint64)
    for case in C.PATHS_FROM_CELLS:
        few = C.scaled(case, 2)
        status, offsets, tags, values = lists_model.column(tape, sbuf, table, roots(few), [C.PATH])
        assert not status.any() and np.array_equal(offsets, C.offsets_of(few, C.PATH_LENGTHS).astype(np.uint32)), case.name
    F = fields_model.Stream(tape, sbuf, table)
    for case in C.FIELDS_FROM_CELLS:
        few = C.scaled(case, 2)
        status, offsets = fields_model.column(F, roots(few))[:2]
        assert not status.any() and np.array_equal(offsets, C.offsets_of(few, C.FIELD_LENGTHS).astype(np.uint32)), case.name
    J = json_text_model.Stream(tape, sbuf, table)
    for case in C.SERIALIZE:
        few = C.scaled(case, 3)
        offsets, chars, status = json_text_model.column(J, roots(few))
        assert not status.any() and np.array_equal(offsets, C.offsets_of(few, C.TEXT_LENGTHS).astype(np.uint32)) and len(chars) == int(offsets[-1]), case.name


def test_the_writers_rows_have_the_lengths_assumed_and_the_cases_scaled_down():
    chars = C.write_chars()
    for name, want in C.WRITE_LENGTHS.items():
        offsets, text, status, counts = write_records_model.records(C.write_columns([name], chars), 0)
        assert offsets.tolist() == [0, want] and status.tolist() == [0] and text == b'{"k":"' + b"x" * C.WRITE_STRINGS[name] + b'"}', name
        assert want == C.WRITE_STRINGS[name] + 8
    for name, want in C.NESTED_LENGTHS.items():
        offsets, text, status, counts = nested_write_model.records(C.nested_fields([name], chars), 0)
        element = b'"' + b"x" * C.NESTED_STRINGS[name] + b'"'
        assert offsets.tolist() == [0, want] and status.tolist() == [0] and text == b'{"k":[' + b",".join([element] * C.NESTED_ELEMENTS[name]) + b"]}", name
    for case in C.WRITE_RECORDS:
        few = C.scaled(case, 3)
        offsets, text, status, counts = write_records_model.records(C.write_columns(C.row_names(few), chars), 0)
        assert not status.any() and np.array_equal(offsets, C.offsets_of(few, C.WRITE_LENGTHS).astype(np.uint32)) and counts.tolist() == [C.rows_of(few), 0, 0, 0]
    for case in C.WRITE_NESTED:
        few = C.scaled(case, 3)
        offsets, text, status, counts = nested_write_model.records(C.nested_fields(C.row_names(few), chars), 0)
        elements = sum(C.NESTED_ELEMENTS[n] for n in C.row_names(few))
        assert not status.any() and np.array_equal(offsets, C.offsets_of(few, C.NESTED_LENGTHS).astype(np.uint32))
        assert counts.tolist() == [C.rows_of(few), 0, 0, 0, elements, 0]


def test_the_streams_of_the_calls_rooted_at_documents():
    """the sums of the plan, and the stream's text for a few small arrays: every line parses (the oracle) to an array whose $[*] has as many matches as the
    line has ones and whose count field says so"""
    for name, elements in C.STREAMS.items():
        assert max(elements) < (1 << 24) - 1 and min(elements) >= 1
    D, E = len(C.STREAM_T2), sum(C.STREAM_T2)
    assert (D, E) == (1011, 68174068) and 63 * E + D == C.T2
    assert sum(C.STREAM_T3) == 1 << 26 and 64 * sum(C.STREAM_T3) == C.T3
    for case in C.ROOTS:
        lengths = C.roots_lengths(case)
        assert int(lengths.sum()) == case.total and len(lengths) == len(case.paths) * len(C.STREAMS[case.stream])
        assert {"T1": C.HALF < case.total < C.LIMIT, "T2": case.total == C.T2, "T3": case.total == C.T3}[case.level]
    assert sum(2 * e + 2 for e in C.STREAM_T2) < 140 << 20 and sum(2 * e + 2 for e in C.STREAM_T3) < 140 << 20
    small = (1, 2, 5, 2, 67)
    text = C.roots_stream(small).tobytes()
    assert text == b"".join(b"[" + b",".join([b"1"] * e) + b"]\n" for e in small)
    orc = checkers.Oracle()
    parsed = []
    for line in text.splitlines():
        err, tape, sbuf = orc.dom_parse(np.frombuffer(line, np.uint8))
        assert err == 0
        parsed.append((tape, sbuf))
    tape, sbuf, table = query_cases.lay_out(parsed)
    import json_text_cases
    roots = json_text_cases.root_row(tape, sbuf, table)
    status, offsets, tags, values = lists_model.column(tape, sbuf, table, roots, [C.PATH, b"$[0]"])
    assert not status.any() and np.diff(offsets.astype(np.int64)).tolist() == list(small) + [1] * len(small)
