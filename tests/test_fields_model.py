"""CPU tier: tests/fields_model.py -- the plain Python object iteration and size() rooted at a cell that the rows of sjgpu_object_fields_from_cells_device and
sjgpu_cell_sizes_device are compared with -- is pinned against tests/golden/fields.json (the real reference, asked e.get_object(), its fields and size() for
every e of doc.at_path_with_wildcard(p), tests/golden/make_fields_golden.py) and, through two laws, against tests/lists_model.py over every row of
tests/golden/lists.json and tests/golden/paths.json: the value cells of an object root are its `$.*` matches, and a container's size is the number of its
fields / of its `$[*]` matches."""
import json
import os

import pytest

import checkers
import fields_model
import path_cases
import path_model
import query_cases
from simdjson_amd import _paths
from test_lists_model import fixture as lists_fixture

GOLDEN = os.path.join(_paths.REPO_ROOT, "tests", "golden", "fields.json")


def fixture():
    """-> (documents, row paths, tables[document][row path]: "E <code>" or the rows' lines, {elements: dom::array::size()})"""
    g = json.load(open(GOLDEN))
    tables = [[t if isinstance(t, str) else [g["rows"][r] for r in t] for t in per_doc] for per_doc in g["tables"]]
    return [bytes.fromhex(d) for d in g["documents"]], [bytes.fromhex(p) for p in g["row_paths"]], tables, {int(k): v for k, v in g["array_sizes"].items()}


def render(S, cell):
    """a root as the fixture's generator prints it"""
    status, slots = S.fields_from(cell)
    size, code = S.size_of(cell)
    assert (code == 0) == (int(cell[0]) in fields_model.CONTAINERS) and (status == 0 or not slots)
    head = str(size if code == 0 else code)
    if status:
        return f"{head} E {status}"
    assert all(kt == ord('"') for kt, _, _, _ in slots)
    return f"{head} F" + "".join(";" + fields_model.pointer_model.string_of(S.sbuf, kv).hex() + ":" + query_cases.render(t, v, S.sbuf) for _, kv, t, v in slots)


@pytest.fixture(scope="module")
def orc():
    return checkers.Oracle()


def parse_all(orc, docs):
    parsed = []
    for d in docs:
        err, tape, sbuf = orc.dom_parse(d)
        assert err == 0, d[:100]
        parsed.append((tape, sbuf))
    return parsed


def test_fixture_covers_what_it_is_for():
    docs, row_paths, tables, array_sizes = fixture()
    lists_docs, lists_row_paths, _, _ = lists_fixture()
    assert docs[: len(lists_docs)] == lists_docs and row_paths == lists_row_paths and len(docs) > len(lists_docs)
    assert os.path.getsize(GOLDEN) < 1 << 18
    rows = [row for per_doc in tables for t in per_doc if not isinstance(t, str) for row in t]
    fields = [f.split(":", 1) for row in rows if " F;" in row for f in row.split(";")[1:]]
    keys = {bytes.fromhex(k) for k, _ in fields}
    assert {b"", b"\x00", b"a\x00b", b"line\nfeed", b'q"uote', b"sl/ash", "\U0001F600".encode(), "é€\U0001F600".encode()} <= keys
    assert any(row == "0 F" for row in rows) and any(row.startswith("1 F;") for row in rows) and any(row.startswith("300 F;") and row.count(";") == 300 for row in rows)
    assert any(row.count(";64:") == 3 for row in rows)  # duplicate keys, all kept, in order
    assert {v[0] for _, v in fields} == set('ludtfns{[')  # every kind of value, objects and arrays nested as values among them
    assert {row for row in rows if " E " in row} >= {"17 E 17", "0 E 17", "3 E 17"}  # scalars, and arrays with their sizes
    assert array_sizes == {0xFFFFFE: 0xFFFFFE, 0xFFFFFF: 0xFFFFFF, 0x1000000: 0xFFFFFF}  # size() saturates with the tape's count field


def test_model_equals_the_reference_on_the_fixture(orc):
    docs, row_paths, tables, _ = fixture()
    parsed = parse_all(orc, docs)
    tape, sbuf, table = query_cases.lay_out(parsed)
    S = fields_model.Stream(tape, sbuf, table)  # all documents as one stream: absolute indices and offsets
    cells = 0
    for i, (own_tape, own_sbuf) in enumerate(parsed):
        alone = fields_model.Stream(*query_cases.lay_out([parsed[i]]))  # ... and every document alone
        tb, sb = int(table["tape_begin"][i]), int(table["string_begin"][i])
        for j, rp in enumerate(row_paths):
            want = tables[i][j]
            for stream, tb_, sb_ in ((S, tb, sb), (alone, 0, 0)):
                status, roots = path_model.matches(own_tape.tolist(), own_sbuf.tobytes(), rp, tb_, sb_)
                if isinstance(want, str):
                    assert f"E {status}" == want
                    assert stream.fields_from((status, 0)) == (status, []) and stream.size_of((status, 0)) == (0, status)  # a failed result is forwarded
                    continue
                assert status == 0 and len(roots) == len(want), (docs[i][:80], rp)
                for root, row in zip(roots, want):
                    assert render(stream, root) == row, (docs[i][:80], rp, root)
                    cells += 1
    assert cells > 1400, cells


def rows_of_the_other_fixtures(orc):
    """every row of tests/golden/lists.json and tests/golden/paths.json, and of the fields fixture: (stream, root cell)"""
    docs, row_paths, _, _ = fixture()  # (the documents of the lists fixture, and more)
    p_docs, p_paths, _ = path_cases.fixture()
    for documents, paths in ((docs, row_paths), (p_docs, p_paths)):
        parsed = parse_all(orc, documents)
        tape, sbuf, table = query_cases.lay_out(parsed)
        S = fields_model.Stream(tape, sbuf, table)
        for i, (own_tape, own_sbuf) in enumerate(parsed):
            own_tape, own_sbuf = own_tape.tolist(), own_sbuf.tobytes()
            for p in paths:
                status, roots = path_model.matches(own_tape, own_sbuf, p, int(table["tape_begin"][i]), int(table["string_begin"][i]))
                for root in roots:
                    yield S, root


def test_the_two_laws_over_the_rows_of_the_lists_and_paths_fixtures(orc):
    """Law 1: the value cells of an object root are, in order, lists_model's matches of `$.*`.  Law 2: an object's size is the number of its fields, an
    array's the number of its `$[*]` matches."""
    objects = arrays = scalars = fields = 0
    for S, root in rows_of_the_other_fixtures(orc):
        status, slots = S.fields_from(root)
        size, code = S.size_of(root)
        if root[0] == ord("{"):
            assert (status, code) == (0, 0)
            assert (0, [(t, v) for _, _, t, v in slots]) == S.matches_from(root, b"$.*"), root  # (tests/lists_model.py's, inherited)
            assert size == len(slots)
            objects += 1
            fields += len(slots)
        elif root[0] == ord("["):
            assert (status, slots, code) == (17, [], 0)
            elements = S.matches_from(root, b"$[*]")
            assert (elements[0], len(elements[1])) == (0, size), root
            arrays += 1
        else:
            assert (status, slots, size, code) == (17, [], 0, 17)
            scalars += 1
    print(f"{objects} object rows with {fields} fields, {arrays} array rows, {scalars} scalar rows")
    assert objects > 400 and arrays > 400 and scalars > 800 and fields > 1000, (objects, arrays, scalars, fields)  # (what the fixtures hold: 446, 496, 891, 1 078)


def test_roots_that_are_no_elements_and_patched_counts(orc):
    parsed = parse_all(orc, [b"[1]", b'{"a":{"x":1,"y":[2],"z":"s"},"n":12}', b"7"])
    tape, sbuf, table = query_cases.lay_out(parsed)
    S = fields_model.Stream(tape, sbuf, table)
    begins = [int(b) for b in table["tape_begin"]]
    a_cell = S.matches_from(fields_model.rows_model.root_cell(S.tape, S.sbuf, table, 1), b"$.a")[1][0]
    tag, value = a_cell
    status, slots = S.fields_from(a_cell)
    assert chr(tag) == "{" and status == 0 and [chr(t) for _, _, t, _ in slots] == ["l", "[", '"'] and S.size_of(a_cell) == (3, 0)
    assert [fields_model.pointer_model.string_of(S.sbuf, kv) for _, kv, _, _ in slots] == [b"x", b"y", b"z"]
    c, high = value & 0xFFFFFFFF, value >> 32
    bad = [(ord("["), value), (tag, ((high + 1) << 32) | c), (tag, (high << 32) | begins[1]), (tag, (high << 32) | begins[3]), (tag, (high << 32) | 0xFFFFFFFF),
           (tag, (high << 32) | (c + 1)), (0, 0), (ord("r"), value), (ord("}"), value), (0x5A, value), (16, 0), (18, 0), (21, 0), (255, 7)]
    for cell in bad:
        assert S.fields_from(cell) == (20, []) and S.size_of(cell) == (0, 20), cell
    for code in (17, 19, 20, 22):
        assert S.fields_from((code, value)) == (code, []) and S.size_of((code, value)) == (0, code)
    for scalar in ((ord("l"), 7), (ord("t"), 1), (ord('"'), (3 << 32) | 9), (ord("n"), 0), (ord("d"), 1 << 62), (ord("u"), 1 << 63), (ord("f"), 0)):
        assert S.fields_from(scalar) == (17, []) and S.size_of(scalar) == (0, 17)
    # the count field decides the slots; saturated, the walk does
    for patched, want in ((0xFFFFFF, slots), (5, slots + [fields_model.PAD] * 2), (2, slots[:2]), (0, [])):
        P = fields_model.Stream(list(S.tape), S.sbuf, table)
        P.tape[c] = (P.tape[c] & ~(0xFFFFFF << 32)) | (patched << 32)
        assert P.fields_from(a_cell) == (0, want) and P.size_of(a_cell) == (patched, 0), patched
