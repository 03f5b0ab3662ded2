"""CPU tier: tests/lists_model.py -- the plain Python at_path_with_wildcard rooted at a cell that the columns of sjgpu_at_paths_from_cells_device are
compared with -- is pinned twice: cell for cell against tests/golden/lists.json (the real reference, asked e.at_path_with_wildcard(q) for every e of
doc.at_path_with_wildcard(p), tests/golden/make_lists_golden.py), and against tests/golden/paths.json through the law of composition: the matches of
A + B from a document's root are, in order, the matches of B rooted at the matches of A."""
import json
import os

import numpy as np
import pytest

import checkers
import lists_model
import path_cases
import path_model
import query_cases
import rows_model
from simdjson_amd import _paths

GOLDEN = os.path.join(_paths.REPO_ROOT, "tests", "golden", "lists.json")


def fixture():
    g = json.load(open(GOLDEN))
    tables = [[t if isinstance(t, str) else [g["rows"][r] for r in t] for t in per_doc] for per_doc in g["tables"]]
    return [bytes.fromhex(d) for d in g["documents"]], [bytes.fromhex(p) for p in g["row_paths"]], [bytes.fromhex(p) for p in g["paths"]], tables


@pytest.fixture(scope="module")
def orc():
    return checkers.Oracle()


def parse_all(orc, docs):
    parsed = []
    for d in docs:
        err, tape, sbuf = orc.dom_parse(d)
        assert err == 0, d
        parsed.append((tape, sbuf))
    return parsed


def test_fixture_covers_what_it_is_for():
    docs, row_paths, paths, tables = fixture()
    assert docs == path_cases.fixture()[0]  # the documents of make_paths_golden.py
    assert row_paths == [b"$[*]", b"$.*", b"$.a[*]", b"$.statuses[*]", b"$.*.*"] and 28 <= len(paths) <= 36
    assert os.path.getsize(GOLDEN) <= os.path.getsize(path_cases.GOLDEN)
    assert b"" in paths and any(b"*" in p and p[:1] == b"$" for p in paths) and any(b"*" in p and p[:1] != b"$" for p in paths)
    assert any(b"*" not in p and p for p in paths) and b"$..b" in paths
    flat = [c for per_doc in tables for t in per_doc if not isinstance(t, str) for row in t for c in row]
    for code in (17, 19, 20, 22):
        assert flat.count(f"E {code}") >= 5, code
    assert sum(1 for c in flat if c.count(";") >= 2) >= 100
    # scalar roots: rows that answer every path, the empty and the malformed ones included, with nothing
    rows = [row for per_doc in tables for t in per_doc if not isinstance(t, str) for row in t]
    assert sum(1 for row in rows if all(c == "M" for c in row)) >= 50
    # the hashtags of each status: the parent of every element is kept
    d = docs.index(b'{"statuses":[{"user":{"id":1,"name":"a"},"tags":["x","y"]},{"user":{"id":2},"tags":[]},{"nouser":1},7]}')
    t = tables[d][row_paths.index(b"$.statuses[*]")]
    k = paths.index(b"$.tags[*]")
    assert [row[k] for row in t] == ["M;s 78;s 79", "M", "M", "M"]
    assert [row[paths.index(b"$.user.id")] for row in t] == ["M;l 1", "M;l 2", "E 20", "M"]


def test_model_equals_the_reference_on_the_fixture(orc):
    docs, row_paths, paths, tables = fixture()
    parsed = parse_all(orc, docs)
    tape, sbuf, table = query_cases.lay_out(parsed)
    S = lists_model.Stream(tape, sbuf, table)  # all documents as one stream: absolute indices and offsets
    cells = 0
    for i, (own_tape, own_sbuf) in enumerate(parsed):
        alone = lists_model.Stream(*query_cases.lay_out([parsed[i]]))  # ... and every document alone
        tb, sb = int(table["tape_begin"][i]), int(table["string_begin"][i])
        for j, rp in enumerate(row_paths):
            want = tables[i][j]
            for stream, tb_, sb_ in ((S, tb, sb), (alone, 0, 0)):
                status, roots = path_model.matches(own_tape.tolist(), own_sbuf.tobytes(), rp, tb_, sb_)
                if isinstance(want, str):
                    assert f"E {status}" == want
                    # a failed result answers every path with its code
                    assert all(stream.matches_from((status, 0), p) == (status, []) for p in paths)
                    continue
                assert status == 0 and len(roots) == len(want), (docs[i][:80], rp)
                for root, row in zip(roots, want):
                    for p, cell in zip(paths, row):
                        code, found = stream.matches_from(root, p)
                        assert path_cases.render(code, found, stream.sbuf) == cell, (docs[i][:80], rp, root, p)
                        cells += 1
    assert cells > 15000, cells


def splits(path):
    """every A + B == path with A ending in `[*]` or `.*` and B beginning with `.` or `[`"""
    return [(path[:i], path[i:]) for i in range(2, len(path)) if path[i - 3: i] == b"[*]" or path[i - 2: i] == b".*" if path[i: i + 1] in (b".", b"[")]


def test_composition_equals_the_reference_on_the_paths_fixture(orc):
    """For every document and path of tests/golden/paths.json and every split A + B behind a wildcard with status(A) == 0: the fixture's cell for A + B is the
    concatenation, in order, of the rooted matches of B over the matches of A; a row whose status is not 0 contributes nothing.
    Measured on the model: 1 840 splits, 261 with a non-empty result, 2 465 roots of which 888 are scalars, root statuses 17 x 184, 19 x 47, 20 x 300, 22 x 152."""
    docs, paths, cells = path_cases.fixture()
    parsed = parse_all(orc, docs)
    tape, sbuf, table = query_cases.lay_out(parsed)
    S = lists_model.Stream(tape, sbuf, table)
    checked = nonempty = n_roots = scalars = 0
    codes = {}
    for i, (own_tape, own_sbuf) in enumerate(parsed):
        own_tape, own_sbuf = own_tape.tolist(), own_sbuf.tobytes()
        tb, sb = int(table["tape_begin"][i]), int(table["string_begin"][i])
        for j, p in enumerate(paths):
            for a, b in splits(p):
                status, roots = path_model.matches(own_tape, own_sbuf, a, tb, sb)
                if status:
                    continue
                out = []
                for root in roots:
                    n_roots += 1
                    scalars += root[0] in rows_model.SCALARS
                    code, found = S.matches_from(root, b)
                    if code:
                        assert not found
                        codes[code] = codes.get(code, 0) + 1
                    out += found
                assert path_cases.render(0, out, S.sbuf) == cells[i][j], (docs[i][:80], a, b)
                checked += 1
                nonempty += bool(out)
    print(f"{checked} splits, {nonempty} with a non-empty result, {n_roots} roots of which {scalars} are scalars, root statuses {dict(sorted(codes.items()))}")
    assert checked >= 1800 and nonempty >= 250 and scalars >= 800, (checked, nonempty, scalars)
    assert all(codes.get(c, 0) >= 40 for c in (17, 19, 20, 22)), codes


def test_roots_that_are_no_elements(orc):
    """the rows of the header's table that no composition reaches: cells that disagree with the tape, tags that are none -- for every path, the empty and the
    malformed ones included"""
    parsed = parse_all(orc, [b"[1]", b'{"a":{"b":[1,2,{"c":"d"}]},"n":12}', b"7"])
    tape, sbuf, table = query_cases.lay_out(parsed)
    S = lists_model.Stream(tape, sbuf, table)
    begins = [int(b) for b in table["tape_begin"]]
    a_cell = rows_model.walk_from(S.tape, S.sbuf, rows_model.root_cell(S.tape, S.sbuf, table, 1), b"/a", table)
    tag, value = a_cell
    assert chr(tag) == "{" and S.matches_from(a_cell, b"$.b[*]") == (0, [(ord("l"), 1), (ord("l"), 2), S.matches_from(a_cell, b".b[2]")[1][0]])
    assert S.matches_from(a_cell, b"") == (22, []) and S.matches_from(a_cell, b"$.x") == (20, []) and S.matches_from(a_cell, b"$.x[*]") == (0, [])
    c, high = value & 0xFFFFFFFF, value >> 32
    bad = [(ord("["), value), (tag, ((high + 1) << 32) | c), (tag, (high << 32) | begins[1]), (tag, (high << 32) | begins[3]), (tag, (high << 32) | 0xFFFFFFFF),
           (tag, (high << 32) | (c + 1)), (0, 0), (ord("r"), value), (ord("}"), value), (0x5A, value), (16, 0), (18, 0), (21, 0), (255, 7)]
    everything = (b"", b"$", b"$[*]", b"$.b[*]", b"$.b", b"b", b"$..b", b"$[*")
    for cell in bad:
        assert all(S.matches_from(cell, p) == (20, []) for p in everything), cell
    for code in rows_model.FAILURES:
        assert all(S.matches_from((code, v), p) == (code, []) for p in everything for v in (0, value))
    for scalar in ((ord("l"), 7), (ord("t"), 1), (ord('"'), (3 << 32) | 9), (ord("n"), 0), (ord("d"), 1 << 62), (ord("u"), 1 << 63), (ord("f"), 0)):
        assert all(S.matches_from(scalar, p) == (0, []) for p in everything)
    status, offsets, tags, values = lists_model.column(tape, sbuf, table, (np.array([tag, 17, ord("l"), tag], np.uint8), np.array([value, 0, 5, value + 1], np.uint64)),
                                                       [b"$.b[*]", b"$.b"])
    assert status.tolist() == [[0, 17, 0, 20], [0, 17, 0, 20]] and offsets.tolist() == [0, 3, 3, 3, 3, 4, 4, 4, 4] and [chr(t) for t in tags] == ["l", "l", "{", "["]
