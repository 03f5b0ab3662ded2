"""CPU tier: tests/rows_model.py -- the plain Python at_pointer rooted at a cell that the columns of sjgpu_at_pointers_from_cells_device are compared with --
is pinned against tests/golden/pointers.json (the real reference's dom::parser::parse(document).at_pointer(pointer)) through the reference's own law:
at_pointer on a child is the recursion step of at_pointer on its parent, so doc.at_pointer(a).at_pointer(b) == doc.at_pointer(a + b) whenever the first
call succeeds, and an error stays the error it is (simdjson_result<element>::at_pointer)."""
import pytest

import checkers
import pointer_model
import query_cases
import rows_model


@pytest.fixture(scope="module")
def orc():
    return checkers.Oracle()


@pytest.fixture(scope="module")
def stream(orc):
    docs, pointers, cells = query_cases.fixture()
    parsed = []
    for d in docs:
        err, tape, sbuf = orc.dom_parse(d)
        assert err == 0, d
        parsed.append((tape, sbuf))
    tape, sbuf, table = query_cases.lay_out(parsed)
    return docs, pointers, cells, parsed, tape.tolist(), sbuf.tobytes(), table


def splits(pointer):
    """every a + b == pointer with b beginning at a slash, and the split behind the last byte"""
    return [(pointer[:i], pointer[i:]) for i in range(len(pointer)) if pointer[i: i + 1] == b"/"] + [(pointer, b"")]


def test_composition_equals_the_reference_on_the_fixture(stream):
    """For every fixture document and pointer and every split a + b: walk(a) succeeded -> walk_from(cell(a), b) is the fixture's cell for a + b; walk(a) failed ->
    walk_from returns that code.
    Not vacuous, on the model alone: at least 30 % of the COMPOSED cells are hits and each of 17, 19, 20 and 22 occurs among them.  A composed cell is one that two
    walks made: a is not empty and walk(a) found an element, so walk_from started below a document's root.  The other splits are checked against the law all the
    same, but compose nothing -- with a empty walk_from starts at the root like tests/pointer_model.py's walk, and behind a failed walk(a) nothing is walked.
    Measured: 732 composed cells, 292 of them hits (39.9 %), 263 x 20, 68 x 22, 59 x 17, 50 x 19; their roots are 254 objects, 178 arrays and 300 scalars.  The split
    behind the last byte (b empty: the empty pointer asked of a found cell) is among them; without it 98 of 538 (18.2 %).  Over ALL 15 925 splits 551 are hits
    (3.5 %): the fixture was made to hold every error at least a hundred times, and only 4.4 % of its own cells are hits, so no reading that counts the splits
    with an empty a can reach 30 %."""
    docs, pointers, cells, parsed, tape, sbuf, table = stream
    checked = composed = hits = 0
    seen = set()
    for i in range(len(docs)):
        root = rows_model.root_cell(tape, sbuf, table, i)
        own_tape, own_sbuf = parsed[i]
        tb, sb = int(table["tape_begin"][i]), int(table["string_begin"][i])
        assert root == pointer_model.walk(own_tape, own_sbuf, b"", tb, sb)
        for j, p in enumerate(pointers):
            for a, b in splits(p):
                first = rows_model.walk_from(tape, sbuf, root, a, table)
                assert first == pointer_model.walk(own_tape, own_sbuf, a, tb, sb), (docs[i][:80], a)
                second = rows_model.walk_from(tape, sbuf, first, b, table)
                checked += 1
                if first[0] in rows_model.FAILURES:
                    assert second == (first[0], 0), (docs[i][:80], a, b)
                    continue
                assert query_cases.render(second[0], second[1], sbuf) == cells[i][j], (docs[i][:80], a, b)
                if a:
                    composed += 1
                    hits += second[0] >= 34
                    seen.add(second[0])
    print(f"{checked} splits, {composed} composed cells, {hits} hits")
    assert checked > 10000 and composed > 500 and hits >= 0.30 * composed, (checked, composed, hits)
    assert set(rows_model.FAILURES) <= seen, seen


def test_roots_that_are_no_elements(stream):
    """the rows of the header's table that no composition reaches: cells that disagree with the tape, tags that are none"""
    docs, pointers, cells, parsed, tape, sbuf, table = stream
    first = b'{"a":1,"b":{"c":[10,20,{"d":"x"}]},"":"empty key","0":"zero","a/b":"slash","m~n":"tilde"}'
    i = docs.index(first)
    base, end = int(table["tape_begin"][i]), int(table["tape_begin"][i + 1])
    root = rows_model.root_cell(tape, sbuf, table, i)
    b_cell = rows_model.walk_from(tape, sbuf, root, b"/b", table)
    assert chr(b_cell[0]) == "{" and rows_model.walk_from(tape, sbuf, b_cell, b"/c/1", table) == (ord("l"), 20)
    tag, value = b_cell
    c, high = value & 0xFFFFFFFF, value >> 32
    bad = [(ord("["), value),                                  # the tape's word there opens an object
           (tag, ((high + 1) << 32) | c), (tag, ((high - 1) << 32) | c),  # not where the tape's word points
           (tag, (high << 32) | base), (tag, (high << 32) | end),       # on a root word
           (tag, (high << 32) | len(tape)), (tag, (high << 32) | 0xFFFFFFFF),  # behind the last document
           (tag, (high << 32) | (c + 1)),                         # a key word
           (0, 0), (ord("r"), value), (ord("}"), value), (0x5A, value), (16, 0), (18, 0), (21, 0), (255, 7)]  # tags that are none
    for cell in bad:
        for p in (b"", b"/c", b"c", b"/~2"):
            assert rows_model.walk_from(tape, sbuf, cell, p, table) == (20, 0), (cell, p)
    if base:  # the last word of the document in front: a root word too
        assert rows_model.walk_from(tape, sbuf, (tag, (high << 32) | (base - 1)), b"", table) == (20, 0)
    for code in rows_model.FAILURES:
        for p in (b"", b"/c", b"c", b"/~2"):
            assert rows_model.walk_from(tape, sbuf, (code, 0), p, table) == (code, 0)
            assert rows_model.walk_from(tape, sbuf, (code, 12345), p, table) == (code, 0)
    for scalar in ((ord("l"), 7), (ord("t"), 1), (ord('"'), (3 << 32) | 9), (ord("n"), 0), (ord("d"), 1 << 62), (ord("u"), 1 << 63), (ord("f"), 0)):
        assert rows_model.walk_from(tape, sbuf, scalar, b"", table) == scalar  # unchanged, whatever its value says
        assert rows_model.walk_from(tape, sbuf, scalar, b"/x", table) == (20, 0) and rows_model.walk_from(tape, sbuf, scalar, b"/x/~0/~2", table) == (20, 0)
        assert rows_model.walk_from(tape, sbuf, scalar, b"x", table) == (22, 0) and rows_model.walk_from(tape, sbuf, scalar, b"/x~", table) == (22, 0)
    # a container root and a pointer without its slash
    assert rows_model.walk_from(tape, sbuf, b_cell, b"c", table) == (22, 0)
    assert rows_model.walk_from(tape, sbuf, b_cell, b"", table) == b_cell
