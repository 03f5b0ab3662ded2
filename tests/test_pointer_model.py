"""CPU tier: tests/pointer_model.py -- the plain Python walk the device's columns are compared with -- is pinned twice: cell for cell against
tests/golden/pointers.json (the real reference's dom::parser::parse(document).at_pointer(pointer), tests/golden/make_pointers_golden.py) over the
oracle's tapes, and on random documents against Python's json."""
import json
import struct

import numpy as np
import pytest

import checkers
import pointer_model
import query_cases
import stream_cases


@pytest.fixture(scope="module")
def orc():
    return checkers.Oracle()


def test_fixture_covers_what_it_is_for():
    docs, pointers, cells = query_cases.fixture()
    assert len(docs) >= 60 and len(pointers) >= 60 and len(cells) == len(docs) and all(len(row) == len(pointers) for row in cells)
    flat = [c for row in cells for c in row]
    for code in pointer_model.CODES:
        assert flat.count(f"E {code}") >= 100, code
    for kind in "lud tfn s {[".replace(" ", ""):
        assert any(c[0] == kind for c in flat), kind
    # the rows of the issue's table, by one witness each: (document, pointer) -> cell
    at = {(d, p): cells[i][j] for i, d in enumerate(docs) for j, p in enumerate(pointers)}
    first = b'{"a":1,"b":{"c":[10,20,{"d":"x"}]},"":"empty key","0":"zero","a/b":"slash","m~n":"tilde"}'
    nums = b"[0,1,2,3,4,5,6,7,8,9,10,11]"
    mixed = b'[1,[2,3],{"":"e","k":1},"s",null,true,1.25]'
    assert at[first, b""].startswith("{ ") and at[b"12", b""] == "l 12"
    assert at[first, b"/missing/~2"] == "E 20" and at[first, b"/~2"] == "E 22" and at[first, b"/a~"] == "E 22"
    assert at[first, b"/"] == "s " + b"empty key".hex() and at[first, b"/0"] == "s " + b"zero".hex()
    assert at[first, b"/a~1b"] == "s " + b"slash".hex() and at[first, b"/m~0n"] == "s " + b"tilde".hex()
    assert at[nums, b"/"] == "E 22" and at[nums, b"/-"] == "E 19" and at[nums, b"/-/x"] == "E 17" and at[nums, b"/0x"] == "E 17"
    assert at[nums, b"/01"] == "E 22" and at[nums, b"/00"] == "E 22" and at[nums, b"/12"] == "E 19" and at[nums, b"/11"] == "l 11"
    assert at[nums, b"/99999999999999999999"] == "E 19" and at[nums, b"/18446744073709551616"] == "E 19"
    assert at[mixed, b"/1/"] == "E 22" and at[mixed, b"/2/"] == "s " + b"e".hex()
    assert at[b"12", b"/b~0/c~2"] == "E 20" and at[b"12", b"/~2"] == "E 22" and at[b"12", b"a"] == "E 22" and at[first, b"a"] == "E 22"
    assert at[b'{"ab":"plain first","a\\u0062":"escaped second"}', b"/ab"] == "s " + b"plain first".hex()
    assert at[b'{"a\\u0062":"ab","\\u0061":"a","x\\ny":1,"q\\"r":2,"\\\\":3,"\\/":4}', b"/ab"] == "s " + b"ab".hex()
    assert at[b'{"a\\u0000b":1,"a":2,"\\u0000":3,"a\\u0000":4}', b"/a\x00b"] == "l 1"
    assert at[b'{"a":1,"a":2,"b":{"x":1},"b":{"x":2},"c":[1],"c":{"0":9}}', b"/a"] == "l 1"


def test_model_equals_the_reference_on_the_fixture(orc):
    docs, pointers, cells = query_cases.fixture()
    parsed = []
    for d in docs:
        err, tape, sbuf = orc.dom_parse(d)
        assert err == 0, d
        parsed.append((tape, sbuf))
    # every document alone, and all of them laid out as one stream (absolute offsets)
    for i, (tape, sbuf) in enumerate(parsed):
        for j, p in enumerate(pointers):
            tag, value = pointer_model.walk(tape, sbuf, p)
            assert query_cases.render(tag, value, sbuf) == cells[i][j], (docs[i][:80], p[:40])
    tape, sbuf, table = query_cases.lay_out(parsed)
    tags, values = pointer_model.columns(parsed, pointers)
    for i in range(len(docs)):
        for j in range(len(pointers)):
            assert query_cases.render(tags[j, i], values[j, i], sbuf) == cells[i][j]
    query_cases.check_container_cells(tags, values, tape, table)


def _same(tag, value, sbuf, want):
    """a cell against the Python value json found at the same path"""
    c = chr(tag) if tag >= 34 else None
    if isinstance(want, bool):
        return c == ("t" if want else "f") and value == int(want)
    if want is None:
        return c == "n" and value == 0
    if isinstance(want, int):
        if c == "l":
            return struct.unpack("<q", struct.pack("<Q", value))[0] == want
        return c == "u" and value == want
    if isinstance(want, float):
        return c == "d" and value == struct.unpack("<Q", struct.pack("<d", want))[0]  # bit-equal
    if isinstance(want, str):
        return c == '"' and pointer_model.string_of(sbuf, value) == want.encode()
    return c == ("{" if isinstance(want, dict) else "[")


def _resolve(value, pointer):
    """RFC 6901 over a Python value for pointers made by query_cases.paths_of (well-formed, canonical indices) -> (found, value)"""
    for token in pointer.split(b"/")[1:]:
        if isinstance(value, dict):
            key = token.replace(b"~1", b"/").replace(b"~0", b"~").decode()
            if key not in value:
                return False, None
            value = value[key]
        elif isinstance(value, list):
            if not token.isdigit() or int(token) >= len(value):
                return False, None
            value = value[int(token)]
        else:
            return False, None
    return True, value


def test_model_equals_json_on_random_documents(orc):
    rng = np.random.default_rng(40)
    docs = stream_cases.valid_documents(rng, 500)
    checked = misses = 0
    foreign = []
    for d in docs:
        err, tape, sbuf = orc.dom_parse(d)
        assert err == 0
        value = json.loads(d, object_pairs_hook=query_cases.first_wins)
        own = sorted(set(query_cases.paths_of(value)))
        # every path of the document, and the paths of the document in front of it (mostly absent here)
        for p in own + foreign[:20]:
            found, want = _resolve(value, p)
            tag, cell = pointer_model.walk(tape, sbuf, p)
            if found:
                assert _same(tag, cell, sbuf, want), (d[:120], p, tag, cell)
                checked += 1
            else:
                assert tag in pointer_model.CODES and cell == 0, (d[:120], p, tag)
                misses += 1
        foreign = own
    assert checked > 3000 and misses > 1000, (checked, misses)


def test_the_harvest_is_not_vacuous(orc):
    """the pointers tests/test_gpu_query.py asks of its 2000 random documents: half of them from paths that exist, and the MODEL alone finds at least 30 % hits and
    at least 10 % each of NO_SUCH_FIELD and INDEX_OUT_OF_BOUNDS among the cells"""
    rng = np.random.default_rng(61)
    docs = stream_cases.valid_documents(rng, 2000)
    pointers = query_cases.harvest(docs, 32)
    existing = set()
    for d in docs:
        existing.update(query_cases.paths_of(json.loads(d, object_pairs_hook=query_cases.first_wins)))
    assert len(pointers) == 32 and all(p in existing for p in pointers[:16]) and not any(p in existing for p in pointers[16:])
    assert len(set(pointers[:16])) >= 8  # (the root pointer is repeated, the other paths are not)
    parsed = []
    for d in docs:
        err, tape, sbuf = orc.dom_parse(d)
        assert err == 0
        parsed.append((tape.tolist(), sbuf.tobytes()))
    tags, _ = pointer_model.columns(parsed, pointers)
    hits, nsf, oob = (tags >= 34).mean(), (tags == 20).mean(), (tags == 19).mean()
    assert hits >= 0.30 and nsf >= 0.10 and oob >= 0.10, (hits, nsf, oob)
    assert (tags[16:] < 34).all()
