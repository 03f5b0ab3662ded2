"""CPU tier: tests/path_model.py -- the plain Python recursion the device's ragged columns are compared with -- is pinned twice: cell for cell against
tests/golden/paths.json (the real reference's dom::parser::parse(document).at_path_with_wildcard(path), tests/golden/make_paths_golden.py) over the
oracle's tapes, and on random documents against Python's json."""
import json
import os

import numpy as np
import pytest

import checkers
import path_cases
import path_model
import stream_cases
from test_pointer_model import _same


@pytest.fixture(scope="module")
def orc():
    return checkers.Oracle()


def test_fixture_covers_what_it_is_for():
    docs, paths, cells = path_cases.fixture()
    assert 35 <= len(docs) <= 60 and len(paths) >= 60 and len(cells) == len(docs) and all(len(row) == len(paths) for row in cells)
    assert os.path.getsize(path_cases.GOLDEN) <= os.path.getsize(os.path.join(os.path.dirname(path_cases.GOLDEN), "pointers.json"))
    flat = [c for row in cells for c in row]
    for code in (17, 19, 20, 22):
        assert flat.count(f"E {code}") >= 5, code
    assert flat.count("M") >= 500 and sum(1 for c in flat if c.count(";") >= 2) >= 100
    at = {(d, p): cells[i][j] for i, d in enumerate(docs) for j, p in enumerate(paths)}
    A = b'{"a":[{"b":1,"c":[1,2]},{"b":2},{"x":3},5],"k":{"p":{"b":7},"q":{"b":8}},"s*":1,"e":[],"o":{}}'
    B = b'[[1,2],[3],{"b":[4]},6]'
    # the table of the issue, row by row
    assert at[A, b"$.a[*].b"] == "M;l 1;l 2" and at[A, b"$.k.*.b"] == at[A, b"$.k[*].b"] == "M;l 7;l 8" and at[A, b"$.a[*].c[*]"] == "M;l 1;l 2"
    assert at[A, b"$.*.*"].count(";") == 6 and at[A, b"$.a[*].c[0]"] == "M;l 1" and at[A, b"$.a.1.*"] == at[A, b"$.a/1.*"] == "M;l 2"
    assert at[A, b".a[*].b"] == "M;l 1;l 2" and at[A, b"$.a[0].b"] == "M;l 1" and at[A, b"$.a[0].c[*]"] == "M" and at[A, b"$.s*"] == "M"
    for p in (b"$.a[*]['b']", b"$['a'][*]['b']", b"$.a[*]x", b"$.a[*", b"$.a[*].b.z", b"$.missing[*]", b"$.e[*]", b"$.o.*"):
        assert at[A, p] == "M", p
    assert at[A, b"$.missing"] == "E 20" and at[B, b"$.missing"] == "E 17" and at[A, b"$..b"] == "E 20" and at[B, b"$..b"] == "E 22"
    for p in (b"$[0][*]", b"$[2].b[*]", b"a[*]", b"", b"$"):
        assert at[A, p] == at[B, p] == "E 22", p
    assert at[B, b"$[*][*]"] == "M;l 1;l 2;l 3;[ 4" and at[B, b"$[*][0]"] == "M;l 1;l 3" and at[B, b"$[*].b[*]"] == "M;l 4"
    # a scalar root: status 0 and nothing, even for the empty path
    for root in (b"12", b'"str"', b"null"):
        assert all(at[root, p] == "M" for p in paths)
    # eight nested wildcards reach the ninth level
    deep = b"[" * 8 + b"[1,2],[3]" + b"]" * 8
    assert at[deep, b"$[*][*][*][*][*][*][*][*]"] == "M;[ 6;[ 4"
    # a number whose value word looks like a tape word, as a match
    assert at[b'[8863084066665136133,"x",{"k":1}]', b"$[*]"] == "M;l 8863084066665136133;s 78;{ 5"


def test_model_equals_the_reference_on_the_fixture(orc):
    docs, paths, cells = path_cases.fixture()
    parsed = []
    for d in docs:
        err, tape, sbuf = orc.dom_parse(d)
        assert err == 0, d
        parsed.append((tape.tolist(), sbuf.tobytes()))
    for i, (tape, sbuf) in enumerate(parsed):  # every document alone
        for j, p in enumerate(paths):
            status, found = path_model.matches(tape, sbuf, p)
            assert path_cases.render(status, found, sbuf) == cells[i][j], (docs[i][:80], p[:40])
    sbuf = b"".join(s for _, s in parsed)  # ... and all of them laid out as one stream (absolute offsets)
    status, offsets, tags, values = path_model.column(parsed, paths)
    for i in range(len(docs)):
        for j in range(len(paths)):
            assert path_cases.render(*path_cases.cell(status, offsets, tags, values, j, i, len(docs)), sbuf) == cells[i][j]
    tape = np.concatenate([np.array(t, np.uint64) for t, _ in parsed])
    path_cases.check_container_matches(np.array(tags, np.uint8), np.array(values, np.uint64), tape)


class Fields(list):
    """an object as json found it: every (key, value), duplicates included -- what get_values walks"""


def test_model_equals_json_on_random_documents(orc):
    rng = np.random.default_rng(41)
    docs = stream_cases.valid_documents(rng, 800)
    checked = 0

    def kids(v):
        return [x for _, x in v] if isinstance(v, Fields) else (v if isinstance(v, list) else [])

    def same(found, want, sbuf):
        assert len(found) == len(want)
        for (tag, value), w in zip(found, want):
            assert _same(tag, value, sbuf, {} if isinstance(w, Fields) else w), (tag, value, w)
        return len(found)
    for d in docs:
        err, tape, sbuf = orc.dom_parse(d)
        assert err == 0
        tape, sbuf = tape.tolist(), sbuf.tobytes()
        value = json.loads(d, object_pairs_hook=Fields)
        level1 = kids(value)
        level2 = [x for v in level1 for x in kids(v)]
        for path in (b"$[*]", b"$.*"):
            status, found = path_model.matches(tape, sbuf, path)
            assert status == 0
            checked += same(found, level1, sbuf)
        status, found = path_model.matches(tape, sbuf, b"$.*.*")
        assert status == 0
        checked += same(found, level2, sbuf)
        assert path_model.matches(tape, sbuf, b"$[*][*]") == (status, found)
    assert checked > 3000, checked


def test_the_small_records_are_not_vacuous(orc):
    """the condition tests/test_paths_emu.py and tests/test_gpu_paths.py rest on, on the MODEL alone: the generator draws six kinds of record uniformly, so
    `$.tags[*]`, `$.f[*]` and `$.a.b.c[*].d` match in 1/6 of the documents each and `$[*]` in 5/6"""
    docs = stream_cases.small_records(np.random.default_rng(51), 6000)
    parsed = []
    for d in docs:
        err, tape, sbuf = orc.dom_parse(d)
        assert err == 0
        parsed.append((tape.tolist(), sbuf.tobytes()))
    status, offsets, _, _ = path_cases.model_column(parsed, path_cases.SMALL_RECORD_PATHS)
    share = (np.diff(offsets.astype(np.int64)).reshape(len(path_cases.SMALL_RECORD_PATHS), len(docs)) > 0).mean(axis=1)
    assert (np.delete(status, 7, axis=0) == 0).all()  # only `$.name`, the path without a wildcard, can be an error: 17 for an array root, 20 for an object without it
    assert set(status[7].tolist()) == {0, 17, 20}
    assert share[0] > 0.10 and share[1] > 0.10 and share[5] > 0.10 and share[3] > 0.50, share
