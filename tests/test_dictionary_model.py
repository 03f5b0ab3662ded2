"""CPU tier: tests/dictionary_model.py -- the plain Python `dict` that the codes and dictionaries of sjgpu_dictionary_encode_device and the censuses of
sjgpu_cell_kinds_by_code_device are compared with -- is pinned against tests/golden/dictionary.json (the real reference: get_string() / key_value_pair::key entered
into a std::unordered_map<std::string_view, ...> in the order met, tests/golden/make_dictionary_golden.py) over twitter.json, citm_catalog.json and a hand-made
document, and the fixture against the counts Python's json gives for twitter.json."""
import json
import os

import numpy as np
import pytest

import checkers
import dictionary_cases
import dictionary_model
from dictionary_cases import KEYS, VALUES


@pytest.fixture(scope="module")
def orc():
    return checkers.Oracle()


def case_of(cases, document, mode, path):
    found, = [c for c in cases if (c["document"], c["mode"], c["path"]) == (document, mode, path)]
    return found


def test_fixture_covers_what_it_is_for():
    docs, cases = dictionary_cases.fixture()
    assert os.path.getsize(dictionary_cases.GOLDEN) < 1 << 18 and len(docs) == 3 and {c["document"] for c in cases} == {0, 1, 2}
    lang = case_of(cases, 0, VALUES, b"$.statuses[*].lang")
    assert (lang["strings"], lang["counts"], lang["first"][0], lang["nulls"]) == ([b"ja", b"zh"], [96, 4], 0, 0)
    assert case_of(cases, 0, VALUES, b"$.statuses[*].user.lang")["strings"] == [b"en", b"ja", b"it", b"es", b"zh-cn"]
    zone = case_of(cases, 0, VALUES, b"$.statuses[*].user.time_zone")
    assert (zone["nulls"], len(zone["strings"]), zone["cells"]) == (81, 7, 100)
    users, statuses = case_of(cases, 0, KEYS, b"$.statuses[*].user"), case_of(cases, 0, KEYS, b"$.statuses[*]")
    assert (len(users["strings"]), users["cells"]) == (40, 3986) and (len(statuses["strings"]), statuses["cells"]) == (25, 2388)
    # the same from Python's json and a dict
    tw = json.loads(docs[0])
    seen = {}
    for s in tw["statuses"]:
        for k in s["user"]:
            seen[k] = seen.get(k, 0) + 1
    assert [k.encode() for k in seen] == users["strings"] and list(seen.values()) == users["counts"]
    # the hand-made document: what the contract says about equality
    hand = case_of(cases, 2, VALUES, b"$[*]")
    S = hand["strings"]
    assert S[:5] == [b"a\x00b", b"a", b"a\x00", b"A", b""] and S.count(b"A") == 1 and hand["counts"][S.index(b"A")] == 3  # "A", "A" and "A" again
    assert hand["counts"][S.index(b"")] == 2 and hand["counts"][S.index(b"a\x00b")] == 2 and hand["nulls"] == 11
    assert {len(s) for s in S} >= {0, 1, 2, 3, 7, 8, 9, 15, 16, 17, 299, 300} and b"x" * 299 + b"y" in S and b"x" * 299 + b"z" in S and b"x" * 299 in S
    assert S.count("é".encode()) == 1 and hand["counts"][S.index("é".encode())] == 2 and hand["counts"][S.index(b"line\nfeed")] == 2
    keys = case_of(cases, 2, KEYS, b"$[*]")
    assert keys["strings"] == [b"k", b"", b"a\x00b", b"A", b"a", b"a\x00", b"only"] and keys["counts"] == [1, 2, 2, 3, 5, 1, 1]
    assert keys["counts"][keys["strings"].index(b"a")] == 5  # duplicate keys of one object are fields like any other
    assert any(len(c["strings"]) == 1 and c["cells"] > 200 for c in cases) and any(len(c["strings"]) == c["cells"] > 100 for c in cases)  # one value; all distinct
    assert any(c["cells"] == 0 for c in cases) and any(c["nulls"] == c["cells"] > 0 for c in cases)


def test_model_equals_the_reference_on_the_fixture(orc):
    cells = 0
    for c, sbuf, (tags, values), (vtags, vvalues) in dictionary_cases.fixture_rows(orc):
        what = (c["document"], c["mode"], c["path"])
        codes, first, dict_values, counts = dictionary_model.encode(tags, values, sbuf)
        assert len(tags) == c["cells"] and codes.tolist() == c["codes"], what
        assert first.tolist() == c["first"] and counts.tolist() == c["counts"], what
        assert [dictionary_model.string_of(sbuf, ord('"'), v) for v in dict_values.tolist()] == c["strings"] == dictionary_model.strings(tags, values, sbuf), what
        kinds = dictionary_model.kinds_by_code(codes, vtags, vvalues, len(first))
        assert kinds[:, :10].tolist() == c["kinds"] and not kinds[:, 10:].any(), what
        cells += len(tags)
    assert cells > 13000, cells  # (what the fixture holds: 13 899)


def test_census_by_code_law_and_edges():
    """the rows of the census by code sum to the census of the cells that have a code inside the groups; codes outside count nowhere"""
    rng = np.random.default_rng(7)
    n = 5000
    tags = rng.choice(np.frombuffer(b'{["ludtfn\x11\x13\x14\x16\x00Z', np.uint8), n)
    values = rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2)
    codes = rng.integers(-3, 50, n).astype(np.int32)
    for groups in (0, 1, 40, 47, 60):
        got = dictionary_model.kinds_by_code(codes, tags, values, groups)
        inside = (codes >= 0) & (codes < groups)
        want = dictionary_model.cast_model.kinds(tags[inside][None, :], values[inside][None, :])[0]
        assert got.shape == (groups, 16) and np.array_equal(got.sum(axis=0, dtype=np.uint64), want if groups else np.zeros(16))
