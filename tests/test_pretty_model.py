"""CPU tier: tests/pretty_model.py -- the plain Python prettify(element) that the texts of sjgpu_prettify_cells_device and sjgpu_prettify_cells_wide_device are compared
with -- is pinned against tests/golden/pretty.json (the real reference: simdjson::prettify(e) for the elements of at_path_with_wildcard,
tests/golden/make_pretty_golden.py) over twitter.json, citm_catalog.json, the hand-made document of the minify fixture and 96 chains (one column per level) whose leaf lies on either side of
the 16th, 32nd, ... level; against Python's json where the two agree; and against the minify model: an indented text without its layout is the minified text."""
import json
import os

import pytest

import checkers
import json_text_cases
import json_text_model
import pretty_cases
import pretty_model


@pytest.fixture(scope="module")
def orc():
    return checkers.Oracle()


def test_fixture_covers_what_it_is_for():
    docs, cases = pretty_cases.fixture()
    text_docs, text_cases, _ = json_text_cases.fixture()
    assert os.path.getsize(pretty_cases.GOLDEN) < 1 << 20 and docs[:3] == text_docs and docs[3:] == pretty_cases.chain_documents()
    assert [(c["document"], c["path"], c["cells"]) for c in cases[:14]] == [(c["document"], c["path"], c["cells"]) for c in text_cases]  # the same three documents, the same cases
    assert [(c["document"], c["path"], c["cells"]) for c in cases[14:]] == [(d, b"$[*]", 12) for d in range(3, len(docs))]  # a level's twelve chains, each a cell
    assert any("texts" in c for c in cases) and any("sha256" in c for c in cases) and any(c["cells"] == 0 for c in cases)
    assert len(pretty_cases.chains()) == 8 * 6 * 2 and pretty_cases.CHAIN_LEVELS == [14, 15, 16, 17, 31, 32, 33, 65]
    hand = [c for c in cases if (c["document"], c["path"]) == (2, b"$[*]")][0]["texts"]
    for want in (b"{}\n", b"[]\n", b'""\n', b"[\n    []\n]\n", b'{\n    "": {}\n}\n', b"-0.0\n", b"true\n", b"null\n"):
        assert want in hand, want


def test_model_equals_the_reference_on_the_fixture(orc):
    cells = 0
    for c, (tape, sbuf, table), row in pretty_cases.fixture_rows(orc):
        offsets, chars, status = pretty_model.column(pretty_model.Stream(tape, sbuf, table), row)
        assert not status.any(), (c["document"], c["path"])
        pretty_cases.assert_texts_are_the_fixtures(c, json_text_cases.split(offsets, chars))
        cells += len(row[0])
    assert cells > 900 + 96, cells


def test_what_the_chains_are_for(orc):
    """the model's texts of the chains -- the fixture's, by its digests (above) -- show the container of the 16th level, once an array and once an object of two keys:
    flat, its children from indent 0 and each with a newline of its own"""
    keys = [(lv, lf, ph) for lv in pretty_cases.CHAIN_LEVELS for lf in pretty_cases.CHAIN_LEAVES for ph in pretty_cases.CHAIN_PHASES]
    parsed = [orc.dom_parse(d)[1:] for d in pretty_cases.chains()]
    stream = json_text_cases.stream_of(parsed)
    offsets, chars, status = pretty_model.column(pretty_model.Stream(*stream), json_text_cases.root_row(*stream))
    by_chain = dict(zip(keys, json_text_cases.split(offsets, chars)))
    assert not status.any()
    assert b'\n' + b" " * 60 + b'"k": [1\n,7\n],\n' in by_chain[(16, b"7", 1)] and b'\n' + b" " * 60 + b'{"k":7\n,"z":0\n}\n' + b" " * 56 + b"]" in by_chain[(16, b"7", 0)]
    assert b'{"k":[]\n,"z":0\n}' in by_chain[(16, b"[]", 0)] and b"[1\n,{}\n]" in by_chain[(16, b"{}", 1)]  # an empty container inside a flat one
    assert b'[1\n,[\n    1,\n    [\n        2\n    ],\n    {},\n    "x"\n]\n]' in by_chain[(16, b'[1,[2],{},"x"]', 1)]  # ... and one that has children: afresh
    assert by_chain[(15, b"[]", 1)].count(b"[]") == 1 and b"[1,\n" not in by_chain[(14, b"7", 0)]  # at the 15th level nothing is flat yet
    assert all(b" " * 61 not in t for t in by_chain.values()) and all(t.endswith(b"\n") for t in by_chain.values())


def test_model_agrees_with_pythons_json_where_both_are_defined(orc):
    """twitter.json and citm_catalog.json hold no double, no control character, no empty container below 16 levels... but they do hold empty containers, which
    json.dumps(indent=4) writes as [] and {} too: the same text, and a newline"""
    docs, _ = pretty_cases.fixture()
    for d in docs[:2]:
        err, tape, sbuf = orc.dom_parse(d)
        assert err == 0
        stream = json_text_cases.stream_of([(tape, sbuf)])
        _, chars, status = pretty_model.column(pretty_model.Stream(*stream), json_text_cases.root_row(*stream))
        assert not status.any() and chars.decode() == json.dumps(json.loads(d), indent=4, ensure_ascii=False) + "\n"


def test_a_text_parsed_again_is_the_value_of_the_minified_text(orc):
    """every chain, every deep document: the layout adds blanks and newlines between tokens and nothing else"""
    documents = pretty_cases.chains() + [json_text_cases.deep_document(d) for d in json_text_cases.DEPTHS] + [pretty_cases.flat_container_of(40), pretty_cases.flat_container_of(40, True)]
    for doc in documents:
        err, tape, sbuf = orc.dom_parse(doc, max_depth=json_text_cases.MAX_DEPTH)
        assert err == 0
        stream = json_text_cases.stream_of([(tape, sbuf)])
        root = json_text_cases.root_row(*stream)
        _, pretty, status = pretty_model.column(pretty_model.Stream(*stream), root)
        _, plain, _ = json_text_model.column(json_text_model.Stream(*stream), root)
        assert not status.any() and plain == doc and pretty.endswith(b"\n")
        assert b"".join(pretty.split()) == b"".join(plain.split())  # (no string of these documents holds a blank)
