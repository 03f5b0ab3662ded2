"""CPU tier: tests/json_text_model.py -- the plain Python minify(element) that the texts of sjgpu_serialize_cells_device are compared with -- is pinned against
tests/golden/json_text.json (the real reference: simdjson::minify(e) for the elements of at_path_with_wildcard, and simdjson::internal::to_chars for a table of
doubles, tests/golden/make_json_text_golden.py) over twitter.json, citm_catalog.json and a hand-made document, and against Python's json where the two agree."""
import json
import os

import pytest

import checkers
import json_text_cases
import json_text_model


@pytest.fixture(scope="module")
def orc():
    return checkers.Oracle()


def test_fixture_covers_what_it_is_for():
    docs, cases, doubles = json_text_cases.fixture()
    assert os.path.getsize(json_text_cases.GOLDEN) < 1 << 20 and len(docs) == 3 and {c["document"] for c in cases} == {0, 1, 2}
    paths = {(c["document"], c["path"]) for c in cases}
    assert paths >= {(0, b"$.statuses[*].entities"), (0, b"$.statuses[*].user"), (0, b"$.statuses[*]"), (0, b"$.statuses[*].text"), (0, b"$.statuses[*].id"),
                     (0, b"$.search_metadata"), (0, b"$"), (0, b"$.statuses[*].no_such_field"), (1, b"$.events.*"), (1, b"$.performances[*].seatCategories"), (2, b"$[*]"), (2, b"$")}
    assert any("texts" in c for c in cases) and any("sha256" in c for c in cases) and any(c["cells"] == 0 for c in cases)
    hand = [c for c in cases if (c["document"], c["path"]) == (2, b"$[*]")][0]["texts"]
    for want in (b"{}", b"[]", b'""', b"[[]]", b"[{}]", b'{"":{}}', b'"\\b\\t\\n\\f\\r"', b"-9223372036854775808", b"18446744073709551615", b"9223372036854775808", b"-0.0", b"0.0",
                 b"100.0", b"1.5e-07", b"0.0001", b"1e-05", b"1e+16", b"1e+15", b"999999999999999.0", b"5e-324", b"1.7976931348623157e+308", b"true", b"false", b"null",
                 b'{"k\\u0000z":1,"q\\"uote":"\\\\","a":1,"a":2,"":""}'):
        assert want in hand, want
    controls = [t for t in hand if t.startswith(b'"\\u0000\\u0001')][0]
    assert controls == b'"' + b"".join(json_text_model.ESCAPED[c] for c in range(0x20)) + b'"' and b"\\u001f" in controls and b"\\u000b" in controls
    assert any("\u007f/é😀 plain / text".encode() in t for t in hand)  # DEL, a solidus and the multi-byte characters leave as they are
    table = dict(doubles)
    groups, kept = json_text_cases.double_groups(), json_text_cases.fixture_double_groups()
    assert {name: len(g) for name, g in groups.items()} == {name: d["count"] for name, d in kept.items()} == {
        "powers_of_two": 3 * 2046, "powers_of_ten": 3 * 632, "random": 4000, "subnormal_powers_of_two": 3 * 52 - 4, "tag_lookalikes": 12 * 64}
    assert all({(e << 52) - 1, e << 52, (e << 52) + 1} <= set(groups["powers_of_two"]) for e in (1, 2, 1023, 2046))
    sub = groups["subnormal_powers_of_two"]
    assert sub[:5] == [1, 2, 3, 4, 5] and len(set(sub)) == len(sub) and max(sub) == (1 << 51) + 1 and all({(1 << k) - 1, 1 << k, (1 << k) + 1} <= set(sub) for k in range(1, 52))
    assert [b >> 56 for b in groups["tag_lookalikes"]] == [t for t in json_text_cases.TAPE_TAGS for _ in range(64)] and len(set(groups["tag_lookalikes"])) == 12 * 64
    assert table[0x3FF0000000000000] == b"1.0" and table[1] == b"5e-324" and table[1 << 63] == b"-0.0" and table[0x7FEFFFFFFFFFFFFF] == b"1.7976931348623157e+308"
    assert {len(t.replace(b".", b"").replace(b"-", b"").split(b"e")[0].lstrip(b"0")) for t in table.values()} >= {1, 15, 16, 17}


def test_double_text_equals_the_reference_on_the_fixtures_table():
    _, _, doubles = json_text_cases.fixture()
    for bits, text in doubles:
        assert json_text_model.double_text(bits) == text, hex(bits)
    kept = json_text_cases.fixture_double_groups()
    for name, group in json_text_cases.double_groups().items():
        assert json_text_cases.group_digest([json_text_model.double_text(b) for b in group]) == kept[name]["sha256"], name


def test_model_equals_the_reference_on_the_fixture(orc):
    cells = 0
    for c, (tape, sbuf, table), row in json_text_cases.fixture_rows(orc):
        offsets, chars, status = json_text_model.column(json_text_model.Stream(tape, sbuf, table), row)
        assert not status.any(), (c["document"], c["path"])
        json_text_cases.assert_texts_are_the_fixtures(c, json_text_cases.split(offsets, chars))
        cells += len(row[0])
    assert cells > 900, cells


def test_model_agrees_with_pythons_json_where_both_are_defined(orc):
    """twitter.json and citm_catalog.json hold no double and no control character: json.dumps without blanks and without \\u escapes is the same text"""
    docs, _, _ = json_text_cases.fixture()
    for d in docs[:2]:
        err, tape, sbuf = orc.dom_parse(d)
        assert err == 0
        stream = json_text_cases.stream_of([(tape, sbuf)])
        _, chars, status = json_text_model.column(json_text_model.Stream(*stream), json_text_cases.root_row(*stream))
        assert not status.any() and chars.decode() == json.dumps(json.loads(d), separators=(",", ":"), ensure_ascii=False)


@pytest.mark.parametrize("depth", json_text_cases.DEPTHS)
def test_deep_documents(orc, depth):
    doc = json_text_cases.deep_document(depth)
    err, tape, sbuf = orc.dom_parse(doc, max_depth=json_text_cases.MAX_DEPTH)
    assert err == 0, depth
    stream = json_text_cases.stream_of([(tape, sbuf)])
    _, chars, status = json_text_model.column(json_text_model.Stream(*stream), json_text_cases.root_row(*stream))
    assert not status.any() and chars == doc  # (written without blanks and without escapes: it is its own minified text)
