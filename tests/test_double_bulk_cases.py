"""CPU tier: tests/double_bulk_cases.py -- what tests/test_gpu_doubles.py expects of every printer and parser of doubles on the device -- is pinned here first: each
group's texts against the digests tests/golden/json_text.json holds from the real reference, the documents made of them against the oracle's parse (pinned against
the reference on this tier), and the spread of the texts' lengths."""
import numpy as np
import pytest

import checkers
import double_bulk_cases as B
import json_text_cases

SHORTEST, LONGEST = 3, 24  # "1.0"; "-1.2345678901234567e-308": a sign, 17 digits, the point, e, the exponent's sign and three digits


@pytest.fixture(scope="module")
def orc():
    return checkers.Oracle()


def test_the_groups_are_the_fixtures():
    kept = json_text_cases.fixture_double_groups()
    assert list(kept) == B.GROUPS == list(json_text_cases.double_groups())
    for name in B.GROUPS:
        g = B.group(name)
        assert g.n == kept[name]["count"] == len(g.texts) and json_text_cases.group_digest(g.texts) == kept[name]["sha256"], name
        assert not any((b >> 52) & 0x7FF == 0x7FF for b in g.bits), name
    for name in B.SIGNED_GROUPS:
        g, plain = B.group(name, negated=True), B.group(name)
        assert g.bits == [b | B.SIGN for b in plain.bits] and g.texts == [b"-" + t for t in plain.texts] and g.bits != plain.bits
    assert set(B.LANE_PER_WORD_GROUPS) <= set(B.GROUPS) and set(B.SIGNED_GROUPS) <= set(B.GROUPS)


@pytest.mark.parametrize("negated", [False, True], ids=["as they are", "negated"])
@pytest.mark.parametrize("name", B.GROUPS)
def test_the_oracle_parses_every_document_back_to_the_bits(orc, name, negated):
    if negated and name not in B.SIGNED_GROUPS:
        return
    g = B.group(name, negated)
    err, tape, sbuf = orc.dom_parse(g.array)
    assert err == 0 and len(sbuf) == 0 and np.array_equal(tape, g.array_tape())
    tags = (tape >> np.uint64(56)).astype(np.uint8)
    assert chr(tags[1]) == "[" and chr(tags[-2]) == "]" and (tags[2:-2:2] == ord("d")).all() and tape[3:-2:2].tolist() == g.bits  # (said once more without the builder)
    singles = g.scalar_tapes().reshape(g.n, 4)
    for text, want in zip(g.texts, singles):
        err, tape, _ = orc.dom_parse(text)
        assert err == 0 and np.array_equal(tape, want), text
    err, tape, sbuf = orc.dom_parse(g.quoted)
    assert err == 0 and len(tape) == g.n + 4 and ((tape[2:-2] >> np.uint64(56)) == 0x22).all()
    records = sbuf.tobytes()
    at = 0
    for t in g.texts:  # a string record: its length in four bytes, the bytes, a NUL
        assert records[at: at + 4] == len(t).to_bytes(4, "little") and records[at + 4: at + 4 + len(t)] == t
        at += 4 + len(t) + 1
    assert at == len(records)
    err, tape, sbuf = orc.dom_parse(g.object)
    assert err == 0 and len(tape) == 3 * g.n + 4 and tape[4:-2:3].tolist() == g.bits and ((tape[3:-2:3] >> np.uint64(56)) == ord("d")).all()
    for prefix in B.INTEGER_PREFIXES + B.LITERAL_PREFIXES:
        err, tape, _ = orc.dom_parse(B.array_document(g.texts[:50], prefix))
        words = len(prefix) * (2 if prefix[0] == b"7" else 1)
        assert err == 0 and tape[2 + words + 1: -2: 2].tolist() == g.bits[:50]


def test_the_documents_are_what_they_say():
    g = B.group("subnormal_powers_of_two")
    assert g.texts[:3] == [b"5e-324", b"1e-323", b"1.5e-323"] and g.array.startswith(b"[5e-324,1e-323,1.5e-323,") and g.ndjson.startswith(b"5e-324\n1e-323\n")
    assert g.quoted.startswith(b'["5e-324","1e-323",') and g.object.startswith(b'{"k0":5e-324,"k1":1e-323,') and g.pretty.startswith(b"[\n    5e-324,\n    1e-323,\n")
    assert g.pretty.endswith(b"e-308\n]\n") and g.pretty.count(b"\n") == g.n + 2 and g.loose_pretty == g.ndjson
    assert B.pretty_array([b"1.0"], [b"7", b"-8"]) == b"[\n    7,\n    -8,\n    1.0\n]\n" and B.array_document([b"1.0"], [b"null"]) == b"[null,1.0]"
    tags, values = g.cells()
    assert tags.tolist() == [ord("d")] * g.n and values.tolist() == g.bits
    assert [len(p) for p in B.INTEGER_PREFIXES] == [len(p) for p in B.LITERAL_PREFIXES] == [1, 2, 3]


def test_every_length_a_text_can_have_occurs():
    """No text of a double is shorter than three characters -- a digit, the point, a digit; the shortest with an exponent, 1e+16, has five --, so the lengths 1 and 2
    cannot occur and are not asked for.  The longest is measured: over the groups, whose texts are the reference's by their digests, and over the fixture's table."""
    lengths = {len(t) for name in B.GROUPS for t in B.group(name).texts}
    _, _, table = json_text_cases.fixture()
    print("lengths of the groups' texts:", sorted(lengths), "the longest of the fixture's table:", max(len(t) for _, t in table))
    assert min(lengths) == SHORTEST and max(lengths) == LONGEST >= max(len(t) for _, t in table)
    assert lengths == set(range(SHORTEST, LONGEST + 1))
    by_group = {name: {len(t) for t in B.group(name).texts} for name in B.GROUPS}
    assert max(by_group["random"]) == LONGEST and min(by_group["powers_of_two"]) == SHORTEST
