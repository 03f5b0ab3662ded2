"""CPU tier: tests/cast_model.py -- the numpy model of sjgpu_cast_cells_device and sjgpu_cell_kinds_device that the emulated and the real kernels are compared
with -- is pinned answer for answer against tests/golden/casts.json (the real reference, asked parse(`[X]`).at_pointer(p).get_int64() and its six siblings,
tests/golden/make_casts_golden.py).  The cells are tests/pointer_model.py's over tapes the oracle built.  The getter a loader infers from a census is checked
by hand-written rows, the model's and capi.infer_getters alike."""
import json
import os

import numpy as np
import pytest

import cast_model
import checkers
import pointer_model
from simdjson_amd import _paths, capi

GOLDEN = os.path.join(_paths.REPO_ROOT, "tests", "golden", "casts.json")
REQUIRED = [b"0", b"-1", b"9223372036854775807", b"9223372036854775808", b"9223372036854775809", b"18446744073709551615", b"18446744073709551616",
            b"-9223372036854775808", b"9007199254740992", b"9007199254740993", b"-9007199254740993", b"18446744073709549568", b"18446744073709550591",
            b"18446744073709550592", b"1e19", b"-0.0", b"1.5", b"5e-324", b"1.7976931348623157e308", b"true", b"false", b"null", b'""', b'"abc"', b"[]", b"{}",
            b"[1]", b'{"a":1}']


def fixture():
    """-> (values, pointers, table): table[value] is "P <code>" or, per pointer, the seven answers"""
    g = json.load(open(GOLDEN))
    assert g["getters"] == cast_model.GETTER_NAMES
    table = [t if isinstance(t, str) else [g["rows"][r].split(";") for r in t] for t in g["table"]]
    return [bytes.fromhex(x) for x in g["values"]], [bytes.fromhex(p) for p in g["pointers"]], table


def fixture_cells(orc):
    """every (value, pointer) of the fixture the reference parsed, as ONE row of cells -> (tags uint8[n], words uint64[n], answers[n][7], string buffers[n])"""
    values, pointers, table = fixture()
    tags, words, answers, sbufs = [], [], [], []
    for x, per_pointer in zip(values, table):
        err, tape, sbuf = orc.dom_parse(b"[" + x + b"]")
        if isinstance(per_pointer, str):
            assert err != 0, x  # the oracle rejects what the reference rejects
            continue
        assert err == 0, x
        for p, seven in zip(pointers, per_pointer):
            t, w = pointer_model.walk(tape, sbuf, p)
            tags.append(t)
            words.append(w)
            answers.append(seven)
            sbufs.append(sbuf)
    return np.array(tags, np.uint8), np.array(words, np.uint64), answers, sbufs


@pytest.fixture(scope="module")
def orc():
    return checkers.Oracle()


def test_fixture_covers_what_it_is_for():
    values, pointers, table = fixture()
    assert set(REQUIRED) <= set(values) and pointers == [b"/0", b"/1", b"/0/x", b"/~", b"x"]
    assert os.path.getsize(GOLDEN) < 8192
    flat = [a for t in table if not isinstance(t, str) for seven in t for a in seven]
    for code in (17, 18, 19, 20, 22):
        assert flat.count(f"E {code}") >= 7, code
    assert table[values.index(b"18446744073709551616")][:2] == "P "  # beyond 64 bits: no element to ask
    first = {x: t[0] for x, t in zip(values, table) if not isinstance(t, str)}
    # the rules the header states, as the reference answered them
    assert first[b"9223372036854775808"][:2] == ["E 18", "8000000000000000"] and first[b"-1"][:2] == ["ffffffffffffffff", "E 18"]
    assert first[b"9007199254740993"][2] == "4340000000000000" and first[b"18446744073709550591"][2] == "43efffffffffffff"
    assert first[b"18446744073709550592"][2] == first[b"18446744073709551615"][2] == "43f0000000000000"
    assert first[b"null"] == ["E 17"] * 7 and first[b"true"][3] == "0000000000000001" and first[b'"abc"'][4] == "S 616263"
    # a failed result answers every getter with its own code
    for t in table:
        if not isinstance(t, str):
            assert t[1] == ["E 19"] * 7 and t[4] == ["E 22"] * 7
    assert table[values.index(b"{}")][2] == ["E 20"] * 7


def test_model_equals_the_reference_on_the_fixture(orc):
    tags, words, answers, sbufs = fixture_cells(orc)
    n = len(tags)
    assert n == 27 * 5 and set(b'{["ludtfn') | {17, 19, 20, 22} <= set(tags.tolist())
    getters = list(range(1, 8))
    value_out, code, valid, counts = cast_model.cast(np.tile(tags, (7, 1)), np.tile(words, (7, 1)), getters)
    for k, g in enumerate(getters):
        for i in range(n):
            a = answers[i][k]
            where = (cast_model.GETTER_NAMES[k], i, a)
            if a.startswith("E "):
                assert code[k, i] == int(a[2:]) and value_out[k, i] == 0, where
                continue
            assert code[k, i] == 0, where
            if a.startswith("S "):
                assert pointer_model.string_of(sbufs[i], int(value_out[k, i])).hex() == a[2:], where
            elif a[0] in "AO":
                assert value_out[k, i] == words[i] and tags[i] == ord("[" if a[0] == "A" else "{"), where
            else:
                assert int(value_out[k, i]) == int(a, 16), where
        assert counts[k].tolist() == [sum(1 for i in range(n) if not answers[i][k].startswith("E ")), int((tags == ord("n")).sum()),
                                      sum(1 for i in range(n) if answers[i][k] == "E 18"), int((tags < 34).sum())]
        bits = np.unpackbits(valid[k].view(np.uint8), bitorder="little")
        assert bits[:n].tolist() == [int(not answers[i][k].startswith("E ")) for i in range(n)] and not bits[n:].any()
    census = cast_model.kinds(tags[None, :], words[None, :])[0]
    assert census[:9].tolist() == [int((tags == c).sum()) for c in b'{["ludtfn'] and census[9] == 3  # -1, INT64_MIN, -9007199254740993
    assert census[10:].tolist() == [int((tags == c).sum()) for c in (17, 19, 20, 22)] + [0, 0] and int(census.sum()) - 3 == n


def test_bytes_that_are_no_tags_and_held_codes():
    """all 256 tag bytes under every getter: 1 .. 33 forwarded, 0 and every other byte that is no tag 17"""
    tags = np.arange(256, dtype=np.uint8)
    words = np.full(256, 5, np.uint64)
    for g in range(1, 8):
        value_out, code = cast_model.cast_row(tags, words, g)
        for t in range(256):
            if 1 <= t <= 33:
                assert code[t] == t and value_out[t] == 0
            elif chr(t) not in '{["ludtfn':
                assert code[t] == 17 and value_out[t] == 0
        assert code[ord("Z")] == code[ord("r")] == code[ord("}")] == code[ord("]")] == code[0] == 17
    census = cast_model.kinds(tags[None, :], words[None, :])[0]
    assert census.tolist() == [1] * 9 + [0] + [1] * 4 + [256 - 13, 0]


def row(**counts):
    slots = {"obj": 0, "arr": 1, "str": 2, "l": 3, "u": 4, "d": 5, "t": 6, "f": 7, "n": 8, "neg": 9, "e17": 10, "e19": 11, "e20": 12, "e22": 13, "other": 14}
    r = [0] * 16
    for name, c in counts.items():
        r[slots[name]] = c
    return r


INFER_ROWS = [
    (row(t=3, f=2), cast_model.BOOL), (row(t=1, n=9, e20=4), cast_model.BOOL), (row(str=7), cast_model.STRING), (row(str=7, n=1, e17=1), cast_model.STRING),
    (row(arr=2), cast_model.ARRAY), (row(obj=2, e19=1, e22=1), cast_model.OBJECT),
    (row(l=5), cast_model.INT64), (row(l=5, neg=5), cast_model.INT64), (row(l=5, neg=2, n=3), cast_model.INT64),
    (row(l=5, d=1), cast_model.DOUBLE), (row(d=4), cast_model.DOUBLE), (row(u=1, d=1, l=1, neg=1), cast_model.DOUBLE),
    (row(u=2), cast_model.UINT64), (row(u=2, l=3), cast_model.UINT64), (row(u=2, l=3, neg=1), cast_model.DOUBLE),  # (the last one lossy, as get_double is)
    (row(), 0), (row(n=4, e20=2), 0), (row(l=1, str=1), 0), (row(t=1, l=1), 0), (row(arr=1, obj=1), 0), (row(l=3, other=1), 0), (row(other=2), 0),
    (row(str=1, t=1), 0), (row(d=1, arr=1), 0),
]


def test_infer_getters_by_hand_written_rows():
    for infer in (cast_model.infer_getters, capi.infer_getters):
        assert infer(np.array([r for r, _ in INFER_ROWS], np.uint32)) == [g for _, g in INFER_ROWS]
        assert infer(np.zeros((0, 16), np.uint32)) == []
    assert (capi.GET_INT64, capi.GET_UINT64, capi.GET_DOUBLE, capi.GET_BOOL, capi.GET_STRING, capi.GET_ARRAY, capi.GET_OBJECT) == (1, 2, 3, 4, 5, 6, 7)
