"""Shared by the tests of the nested writer (tests/test_nested_write_model.py, tests/test_nested_emu.py, tests/test_gpu_nested.py) and by the generator of their
fixture (tests/golden/make_nested_write_golden.py): the tables tests/golden/nested_write.json holds the reference's texts for, defined once, here; how a table becomes
the arrays sjgpu_write_nested_device reads; and the tables made by rule for the edges of its kernels.

A TABLE is {"name", "n", "fields": [field]}: a field is a column of tests/write_records_cases.py ({"key", "kind", "cells"}) or a LIST field {"key", "kind",
"lists": [None | [element, ...]] * n} -- None an invalid list, an element None (its validity bit is 0), an int (kinds 1 .. 4) or bytes (5, 9: a string; 8: a JSON text).
Its ARRAYS are {"n", "fields": [a column's arrays (over the ELEMENTS for a list field) + "list_offsets": uint32[n + 1] | None, "list_valid": uint64[ceil(n / 64)] |
None, "elements": int]} -- what the model, the emulation's driver and the device take."""
import hashlib
import json
import os
import struct

import numpy as np

import json_text_cases
import write_records_cases as plain
from simdjson_amd import _paths
from write_records_cases import BOOL, DOUBLE, INT64, JSON, NEWLINE, OMIT_NULLS, STRING, STRING_CELLS, UINT64, bits_of, column  # noqa: F401

GOLDEN = os.path.join(_paths.REPO_ROOT, "tests", "golden", "nested_write.json")
ARRAY_ROWS, BARE = 4, 8
SMALL = 3 << 10
LIST_LENGTHS = [0, 1, 2, 63, 64, 65]
GARBAGE = 0xFFFFFFF0  # the list offset between two invalid lists: nobody reads it


def legal_flags(K):
    """every legal combination of the four flags for a table of K fields"""
    return [0, 1, 2, 3, ARRAY_ROWS, ARRAY_ROWS | NEWLINE] + ([BARE, BARE | OMIT_NULLS, BARE | NEWLINE, BARE | OMIT_NULLS | NEWLINE] if K == 1 else [])


def list_field(key, kind, lists):
    return {"key": bytes(key), "kind": kind, "lists": [None if x is None else list(x) for x in lists]}


def is_list(f):
    return "lists" in f


# ---- the tables of the fixture ------------------------------------------------------------------------------------------------------------------------------
def _every_kind():
    """a list field of every element kind beside a plain one of every other row; empty lists, invalid lists, invalid elements at the ends and in the middle"""
    n = 6
    return {"name": "every_kind", "n": n, "fields": [
        column(b"id", INT64, [0, None, 2, 3, (1 << 64) - 4, 5]),
        list_field(b"i", INT64, [[1, None, (1 << 64) - 3], [], None, [None], [0], [None, 7, None]]),
        list_field(b"u", UINT64, [[], [1, 2], [None, (1 << 64) - 1], None, None, [3]]),
        list_field(b"d", DOUBLE, [[bits_of(1.0), bits_of(-0.0), bits_of(1e300)], None, [], [None, bits_of(0.1)], [bits_of(-2.5e-7)], [bits_of(1e21), None]]),
        list_field(b"b", BOOL, [[0, 1, 2], [None], [], None, [1 << 63, None], [0]]),
        list_field(b's"', STRING, [[b"", b'q"uote', None], [b"back\\slash", b"\n"], None, [], ["é€".encode()], [b"0123456789abcdef", None, b"\x00\x1f"]]),
        list_field(b"c", STRING_CELLS, [[b"cell"], None, [None, b"", b"tab\there"], [b"x", b"/"], [], [b"\x7f"]]),
        list_field(b"j", JSON, [[b'{"a":[1,2,{"b":null}]}', b"", b"7"], [], [None, b'"s"'], None, [b"null", b"[true,false]"], [b"{}"]]),
        column(b"name", STRING, [b"a", b"b", None, b"d", b"e", b"f"])]}


def _lengths():
    """lists of 0, 1, 2, 63, 64 and 65 elements under every shape of element validity -- all valid (no validity words), none, alternating, only the word's edges --
    with two invalid lists in a row, so that an offset nobody may read lies between them"""
    rows = LIST_LENGTHS + [None, None, 3]
    def lists(shape):
        out, at = [], 0
        for m in rows:
            if m is None:
                out.append(None)
                continue
            out.append([None if shape(at + i) else (at + i) * 2654435761 % (1 << 64) for i in range(m)])
            at += m
        return out
    return {"name": "lengths", "n": len(rows), "fields": [
        list_field(b"all", INT64, lists(lambda e: False)), list_field(b"none", INT64, lists(lambda e: True)), list_field(b"odd", UINT64, lists(lambda e: e % 2 == 0)),
        list_field(b"edges", INT64, lists(lambda e: e % 64 in (0, 63)))]}


def _string_lengths():
    """the strings of the plain fixture -- an escapable byte at every position of lengths 0, 7, 8, 9, 15, 16, 17 -- as elements, one list per length"""
    cells = plain._string_lengths()["columns"][0]["cells"]
    lists = [[c for c in cells if len(c) == m] for m in plain.STRING_LENGTHS]
    return {"name": "string_lengths", "n": len(lists), "fields": [list_field(b"s", STRING, lists), list_field(b"c", STRING_CELLS, lists)]}


def _integers():
    t = plain._integers()
    i64, u64 = t["columns"][0]["cells"], t["columns"][1]["cells"]
    return {"name": "integers", "n": 3, "fields": [list_field(b"i", INT64, [i64, [], i64[::-1]]), list_field(b"u", UINT64, [u64, u64[::-1], []])]}


def _doubles():
    """the explicit table of doubles of tests/json_text_cases.py as elements; one field, so the bare row shape is legal"""
    bits = [b for b, _ in json_text_cases.fixture()[2]]
    return {"name": "doubles", "n": 4, "fields": [list_field(b"d", DOUBLE, [bits, None, [bits[0], None, bits[1]], []])]}


def _bare_strings():
    return {"name": "bare_strings", "n": 6, "fields": [list_field(b"ignored", STRING, [[b"a", b'"', None], None, [], None, None, [b"z" * 20]])]}


def _bare_plain():
    """the bare row shape over PLAIN fields: a number, and a JSON text with an empty one and an invalid one (composition feeds these back)"""
    return {"name": "bare_plain", "n": 5, "fields": [column(b"", JSON, [b"[1,2]", b"", None, b'{"k":"v"}', b"0"])]}


def _json_elements():
    _, cases, _ = json_text_cases.fixture()
    texts = [c for c in cases if (c["document"], c["path"]) == (2, b"$[*]")][0]["texts"]
    elements = list(texts[:3]) + [b"", None] + list(texts[3:])
    return {"name": "json_elements", "n": 3, "fields": [list_field(b"j", JSON, [elements, [b"", None], elements[::-1]])]}


def _no_fields():
    return {"name": "no_fields", "n": 2, "fields": []}


def _keys():
    """keys that need escaping in front of lists; under ARRAY_ROWS nobody looks at them"""
    keys = [b"plain", b"", b"nul\x00inside", b'q"uote', bytes(range(0x20)), "clé".encode(), b"dup", b"dup"]
    return {"name": "keys", "n": 2, "fields": [list_field(k, INT64, [[i, None], None]) if i % 2 else column(k, BOOL, [i, None]) for i, k in enumerate(keys)]}


def fixture_tables():
    return [_every_kind(), _lengths(), _string_lengths(), _integers(), _doubles(), _bare_strings(), _bare_plain(), _json_elements(), _no_fields(), _keys()]


def _cell_blob(kind, cell):
    if cell is None:
        return b"\x00"
    if kind <= BOOL:
        return b"\x01" + struct.pack("<Q", cell)
    return b"\x01" + struct.pack("<I", len(cell)) + cell


def table_blob(t):
    """one table as tests/golden/nested_write_golden.cpp reads it"""
    out = [struct.pack("<II", t["n"], len(t["fields"]))]
    for f in t["fields"]:
        out.append(struct.pack("<I", len(f["key"])) + f["key"] + struct.pack("<IB", f["kind"], 1 if is_list(f) else 0))
    for r in range(t["n"]):
        for f in t["fields"]:
            if not is_list(f):
                out.append(_cell_blob(f["kind"], f["cells"][r]))
            elif f["lists"][r] is None:
                out.append(b"\x00")
            else:
                out.append(b"\x01" + struct.pack("<I", len(f["lists"][r])) + b"".join(_cell_blob(f["kind"], e) for e in f["lists"][r]))
    return b"".join(out)


def fixture():
    """-> {table name: {"blob_sha256", flags: [text bytes per row] | {"lengths", "sha256"}}}"""
    g = json.load(open(GOLDEN))
    out = {}
    for t in g["tables"]:
        entry = {"blob_sha256": t["blob_sha256"]}
        for flags, f in t["flags"].items():
            entry[int(flags)] = [bytes.fromhex(x) for x in f["texts"]] if "texts" in f else f
        out[t["name"]] = entry
    return out


assert_rows_are_the_fixtures = plain.assert_rows_are_the_fixtures
split = plain.split


# ---- a table as arrays ----------------------------------------------------------------------------------------------------------------------------------------
def arrays_of(t, tail_ones=False, lead=0):
    """the table as arrays.  A list field's elements are its lists back to back behind `lead` elements that belong to no list (list_offsets[0] == lead); a field
    without an invalid list has no list validity words; the offset between two invalid lists is GARBAGE"""
    n, out = t["n"], []
    for f in t["fields"]:
        if not is_list(f):
            a = plain.arrays_of({"n": n, "columns": [f]}, tail_ones)["columns"][0]
            a.update(list_offsets=None, list_valid=None, elements=0)
            out.append(a)
            continue
        filler = 0 if f["kind"] <= BOOL else b"lead"
        elements, offsets = [filler] * lead, [lead]
        for x in f["lists"]:
            elements += x or []
            offsets.append(len(elements))
        a = plain.arrays_of({"n": len(elements), "columns": [column(f["key"], f["kind"], elements)]}, tail_ones)["columns"][0]
        for r in range(1, n):
            if f["lists"][r - 1] is None and f["lists"][r] is None:
                offsets[r] = GARBAGE
        a["list_offsets"] = np.array(offsets, np.uint32)
        a["list_valid"] = plain.valid_words([x is not None for x in f["lists"]], n, tail_ones) if any(x is None for x in f["lists"]) else None
        a["elements"] = len(elements)
        out.append(a)
    return {"n": n, "fields": out}


def as_plain_arrays(arrays):
    """the arrays of a table WITHOUT list fields as tests/write_records_model.py and sjgpu_write_records_device take them"""
    assert all(f["list_offsets"] is None for f in arrays["fields"])
    return {"n": arrays["n"], "columns": arrays["fields"]}


# ---- tables by rule: the edges of the kernels ------------------------------------------------------------------------------------------------------------------
def mixed_table(n, seed=0):
    """the six plain columns of write_records_cases.mixed_table with three list fields among them: 0 .. 4 int64 per row, 0 .. 3 strings, 0 .. 2 doubles (a non-finite
    one now and then), every ninth list invalid, every fifth element invalid"""
    t = plain.mixed_table(n, seed)
    rng = np.random.default_rng(2000 + n + seed)
    def lists(make, most, k):
        out = []
        for r in range(n):
            if (r + k) % 9 == 0:
                out.append(None)
            else:
                out.append([None if (r + i + k) % 5 == 0 else make(r, i) for i in range(int(rng.integers(0, most + 1)))])
        return out
    ints = lists(lambda r, i: int(rng.integers(0, 1 << 63)) * 2 + (r & 1), 4, 0)
    strs = lists(lambda r, i: b"h%d" % (r * 7 + i) + (b'"\\' if (r + i) % 4 == 0 else b""), 3, 1)
    dbls = lists(lambda r, i: 0x7FF8000000000000 if (r + i) % 13 == 0 else bits_of((r - 40) * 0.25 + i * 1e-3), 2, 2)
    c = t["columns"]
    return {"name": f"nested_mixed_{n}", "n": n, "fields": [c[0], list_field(b"ints", INT64, ints), c[1], c[2], list_field(b"tags", STRING_CELLS, strs), c[3], c[4],
                                                             list_field(b"ds", DOUBLE, dbls), c[5]]}


def narrow_table(n, seed=0):
    """one id and one short list<int64> per row: 256 rows fit the window"""
    t = mixed_table(n, seed)
    return {"name": f"nested_narrow_{n}", "n": n, "fields": [t["fields"][0], t["fields"][1]]}


def wide_table(K, n=70):
    """K fields, list and plain ones in turn, of cycling kinds"""
    fields = []
    for k in range(K):
        kind = [INT64, UINT64, DOUBLE, BOOL, STRING, STRING_CELLS, JSON][k % 7]
        def value(r, i):
            if kind <= BOOL:
                return bits_of(r + i / 4) if kind == DOUBLE else (r * 2654435761 + i) % (1 << 64) if kind != BOOL else (r + i) & 1
            return (b"[%d]" % (r + i) if (r + i) % 9 else b"") if kind == JSON else b"v%d" % (r + i)
        if k % 2:
            fields.append(list_field(b"k%d" % k, kind, [None if (r + k) % 5 == 0 else [None if (r + i) % 4 == 0 else value(r, i) for i in range((r + k) % 4)] for r in range(n)]))
        else:
            fields.append(column(b"k%d" % k, kind, [None if (r + k) % 5 == 0 else value(r, k) for r in range(n)]))
    return {"name": f"nested_wide_{K}", "n": n, "fields": fields}


def digits_table(lengths, key=b"v"):
    """one list<uint64> "v" per row whose text {"v":[...]} + line feed takes exactly lengths[r] bytes: elements of 9 digits and one that takes the rest (lengths[r] >= 9)
    -- for spans that end exactly where a test wants them"""
    frame = len(b'{"":[]}\n') + len(key)
    lists = []
    for r, total in enumerate(lengths):
        body = total - frame
        assert body >= 1, total
        full, rest = divmod(body, 10)  # an element of 9 digits and its comma
        if rest == 0:
            full, rest = full - 1, 10
        # `full` elements of 9 digits with a comma each, then one of rest digits (1 .. 10: ten digits when the rest would be none)
        elements = [100000000 + (r * 31 + i) % 899999999 for i in range(full)] + [10 ** (rest - 1) + (r % 9 if rest > 1 else r % 9)]
        lists.append(elements)
    return {"name": "digits", "n": len(lengths), "fields": [list_field(key, UINT64, lists)]}


# ---- the fill's grouping (k_nested_fill): which road the 256 rows of an iteration take, from the output's offsets alone ------------------------------------------
ROWS_PER_STEP, WINDOW, GRID_ROWS = plain.ROWS_PER_STEP, plain.WINDOW, plain.GRID_ROWS


def group_rows(offsets, r0, window=WINDOW):
    """the rows of one window use for the iteration that begins at row r0 -- 256, 128, 64, 32 -- or 0 for the direct road: the largest size for which every group's
    span fits the window"""
    n = len(offsets) - 1
    r_end = min(r0 + ROWS_PER_STEP, n)
    for size in (256, 128, 64, 32):
        edges = [int(offsets[min(r0 + g, r_end)]) for g in range(0, ROWS_PER_STEP + 1, size)]
        if all(b - a <= window for a, b in zip(edges[:-1], edges[1:])):
            return size
    return 0


def grouping_cases(window=WINDOW, rows_after=5):
    """{name: (table, the group size its first iteration must take)} -- under NEWLINE; digits_table makes every row's length exact"""
    W, after = window, [10 + r for r in range(rows_after)]
    even = [W // 256] * 256
    def bump(lengths, r, by):
        out = list(lengths)
        out[r] += by
        return out
    return {
        "256 rows of exactly the window": (digits_table(even + after), 256),
        "one byte more, both halves fit": (digits_table(bump(even, 255, 1) + after), 128),
        "64-row groups fit, a 128-row group does not": (digits_table([300] * 256 + after), 64),
        "a 32-row group of exactly the window": (digits_table([W // 32] * 32 + [10] * 224 + after), 32),
        "a 32-row group of one byte more": (digits_table(bump([W // 32] * 32, 31, 1) + [10] * 224 + after), 0),
        "a short iteration: a 32-row group of exactly the window, then 8 rows": (digits_table([10] * 32 + [W // 32] * 40), 32),
    }


def long_row_table(long_bytes=65536):
    """three iterations and seven rows of narrow_table, one row of the second with a list whose text takes long_bytes and more"""
    n = 3 * ROWS_PER_STEP + 7
    t = narrow_table(n)
    t["fields"][1]["lists"][ROWS_PER_STEP + 100] = [(1 << 63) + i for i in range(long_bytes // 20 + 1)]
    return t


def bad_lists():
    """-> (arrays, the rows that must have status 19): list offsets that run backwards and that end beyond `elements` under a valid bit, an element string that ends
    beyond its characters, an element cell whose offset + length does; the neighbours are served"""
    n = 10
    t = {"name": "bad_lists", "n": n, "fields": [list_field(b"i", INT64, [[r, r + 1] for r in range(n)]), list_field(b"s", STRING, [[b"s%d" % r, b"t"] for r in range(n)]),
                                                 list_field(b"c", STRING_CELLS, [[b"c%d" % r] for r in range(n)]), column(b"r", UINT64, list(range(n)))]}
    a = arrays_of(t, lead=2)
    i, s, c = a["fields"][0], a["fields"][1], a["fields"][2]
    i["list_offsets"][3] = i["list_offsets"][4] + 1     # row 3 runs backwards (row 2 is longer for it, and still inside: served)
    i["list_offsets"][n] = i["elements"] + 1            # row n - 1 ends one element beyond
    s["chars_bytes"] = int(s["offsets"][int(s["list_offsets"][6])]) - 1  # the LAST element of row 5 ends one byte beyond chars_bytes, and so does every later one
    c["values"][int(c["list_offsets"][1])] = np.uint64((c["chars_bytes"] - 1) | (2 << 32))  # row 1's element: offset + length one byte too far
    return a, [1, 3] + list(range(5, n))


def hidden_bad_lists():
    """the bad words of bad_lists() under validity bits of 0 -- the lists' where the list offsets are bad, the elements' where the element is: every row is served"""
    a, bad = bad_lists()
    n = a["n"]
    i, s, c = a["fields"][0], a["fields"][1], a["fields"][2]
    i["list_valid"] = plain.valid_words([r not in (3, n - 1) for r in range(n)], n)
    s["valid"] = plain.valid_words([int(s["offsets"][e + 1]) <= s["chars_bytes"] for e in range(s["elements"])], s["elements"])
    c["valid"] = plain.valid_words([e != int(c["list_offsets"][1]) for e in range(c["elements"])], c["elements"])
    return a
