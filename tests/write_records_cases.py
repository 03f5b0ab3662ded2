"""Shared by the tests of the record writer (tests/test_write_records_model.py, tests/test_write_emu.py, tests/test_gpu_write.py) and by the generator of their
fixture (tests/golden/make_write_records_golden.py): the tables tests/golden/write_records.json holds the reference's texts for, defined once, here; how a table
becomes the arrays sjgpu_write_records_device reads; and the tables made by rule for the edges of its kernels -- row counts, column counts, validity words, spans
around the staged road's window, bad offsets and doubles without a text.

A TABLE is {"name", "n", "columns": [{"key": bytes, "kind": SJGPU_COL_*, "cells": [None | int | bytes] * n}]}: None is a cell whose validity bit is 0, an int the 64
bits of a number or a boolean (kinds 1 .. 4), bytes a string (kinds 5, 9) or a JSON text (kind 8).
Its ARRAYS are {"n", "columns": [{"key", "kind", "values": uint64[n] | None, "valid": uint64[ceil(n / 64)] | None, "offsets": uint32[n + 1] | None,
"chars": uint8[...] | None, "chars_bytes": int}]} -- what the model, the emulation's driver and the device take."""
import hashlib
import json
import os
import struct

import numpy as np

import json_text_cases
from simdjson_amd import _paths

GOLDEN = os.path.join(_paths.REPO_ROOT, "tests", "golden", "write_records.json")
INT64, UINT64, DOUBLE, BOOL, STRING, JSON, STRING_CELLS = 1, 2, 3, 4, 5, 8, 9
OMIT_NULLS, NEWLINE = 1, 2
ALL_FLAGS = (0, OMIT_NULLS, NEWLINE, OMIT_NULLS | NEWLINE)
SMALL = 6 << 10
ROWS_PER_STEP, MAX_WORKGROUPS, WINDOW = 256, 512, 28 << 10  # of sjgpu_write.hip: a workgroup iteration's rows, the grid's cap, the staged road's window
ROW_COUNTS = [0, 1, 63, 64, 65, 255, 256, 257, 513]
GRID_ROWS = MAX_WORKGROUPS * ROWS_PER_STEP + 1
COLUMN_COUNTS = [0, 1, 2, 64]
STRING_LENGTHS = [0, 7, 8, 9, 15, 16, 17]
POISON_WORD = 0x5A5A5A5A5A5A5A5A


def bits_of(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def column(key, kind, cells):
    return {"key": bytes(key), "kind": kind, "cells": list(cells)}


# ---- the tables of the fixture ------------------------------------------------------------------------------------------------------------------------------
def _every_kind():
    n = 9
    texts = [b'{"a":[1,2,{"b":null}]}', b"[]", b"", b"7", b'"s"', None, b"null", b'[true,false]', b"{}"]
    return {"name": "every_kind", "n": n, "columns": [
        column(b"i", INT64, [0, 1, (1 << 64) - 1, None, 42, 1 << 63, 7, None, 1000000]),
        column(b"u", UINT64, [0, None, (1 << 64) - 1, 3, 42, 1 << 63, 7, 8, None]),
        column(b"d", DOUBLE, [bits_of(0.0), bits_of(-0.0), None, bits_of(1.5), bits_of(1e21), bits_of(-2.5e-7), bits_of(100.0), None, bits_of(0.1)]),
        column(b"b", BOOL, [0, 1, 2, None, 1 << 63, 0, 1, None, 0]),
        column(b"s", STRING, [b"", b"plain", None, b'q"uote', b"back\\slash", b"\n", "é€".encode(), None, b"0123456789abcdef"]),
        column(b"c", STRING_CELLS, [b"cell", None, b"", b"\x00\x1f", b"tab\there", b"x", None, b"/", b"\x7f"]),
        column(b"j", JSON, texts)]}


def _keys():
    keys = [b"plain", b"", b"nul\x00inside", b'q"uote', b"back\\slash", bytes(range(0x20)), b"\b\t\n\f\r", "clé".encode(), b"dup", b"dup", b"\x7f/"]
    return {"name": "keys", "n": 3, "columns": [column(k, INT64, [i, None, (1 << 64) - i - 1]) for i, k in enumerate(keys)]}


def _long_key():
    return {"name": "long_key", "n": 2, "columns": [column(b"k" * 1023 + b'"', INT64, [1, None]), column(b"", BOOL, [None, 1])]}


def _bytes256():
    whole = bytes(range(256))
    cells = [whole] + [whole[16 * i: 16 * i + 16] for i in range(16)] + [whole[::-1]]
    return {"name": "bytes256", "n": len(cells), "columns": [column(b"s", STRING, cells), column(b"c", STRING_CELLS, cells)]}


def _string_lengths():
    """strings of length 0, 7, 8, 9, 15, 16, 17 with an escapable byte at every position (every position of the eight-byte word, in every word), and without one"""
    escapable = [b'"', b"\\", b"\n", b"\x01", b"\x1f", b"\r"]
    cells, at = [], 0
    for n in STRING_LENGTHS:
        plain = bytes(0x61 + (i % 26) for i in range(n))
        cells.append(plain)
        for pos in range(n):
            cells.append(plain[:pos] + escapable[at % len(escapable)] + plain[pos + 1:])
            at += 1
    return {"name": "string_lengths", "n": len(cells), "columns": [column(b"s", STRING, cells), column(b"c", STRING_CELLS, cells)]}


def _integers():
    i64 = [0, 1, (1 << 64) - 1, (1 << 63) - 1, 1 << 63, 9, 10, (1 << 64) - 10, 99999999, 100000000, 9999999999999999, 10000000000000000, 10 ** 18, (1 << 64) - 10 ** 18]
    u64 = [0, 1, (1 << 64) - 1, (1 << 63) - 1, 1 << 63, 9, 10, 10 ** 19, 99999999, 100000000, 9999999999999999, 10000000000000000, 10 ** 19 - 1, 12345678901234567890]
    return {"name": "integers", "n": len(i64), "columns": [column(b"i", INT64, i64), column(b"u", UINT64, u64)]}


def _doubles():
    """the explicit table of doubles of tests/json_text_cases.py (the one tests/golden/json_text.json holds the texts of)"""
    bits = [b for b, _ in json_text_cases.fixture()[2]]
    return {"name": "doubles", "n": len(bits), "columns": [column(b"d", DOUBLE, bits)]}


def _json_cells():
    """JSON cells taken from tests/golden/json_text.json: the elements of the hand-made document, with an empty text and an invalid cell among them"""
    _, cases, _ = json_text_cases.fixture()
    texts = [c for c in cases if (c["document"], c["path"]) == (2, b"$[*]")][0]["texts"]
    cells = list(texts[:3]) + [b"", None] + list(texts[3:])
    return {"name": "json_cells", "n": len(cells), "columns": [column(b"j", JSON, cells), column(b"n", UINT64, list(range(len(cells))))]}


def fixture_tables():
    return [_every_kind(), _keys(), _long_key(), _bytes256(), _string_lengths(), _integers(), _doubles(), _json_cells()]


def table_blob(t):
    """one table as tests/golden/write_records_golden.cpp reads it"""
    out = [struct.pack("<II", t["n"], len(t["columns"]))]
    for c in t["columns"]:
        out.append(struct.pack("<I", len(c["key"])) + c["key"] + struct.pack("<I", c["kind"]))
    for r in range(t["n"]):
        for c in t["columns"]:
            cell = c["cells"][r]
            if cell is None:
                out.append(b"\x00")
            elif c["kind"] <= BOOL:
                out.append(b"\x01" + struct.pack("<Q", cell))
            else:
                out.append(b"\x01" + struct.pack("<I", len(cell)) + cell)
    return b"".join(out)


def fixture():
    """-> {table name: {"blob_sha256", flags: [text bytes per row] | {"lengths", "sha256"}}}"""
    g = json.load(open(GOLDEN))
    out = {}
    for t in g["tables"]:
        entry = {"blob_sha256": t["blob_sha256"]}
        for flags in ALL_FLAGS:
            f = t["flags"][str(flags)]
            entry[flags] = [bytes.fromhex(x) for x in f["texts"]] if "texts" in f else f
        out[t["name"]] = entry
    return out


def assert_rows_are_the_fixtures(want, texts, what):
    """texts: one bytes per row -- byte for byte the fixture's, through their lengths and the digest of all of them where the fixture keeps only those"""
    if isinstance(want, list):
        assert len(texts) == len(want), what
        for r, (got, w) in enumerate(zip(texts, want)):
            assert got == w, (what, r, got[:200], w[:200])
    else:
        assert [len(x) for x in texts] == want["lengths"], what
        assert hashlib.sha256(b"".join(texts)).hexdigest() == want["sha256"], what


# ---- a table as arrays ----------------------------------------------------------------------------------------------------------------------------------------
def valid_words(bits, n, tail_ones=False):
    """bits: n booleans -> uint64[ceil(n / 64)], least significant bit first; tail_ones: the bits at and beyond n of the last word all ones (they are not looked at)"""
    words = np.zeros((n + 63) // 64, np.uint64)
    for r, b in enumerate(bits):
        if b:
            words[r >> 6] |= np.uint64(1 << (r & 63))
    if tail_ones and n % 64:
        words[-1] |= np.uint64(((1 << 64) - 1) & ~((1 << (n % 64)) - 1))
    return words


def arrays_of(t, tail_ones=False, lead=3):
    """the table as arrays.  A column without an invalid cell has no validity words (a null valid_dev).  What lies under an invalid cell is poison: a value word of 0x5A
    bytes, offsets that run backwards where the neighbours allow it.  lead: bytes in front of a STRING_CELLS column's first string (a string buffer begins anywhere)"""
    n, cols = t["n"], []
    for c in t["columns"]:
        cells, kind = c["cells"], c["kind"]
        a = {"key": c["key"], "kind": kind, "values": None, "valid": None, "offsets": None, "chars": None, "chars_bytes": 0}
        if any(x is None for x in cells):
            a["valid"] = valid_words([x is not None for x in cells], n, tail_ones)
        if kind <= BOOL:
            a["values"] = np.array([POISON_WORD if x is None else x for x in cells], np.uint64)
        elif kind == STRING_CELLS:
            chars, values = bytearray(b"\xEE" * lead), []
            for x in cells:
                if x is None:
                    values.append(POISON_WORD)
                else:
                    values.append(len(chars) | (len(x) << 32))
                    chars += x
            a["values"], a["chars"] = np.array(values, np.uint64), np.frombuffer(bytes(chars), np.uint8).copy()
            a["chars_bytes"] = len(chars)
        else:
            chars, offsets = bytearray(), [0]
            for x in cells:
                chars += x or b""
                offsets.append(len(chars))
            a["offsets"], a["chars"] = np.array(offsets, np.uint32), np.frombuffer(bytes(chars), np.uint8).copy()
            a["chars_bytes"] = len(chars)
        cols.append(a)
    return {"n": n, "columns": cols}


def split(offsets, chars):
    chars = bytes(chars)
    offsets = np.asarray(offsets).tolist()
    return [chars[a:b] for a, b in zip(offsets[:-1], offsets[1:])]


# ---- tables by rule: the edges of the kernels ------------------------------------------------------------------------------------------------------------------
def mixed_table(n, seed=0):
    """n rows of six columns of every fixed-width kind and both string layouts, every seventh cell invalid, a non-finite double now and then"""
    rng = np.random.default_rng(1000 + n + seed)
    ints = rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n, dtype=np.uint64)
    small = rng.integers(0, 100000, n)
    dbl = (rng.standard_normal(n) * 10.0 ** rng.integers(-8, 9, n)).view(np.uint64) if n else np.zeros(0, np.uint64)

    def cells(values, k):
        return [None if (r + k) % 7 == 0 else int(v) for r, v in enumerate(values)]
    strings = [None if (r + 4) % 7 == 0 else (b"s%d" % small[r]) + (b'"\n' if r % 5 == 0 else b"") + b"x" * int(small[r] % 23) for r in range(n)]
    doubles = cells(dbl, 2)
    for r in range(3, n, 11):
        doubles[r] = [0x7FF0000000000000, 0xFFF0000000000000, 0x7FF8000000000000, 0xFFF8000000000123][(r // 11) % 4]
    return {"name": f"mixed_{n}", "n": n, "columns": [
        column(b"id", INT64, cells(ints, 0)), column(b"count", UINT64, cells(small, 1)), column(b"score", DOUBLE, doubles), column(b"ok", BOOL, cells(small % 2, 3)),
        column(b"name", STRING, strings), column(b"tag", STRING_CELLS, [None if x is None else x[::-1] for x in strings])]}


def narrow_table(n, seed=0):
    """the first and the fifth column of mixed_table: rows short enough for 256 of them to fit the staged road's window (mixed_table's do not)"""
    t = mixed_table(n, seed)
    return {"name": f"narrow_{n}", "n": n, "columns": [t["columns"][0], t["columns"][4]]}


def wide_table(K, n=70):
    """K columns (the interface's most: 64) of cycling kinds, short keys"""
    cols = []
    for k in range(K):
        kind = [INT64, UINT64, DOUBLE, BOOL, STRING, STRING_CELLS, JSON][k % 7]
        if kind <= BOOL:
            cells = [None if (r + k) % 5 == 0 else (bits_of(r + k / 4) if kind == DOUBLE else (r * 2654435761 + k) % (1 << 64) if kind != BOOL else r & 1) for r in range(n)]
        elif kind == JSON:
            cells = [None if (r + k) % 5 == 0 else (b"" if (r + k) % 9 == 0 else b"[%d]" % r) for r in range(n)]
        else:
            cells = [None if (r + k) % 5 == 0 else b"v%d" % (r + k) for r in range(n)]
        cols.append(column(b"k%d" % k, kind, cells))
    return {"name": f"wide_{K}", "n": n, "columns": cols}


def span_table(total, n=ROWS_PER_STEP, long_row=None, rows_after=0, newline=True):
    """n rows of one STRING column "s" whose texts -- {"s":"..."} and, under newline, a line feed -- take `total` bytes together (the span of one workgroup
    iteration), then rows_after short rows; long_row: the one row that takes what the even split leaves over (by default the last)"""
    frame = len(b'{"s":""}') + (1 if newline else 0)
    assert total >= n * frame
    body = total - n * frame
    each = [body // n] * n
    each[n - 1 if long_row is None else long_row] += body - sum(each)
    cells = [bytes(0x41 + (r + i) % 26 for i in range(m)) for r, m in enumerate(each)]
    cells += [b"after%d" % r for r in range(rows_after)]
    return {"name": f"span_{total}", "n": len(cells), "columns": [column(b"s", STRING, cells)]}


def nonfinite_table():
    """NaN, the infinities and a NaN with a payload among finite doubles, a second column so that a row is never empty by accident"""
    bits = [bits_of(1.0), 0x7FF8000000000000, 0x7FF0000000000000, 0xFFF0000000000000, 0x7FF8000000000ABC, 0xFFFFFFFFFFFFFFFF, 0x7FF0000000000001, bits_of(-0.0), None,
            0x7FEFFFFFFFFFFFFF]
    return {"name": "nonfinite", "n": len(bits), "columns": [column(b"d", DOUBLE, bits), column(b"r", UINT64, list(range(len(bits))))]}


def bad_offsets(arrays_under_valid_bits=False):
    """-> (arrays, the rows that must have status 19): a STRING column whose offsets run backwards at one row and end beyond chars_bytes at another, a JSON column with
    the same, a STRING_CELLS column with a cell whose offset + length is one byte too far and one whose offset alone is.  arrays_under_valid_bits: the same words, but
    every bad cell's validity bit is 0 -- every row is served, the bad cells as nulls"""
    n = 12
    good = [b"s%d" % r for r in range(n)]
    t = {"name": "bad_offsets", "n": n, "columns": [column(b"s", STRING, good), column(b"j", JSON, [b"%d" % r for r in range(n)]), column(b"c", STRING_CELLS, good),
                                                     column(b"i", INT64, list(range(n)))]}
    a = arrays_of(t)
    s, j, c = a["columns"][0], a["columns"][1], a["columns"][2]
    s["offsets"][3] = s["offsets"][4] + 2           # row 3 runs backwards (row 2 is longer for it, and still inside: served)
    s["chars_bytes"] = int(s["offsets"][n]) - 1     # row n - 1 ends one byte beyond chars_bytes
    j["offsets"][7] = 0xFFFFFFF0                    # row 6 ends far beyond; row 7 runs backwards
    c["values"][9] = np.uint64((c["chars_bytes"] - 1) | (2 << 32))   # offset + length one byte too far
    c["values"][10] = np.uint64((c["chars_bytes"] + 1) | (0 << 32))  # an empty cell that begins beyond the end
    bad = {3: [0], n - 1: [0], 6: [1], 7: [1], 9: [2], 10: [2]}
    if arrays_under_valid_bits:
        for k in range(3):
            a["columns"][k]["valid"] = valid_words([k not in bad.get(r, []) for r in range(n)], n)
        return a, []
    return a, sorted(bad)
