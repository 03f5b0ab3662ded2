"""Shared by the tests of the dictionary calls (tests/test_dictionary_model.py, tests/test_dict_emu.py, tests/test_gpu_dict.py): the fixture
tests/golden/dictionary.json (the real reference, tests/golden/make_dictionary_golden.py), the rows of cells its cases stand for -- made by the oracle's tapes and
the Python models of the paths and the fields calls --, and rows of cells made by hand: strings of chosen lengths, tricky pairs, cells that are no strings."""
import json
import os
import struct

import numpy as np

import fields_model
import path_model
import query_cases
from simdjson_amd import _paths

GOLDEN = os.path.join(_paths.REPO_ROOT, "tests", "golden", "dictionary.json")
VALUES, KEYS = 0, 1
STRING = ord('"')
ROW_COUNTS = [0, 1, 63, 64, 65, 255, 256, 257, 4097]
LENGTHS = [0, 1, 7, 8, 9, 15, 16, 17, 300]


def fixture():
    """-> (documents as bytes, cases: the fixture's dicts with "path" as bytes and "strings" as a list of bytes)"""
    g = json.load(open(GOLDEN))
    docs = [open(os.path.join(_paths.REPO_ROOT, "tests", "golden", "jsonexamples", d), "rb").read() if isinstance(d, str) else bytes.fromhex(d["hex"]) for d in g["documents"]]
    cases = [dict(c, path=bytes.fromhex(c["path"]), strings=[bytes.fromhex(s) for s in c["strings"]]) for c in g["cases"]]
    return docs, cases


def fixture_rows(orc):
    """-> [(case, string buffer uint8[...], (tags, values): the row the case encodes, (tags, values): the value row beside it)] over the oracle's tape of each
    document alone: a values case is the flattened matches of its path (its own value row), a keys case the key row and the value row of the fields of its matches"""
    docs, cases = fixture()
    parsed = {}
    out = []
    for c in cases:
        d = c["document"]
        if d not in parsed:
            err, tape, sbuf = orc.dom_parse(docs[d])
            assert err == 0
            parsed[d] = (tape, sbuf, fields_model.Stream(*query_cases.lay_out([(tape, sbuf)])), tape.tolist(), sbuf.tobytes())
        tape, sbuf, S, tape_list, sbuf_bytes = parsed[d]
        _, _, tags, values = path_model.column([(tape_list, sbuf_bytes)], [c["path"]])
        row = (np.array(tags, np.uint8), np.array(values, np.uint64))
        if c["mode"] == VALUES:
            out.append((c, sbuf, row, row))
        else:
            _, _, key_tags, key_values, vtags, vvalues = fields_model.column(S, row)
            out.append((c, sbuf, (key_tags, key_values), (vtags, vvalues)))
    return out


class Strings:
    """a string buffer built by hand: add(bytes) -> the string cell's word; the strings lie back to back behind a 4-byte length each, as the tape's records do, so
    that equal strings entered twice lie at two offsets"""

    def __init__(self):
        self.parts, self.size = [], 0

    def add(self, s):
        self.parts.append(struct.pack("<I", len(s)) + s + b"\0")
        word = (len(s) << 32) | (self.size + 4)
        self.size += len(s) + 5
        return word

    def buffer(self):
        return np.frombuffer(b"".join(self.parts), np.uint8).copy() if self.parts else np.zeros(0, np.uint8)


def string_row(strings):
    """a list of bytes -> (sbuf, (tags, values)), every occurrence a record of its own"""
    B = Strings()
    values = np.array([B.add(s) for s in strings], np.uint64)
    return B.buffer(), (np.full(len(strings), STRING, np.uint8), values)


def text_of_length(rng, length, pool=8):
    """one of `pool` strings of that length; strings of one length share a long prefix: they differ in their last byte or, from 9 bytes on, in the last but eight"""
    k = int(rng.integers(pool))
    if length == 0:
        return b""
    body = bytearray(b"p" * length)
    body[-1] = ord("a") + (k & 3)
    if length > 8:
        body[-9] = ord("a") + (k >> 2)
    return bytes(body)


def mixed_strings(rng, n):
    """n strings of the LENGTHS, drawn from a small pool per length: many repeats, pairs that differ in their last byte only, and each a prefix of the next length's"""
    return [text_of_length(rng, LENGTHS[int(rng.integers(len(LENGTHS)))]) for _ in range(n)]


def non_string_cells(string_bytes):
    """cells the encode counts as nulls: every other tag, every code, bytes that are neither, and string cells that point outside the buffer"""
    cells = [(ord(t), 7) for t in '{[ludtfn'] + [(c, 0) for c in (17, 19, 20, 22)] + [(0, 0), (1, 5), (33, 0), (ord("r"), 4), (ord("}"), 0), (0x5A, 0x5A5A5A5A5A5A5A5A), (255, 1),
                                                                                     (ord("'"), 4), (ord('"') + 1, 4)]
    cells += [(STRING, (1 << 32) | string_bytes), (STRING, (2 << 32) | (string_bytes - 1)), (STRING, 0xFFFFFFFFFFFFFFFF), (STRING, (0xFFFFFFFF << 32) | 4),
              (STRING, (string_bytes + 1) << 32), (STRING, 0xFFFFFFFF)]
    return cells


def rotating_row(n):
    """every wave of 64 cells holds the same three strings, in an order that rotates from wave to wave"""
    three = [b"alpha", b"beta", b"alphabet"]
    return [three[(i + i // 64) % 3] for i in range(n)]
