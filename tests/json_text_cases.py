"""Shared by the tests of the JSON text call (tests/test_json_text_model.py, tests/test_json_emu.py, tests/test_gpu_json.py): the fixture
tests/golden/json_text.json (the real reference, tests/golden/make_json_text_golden.py), the rows of cells its cases stand for -- made by the oracle's tapes and the
Python model of the paths call --, and streams made by hand: deep documents on both sides of the bit stack's spill, strings of chosen lengths and bytes, cells of every
kind, and tapes broken on purpose."""
import hashlib
import json
import os
import random
import struct

import numpy as np

import path_model
import query_cases
import rows_model
from simdjson_amd import _paths

GOLDEN = os.path.join(_paths.REPO_ROOT, "tests", "golden", "json_text.json")
ROW_COUNTS = [0, 1, 63, 64, 65, 257]
DEPTHS = [63, 64, 65, 70, 1100]
MAX_DEPTH = 2048  # what the deep documents are parsed with (the parser's default, 1 024, stops short of the deepest)
STRING_LENGTHS = list(range(18)) + [299]
TAPE_TAGS = b'[{]}"ludtfnr'  # the top byte of every kind of tape word


def bits_of(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def double_groups():
    """The bulk of the doubles' table, made by rule (the generator and the tests share it) -> {name: [bits]}: every power of two with its neighbours one ulp either
    side (the lower one lies across the shorter interval), every power of ten with its neighbours, seeded random bit patterns, the powers of two below the smallest
    normal -- one mantissa bit each, down to bit pattern 1 -- with their neighbours, and 64 seeded doubles under each of the twelve tape tags as their top byte: a
    payload word that looks like a tag word to whoever reads the tape a word at a time (all finite: no tag is 0x7F or 0xFF).  The fixture keeps the count and
    the SHA-256 of each group's texts, joined by newlines; the doubles whose text is worth reading are in its explicit table."""
    two = [b for e in range(1, 2047) for b in ((e << 52) - 1, e << 52, (e << 52) + 1)]
    ten = [bits_of(float("1e%d" % k)) + d for k in range(-323, 309) for d in (-1, 0, 1)]
    rng, rnd = random.Random(20261019), []
    while len(rnd) < 4000:
        b = rng.getrandbits(64)
        if (b >> 52) & 0x7FF != 0x7FF:
            rnd.append(b)
    sub = []
    for k in range(52):
        for b in ((1 << k) - 1, 1 << k, (1 << k) + 1):
            if b != 0 and b not in sub:
                sub.append(b)
    rng = random.Random(20261021)
    tags = [(tag << 56) | rng.getrandbits(56) for tag in TAPE_TAGS for _ in range(64)]
    return {"powers_of_two": two, "powers_of_ten": ten, "random": rnd, "subnormal_powers_of_two": sub, "tag_lookalikes": tags}


def group_digest(texts):
    return hashlib.sha256(b"\n".join(texts)).hexdigest()


def fixture():
    """-> (documents as bytes, cases: the fixture's dicts with "path" as bytes and, for the small columns, "texts" as a list of bytes, doubles: the explicit table
    [(bits, text bytes)]); the bulk groups' counts and digests: fixture_double_groups()"""
    g = json.load(open(GOLDEN))
    docs = [open(os.path.join(_paths.REPO_ROOT, "tests", "golden", "jsonexamples", d), "rb").read() if isinstance(d, str) else bytes.fromhex(d["hex"]) for d in g["documents"]]
    cases = []
    for c in g["cases"]:
        c = dict(c, path=bytes.fromhex(c["path"]))
        if "texts" in c:
            c["texts"] = [bytes.fromhex(t) for t in c["texts"]]
        cases.append(c)
    doubles = [(int(line[:16], 16), line[17:].encode()) for line in g["doubles"].split("\n")]
    return docs, cases, doubles


def fixture_double_groups():
    """-> {name: {"count", "sha256"}} for the groups of double_groups()"""
    return json.load(open(GOLDEN))["double_groups"]


def assert_texts_are_the_fixtures(c, texts):
    """texts: one bytes per cell -- byte for byte the fixture's, through their lengths and the digest of all of them where the fixture keeps only those"""
    what = (c["document"], c["path"])
    assert len(texts) == c["cells"], what
    if "texts" in c:
        for r, (got, want) in enumerate(zip(texts, c["texts"])):
            assert got == want, (what, r, got[:200], want[:200])
    else:
        assert [len(t) for t in texts] == c["lengths"], what
        assert hashlib.sha256(b"".join(texts)).hexdigest() == c["sha256"], what


def split(offsets, chars):
    chars = bytes(chars)
    offsets = np.asarray(offsets).tolist()
    return [chars[a:b] for a, b in zip(offsets[:-1], offsets[1:])]


def stream_of(parsed):
    """[(tape, sbuf)] per document -> (tape uint64[...], sbuf uint8[...], table) as sjgpu_stage2_many_device lays them out"""
    return query_cases.lay_out(parsed)


def root_row(tape, sbuf, table):
    """the root cell of every document of a stream -> (tags, values)"""
    cells = [rows_model.root_cell(tape, sbuf, table, d) for d in range(len(table) - 1)]
    return np.array([t for t, _ in cells], np.uint8), np.array([v for _, v in cells], np.uint64)


def fixture_rows(orc):
    """-> [(case, (tape, sbuf, table) of the case's document alone, (tags, values): the row the case serialises)]; the path $ is the document's root cell"""
    docs, cases, _ = fixture()
    parsed, out = {}, []
    for c in cases:
        d = c["document"]
        if d not in parsed:
            err, tape, sbuf = orc.dom_parse(docs[d])
            assert err == 0
            parsed[d] = (stream_of([(tape, sbuf)]), tape.tolist(), sbuf.tobytes())
        stream, tape_list, sbuf_bytes = parsed[d]
        if c["path"] == b"$":
            row = root_row(*stream)
        else:
            _, _, tags, values = path_model.column([(tape_list, sbuf_bytes)], [c["path"]])
            row = (np.array(tags, np.uint8), np.array(values, np.uint64))
        out.append((c, stream, row))
    return out


def deep_document(depth):
    """`depth` containers inside one another, objects and arrays alternating, with a string both as a key and as a value at every level and a sibling behind every
    child container: what lies behind a pop must still know whether it is in an object"""
    head, tail = [], []
    for level in range(depth):
        if level % 2 == 0:
            head.append(b'{"s%d":"v%d","c":' % (level, level))
            tail.append(b',"after%d":"k"}' % level)
        else:
            head.append(b'["e%d",' % level)
            tail.append(b',"z%d",{"in":"obj"},["in","arr"]]' % level)
    return b"".join(head) + b'"bottom"' + b"".join(reversed(tail))


def string_cases():
    """strings of length 0 .. 17 and 299 built from every byte 0x00 .. 0x7f and multi-byte characters, as JSON sources: each escape at every position of the eight-byte
    step, and runs without any"""
    def source_of(codepoints):
        return '"' + "".join("\\u%04x" % c if c < 0x20 or c in (0x22, 0x5C, 0x7F) else chr(c) for c in codepoints) + '"'
    pool = list(range(0x80)) + [0xE9, 0x20AC, 0x1F600]
    out, at = [], 0
    for n in STRING_LENGTHS:
        for variant in range(4 if n else 1):
            cps = []
            while len(cps) < n:  # n characters (their bytes may be more)
                cps.append(pool[at % len(pool)] if variant != 3 else 0x61 + (at % 26))
                at += 1 if variant != 2 else 7
            text = source_of(cps)
            out.append(text.encode("utf-8"))
    return out


def strings_document():
    return b"[" + b",".join(string_cases()) + b',{' + b",".join(s + b":" + s for s in string_cases()[:40]) + b"}]"


def every_kind_of_cell(string_bytes, container_cell):
    """(tag, value, served): every kind of scalar root, every code, bytes that are neither, string cells outside the buffer, a container cell that disagrees"""
    tag, value = container_cell
    cells = [(ord("t"), 1, True), (ord("f"), 0, True), (ord("n"), 0, True), (ord("l"), 0, True), (ord("l"), (1 << 64) - 1, True), (ord("l"), 1 << 63, True),
             (ord("l"), (1 << 63) - 1, True), (ord("u"), (1 << 64) - 1, True), (ord("u"), 1 << 63, True), (ord("u"), 7, True), (ord("d"), 0, True), (ord("d"), 1 << 63, True),
             (ord("d"), 0x3FF8000000000000, True), (ord("d"), 0x7FEFFFFFFFFFFFFF, True), (ord("d"), 1, True), (ord("d"), 0x7FF0000000000000, False),
             (ord("d"), 0xFFF8000000000000, False), (ord('"'), 4, True), (ord('"'), string_bytes, True)]
    cells += [(c, 0, False) for c in (17, 19, 20, 22)]
    cells += [(0, 0, False), (1, 5, False), (33, 0, False), (ord("r"), 4, False), (ord("}"), 0, False), (0x5A, 0x5A5A5A5A5A5A5A5A, False), (255, 1, False), (ord("'"), 4, False)]
    cells += [(ord('"'), (1 << 32) | string_bytes, False), (ord('"'), (2 << 32) | (string_bytes - 1), False), (ord('"'), 0xFFFFFFFFFFFFFFFF, False),
              (ord('"'), (string_bytes + 1) << 32, False)]
    cells += [(tag, value, True), (tag ^ 0x20, value, False), (tag, value + (1 << 32), False), (tag, value + 1, False), (tag, value & 0xFFFFFFFF, False), (tag, 0, False)]
    return cells


def broken_tapes(tape, table):
    """tape: one document's words (a numpy array, its root a container with containers, strings and numbers inside).  -> [(what, broken copy)]: each must turn the root
    cell -- taken from the INTACT tape -- into status 20, or, where the root's own words disagree, be refused the same way"""
    tape = np.asarray(tape, np.uint64)
    tags = (tape >> np.uint64(56)).astype(np.uint8)
    opens = [i for i in range(2, len(tape) - 2) if tags[i] in (0x7B, 0x5B) and not (tags[i - 1] in (0x6C, 0x75, 0x64))]
    closes = [i for i in range(2, len(tape) - 2) if tags[i] in (0x7D, 0x5D) and not (tags[i - 1] in (0x6C, 0x75, 0x64))]
    strings = [i for i in range(2, len(tape) - 2) if tags[i] == 0x22 and not (tags[i - 1] in (0x6C, 0x75, 0x64))]
    out = []

    def patched(what, i, word):
        t = tape.copy()
        t[i] = np.uint64(word)
        out.append((what, t))
    inner_open, inner_close, a_string = opens[len(opens) // 2], closes[len(closes) // 2], strings[len(strings) // 2]
    patched("a closing word that points at another word", inner_close, int(tape[inner_close]) + 1)
    patched("a closing word of the other kind", inner_close, int(tape[inner_close]) ^ (0x26 << 56))  # } <-> [ ... any other tag
    patched("an opening word that ends elsewhere", inner_open, int(tape[inner_open]) + 1)
    patched("an unknown tag", a_string, (int(tape[a_string]) & ((1 << 56) - 1)) | (ord("x") << 56))
    patched("a root word inside", a_string, ord("r") << 56)
    patched("a string payload outside the buffer", a_string, (ord('"') << 56) | 0xFFFFFFFFFF)
    patched("a closing word too early", a_string, int(tape[len(tape) - 2]))
    return out
