#!/usr/bin/env python3
"""Generates tests/golden/dictionary.json from the REAL reference: the dictionary of a column -- its distinct strings in order of first occurrence, where each was
met first, how often, and the code of every cell -- as std::unordered_map<std::string_view, ...> over what get_string() / key_value_pair::key return gives it
(the yardstick of sjgpu_dictionary_encode_device and sjgpu_cell_kinds_by_code_device, include/sjgpu_dict.h).

Run where the reference lies (needs its headers and oracle/_ref/libsjref.so):   python tests/golden/make_dictionary_golden.py

tests/golden/dictionary_golden.cpp -- a small program of our own -- is compiled against them into a temporary directory and fed the documents and cases below.
A case is (document, mode, path): mode 0 takes the elements of at_path_with_wildcard(path) as a column of values (no string: a null), mode 1 takes the keys of the
fields of the objects among them, in iteration order, and counts the kinds of the values under every key.  The fixture: "documents" (a file of
tests/golden/jsonexamples by name, or the bytes as hex), and per case "document", "mode", "path" (hex), "cells", "nulls", "strings" (hex, in order of first
occurrence), "first", "counts", "kinds" (ten counts per string: { [ " l u d t f n and negative l) and "codes".
"""
import json
import os
import struct
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from simdjson_amd import _paths  # noqa: E402

LONG = b"x" * 299
# what the contract says about equality: a NUL is a byte like any other, an escape is its character, "" is a string; pairs that differ in their last byte only, or
# of which one is a prefix of the other, at the lengths around the compare's 8-byte steps; cells that are no strings among them
HAND_MADE = (b'["a\\u0000b","a","a\\u0000","\\u0041","A","","a","",1,null,"a\\u0000b",{"k":"v"},["a"],true,-2.5,"abcdefg","abcdefgh","abcdefgi","abcdefghi",'
             b'"abcdefgh","0123456789abcde","0123456789abcdef","0123456789abcdeg","0123456789abcdefg","0123456789abcdef","' + LONG + b'y","' + LONG + b'z","' + LONG + b'","' +
             LONG + b'y","\\u00e9","\xc3\xa9","e","line\\nfeed","line\\u000afeed",false,"A",'
             b'{"":1,"a\\u0000b":2,"A":-3,"a":"s"},{"\\u0041":"x","a":null,"a\\u0000":-1,"":[1],"a\\u0000b":18446744073709551615,"only":{}},{},'
             b'{"a":1.5,"a":true,"a":false,"A":7}]')
DOCUMENTS = ["twitter.json", "citm_catalog.json", HAND_MADE]
VALUES, KEYS = 0, 1
CASES = [
    (0, VALUES, b"$.statuses[*].lang"), (0, VALUES, b"$.statuses[*].user.lang"), (0, VALUES, b"$.statuses[*].user.time_zone"), (0, VALUES, b"$.statuses[*].user.screen_name"),
    (0, VALUES, b"$.statuses[*].id"), (0, VALUES, b"$.statuses[*].entities.hashtags[*].text"), (0, VALUES, b"$.statuses[*].no_such_field"),
    (0, KEYS, b"$.statuses[*].user"), (0, KEYS, b"$.statuses[*]"), (0, KEYS, b"$.statuses[*].entities"), (0, KEYS, b"$.search_metadata"),
    (1, VALUES, b"$.performances[*].venueCode"), (1, VALUES, b"$.events.*.name"), (1, VALUES, b"$.events.*.logo"), (1, VALUES, b"$.performances[*].logo"),
    (1, VALUES, b"$.areaNames.*"), (1, KEYS, b"$.events.*"), (1, KEYS, b"$.performances[*]"), (1, KEYS, b"$.performances[*].seatCategories[*]"), (1, KEYS, b"$.events"),
    (2, VALUES, b"$[*]"), (2, KEYS, b"$[*]"), (2, VALUES, b"$[*].a"), (2, VALUES, b"$[*][*]"),
]


def document_bytes(d):
    return open(os.path.join(HERE, "jsonexamples", d), "rb").read() if isinstance(d, str) else d


def main():
    ref_inc = os.path.join(_paths.REFERENCE_DIR, "include")
    ref_dir = os.path.dirname(_paths.LIB_REF)
    docs = [document_bytes(d) for d in DOCUMENTS]
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "dictionary_golden")
        subprocess.run(["g++", "-O2", "-std=c++17", "-DSIMDJSON_THREADS_ENABLED=1", "-I", ref_inc, os.path.join(HERE, "dictionary_golden.cpp"), "-o", exe,
                        "-L", ref_dir, "-lsjref", "-lpthread", f"-Wl,-rpath,{ref_dir}"], check=True)
        blob = (struct.pack("<I", len(docs)) + b"".join(struct.pack("<I", len(x)) + x for x in docs) + struct.pack("<I", len(CASES)) +
                b"".join(struct.pack("<III", d, mode, len(p)) + p for d, mode, p in CASES))
        lines = subprocess.run([exe], input=blob, capture_output=True, check=True).stdout.decode().splitlines()
    at, cases = 0, []
    for d, mode, p in CASES:
        head = lines[at].split()
        at += 1
        assert head[0] == "C" and head[1] != "E", (p, head)
        cells, nulls, distinct = (int(x) for x in head[1:])
        entries = [line.split() for line in lines[at: at + distinct]]
        at += distinct
        codes = [] if lines[at] == "." else [int(x) for x in lines[at].split()]
        at += 1
        assert len(codes) == cells and codes.count(-1) == nulls
        cases.append({"document": d, "mode": mode, "path": p.hex(), "cells": cells, "nulls": nulls, "strings": ["" if e[0] == "-" else e[0] for e in entries],
                      "first": [int(e[1]) for e in entries], "counts": [int(e[2]) for e in entries], "kinds": [[int(x) for x in e[3:]] for e in entries], "codes": codes})
    assert at == len(lines)
    out = {"documents": [d if isinstance(d, str) else {"hex": d.hex()} for d in DOCUMENTS], "cases": cases}
    path = os.path.join(HERE, "dictionary.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    for c in cases:
        print(DOCUMENTS[c["document"]] if isinstance(DOCUMENTS[c["document"]], str) else "hand-made", "values" if c["mode"] == VALUES else "keys", bytes.fromhex(c["path"]).decode(),
              c["cells"], "cells,", c["nulls"], "nulls,", len(c["strings"]), "distinct")
    print(os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
