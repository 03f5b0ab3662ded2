#!/usr/bin/env python3
"""Generates tests/golden/json_text.json from the REAL reference: the JSON text of the elements of a column -- simdjson::minify(e) for every element e of
doc.at_path_with_wildcard(path), the path $ standing for the root element itself -- and the text of a table of doubles, simdjson::internal::to_chars (the yardstick of sjgpu_serialize_cells_device,
include/sjgpu_json.h, and of simdjson_amd/csrc/sj_dtoa.h).

Run where the reference lies (needs its headers and oracle/_ref/libsjref.so):   python tests/golden/make_json_text_golden.py

tests/golden/json_text_golden.cpp -- a small program of our own -- is compiled against them into a temporary directory and fed the documents, cases and doubles
below.  The fixture: "documents" (a file of tests/golden/jsonexamples by name, or the bytes as hex); per case "document", "path" (hex), "cells" and either "texts"
(hex, one per cell: a column of at most SMALL bytes) or "lengths" and "sha256" (of the texts back to back: the large columns); "doubles", one
string of lines "<bits as 16 hex digits> <text>" (the doubles whose text is worth reading), and "double_groups": the count and the SHA-256 of the texts, joined by
newlines, of each group of tests/json_text_cases.py's double_groups() -- the powers of two (the subnormal ones a group of their own) and of ten with their
neighbours, the random bit patterns and the doubles whose top byte is a tape tag, made by rule.
"""
import hashlib
import json
import os
import random
import struct
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

sys.path.insert(0, os.path.join(ROOT, "tests"))

from json_text_cases import bits_of, double_groups, group_digest  # noqa: E402
from simdjson_amd import _paths  # noqa: E402

SMALL = 6 << 10
CONTROLS = "".join("\\u%04x" % c for c in range(0x20))
# every escape class, keys with NUL and quotes, the empty containers and the empty string, nested empties, duplicate keys, the integers' extremes, -0.0, and doubles of
# every layout
HAND_MADE = (b'[{},[],"",[[]],[{}],[[],[]],{"":{}},{"a":[]},{"k\\u0000z":1,"q\\"uote":"\\\\","a":1,"a":2,"":""},"\\b\\t\\n\\f\\r","' + CONTROLS.encode() +
             b'","\\u007f\\/\\u00e9\\ud83d\\ude00 plain / text","\xc3\xa9\xe2\x82\xac\xf0\x9f\x98\x80","quote\\"back\\\\slash","0123456\\n","01234567\\t8",'
             b'-9223372036854775808,9223372036854775807,9223372036854775808,18446744073709551615,0,-1,10,-10,99999999999999999,-0.0,0.0,1e2,1.5e-7,1e-4,1e-5,0.00012345,'
             b'1e15,1e16,999999999999999.0,123456789012345.6,1234567890123456789012.0,1.7976931348623157e308,5e-324,2.2250738585072014e-308,0.1,0.30000000000000004,'
             b'true,false,null,{"nested":{"deep":[1,[2,[3,{"x":[{}],"y":[[]]}]]],"t":true,"n":null,"d":-2.5},"last":"z"}]')
DOCUMENTS = ["twitter.json", "citm_catalog.json", HAND_MADE]
CASES = [
    (0, b"$.statuses[*].entities"), (0, b"$.statuses[*].user"), (0, b"$.statuses[*]"), (0, b"$.statuses[*].text"), (0, b"$.statuses[*].id"), (0, b"$.search_metadata"), (0, b"$"),
    (0, b"$.statuses[*].no_such_field"),
    (1, b"$.events.*"), (1, b"$.performances[*].seatCategories"),
    (2, b"$[*]"), (2, b"$"), (2, b"$[*][*]"), (2, b"$[*].*"),
]


def double_table():
    """the explicit table: the doubles whose text a reader wants to see (the bulk is json_text_cases.double_groups(), kept as digests)"""
    bits = [1, 2, 0x000FFFFFFFFFFFFF, 0x0010000000000000, 0x7FEFFFFFFFFFFFFF, 0, 1 << 63, bits_of(-0.1), bits_of(-1e22), bits_of(-5e-324)]
    for text in ("1e-5", "9.999999999999999e-6", "1e-4", "0.00010000000000000002", "9.999999999999999e-5", "1e15", "999999999999999.9", "1e16", "9999999999999998.0",
                 "1000000000000001.0", "0.001", "0.01", "0.5", "1.0", "2.0", "3.0", "7e22", "9e15", "123456789012345.0", "12345678901234.5", "1.5", "0.3", "1.0000000000000002",
                 "4.35", "0.000123456789012345", "5e-5", "123.0", "1234567890123456.0", "12345678901234567.0", "1.2345678901234567", "0.12345678901234566", "9007199254740993.0"):
        bits.append(bits_of(float(text)))
    for digits in (1, 15, 16, 17):
        rng = random.Random(digits)
        for _ in range(40):
            bits.append(bits_of(float("%d.%se%d" % (rng.randint(1, 9), "".join(str(rng.randint(1, 9)) for _ in range(digits - 1)) or "0", rng.randint(-300, 300)))))
    return bits


def document_bytes(d):
    return open(os.path.join(HERE, "jsonexamples", d), "rb").read() if isinstance(d, str) else d


def main():
    ref_inc = os.path.join(_paths.REFERENCE_DIR, "include")
    ref_dir = os.path.dirname(_paths.LIB_REF)
    docs = [document_bytes(d) for d in DOCUMENTS]
    explicit, groups = double_table(), double_groups()
    doubles = explicit + [b for g in groups.values() for b in g]
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "json_text_golden")
        subprocess.run(["g++", "-O2", "-std=c++17", "-DSIMDJSON_THREADS_ENABLED=1", "-I", ref_inc, os.path.join(HERE, "json_text_golden.cpp"), "-o", exe,
                        "-L", ref_dir, "-lsjref", "-lpthread", f"-Wl,-rpath,{ref_dir}"], check=True)
        blob = (struct.pack("<I", len(docs)) + b"".join(struct.pack("<I", len(x)) + x for x in docs) + struct.pack("<I", len(CASES)) +
                b"".join(struct.pack("<II", d, len(p)) + p for d, p in CASES) + struct.pack("<I", len(doubles)) + b"".join(struct.pack("<Q", b) for b in doubles))
        lines = subprocess.run([exe], input=blob, capture_output=True, check=True).stdout.decode().splitlines()
    at, cases = 0, []
    for d, p in CASES:
        head = lines[at].split()
        at += 1
        assert head[0] == "C" and head[1] != "E", (p, head)
        cells = int(head[1])
        texts = [bytes.fromhex(line) for line in lines[at: at + cells]]
        at += cells
        case = {"document": d, "path": p.hex(), "cells": cells}
        if sum(len(t) for t in texts) <= SMALL:
            case["texts"] = [t.hex() for t in texts]
        else:
            case["lengths"] = [len(t) for t in texts]
            case["sha256"] = hashlib.sha256(b"".join(texts)).hexdigest()
        cases.append(case)
    texts = []
    for b in doubles:
        tag, bits, text = lines[at].split()
        at += 1
        assert tag == "D" and int(bits, 16) == b
        texts.append(text)
    assert at == len(lines)
    table = [f"{b:016x} {t}" for b, t in zip(explicit, texts)]
    digests, first = {}, len(explicit)
    for name, g in groups.items():
        digests[name] = {"count": len(g), "sha256": group_digest([t.encode() for t in texts[first: first + len(g)]])}
        first += len(g)
    out = {"documents": [d if isinstance(d, str) else {"hex": d.hex()} for d in DOCUMENTS], "cases": cases, "doubles": "\n".join(table), "double_groups": digests}
    path = os.path.join(HERE, "json_text.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    for c in cases:
        print(DOCUMENTS[c["document"]] if isinstance(DOCUMENTS[c["document"]], str) else "hand-made", bytes.fromhex(c["path"]).decode(), c["cells"], "cells,",
              "texts" if "texts" in c else "lengths + digest")
    print(len(table), "doubles in the table,", sum(d["count"] for d in digests.values()), "in the groups;", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
