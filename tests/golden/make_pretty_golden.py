#!/usr/bin/env python3
"""Generates tests/golden/pretty.json from the REAL reference: the indented JSON text of the elements of a column -- simdjson::prettify(e) for every element e of
doc.at_path_with_wildcard(path), the path $ standing for the root element itself (the yardstick of sjgpu_prettify_cells_device and
sjgpu_prettify_cells_wide_device, include/sjgpu_pretty.h).

Run where the reference lies (needs its headers and oracle/_ref/libsjref.so):   python tests/golden/make_pretty_golden.py

tests/golden/pretty_golden.cpp -- a small program of our own -- is compiled against them into a temporary directory and fed the documents and cases below: the three
documents and the fourteen cases of tests/golden/make_json_text_golden.py, and behind them the chains of tests/pretty_cases.py -- documents made by hand whose leaf
lies 14, 15, 16, 17, 31, 32, 33 and 65 containers deep, one document per level (the array of its twelve chains), asked for `$[*]`: every chain a cell.  The fixture: "documents" (a file of tests/golden/jsonexamples by name, the bytes
as hex, or "chains_of_level": pretty_cases.chain_document of that level); per case "document", "path" (hex), "cells" and either "texts" (hex, one per cell: a column of at most SMALL bytes) or "lengths" and "sha256" (of the texts
back to back: the large columns)."""
import hashlib
import json
import os
import struct
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

from make_json_text_golden import CASES as TEXT_CASES, DOCUMENTS as TEXT_DOCUMENTS, document_bytes  # noqa: E402
from pretty_cases import CHAIN_LEVELS, chain_document  # noqa: E402
from simdjson_amd import _paths  # noqa: E402

SMALL = 6 << 10
DOCUMENTS = list(TEXT_DOCUMENTS) + [chain_document(level) for level in CHAIN_LEVELS]
CASES = list(TEXT_CASES) + [(d, b"$[*]") for d in range(len(TEXT_DOCUMENTS), len(DOCUMENTS))]


def main():
    ref_inc = os.path.join(_paths.REFERENCE_DIR, "include")
    ref_dir = os.path.dirname(_paths.LIB_REF)
    docs = [document_bytes(d) for d in DOCUMENTS]
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "pretty_golden")
        subprocess.run(["g++", "-O2", "-std=c++17", "-DSIMDJSON_THREADS_ENABLED=1", "-I", ref_inc, os.path.join(HERE, "pretty_golden.cpp"), "-o", exe,
                        "-L", ref_dir, "-lsjref", "-lpthread", f"-Wl,-rpath,{ref_dir}"], check=True)
        blob = (struct.pack("<I", len(docs)) + b"".join(struct.pack("<I", len(x)) + x for x in docs) + struct.pack("<I", len(CASES)) +
                b"".join(struct.pack("<II", d, len(p)) + p for d, p in CASES))
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
    assert at == len(lines)
    named = [d if isinstance(d, str) else {"hex": d.hex()} for d in TEXT_DOCUMENTS] + [{"chains_of_level": level} for level in CHAIN_LEVELS]  # (made by rule: the rule's name)
    out = {"documents": named, "cases": cases}
    path = os.path.join(HERE, "pretty.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print(len(cases), "cases,", sum("texts" in c for c in cases), "as texts;", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
