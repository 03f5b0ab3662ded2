#!/usr/bin/env python3
"""Generates tests/golden/lists.json from the REAL reference: what e.at_path_with_wildcard(q) returns for every element e of
dom::parser::parse(document).at_path_with_wildcard(p), for the documents, row paths p and child paths q below (the yardstick of
sjgpu_at_paths_from_cells_device, include/sjgpu_lists.h).

Run where the reference lies (needs its headers and oracle/_ref/libsjref.so):   python tests/golden/make_lists_golden.py

tests/golden/lists_golden.cpp -- a small program of our own -- is compiled against them into a temporary directory, fed the lists and asked cell by
cell.  The documents are those of tests/golden/make_paths_golden.py.  The fixture: "documents", "row_paths" and "paths" as hex, and
"tables"[document][row path]: "E <code>" where the row path failed, else one entry per row: an index into "rows", the distinct rows (most rows are
scalars and answer every path alike).  A row is the list of its cells in the order of "paths", a cell as tests/golden/paths.json records it:
    "E <code>" | "M" + ";<match>" per match, in the reference's order
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
sys.path.insert(0, HERE)

from simdjson_amd import _paths  # noqa: E402
from make_paths_golden import DOCUMENTS  # noqa: E402

ROW_PATHS = [b"$[*]", b"$.*", b"$.a[*]", b"$.statuses[*]", b"$.*.*"]

PATHS = [
    # lists below a row, with and without `$`
    b"$[*]", b"[*]", b"$.*", b".*", b"$.tags[*]", b".tags[*]", b"$.c[*]", b"$.b[*]", b"$.user.*", b"$.*.*", b"$[*][*]", b"$[*].b", b"$.*[*]", b"$[*][0]",
    # no wildcard: one match or the pointer's code, at depth 0 of the ROW
    b"$.b", b".b", b"$.user.id", b"$[0]", b"[1]", b"$.x", b"$[-]", b"$[01]", b"$.user.name",
    # malformed and empty: 22 for a container row, nothing for a scalar row
    b"", b"$", b"b[*]", b"$..b", b"$[0][*]", b"$.b[", b"$[*", b"$.[*]", b"$*",
]


def main():
    paths = list(dict.fromkeys(PATHS))
    ref_inc = os.path.join(_paths.REFERENCE_DIR, "include")
    ref_dir = os.path.dirname(_paths.LIB_REF)
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "lists_golden")
        subprocess.run(["g++", "-O1", "-std=c++17", "-DSIMDJSON_THREADS_ENABLED=1", "-I", ref_inc, os.path.join(HERE, "lists_golden.cpp"), "-o", exe,
                        "-L", ref_dir, "-lsjref", "-lpthread", f"-Wl,-rpath,{ref_dir}"], check=True)
        blob = struct.pack("<III", len(DOCUMENTS), len(ROW_PATHS), len(paths)) + b"".join(struct.pack("<I", len(x)) + x for x in DOCUMENTS + ROW_PATHS + paths)
        lines = subprocess.run([exe], input=blob, capture_output=True, check=True).stdout.decode().splitlines()
    at = 0
    tables, distinct = [], {}
    for _ in DOCUMENTS:
        per_doc = []
        for _ in ROW_PATHS:
            head = lines[at]
            at += 1
            assert head.startswith("R "), head
            if head.startswith("R E "):
                per_doc.append(head[2:])
                continue
            rows = int(head[2:])
            per_doc.append([distinct.setdefault(tuple(lines[at + r * len(paths): at + (r + 1) * len(paths)]), len(distinct)) for r in range(rows)])
            at += rows * len(paths)
        tables.append(per_doc)
    assert at == len(lines)
    out = {"documents": [d.hex() for d in DOCUMENTS], "row_paths": [p.hex() for p in ROW_PATHS], "paths": [p.hex() for p in paths], "rows": [list(r) for r in distinct],
           "tables": tables}
    path = os.path.join(HERE, "lists.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    kinds = {}
    rows = 0
    for per_doc in tables:
        for t in per_doc:
            if isinstance(t, str):
                continue
            rows += len(t)
            for row in t:
                for c in out["rows"][row]:
                    kind = c if c[0] == "E" else ("M none" if c == "M" else ("M one" if c.count(";") == 1 else "M more"))
                    kinds[kind] = kinds.get(kind, 0) + 1
    print(len(DOCUMENTS), "documents x", len(ROW_PATHS), "row paths,", rows, "rows", f"({len(distinct)} distinct) x", len(paths), "paths,", os.path.getsize(path), "bytes;", dict(sorted(kinds.items())))


if __name__ == "__main__":
    main()
