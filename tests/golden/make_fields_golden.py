#!/usr/bin/env python3
"""Generates tests/golden/fields.json from the REAL reference: what e.get_object() and `for (dom::key_value_pair f : object)` give, and what size() gives,
for every element e of dom::parser::parse(document).at_path_with_wildcard(p), for the documents and row paths p below (the yardstick of
sjgpu_object_fields_from_cells_device and sjgpu_cell_sizes_device, include/sjgpu_fields.h); and dom::array::size() of three arrays around the saturation
of the tape's count field, of which only the three numbers are kept.

Run where the reference lies (needs its headers and oracle/_ref/libsjref.so):   python tests/golden/make_fields_golden.py

tests/golden/fields_golden.cpp -- a small program of our own -- is compiled against them into a temporary directory and fed the lists.  The documents are
those of tests/golden/make_lists_golden.py and the EXTRA ones below; the row paths are its ROW_PATHS.  The fixture: "documents" and "row_paths" as hex,
"tables"[document][row path]: "E <code>" where the row path failed, else one entry per row: an index into "rows", the distinct rows.  A row is
    "<size> E <code>" | "<size> F" + ";<key as hex>:<value>" per field, in the reference's order
the value as tests/golden/paths.json renders a match, <size> what size() returns for an object or array row and 17 for a scalar row; and
"array_sizes": {elements: dom::array::size()} for 0xFFFFFE, 0xFFFFFF and 0x1000000 elements.
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
from make_lists_golden import ROW_PATHS  # noqa: E402
from make_paths_golden import DOCUMENTS  # noqa: E402

WIDE_OBJECT = b"{" + b",".join(b'"k%03d":%s' % (i, (b"%d" % i, b'"v%d"' % i, b"[%d]" % i, b'{"i":%d}' % i, b"null", b"-%d.5" % i)[i % 6]) for i in range(300)) + b"}"
KEYS = (b'{"":0,"\\u0000":1,"a\\u0000b":2,"line\\nfeed":3,"q\\"uote":4,"sl\\/ash":5,"\\ud83d\\ude00":6,"\xc3\xa9\xe2\x82\xac\xf0\x9f\x98\x80":7,'
        b'"tab\\tback\\\\slash":8}')

EXTRA = [
    # `$[*]`: an array of mixed rows -- objects of every shape, an array, every scalar
    b'[{},{"one":1},{"d":1,"d":2,"e":3,"d":"again"},' + KEYS + b',{"o":{"p":{"q":{}},"r":[{"s":1}]},"t":[[]],"u":{}},[1,{"x":2},[3]],[],"str","",0,-1,18446744073709551615,1.5,-0.0,'
    b'true,false,null]',
    b"[" + WIDE_OBJECT + b",{}]",
    # `$.*` and `$.*.*`: objects nested as values
    b'{"a":{"b":{"c":1,"d":{"e":[1,2]}},"b2":{}},"z":{"y":{"x":null}},"n":7,"l":[{"k":1},{}]}',
    b'{"statuses":[{"en":"hello","de":"hallo","":"none"},{"counts":{"u1":3,"u2":4,"u1":5}},[{"h":1}],{}]}',
    b"{}",
    b'{"only":{"f":true}}',
    # every kind of value behind a key
    b'[{"l":-5,"u":18446744073709551615,"d":2.5,"t":true,"f":false,"n":null,"s":"text","o":{"k":"v"},"a":[1,"two"]}]',
]


def main():
    docs = DOCUMENTS + EXTRA
    ref_inc = os.path.join(_paths.REFERENCE_DIR, "include")
    ref_dir = os.path.dirname(_paths.LIB_REF)
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "fields_golden")
        subprocess.run(["g++", "-O2", "-std=c++17", "-DSIMDJSON_THREADS_ENABLED=1", "-I", ref_inc, os.path.join(HERE, "fields_golden.cpp"), "-o", exe,
                        "-L", ref_dir, "-lsjref", "-lpthread", f"-Wl,-rpath,{ref_dir}"], check=True)
        blob = struct.pack("<II", len(docs), len(ROW_PATHS)) + b"".join(struct.pack("<I", len(x)) + x for x in docs + ROW_PATHS)
        lines = subprocess.run([exe], input=blob, capture_output=True, check=True).stdout.decode().splitlines()
    at = 0
    tables, distinct = [], {}
    for _ in docs:
        per_doc = []
        for _ in ROW_PATHS:
            head = lines[at]
            at += 1
            assert head.startswith("R "), head
            if head.startswith("R E "):
                per_doc.append(head[2:])
                continue
            rows = int(head[2:])
            per_doc.append([distinct.setdefault(line, len(distinct)) for line in lines[at: at + rows]])
            at += rows
        tables.append(per_doc)
    array_sizes = {}
    for line in lines[at:]:
        a, n, size = line.split()
        assert a == "A"
        array_sizes[n] = int(size)
    assert sorted(array_sizes) == sorted(str(n) for n in (0xFFFFFE, 0xFFFFFF, 0x1000000)), array_sizes
    out = {"documents": [d.hex() for d in docs], "row_paths": [p.hex() for p in ROW_PATHS], "rows": list(distinct), "tables": tables, "array_sizes": array_sizes}
    path = os.path.join(HERE, "fields.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    rows = sum(len(t) for per_doc in tables for t in per_doc if not isinstance(t, str))
    kinds = {}
    for line in distinct:
        body = line.split(" ", 1)[1]
        kind = body if body[0] == "E" else ("F none" if body == "F" else "F some")
        kinds[kind] = kinds.get(kind, 0) + 1
    print(len(docs), "documents x", len(ROW_PATHS), "row paths,", rows, "rows", f"({len(distinct)} distinct),", os.path.getsize(path), "bytes;", dict(sorted(kinds.items())),
          array_sizes)


if __name__ == "__main__":
    main()
