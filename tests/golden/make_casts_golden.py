#!/usr/bin/env python3
"""Generates tests/golden/casts.json from the REAL reference: what dom::parser::parse(`[X]`).at_pointer(p).get_int64() and its six siblings
(get_uint64, get_double, get_bool, get_string, get_array, get_object) return for the values X and the pointers p below -- the element itself and
results that failed on the way (the yardstick of sjgpu_cast_cells_device, include/sjgpu_cast.h).

Run where the reference lies (needs its headers and oracle/_ref/libsjref.so):   python tests/golden/make_casts_golden.py

tests/golden/casts_golden.cpp -- a small program of our own -- is compiled against them into a temporary directory, fed the lists and asked getter by
getter.  The fixture: "values" and "pointers" as hex, "getters" (the order of the answers), and "table"[value]: "P <code>" where the reference rejects
`[X]`, else per pointer an index into "rows", the distinct answers.  A row is seven answers joined by `;`:
    "E <code>" | 16 hex digits (the 64 bits of the int64 / uint64 / double; a bool is 1 or 0) | "S <hex bytes>" | "A <elements>" | "O <fields>"
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

VALUES = [
    b"0", b"-1", b"9223372036854775807", b"9223372036854775808", b"9223372036854775809", b"18446744073709551615", b"18446744073709551616",
    b"-9223372036854775808",
    # the doubles' integers end at 2^53: round to nearest even on both sides, and at the top of the u range
    b"9007199254740992", b"9007199254740993", b"-9007199254740993", b"18446744073709549568", b"18446744073709550591", b"18446744073709550592",
    b"1e19", b"-0.0", b"1.5", b"5e-324", b"1.7976931348623157e308",
    b"true", b"false", b"null", b'""', b'"abc"', b"[]", b"{}", b"[1]", b'{"a":1}',
]
# the element; beyond the array (19); a field of it (20 for an object, what a scalar or an array answers otherwise); two malformed ones
POINTERS = [b"/0", b"/1", b"/0/x", b"/~", b"x"]
GETTERS = ["int64", "uint64", "double", "bool", "string", "array", "object"]


def main():
    ref_inc = os.path.join(_paths.REFERENCE_DIR, "include")
    ref_dir = os.path.dirname(_paths.LIB_REF)
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "casts_golden")
        subprocess.run(["g++", "-O1", "-std=c++17", "-DSIMDJSON_THREADS_ENABLED=1", "-I", ref_inc, os.path.join(HERE, "casts_golden.cpp"), "-o", exe,
                        "-L", ref_dir, "-lsjref", "-lpthread", f"-Wl,-rpath,{ref_dir}"], check=True)
        blob = struct.pack("<II", len(VALUES), len(POINTERS)) + b"".join(struct.pack("<I", len(x)) + x for x in VALUES + POINTERS)
        lines = subprocess.run([exe], input=blob, capture_output=True, check=True).stdout.decode().splitlines()
    at = 0
    table, distinct = [], {}
    for _ in VALUES:
        if lines[at].startswith("P "):
            table.append(lines[at])
            at += 1
            continue
        table.append([distinct.setdefault(lines[at + j], len(distinct)) for j in range(len(POINTERS))])
        at += len(POINTERS)
    assert at == len(lines)
    out = {"values": [x.hex() for x in VALUES], "pointers": [p.hex() for p in POINTERS], "getters": GETTERS, "rows": list(distinct), "table": table}
    path = os.path.join(HERE, "casts.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    answers = {}
    for row in distinct:
        for a in row.split(";"):
            kind = a if a[0] == "E" else a[0] if a[0] in "SAO" else "bits"
            answers[kind] = answers.get(kind, 0) + 1
    print(len(VALUES), "values x", len(POINTERS), "pointers x", len(GETTERS), "getters,", len(distinct), "distinct rows,", os.path.getsize(path), "bytes;",
          sum(isinstance(t, str) for t in table), "rejected;", dict(sorted(answers.items())))


if __name__ == "__main__":
    main()
