#!/usr/bin/env python3
"""Generates tests/golden/nested_write.json from the REAL reference: the nested JSON simdjson::builder::string_builder writes for the tables of
tests/nested_write_cases.py (fixture_tables()), under every legal combination of the four flags (the yardstick of sjgpu_write_nested_device,
include/sjgpu_nested.h).

Run where the reference lies (needs its headers and oracle/_ref/libsjref.so):   python tests/golden/make_nested_write_golden.py

tests/golden/nested_write_golden.cpp -- a small program of our own -- is compiled against them into a temporary directory (-std=c++20: the builder's append(range)
and append(optional) stand on concepts) and fed the tables.  The fixture: per table "name", "rows", "fields", the "blob_sha256" of the bytes the program was fed, and
per flags either "texts" (hex, one per row) or, above SMALL bytes, "lengths" and "sha256" (of the texts back to back).  Doubles that are not finite are not in it:
the reference has no text for them, and tests/nested_write_model.py covers them by rule."""
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

from simdjson_amd import _paths  # noqa: E402
from nested_write_cases import SMALL, fixture_tables, legal_flags, table_blob  # noqa: E402


def main():
    ref_inc = os.path.join(_paths.REFERENCE_DIR, "include")
    ref_dir = os.path.dirname(_paths.LIB_REF)
    tables = fixture_tables()
    blobs = [table_blob(t) for t in tables]
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "nested_write_golden")
        subprocess.run(["g++", "-O2", "-std=c++20", "-DSIMDJSON_THREADS_ENABLED=1", "-I", ref_inc, os.path.join(HERE, "nested_write_golden.cpp"), "-o", exe,
                        "-L", ref_dir, "-lsjref", "-lpthread", f"-Wl,-rpath,{ref_dir}"], check=True)
        lines = subprocess.run([exe], input=struct.pack("<I", len(tables)) + b"".join(blobs), capture_output=True, check=True).stdout.decode().split("\n")
    at, out = 0, []
    for i, (t, blob) in enumerate(zip(tables, blobs)):
        entry = {"name": t["name"], "rows": t["n"], "fields": len(t["fields"]), "blob_sha256": hashlib.sha256(blob).hexdigest(), "flags": {}}
        for flags in sorted(legal_flags(len(t["fields"]))):
            assert lines[at].split() == ["T", str(i), str(flags)], lines[at]
            texts = [bytes.fromhex(x) for x in lines[at + 1: at + 1 + t["n"]]]
            at += 1 + t["n"]
            assert all(texts) or flags & 9 == 9  # (only a bare row that was left out is empty)
            if sum(len(x) for x in texts) <= SMALL:
                entry["flags"][str(flags)] = {"texts": [x.hex() for x in texts]}
            else:
                entry["flags"][str(flags)] = {"lengths": [len(x) for x in texts], "sha256": hashlib.sha256(b"".join(texts)).hexdigest()}
        out.append(entry)
        print(t["name"], t["n"], "rows,", len(t["fields"]), "fields:", ", ".join("texts" if "texts" in f else "lengths + digest" for f in entry["flags"].values()))
    assert lines[at:] == [""], lines[at:][:3]
    path = os.path.join(HERE, "nested_write.json")
    with open(path, "w") as f:
        json.dump({"tables": out}, f, separators=(",", ":"))
    print(os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
