#!/usr/bin/env python3
"""Generates tests/golden/write_records.json from the REAL reference: the JSON records simdjson::builder::string_builder writes for the tables of
tests/write_records_cases.py (fixture_tables()), under the four combinations of the two flags (the yardstick of sjgpu_write_records_device, include/sjgpu_write.h).

Run where the reference lies (needs its headers and oracle/_ref/libsjref.so):   python tests/golden/make_write_records_golden.py

tests/golden/write_records_golden.cpp -- a small program of our own -- is compiled against them into a temporary directory (-std=c++17: string_builder needs no
concepts) and fed the tables.  The fixture: per table "name", "rows", "columns", the bytes the program was fed -- "blob" as hex, or "blob_bytes" for a table above SMALL
bytes -- with their "blob_sha256", and per flags either "texts" (hex, one per row) or, above SMALL bytes, "lengths" and "sha256" (of the texts back to back).
Doubles that are not finite are not in it: the reference has no text for them, and tests/write_records_model.py covers them by rule."""
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
from write_records_cases import ALL_FLAGS, SMALL, fixture_tables, table_blob  # noqa: E402


def main():
    ref_inc = os.path.join(_paths.REFERENCE_DIR, "include")
    ref_dir = os.path.dirname(_paths.LIB_REF)
    tables = fixture_tables()
    blobs = [table_blob(t) for t in tables]
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "write_records_golden")
        subprocess.run(["g++", "-O2", "-std=c++17", "-DSIMDJSON_THREADS_ENABLED=1", "-I", ref_inc, os.path.join(HERE, "write_records_golden.cpp"), "-o", exe,
                        "-L", ref_dir, "-lsjref", "-lpthread", f"-Wl,-rpath,{ref_dir}"], check=True)
        lines = subprocess.run([exe], input=struct.pack("<I", len(tables)) + b"".join(blobs), capture_output=True, check=True).stdout.decode().splitlines()
    at, out = 0, []
    for i, (t, blob) in enumerate(zip(tables, blobs)):
        entry = {"name": t["name"], "rows": t["n"], "columns": len(t["columns"]), "blob_sha256": hashlib.sha256(blob).hexdigest(), "flags": {}}
        if len(blob) <= SMALL:
            entry["blob"] = blob.hex()
        else:
            entry["blob_bytes"] = len(blob)
        for flags in ALL_FLAGS:
            assert lines[at].split() == ["T", str(i), str(flags)], lines[at]
            texts = [bytes.fromhex(x) for x in lines[at + 1: at + 1 + t["n"]]]
            at += 1 + t["n"]
            assert all(texts)
            if sum(len(x) for x in texts) <= SMALL:
                entry["flags"][str(flags)] = {"texts": [x.hex() for x in texts]}
            else:
                entry["flags"][str(flags)] = {"lengths": [len(x) for x in texts], "sha256": hashlib.sha256(b"".join(texts)).hexdigest()}
        out.append(entry)
        print(t["name"], t["n"], "rows,", len(t["columns"]), "columns:", ", ".join("texts" if "texts" in f else "lengths + digest" for f in entry["flags"].values()))
    assert at == len(lines)
    path = os.path.join(HERE, "write_records.json")
    with open(path, "w") as f:
        json.dump({"tables": out}, f, separators=(",", ":"))
    print(os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
