#!/usr/bin/env python3
"""Generates tests/golden/pivot.json from the REAL reference: what element::at_key(k) and element::at_key_case_insensitive(k) answer for every record of the
small NDJSON record sets below and every key of each set's list (the yardstick of sjgpu_pivot_fields_device, include/sjgpu_pivot.h, and of
simdjson_amd/pivot.py's records_many).

Run where the reference lies (needs its headers and oracle/_ref/libsjref.so):   python tests/golden/make_pivot_golden.py

tests/golden/pivot_golden.cpp -- a small program of our own -- is compiled against them into a temporary directory and fed the sets.  The keys of a set are
every distinct key of its records (unescaped, in order of first occurrence: Python's json with object_pairs_hook, which keeps duplicates) and the ABSENT ones
below.  The sets hold duplicate keys, "\\u0041" beside "A", the empty key, keys with / and ~, keys with an embedded NUL that differ only behind it, ID / Id / id
in one row and across rows, a key with a byte >= 0x80 in two cases, rows that are arrays, scalars and null, an empty object, and nested objects as values.
The fixture: "answers": the distinct answers, "E <code>" or "V <minify(element)>"; "sets"[s]: "records" and "keys" as hex, and "at_key" / "at_key_ci"
[record][key]: an index into "answers".
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

SETS = [
    [b'{"a":1,"a":2}',
     b'{"\\u0041":"escaped","A":"plain","a":3}',
     b'{"":"empty","/":"slash","~":"tilde","a/b":1,"m~n":2,"~0":3,"~1":4}',
     b'{"a\\u0000b":1,"A\\u0000c":2,"a\\u0000c":3}',
     b'{"ID":1,"Id":2,"id":3}',
     b'{"id":4}',
     b'{"Id":5,"x":{"ID":6,"id":[1,2]}}',
     b'{"iD":7,"ID":8}',
     b'{"\xc3\xa9":1,"\xc3\x89":2,"\xc3\xa9X":3,"\xc3\xa9x":4}',
     b'[1,2]',
     b'"str"',
     b'7',
     b'null',
     b'{}',
     b'{"o":{"p":{"q":[]}},"arr":[{"k":"v"}],"t":true,"n":null,"s":"text","d":-1.5}',
     b'true',
     b'{"A\\u0000c":"first","a\\u0000b":"second","X":{"a":{}},"x":0}'],
    [b'{"id":1,"name":"one","ok":true,"tags":["a","b"],"score":0.5}',
     b'{"id":2,"name":"two","ok":false,"tags":[],"score":2}',
     b'{"name":"three","id":3,"extra":{"deep":{"er":null}}}',
     b'{"id":18446744073709551615,"name":null}',
     b'{"id":-4,"NAME":"four","Name":"FOUR","ok":true}'],
    [b'[{"a":1}]', b'2', b'"a"', b'null'],
]
ABSENT = [b"absent", b"A\0B", b"a\0", b"ID ", b"\xc3\x89x", b"NAME", b"Tags", b"a/B", b"M~N"]


def keys_of(records):
    seen = {}
    for r in records:
        if r[:1] == b"{":  # the root's own keys alone: what lies deeper is a value
            for k, _ in json.loads(r.decode("utf-8"), object_pairs_hook=lambda pairs: pairs):
                seen.setdefault(k.encode("utf-8"), None)
    return list(seen) + [k for k in ABSENT if k not in seen]


def main():
    ref_inc = os.path.join(_paths.REFERENCE_DIR, "include")
    ref_dir = os.path.dirname(_paths.LIB_REF)
    keys = [keys_of(records) for records in SETS]
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "pivot_golden")
        subprocess.run(["g++", "-O1", "-std=c++17", "-DSIMDJSON_THREADS_ENABLED=1", "-I", ref_inc, os.path.join(HERE, "pivot_golden.cpp"), "-o", exe,
                        "-L", ref_dir, "-lsjref", "-lpthread", f"-Wl,-rpath,{ref_dir}"], check=True)
        blob = struct.pack("<I", len(SETS))
        for records, ks in zip(SETS, keys):
            blob += struct.pack("<II", len(records), len(ks)) + b"".join(struct.pack("<I", len(x)) + x for x in records + ks)
        lines = subprocess.run([exe], input=blob, capture_output=True, check=True).stdout.decode("utf-8").split("\n")[:-1]
    answers, sets, at = {}, [], 0
    for records, ks in zip(SETS, keys):
        plain, folded = [], []
        for _ in records:
            both = [answers.setdefault(line, len(answers)) for line in lines[at: at + 2 * len(ks)]]
            at += 2 * len(ks)
            plain.append(both[0::2])
            folded.append(both[1::2])
        sets.append({"records": [r.hex() for r in records], "keys": [k.hex() for k in ks], "at_key": plain, "at_key_ci": folded})
    assert at == len(lines), (at, len(lines))
    out = {"answers": list(answers), "sets": sets}
    path = os.path.join(HERE, "pivot.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    codes = sorted({a for a in answers if a[0] == "E"})
    print(len(SETS), "sets,", sum(len(s) for s in SETS), "records,", sum(len(k) for k in keys), "keys,", len(answers), "distinct answers,", codes, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
