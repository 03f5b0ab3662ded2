#!/usr/bin/env python3
"""Generates tests/golden/paths.json from the REAL reference: what dom::parser::parse(document).at_path_with_wildcard(path) returns for every
document x path below (the yardstick of sjgpu_at_paths_device, include/sjgpu_paths.h).

Run where the reference lies (needs its headers and oracle/_ref/libsjref.so):   python tests/golden/make_paths_golden.py

tests/golden/paths_golden.cpp -- a small program of our own -- is compiled against them into a temporary directory, fed the lists and asked cell by
cell.  The fixture: "documents" and "paths" as hex, "cells"[document][path] as the program printed them:
    "E <code>" | "M" + ";<match>" per match, in the reference's order, a match rendered as tests/golden/pointers.json renders a cell
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

PROBE_OBJECT = b'{"a":[{"b":1,"c":[1,2]},{"b":2},{"x":3},5],"k":{"p":{"b":7},"q":{"b":8}},"s*":1,"e":[],"o":{}}'
PROBE_ARRAY = b'[[1,2],[3],{"b":[4]},6]'
NINE_DEEP = b"[" * 8 + b"[1,2],[3]" + b"]" * 8  # the innermost arrays lie nine levels deep

DOCUMENTS = [
    # every kind of root
    b"{}", b"[]", b'"str"', b"12", b"-5", b"18446744073709551615", b"1.5", b"true", b"false", b"null",
    # the two probes whose answers the header's table quotes
    PROBE_OBJECT, PROBE_ARRAY,
    # duplicate keys under a wildcard: get_values gives every field, at_pointer the first
    b'{"a":1,"a":2,"b":{"x":1,"x":2},"b":{"x":3},"k":[1],"k":[2,3]}',
    # escaped, `~`, `/`, empty and multi-byte keys as PTR keys
    '{"a/b":{"x":1},"m~n":{"x":2},"":{"x":3},"é":{"x":4},"a\\u0062":{"x":5},"q\\"r":{"x":6},"日本":[7,8],"a":{"b":{"x":9}}}'.encode(),
    # the bracket-quoted forms, and keys that hold their punctuation
    b'{"k":[1,2],"\'k\'":[3],"k\']":[4],"a":{"k":[5,6]},"k[*]":[7]}',
    # leading-zero, `-` and overflowing indices as keys, asked of arrays and of objects
    b'{"a":[[1,2],[3,4]],"01":{"x":1},"-":[5],"0":[6],"99999999999999999999":[7]}',
    b'[[10,11],[20],[[30]],"s"]',
    # empty containers on the way
    b'{"a":[],"b":{},"c":[[],{},[1]],"d":{"e":[],"f":{"g":[]}},"k":{}}',
    b"[[],{},[[]],[{}]]",
    # numbers whose value word looks like a tape word, under a wildcard (the value-word documents of make_pointers_golden.py)
    b'[8863084066665136133,"x",{"k":1}]',
    b'[2.2181357552966544e+130,"x",{"k":2}]',
    b'{"n":8863084066665136133,"d":2.2181357552966544e+130,"k":"behind"}',
    b'{"a":[8863084066665136133,2.2181357552966544e+130,{"b":8863084066665136133}],"k":{"p":2.2181357552966544e+130}}',
    # eight nested wildcards
    NINE_DEEP,
    b'{"a":[{"b":[{"c":[{"d":[{"e":[1,"x"]}]}]}]}]}',
    # records
    b'{"id":7,"name":"user7","ok":true,"tags":["a","b\\n"],"score":7.5}',
    b'[7,"x7",null,{"k":[]},-1e7]',
    b'{"a":{"b":{"c":[4,{"d":"\\u00e94"}]}}}',
    b'{"e":"","f":[[],[[]],{}],"g":5}',
    b'{"statuses":[{"user":{"id":1,"name":"a"},"tags":["x","y"]},{"user":{"id":2},"tags":[]},{"nouser":1},7]}',
    b'{"items":[{"price":1.5},{"price":2},{"name":"n"}],"tags":["a","b"]}',
    # whitespace changes nothing
    b' { "a" : [ { "b" : 1 } , { "b" : [ 2 ] } ] , "k" : { "p" : { "b" : 7 } } } ',
    # the rest of the kinds as matches
    b'[{"b":1},[{"b":2}],"b",{"b":[1,2]}]',
    b'{"a":[-1,1e308,9223372036854775808,-9223372036854775808,true,false,null]}',
    b'{"a":["","\\u0000","\\ud83d\\ude00"],"k":{"p":""}}',
    b'{"t":true,"f":false,"n":null,"s":"str","d":2.5}',
    b'{"0":[["a","b"],["c"]],"1":[[],[[]],{}]}',
    b'{"a":{"a":{"a":{"a":"deep"}}}}',
    b'[[[1,[2]],[3]],[[4]],5,[6,[7,[8]]]]',
    b'{"a":{"1":{"x":"object"}},"b":[0,{"x":"array"}]}',
]

PATHS = [
    # the rows of the issue's table
    b"$.a[*].b", b"$.k.*.b", b"$.k[*].b", b"$.a[*].c[*]", b"$.*.*", b"$.a[*].c[0]", b"$.a.1.*", b"$.a/1.*", b".a[*].b", b"$.a[0].b", b"$.a[0].c[*]", b"$.s*",
    b"$.a[*]['b']", b"$['a'][*]['b']", b"$.a[*]x", b"$.a[*", b"$.a[*].b.z", b"$.missing[*]", b"$.e[*]", b"$.o.*", b"$.missing", b"$..b", b"$[0][*]", b"$[2].b[*]",
    b"a[*]", b"", b"$", b"$[*][*]", b"$[*][0]", b"$[*].b[*]",
    # the plain wildcards
    b"$[*]", b"$.*", b"[*]", b".*", b"$.*[*]", b"$[*].*", b"$[*][*][*]", b"$[*][*][*][*][*][*][*][*]", b"$.*[*].*[*].*[*].*[*]", b"$[*].k", b"$.*.x", b"$.*['x']", b'$.*["x"]',
    # the records' questions
    b"$.tags[*]", b"$.statuses[*].user.id", b"$.statuses[*].tags[*]", b"$.items[*].price", b"$.f[*]", b"$.f[*][*]", b"$.a.b.c[*].d", b"$.name",
    # bracket-quoted keys, terminated and not
    b"$['k'][*]", b'$["k"][*]', b"$.a['k'][*]", b"$['k'[*]", b'$["k[*]', b"$['k][*]", b"$['k", b"$[\"k']\"][*]",
    # keys a pointer reads in its own way
    b"$.a/b.*", b"$.m~0n.*", b"$.m~n.*", "$.é.*".encode(), "$.日本[*]".encode(), b"$.ab.*", b"$['q\"r'].*", b"$['']['x']", b"$[''].*", b"$..*",
    # indices as keys
    b"$.a.0[*]", b"$.a.1[*]", b"$.a.01[*]", b"$.a.-[*]", b"$.a.2[*]", b"$.a.99999999999999999999[*]", b"$.01.*", b"$.-[*]", b"$.0[*]", b"$.0.*[*]", b"$.b.1.*",
    # no wildcard: at_path alone
    b"$[0]", b"$[1]", b"$[-]", b"$[01]", b"$.a[1]", b"$.a.a.a.a", b"$.k[0]", b"$.a['b']", b"$[", b"$[0", b"$.a[", b"$.", b"$.a.", b"$*",
    # what is left behind the last wildcard
    b"$[*]x", b"$.[*]", b"$.*.", b"$[*].", b"$[*][", b"$.*[0]", b"$[*][-]",
]


def main():
    paths = list(dict.fromkeys(PATHS))
    ref_inc = os.path.join(_paths.REFERENCE_DIR, "include")
    ref_dir = os.path.dirname(_paths.LIB_REF)
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "paths_golden")
        subprocess.run(["g++", "-O1", "-std=c++17", "-DSIMDJSON_THREADS_ENABLED=1", "-I", ref_inc, os.path.join(HERE, "paths_golden.cpp"), "-o", exe,
                        "-L", ref_dir, "-lsjref", "-lpthread", f"-Wl,-rpath,{ref_dir}"], check=True)
        blob = struct.pack("<II", len(DOCUMENTS), len(paths)) + b"".join(struct.pack("<I", len(x)) + x for x in DOCUMENTS + paths)
        lines = subprocess.run([exe], input=blob, capture_output=True, check=True).stdout.decode().splitlines()
    assert len(lines) == len(DOCUMENTS) * len(paths)
    cells = [lines[d * len(paths): (d + 1) * len(paths)] for d in range(len(DOCUMENTS))]
    out = {"documents": [d.hex() for d in DOCUMENTS], "paths": [p.hex() for p in paths], "cells": cells}
    path = os.path.join(HERE, "paths.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    kinds = {}
    for row in cells:
        for c in row:
            kind = c if c[0] == "E" else ("M none" if c == "M" else "M some")
            kinds[kind] = kinds.get(kind, 0) + 1
    print(len(DOCUMENTS), "documents x", len(paths), "paths,", os.path.getsize(path), "bytes;", dict(sorted(kinds.items())))


if __name__ == "__main__":
    main()
