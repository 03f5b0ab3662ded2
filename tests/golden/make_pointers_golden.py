#!/usr/bin/env python3
"""Generates tests/golden/pointers.json from the REAL reference: what dom::parser::parse(document).at_pointer(pointer) returns for every
document x pointer below (the yardstick of sjgpu_at_pointers_device, include/sjgpu_query.h).

Run where the reference lies (needs its headers and oracle/_ref/libsjref.so):   python tests/golden/make_pointers_golden.py

tests/golden/pointers_golden.cpp -- a small program of our own -- is compiled against them into a temporary directory, fed the lists and asked
cell by cell.  The fixture: "documents" and "pointers" as hex, "cells"[document][pointer] as the program printed them:
    "E <code>" | "l|u|d <the value's 64 bits>" | "t" | "f" | "n" | "s <hex of the bytes>" | "{ <tape words spanned>" | "[ <tape words spanned>"
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

K255, K256, K257 = b"k" * 255, b"k" * 256, b"k" * 257

DOCUMENTS = [
    # every kind of root
    b"{}", b"[]", b'"str"', b'""', b"12", b"-5", b"18446744073709551615", b"1.5", b"-0.0", b"true", b"false", b"null",
    # the walk's bread and butter
    b'{"a":1,"b":{"c":[10,20,{"d":"x"}]},"":"empty key","0":"zero","a/b":"slash","m~n":"tilde"}',
    b'{"b":5,"s":"str","t":true,"n":null,"f":false,"d":2.5,"u":9223372036854775808}',
    b'{"missing":{"~2":1},"a~":1,"~":2,"/":3,"~1":4,"~0":5,"~2":6}',
    # duplicate keys: the first wins
    b'{"a":1,"a":2,"b":{"x":1},"b":{"x":2},"c":[1],"c":{"0":9}}',
    # escaped keys are compared unescaped
    b'{"a\\u0062":"ab","\\u0061":"a","x\\ny":1,"q\\"r":2,"\\\\":3,"\\/":4}',
    b'{"ab":"plain first","a\\u0062":"escaped second"}',
    # a NUL in a key
    b'{"a\\u0000b":1,"a":2,"\\u0000":3,"a\\u0000":4}',
    # keys that are prefixes of each other, longest first and shortest first
    b'{"abc":3,"ab":2,"a":1,"":0}',
    b'{"":0,"a":1,"ab":2,"abc":3,"abcd":{"abc":{"ab":{"a":{"":"deep"}}}}}',
    # keys around 256 bytes
    b'{"' + K255 + b'":255,"' + K256 + b'":256,"' + K257 + b'":257}',
    b'{"' + K257 + b'":257,"' + K255 + b'x":"256 with another last byte","' + K256 + b'":256}',
    b'{"' + K255 + b'":{"' + K256 + b'":[{"' + K257 + b'":"all three"}]}}',
    # multi-byte UTF-8 keys, plain and escaped
    '{"é":1,"日本":2,"😀":3,"e":4,"日":5}'.encode(),
    b'{"\\u00e9":1,"\\u65e5\\u672c":2,"\\ud83d\\ude00":3}',
    # arrays
    b"[0,1,2,3,4,5,6,7,8,9,10,11]",
    b'[[1,2],[3,[4,5]],{"k":[6]}]',
    b'[1,[2,3],{"":"e","k":1},"s",null,true,1.25]',
    b'[{"-":1},{"x":2},{"0":{"-":3}}]',
    b'[[[[["deep"]]]]]',
    b'["only"]',
    b'[{"a":1},{"a":2},{"b":{"c":[10,20,{"d":"y"}]}}]',
    # tokens an object and an array read differently
    b'{"-":{"x":1},"01":1,"00":2,"0x":3,"1":{"":"deep"},"10":"ten"}',
    b'{"0":[["a","b"],["c"]],"1":[[],[[]],{}]}',
    b'{"18446744073709551615":"max","18446744073709551616":"beyond","99999999999999999999":"far"}',
    # numbers whose value word looks like a tape word: the integer is '{' << 56 | 5, the double has '[' in its top byte
    b'[8863084066665136133,"x",{"k":1}]',
    b'[2.2181357552966544e+130,"x",{"k":2}]',
    b'{"n":8863084066665136133,"d":2.2181357552966544e+130,"k":"behind"}',
    # NDJSON-like records
    b'{"id":7,"name":"user7","ok":true,"tags":["a","b\\n"],"score":7.5}',
    b'[7,"x7",null,{"k":[]},-1e7]',
    b'{"text":"lorem ipsum","n":3}',
    b'{"a":{"b":{"c":[4,{"d":"\\u00e94"}]}}}',
    b'{"e":"","f":[[],[[]],{}],"g":5}',
    # empty containers and empty strings on the way
    b'{"a":{},"b":[],"c":"","":{"":{"":1}}}',
    b'[[],{},"",[[]]]',
    b'{"a":[],"b":{"c":[]}}',
    b'{"a":null,"b":{"c":null}}',
    b'{"a":"1","b":{"c":"[10,20]"}}',
    # whitespace changes nothing
    b' { "a" : 1 , "b" : { "c" : [ 10 , 20 , { "d" : "x" } ] } } ',
    # deeper and wider
    b'{"a":{"a":{"a":{"a":{"a":{"a":"six"}}}}}}',
    b'{"z0":0,"z1":1,"z2":2,"z3":3,"z4":4,"z5":5,"z6":6,"z7":7,"z8":8,"z9":9,"a":"last","b":{"c":[1,2,3,4]}}',
    b'{"b":{"c":{"2":{"d":"object all the way"}}}}',
    b'{"b":[{"c":1}],"a":[[1]]}',
    b'{"b":{"c":[10,20,[30]]},"a":{"":1}}',
    b'[{"b":1},[{"b":2}],"b"]',
    b'{"a":-1,"b":{"c":[-9223372036854775808,9223372036854775807,18446744073709551615]}}',
    b'{"a":1e308,"b":{"c":[4.9e-324,0.1,1e-7]}}',
    b'{"s":{"x":"under s"},"a":{"b":"under a"}}',
    b'{"k":{"k":{"k":1}},"2":{"k":[["x"]]}}',
    b'[[0],[1,[10,[100]]],{"k":["v"]}]',
    b'{"a":[{"":[{"":"x"}]}]}',
    b'{"a":true,"b":false}',
    b'{"a":"\\u0000","b":{"c":["\\ud83d\\ude00"]}}',
    b'{"tags":["a","b"],"f":[[1],[[2]]],"id":"not a number"}',
]

POINTERS = [
    b"", b"/", b"//", b"/a", b"/b", b"/b/c", b"/b/c/2/d", b"/b/c/2", b"/b/c/3", b"/b/c/0/x", b"/a/", b"/a/b",
    # lazily reported defects
    b"/missing/~2", b"/~2", b"/a~", b"/~", b"/a/~", b"/0/~2", b"/b~0/c~2", b"/b/~2", b"/s/x", b"/b~0",
    # no leading slash: invalid for every root
    b"a", b"a/b", b"~",
    # escapes
    b"/a~1b", b"/m~0n", b"/m~n", b"/~0", b"/~1", b"/~01", b"/~00", b"/~1~0",
    # indices
    b"/0", b"/1", b"/2", b"/1/", b"/2/", b"/-", b"/-/x", b"/0/-", b"/b/c/-", b"/b/c/-/x", b"/0x", b"/01", b"/00", b"/b/c/01", b"/10", b"/11", b"/12",
    b"/18446744073709551615", b"/18446744073709551616", b"/99999999999999999999", b"/1/1/0", b"/1/1/1", b"/2/k", b"/2/k/0", b"/0/0/0/0/0", b"/1/x",
    # keys
    b"/ab", b"/abc", b"/abcd/abc/ab/a/", b"/a\x00b", b"/\x00", b"/a\x00", "/é".encode(), "/日本".encode(), "/😀".encode(), "/日".encode(),
    b"/" + K255, b"/" + K256, b"/" + K257, b"/" + b"k" * 254, b"/" + K255 + b"x", b"/" + K255 + b"/" + K256 + b"/0/" + K257,
    b"/x\ny", b'/q"r', b"/\\", b"/a/a/a/a/a/a", b"/k/k/k", b"/n", b"/d", b"/k", b"/id", b"/name", b"/tags/1", b"/a/b/c/1/d", b"/f/1/0", b"/text", b"/score",
    b"//", b"///",
]


def main():
    pointers = list(dict.fromkeys(POINTERS))
    ref_inc = os.path.join(_paths.REFERENCE_DIR, "include")
    ref_dir = os.path.dirname(_paths.LIB_REF)
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "pointers_golden")
        subprocess.run(["g++", "-O1", "-std=c++17", "-DSIMDJSON_THREADS_ENABLED=1", "-I", ref_inc, os.path.join(HERE, "pointers_golden.cpp"), "-o", exe,
                        "-L", ref_dir, "-lsjref", "-lpthread", f"-Wl,-rpath,{ref_dir}"], check=True)
        blob = struct.pack("<II", len(DOCUMENTS), len(pointers)) + b"".join(struct.pack("<I", len(x)) + x for x in DOCUMENTS + pointers)
        lines = subprocess.run([exe], input=blob, capture_output=True, check=True).stdout.decode().splitlines()
    assert len(lines) == len(DOCUMENTS) * len(pointers)
    cells = [lines[d * len(pointers): (d + 1) * len(pointers)] for d in range(len(DOCUMENTS))]
    out = {"documents": [d.hex() for d in DOCUMENTS], "pointers": [p.hex() for p in pointers], "cells": cells}
    path = os.path.join(HERE, "pointers.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    kinds = {}
    for row in cells:
        for c in row:
            kinds[c.split()[0] + (c.split()[1] if c[0] == "E" else "")] = kinds.get(c.split()[0] + (c.split()[1] if c[0] == "E" else ""), 0) + 1
    print(len(DOCUMENTS), "documents x", len(pointers), "pointers,", os.path.getsize(path), "bytes;", dict(sorted(kinds.items())))


if __name__ == "__main__":
    main()
