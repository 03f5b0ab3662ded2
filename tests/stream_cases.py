"""Streams of documents for the stage-2 tests of document streams (tests/test_tape_many_emu.py on the CPU tier, tests/test_gpu_stream_tape.py on the
GPU): how documents are joined, the ways one document of a stream is broken, and the hand-written table of lists whose outcome is read off the
reference's streaming walk (json_iterator.h:120-244).  Everything is generated here; nothing is read from the reference."""
import numpy as np

import jsongen

SEPARATORS = (b"\n", b"", b"\r\n  ")


def join(docs, sep):
    """(stream, byte offset of every document).  sep == b"": nothing between two documents where brackets allow it (a container behind a container),
    a newline elsewhere -- two scalars written without a gap would be ONE token."""
    out, begins = bytearray(), []
    for k, d in enumerate(docs):
        if k:
            glue = sep
            if sep == b"":
                glue = b"" if out[-1:] in (b"]", b"}") and d[:1] in (b"[", b"{") else b"\n"
            out += glue
        begins.append(len(out) + (len(d) - len(d.lstrip())))
        out += d
    return bytes(out), begins


# Breakages for which the streaming and the regular walk meet the same first error: the document keeps its outer brackets and its bracket balance, so
# the regular walk's comparison of the outer bracket with the last token (json_iterator.h:139-144) passes and nothing is left over behind the root value
# (:237-240) -- the two places where the walks differ.  `%s` takes the damaged piece.
DAMAGE = {
    "misspelt atom": (b'{"k":[1,2,{"a":%s}],"z":true}', [b"tru", b"nul", b"fals", b"truex", b"nulll", b"falsy"]),
    "bad number": (b'{"k":[1,2,{"a":%s}],"z":true}', [b"01", b"1.", b"-", b"1e", b"1.5x", b"--1"]),
    "number beyond 64 bits": (b'[{"n":%s},2]', [b"123456789012345678901", b"-123456789012345678901", b"99999999999999999999"]),
    "bad escape": (b'["ok",{"s":%s},1]', [b'"\\q"', b'"a\\u12G4"', b'"\\ud800"']),
    "doubled or leading comma": (b'{"k":%s,"z":1}', [b"[1,,2]", b"[,1]", b'{"a":1,,"b":2}', b'{,"a":1}']),
    "missing colon": (b'[1,%s,2]', [b'{"a" 1}', b'{"a":1,"b" 2}']),
    "key without a value": (b'[1,%s,2]', [b'{"a":}', b'{"a"}', b'{"a":1,"b"}']),
    "! in a value position": (b'{"k":[1,%s]}', [b"!", b"[!]", b'{"a":!}']),
}


def broken_documents():
    """(class, document) for every breakage above"""
    return [(name, shell % piece) for name, (shell, pieces) in DAMAGE.items() for piece in pieces]


def too_deep(max_depth):
    """a document nested one level beyond max_depth (and not empty at the bottom: an empty container is written without descending)"""
    return b"[" * (max_depth + 1) + b"1" + b"]" * (max_depth + 1)


def valid_documents(rng, count, max_depth=6):
    return [jsongen.random_document(rng, max_depth=max_depth) for _ in range(count)]


def small_records(rng, count):
    """NDJSON-like records of a few tokens each, every token kind among them"""
    out = []
    for k in range(count):
        kind = int(rng.integers(0, 6))
        if kind == 0:
            out.append(b'{"id":%d,"name":"user%d","ok":true,"tags":["a","b\\n"],"score":%d.5}' % (k, k, k % 97))
        elif kind == 1:
            out.append(b'[%d,"x%d",null,{"k":[]},-1e%d]' % (k, k, k % 30))
        elif kind == 2:
            out.append(b'{"text":"%s","n":%d}' % (b"lorem ipsum " * int(rng.integers(1, 12)), k))
        elif kind == 3:
            out.append([b"true", b"null", b"12", b'"s"', b"-0.5", b"[]", b"{}"][k % 7])
        elif kind == 4:
            out.append(b'{"a":{"b":{"c":[%d,{"d":"\\u00e9%d"}]}}}' % (k, k))
        else:
            out.append(b'{"e":"","f":[[],[[]],{}],"g":%d}' % k)
    return out


# (stream, max_depth) -> (documents delivered, code): read off json_iterator.h:120-244, not produced by running anything
HAND_WRITTEN = [
    (b'{"a":1} {"b":2}', 1024, 2, 0),
    (b"1 2 3", 1024, 3, 0),
    (b'"a" "b"', 1024, 2, 0),
    (b"[] {}", 1024, 2, 0),
    (b"true false null", 1024, 3, 0),
    (b'{"a":1}} {"b":2}', 1024, 1, 3),
    (b'[1,2 {"b":2}', 1024, 0, 3),
    (b'{"a":1} [1,2', 1024, 1, 3),
    (b"[1] ]", 1024, 1, 3),
    (b'{"a":1} , {"b":2}', 1024, 1, 3),
    (b'{"a":tru} {"b":2}', 1024, 0, 6),
    (b'{"a":1} {"b":nul}', 1024, 1, 8),
    (b"1 2x 3", 1024, 1, 9),
    (b'{"a":"\\q"} 1', 1024, 0, 5),
    (b"1 123456789012345678901", 1024, 1, 10),
    (b"!", 1024, 0, 3),
    (b"1 [!]", 1024, 1, 9),
    (b"[1] [[1]] [1]", 2, 1, 4),
    (b"1 [] [1]", 1, 2, 4),
    (b"", 1024, 0, 13),
]


def stray_close_behind_a_large_document(rng, records=400):
    """`{"a":1}} {"b":2}` with a first document of several thousand tokens and several levels: the stray bracket must not touch its bracket words"""
    first = b'{"rows":[' + b",".join(b'{"i":%d,"v":[[%d,{"w":[1,2,3]}],"t"],"o":{"p":{"q":null}}}' % (k, k) for k in range(records)) + b'],"end":{"x":[{}]}}'
    return first + b'} {"b":2}'
