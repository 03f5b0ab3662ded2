"""Shared by the tests of the two prettify calls (tests/test_pretty_model.py, tests/test_pretty_emu.py, tests/test_pretty_wide_emu.py, tests/test_gpu_pretty.py) and by
tests/golden/make_pretty_golden.py: the fixture tests/golden/pretty.json (the real reference), the rows its cases stand for, and the documents made by hand for what
only the indented text can get wrong -- chains of containers whose leaf lies on either side of the 16th, 32nd, ... level, where the reference writes a container flat
and starts afresh inside it."""
import json
import os

import numpy as np

import json_text_cases
import path_model
from simdjson_amd import _paths

GOLDEN = os.path.join(_paths.REPO_ROOT, "tests", "golden", "pretty.json")
CHAIN_LEVELS = [14, 15, 16, 17, 31, 32, 33, 65]  # how many containers lie around the leaf
# a scalar, a string, the two empty containers, an array and an object that have children (and empty containers among them)
CHAIN_LEAVES = [b"7", b'"s"', b"[]", b"{}", b'[1,[2],{},"x"]', b'{"a":1,"b":[],"c":{"d":null}}']
CHAIN_PHASES = [0, 1]  # which of the two kinds the outermost container is: the container of the 16th level is once an array and once an object (of two keys)


def chain(level, leaf, phase):
    """`level` containers around `leaf`, arrays `[1,<child>]` and objects `{"k":<child>,"z":0}` alternating, the outermost an array when phase is 0"""
    head, tail = [], []
    for a in range(level):
        if (a + phase) % 2 == 0:
            head.append(b"[1,")
            tail.append(b"]")
        else:
            head.append(b'{"k":')
            tail.append(b',"z":0}')
    return b"".join(head) + leaf + b"".join(reversed(tail))


def chains():
    return [chain(level, leaf, phase) for level in CHAIN_LEVELS for leaf in CHAIN_LEAVES for phase in CHAIN_PHASES]


def chain_document(level):
    """the array of a level's twelve chains, so that `$[*]` is a column of them, each a cell of its own (the order of chains())"""
    return b"[" + b",".join(chain(level, leaf, phase) for leaf in CHAIN_LEAVES for phase in CHAIN_PHASES) + b"]"


def chain_documents():
    return [chain_document(level) for level in CHAIN_LEVELS]


def flat_container_of(children, as_object=False):
    """15 arrays around one container of `children` children -- scalars, strings, empty and small containers in turn --: the container the reference writes flat"""
    def value(i):
        return (b"%d" % i, b'"v%d"' % i, b"[]", b'{"x":[%d,{}]}' % i, b"true", b"[[%d]]" % i)[i % 6]
    if as_object:
        inner = b"{" + b",".join(b'"k%d":' % i + value(i) for i in range(children)) + b"}"
    else:
        inner = b"[" + b",".join(value(i) for i in range(children)) + b"]"
    return b"[" * 15 + inner + b"]" * 15


def fixture():
    """-> (documents as bytes, cases: the fixture's dicts with "path" as bytes and, for the small columns, "texts" as a list of bytes)"""
    g = json.load(open(GOLDEN))
    docs = [open(os.path.join(_paths.REPO_ROOT, "tests", "golden", "jsonexamples", d), "rb").read() if isinstance(d, str) else
            chain_document(d["chains_of_level"]) if "chains_of_level" in d else bytes.fromhex(d["hex"]) for d in g["documents"]]
    cases = []
    for c in g["cases"]:
        c = dict(c, path=bytes.fromhex(c["path"]))
        if "texts" in c:
            c["texts"] = [bytes.fromhex(t) for t in c["texts"]]
        cases.append(c)
    return docs, cases


def fixture_rows(orc):
    """-> [(case, (tape, sbuf, table) of the case's document alone, (tags, values): the row the case stands for)]; the path $ is the document's root cell"""
    docs, cases = fixture()
    parsed, out = {}, []
    for c in cases:
        d = c["document"]
        if d not in parsed:
            err, tape, sbuf = orc.dom_parse(docs[d])
            assert err == 0
            parsed[d] = (json_text_cases.stream_of([(tape, sbuf)]), tape.tolist(), sbuf.tobytes())
        stream, tape_list, sbuf_bytes = parsed[d]
        if c["path"] == b"$":
            row = json_text_cases.root_row(*stream)
        else:
            _, _, tags, values = path_model.column([(tape_list, sbuf_bytes)], [c["path"]])
            row = (np.array(tags, np.uint8), np.array(values, np.uint64))
        out.append((c, stream, row))
    return out


def assert_texts_are_the_fixtures(c, texts):
    json_text_cases.assert_texts_are_the_fixtures(c, texts)


# CAPACITY: 15 arrays inside one another, the innermost (14 open around it, the deepest that is not flat) of CAPACITY_ONES ones, each behind a newline, 60 blanks and,
# from the second on, a comma: 63 bytes per element, about 2 MB per root.  CAPACITY_ROWS times the same root passes 2^32
CAPACITY_ONES = 32767
CAPACITY_DOCUMENT = b"[" * 15 + b",".join([b"1"] * CAPACITY_ONES) + b"]" * 15
CAPACITY_ROWS = 2080  # the first count at which 2 065 220 bytes a root pass 2^32
