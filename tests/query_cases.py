"""Shared by the tests of the queries over tapes (tests/test_pointer_model.py, tests/test_query_emu.py, tests/test_gpu_query.py): the fixture
tests/golden/pointers.json, a cell of sjgpu_at_pointers_device rendered the way the fixture records it, streams laid out as
sjgpu_stage2_many_device lays them out, and pointers harvested from documents."""
import json
import os

import numpy as np

import pointer_model
from simdjson_amd import _paths

GOLDEN = os.path.join(_paths.REPO_ROOT, "tests", "golden", "pointers.json")
DOC_SPAN = np.dtype([("first_token", np.uint32), ("byte_begin", np.uint32), ("tape_begin", np.uint32), ("string_begin", np.uint32)])
SMALL_RECORD_POINTERS = [b"/id", b"/name", b"/tags/1", b"/a/b/c/1/d", b"/f/1/0", b"/text", b"/score", b"/0", b"/1/", b""]


def fixture():
    g = json.load(open(GOLDEN))
    return [bytes.fromhex(d) for d in g["documents"]], [bytes.fromhex(p) for p in g["pointers"]], g["cells"]


def render(tag, value, sbuf):
    """a cell as the fixture's generator prints it (sbuf: the array a string cell's offset is absolute in)"""
    tag, value = int(tag), int(value)
    if tag in pointer_model.CODES:
        assert value == 0, "a failed cell holds 0"
        return f"E {tag}"
    c = chr(tag)
    if c in "lud":
        return f"{c} {value}"
    if c in "tfn":
        assert value == (1 if c == "t" else 0)
        return c
    if c == '"':
        return "s " + pointer_model.string_of(sbuf, value).hex()
    assert c in "{[", tag
    return f"{c} {(value >> 32) - (value & 0xFFFFFFFF)}"


def lay_out(parsed):
    """[(tape, string_buf)] per document -> (tape, string_buf, table of documents + 1 entries) back to back"""
    tape = np.concatenate([t for t, _ in parsed]) if parsed else np.zeros(0, np.uint64)
    sbuf = np.concatenate([s for _, s in parsed] + [np.zeros(0, np.uint8)]).astype(np.uint8)
    table = np.zeros(len(parsed) + 1, DOC_SPAN)
    table["tape_begin"] = np.concatenate([[0], np.cumsum([len(t) for t, _ in parsed])])
    table["string_begin"] = np.concatenate([[0], np.cumsum([len(s) for _, s in parsed])])
    return tape.astype(np.uint64), sbuf, table


def check_container_cells(tags, values, tape, table):
    """a container cell delimits a sub-tape: its first word opens, its last closes and points back, and it lies inside its document"""
    for k, d in zip(*np.nonzero((tags == ord("{")) | (tags == ord("[")))):
        lo, hi = int(values[k, d]) & 0xFFFFFFFF, int(values[k, d]) >> 32
        assert int(table["tape_begin"][d]) < lo < hi < int(table["tape_begin"][d + 1])
        assert int(tape[lo]) >> 56 == int(tags[k, d]) and int(tape[hi - 1]) >> 56 == int(tags[k, d]) + 2
        assert (int(tape[hi - 1]) & 0xFFFFFFFF) + int(table["tape_begin"][d]) == lo


def paths_of(value, prefix=b"", out=None):
    """every JSON pointer that exists in a Python value (from json.loads), the containers' own included"""
    out = [] if out is None else out
    out.append(prefix)
    if isinstance(value, dict):
        for key, v in value.items():
            paths_of(v, prefix + b"/" + key.encode("utf-8", "surrogatepass").replace(b"~", b"~0").replace(b"/", b"~1"), out)
    elif isinstance(value, list):
        for i, v in enumerate(value):
            paths_of(v, prefix + b"/%d" % i, out)
    return out


def first_wins(pairs):
    d = {}
    for k, v in pairs:
        d.setdefault(k, v)
    return d


MISSES = [b"/5", b"/6", b"/7", b"/8", b"/9", b"/10", b"/99", b"/12345678901234567890123", b"/0/5",  # indices out of range (an object answers NO_SUCH_FIELD)
          b"/nope", b"/a/nope", b"/Zq/x",                                                           # absent keys (an array answers INCORRECT_TYPE)
          b"/0/0/0/0/0/0/0", b"/0/a/b", b"/1/1/1/1", b"/2/x/0"]                                     # paths that run into scalars


def commonest_paths(docs, depth=3):
    """the paths of at most `depth` tokens that exist in the documents, the commonest first"""
    seen = {}
    for d in docs:
        for p in set(paths_of(json.loads(d, object_pairs_hook=first_wins))):
            if p.count(b"/") <= depth:
                seen[p] = seen.get(p, 0) + 1
    return sorted(seen, key=lambda p: (-seen[p], p))


def harvest(docs, count=32, share=0.30):
    """`count` pointers for the random documents of jsongen, half of them harvested from paths that exist in the documents, the other half paths that cannot hit
    (MISSES), such that at least `share` of the count x documents cells are hits.
    jsongen's documents share no schema: the only path most of them have is the root (every document), then `/0` (3 in 8), `/1`, `/2`, ... and nothing below the
    first level reaches 4 %.  16 DISTINCT paths therefore hit 7.7 % of the cells at best, and a share of 30 % of all cells needs the harvested half to hit in 60 %
    of its own.  So the harvest is taken with repetition, greedily by hits: the next pointer is the commonest path not taken yet unless the share would then be
    out of reach with the pointers left, in which case it is the root pointer once more.  Two rows of one pointer are two rows of cells like any other two
    (a row is a workgroup row of its own with its own copy of the program); the distinct paths this leaves out are run by distinct_harvest below."""
    common = commonest_paths(docs)
    assert common[0] == b""
    counts = {p: 0 for p in common}
    for d in docs:
        for p in set(paths_of(json.loads(d, object_pairs_hook=first_wins))):
            if p in counts:
                counts[p] += 1
    half, need = count // 2, share * count * len(docs)
    taken, hits, fresh = [], 0, 0
    while len(taken) < half:
        left = half - len(taken) - 1
        p = common[fresh] if fresh < len(common) else b""
        if hits + counts[p] + left * counts[b""] < need:  # (with the commonest path: the rest as root pointers would no longer do)
            p = b""
        else:
            fresh += 1
        taken.append(p)
        hits += counts[p]
    assert hits >= need, "not even the root pointer alone reaches the share"
    return taken + MISSES[: count - half]


def distinct_harvest(docs, count=32):
    """the 16 commonest distinct paths and the 16 misses: fewer hits (nothing is asserted about their share), more kinds of them -- the second level included"""
    return commonest_paths(docs)[: count // 2] + MISSES[: count - count // 2]
