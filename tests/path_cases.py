"""Shared by the tests of the paths over tapes (tests/test_path_model.py, tests/test_paths_emu.py, tests/test_gpu_paths.py): the fixture
tests/golden/paths.json, a cell of sjgpu_at_paths_device rendered the way the fixture records it, a ragged column compared with tests/path_model.py,
and JSONPaths derived from the pointers that exist in documents."""
import json
import os
import re

import numpy as np

import path_model
import query_cases
from simdjson_amd import _paths

GOLDEN = os.path.join(_paths.REPO_ROOT, "tests", "golden", "paths.json")
SMALL_RECORD_PATHS = [b"$.tags[*]", b"$.f[*]", b"$.f[*][*]", b"$[*]", b"$.*", b"$.a.b.c[*].d", b"$[*].k", b"$.name", b"$.missing[*]"]


def fixture():
    g = json.load(open(GOLDEN))
    return [bytes.fromhex(d) for d in g["documents"]], [bytes.fromhex(p) for p in g["paths"]], g["cells"]


def render(status, cells, sbuf):
    """a cell -- its status and its (tag, value) matches -- as the fixture's generator prints it"""
    if status:
        assert not cells, "a cell with a status has no matches"
        return f"E {int(status)}"
    return "M" + "".join(";" + query_cases.render(t, v, sbuf) for t, v in cells)


def cell(status, offsets, tags, values, k, d, docs):
    """-> (status, [(tag, value)]) of cell (k, d) of a ragged column"""
    c = k * docs + d
    lo, hi = int(offsets[c]), int(offsets[c + 1])
    return int(status[k][d]), [(int(tags[i]), int(values[i])) for i in range(lo, hi)]


def model_column(parsed, paths):
    """tests/path_model.py's column as arrays: (status uint8[K, docs], offsets uint32[K * docs + 1], tags uint8[matches], values uint64[matches])"""
    status, offsets, tags, values = path_model.column(parsed, paths)
    return (np.array(status, np.uint8).reshape(len(paths), len(parsed)), np.array(offsets, np.uint32), np.array(tags, np.uint8), np.array(values, np.uint64))


def assert_column(got, want, what=""):
    for g, w, name in zip(got, want, ("status", "offsets", "tags", "values")):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, f"{what}{name}: shape {g.shape}, the model {w.shape}"
        if not np.array_equal(g, w):
            at = tuple(int(x) for x in np.argwhere(g != w)[0])
            raise AssertionError(f"{what}{name}{list(at)} = {int(g[at])}, the model {int(w[at])}")


def check_container_matches(tags, values, tape):
    """a container match delimits a sub-tape: its first word opens, its last closes and points back"""
    for i in np.nonzero((tags == ord("{")) | (tags == ord("[")))[0]:
        lo, hi = int(values[i]) & 0xFFFFFFFF, int(values[i]) >> 32
        assert lo < hi <= len(tape) and int(tape[lo]) >> 56 == int(tags[i]) and int(tape[hi - 1]) >> 56 == int(tags[i]) + 2, i


def path_of_pointer(pointer):
    """a JSON pointer made by query_cases.paths_of as a JSONPath with every array index replaced by `[*]`; None when a key cannot be written as `.key`"""
    out = b"$"
    for token in pointer.split(b"/")[1:]:
        if re.fullmatch(rb"\d+", token):
            out += b"[*]"
        elif token and not re.search(rb"[.\[*~]", token):
            out += b"." + token
        else:
            return None
    return out


def wildcard_paths(docs, count=14):
    """`count` distinct JSONPaths derived from the commonest pointers of the documents (every index turned into `[*]`), then `$[*]` and `$.*`"""
    out = []
    for p in query_cases.commonest_paths(docs):
        path = path_of_pointer(p)
        if path is not None and path not in (b"$", b"$[*]", b"$.*") and path not in out:
            out.append(path)
        if len(out) == count:
            break
    return out + [b"$[*]", b"$.*"]
