"""GPU tier (-m gpu): what the other tests leave open about the *_many calls of simdjson_amd/capi.py (extract_many, explode_many, table_many, lists_many,
typed_table_many) -- what each returns when there is nothing to return (a stage-1 error, a broken first document, no pointers / paths), WHICH entry points of
the C-ABI each call goes through and in which order, and that table_many and typed_table_many hand out the same cells.  Every expected value is a literal,
recorded from the calls as they were before their shared steps (the resident stream, the capacity retry, the rows of the row path) became helpers: the layer
may be rearranged, what it answers and the work it asks of the library may not."""
import numpy as np
import pytest

from simdjson_amd import build, capi

pytestmark = pytest.mark.gpu

STREAM = b'{"a":[1,2],"b":"x"}\n{"a":[],"b":"yz"}\n{"a":[3],"c":null}'
UNCLOSED = b'{"a":"x'               # (a) stage 1 itself refuses the buffer
BROKEN_FIRST = b'{"a":tru}\n{"a":1}'  # (b) stage 1 passes, the first document is broken: no document is delivered
ROW_PATH = b"$.a[*]"
CALLS = ("extract_many", "explode_many", "table_many", "lists_many", "typed_table_many")


@pytest.fixture(scope="module")
def parser():
    build.build_sjgpu()
    p = capi.DomParserImplementation(1 << 20)
    yield p
    p.close()


def run(p, name, data, K, row_path=ROW_PATH, items=None, **kw):
    """the call `name` over `data` with K pointers (the root, K times) or paths (`$`, K times) unless `items` names them, the row path where the call takes one"""
    pointers, paths = items or [b""] * K, items or [b"$"] * K
    if name == "extract_many":
        return p.extract_many(data, pointers, **kw)
    if name == "explode_many":
        return p.explode_many(data, paths, **kw)
    if name == "lists_many":
        return p.lists_many(data, row_path, paths, **kw)
    return getattr(p, name)(data, row_path, pointers, **kw)


def pin(x):
    """a result as plain Python: an array becomes (dtype, shape, contents)"""
    if isinstance(x, np.ndarray):
        return (str(x.dtype), tuple(x.shape), x.tolist())
    if isinstance(x, (tuple, list)):
        return type(x)(pin(i) for i in x)
    if isinstance(x, dict):
        return {k: pin(v) for k, v in x.items()}
    return int(x) if isinstance(x, np.integer) else x


class Recorder:
    """stands where parser.L stood: notes the name of every sjgpu_* function asked of the library and hands out the library's own"""

    def __init__(self, L):
        self._L, self.names = L, []

    def __getattr__(self, name):
        if name.startswith("sjgpu_"):
            self.names.append(name)
        return getattr(self._L, name)


def recorded(p, name, **kw):
    L = p.L
    p.L = rec = Recorder(L)
    try:
        run(p, name, STREAM, 1, **kw)
    finally:
        p.L = L
    return rec.names


EDGES = {"stage1_error": (UNCLOSED, 1), "broken_first_document": (BROKEN_FIRST, 1), "K0": (STREAM, 0)}
NO_U8, NO_U64, ZERO = ("uint8", (0,), []), ("uint64", (0,), []), ("uint32", (1,), [0])
NO_ROWS = ("uint8", (1, 0), [[]]), ("uint64", (1, 0), [[]])
K0_ROWS = ("uint8", (0, 3), []), ("uint64", (0, 3), [])
ROWS = ("uint32", (4,), [0, 2, 2, 3])  # the rows of $.a[*]: two in the first record, none in the second, one in the third
NO_COLUMN = {"getter": 0, "kinds": ("uint32", (16,), [0] * 16), "tags": NO_U8, "cells": NO_U64}
# What the calls returned before their shared steps became helpers; 15 is UNCLOSED_STRING, 6 is what stage 2 says of `tru}` (T_ATOM_ERROR).  Some of it looks
# odd and is pinned as it is: lists_many answers offsets == [0] (length 1) beside a status of shape (K, 0) when no document was delivered, and again -- K * rows + 1
# entries -- when K == 0; explode_many's status has one row per path even without a document; with K == 0 the table calls still deliver the rows of the row path.
EXPECTED = {
    ("extract_many", "stage1_error"): (15, 0) + NO_ROWS,
    ("extract_many", "broken_first_document"): (6, 0) + NO_ROWS,
    ("extract_many", "K0"): (0, 3) + K0_ROWS,
    ("explode_many", "stage1_error"): (15, 0, NO_ROWS[0], ZERO, NO_U8, NO_U64),
    ("explode_many", "broken_first_document"): (6, 0, NO_ROWS[0], ZERO, NO_U8, NO_U64),
    ("explode_many", "K0"): (0, 3, K0_ROWS[0], ZERO, NO_U8, NO_U64),
    ("table_many", "stage1_error"): (15, 0, ZERO) + NO_ROWS,
    ("table_many", "broken_first_document"): (6, 0, ZERO) + NO_ROWS,
    ("table_many", "K0"): (0, 3, ROWS) + K0_ROWS,
    ("lists_many", "stage1_error"): (15, 0, ZERO, NO_ROWS[0], ZERO, NO_U8, NO_U64),
    ("lists_many", "broken_first_document"): (6, 0, ZERO, NO_ROWS[0], ZERO, NO_U8, NO_U64),
    ("lists_many", "K0"): (0, 3, ROWS, K0_ROWS[0], ZERO, NO_U8, NO_U64),
    ("typed_table_many", "stage1_error"): (15, 0, ZERO, [NO_COLUMN]),
    ("typed_table_many", "broken_first_document"): (6, 0, ZERO, [NO_COLUMN]),
    ("typed_table_many", "K0"): (0, 3, ROWS, []),
}

# (sjgpu_stage1_error_from_flags is asked of the module's own handle, not of the parser's: it is not in the lists)
TAPES = ["sjgpu_stage1_device", "sjgpu_result", "sjgpu_stage2_many_device"]
TABLE = TAPES + ["sjgpu_at_paths_device", "sjgpu_at_pointers_from_cells_device"]
# `$` alone is no path (every cell of it is INVALID_JSON_POINTER, 22, and nothing matches), so a first capacity of 0 is enough for it: one call.  The two
# "overflowing" cases have three matches and a first capacity of 0: the call, and the call once more.
SEQUENCES = {
    "extract_many": ({}, TAPES + ["sjgpu_at_pointers_device"]),
    "explode_many": ({}, TAPES + ["sjgpu_at_paths_device"]),
    "table_many": ({}, TABLE),
    "lists_many": ({}, TAPES + ["sjgpu_at_paths_device", "sjgpu_at_paths_from_cells_device"]),
    "typed_table_many": ({}, TABLE + ["sjgpu_cell_kinds_device", "sjgpu_cast_cells_device"]),
    "explode_many, first_cap=0": ({"first_cap": 0}, TAPES + ["sjgpu_at_paths_device"]),
    "lists_many, first_cap=0": ({"first_cap": 0}, TAPES + ["sjgpu_at_paths_device", "sjgpu_at_paths_from_cells_device"]),
    "explode_many, overflowing": ({"first_cap": 0, "items": [b"$.a[*]"]}, TAPES + ["sjgpu_at_paths_device"] * 2),
    "lists_many, overflowing": ({"first_cap": 0, "row_path": b"$.a", "items": [b"$[*]"]}, TAPES + ["sjgpu_at_paths_device"] + ["sjgpu_at_paths_from_cells_device"] * 2),
    "typed_table_many, a string column": ({"row_path": b"$.b", "items": [b""]},  # "x" and "yz": the gather asks, then delivers three characters
                                          TABLE + ["sjgpu_cell_kinds_device", "sjgpu_cast_cells_device"] + ["sjgpu_gather_strings_device"] * 2),
}
THREE = ("uint8", (3,), [ord("l")] * 3), ("uint64", (3,), [1, 2, 3])  # the numbers of the three records' arrays, in order
OVERFLOWING = {
    "explode_many": (0, 3, ("uint8", (1, 3), [[0, 0, 0]]), ROWS) + THREE,
    "lists_many": (0, 3, ("uint32", (4,), [0, 1, 2, 3]), ("uint8", (1, 3), [[0, 0, 0]]), ROWS) + THREE,
}


@pytest.mark.parametrize("name", CALLS)
@pytest.mark.parametrize("edge", list(EDGES))
def test_edges_return_what_they_returned(parser, name, edge):
    data, K = EDGES[edge]
    got = pin(run(parser, name, data, K))
    print(name, edge, got)
    assert got == EXPECTED[name, edge]


@pytest.mark.parametrize("case", list(SEQUENCES))
def test_the_calls_into_the_library_and_their_order(parser, case):
    kw, want = SEQUENCES[case]
    got = recorded(parser, case.split(",")[0], **kw)
    print(case, got)
    assert got == want


@pytest.mark.parametrize("name", list(OVERFLOWING))
def test_a_first_capacity_too_small_gives_the_same_column(parser, name):
    kw = dict(SEQUENCES[name + ", overflowing"][0])
    assert pin(run(parser, name, STREAM, 1, **kw)) == OVERFLOWING[name]
    del kw["first_cap"]
    assert pin(run(parser, name, STREAM, 1, **kw)) == OVERFLOWING[name]


@pytest.mark.parametrize("wide", [False, True])
def test_table_many_is_the_cells_of_typed_table_many(parser, wide):
    code, docs, row_offsets, tags, values = run(parser, "table_many", STREAM, 2, wide=wide)
    tcode, tdocs, trow_offsets, columns = run(parser, "typed_table_many", STREAM, 2, wide=wide)
    assert (code, docs) == (tcode, tdocs) == (0, 3) and pin(row_offsets) == pin(trow_offsets) == ROWS
    assert len(columns) == 2 and tags.shape == values.shape == (2, 3)
    for k, col in enumerate(columns):
        assert (pin(col["tags"]), pin(col["cells"])) == (pin(tags[k]), pin(values[k])) == THREE


