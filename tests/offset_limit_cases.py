"""The plan of tests/test_gpu_offset_limits.py: for every device call that sums per-cell counts into one 64-bit total and scans u32 offsets in place, small
inputs whose totals lie just below, on and just above what 32 bits hold.

The calls -- sjgpu_gather_strings_device, sjgpu_at_paths_device, sjgpu_at_paths_wide_device, sjgpu_at_paths_from_cells_device,
sjgpu_object_fields_from_cells_device, sjgpu_serialize_cells_device, sjgpu_write_records_device, sjgpu_write_nested_device -- promise "A total beyond 32 bits:
CAPACITY (1)".  Three totals per call:
    T1  inside (2^31, 2^32), the smallest the rows allow: served; the last row ends beyond 2^31
    T2  2^32 - 1 exactly: the largest total that is served; half of its offsets have bit 31 set
    T3  2^32 exactly: refused (one more case lies one row beyond it, stated there)
The totals are cheap because rows may describe the same bytes: 65 536 cells over one 64 KiB string are a 4 GiB column from a few hundred KiB of input.  Only the
calls rooted at DOCUMENTS cannot alias (a lane is a document): their input is a stream of ~136 MB of arrays of ones (roots_stream).

A case is a list of RUNS -- (the name of a distinct row, how many of them) in order -- over a handful of distinct rows whose lengths (bytes, matches or
fields) the plan ASSUMES.  Nothing here is taken from the library under test: tests/test_offset_limit_cases.py (CPU tier) asserts the sums by arithmetic, takes
the text, the matches or the fields of each distinct row from the Python models (pinned against the reference on the CPU tier) and compares their lengths with the
assumed ones, and runs every case scaled down to a handful of rows through the models."""
import collections

import numpy as np

LIMIT = 1 << 32
HALF = 1 << 31
T2, T3 = LIMIT - 1, LIMIT
QUOTE, OPEN_ARRAY, OPEN_OBJECT, INT64 = 0x22, 0x5B, 0x7B, 0x6C
COL_JSON, COL_STRING_CELLS = 8, 9  # SJGPU_COL_JSON, SJGPU_COL_STRING_CELLS (include/sjgpu_write.h)

# runs: ((row name, count), ...); level: "T1" | "T2" | "T3"; total: what the plan claims (asserted against the runs on the CPU tier)
Case = collections.namedtuple("Case", "call name level runs total")


def rows_of(case):
    return sum(count for _, count in case.runs)


def total_of(case, lengths):
    return sum(count * lengths[name] for name, count in case.runs)


def lengths_of(case, lengths):
    """the length of every row, in order: int64[rows]"""
    return np.concatenate([np.full(count, lengths[name], np.int64) for name, count in case.runs])


def offsets_of(case, lengths):
    """the offsets a served case leaves: uint64[rows + 1], an arithmetic progression per run"""
    return np.concatenate([np.zeros(1, np.uint64), np.cumsum(lengths_of(case, lengths)).astype(np.uint64)])


def scaled(case, few=3):
    """the same runs with at most `few` rows each: what the models can walk"""
    return case._replace(runs=tuple((name, min(count, few)) for name, count in case.runs), total=None)


def row_names(case):
    """the distinct row of every row, in order"""
    return [name for name, count in case.runs for _ in range(count)]


# ---- the gather: one string buffer, cells that all point at three records ------------------------------------------------------------------------------
GATHER_LENGTHS = {"s65536": 65536, "s65537": 65537, "s1": 1}


def gather_buffer():
    """-> (sbuf uint8[...], {row name: (tag, value)}): three strings back to back, a string cell (length << 32 | offset) for each"""
    parts, cells, at = [], {}, 0
    for k, (name, n) in enumerate(GATHER_LENGTHS.items()):
        parts.append(np.full(n, ord("a") + k, np.uint8))
        cells[name] = (QUOTE, (n << 32) | at)
        at += n
    return np.concatenate(parts), cells


GATHER = (
    Case("gather", "T1", "T1", (("s65536", 32769),), HALF + 65536),
    Case("gather", "T2", "T2", (("s65537", 65535),), T2),
    Case("gather", "T3", "T3", (("s65537", 65535), ("s1", 1)), T3),
)


# ---- one document for the three calls rooted at cells ----------------------------------------------------------------------------------------------------
# /a /b /c: arrays of 65 536, 65 535 and 1 ones ($[*] matches each element); /oa /ob /oc: objects of as many fields, all of them "k":1 (duplicate keys are
# fields like any other; the count of fields is the opening word's count field, below 0xFFFFFF); /s /t: strings of 65 535 and 65 536 bytes, served from the
# cell itself as the string + 2 quotes; /one: the number 1, one byte of text; /arr: [10,1,1,...] with 32 767 elements -- 2 brackets, 32 768 digits, 32 766
# commas: 65 536 bytes of minified text, served by a walk over the tape
ARR_ELEMENTS = 32767
ROOT_POINTERS = {"a": b"/a", "b": b"/b", "c": b"/c", "oa": b"/oa", "ob": b"/ob", "oc": b"/oc", "s": b"/s", "t": b"/t", "one": b"/one", "arr": b"/arr"}
PATH = b"$[*]"


def document():
    def ones(n):
        return b"[" + b",".join([b"1"] * n) + b"]"

    def fields(n):
        return b"{" + b",".join([b'"k":1'] * n) + b"}"
    return (b'{"a":' + ones(65536) + b',"b":' + ones(65535) + b',"c":' + ones(1) + b',"oa":' + fields(65536) + b',"ob":' + fields(65535) + b',"oc":' + fields(1)
            + b',"s":"' + b"x" * 65535 + b'","t":"' + b"y" * 65536 + b'","one":1,"arr":[10' + b",1" * (ARR_ELEMENTS - 1) + b"]}")


PATH_LENGTHS = {"a": 65536, "b": 65535, "c": 1}      # matches of $[*]
FIELD_LENGTHS = {"oa": 65536, "ob": 65535, "oc": 1}  # fields
TEXT_LENGTHS = {"s": 65535 + 2, "t": 65536 + 2, "one": 1, "arr": 65536}  # bytes of minify(element)

PATHS_FROM_CELLS = (
    Case("paths_from_cells", "T1", "T1", (("a", 32769),), HALF + 65536),
    Case("paths_from_cells", "T2", "T2", (("a", 65535), ("b", 1)), T2),
    Case("paths_from_cells", "T3", "T3", (("a", 65535), ("b", 1), ("c", 1)), T3),
)
FIELDS_FROM_CELLS = (
    Case("fields_from_cells", "T1", "T1", (("oa", 32769),), HALF + 65536),
    Case("fields_from_cells", "T2", "T2", (("oa", 65535), ("ob", 1)), T2),
    Case("fields_from_cells", "T3", "T3", (("oa", 65535), ("ob", 1), ("oc", 1)), T3),
)
SERIALIZE = (
    Case("serialize", "T1", "T1", (("t", 32768),), 2147549184),
    Case("serialize", "T2", "T2", (("s", 65535),), T2),
    Case("serialize", "T3", "T3", (("s", 65535), ("one", 1)), T3),
    # the refusal through the tape walk: 65 537 rows of 65 536 bytes, one row beyond 2^32 -- a total that wraps to 65 536, which "fits" a small capacity
    Case("serialize", "T3 container roots", "T3", (("arr", 65537),), T3 + 65536),
)


# ---- the writers: one column (one list field) of string cells over one run of letters ------------------------------------------------------------------------
# a record is {"k":"<string>"}: the string + 8 bytes; a nested row {"k":["<string>"]}: + 10; with two elements {"k":["<string>","<string>"]}: twice + 13
WRITE_KEY = b"k"
WRITE_CHARS = 65536  # the column's characters: this many letters, every cell a prefix of them
WRITE_STRINGS = {"w65544": 65536, "w65537": 65529, "w65538": 65530}     # row name -> the string's length
WRITE_LENGTHS = {"w65544": 65544, "w65537": 65537, "w65538": 65538}
NESTED_STRINGS = {"n65546": 65536, "n65537": 65527, "n65538": 65528, "pair131085": 65536}
NESTED_LENGTHS = {"n65546": 65546, "n65537": 65537, "n65538": 65538, "pair131085": 131085}
NESTED_ELEMENTS = {"n65546": 1, "n65537": 1, "n65538": 1, "pair131085": 2}

WRITE_RECORDS = (
    Case("write_records", "T1", "T1", (("w65544", 32768),), 2147745792),
    Case("write_records", "T2", "T2", (("w65537", 65535),), T2),
    Case("write_records", "T3", "T3", (("w65537", 65534), ("w65538", 1)), T3),
)
WRITE_NESTED = (
    Case("write_nested", "T1", "T1", (("n65546", 32768),), 2147811328),
    Case("write_nested", "T2", "T2", (("n65537", 65535),), T2),
    Case("write_nested", "T3", "T3", (("n65537", 65534), ("n65538", 1)), T3),
    Case("write_nested", "T1 two elements per row", "T1", (("pair131085", 16384),), 2147696640),
)


def write_chars():
    return np.full(WRITE_CHARS, ord("x"), np.uint8)


def string_cell(n):
    """a string cell of the first n letters of write_chars()"""
    return (n << 32) | 0


def write_columns(names, chars):
    """the one column of the records `names` (a row name per row) as the model takes it"""
    values = np.array([string_cell(WRITE_STRINGS[name]) for name in names], np.uint64)
    return {"n": len(names), "columns": [{"key": WRITE_KEY, "kind": COL_STRING_CELLS, "valid": None, "values": values, "chars": chars, "chars_bytes": len(chars)}]}


def nested_fields(names, chars):
    """the one list field of the rows `names` as the model takes it: the elements of all rows back to back, list_offsets in front of each row's"""
    counts = [NESTED_ELEMENTS[name] for name in names]
    values = np.array([string_cell(NESTED_STRINGS[name]) for name, c in zip(names, counts) for _ in range(c)], np.uint64)
    list_offsets = np.concatenate([np.zeros(1, np.int64), np.cumsum(counts)]).astype(np.uint32)
    return {"n": len(names), "fields": [{"key": WRITE_KEY, "kind": COL_STRING_CELLS, "valid": None, "values": values, "chars": chars, "chars_bytes": len(chars),
                                        "list_offsets": list_offsets, "list_valid": None, "elements": len(values)}]}


# One row ALONE beyond 2^32: n = 1, 64 columns of kind SJGPU_COL_JSON that all name the same offsets [0, WIDE_CELL] and the same characters.  The row's own
# u32 length wraps, the 64-bit sum does not.  The row is { "k00":<cell> , ... , "k63":<cell> }: 64 cells, 64 keys of 3 letters with quotes and a colon, 63
# commas, 2 braces
WIDE_COLUMNS, WIDE_CELL = 64, 64 << 20
WIDE_KEYS = tuple(b"k%02d" % k for k in range(WIDE_COLUMNS))


def wide_row_bytes(cell):
    return WIDE_COLUMNS * cell + sum(len(k) + 3 for k in WIDE_KEYS) + (WIDE_COLUMNS - 1) + 2


WIDE_ROW_TOTAL = wide_row_bytes(WIDE_CELL)  # 2^32 + 449


def wide_columns(cell):
    """the 64 columns over ONE cell of `cell` digits, as the model takes them (the CPU tier calls this with a cell of a few bytes)"""
    chars, offsets = np.full(cell, ord("1"), np.uint8), np.array([0, cell], np.uint32)
    return {"n": 1, "columns": [{"key": k, "kind": COL_JSON, "valid": None, "offsets": offsets, "chars": chars, "chars_bytes": cell} for k in WIDE_KEYS]}


# ---- the calls rooted at documents: a stream of arrays of ones ---------------------------------------------------------------------------------------------
# `$[*]` matches every element of a document, `$[0]` one per document.  T2: D = 1011 documents with E = 68 174 068 elements in all under 63 paths `$[*]` and
# one `$[0]`: 63 E + D = 2^32 - 1.  T1: 32 paths `$[*]` over the same stream.  T3: 64 paths `$[*]` over 1024 documents of 65 536 elements, 2^26 in all.
# Every array stays far below 2^24 elements: no count field saturates.
Roots = collections.namedtuple("Roots", "name level stream paths total")
STREAM_T2 = (67432,) * 1010 + (67748,)
STREAM_T3 = (65536,) * 1024
ROOTS = (
    Roots("T1", "T1", "T2", (PATH,) * 32, 2181570176),
    Roots("T2", "T2", "T2", (PATH,) * 63 + (b"$[0]",), T2),
    Roots("T3", "T3", "T3", (PATH,) * 64, T3),
)
STREAMS = {"T2": STREAM_T2, "T3": STREAM_T3}


def roots_lengths(case):
    """the matches of every cell, in the call's order (path k, document d -> k * docs + d): int64[K * docs]"""
    elements = np.array(STREAMS[case.stream], np.int64)
    return np.concatenate([elements if p == PATH else np.ones(len(elements), np.int64) for p in case.paths])


def roots_stream(elements):
    """NDJSON: one line `[1,1,...,1]` of e ones per entry of `elements` -> uint8[sum(2 e + 2)]; made with np.tile, not with a loop over the elements"""
    pair = np.frombuffer(b"1,", np.uint8)
    lines = {}
    for e in set(elements):
        line = np.empty(2 * e + 2, np.uint8)
        line[0] = ord("[")
        line[1:2 * e + 1] = np.tile(pair, e)
        line[2 * e] = ord("]")  # in the place of the last comma
        line[2 * e + 1] = ord("\n")
        lines[e] = line
    return np.concatenate([lines[e] for e in elements])


ALL_CASES = GATHER + PATHS_FROM_CELLS + FIELDS_FROM_CELLS + SERIALIZE + WRITE_RECORDS + WRITE_NESTED
LENGTHS = {"gather": GATHER_LENGTHS, "paths_from_cells": PATH_LENGTHS, "fields_from_cells": FIELD_LENGTHS, "serialize": TEXT_LENGTHS,
           "write_records": WRITE_LENGTHS, "write_nested": NESTED_LENGTHS}
