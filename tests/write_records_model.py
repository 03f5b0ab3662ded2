"""A plain Python model of sjgpu_write_records_device (include/sjgpu_write.h), the whole contract: the text of every row, status 19 and the rows it empties, the
four counts, the three kinds of invalid cell, null or omission, and validity bits at and beyond n that nobody looks at.  The texts of numbers and strings are those of
tests/json_text_model.py (pinned against the reference's own by tests/test_json_text_model.py); tests/test_write_records_model.py pins this model against
tests/golden/write_records.json, the reference's string_builder."""
import numpy as np

from json_text_model import double_text, number_text, quoted
from write_records_cases import BOOL, DOUBLE, INT64, JSON, NEWLINE, OMIT_NULLS, STRING, STRING_CELLS, UINT64

INDEX_OUT_OF_BOUNDS = 19
M32 = 0xFFFFFFFF


def is_finite(bits):
    return (bits >> 52) & 0x7FF != 0x7FF


def row_text(columns, r, flags):
    """-> (status, text: b"" with a status, invalid cells, of those doubles that are not finite)"""
    fields, nulls, nonfinite = [], 0, 0
    for c in columns:
        kind = c["kind"]
        valid = c["valid"] is None or (int(c["valid"][r >> 6]) >> (r & 63)) & 1 == 1
        value = None
        if valid:  # (what lies under a validity bit of 0 decides nothing)
            if kind in (STRING, JSON):
                a, b = int(c["offsets"][r]), int(c["offsets"][r + 1])
                if b < a or b > c["chars_bytes"]:
                    return INDEX_OUT_OF_BOUNDS, b"", 0, 0
                s = bytes(c["chars"][a:b])
                if kind == STRING:
                    value = quoted(s)
                elif s:
                    value = s
            elif kind == STRING_CELLS:
                w = int(c["values"][r])
                a, n = w & M32, w >> 32
                if a + n > c["chars_bytes"]:
                    return INDEX_OUT_OF_BOUNDS, b"", 0, 0
                value = quoted(bytes(c["chars"][a:a + n]))
            else:
                w = int(c["values"][r])
                if kind == INT64:
                    value = number_text(0x6C, w)
                elif kind == UINT64:
                    value = number_text(0x75, w)
                elif kind == BOOL:
                    value = b"true" if w else b"false"
                elif is_finite(w):
                    assert kind == DOUBLE
                    value = double_text(w)
                else:
                    nonfinite += 1
        if value is None:
            nulls += 1
            if flags & OMIT_NULLS:
                continue
            value = b"null"
        fields.append(quoted(c["key"]) + b":" + value)
    return 0, b"{" + b",".join(fields) + b"}" + (b"\n" if flags & NEWLINE else b""), nulls, nonfinite


def records(arrays, flags):
    """arrays: write_records_cases.arrays_of(table) -> (offsets uint32[n + 1], chars bytes, status uint8[n], counts uint64[4])"""
    offsets, parts, status, counts = [0], [], [], [0, 0, 0, 0]
    for r in range(arrays["n"]):
        code, text, nulls, nonfinite = row_text(arrays["columns"], r, flags)
        status.append(code)
        parts.append(text)
        offsets.append(offsets[-1] + len(text))
        if code:
            counts[1] += 1
        else:
            counts[0] += 1
            counts[2] += nulls
            counts[3] += nonfinite
    return np.array(offsets, np.uint64).astype(np.uint32), b"".join(parts), np.array(status, np.uint8), np.array(counts, np.uint64)
