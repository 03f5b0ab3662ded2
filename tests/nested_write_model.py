"""A plain Python model of sjgpu_write_nested_device (include/sjgpu_nested.h), the whole contract: list fields, the three row shapes, null or omission at the top
level and ALWAYS null inside a list, status 19 and the rows it empties, the six counts, and what nobody reads under a validity bit of 0.  A value's text is that of
tests/write_records_model.py -- one cell of one column through its row_text --, so a table without list fields and without the new flags is that model's by
construction; tests/test_nested_write_model.py pins this one against tests/golden/nested_write.json, the reference's string_builder, and covers by rule what the
reference has no text for: doubles that are not finite, status 19 and BARE | OMIT_NULLS."""
import numpy as np

import write_records_model as plain
from json_text_model import quoted
from nested_write_cases import ARRAY_ROWS, BARE, NEWLINE, OMIT_NULLS

INDEX_OUT_OF_BOUNDS = plain.INDEX_OUT_OF_BOUNDS


def value_text(c, i):
    """cell i of the column c -> (status, its text or None for an invalid one, whether it is a double without a text): the plain model's row of one keyless column"""
    code, text, nulls, nonfinite = plain.row_text([dict(c, key=b"")], i, 0)
    if code:
        return code, None, False
    assert text.startswith(b'{"":') and text.endswith(b"}")
    return 0, None if nulls else text[4:-1], bool(nonfinite)


def row_text(fields, r, flags):
    """-> (status, text: b"" with a status, top-level nulls, doubles without a text, elements, null elements)"""
    array, bare, keyed = bool(flags & ARRAY_ROWS), bool(flags & BARE), not flags & (ARRAY_ROWS | BARE)
    parts, nulls, nonfinite, elements, element_nulls = [], 0, 0, 0, 0
    for f in fields:
        value = None
        if f["list_offsets"] is None:
            code, value, nf = value_text(f, r)
            if code:
                return code, b"", 0, 0, 0, 0
            nonfinite += nf
        elif f["list_valid"] is None or (int(f["list_valid"][r >> 6]) >> (r & 63)) & 1:  # (the offsets of an invalid list decide nothing)
            lo, hi = int(f["list_offsets"][r]), int(f["list_offsets"][r + 1])
            if hi < lo or hi > f["elements"]:
                return INDEX_OUT_OF_BOUNDS, b"", 0, 0, 0, 0
            texts = []
            for e in range(lo, hi):
                code, text, nf = value_text(f, e)
                if code:
                    return code, b"", 0, 0, 0, 0
                nonfinite += nf
                elements += 1
                element_nulls += text is None
                texts.append(b"null" if text is None else text)
            value = b"[" + b",".join(texts) + b"]"
        if value is None:
            nulls += 1
            if flags & OMIT_NULLS:
                continue
            value = b"null"
        parts.append((quoted(f["key"]) + b":" if keyed else b"") + value)
    if bare:
        text = parts[0] if parts else b""
        newline = bool(parts)  # a bare row that was left out is empty: no newline either
    else:
        text = (b"[" if array else b"{") + b",".join(parts) + (b"]" if array else b"}")
        newline = True
    return 0, text + (b"\n" if newline and flags & NEWLINE else b""), nulls, nonfinite, elements, element_nulls


def refused(arrays, flags):
    """the refusals that stand on the flags and K alone"""
    K = len(arrays["fields"])
    return bool(flags & ~15) or (flags & ARRAY_ROWS and flags & (OMIT_NULLS | BARE)) or (flags & BARE and K != 1)


def records(arrays, flags):
    """arrays: nested_write_cases.arrays_of(table) -> (offsets uint32[n + 1], chars bytes, status uint8[n], counts uint64[6])"""
    assert not refused(arrays, flags)
    offsets, parts, status, counts = [0], [], [], [0, 0, 0, 0, 0, 0]
    for r in range(arrays["n"]):
        code, text, nulls, nonfinite, elements, element_nulls = row_text(arrays["fields"], r, flags)
        status.append(code)
        parts.append(text)
        offsets.append(offsets[-1] + len(text))
        if code:
            counts[1] += 1
        else:
            counts[0] += 1
            for j, v in enumerate((nulls, nonfinite, elements, element_nulls)):
                counts[2 + j] += v
    return np.array(offsets, np.uint64).astype(np.uint32), b"".join(parts), np.array(status, np.uint8), np.array(counts, np.uint64)
