"""A plain Python model of sjgpu_dictionary_encode_device and sjgpu_cell_kinds_by_code_device (include/sjgpu_dict.h): a `dict` keyed by the bytes of every string
cell, read from cell 0 upwards -- std::unordered_map<std::string_view, ...> over what get_string() returns -- and tests/cast_model.py's census per group.  It
shares no code with the kernels.  tests/test_dictionary_model.py pins it against tests/golden/dictionary.json (made from the real reference)."""
import numpy as np

import cast_model

STRING = ord('"')


def string_of(sbuf, tag, value, string_bytes=None):
    """the bytes of a string cell inside sbuf[0 .. string_bytes), None for every other cell (a null of the encode)"""
    string_bytes = len(sbuf) if string_bytes is None else string_bytes
    at, length = int(value) & 0xFFFFFFFF, int(value) >> 32
    if int(tag) != STRING or at + length > string_bytes:
        return None
    return bytes(sbuf[at: at + length])


def encode(tags, values, sbuf, string_bytes=None):
    """one row -> (codes int32[n], first uint32[G], dict_values uint64[G], counts uint32[G]); the dictionary's tags are G times '"'"""
    sbuf = bytes(sbuf) if not isinstance(sbuf, (bytes, bytearray)) else sbuf
    seen, first, counts = {}, [], []
    codes = np.full(len(tags), -1, np.int32)
    for r, (t, v) in enumerate(zip(np.asarray(tags, np.uint8).tolist(), np.asarray(values, np.uint64).tolist())):
        s = string_of(sbuf, t, v, string_bytes)
        if s is None:
            continue
        j = seen.setdefault(s, len(seen))
        if j == len(first):
            first.append(r)
            counts.append(0)
        counts[j] += 1
        codes[r] = j
    first = np.array(first, np.uint32)
    return codes, first, np.asarray(values, np.uint64)[first], np.array(counts, np.uint32)


def strings(tags, values, sbuf):
    """the dictionary of a row as bytes, in order of first occurrence"""
    _, first, dict_values, _ = encode(tags, values, sbuf)
    return [string_of(sbuf, STRING, v) for v in dict_values.tolist()]


def kinds_by_code(codes, tags, values, groups):
    """-> uint32[groups, 16]: tests/cast_model.py's census of the cells whose code is g, for every g < groups; other codes count nowhere"""
    codes, tags, values = np.asarray(codes, np.int32), np.asarray(tags, np.uint8), np.asarray(values, np.uint64)
    out = np.zeros((groups, 16), np.uint32)
    for g in np.unique(codes[(codes >= 0) & (codes < groups)]).tolist():
        pick = codes == g
        out[g] = cast_model.kinds(tags[pick][None, :], values[pick][None, :])[0]
    return out
