"""A plain Python model of sjgpu_cast_string_cells_device (include/sjgpu_cast_strings.h): what get_int64_in_string, get_uint64_in_string and
get_double_in_string answer for the content of a string, written from the reference's rules (numberparsing.h: parse_integer_in_string,
parse_unsigned_in_string, parse_double_in_string) with regular expressions, Python's integers and Python's correctly rounded float() -- it shares no code
with the kernels or with sj_number_in_string.h.  tests/test_in_string_model.py pins it against tests/golden/in_string.json (made from the real reference)."""
import json
import math
import os
import re
import struct

import numpy as np

import cast_model

INT64, UINT64, DOUBLE, OR_NUMBER = 1, 2, 3, 0x10
GETTER_NAMES = ["int64", "uint64", "double"]  # the order of the fixture's answers: getter g is GETTER_NAMES[g - 1]
ALL_GETTERS = [INT64, UINT64, DOUBLE, INT64 | OR_NUMBER, UINT64 | OR_NUMBER, DOUBLE | OR_NUMBER]
NUMBER_ERROR, INCORRECT_TYPE, NUMBER_OUT_OF_RANGE = 9, 17, 18
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "in_string.json")

_DIGITS = re.compile(rb"[0-9]*")
_DOUBLE = re.compile(rb"-?[0-9]+(\.[0-9]+)?([eE][+-]?[0-9]{1,19})?")


def integer(content, unsigned):
    """-> (code, value as an unsigned 64-bit pattern)"""
    negative = not unsigned and content[:1] == b"-"
    body = content[1:] if negative else content
    digits = _DIGITS.match(body).group()
    if not digits or len(digits) > (20 if unsigned else 19):
        return INCORRECT_TYPE, 0
    if digits[:1] == b"0" and len(digits) > 1:
        return NUMBER_ERROR, 0
    if len(digits) != len(body):
        return NUMBER_ERROR, 0
    v = -int(digits) if negative else int(digits)
    if not (0 <= v < 1 << 64 if unsigned else -(1 << 63) <= v < 1 << 63):
        return INCORRECT_TYPE, 0
    return 0, v & ((1 << 64) - 1)


def double_grammar(content):
    """-> the code the text alone decides: 17 without a first digit, 9 for every other fault, 0 for a number"""
    body = content[1:] if content[:1] == b"-" else content
    digits = _DIGITS.match(body).group()
    if not digits:
        return INCORRECT_TYPE
    if not _DOUBLE.fullmatch(content) or (digits[:1] == b"0" and len(digits) > 1):
        return NUMBER_ERROR
    return 0


def double(content):
    """-> (code, the 64 bits of the double)"""
    code = double_grammar(content)
    if code:
        return code, 0
    d = float(content.decode("ascii"))
    if math.isinf(d):
        return NUMBER_ERROR, 0
    return 0, struct.unpack("<Q", struct.pack("<d", d))[0]


def answer(content, getter):
    g = getter & 0x0F
    return double(content) if g == DOUBLE else integer(content, g == UINT64)


def load_fixture():
    """-> [(content, [(code, value) per getter int64, uint64, double])]"""
    fx = json.load(open(FIXTURE))
    assert fx["getters"] == GETTER_NAMES
    out = []
    for c, line in zip(fx["contents"], fx["answers"]):
        out.append((bytes.fromhex(c), [(int(a[2:]), 0) if a[0] == "E" else (0, int(a, 16)) for a in line.split(";")]))
    return out


def cast(tags, values, sbuf, getters):
    """tags uint8[K, n], values uint64[K, n], the string buffer's bytes, K getter bytes
    -> (value_out uint64[K, n], code uint8[K, n], valid uint64[K, ceil(n / 64)], counts uint32[K, 8], parked bool[K, n]: the cells the exact road decides)"""
    tags = np.asarray(tags, np.uint8)
    values = np.asarray(values, np.uint64)
    sbuf = bytes(sbuf)
    K, n = tags.shape
    W = (n + 63) // 64
    value_out, code = np.zeros((K, n), np.uint64), np.zeros((K, n), np.uint8)
    valid, counts = np.zeros((K, W), np.uint64), np.zeros((K, 8), np.uint32)
    parked = np.zeros((K, n), bool)
    memo = {}
    for k in range(K):
        g = getters[k] & 0x0F
        numbers_out, numbers_code = cast_model.cast_row(tags[k], values[k], g)  # (the getters 1 .. 3 are the cast's)
        refused = outside = 0
        for i, (t, w) in enumerate(zip(tags[k].tolist(), values[k].tolist())):
            if 1 <= t <= 33:
                c, v = t, 0
            elif t == 0x22:
                off, length = w & 0xFFFFFFFF, w >> 32
                if off + length > len(sbuf):
                    c, v = INCORRECT_TYPE, 0
                    outside += 1
                else:
                    key = (g, off, length)
                    if key not in memo:
                        content = sbuf[off:off + length]
                        slow = g == DOUBLE and takes_the_exact_road(content)
                        memo[key] = (*answer(content, g), slow)
                    c, v, parked[k, i] = memo[key]
            elif getters[k] & OR_NUMBER and t in b"lud":
                c, v = int(numbers_code[i]), int(numbers_out[i])
            else:
                c, v = INCORRECT_TYPE, 0
                refused += 1
            code[k, i], value_out[k, i] = c, v
        bits = np.zeros(W * 64, np.uint8)
        bits[:n] = code[k] == 0
        valid[k] = np.packbits(bits, bitorder="little").view(np.uint64)
        counts[k] = [(code[k] == 0).sum(), (tags[k] == ord("n")).sum(), (code[k] == NUMBER_ERROR).sum(), ((tags[k] >= 1) & (tags[k] <= 33)).sum(), refused, parked[k].sum(), outside, 0]
    return value_out, code, valid, counts, parked


def takes_the_exact_road(content):
    """what slot [5] counts under the double getter: a string of more than 32 bytes, whatever it holds, and a number of more than 19 significant digits"""
    return len(content) > 32 or (double_grammar(content) == 0 and significant_digits(content) > 19)


def significant_digits(content):
    """the digits of the mantissa from the first one that is not 0 on"""
    mantissa = re.match(rb"-?([0-9]*\.?[0-9]*)", content).group(1).replace(b".", b"")
    return len(mantissa.lstrip(b"0"))
