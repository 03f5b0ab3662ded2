"""A plain Python simdjson::minify(element) rooted at a CELL: what sjgpu_serialize_cells_device leaves for one root (include/sjgpu_json.h) -- its status and its
text -- over the stream's tape, string buffer and document table alone.

Written from the header's contract, not from the kernel: the root is settled by tests/rows_model.py's locate (pinned against the reference by the rows fixture);
a container is read RECURSIVELY, child by child between its opening word and the closing word that word names (the kernel walks linearly with a bit per level);
a double's digits come from Python's repr(float) -- the shortest that round-trip, the closest among them -- and only their layout is restated here; an integer is
Python's str(int); a string is escaped from a table.  tests/test_json_text_model.py pins all of it against tests/golden/json_text.json (the real reference)."""
import struct
import sys

import numpy as np

import rows_model
from rows_model import CONTAINERS, E_FIELD, FAILURES, M32, M56

MAX_LEVELS = 4096
sys.setrecursionlimit(max(sys.getrecursionlimit(), 3 * MAX_LEVELS))  # (two frames per nesting level)
ESCAPES = {0x22: b'\\"', 0x5C: b"\\\\", 0x08: b"\\b", 0x09: b"\\t", 0x0A: b"\\n", 0x0C: b"\\f", 0x0D: b"\\r"}
ESCAPED = [ESCAPES.get(c, b"\\u%04x" % c if c < 0x20 else bytes([c])) for c in range(256)]


class Malformed(Exception):
    pass


def quoted(s):
    return b'"' + b"".join(ESCAPED[c] for c in s) + b'"'


def double_text(bits):
    """the reference's to_chars(double) for the finite double with these bits"""
    x = struct.unpack("<d", struct.pack("<Q", bits))[0]
    sign = "-" if bits >> 63 else ""
    x = abs(x)
    if x == 0:
        return (sign + "0.0").encode()
    mantissa, _, exponent = repr(x).partition("e")
    whole, _, fraction = mantissa.partition(".")
    digits = (whole + fraction).lstrip("0")
    e = (int(exponent) if exponent else 0) - len(fraction)
    stripped = digits.rstrip("0")
    e += len(digits) - len(stripped)
    digits = stripped
    k, n = len(digits), len(digits) + e  # n: where the decimal point lies behind the first digit
    if k <= n <= 15:
        text = digits + "0" * (n - k) + ".0"
    elif 0 < n <= 15:
        text = digits[:n] + "." + digits[n:]
    elif -4 < n <= 0:
        text = "0." + "0" * -n + digits
    else:
        text = (digits if k == 1 else digits[0] + "." + digits[1:]) + "e" + ("-" if n - 1 < 0 else "+") + "%02d" % abs(n - 1)
    return (sign + text).encode()


def number_text(tag, word):
    if tag == 0x6C:
        return b"%d" % (word - (1 << 64) if word >> 63 else word)
    if tag == 0x75:
        return b"%d" % word
    if (word >> 52) & 0x7FF == 0x7FF:
        raise Malformed("a double that is no finite number")
    return double_text(word)


LITERALS = {0x74: b"true", 0x66: b"false", 0x6E: b"null"}


class Stream:
    def __init__(self, tape, sbuf, table, string_bytes=None):
        self.tape = tape.tolist() if isinstance(tape, np.ndarray) else tape
        self.sbuf = sbuf.tobytes() if isinstance(sbuf, np.ndarray) else bytes(sbuf)
        self.table = table
        self.string_bytes = len(self.sbuf) if string_bytes is None else string_bytes

    def _string(self, w, d):
        sb, se = int(self.table["string_begin"][d]), int(self.table["string_begin"][d + 1])
        rec = sb + (w & M56)
        if rec + 4 > se:
            raise Malformed("a string record outside the document's buffer")
        n = struct.unpack_from("<I", self.sbuf, rec)[0]
        if rec + 4 + n > se:
            raise Malformed("a string that ends outside the document's buffer")
        return quoted(self.sbuf[rec + 4: rec + 4 + n])

    def _value(self, i, limit, d, level, out):
        """the element that begins at word i and must end at or in front of `limit` -> the index behind it"""
        if i >= limit:
            raise Malformed("a value where the container ends")
        w = self.tape[i]
        t = w >> 56
        if t in CONTAINERS:
            return self._container(i, limit, d, level, out)
        if t == 0x22:
            out.append(self._string(w, d))
            return i + 1
        if t in (0x6C, 0x75, 0x64):
            if i + 1 >= limit:
                raise Malformed("a number without its second word")
            out.append(number_text(t, self.tape[i + 1]))
            return i + 2
        if t in LITERALS:
            out.append(LITERALS[t])
            return i + 1
        raise Malformed("a tag outside the ten")

    def _container(self, i, limit, d, level, out):
        if level >= MAX_LEVELS:
            raise Malformed("too deep")
        base = int(self.table["tape_begin"][d])
        w = self.tape[i]
        t = w >> 56
        close = base + (w & M32) - 1
        if not i < close < limit:
            raise Malformed("a container that does not end inside what surrounds it")
        cw = self.tape[close]
        if cw >> 56 != t + 2 or base + (cw & M32) != i:
            raise Malformed("a closing word that does not match")
        out.append(bytes([t]))
        at, first = i + 1, True
        while at < close:
            if not first:
                out.append(b",")
            first = False
            if t == 0x7B:
                kw = self.tape[at]
                if kw >> 56 != 0x22:
                    raise Malformed("a key that is no string")
                out.append(self._string(kw, d))
                out.append(b":")
                at += 1
            at = self._value(at, close, d, level + 1, out)
        if at != close:
            raise Malformed("a child that runs over its container's end")
        out.append(bytes([t + 2]))
        return close + 1

    def text_of(self, cell):
        """-> (status, the text: b"" with a status)"""
        tag, value = int(cell[0]), int(cell[1])
        if tag in FAILURES:
            return tag, b""
        try:
            if tag in LITERALS:
                return 0, LITERALS[tag]
            if tag in (0x6C, 0x75, 0x64):
                return 0, number_text(tag, value)
            if tag == 0x22:
                at, n = value & M32, value >> 32
                if at + n > self.string_bytes:
                    return E_FIELD, b""
                return 0, quoted(self.sbuf[at: at + n])
            if tag not in CONTAINERS:
                return E_FIELD, b""
            d = rows_model.locate(self.tape, (tag, value), self.table)
            if d is None:
                return E_FIELD, b""
            high = value >> 32
            if high > int(self.table["tape_begin"][d + 1]):
                return E_FIELD, b""
            out = []
            if self._container(value & M32, high, d, 0, out) != high:
                return E_FIELD, b""
            return 0, b"".join(out)
        except Malformed:
            return E_FIELD, b""


def column(S, roots):
    """roots: (tags[rows], values[rows]) -> (offsets uint32[rows + 1], chars bytes, status uint8[rows])"""
    offsets, parts, status = [0], [], []
    for cell in zip(np.asarray(roots[0]).tolist(), np.asarray(roots[1]).tolist()):
        code, text = S.text_of(cell)
        status.append(code)
        parts.append(text)
        offsets.append(offsets[-1] + len(text))
    return np.array(offsets, np.uint32), b"".join(parts), np.array(status, np.uint8)
