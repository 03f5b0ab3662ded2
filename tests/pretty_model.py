"""A plain Python simdjson::prettify(element) rooted at a CELL: what sjgpu_prettify_cells_device and sjgpu_prettify_cells_wide_device leave for one root
(include/sjgpu_pretty.h) -- its status and its text -- over the stream's tape, string buffer and document table alone.

Written from the reference's own shape, not from the kernels': the kernels lay a word out from the number of containers open around it, taken mod 16; this model keeps
the reference's two procedures apart -- an ELEMENT is written from indent 0 and ends with a newline (string_builder::append(element)); a container met at the 16th
level of one element is written FLAT, each child of it as an element of its own (append(array) / append(object)).  The scalars, the strings and every reason to
refuse a sub-tape are tests/json_text_model.py's.  tests/test_pretty_model.py pins all of it against tests/golden/pretty.json (the real reference)."""
import json_text_model
import rows_model
from json_text_model import MAX_LEVELS, Malformed
from rows_model import CONTAINERS, E_FIELD, M32

INDENT_STEP = 4
ELEMENT_LEVELS = 16  # the reference's MAX_DEPTH: an element lays out that many levels itself


class Stream(json_text_model.Stream):
    def _closing(self, i, limit, d, level):
        """the checks of json_text_model's _container on the container that opens at word i -> the index of its closing word"""
        if level >= MAX_LEVELS:
            raise Malformed("too deep")
        base = int(self.table["tape_begin"][d])
        w = self.tape[i]
        close = base + (w & M32) - 1
        if not i < close < limit:
            raise Malformed("a container that does not end inside what surrounds it")
        cw = self.tape[close]
        if cw >> 56 != (w >> 56) + 2 or base + (cw & M32) != i:
            raise Malformed("a closing word that does not match")
        return close

    def _key(self, at, d):
        kw = self.tape[at]
        if kw >> 56 != 0x22:
            raise Malformed("a key that is no string")
        return self._string(kw, d)

    def _element(self, i, limit, d, level, out):
        """append(element): the value at word i from indent 0, and a newline -> the index behind it"""
        at = self._laid_out(i, limit, d, level, 0, out)
        out.append(b"\n")
        return at

    def _laid_out(self, i, limit, d, level, depth, out):
        """the value at word i, `depth` containers of its element open around it (its own indent is written already) -> the index behind it"""
        if i >= limit:
            raise Malformed("a value where the container ends")
        w = self.tape[i]
        t = w >> 56
        if t not in CONTAINERS:
            return json_text_model.Stream._value(self, i, limit, d, level, out)
        close = self._closing(i, limit, d, level)
        is_object = t == 0x7B
        if depth + 1 >= ELEMENT_LEVELS:
            return self._flat(i, close, d, level, is_object, out)
        out.append(bytes([t]))
        at, first = i + 1, True
        while at < close:
            out.append(b"\n" if first else b",\n")
            first = False
            out.append(b" " * (INDENT_STEP * (depth + 1)))
            if is_object:
                out.append(self._key(at, d) + b": ")
                at += 1
            at = self._laid_out(at, close, d, level + 1, depth + 1, out)
        if at != close:
            raise Malformed("a child that runs over its container's end")
        if not first:
            out.append(b"\n" + b" " * (INDENT_STEP * depth))
        out.append(bytes([t + 2]))
        return close + 1

    def _flat(self, i, close, d, level, is_object, out):
        """append(array) / append(object): no blank, no newline of its own; every child an element"""
        t = self.tape[i] >> 56
        out.append(bytes([t]))
        at, first = i + 1, True
        while at < close:
            if not first:
                out.append(b",")
            first = False
            if is_object:
                out.append(self._key(at, d) + b":")
                at += 1
            at = self._element(at, close, d, level + 1, out)
        if at != close:
            raise Malformed("a child that runs over its container's end")
        out.append(bytes([t + 2]))
        return close + 1

    def text_of(self, cell):
        """-> (status, the text: b"" with a status)"""
        tag, value = int(cell[0]), int(cell[1])
        if tag not in CONTAINERS:
            status, text = json_text_model.Stream.text_of(self, cell)
            return status, text + b"\n" if status == 0 else b""
        try:
            d = rows_model.locate(self.tape, (tag, value), self.table)
            if d is None:
                return E_FIELD, b""
            high = value >> 32
            if high > int(self.table["tape_begin"][d + 1]):
                return E_FIELD, b""
            out = []
            if self._element(value & M32, high, d, 0, out) != high:
                return E_FIELD, b""
            return 0, b"".join(out)
        except Malformed:
            return E_FIELD, b""


def column(S, roots):
    """roots: (tags[rows], values[rows]) -> (offsets uint32[rows + 1], chars bytes, status uint8[rows])"""
    return json_text_model.column(S, roots)


def text_bytes(S, cell):
    """the length of one cell's text alone (for totals that no list holds)"""
    return len(S.text_of(cell)[1])

