"""A plain Python `for (key_value_pair f : dom::object(e))` and size() rooted at a CELL: what sjgpu_object_fields_from_cells_device and sjgpu_cell_sizes_device
leave for one root (include/sjgpu_fields.h) -- over the stream's tape, string buffer and document table alone.

The root is settled by tests/rows_model.py's locate (pinned against the reference by the rows fixture), a value's cell is tests/path_model.py's _cell.  What is
new here: the walk over an object's key and value words, the key as a string cell, the header's table of statuses, and the count FIELD of an opening word (bits
32 .. 55, the reference's tape_ref::scope_count) with its two consequences -- a count that reads saturated is walked, and a count that disagrees with the walk
(no tape of a parser has one; the tests patch some) decides how many slots a root has: the fields the walk finds first, then padding.
tests/test_fields_model.py pins it against tests/golden/fields.json (the real reference) and against tests/lists_model.py."""
import struct

import numpy as np

import lists_model
import path_model
import pointer_model
import rows_model
from rows_model import CONTAINERS, E_FIELD, E_TYPE, FAILURES, M32, SCALARS

SATURATED = 0xFFFFFF
PAD = (E_FIELD, 0, E_FIELD, 0)  # a slot the fill did not reach: key tag, key value, value tag, value


def count_field(w):
    return (int(w) >> 32) & SATURATED


class Stream(lists_model.Stream):
    def root(self, cell):
        """-> (status, document or None, opening index) of a root cell"""
        tag, value = int(cell[0]), int(cell[1])
        if tag in FAILURES:
            return tag, None, 0
        if tag in SCALARS:
            return E_TYPE, None, 0
        if tag not in CONTAINERS:
            return E_FIELD, None, 0
        d = rows_model.locate(self.tape, (tag, value), self.table)
        if d is None:
            return E_FIELD, None, 0
        return 0, d, value & M32

    def walk(self, d, c):
        """the fields of the object that opens at absolute word c of document d, in the tape's order -> [(key tag, key value, tag, value)]"""
        tape, sbuf, tb, sb = self.document(d)
        end = (int(self.tape[c]) & M32) - 1  # the closing word, relative to the document
        out, i = [], c - tb + 1
        while i + 1 < end:
            rec = sb + (int(tape[i]) & ((1 << 56) - 1))
            length = struct.unpack_from("<I", self.sbuf, rec)[0]
            tag, value = path_model._cell(tape, sbuf, i + 1, tb, sb)
            out.append((ord('"'), (length << 32) | (rec + 4), tag, value))
            i = pointer_model._next(tape, i + 1)
        return out

    def fields_from(self, cell):
        """-> (status, the slots of the root: [(key tag, key value, tag, value)])"""
        status, d, c = self.root(cell)
        if status == 0 and int(cell[0]) != ord("{"):
            status = E_TYPE  # an array: element::get_object answers INCORRECT_TYPE
        if status:
            return status, []
        found = self.walk(d, c)
        n = count_field(self.tape[c])
        if n == SATURATED:
            n = len(found)
        return 0, found[:n] + [PAD] * (n - len(found))

    def size_of(self, cell):
        """-> (size, code): the count field of a located container's opening word as it stands"""
        status, d, c = self.root(cell)
        return (0, status) if status else (count_field(self.tape[c]), 0)


def column(S, roots):
    """roots: (tags[rows], values[rows]) -> (status uint8[rows], offsets uint32[rows + 1], key_tags uint8[fields], key_values uint64[fields], tags uint8[fields],
    values uint64[fields])"""
    status, offsets, slots = [], [0], []
    for cell in zip(np.asarray(roots[0]).tolist(), np.asarray(roots[1]).tolist()):
        code, found = S.fields_from(cell)
        status.append(code)
        slots += found
        offsets.append(len(slots))
    cols = list(zip(*slots)) if slots else [[], [], [], []]
    return (np.array(status, np.uint8), np.array(offsets, np.uint32), np.array(cols[0], np.uint8), np.array(cols[1], np.uint64), np.array(cols[2], np.uint8),
            np.array(cols[3], np.uint64))


def sizes(S, roots):
    """-> (size uint32[rows], code uint8[rows])"""
    got = [S.size_of(cell) for cell in zip(np.asarray(roots[0]).tolist(), np.asarray(roots[1]).tolist())]
    return np.array([g[0] for g in got], np.uint32), np.array([g[1] for g in got], np.uint8)


def assert_columns(got, want, what=""):
    names = ("status", "offsets", "key_tags", "key_values", "tags", "values")
    for g, w, name in zip(got, want, names):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, f"{what}{name}: shape {g.shape}, the model {w.shape}"
        if not np.array_equal(g, w):
            at = int(np.argwhere(g != w)[0][0])
            raise AssertionError(f"{what}{name}[{at}] = {int(g[at])}, the model {int(w[at])}")
