"""A plain Python at_path_with_wildcard rooted at a CELL: what a cell of sjgpu_at_paths_from_cells_device holds (include/sjgpu_lists.h) -- its status and its
matches in order.

Two parts that are pinned against the real reference already: tests/rows_model.py's locate for the root (which document a container cell lies in, and whether
it agrees with the tape) and tests/path_model.py's _element -- the reference's recursion -- over that document's own slices.  What is new here is the header's
table of root cells: a failed root keeps its code, a scalar root matches nothing and is no error, a cell that is no element is NO_SUCH_FIELD -- for every
path, the empty and the malformed ones included.  tests/test_lists_model.py pins it against tests/golden/lists.json (the real reference, asked
e.at_path_with_wildcard(q) for every e of doc.at_path_with_wildcard(p)) and, through the law of composition, against tests/golden/paths.json."""
import numpy as np

import path_model
import rows_model
from rows_model import CONTAINERS, E_FIELD, FAILURES, M32, SCALARS


class Stream:
    """the stream's arrays, and its documents' own slices (made when a root first asks for them)"""

    def __init__(self, tape, sbuf, table):
        self.tape = tape.tolist() if isinstance(tape, np.ndarray) else tape
        self.sbuf = sbuf.tobytes() if isinstance(sbuf, np.ndarray) else sbuf
        self.table = table
        self.slices = {}

    def document(self, d):
        if d not in self.slices:
            tb, te = int(self.table["tape_begin"][d]), int(self.table["tape_begin"][d + 1])
            sb, se = int(self.table["string_begin"][d]), int(self.table["string_begin"][d + 1])
            self.slices[d] = (self.tape[tb:te], self.sbuf[sb:se], tb, sb)
        return self.slices[d]

    def matches_from(self, cell, path):
        """-> (status, [(tag, value)]) of E.at_path_with_wildcard(path), E the element the cell (tag, value) describes"""
        tag, value = int(cell[0]), int(cell[1])
        if tag in FAILURES:
            return tag, []
        if tag in SCALARS:
            return 0, []
        if tag not in CONTAINERS:
            return E_FIELD, []
        d = rows_model.locate(self.tape, (tag, value), self.table)
        if d is None:
            return E_FIELD, []
        tape, sbuf, tb, sb = self.document(d)
        return path_model._element(tape, sbuf, (value & M32) - tb, bytes(path), tb, sb)


def column(tape, sbuf, table, roots, paths):
    """roots: (tags[rows], values[rows]) -> (status uint8[K, rows], offsets uint32[K * rows + 1], tags uint8[matches], values uint64[matches])"""
    S = tape if isinstance(tape, Stream) else Stream(tape, sbuf, table)
    root_tags, root_values = roots
    rows = len(root_tags)
    status = np.zeros((len(paths), rows), np.uint8)
    offsets, tags, values = [0], [], []
    for k, p in enumerate(paths):
        for r in range(rows):
            code, found = S.matches_from((root_tags[r], root_values[r]), p)
            status[k, r] = code
            for t, v in found:
                tags.append(t)
                values.append(v)
            offsets.append(len(tags))
    return status, np.array(offsets, np.uint32), np.array(tags, np.uint8), np.array(values, np.uint64)
