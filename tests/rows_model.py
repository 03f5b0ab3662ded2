"""A plain Python at_pointer rooted at a CELL: what a cell of sjgpu_at_pointers_from_cells_device holds (include/sjgpu_rows.h).

Written from the header's table of root cells and from the reference's rules (dom/element-inl.h:410-446 -- a container hands the pointer to its own
at_pointer, a scalar answers a non-empty one with NO_SUCH_FIELD or INVALID_JSON_POINTER --, dom/object-inl.h:104-147 and :246-254,
dom/array-inl.h:94-121 with array::at, jsonpathutil.h:20-50).  It recurses like them, element by element with what is left of the pointer, over the
STREAM's arrays with absolute indices: nothing is compiled ahead, and no code is shared with the host's pointer compiler, the kernel or
tests/pointer_model.py's walk from a document's root.  tests/test_rows_model.py pins it against
tests/golden/pointers.json through the law doc.at_pointer(a).at_pointer(b) == doc.at_pointer(a + b)."""
import numpy as np

E_TYPE, E_INDEX, E_FIELD, E_POINTER = 17, 19, 20, 22
FAILURES = (E_TYPE, E_INDEX, E_FIELD, E_POINTER)
CONTAINERS = (0x7B, 0x5B)
SCALARS = tuple(b'"ludtfn')
M32, M56 = (1 << 32) - 1, (1 << 56) - 1
SIZE_MAX = (1 << 64) - 1


class _Doc:
    """the document an element lies in: where its tape words and its string records begin in the stream's arrays, and where its words end"""

    def __init__(self, tape, sbuf, base, end, str_base):
        self.tape, self.sbuf, self.base, self.end, self.str_base = tape, sbuf, base, end, str_base

    def skip(self, i):
        """the index behind the element that begins at word i"""
        w = int(self.tape[i])
        t = w >> 56
        if t in CONTAINERS:
            return self.base + (w & M32)
        return i + 2 if t in (0x6C, 0x75, 0x64) else i + 1

    def key_at(self, i):
        at = self.str_base + (int(self.tape[i]) & M56)
        n = int.from_bytes(bytes(self.sbuf[at: at + 4]), "little")
        return bytes(self.sbuf[at + 4: at + 4 + n])

    def cell(self, i):
        w = int(self.tape[i])
        t = w >> 56
        if t in (0x6C, 0x75, 0x64):
            return t, int(self.tape[i + 1])
        if t == 0x74:
            return t, 1
        if t in (0x66, 0x6E):
            return t, 0
        if t == 0x22:
            at = self.str_base + (w & M56)
            n = int.from_bytes(bytes(self.sbuf[at: at + 4]), "little")
            return t, (n << 32) | (at + 4)
        assert t in CONTAINERS, t
        return t, ((self.base + (w & M32)) << 32) | i


def _well_formed(pointer):
    """is_pointer_well_formed (jsonpathutil.h): a leading slash, and the FIRST tilde is followed by 0 or 1"""
    if not pointer.startswith(b"/"):
        return False
    e = pointer.find(b"~")
    return e < 0 or pointer[e + 1: e + 2] in (b"0", b"1")


def _element(doc, i, pointer):
    """element::at_pointer of the element at word i"""
    t = int(doc.tape[i]) >> 56
    if t == 0x7B:
        return _object(doc, i, pointer)
    if t == 0x5B:
        return _array(doc, i, pointer)
    if pointer:
        return (E_FIELD if _well_formed(pointer) else E_POINTER), 0
    return doc.cell(i)


def _object(doc, i, pointer):
    if not pointer:
        return doc.cell(i)
    if pointer[:1] != b"/":
        return E_POINTER, 0
    pointer = pointer[1:]
    slash = pointer.find(b"/")
    token = pointer if slash < 0 else pointer[:slash]
    if b"~" in token:
        # unescape; a tilde followed by anything but 0 or 1 -- the end of the token included -- is an invalid pointer
        out, j = bytearray(), 0
        while j < len(token):
            if token[j] == 0x7E:
                nxt = token[j + 1: j + 2]
                if nxt not in (b"0", b"1"):
                    return E_POINTER, 0
                out.append(0x7E if nxt == b"0" else 0x2F)
                j += 2
            else:
                out.append(token[j])
                j += 1
        token = bytes(out)
    close = doc.base + (int(doc.tape[i]) & M32) - 1
    at = i + 1
    while at < close:
        if doc.key_at(at) == token:  # the first field with that key
            return _element(doc, at + 1, b"" if slash < 0 else pointer[slash:])
        at = doc.skip(at + 1)
    return E_FIELD, 0


def _array(doc, i, pointer):
    if not pointer:
        return doc.cell(i)
    if pointer[:1] != b"/":
        return E_POINTER, 0
    pointer = pointer[1:]
    if pointer == b"-":
        return E_INDEX, 0
    index = used = 0
    while used < len(pointer) and pointer[used] != 0x2F:
        digit = pointer[used] - 0x30
        if not 0 <= digit <= 9:
            return E_TYPE, 0
        if used > 0 and pointer[0] == 0x30:
            return E_POINTER, 0  # a leading zero in front of more
        if index > (SIZE_MAX - digit) // 10:
            return E_INDEX, 0
        index = index * 10 + digit
        used += 1
    if used == 0:
        return E_POINTER, 0
    close = doc.base + (int(doc.tape[i]) & M32) - 1
    at = i + 1
    while at < close and index:
        at = doc.skip(at)
        index -= 1
    if at >= close:
        return E_INDEX, 0
    return _element(doc, at, pointer[used:])


def locate(tape, cell, table):
    """the document of a container cell, or None when the cell disagrees with the tape (include/sjgpu_rows.h)"""
    tag, value = int(cell[0]), int(cell[1])
    c, high = value & M32, value >> 32
    begins = table["tape_begin"]
    docs = len(begins) - 1
    d = int(np.searchsorted(begins, c, side="left")) - 1  # the last d with tape_begin[d] < c
    if d < 0 or d >= docs or not int(begins[d]) < c < int(begins[d + 1]):
        return None
    w = int(tape[c])
    if w >> 56 != tag or int(begins[d]) + (w & M32) != high:
        return None
    return d


def root_cell(tape, sbuf, table, d):
    """the cell of document d's root element: what the empty pointer gives in sjgpu_at_pointers_device"""
    base = int(table["tape_begin"][d])
    return _Doc(tape, sbuf, base, int(table["tape_begin"][d + 1]), int(table["string_begin"][d])).cell(base + 1)


def walk_from(tape, sbuf, cell, pointer, table):
    """-> (tag, value) of E.at_pointer(pointer), E the element the cell (tag, value) describes; tape / sbuf: the stream's arrays, table: its documents + 1 DOC_SPAN entries"""
    tag, value = int(cell[0]), int(cell[1])
    pointer = bytes(pointer)
    if tag in FAILURES:
        return tag, 0
    if tag in SCALARS:
        if not pointer:
            return tag, value
        return (E_FIELD if _well_formed(pointer) else E_POINTER), 0
    if tag not in CONTAINERS:
        return E_FIELD, 0
    d = locate(tape, cell, table)
    if d is None:
        return E_FIELD, 0
    doc = _Doc(tape, sbuf, int(table["tape_begin"][d]), int(table["tape_begin"][d + 1]), int(table["string_begin"][d]))
    return _element(doc, value & M32, pointer)


def columns(tape, sbuf, table, roots, pointers):
    """roots: (tags[rows], values[rows]) -> (tags uint8[K, rows], values uint64[K, rows])"""
    root_tags, root_values = roots
    rows = len(root_tags)
    tags, values = np.zeros((len(pointers), rows), np.uint8), np.zeros((len(pointers), rows), np.uint64)
    tape = tape.tolist() if isinstance(tape, np.ndarray) else tape
    sbuf = sbuf.tobytes() if isinstance(sbuf, np.ndarray) else sbuf
    for r in range(rows):
        cell = (int(root_tags[r]), int(root_values[r]))
        for k, p in enumerate(pointers):
            tags[k, r], values[k, r] = walk_from(tape, sbuf, cell, p, table)
    return tags, values
