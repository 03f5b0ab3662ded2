"""A plain Python recursion over ONE tape + string buffer for one JSONPath with wildcards: what a cell of sjgpu_at_paths_device holds
(include/sjgpu_paths.h) -- its status and its matches in order.

Written from the reference's rules (dom/element-inl.h:448-459, dom/object-inl.h:155-244, dom/array-inl.h:129-214, jsonpathutil.h:58-161): it recurses
like them and parses what is left of the path at every invocation, so nothing is compiled ahead and no code path is shared with the host's level
compiler (sj_path_program.h) or the kernel.  The at_pointer parts are tests/pointer_model.py's walk, asked of a copy of the element's sub-tape.
tests/test_path_model.py pins it against tests/golden/paths.json (made from the real reference) and against Python's json."""
import pointer_model
from pointer_model import CODES, INVALID_JSON_POINTER, LOW32

OPEN, CLOSE, NUMBERS = (ord("{"), ord("[")), (ord("}"), ord("]")), (ord("l"), ord("u"), ord("d"))


def _sub_tape(tape, c):
    """the element that begins at word c as a document of its own: [root word] + its words, the brackets' payloads moved by c - 1"""
    if c == 1:
        return tape
    nxt = pointer_model._next(tape, c)
    shift = c - 1
    out = [0] + [int(w) for w in tape[c:nxt]]
    i = 1
    while i < len(out):
        t = out[i] >> 56
        if t in OPEN or t in CLOSE:
            out[i] -= shift  # (an opening word: the index behind its partner in the low 32 bits; a closing word: its partner's index)
        i += 2 if t in NUMBERS else 1
    return out


def _cell(tape, sbuf, c, tb, sb):
    """the element at word c in the cell encoding of include/sjgpu_query.h"""
    return pointer_model.walk(_sub_tape(tape, c), sbuf, b"", tb + c - 1, sb)


def _at_pointer(tape, sbuf, c, pointer, tb, sb):
    return pointer_model.walk(_sub_tape(tape, c), sbuf, pointer, tb + c - 1, sb)


def _children(tape, c):
    """the words at which the child VALUES of the container at c begin"""
    w = int(tape[c])
    end = (w & LOW32) - 1
    step = 1 if (w >> 56) == ord("{") else 0
    out, i = [], c + 1 + step
    while i < end:
        out.append(i)
        i = pointer_model._next(tape, i) + step
    return out


def _next_key(r):
    """get_next_key_and_json_path -> (key, what is left); an empty key: none"""
    i = 1 if r[:1] == b"$" else 0
    key = b""
    if r[i: i + 1] == b".":
        i += 1
        start = i
        while i < len(r) and r[i: i + 1] not in (b"[", b"."):
            i += 1
        key = r[start:i]
    elif i + 1 < len(r) and r[i: i + 1] == b"[" and r[i + 1: i + 2] in (b"'", b'"'):
        quote = r[i + 1: i + 2]
        i += 2
        start = i
        while i < len(r) and r[i: i + 1] != quote:
            i += 1
        if i >= len(r) or i + 1 >= len(r) or r[i + 1: i + 2] != b"]":
            return b"", r
        key = r[start:i]
        i += 2
    elif i + 2 < len(r) and r[i: i + 3] == b"[*]":
        key = b"*"
        i += 3
    return key, r[i:]


def _to_pointer(r):
    """json_path_to_pointer_conversion -> the pointer, or None for the sentinel"""
    i = 1 if r[:1] == b"$" else 0
    if i >= len(r) or r[i: i + 1] not in (b".", b"["):
        return None
    esc = {0x7E: b"~0", 0x2F: b"~1"}
    out = bytearray()
    while i < len(r):
        if r[i] == 0x2E:
            out += b"/"
        elif r[i] == 0x5B:
            out += b"/"
            i += 1
            while i < len(r) and r[i] != 0x5D:
                out += esc.get(r[i], r[i: i + 1])
                i += 1
            if i == len(r):
                return None
        else:
            out += esc.get(r[i], r[i: i + 1])
        i += 1
    return bytes(out)


def _element(tape, sbuf, c, r, tb, sb):
    """element::at_path_with_wildcard of the element at word c -> (code, [(tag, value)])"""
    if (int(tape[c]) >> 56) not in OPEN:
        return 0, []
    i = 1 if r[:1] == b"$" else 0
    if i >= len(r) or r[i: i + 1] not in (b".", b"["):
        return INVALID_JSON_POINTER, []
    if b"*" not in r:
        pointer = _to_pointer(r)
        if pointer is None:
            return INVALID_JSON_POINTER, []
        tag, value = _at_pointer(tape, sbuf, c, pointer, tb, sb)
        return (tag, []) if tag in CODES else (0, [(tag, value)])
    if r[i:] in (b"[*]", b".*"):
        return 0, [_cell(tape, sbuf, ch, tb, sb) for ch in _children(tape, c)]
    key, rest = _next_key(r)
    if not key:
        return INVALID_JSON_POINTER, []
    if key == b"*":
        kids = _children(tape, c)
    else:
        tag, value = _at_pointer(tape, sbuf, c, b"/" + key, tb, sb)
        # (a scalar found has no position in its cell, and needs none: it contributes nothing to whatever follows)
        kids = [(value & LOW32) - tb] if tag in OPEN else []
    out = []
    for ch in kids:
        code, found = _element(tape, sbuf, ch, rest, tb, sb)
        if not code:
            out += found
    return 0, out


def matches(tape, sbuf, path, tape_begin=0, string_begin=0):
    """-> (status, [(tag, value)]) of dom::parser::parse(document).at_path_with_wildcard(path): tape / sbuf are the document's own slices,
    tape_begin / string_begin where they lie in the stream's arrays"""
    return _element(tape, sbuf, 1, bytes(path), tape_begin, string_begin)


def column(tapes, paths):
    """tapes: [(tape, string_buf)] per document, laid out back to back -> (status[K][docs], offsets[K * docs + 1], tags[matches], values[matches]) as plain lists"""
    cells = {}
    tb = sb = 0
    for d, (tape, sbuf) in enumerate(tapes):
        for k, p in enumerate(paths):
            cells[k, d] = matches(tape, sbuf, p, tb, sb)
        tb += len(tape)
        sb += len(sbuf)
    status = [[cells[k, d][0] for d in range(len(tapes))] for k in range(len(paths))]
    offsets, tags, values = [0], [], []
    for k in range(len(paths)):
        for d in range(len(tapes)):
            for t, v in cells[k, d][1]:
                tags.append(t)
                values.append(v)
            offsets.append(len(tags))
    return status, offsets, tags, values
