"""A plain Python walk of ONE tape + string buffer for one JSON pointer: what a cell of sjgpu_at_pointers_device holds (include/sjgpu_query.h).

Written from the reference's rules (dom/element-inl.h:410-446, dom/object-inl.h:104-147 and :246-254, dom/array-inl.h:94-121 with array::at,
jsonpathutil.h:20-50), token by token and lazily like them -- nothing is compiled ahead, so it shares no code path with the host's pointer
compiler or the kernel.  tests/test_pointer_model.py pins it against tests/golden/pointers.json (made from the real reference) and against
Python's json."""
import numpy as np

INCORRECT_TYPE, INDEX_OUT_OF_BOUNDS, NO_SUCH_FIELD, INVALID_JSON_POINTER = 17, 19, 20, 22
CODES = (INCORRECT_TYPE, INDEX_OUT_OF_BOUNDS, NO_SUCH_FIELD, INVALID_JSON_POINTER)
SIZE_MAX = (1 << 64) - 1
LOW32, PAYLOAD = 0xFFFFFFFF, (1 << 56) - 1


def _next(tape, i):
    """the index behind the element that begins at word i (payloads relative to tape[0])"""
    w = int(tape[i])
    t = w >> 56
    if t in (ord("{"), ord("[")):
        return w & LOW32
    return i + 2 if t in (ord("l"), ord("u"), ord("d")) else i + 1


def _string(sbuf, payload):
    n = int.from_bytes(bytes(sbuf[payload: payload + 4]), "little")
    return payload + 4, n


def _well_formed(rest):
    """is_pointer_well_formed: only the first `~` counts"""
    if rest[:1] != b"/":
        return False
    e = rest.find(b"~")
    if e < 0:
        return True
    return e != len(rest) - 1 and rest[e + 1: e + 2] in (b"0", b"1")


def _array_index(rest):
    """parse_json_pointer_array_index over `rest` (no leading slash) -> (code, index, token length)"""
    index, j = 0, 0
    while j < len(rest) and rest[j: j + 1] != b"/":
        digit = (rest[j] - 48) & 0xFF
        if digit > 9:
            return INCORRECT_TYPE, 0, j
        if j > 0 and rest[:1] == b"0":
            return INVALID_JSON_POINTER, 0, j
        if index > (SIZE_MAX - digit) // 10:
            return INDEX_OUT_OF_BOUNDS, 0, j
        index = index * 10 + digit
        j += 1
    if j == 0:
        return INVALID_JSON_POINTER, 0, 0
    return 0, index, j


def walk(tape, sbuf, pointer, tape_begin=0, string_begin=0):
    """-> (tag, value) of dom::parser::parse(document).at_pointer(pointer) in the cell format: tape / sbuf are the document's own slices,
    tape_begin / string_begin where they lie in the stream's arrays (what makes the offsets of the cell absolute)"""
    pointer = bytes(pointer)
    cur = 1
    while True:
        w = int(tape[cur])
        t = w >> 56
        if t == ord("{"):
            if not pointer:
                break
            if pointer[:1] != b"/":
                return INVALID_JSON_POINTER, 0
            rest = pointer[1:]
            slash = rest.find(b"/")
            token = rest if slash < 0 else rest[:slash]
            key = bytearray()
            j = 0
            while j < len(token):
                if token[j] != 0x7E:
                    key.append(token[j])
                    j += 1
                    continue
                nxt = token[j + 1: j + 2]  # (the reference reads the terminator behind its copy: nothing there is neither 0 nor 1)
                if nxt == b"0":
                    key.append(0x7E)
                elif nxt == b"1":
                    key.append(0x2F)
                else:
                    return INVALID_JSON_POINTER, 0
                j += 2
            key = bytes(key)
            end = (w & LOW32) - 1
            i = cur + 1
            found = None
            while i < end:
                at, n = _string(sbuf, int(tape[i]) & PAYLOAD)
                if n == len(key) and bytes(sbuf[at: at + n]) == key:
                    found = i + 1
                    break
                i = _next(tape, i + 1)
            if found is None:
                return NO_SUCH_FIELD, 0
            cur = found
            pointer = b"" if slash < 0 else rest[slash:]
        elif t == ord("["):
            if not pointer:
                break
            if pointer[:1] != b"/":
                return INVALID_JSON_POINTER, 0
            rest = pointer[1:]
            if rest == b"-":
                return INDEX_OUT_OF_BOUNDS, 0
            code, index, used = _array_index(rest)
            if code:
                return code, 0
            end = (w & LOW32) - 1
            i = cur + 1
            k = 0
            while i < end and k < index:
                i = _next(tape, i)
                k += 1
            if i >= end:
                return INDEX_OUT_OF_BOUNDS, 0
            cur = i
            pointer = rest[used:]
        else:
            if pointer:
                return (NO_SUCH_FIELD if _well_formed(pointer) else INVALID_JSON_POINTER), 0
            break
    w = int(tape[cur])
    t = w >> 56
    if t in (ord("l"), ord("u"), ord("d")):
        return t, int(tape[cur + 1])
    if t == ord("t"):
        return t, 1
    if t in (ord("f"), ord("n")):
        return t, 0
    if t == ord('"'):
        at, n = _string(sbuf, w & PAYLOAD)
        return t, (n << 32) | (string_begin + at)
    assert t in (ord("{"), ord("["))
    return t, ((tape_begin + (w & LOW32)) << 32) | (tape_begin + cur)


def string_of(sbuf, value):
    """the bytes of a string cell (sbuf: the array the cell's offset is absolute in)"""
    at, n = value & LOW32, value >> 32
    return bytes(sbuf[at: at + n])


def columns(tapes, pointers):
    """tapes: [(tape, string_buf)] per document, laid out back to back as sjgpu_stage2_many_device lays them out -> (tags uint8[K, docs], values uint64[K, docs])"""
    tags = np.zeros((len(pointers), len(tapes)), np.uint8)
    values = np.zeros((len(pointers), len(tapes)), np.uint64)
    tb = sb = 0
    for d, (tape, sbuf) in enumerate(tapes):
        for k, p in enumerate(pointers):
            t, v = walk(tape, sbuf, p, tb, sb)
            tags[k, d] = t
            values[k, d] = v
        tb += len(tape)
        sb += len(sbuf)
    return tags, values
