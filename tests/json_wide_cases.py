"""Shared by the tests of the wide JSON text call (tests/test_json_wide_emu.py, tests/test_gpu_json_wide.py): the cases that only a call with one lane per tape word
can get wrong, beside the narrow call's cases of tests/json_text_cases.py -- roots that overlap, roots whose word counts stand on the edges of the lanes', the waves' and
the workgroups' shares, a parity that crosses workgroups, second words of numbers that look like tags at the borders of the shares, empty containers in every place,
and the row whose range space is beyond 32 bits."""
import numpy as np

import path_model

LANE_SHARE, WAVE_SHARE, WORKGROUP_SHARE = 1, 64, 256  # slots of the range space (sjgpu_json_wide.hip: one slot per lane, JW_THREADS lanes)
SHARE_EDGE_WORDS = [WAVE_SHARE - 1, WAVE_SHARE, WAVE_SHARE + 1, WORKGROUP_SHARE - 1, WORKGROUP_SHARE, WORKGROUP_SHARE + 1, 2 * WORKGROUP_SHARE - 1, 2 * WORKGROUP_SHARE,
                    2 * WORKGROUP_SHARE + 1]
BORDER_SLOTS = [WAVE_SHARE - 1, WAVE_SHARE, WORKGROUP_SHARE - 1, WORKGROUP_SHARE]  # where the number's SECOND word lies, counted from its root's opening word
TAG_LIKE_INTEGERS = [0x7B << 56, 0x5D << 56, 0x6C << 56]  # int64 values whose top byte is { ] l
RANGE_LIMIT = 0xFFFFFFF0

NESTED_DOCUMENT = b'{"a":[1,{"b":[true,null,"x"]},2.5],"c":{"d":"e"},"f":[]}'
EMPTY_CONTAINER_DOCUMENTS = [b'[{},1,[],"a",{}]', b'{"a":{},"b":[],"c":{}}', b"[[],[],[]]", b"[{}]", b'{"a":[]}', b"[[[]],{},[{}]]", b"{}", b"[]", b'[1,{},2]']


def document_of_words(words):
    """an array whose tape has exactly `words` words between its opening and its closing word, both included: words - 2 literals"""
    assert words >= 2
    return b"[" + b",".join([b"true", b"false", b"null"][i % 3] for i in range(words - 2)) + b"]"


def wide_object(fields):
    """an object of `fields` fields, minified: strings, integers, literals and small containers as values, so that a key is told from a string value by parity alone"""
    def value(i):
        return (b'"v%d"' % i, b"%d" % i, b"true", b'{"x":[]}')[i % 4]
    return b"{" + b",".join(b'"k%d":' % i + value(i) for i in range(fields)) + b"}"


def number_at_slot(slot, value):
    """an array, minified, whose word `slot` (the opening word is word 0) is the second word of the integer `value`; more of them and an object follow"""
    items = [b"null"] * (slot - 2) + [b"%d" % value, b'"x"', b'{"a":%d}' % value, b"%d" % value, b"%d" % value, b"[%d]" % value]
    return b"[" + b",".join(items) + b"]"


def children(stream, path=b"$.*"):
    """the cells of `path` in the first document of a stream (tape, sbuf, table) -> [(tag, value)]"""
    tape, sbuf, table = stream
    tb, te = int(table["tape_begin"][0]), int(table["tape_begin"][1])
    sb, se = int(table["string_begin"][0]), int(table["string_begin"][1])
    code, found = path_model.matches(np.asarray(tape)[tb:te].tolist(), np.asarray(sbuf)[sb:se].tobytes(), path, tb, sb)
    return found


def overlapping_row(stream):
    """the root of NESTED_DOCUMENT twice, its first child -- a container inside it --, and the root once more"""
    import rows_model
    root = rows_model.root_cell(*stream, 0)
    child = children(stream)[0]
    cells = [root, root, child, root]
    assert chr(child[0]) == "["
    return np.array([t for t, _ in cells], np.uint8), np.array([v for _, v in cells], np.uint64)


RANGE_ROOTS, RANGE_ONES = 65537, 32767
RANGE_DOCUMENT = b"[" + b",".join([b"1"] * RANGE_ONES) + b"]"  # 65 536 words


def range_row(root_tag, root_value):
    """RANGE_ROOTS times the same root: 65 537 x 65 536 = 2^32 + 65 536 slots"""
    assert (int(root_value) >> 32) - (int(root_value) & 0xFFFFFFFF) == 2 * RANGE_ONES + 2
    assert RANGE_ROOTS * (2 * RANGE_ONES + 2) > RANGE_LIMIT
    return np.full(RANGE_ROOTS, root_tag, np.uint8), np.full(RANGE_ROOTS, root_value, np.uint64)


def range_refusal(orc, parsed_stream):
    import rows_model
    stream = parsed_stream(orc, [RANGE_DOCUMENT])
    tag, value = rows_model.root_cell(*stream, 0)
    return stream, range_row(tag, value)
