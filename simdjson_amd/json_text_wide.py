"""Cells as JSON text, breadth first (include/sjgpu_json_wide.h): the calls of simdjson_amd/json_text.py through sjgpu_serialize_cells_wide_device, which has the narrow
call's contract and one lane per tape word where that has one lane per cell -- the call to take for ONE large document, `$.statuses`, or any large sub-tree.  Free
functions that take a capi.DomParserImplementation as their first argument, for the reason json_text's are; they return what their narrow twins return, with the same
capacity retry.  Which of the two to take is the caller's decision."""
import ctypes

from .json_text import _documents_as_json, _json_column

_NAME = "sjgpu_serialize_cells_wide_device"


def serialize_cells_wide_device(p, tape_ptr, tape_words, strbuf_ptr, strbuf_bytes, docs_ptr, docs, root_value_ptr, root_tag_ptr, rows, offsets_ptr, status_ptr, chars_ptr,
                                chars_cap, stream=0):
    """sjgpu_serialize_cells_wide_device: the arguments and the answers of json_text.serialize_cells_device, and one code more: capi.SJGPU_E_RANGE, when the words of the
    located container roots laid end to end, plus one slot per other root, exceed 0xFFFFFFF0 (status complete, nothing else written).
    -> (code, bytes the texts take)"""
    total = ctypes.c_uint64(0)
    rc = p.L.sjgpu_serialize_cells_wide_device(p.h, tape_ptr, int(tape_words), strbuf_ptr, int(strbuf_bytes), docs_ptr, int(docs), root_value_ptr or None, root_tag_ptr or None,
                                               int(rows), offsets_ptr, status_ptr or None, chars_ptr or None, int(chars_cap), stream or None, ctypes.byref(total))
    return p._raise_infra(_NAME, rc), int(total.value)


def json_column_wide_many(p, data, path, wide=False, max_depth=1024):
    """json_text.json_column_many with the matches serialised by the wide call (wide: which PATHS call finds them, as there)
    -> (offsets uint32[rows + 1], chars uint8[bytes], status uint8[rows])"""
    return _json_column(p, data, path, wide, max_depth, serialize_cells_wide_device, _NAME)


def documents_as_json_wide_many(p, data, max_depth=1024):
    """json_text.documents_as_json_many through the wide call: one big document is as many lanes' work as its tape has words
    -> (offsets uint32[docs + 1], chars uint8[bytes], status uint8[docs])"""
    return _documents_as_json(p, data, max_depth, serialize_cells_wide_device, _NAME)
