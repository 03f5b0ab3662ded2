"""Cells as indented JSON text (include/sjgpu_pretty.h): the calls of simdjson_amd/json_text.py and simdjson_amd/json_text_wide.py with the layout of
simdjson::prettify(element) -- four blanks per level, one child per line, a blank behind a key's colon, a newline at the end of every text --, by
sjgpu_prettify_cells_device (one lane per cell) or sjgpu_prettify_cells_wide_device (one lane per tape word).  Free functions that take a
capi.DomParserImplementation as their first argument, for the reason json_text's are; they return what their minify twins return, with the same capacity retry.
Which of the two roads to take is the caller's decision (one_lane_per_word)."""
import ctypes

from .json_text import _documents_as_json, _json_column

_NARROW, _WIDE = "sjgpu_prettify_cells_device", "sjgpu_prettify_cells_wide_device"


def prettify_cells_device(p, tape_ptr, tape_words, strbuf_ptr, strbuf_bytes, docs_ptr, docs, root_value_ptr, root_tag_ptr, rows, offsets_ptr, status_ptr, chars_ptr, chars_cap,
                          stream=0):
    """sjgpu_prettify_cells_device: the arguments and the answers of json_text.serialize_cells_device; the texts are simdjson::prettify's
    -> (code, bytes the texts take)"""
    total = ctypes.c_uint64(0)
    rc = p.L.sjgpu_prettify_cells_device(p.h, tape_ptr, int(tape_words), strbuf_ptr, int(strbuf_bytes), docs_ptr, int(docs), root_value_ptr or None, root_tag_ptr or None,
                                         int(rows), offsets_ptr, status_ptr or None, chars_ptr or None, int(chars_cap), stream or None, ctypes.byref(total))
    return p._raise_infra(_NARROW, rc), int(total.value)


def prettify_cells_wide_device(p, tape_ptr, tape_words, strbuf_ptr, strbuf_bytes, docs_ptr, docs, root_value_ptr, root_tag_ptr, rows, offsets_ptr, status_ptr, chars_ptr,
                               chars_cap, stream=0):
    """sjgpu_prettify_cells_wide_device: the arguments and the answers of json_text_wide.serialize_cells_wide_device, capi.SJGPU_E_RANGE included; the outputs are
    prettify_cells_device's bit for bit
    -> (code, bytes the texts take)"""
    total = ctypes.c_uint64(0)
    rc = p.L.sjgpu_prettify_cells_wide_device(p.h, tape_ptr, int(tape_words), strbuf_ptr, int(strbuf_bytes), docs_ptr, int(docs), root_value_ptr or None, root_tag_ptr or None,
                                              int(rows), offsets_ptr, status_ptr or None, chars_ptr or None, int(chars_cap), stream or None, ctypes.byref(total))
    return p._raise_infra(_WIDE, rc), int(total.value)


def pretty_column_many(p, data, path, wide=False, one_lane_per_word=False, max_depth=1024):
    """json_text.json_column_many with every match as what simdjson::prettify gives for it (wide: which PATHS call finds the matches, as there;
    one_lane_per_word: the wide serialising call).  The first guess of the capacity is the source's length; an indented text usually exceeds it, and the call is then
    repeated once with the capacity it reported.
    -> (offsets uint32[rows + 1], chars uint8[bytes], status uint8[rows])"""
    entry, name = (prettify_cells_wide_device, _WIDE) if one_lane_per_word else (prettify_cells_device, _NARROW)
    return _json_column(p, data, path, wide, max_depth, entry, name)


def documents_as_pretty_many(p, data, one_lane_per_word=False, max_depth=1024):
    """json_text.documents_as_json_many with every document as its indented text, one row per document
    -> (offsets uint32[docs + 1], chars uint8[bytes], status uint8[docs])"""
    entry, name = (prettify_cells_wide_device, _WIDE) if one_lane_per_word else (prettify_cells_device, _NARROW)
    return _documents_as_json(p, data, max_depth, entry, name)
