"""Cells as JSON text (include/sjgpu_json.h): every cell of a row serialised on the device the way simdjson::minify(element) serialises an element, as one
offsets / chars pair (Arrow's utf8 layout).  Free functions that take a capi.DomParserImplementation as their first argument: a thin mirror of the C entry point,
and two calls in the manner of the parser's *_many methods -- one column kept as JSON (json_column_many), every document of a stream minified through its tape
(documents_as_json_many)."""
import ctypes

import numpy as np

from .capi import ResidentStream, _refused, _to_capacity


def serialize_cells_device(p, tape_ptr, tape_words, strbuf_ptr, strbuf_bytes, docs_ptr, docs, root_value_ptr, root_tag_ptr, rows, offsets_ptr, status_ptr, chars_ptr, chars_cap,
                           stream=0):
    """sjgpu_serialize_cells_device: the JSON text of the `rows` cells root_value_ptr / root_tag_ptr (a row of at_pointers_device's output, the matches of at_paths_device,
    a value row of object_fields_from_cells_device); offsets_ptr -> rows + 1 uint32, status_ptr -> rows bytes, chars_ptr -> chars_cap bytes.
    -> (code, bytes the texts take): 0, CAPACITY, SJGPU_E_OVERFLOW with the capacity needed, or a negative SJGPU_E_* (raises on HIP errors and on memory the context
    could not get)"""
    total = ctypes.c_uint64(0)
    rc = p.L.sjgpu_serialize_cells_device(p.h, tape_ptr, int(tape_words), strbuf_ptr, int(strbuf_bytes), docs_ptr, int(docs), root_value_ptr or None, root_tag_ptr or None,
                                          int(rows), offsets_ptr, status_ptr or None, chars_ptr or None, int(chars_cap), stream or None, ctypes.byref(total))
    return p._raise_infra("sjgpu_serialize_cells_device", rc), int(total.value)


def _serialize(p, S, roots, offsets, status, cap, entry=None):
    """one sjgpu_serialize_cells_device (entry: the binding of another call with its contract, simdjson_amd/json_text_wide.py) over the tapes of S, into characters it
    allocates for cap bytes: the `call` of _to_capacity -> (rc, bytes, chars)"""
    import torch
    chars = torch.empty(max(cap, 1), dtype=torch.uint8, device=S.dev)
    rc, total = (entry or serialize_cells_device)(p, *S.args(), *roots, offsets.data_ptr(), status.data_ptr(), chars.data_ptr(), cap, S.stream)
    return rc, total, chars


def json_column_many(p, data, path, wide=False, max_depth=1024):
    """One column kept as JSON text: the matches of `path` in every document, flattened, each as what simdjson::minify gives for it.  Upload, stage 1,
    sjgpu_stage2_many_device, ONE sjgpu_at_paths_device call with K = 1 (wide: sjgpu_at_paths_wide_device) and sjgpu_serialize_cells_device over its matches --
    repeated once with the capacity it reported; the first guess is the source's length, which a minified text of it rarely exceeds (a \\u0001 is six bytes either
    way, an é written as \\u00e9 shrinks; a number may grow: 1e2 becomes 100.0) --, with everything resident.  Text r is chars[offsets[r] .. offsets[r + 1]).
    -> (offsets uint32[rows + 1], chars uint8[bytes], status uint8[rows]); raises SjgpuError when no document was delivered"""
    return _json_column(p, data, path, wide, max_depth, None, "sjgpu_serialize_cells_device")


def _json_column(p, data, path, wide, max_depth, entry, name):
    """json_column_many with the serialising call given (entry: None for sjgpu_serialize_cells_device; name: what a refusal is reported as)"""
    from .capi import SjgpuError
    import torch
    S = ResidentStream(p, data, max_depth)
    if S.docs == 0:  # (a stream that breaks behind its first documents serves those, as the other *_many calls do)
        raise SjgpuError(f"json_column_many: the stream has no document to query (error {S.code})")
    row_offsets, row_status, root_values, root_tags, rows = p._rows_of(S, path, wide)
    offsets = torch.empty(rows + 1, dtype=torch.int32, device=S.dev)
    status = torch.empty(max(rows, 1), dtype=torch.uint8, device=S.dev)
    roots = (root_values.data_ptr(), root_tags.data_ptr(), rows)
    rc, total, chars = _to_capacity(lambda cap: _serialize(p, S, roots, offsets, status, cap, entry), int(S.length))
    _refused(name, rc)
    S.synchronize()
    return offsets.cpu().numpy().view(np.uint32), chars[:total].cpu().numpy(), status[:rows].cpu().numpy()


def documents_as_json_many(p, data, max_depth=1024):
    """Every document of a stream as its minified text, through its tape, one row per document: json_column_many with the documents' root cells --
    sjgpu_at_pointers_device with the empty pointer (a bare `$` is no path: at_path_with_wildcard answers it with INVALID_JSON_POINTER) -- in the place of a path's matches.
    -> (offsets uint32[docs + 1], chars uint8[bytes], status uint8[docs]); raises SjgpuError when no document was delivered"""
    return _documents_as_json(p, data, max_depth, None, "sjgpu_serialize_cells_device")


def _documents_as_json(p, data, max_depth, entry, name):
    """documents_as_json_many with the serialising call given, as _json_column"""
    from .capi import SjgpuError
    import torch
    S = ResidentStream(p, data, max_depth)
    if S.docs == 0:
        raise SjgpuError(f"documents_as_json_many: the stream has no document (error {S.code})")
    root_values = torch.empty(S.docs, dtype=torch.int64, device=S.dev)
    root_tags = torch.empty(S.docs, dtype=torch.uint8, device=S.dev)
    _refused("sjgpu_at_pointers_device", p.at_pointers_device(*S.args(), [b""], root_values.data_ptr(), root_tags.data_ptr(), S.stream))
    offsets = torch.empty(S.docs + 1, dtype=torch.int32, device=S.dev)
    status = torch.empty(S.docs, dtype=torch.uint8, device=S.dev)
    roots = (root_values.data_ptr(), root_tags.data_ptr(), S.docs)
    rc, total, chars = _to_capacity(lambda cap: _serialize(p, S, roots, offsets, status, cap, entry), int(S.length))
    _refused(name, rc)
    S.synchronize()
    return offsets.cpu().numpy().view(np.uint32), chars[:total].cpu().numpy(), status.cpu().numpy()
