"""Dictionaries over device cells (include/sjgpu_dict.h): a row of string cells as int32 codes plus a dictionary in order of first occurrence, and the census of a
value row per code.  Free functions that take a capi.DomParserImplementation as their first argument: two thin mirrors of the C entry points, and two calls in the
manner of the parser's *_many methods -- one column as a categorical (dictionary_many), the schema of a set of records (schema_many)."""
import ctypes

import numpy as np

from . import capi
from .capi import ResidentStream, _refused, _to_capacity


def dictionary_encode_device(p, strbuf_ptr, strbuf_bytes, value_row_ptr, tag_row_ptr, n, codes_ptr, dict_value_ptr, dict_tag_ptr, dict_first_ptr, dict_count_ptr, dict_cap,
                             stream=0):
    """sjgpu_dictionary_encode_device: one row of n cells -> codes_ptr (n int32) and the dictionary's four arrays (dict_cap uint64 / bytes / uint32 / uint32).
    -> (code, distinct strings): 0, SJGPU_E_OVERFLOW with the capacity needed, or a negative SJGPU_E_* (raises on HIP errors and on memory the context could not get)"""
    distinct = ctypes.c_uint64(0)
    rc = p.L.sjgpu_dictionary_encode_device(p.h, strbuf_ptr or None, int(strbuf_bytes), value_row_ptr or None, tag_row_ptr or None, int(n), codes_ptr or None,
                                            dict_value_ptr or None, dict_tag_ptr or None, dict_first_ptr or None, dict_count_ptr or None, int(dict_cap), stream or None,
                                            ctypes.byref(distinct))
    return p._raise_infra("sjgpu_dictionary_encode_device", rc), int(distinct.value)


def kinds_by_code_device(p, codes_ptr, value_ptr, tag_ptr, n, groups, kinds_ptr, stream=0):
    """sjgpu_cell_kinds_by_code_device: the census of the n cells value_ptr / tag_ptr per code; kinds_ptr -> groups * 16 uint32.  Only enqueues.
    -> 0 or a negative SJGPU_E_* for arguments the call refuses (raises on HIP errors)"""
    return p._raise_infra("sjgpu_cell_kinds_by_code_device",
                          p.L.sjgpu_cell_kinds_by_code_device(p.h, codes_ptr or None, value_ptr or None, tag_ptr or None, int(n), int(groups), kinds_ptr or None, stream or None))


FIRST_DICT_CAP = 1024  # the first guess of the *_many calls: a categorical column or a set of keys is small; a larger one costs the second call


def _encode(p, S, values, tags, n, codes, cap):
    """one sjgpu_dictionary_encode_device over a row of S's cells, into a dictionary it allocates for cap entries: the `call` of _to_capacity
    -> (rc, distinct, (dict_values, dict_tags, dict_first, dict_counts))"""
    import torch
    dict_values = torch.empty(max(cap, 1), dtype=torch.int64, device=S.dev)
    dict_tags = torch.empty(max(cap, 1), dtype=torch.uint8, device=S.dev)
    dict_first, dict_counts = (torch.empty(max(cap, 1), dtype=torch.int32, device=S.dev) for _ in range(2))
    rc, distinct = dictionary_encode_device(p, S.sbuf.data_ptr(), S.sb, values.data_ptr(), tags.data_ptr(), n, codes.data_ptr(), dict_values.data_ptr(), dict_tags.data_ptr(),
                                            dict_first.data_ptr(), dict_counts.data_ptr(), cap, S.stream)
    return rc, distinct, (dict_values, dict_tags, dict_first, dict_counts)


def _dictionary_of(p, S, values, tags, n):
    """the encode of one row, repeated once at the capacity it reported, and ONE gather over the dictionary row
    -> (codes int32[max(n, 1)], distinct, dict_offsets int32[distinct + 1], dict_chars uint8[>= bytes], bytes, dict_counts int32[>= distinct]), tensors of the device"""
    import torch
    codes = torch.empty(max(n, 1), dtype=torch.int32, device=S.dev)
    rc, distinct, (dict_values, dict_tags, _, dict_counts) = _to_capacity(lambda cap: _encode(p, S, values, tags, n, codes, cap), FIRST_DICT_CAP)
    _refused("sjgpu_dictionary_encode_device", rc)
    dict_offsets = torch.empty(distinct + 1, dtype=torch.int32, device=S.dev)
    gather = lambda cap: p._key_chars(S, dict_values, dict_tags, distinct, dict_offsets, cap)  # noqa: E731
    rc, total, dict_chars = _to_capacity(gather, 32 * distinct)
    _refused("sjgpu_gather_strings_device", rc)
    return codes, distinct, dict_offsets, dict_chars, total, dict_counts


def dictionary_many(p, data, path, wide=False, max_depth=1024):
    """One column as a categorical: the matches of `path` in every document, flattened, as codes into a dictionary of its distinct strings in order of first
    occurrence (a match that is no string: -1).  Upload, stage 1, sjgpu_stage2_many_device, ONE sjgpu_at_paths_device call with K = 1 (wide:
    sjgpu_at_paths_wide_device), sjgpu_dictionary_encode_device over its matches -- repeated once with the capacity it reported -- and ONE
    sjgpu_gather_strings_device over the dictionary row, with everything resident.  The rows of document d are row_offsets[d] .. row_offsets[d + 1]; string j
    of the dictionary is dict_chars[dict_offsets[j] .. dict_offsets[j + 1]) and counts[j] rows hold it.
    -> (error_code of the first broken document or 0, documents delivered, row_offsets uint32[docs + 1], codes int32[rows], dict_offsets uint32[distinct + 1],
    dict_chars uint8[...], counts uint32[distinct])"""
    S = ResidentStream(p, data, max_depth)
    if S.docs == 0:
        return S.code, 0, np.zeros(1, np.uint32), np.zeros(0, np.int32), np.zeros(1, np.uint32), np.zeros(0, np.uint8), np.zeros(0, np.uint32)
    row_offsets, row_status, values, tags, rows = p._rows_of(S, path, wide)
    codes, distinct, dict_offsets, dict_chars, total, dict_counts = _dictionary_of(p, S, values, tags, rows)
    S.synchronize()
    return (S.code, S.docs, row_offsets.cpu().numpy().view(np.uint32), codes[:rows].cpu().numpy(), dict_offsets.cpu().numpy().view(np.uint32), dict_chars[:total].cpu().numpy(),
            dict_counts[:distinct].cpu().numpy().view(np.uint32))


def schema_many(p, data, row_path, wide=False, max_depth=1024):
    """The schema of a set of records: the distinct keys of the objects `row_path` matches, in order of first appearance, how many fields carry each, and the
    census of the values under each key.  fields_many's calls (the rows, sjgpu_object_fields_from_cells_device), sjgpu_dictionary_encode_device over the key
    row, sjgpu_cell_kinds_by_code_device over the value row, and the gather of the dictionary, with everything resident.
    -> (error_code of the first broken document or 0, documents delivered, keys: list of bytes, counts uint32[keys], kinds uint32[keys, 16] as
    sjgpu_cell_kinds_device counts, getters: capi.infer_getters(kinds), the getter a loader would ask of the column under each key or 0)"""
    import torch
    S = ResidentStream(p, data, max_depth)
    if S.docs == 0:
        return S.code, 0, [], np.zeros(0, np.uint32), np.zeros((0, 16), np.uint32), []
    row_offsets, row_status, root_values, root_tags, rows = p._rows_of(S, row_path, wide)
    offsets = torch.empty(rows + 1, dtype=torch.int32, device=S.dev)
    status = torch.empty(max(rows, 1), dtype=torch.uint8, device=S.dev)
    roots = (root_values.data_ptr(), root_tags.data_ptr(), rows)
    rc, fields, (key_values, key_tags, values, tags) = _to_capacity(lambda cap: p._fields(S, roots, offsets, status, cap), int(S.tw // 8 + 1))
    _refused("sjgpu_object_fields_from_cells_device", rc)
    codes, distinct, dict_offsets, dict_chars, total, dict_counts = _dictionary_of(p, S, key_values, key_tags, fields)
    kinds = torch.empty((max(distinct, 1), 16), dtype=torch.int32, device=S.dev)
    _refused("sjgpu_cell_kinds_by_code_device", kinds_by_code_device(p, codes.data_ptr(), values.data_ptr(), tags.data_ptr(), fields, distinct, kinds.data_ptr(), S.stream))
    S.synchronize()
    at, chars = dict_offsets.cpu().numpy().view(np.uint32).tolist(), dict_chars[:total].cpu().numpy().tobytes()
    kinds = kinds[:distinct].cpu().numpy().view(np.uint32)
    return S.code, S.docs, [chars[at[j]: at[j + 1]] for j in range(distinct)], dict_counts[:distinct].cpu().numpy().view(np.uint32), kinds, capi.infer_getters(kinds)
