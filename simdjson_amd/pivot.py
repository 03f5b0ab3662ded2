"""A map column pivoted into a record table (include/sjgpu_pivot.h): the fields of every row -- parent row, key code, value cell, as
sjgpu_object_fields_from_cells_device and sjgpu_dictionary_encode_device leave them on the device -- scattered into one column per key.  Free functions that take a
capi.DomParserImplementation as their first argument, as in simdjson_amd/dictionary.py: the thin mirror of the C entry point, and one call in the manner of the
parser's *_many methods -- the table of a set of records with a column per learned key (records_many)."""
import numpy as np

from . import capi
from .capi import ResidentStream, _refused, _to_capacity
from .dictionary import _dictionary_of

CHUNK = 64  # the K limit of sjgpu_cell_kinds_device and sjgpu_cast_cells_device


def pivot_fields_device(p, offsets_ptr, status_ptr, rows, codes_ptr, value_ptr, tag_ptr, fields, column_of_code_ptr, groups, columns, value_out_ptr, tag_out_ptr, stream=0):
    """sjgpu_pivot_fields_device: the fields offsets_ptr (rows + 1 uint32) / status_ptr (rows bytes) / value_ptr, tag_ptr (fields uint64 / bytes) with the codes of
    their keys codes_ptr (fields int32) -> cell (c, r) at c * rows + r of value_out_ptr (columns * rows uint64) and tag_out_ptr (as many bytes): the first field of row
    r whose column is c, or 20; column_of_code_ptr (groups int32) maps codes to columns, 0: column = code.  Only enqueues.
    -> 0 or a negative SJGPU_E_* for arguments the call refuses (raises on HIP errors)"""
    return p._raise_infra("sjgpu_pivot_fields_device",
                          p.L.sjgpu_pivot_fields_device(p.h, offsets_ptr or None, status_ptr or None, int(rows), codes_ptr or None, value_ptr or None, tag_ptr or None, int(fields),
                                                        column_of_code_ptr or None, int(groups), int(columns), value_out_ptr or None, tag_out_ptr or None, stream or None))


def fold_key(key):
    """The class of a key under the reference's key_equals_case_insensitive (include/simdjson/dom/object-inl.h:356-367): equal length, then strncasecmp over that
    length -- which folds ASCII letters only and stops at the first NUL.  Two keys are one key there exactly when their fold_key is equal."""
    key = bytes(key)
    nul = key.find(b"\0")
    return len(key), (key if nul < 0 else key[:nul]).lower()  # (bytes.lower() folds A-Z alone: a byte >= 0x80 stays)


def column_map(dictionary, counts, keys=None, min_count=1, fold_case=False):
    """The columns of a table over a dictionary of keys (list of bytes in order of first occurrence) -> (names, column_of_code int32[len(dictionary)], pick).
    keys None: a column for every key whose count is >= min_count, in order of first occurrence; else one for each listed key, in the order given (a key the
    dictionary does not hold gets a column no code maps to).  fold_case: the columns are the classes of fold_key -- a class is named by its spelling that occurs
    first and counts the fields of all its spellings.  pick: None, or for a list that names one column twice the index of the pivoted column behind each name."""
    same = fold_key if fold_case else bytes
    if keys is None:
        total, first = {}, {}
        for j, k in enumerate(dictionary):
            total[same(k)] = total.get(same(k), 0) + int(counts[j])
            first.setdefault(same(k), k)
        names = [first[c] for c in first if total[c] >= min_count]
        listed = names
    else:
        names = [bytes(k) for k in keys]
        listed = names
    column_of_class, pick = {}, []
    for k in listed:
        pick.append(column_of_class.setdefault(same(k), len(column_of_class)))
    column_of_code = np.array([column_of_class.get(same(k), -1) for k in dictionary], np.int32)
    return names, column_of_code, (None if len(column_of_class) == len(names) else pick)


def records_many(p, data, row_path, keys=None, min_count=1, fold_case=False, wide=False, max_depth=1024):
    """The table of a set of records, one column per key: schema_many's calls (the rows, sjgpu_object_fields_from_cells_device, sjgpu_dictionary_encode_device over the
    key row, the gather of the dictionary), the map from key codes to columns (column_map; folding the dictionary's strings is host work, the map is uploaded once),
    ONE sjgpu_pivot_fields_device call, then sjgpu_cell_kinds_device and sjgpu_cast_cells_device in chunks of 64 columns with capi.infer_getters choosing each
    getter, everything resident.  Column c answers element::at_key(names[c]) for every row -- with fold_case element::at_key_case_insensitive(names[c]).
    -> (error_code of the first broken document or 0, documents delivered, rows, names: list of bytes, tags uint8[C, rows], cells uint64[C, rows],
    kinds uint32[C, 16], getters: list of SJGPU_GET_* or 0, values uint64[C, rows]: the words sjgpu_cast_cells_device wrote (view them as the getter's type),
    valid uint64[C, ceil(rows / 64)]: its validity words, codes uint8[C, rows]: its codes, 0 = valid).  A column whose getter is 0 is left as cells: its rows of
    values, valid and codes are zeros."""
    import torch
    S = ResidentStream(p, data, max_depth)

    def empty(names, rows):
        C, W = len(names), (rows + 63) // 64
        return (S.code, S.docs, rows, names, np.full((C, rows), capi.NO_SUCH_FIELD, np.uint8), np.zeros((C, rows), np.uint64), np.zeros((C, 16), np.uint32), [0] * C,
                np.zeros((C, rows), np.uint64), np.zeros((C, W), np.uint64), np.zeros((C, rows), np.uint8))
    if S.docs == 0:
        return empty([] if keys is None else [bytes(k) for k in keys], 0)
    row_offsets, row_status, root_values, root_tags, rows = p._rows_of(S, row_path, wide)
    offsets = torch.empty(rows + 1, dtype=torch.int32, device=S.dev)
    status = torch.empty(max(rows, 1), dtype=torch.uint8, device=S.dev)
    roots = (root_values.data_ptr(), root_tags.data_ptr(), rows)
    rc, fields, (key_values, key_tags, values, tags) = _to_capacity(lambda cap: p._fields(S, roots, offsets, status, cap), int(S.tw // 8 + 1))
    _refused("sjgpu_object_fields_from_cells_device", rc)
    codes, distinct, dict_offsets, dict_chars, total, dict_counts = _dictionary_of(p, S, key_values, key_tags, fields)
    at, chars = dict_offsets.cpu().numpy().view(np.uint32).tolist(), dict_chars[:total].cpu().numpy().tobytes()
    dictionary = [chars[at[j]: at[j + 1]] for j in range(distinct)]
    names, column_of_code, pick = column_map(dictionary, dict_counts[:distinct].cpu().numpy().view(np.uint32), keys, min_count, fold_case)
    C = len(names)
    if C == 0 or rows == 0:
        S.synchronize()
        return empty(names, rows)
    pivoted = C if pick is None else max(pick) + 1
    cells = torch.empty((pivoted, rows), dtype=torch.int64, device=S.dev)
    cell_tags = torch.empty((pivoted, rows), dtype=torch.uint8, device=S.dev)
    d_map = torch.from_numpy(column_of_code).to(S.dev) if distinct else None
    _refused("sjgpu_pivot_fields_device", pivot_fields_device(p, offsets.data_ptr(), status.data_ptr(), rows, codes.data_ptr(), values.data_ptr(), tags.data_ptr(), fields,
                                                              d_map.data_ptr() if distinct else 0, distinct, pivoted, cells.data_ptr(), cell_tags.data_ptr(), S.stream))
    if pick is not None:  # a list that names one column twice: both names read the same pivoted column
        index = torch.tensor(pick, dtype=torch.int64, device=S.dev)
        cells, cell_tags = cells.index_select(0, index).contiguous(), cell_tags.index_select(0, index).contiguous()
    kinds = torch.empty((C, 16), dtype=torch.int32, device=S.dev)
    for c0 in range(0, C, CHUNK):
        K = min(CHUNK, C - c0)
        _refused("sjgpu_cell_kinds_device", p.cell_kinds_device(cells[c0].data_ptr(), cell_tags[c0].data_ptr(), rows, K, kinds[c0].data_ptr(), S.stream))
    S.synchronize()
    kinds_h = kinds.cpu().numpy().view(np.uint32)
    getters = capi.infer_getters(kinds_h)
    W = (rows + 63) // 64
    out_values = torch.zeros((C, rows), dtype=torch.int64, device=S.dev)
    out_codes = torch.zeros((C, rows), dtype=torch.uint8, device=S.dev)
    out_valid = torch.zeros((C, W), dtype=torch.int64, device=S.dev)
    cast = [c for c in range(C) if getters[c]]
    for j0 in range(0, len(cast), CHUNK):
        chunk = cast[j0: j0 + CHUNK]
        index = torch.tensor(chunk, dtype=torch.int64, device=S.dev)
        in_values, in_tags = cells.index_select(0, index).contiguous(), cell_tags.index_select(0, index).contiguous()  # the columns with a getter, back to back
        got_values = torch.empty((len(chunk), rows), dtype=torch.int64, device=S.dev)
        got_codes = torch.empty((len(chunk), rows), dtype=torch.uint8, device=S.dev)
        got_valid = torch.empty((len(chunk), W), dtype=torch.int64, device=S.dev)
        counts = torch.empty((len(chunk), 4), dtype=torch.int32, device=S.dev)
        _refused("sjgpu_cast_cells_device", p.cast_cells_device(in_values.data_ptr(), in_tags.data_ptr(), rows, [getters[c] for c in chunk], got_values.data_ptr(),
                                                                got_codes.data_ptr(), got_valid.data_ptr(), counts.data_ptr(), S.stream))
        out_values.index_copy_(0, index, got_values)
        out_codes.index_copy_(0, index, got_codes)
        out_valid.index_copy_(0, index, got_valid)
    S.synchronize()
    return (S.code, S.docs, rows, names, cell_tags.cpu().numpy(), cells.cpu().numpy().view(np.uint64), kinds_h, getters, out_values.cpu().numpy().view(np.uint64),
            out_valid.cpu().numpy().view(np.uint64), out_codes.cpu().numpy())
