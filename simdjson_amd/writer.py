"""Typed columns as JSON records (include/sjgpu_write.h): row r of K device-resident columns written on the device as the object {"key0":v0,"key1":v1,...}, every
row's text into one offsets / chars pair -- what the reference's builder::string_builder writes, for columns that live in device memory.  Free functions that take a
capi.DomParserImplementation as their first argument: a thin mirror of the C entry point, a call over torch tensors, and one in the manner of the parser's *_many
methods -- NDJSON in, projected NDJSON out, nothing leaving the device in between (project_many).
List columns and array rows as nested JSON (include/sjgpu_nested.h) have the same three: write_nested_device, write_nested and project_rows_many."""
import ctypes

import numpy as np

from .capi import (COL_BOOL, COL_DOUBLE, COL_INT64, COL_JSON, COL_STRING, COL_STRING_CELLS, COL_UINT64, GET_ARRAY, GET_OBJECT, GET_STRING, WRITE_NEWLINE,  # noqa: F401
                   WRITE_ARRAY_ROWS, WRITE_BARE, WRITE_OMIT_NULLS, ResidentStream, WriteColumn, WriteField, _refused, _to_capacity)


def _fill_column(col, c, keep):
    key = bytes(c.get("key") or b"")
    buf = ctypes.create_string_buffer(key, len(key)) if key else None
    keep.append(buf)
    col.key = ctypes.cast(buf, ctypes.c_void_p) if key else None
    col.key_len = len(key)
    col.kind = int(c["kind"])
    col.values_dev = c.get("values") or None
    col.valid_dev = c.get("valid") or None
    col.offsets_dev = c.get("offsets") or None
    col.chars_dev = c.get("chars") or None
    col.chars_bytes = int(c.get("chars_bytes", 0))


def _table(columns):
    """columns: a list of dicts -- "key" (bytes, unescaped), "kind" (SJGPU_COL_*) and, as device addresses (0 or absent: null), "values", "valid", "offsets", "chars"
    with "chars_bytes" -> (the sjgpu_write_column array or None, what keeps the keys alive for the call)"""
    K = len(columns)
    if K == 0:
        return None, []
    table, keep = (WriteColumn * K)(), []
    for k, c in enumerate(columns):
        _fill_column(table[k], c, keep)
    return table, keep


def _field_table(fields):
    """fields: dicts as for _table with, for a LIST field, "list_offsets", "list_valid" (addresses) and "elements"; "key" may be absent where keys are not written
    -> (the sjgpu_write_field array or None, what keeps the keys alive for the call)"""
    K = len(fields)
    if K == 0:
        return None, []
    table, keep = (WriteField * K)(), []
    for k, f in enumerate(fields):
        _fill_column(table[k].col, f, keep)
        table[k].list_offsets_dev = f.get("list_offsets") or None
        table[k].list_valid_dev = f.get("list_valid") or None
        table[k].elements = int(f.get("elements", 0))
    return table, keep


def write_records_device(p, columns, n, flags, offsets_ptr, status_ptr, chars_ptr, chars_cap, counts_ptr, stream=0):
    """sjgpu_write_records_device: the JSON object of each of the n rows of `columns` (dicts of device addresses, see _table); offsets_ptr -> n + 1 uint32,
    status_ptr -> n bytes, chars_ptr -> chars_cap bytes, counts_ptr -> 4 uint64.
    -> (code, bytes the texts take): 0, CAPACITY, SJGPU_E_OVERFLOW with the capacity needed, or a negative SJGPU_E_* (raises on HIP errors and on memory the context
    could not get)"""
    table, keep = _table(columns)
    total = ctypes.c_uint64(0)
    rc = p.L.sjgpu_write_records_device(p.h, table, len(columns), int(n), int(flags), offsets_ptr or None, status_ptr or None, chars_ptr or None, int(chars_cap),
                                        counts_ptr or None, stream or None, ctypes.byref(total))
    del keep
    return p._raise_infra("sjgpu_write_records_device", rc), int(total.value)


def _addresses(columns):
    """columns of tensors -> columns of addresses (for write_records_device); a column's tensors stay the caller's to keep"""
    out = []
    for c in columns:
        d = {"key": c["key"], "kind": c["kind"]}
        for name in ("values", "valid", "offsets", "chars"):
            t = c.get(name)
            if t is not None:
                d[name] = t.data_ptr()
        if c.get("chars") is not None:
            d["chars_bytes"] = int(c.get("chars_bytes", c["chars"].numel()))
        out.append(d)
    return out


def write_records(p, columns, n, omit_nulls=False, newline=True, stream=0):
    """The rows of a table of torch tensors as JSON records.  columns: a list of dicts -- "key" (bytes), "kind" (SJGPU_COL_*), and the tensors the kind reads:
    "values" (8-byte elements, n of them: INT64, UINT64, DOUBLE, BOOL, STRING_CELLS), "offsets" (int32, n + 1) with "chars" (uint8) for STRING and JSON, "chars" for
    STRING_CELLS ("chars_bytes": how many of its bytes count, by default all), "valid" (8-byte elements, ceil(n / 64): Arrow validity) or none.
    One sjgpu_write_records_device call, repeated once at the capacity it reported (the first guess: 32 bytes per cell).  stream: a raw stream, by default torch's
    current one on the parser's device.
    -> (offsets int32[n + 1], chars uint8[bytes], status uint8[n], counts int64[4]), tensors of the device; raises SjgpuError on a refusal"""
    import torch
    dev = torch.device("cuda", p.device)
    stream = stream or torch.cuda.current_stream(dev).cuda_stream
    flags = (WRITE_OMIT_NULLS if omit_nulls else 0) | (WRITE_NEWLINE if newline else 0)
    offsets = torch.empty(n + 1, dtype=torch.int32, device=dev)
    status = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
    counts = torch.empty(4, dtype=torch.int64, device=dev)
    table = _addresses(columns)

    def call(cap):
        chars = torch.empty(max(cap, 1), dtype=torch.uint8, device=dev)
        rc, total = write_records_device(p, table, n, flags, offsets.data_ptr(), status.data_ptr(), chars.data_ptr(), cap, counts.data_ptr(), stream)
        return rc, total, chars
    rc, total, chars = _to_capacity(call, 32 * max(len(columns), 1) * n)
    _refused("sjgpu_write_records_device", rc)
    return offsets, chars[:total], status[:n], counts


def project_many(p, data, fields, omit_nulls=False, max_depth=1024):
    """NDJSON in, projected NDJSON out.  fields: [(json_pointer bytes, SJGPU_GET_*, out_key bytes), ...]; every document of the stream becomes one line
    {"out_key0":v0,...}, v the value at the pointer read through its getter: a number or a boolean as sjgpu_cast_cells_device delivers it, a string written from the
    string buffer as it lies there (SJGPU_COL_STRING_CELLS: no gather), an array or an object as sjgpu_serialize_cells_device writes it (SJGPU_COL_JSON).  A field that is
    missing, null or of another type is null, or left out under omit_nulls.  Upload, stage 1, sjgpu_stage2_many_device, ONE sjgpu_at_pointers_device, ONE
    sjgpu_cast_cells_device, a sjgpu_serialize_cells_device per ARRAY / OBJECT field and sjgpu_write_records_device, with everything resident.
    -> (offsets uint32[docs + 1], chars uint8[bytes], status uint8[docs], counts uint64[4]) on the host; raises SjgpuError when no document was delivered"""
    from .capi import SjgpuError
    from .json_text import _serialize
    import torch
    S = ResidentStream(p, data, max_depth)
    if S.docs == 0:
        raise SjgpuError(f"project_many: the stream has no document to project (error {S.code})")
    K, n = len(fields), S.docs
    columns, keep = [], []
    if K:
        W = (n + 63) // 64
        values = torch.empty((K, n), dtype=torch.int64, device=S.dev)
        tags = torch.empty((K, n), dtype=torch.uint8, device=S.dev)
        _refused("sjgpu_at_pointers_device", p.at_pointers_device(*S.args(), [bytes(f[0]) for f in fields], values.data_ptr(), tags.data_ptr(), S.stream))
        cast = torch.empty((K, n), dtype=torch.int64, device=S.dev)
        codes = torch.empty((K, n), dtype=torch.uint8, device=S.dev)
        valid = torch.empty((K, W), dtype=torch.int64, device=S.dev)
        cast_counts = torch.empty((K, 4), dtype=torch.int32, device=S.dev)
        _refused("sjgpu_cast_cells_device", p.cast_cells_device(values.data_ptr(), tags.data_ptr(), n, [int(f[1]) for f in fields], cast.data_ptr(), codes.data_ptr(),
                                                                 valid.data_ptr(), cast_counts.data_ptr(), S.stream))
        keep += [values, tags, cast, codes, valid, cast_counts]
        for k, (_, getter, key) in enumerate(fields):
            if getter in (GET_ARRAY, GET_OBJECT):
                # the cells that passed the cast as they came, every other one as a code: the serializer leaves length 0 for it, which the writer takes for null
                masked = torch.where(codes[k] == 0, tags[k], torch.full_like(tags[k], 17))
                offsets = torch.empty(n + 1, dtype=torch.int32, device=S.dev)
                status = torch.empty(n, dtype=torch.uint8, device=S.dev)
                roots = (values[k].data_ptr(), masked.data_ptr(), n)
                rc, total, chars = _to_capacity(lambda cap: _serialize(p, S, roots, offsets, status, cap), int(S.length))
                _refused("sjgpu_serialize_cells_device", rc)
                keep += [masked, offsets, status, chars]
                columns.append({"key": key, "kind": COL_JSON, "offsets": offsets, "chars": chars, "chars_bytes": total})
            elif getter == GET_STRING:
                columns.append({"key": key, "kind": COL_STRING_CELLS, "values": cast[k], "valid": valid[k], "chars": S.sbuf, "chars_bytes": S.sb})
            else:
                columns.append({"key": key, "kind": int(getter), "values": cast[k], "valid": valid[k]})
    offsets, chars, status, counts = write_records(p, columns, n, omit_nulls=omit_nulls, newline=True, stream=S.stream)
    S.synchronize()
    del keep
    return offsets.cpu().numpy().view(np.uint32), chars.cpu().numpy(), status.cpu().numpy(), counts.cpu().numpy().view(np.uint64)


# ---- list columns and array rows as nested JSON (include/sjgpu_nested.h) ---------------------------------------------------------------------------------------
def write_nested_device(p, fields, n, flags, offsets_ptr, status_ptr, chars_ptr, chars_cap, counts_ptr, stream=0):
    """sjgpu_write_nested_device: the JSON value of each of the n rows of `fields` (dicts of device addresses, see _field_table) -- an object, under WRITE_ARRAY_ROWS
    an array, under WRITE_BARE the one field's value alone; offsets_ptr -> n + 1 uint32, status_ptr -> n bytes, chars_ptr -> chars_cap bytes, counts_ptr -> 6 uint64.
    -> (code, bytes the texts take): 0, CAPACITY, SJGPU_E_OVERFLOW with the capacity needed, or a negative SJGPU_E_* (raises on HIP errors and on memory the context
    could not get)"""
    table, keep = _field_table(fields)
    total = ctypes.c_uint64(0)
    rc = p.L.sjgpu_write_nested_device(p.h, table, len(fields), int(n), int(flags), offsets_ptr or None, status_ptr or None, chars_ptr or None, int(chars_cap),
                                       counts_ptr or None, stream or None, ctypes.byref(total))
    del keep
    return p._raise_infra("sjgpu_write_nested_device", rc), int(total.value)


def _field_addresses(fields):
    out = _addresses(fields)
    for d, f in zip(out, fields):
        if f.get("list_offsets") is not None:
            d["list_offsets"] = f["list_offsets"].data_ptr()
            d["elements"] = int(f["elements"])
            if f.get("list_valid") is not None:
                d["list_valid"] = f["list_valid"].data_ptr()
    return out


def write_nested(p, fields, n, omit_nulls=False, newline=True, array_rows=False, bare=False, stream=0, first_cap=None):
    """The rows of a table of torch tensors as nested JSON.  fields: dicts as for write_records -- "key" is not needed under array_rows and bare --; a LIST field has
    "list_offsets" (int32, n + 1: Arrow list offsets into the element tensors, a slice of a longer row of offsets will do), "elements" (how many entries the element
    tensors "values" / "valid" / "offsets" / "chars" have) and "list_valid" (8-byte elements, ceil(n / 64)) or none.
    One sjgpu_write_nested_device call, repeated once at the capacity it reported (first_cap: the first guess, by default 32 bytes per cell and 16 per element).
    -> (offsets int32[n + 1], chars uint8[bytes], status uint8[n], counts int64[6]), tensors of the device; raises SjgpuError on a refusal"""
    import torch
    dev = torch.device("cuda", p.device)
    stream = stream or torch.cuda.current_stream(dev).cuda_stream
    flags = (WRITE_OMIT_NULLS if omit_nulls else 0) | (WRITE_NEWLINE if newline else 0) | (WRITE_ARRAY_ROWS if array_rows else 0) | (WRITE_BARE if bare else 0)
    offsets = torch.empty(n + 1, dtype=torch.int32, device=dev)
    status = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
    counts = torch.empty(6, dtype=torch.int64, device=dev)
    table = _field_addresses(fields)

    def call(cap):
        chars = torch.empty(max(cap, 1), dtype=torch.uint8, device=dev)
        rc, total = write_nested_device(p, table, n, flags, offsets.data_ptr(), status.data_ptr(), chars.data_ptr(), cap, counts.data_ptr(), stream)
        return rc, total, chars
    guess = 32 * max(len(fields), 1) * n + 16 * sum(int(f.get("elements", 0)) for f in fields if f.get("list_offsets") is not None)
    rc, total, chars = _to_capacity(call, guess if first_cap is None else int(first_cap))
    _refused("sjgpu_write_nested_device", rc)
    return offsets, chars[:total], status[:n], counts


def _cells_as_column(p, S, values, tags, n, getter, keep):
    """n cells (tensors of the device) read through `getter` -> the tensors of a column or of a list's elements: a number or a boolean as sjgpu_cast_cells_device
    delivers it, a string from the string buffer as it lies there (SJGPU_COL_STRING_CELLS), an array or an object as sjgpu_serialize_cells_device writes it"""
    from .json_text import _serialize
    import torch
    if n == 0:
        return {"kind": COL_JSON if getter in (GET_ARRAY, GET_OBJECT) else COL_STRING_CELLS if getter == GET_STRING else int(getter)}
    cast = torch.empty(n, dtype=torch.int64, device=S.dev)
    codes = torch.empty(n, dtype=torch.uint8, device=S.dev)
    valid = torch.empty((n + 63) // 64, dtype=torch.int64, device=S.dev)
    cast_counts = torch.empty(4, dtype=torch.int32, device=S.dev)
    _refused("sjgpu_cast_cells_device", p.cast_cells_device(values.data_ptr(), tags.data_ptr(), n, [int(getter)], cast.data_ptr(), codes.data_ptr(), valid.data_ptr(),
                                                             cast_counts.data_ptr(), S.stream))
    keep += [cast, codes, valid, cast_counts]
    if getter in (GET_ARRAY, GET_OBJECT):
        # the cells that passed the cast as they came, every other one as a code: the serializer leaves length 0 for it, which the writer takes for null
        masked = torch.where(codes == 0, tags[:n], torch.full_like(tags[:n], 17))
        offsets = torch.empty(n + 1, dtype=torch.int32, device=S.dev)
        status = torch.empty(n, dtype=torch.uint8, device=S.dev)
        roots = (values.data_ptr(), masked.data_ptr(), n)
        rc, total, chars = _to_capacity(lambda cap: _serialize(p, S, roots, offsets, status, cap), int(S.length))
        _refused("sjgpu_serialize_cells_device", rc)
        keep += [masked, offsets, status, chars]
        return {"kind": COL_JSON, "offsets": offsets, "chars": chars, "chars_bytes": total}
    if getter == GET_STRING:
        return {"kind": COL_STRING_CELLS, "values": cast, "valid": valid, "chars": S.sbuf, "chars_bytes": S.sb}
    return {"kind": int(getter), "values": cast, "valid": valid}


def _row_fields(p, S, row_path, fields):
    """the field table of project_rows_many over the resident stream S, everything enqueued on S.stream -> (fields of tensors for write_nested, rows, what must live
    until the write has run)"""
    import torch
    fields = [(bytes(f[0]), int(f[1]), bytes(f[2])) for f in fields]
    for spec, _, _ in fields:
        if spec.startswith(b"$") and b"*" not in spec:
            raise ValueError(f"project_rows_many: {spec!r} is a path without a wildcard; write it as a JSON pointer")
    listed = [k for k, f in enumerate(fields) if f[0].startswith(b"$")]
    plain = [k for k in range(len(fields)) if k not in listed]
    row_offsets, row_status, root_values, root_tags, rows = p._rows_of(S, row_path, False)
    keep, table = [row_offsets, row_status, root_values, root_tags], [None] * len(fields)
    roots = (root_values.data_ptr(), root_tags.data_ptr(), rows)
    if listed and rows:
        L = len(listed)
        offsets = torch.empty(L * rows + 1, dtype=torch.int32, device=S.dev)
        status = torch.empty((L, rows), dtype=torch.uint8, device=S.dev)
        name = "sjgpu_at_paths_from_cells_device"
        rc, matches, (values, tags) = _to_capacity(lambda cap: p._matches(name, S, [fields[k][0] for k in listed], offsets, status, cap, roots), int(S.tw // 8 + 1))
        _refused(name, rc)
        keep += [offsets, status, values, tags]
        by_getter = {}
        for j, k in enumerate(listed):  # the elements of every list field are ALL the matches, cast once per getter; a field's lists are its slice of the offsets
            getter = fields[k][1]
            if getter not in by_getter:
                by_getter[getter] = _cells_as_column(p, S, values, tags, matches, getter, keep)
            table[k] = dict(by_getter[getter], key=fields[k][2], list_offsets=offsets[j * rows: (j + 1) * rows + 1], elements=matches)
    if plain and rows:
        P = len(plain)
        values = torch.empty((P, rows), dtype=torch.int64, device=S.dev)
        tags = torch.empty((P, rows), dtype=torch.uint8, device=S.dev)
        _refused("sjgpu_at_pointers_from_cells_device", p.at_pointers_from_cells_device(*S.args(), *roots, [fields[k][0] for k in plain], values.data_ptr(), tags.data_ptr(),
                                                                                         S.stream))
        keep += [values, tags]
        for j, k in enumerate(plain):
            table[k] = dict(_cells_as_column(p, S, values[j], tags[j], rows, fields[k][1], keep), key=fields[k][2])
    return (table if rows else []), rows, keep


def project_rows_many(p, data, row_path, fields, omit_nulls=False, max_depth=1024):
    """NDJSON (or one document) in, one NDJSON line per match of row_path out.  fields: [(json_pointer or path, SJGPU_GET_*, out_key bytes), ...], each rooted at
    the row.  A path -- it begins with $ and has a wildcard -- becomes a LIST field: its matches under the row, in order, each read through the getter, one that is
    of another type as null in its place; any other entry is a JSON pointer and a plain field as in project_many.  Upload, stage 1, sjgpu_stage2_many_device, the
    rows (ONE sjgpu_at_paths_device), ONE sjgpu_at_paths_from_cells_device for all list fields and ONE sjgpu_at_pointers_from_cells_device for all plain ones, a
    sjgpu_cast_cells_device (and, for arrays and objects, a sjgpu_serialize_cells_device) per field, sjgpu_write_nested_device: nothing leaves the device in between.
    -> (offsets uint32[rows + 1], chars uint8[bytes], status uint8[rows], counts uint64[6]) on the host; raises SjgpuError when no document was delivered"""
    from .capi import SjgpuError
    S = ResidentStream(p, data, max_depth)
    if S.docs == 0:
        raise SjgpuError(f"project_rows_many: the stream has no document to project (error {S.code})")
    table, rows, keep = _row_fields(p, S, row_path, fields)
    offsets, chars, status, counts = write_nested(p, table, rows, omit_nulls=omit_nulls, newline=True, stream=S.stream)
    S.synchronize()
    del keep
    return offsets.cpu().numpy().view(np.uint32), chars.cpu().numpy(), status.cpu().numpy(), counts.cpu().numpy().view(np.uint64)
