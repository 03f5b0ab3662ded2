"""ctypes mirror of include/sjgpu.h (the C-ABI of libsjgpu.so, HIP kernels for gfx950).

Host-side names follow the reference's plug-in interface for this path
(/root/reference/include/simdjson/implementation.h:97-128,
 /root/reference/include/simdjson/internal/dom_parser_implementation.h:80): `stage1`, `minify`,
`validate_utf8`, `set_capacity`, error codes as simdjson::error_code integers.

There is no CPU fallback: a missing library or a missing GPU raises.
"""
import ctypes
import os

import numpy as np

from . import _paths

# simdjson::error_code values on this path (include/simdjson/error.h:19-53)
SUCCESS, CAPACITY, MEMALLOC, UTF8_ERROR, EMPTY, UNESCAPED_CHARS, UNCLOSED_STRING, UNEXPECTED_ERROR = 0, 1, 2, 11, 13, 14, 15, 24
# simdjson::stage1_mode (internal/dom_parser_implementation.h:22-27)
REGULAR, STREAMING_PARTIAL, STREAMING_FINAL, JSON_SEQUENCE_PARTIAL, JSON_SEQUENCE_FINAL, COMMA_DELIMITED_PARTIAL, COMMA_DELIMITED_FINAL = range(7)
F_UNCLOSED_STRING, F_UNESCAPED_CTRL, F_UTF8_ERROR, F_IDX_OVERFLOW, F_INTERNAL, F_RANGE_CARRY = 1, 2, 4, 8, 16, 32

EXPORTS = [
    "sjgpu_device_count", "sjgpu_ctx_create", "sjgpu_ctx_destroy", "sjgpu_set_capacity", "sjgpu_capacity",
    "sjgpu_last_error", "sjgpu_stage1", "sjgpu_minify", "sjgpu_validate_utf8", "sjgpu_validate_utf8_pieces", "sjgpu_stage1_device",
    "sjgpu_minify_device", "sjgpu_validate_utf8_device", "sjgpu_result", "sjgpu_stage1_error_from_flags", "sjgpu_stage1_tokens_device", "sjgpu_depth_scan_tokens_device",
    "sjgpu_stage1_finish_host", "sjgpu_trim_partial_utf8", "sjgpu_profile_enable", "sjgpu_profile_read", "sjgpu_set_pipeline", "sjgpu_debug_trace_stage1",
    "sjgpu_clean_cut", "sjgpu_string_parity_device", "sjgpu_stage1_shard_device", "sjgpu_minify_shard_device",
    "sjgpu_stage1_range_device", "sjgpu_minify_range_device",
    "sjgpu_host_alloc", "sjgpu_host_free", "sjgpu_host_register", "sjgpu_host_unregister", "sjgpu_last_pipeline",
    "sjgpu_profile_kernel", "sjgpu_debug_trace_pipelined", "sjgpu_debug_string_path", "sjgpu_stage1_many", "sjgpu_stage1_finish_device",
    "sjgpu_depth_scan_device", "sjgpu_parse_strings_device", "sjgpu_stage2_device", "sjgpu_stage2_tokens_device", "sjgpu_parse", "sjgpu_pool_trim", "sjgpu_stream_register", "sjgpu_stream_unregister", "sjgpu_stream_unregister_len", "sjgpu_debug_stream_extent", "sjgpu_match_keys_device", "sjgpu_comm_unique_id", "sjgpu_comm_create", "sjgpu_comm_destroy", "sjgpu_comm_last_error", "sjgpu_comm_ranks", "sjgpu_comm_gather_indices", "sjgpu_mgpu_create", "sjgpu_mgpu_destroy", "sjgpu_mgpu_count", "sjgpu_mgpu_stage1", "sjgpu_mgpu_minify",
    "sjgpu_mgpu_validate_utf8",
]


class SjgpuError(RuntimeError):
    pass


class Doc(ctypes.Structure):
    """sjgpu_doc (include/sjgpu.h): one document of a sjgpu_stage1_many batch."""
    _fields_ = [("buf", ctypes.c_void_p), ("len", ctypes.c_size_t), ("idx_out", ctypes.c_void_p), ("idx_words", ctypes.c_size_t),
                ("n", ctypes.c_uint32), ("error", ctypes.c_int)]


# what include/sjgpu_debug.h declares (diagnostics of the single-pass workspace: an extension of the C-ABI with a header of its own)
DEBUG_EXPORTS = ["sjgpu_debug_read_workspace", "sjgpu_debug_gave_up_count"]


# what include/sjgpu_stream.h declares (document streams: an extension of the C-ABI with a header of its own)
STREAM_EXPORTS = ["sjgpu_stage2_many_device", "sjgpu_parse_many"]
# sjgpu_doc_span (include/sjgpu_stream.h): one entry of the document table of sjgpu_stage2_many_device / sjgpu_parse_many
DOC_SPAN = np.dtype([("first_token", np.uint32), ("byte_begin", np.uint32), ("tape_begin", np.uint32), ("string_begin", np.uint32)])


# what include/sjgpu_query.h declares (queries over device tapes: JSON pointers -> typed columns, a string column -> offsets + characters)
QUERY_EXPORTS = ["sjgpu_at_pointers_device", "sjgpu_gather_strings_device"]
# simdjson::error_code values a cell of sjgpu_at_pointers_device can hold instead of a tape tag (include/simdjson/error.h)
INCORRECT_TYPE, INDEX_OUT_OF_BOUNDS, NO_SUCH_FIELD, INVALID_JSON_POINTER = 17, 19, 20, 22


# what include/sjgpu_paths.h declares (JSONPath with wildcards over device tapes: one ragged column, CSR style)
PATH_EXPORTS = ["sjgpu_at_paths_device", "sjgpu_at_paths_wide_device"]


# what include/sjgpu_rows.h declares (record tables over device tapes: JSON pointers rooted at the cells of a column)
ROWS_EXPORTS = ["sjgpu_at_pointers_from_cells_device"]


# what include/sjgpu_lists.h declares (list columns over device tapes: JSONPaths with wildcards rooted at the cells of a column)
LISTS_EXPORTS = ["sjgpu_at_paths_from_cells_device"]


# what include/sjgpu_cast.h declares (typed getters over a column: get<T> per cell with validity bits, and the census of a column's tags)
CAST_EXPORTS = ["sjgpu_cell_kinds_device", "sjgpu_cast_cells_device"]
# SJGPU_GET_*: the getter a row of sjgpu_cast_cells_device asks of its cells
GET_INT64, GET_UINT64, GET_DOUBLE, GET_BOOL, GET_STRING, GET_ARRAY, GET_OBJECT = 1, 2, 3, 4, 5, 6, 7
NUMBER_OUT_OF_RANGE = 18  # what get_int64 answers a u cell, get_uint64 a negative l
SJGPU_E_OVERFLOW = -5  # (include/sjgpu.h) an output was too small; the calls with a capacity report the one they need beside it


# what include/sjgpu_cast_strings.h declares (numbers held in strings: get_int64_in_string, get_uint64_in_string, get_double_in_string per cell)
CAST_STRINGS_EXPORTS = ["sjgpu_cast_string_cells_device"]
# SJGPU_GETS_*: the getter a row of sjgpu_cast_string_cells_device asks of its string cells; GETS_OR_NUMBER is a flag or-ed into it (number cells are cast as well)
GETS_INT64, GETS_UINT64, GETS_DOUBLE, GETS_OR_NUMBER = 1, 2, 3, 0x10
NUMBER_ERROR = 9  # what a string that is no number of the getter's kind answers where it is not INCORRECT_TYPE


# what include/sjgpu_fields.h declares (map columns over device tapes: the fields of each cell's object, keys as string cells, and the size() of each cell's container)
FIELDS_EXPORTS = ["sjgpu_object_fields_from_cells_device", "sjgpu_cell_sizes_device"]


# what include/sjgpu_dict.h declares (dictionaries over device cells: a row of string cells as codes + a dictionary in order of first occurrence, and the census of a
# value row per code); the bindings are the free functions of simdjson_amd/dictionary.py
DICT_EXPORTS = ["sjgpu_dictionary_encode_device", "sjgpu_cell_kinds_by_code_device"]
SJGPU_E_INTERNAL = -7  # (include/sjgpu_dict.h) a bounded loop of the library ran out: a bug of the library


# what include/sjgpu_pivot.h declares (a map column pivoted into a record table: one column per key code, the first field of a row that maps to a column wins); the
# bindings are the free functions of simdjson_amd/pivot.py
PIVOT_EXPORTS = ["sjgpu_pivot_fields_device"]


# what include/sjgpu_json.h declares (cells as JSON text: minify(element) per cell into offsets + chars); the bindings are the free functions of
# simdjson_amd/json_text.py
JSON_EXPORTS = ["sjgpu_serialize_cells_device"]
# what include/sjgpu_json_wide.h declares (the same texts, one lane per tape word); the bindings are the free functions of simdjson_amd/json_text_wide.py
JSON_WIDE_EXPORTS = ["sjgpu_serialize_cells_wide_device"]
SJGPU_E_RANGE = -8  # (include/sjgpu_json_wide.h) the range space of the call exceeds 0xFFFFFFF0 slots
# what include/sjgpu_pretty.h declares (prettify(element) per cell, by either road); the bindings are the free functions of simdjson_amd/pretty_text.py
PRETTY_EXPORTS = ["sjgpu_prettify_cells_device", "sjgpu_prettify_cells_wide_device"]


# what include/sjgpu_write.h declares (typed columns as JSON records: one object per row into offsets + chars); the bindings are the free functions of
# simdjson_amd/writer.py
WRITE_EXPORTS = ["sjgpu_write_records_device"]
# SJGPU_COL_*: what a column of sjgpu_write_records_device holds (1 .. 4 are SJGPU_GET_INT64 .. SJGPU_GET_BOOL)
COL_INT64, COL_UINT64, COL_DOUBLE, COL_BOOL, COL_STRING, COL_JSON, COL_STRING_CELLS = 1, 2, 3, 4, 5, 8, 9
WRITE_OMIT_NULLS, WRITE_NEWLINE = 1, 2
INDEX_OUT_OF_BOUNDS = 19  # the status of a row with a string or JSON cell outside its column's characters


class WriteColumn(ctypes.Structure):
    """sjgpu_write_column"""
    _fields_ = [("key", ctypes.c_void_p), ("key_len", ctypes.c_uint32), ("kind", ctypes.c_uint32), ("values_dev", ctypes.c_void_p), ("valid_dev", ctypes.c_void_p),
                ("offsets_dev", ctypes.c_void_p), ("chars_dev", ctypes.c_void_p), ("chars_bytes", ctypes.c_uint64)]


# what include/sjgpu_nested.h declares (list columns and array rows as nested JSON: the writer above with list fields, array rows and bare values); the bindings are
# free functions of simdjson_amd/writer.py too
NESTED_EXPORTS = ["sjgpu_write_nested_device"]
WRITE_ARRAY_ROWS, WRITE_BARE = 4, 8


class WriteField(ctypes.Structure):
    """sjgpu_write_field"""
    _fields_ = [("col", WriteColumn), ("list_offsets_dev", ctypes.c_void_p), ("list_valid_dev", ctypes.c_void_p), ("elements", ctypes.c_uint64)]


def infer_getters(kinds):
    """The getter a loader would ask of each row, from its census (kinds: K x 16 counts as sjgpu_cell_kinds_device leaves them) -> list of K SJGPU_GET_* or 0.
    The ELEMENTS of a row are its cells except the nulls and the codes 17 / 19 / 20 / 22 (they become invalid bits under any getter):
    all t / f: BOOL; all strings: STRING; all arrays: ARRAY; all objects: OBJECT; numbers only: DOUBLE when there is a d, else INT64 without a u, else UINT64
    without a negative l, else -- a u beside a negative l, no 64-bit integer holds both -- DOUBLE, which is LOSSY above 2^53 as get_double is.
    No elements, a mix of kinds or a byte that is no tag: 0, "leave the row as cells"."""
    picked = []
    for row in np.asarray(kinds).reshape(-1, 16).tolist():
        n_obj, n_arr, n_str, n_l, n_u, n_d, n_t, n_f, _, n_neg = row[:10]
        elements = n_obj + n_arr + n_str + n_l + n_u + n_d + n_t + n_f + row[14]
        if elements == 0:
            picked.append(0)
        elif n_t + n_f == elements:
            picked.append(GET_BOOL)
        elif n_str == elements:
            picked.append(GET_STRING)
        elif n_arr == elements:
            picked.append(GET_ARRAY)
        elif n_obj == elements:
            picked.append(GET_OBJECT)
        elif n_l + n_u + n_d == elements:
            picked.append(GET_DOUBLE if n_d or (n_u and n_neg) else GET_UINT64 if n_u else GET_INT64)
        else:
            picked.append(0)
    return picked


class ScanResult(ctypes.Structure):
    _fields_ = [("n", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("out_len", ctypes.c_uint64)]


_lib = None


def load_library():
    """dlopen libsjgpu.so (raises if it has not been built: the product path never degrades to CPU)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_paths.LIB_SJGPU):
        raise SjgpuError(f"{_paths.LIB_SJGPU} not built (run python -m simdjson_amd.build)")
    # PyTorch wheels bundle their own libamdhip64.so.7 / libhsa-runtime64.so.1, and two HIP runtimes in
    # one process cannot both open the GPU ("No HIP GPUs are available" in whichever comes second).
    # Importing torch FIRST makes the loader resolve libsjgpu's DT_NEEDED libamdhip64.so.7 to the
    # already-loaded copy (same SONAME), so a process that uses torch for device memory / streams /
    # torch.distributed and libsjgpu for the kernels runs on ONE runtime.  Pure C/C++ users of
    # libsjgpu (the simdjson plug-in shim) simply get /opt/rocm's runtime.
    if os.environ.get("SJGPU_NO_TORCH", "0") != "1":
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    L = ctypes.CDLL(_paths.LIB_SJGPU)
    vp, sz, u32p = ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint32)
    L.sjgpu_device_count.restype = ctypes.c_int
    L.sjgpu_ctx_create.restype = ctypes.c_int
    L.sjgpu_ctx_create.argtypes = [ctypes.c_int, sz, ctypes.POINTER(vp)]
    L.sjgpu_ctx_destroy.restype = None
    L.sjgpu_ctx_destroy.argtypes = [vp]
    L.sjgpu_set_capacity.restype = ctypes.c_int
    L.sjgpu_set_capacity.argtypes = [vp, sz]
    L.sjgpu_capacity.restype = sz
    L.sjgpu_capacity.argtypes = [vp]
    L.sjgpu_last_error.restype = ctypes.c_char_p
    L.sjgpu_last_error.argtypes = [vp]
    L.sjgpu_stage1.restype = ctypes.c_int
    L.sjgpu_stage1.argtypes = [vp, vp, sz, ctypes.c_int, vp, sz, u32p, u32p]
    L.sjgpu_minify.restype = ctypes.c_int
    L.sjgpu_minify.argtypes = [vp, vp, sz, vp, ctypes.POINTER(sz)]
    L.sjgpu_validate_utf8.restype = ctypes.c_int
    L.sjgpu_validate_utf8.argtypes = [vp, vp, sz, ctypes.POINTER(ctypes.c_int)]
    L.sjgpu_validate_utf8_pieces.restype = ctypes.c_int
    L.sjgpu_validate_utf8_pieces.argtypes = [vp, vp, sz, sz, ctypes.POINTER(ctypes.c_int)]
    L.sjgpu_stage1_device.restype = ctypes.c_int
    L.sjgpu_stage1_device.argtypes = [vp, vp, sz, vp, sz, vp]
    L.sjgpu_minify_device.restype = ctypes.c_int
    L.sjgpu_minify_device.argtypes = [vp, vp, sz, vp, vp]
    L.sjgpu_validate_utf8_device.restype = ctypes.c_int
    L.sjgpu_validate_utf8_device.argtypes = [vp, vp, sz, vp]
    L.sjgpu_stage1_tokens_device.restype = ctypes.c_int
    L.sjgpu_stage1_tokens_device.argtypes = [vp, vp, sz, vp, sz, vp, sz, vp]
    L.sjgpu_depth_scan_tokens_device.restype = ctypes.c_int
    L.sjgpu_depth_scan_tokens_device.argtypes = [vp, vp, ctypes.c_uint32, vp, vp]
    L.sjgpu_result.restype = ctypes.c_int
    L.sjgpu_result.argtypes = [vp, vp, ctypes.POINTER(ScanResult)]
    L.sjgpu_stage1_error_from_flags.restype = ctypes.c_int
    L.sjgpu_stage1_error_from_flags.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
    L.sjgpu_stage1_finish_host.restype = ctypes.c_int
    L.sjgpu_stage1_finish_host.argtypes = [vp, sz, ctypes.c_int, vp, ctypes.c_uint32, ctypes.c_uint32, u32p, u32p]
    L.sjgpu_debug_trace_stage1.restype = ctypes.c_int
    L.sjgpu_debug_trace_stage1.argtypes = [vp, vp, sz, vp, sz, vp, ctypes.c_uint32]
    L.sjgpu_debug_string_path.restype = ctypes.c_int
    L.sjgpu_debug_string_path.argtypes = [vp]
    L.sjgpu_debug_read_workspace.restype = ctypes.c_int
    L.sjgpu_debug_read_workspace.argtypes = [vp, ctypes.POINTER(ScanResult), vp, sz, ctypes.POINTER(sz)]
    L.sjgpu_debug_gave_up_count.restype = ctypes.c_uint64
    L.sjgpu_debug_gave_up_count.argtypes = [vp]
    L.sjgpu_debug_trace_pipelined.restype = ctypes.c_int
    L.sjgpu_debug_trace_pipelined.argtypes = [vp, vp, sz, vp, sz, vp, ctypes.c_uint32, u32p]
    L.sjgpu_stage1_many.restype = ctypes.c_int
    L.sjgpu_stage1_many.argtypes = [vp, ctypes.POINTER(Doc), sz]
    L.sjgpu_stage1_finish_device.restype = ctypes.c_int
    L.sjgpu_stage1_finish_device.argtypes = [vp, vp, sz, ctypes.c_int, vp, ctypes.c_uint32, ctypes.c_uint32, vp, u32p, u32p]
    L.sjgpu_depth_scan_device.restype = ctypes.c_int
    L.sjgpu_depth_scan_device.argtypes = [vp, vp, vp, ctypes.c_uint32, vp, vp]
    L.sjgpu_parse_strings_device.restype = ctypes.c_int
    L.sjgpu_parse_strings_device.argtypes = [vp, vp, sz, vp, ctypes.c_uint32, ctypes.c_int, vp, sz, vp, vp, ctypes.POINTER(ctypes.c_uint64), u32p, u32p]
    u64p = ctypes.POINTER(ctypes.c_uint64)
    L.sjgpu_stage2_device.restype = ctypes.c_int
    L.sjgpu_stage2_device.argtypes = [vp, vp, sz, vp, ctypes.c_uint32, ctypes.c_uint32, vp, sz, vp, sz, vp, u64p, u64p]
    L.sjgpu_stage2_tokens_device.restype = ctypes.c_int
    L.sjgpu_stage2_tokens_device.argtypes = [vp, vp, sz, vp, ctypes.c_uint32, vp, ctypes.c_uint32, vp, sz, vp, sz, vp, u64p, u64p]
    L.sjgpu_match_keys_device.restype = ctypes.c_int
    L.sjgpu_match_keys_device.argtypes = [vp, vp, sz, vp, ctypes.c_uint32, vp, vp, ctypes.c_uint32, vp, vp, u32p]
    L.sjgpu_parse.restype = ctypes.c_int
    L.sjgpu_parse.argtypes = [vp, vp, sz, ctypes.c_uint32, vp, sz, vp, sz, u64p, u64p]
    L.sjgpu_stage2_many_device.restype = ctypes.c_int
    L.sjgpu_stage2_many_device.argtypes = [vp, vp, sz, vp, ctypes.c_uint32, ctypes.c_uint32, vp, sz, vp, sz, vp, sz, vp, u32p, u64p, u64p]
    L.sjgpu_parse_many.restype = ctypes.c_int
    L.sjgpu_parse_many.argtypes = [vp, vp, sz, ctypes.c_uint32, vp, sz, vp, sz, vp, sz, u32p, u64p, u64p]
    L.sjgpu_at_pointers_device.restype = ctypes.c_int
    L.sjgpu_at_pointers_device.argtypes = [vp, vp, ctypes.c_uint64, vp, ctypes.c_uint64, vp, ctypes.c_uint32, vp, vp, ctypes.c_uint32, vp, vp, vp]
    L.sjgpu_gather_strings_device.restype = ctypes.c_int
    L.sjgpu_gather_strings_device.argtypes = [vp, vp, ctypes.c_uint64, vp, vp, ctypes.c_uint32, vp, vp, ctypes.c_uint64, vp, u64p]
    L.sjgpu_at_paths_device.restype = ctypes.c_int
    L.sjgpu_at_paths_device.argtypes = [vp, vp, ctypes.c_uint64, vp, ctypes.c_uint64, vp, ctypes.c_uint32, vp, vp, ctypes.c_uint32, vp, vp, vp, vp, ctypes.c_uint64, vp, u64p]
    L.sjgpu_at_paths_wide_device.restype = ctypes.c_int
    L.sjgpu_at_paths_wide_device.argtypes = L.sjgpu_at_paths_device.argtypes
    L.sjgpu_at_pointers_from_cells_device.restype = ctypes.c_int
    L.sjgpu_at_pointers_from_cells_device.argtypes = [vp, vp, ctypes.c_uint64, vp, ctypes.c_uint64, vp, ctypes.c_uint32, vp, vp, ctypes.c_uint32, vp, vp, ctypes.c_uint32, vp, vp, vp]
    L.sjgpu_at_paths_from_cells_device.restype = ctypes.c_int
    L.sjgpu_at_paths_from_cells_device.argtypes = [vp, vp, ctypes.c_uint64, vp, ctypes.c_uint64, vp, ctypes.c_uint32, vp, vp, ctypes.c_uint32, vp, vp, ctypes.c_uint32, vp, vp, vp, vp,
                                                   ctypes.c_uint64, vp, u64p]
    L.sjgpu_cell_kinds_device.restype = ctypes.c_int
    L.sjgpu_cell_kinds_device.argtypes = [vp, vp, vp, ctypes.c_uint32, ctypes.c_uint32, vp, vp]
    L.sjgpu_cast_cells_device.restype = ctypes.c_int
    L.sjgpu_cast_cells_device.argtypes = [vp, vp, vp, ctypes.c_uint32, ctypes.c_uint32, vp, vp, vp, vp, vp, vp]
    L.sjgpu_cast_string_cells_device.restype = ctypes.c_int
    L.sjgpu_cast_string_cells_device.argtypes = [vp, vp, ctypes.c_uint64, vp, vp, ctypes.c_uint32, ctypes.c_uint32, vp, vp, vp, vp, vp, vp]
    L.sjgpu_object_fields_from_cells_device.restype = ctypes.c_int
    L.sjgpu_object_fields_from_cells_device.argtypes = [vp, vp, ctypes.c_uint64, vp, ctypes.c_uint64, vp, ctypes.c_uint32, vp, vp, ctypes.c_uint32, vp, vp, vp, vp, vp, vp,
                                                        ctypes.c_uint64, vp, u64p]
    L.sjgpu_cell_sizes_device.restype = ctypes.c_int
    L.sjgpu_cell_sizes_device.argtypes = [vp, vp, ctypes.c_uint64, vp, ctypes.c_uint32, vp, vp, ctypes.c_uint32, vp, vp, vp]
    L.sjgpu_dictionary_encode_device.restype = ctypes.c_int
    L.sjgpu_dictionary_encode_device.argtypes = [vp, vp, ctypes.c_uint64, vp, vp, ctypes.c_uint32, vp, vp, vp, vp, vp, ctypes.c_uint64, vp, u64p]
    L.sjgpu_cell_kinds_by_code_device.restype = ctypes.c_int
    L.sjgpu_cell_kinds_by_code_device.argtypes = [vp, vp, vp, vp, ctypes.c_uint32, ctypes.c_uint32, vp, vp]
    L.sjgpu_pivot_fields_device.restype = ctypes.c_int
    L.sjgpu_pivot_fields_device.argtypes = [vp, vp, vp, ctypes.c_uint32, vp, vp, vp, ctypes.c_uint64, vp, ctypes.c_uint32, ctypes.c_uint32, vp, vp, vp]
    L.sjgpu_serialize_cells_device.restype = ctypes.c_int
    L.sjgpu_serialize_cells_device.argtypes = [vp, vp, ctypes.c_uint64, vp, ctypes.c_uint64, vp, ctypes.c_uint32, vp, vp, ctypes.c_uint32, vp, vp, vp, ctypes.c_uint64, vp, u64p]
    L.sjgpu_serialize_cells_wide_device.restype = ctypes.c_int
    L.sjgpu_serialize_cells_wide_device.argtypes = L.sjgpu_serialize_cells_device.argtypes
    L.sjgpu_prettify_cells_device.restype = ctypes.c_int
    L.sjgpu_prettify_cells_device.argtypes = L.sjgpu_serialize_cells_device.argtypes
    L.sjgpu_prettify_cells_wide_device.restype = ctypes.c_int
    L.sjgpu_prettify_cells_wide_device.argtypes = L.sjgpu_serialize_cells_device.argtypes
    L.sjgpu_write_records_device.restype = ctypes.c_int
    L.sjgpu_write_records_device.argtypes = [vp, vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, vp, vp, vp, ctypes.c_uint64, vp, vp, u64p]
    L.sjgpu_write_nested_device.restype = ctypes.c_int
    L.sjgpu_write_nested_device.argtypes = [vp, vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, vp, vp, vp, ctypes.c_uint64, vp, vp, u64p]
    L.sjgpu_comm_unique_id.restype = ctypes.c_int
    L.sjgpu_comm_unique_id.argtypes = [vp, sz]
    L.sjgpu_comm_create.restype = ctypes.c_int
    L.sjgpu_comm_create.argtypes = [ctypes.c_int, ctypes.c_int, vp, sz, ctypes.c_int, ctypes.POINTER(vp)]
    L.sjgpu_comm_destroy.restype = None
    L.sjgpu_comm_destroy.argtypes = [vp]
    L.sjgpu_comm_last_error.restype = ctypes.c_char_p
    L.sjgpu_comm_last_error.argtypes = [vp]
    L.sjgpu_comm_ranks.restype = ctypes.c_int
    L.sjgpu_comm_ranks.argtypes = [vp]
    L.sjgpu_comm_gather_indices.restype = ctypes.c_int
    L.sjgpu_comm_gather_indices.argtypes = [vp, vp, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int, vp, sz, u64p, u64p, vp]
    L.sjgpu_mgpu_create.restype = ctypes.c_int
    L.sjgpu_mgpu_create.argtypes = [ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.POINTER(vp)]
    L.sjgpu_mgpu_destroy.restype = None
    L.sjgpu_mgpu_destroy.argtypes = [vp]
    L.sjgpu_mgpu_count.restype = ctypes.c_int
    L.sjgpu_mgpu_count.argtypes = [vp]
    L.sjgpu_mgpu_stage1.restype = ctypes.c_int
    L.sjgpu_mgpu_stage1.argtypes = [vp, vp, sz, ctypes.c_int, vp, sz, u32p, u32p]
    L.sjgpu_mgpu_minify.restype = ctypes.c_int
    L.sjgpu_mgpu_minify.argtypes = [vp, vp, sz, vp, ctypes.POINTER(sz)]
    L.sjgpu_mgpu_validate_utf8.restype = ctypes.c_int
    L.sjgpu_mgpu_validate_utf8.argtypes = [vp, vp, sz, ctypes.POINTER(ctypes.c_int)]
    L.sjgpu_set_pipeline.restype = ctypes.c_int
    L.sjgpu_set_pipeline.argtypes = [vp, ctypes.c_int]
    L.sjgpu_profile_enable.restype = ctypes.c_int
    L.sjgpu_profile_enable.argtypes = [vp, ctypes.c_int]
    L.sjgpu_profile_read.restype = ctypes.c_int
    L.sjgpu_profile_read.argtypes = [vp, ctypes.POINTER(ctypes.c_double), u32p]
    L.sjgpu_trim_partial_utf8.restype = sz
    L.sjgpu_trim_partial_utf8.argtypes = [vp, sz]
    L.sjgpu_clean_cut.restype = sz
    L.sjgpu_clean_cut.argtypes = [vp, sz, sz]
    L.sjgpu_string_parity_device.restype = ctypes.c_int
    L.sjgpu_string_parity_device.argtypes = [vp, vp, sz, vp]
    L.sjgpu_stage1_shard_device.restype = ctypes.c_int
    L.sjgpu_stage1_shard_device.argtypes = [vp, vp, sz, ctypes.c_int, vp, sz, vp]
    L.sjgpu_minify_shard_device.restype = ctypes.c_int
    L.sjgpu_minify_shard_device.argtypes = [vp, vp, sz, ctypes.c_int, vp, vp]
    L.sjgpu_stage1_range_device.restype = ctypes.c_int
    L.sjgpu_stage1_range_device.argtypes = [vp, vp, sz, sz, ctypes.c_int, ctypes.c_int, ctypes.c_uint32, vp, sz, vp]
    L.sjgpu_minify_range_device.restype = ctypes.c_int
    L.sjgpu_minify_range_device.argtypes = [vp, vp, sz, sz, ctypes.c_int, ctypes.c_int, ctypes.c_uint32, vp, vp]
    L.sjgpu_last_pipeline.restype = ctypes.c_int
    L.sjgpu_last_pipeline.argtypes = [vp]
    L.sjgpu_profile_kernel.restype = ctypes.c_char_p
    L.sjgpu_profile_kernel.argtypes = [vp]
    L.sjgpu_host_alloc.restype = vp
    L.sjgpu_host_alloc.argtypes = [sz]
    L.sjgpu_host_free.restype = None
    L.sjgpu_host_free.argtypes = [vp]
    L.sjgpu_host_register.restype = ctypes.c_int
    L.sjgpu_host_register.argtypes = [vp, sz]
    L.sjgpu_host_unregister.restype = ctypes.c_int
    L.sjgpu_host_unregister.argtypes = [vp]
    _lib = L
    return L


def _as_u8(data):
    if isinstance(data, np.ndarray):
        return np.ascontiguousarray(data, dtype=np.uint8)
    return np.frombuffer(bytes(data), dtype=np.uint8).copy() if len(data) else np.zeros(0, np.uint8)


def strbuf_bytes(length):
    """the string buffer that `length` bytes of JSON can need (include/sjgpu.h, sjgpu_stage2_device)"""
    return 5 * (length // 3) + 256


def _blob(items):
    """A list of bytes as the C-ABI takes one (names, JSON pointers, paths) -> (the bytes back to back as a char pointer, their lengths as a pointer to uint32 or None
    when there are none, the count).  The two pointers are ctypes objects that keep what they point into alive: hold them for the call, no longer (the calls copy)."""
    lens = np.array([len(x) for x in items], dtype=np.uint32)
    return ctypes.cast(ctypes.c_char_p(b"".join(items)), ctypes.c_void_p), lens.ctypes.data_as(ctypes.c_void_p) if len(lens) else None, len(items)


def _to_capacity(call, cap):
    """call(cap) -> (rc, needed, outputs), the outputs allocated for `cap` by the call itself.  At most two calls: a second one, with the capacity the first
    reported, only after SJGPU_E_OVERFLOW.  -> what the last call returned"""
    rc, needed, outputs = call(cap)
    if rc == SJGPU_E_OVERFLOW:
        rc, needed, outputs = call(needed)
    return rc, needed, outputs


def _refused(name, rc):
    """raises for a call that did not end with 0; the error carries the call's answer as .code (CAPACITY: a total beyond 32 bits, which no larger array cures)"""
    if rc:
        err = SjgpuError(f"{name}: the output needs offsets beyond 32 bits (CAPACITY)" if rc == CAPACITY else f"{name} refused its arguments ({rc})")
        err.code = rc
        raise err


class ResidentStream:
    """A host buffer's way to resident tapes, the steps every *_many call begins with: upload, stage 1, sjgpu_stage2_many_device, everything on the parser's device
    and on torch's current stream (`stream`).  Holds the tensors buf, idx, tape, sbuf, table -- keep the object for as long as anything enqueued may read them --
    and n (tokens), code, docs, tw (tape words), sb (string bytes).  doc_cap: the documents to make room for, by default n (a document has a token).
    Nothing to query leaves docs == 0: an empty buffer (code EMPTY, no tensor), a stage-1 error (that code; buf and idx only), a broken first document (its code).
    The capacities are the contract of include/sjgpu_stream.h, and this is the one place that spells them."""
    PADDING = 64  # slack behind the buffer: the kernels may read it and never depend on it

    def __init__(self, parser, data, max_depth=1024, doc_cap=None):
        import torch
        a = _as_u8(data)
        self.p, self.length, self.max_depth = parser, len(a), max_depth
        self.code, self.docs, self.n, self.tw, self.sb = EMPTY, 0, 0, 0, 0
        if len(a) == 0:
            return
        self.dev = dev = torch.device("cuda", parser.device)
        self._stream = torch.cuda.current_stream(dev)
        self.stream = self._stream.cuda_stream
        self.buf = torch.from_numpy(np.concatenate([a, np.zeros(self.PADDING, np.uint8)])).to(dev)
        self.idx = torch.empty(len(a) + 16, dtype=torch.int32, device=dev)
        rc = parser.stage1_device(self.buf.data_ptr(), len(a), self.idx.data_ptr(), len(a) + 3, self.stream)
        self.n, flags, _ = parser.result(self.stream)
        self.code = rc or stage1_error_from_flags(self.n, flags)
        if self.code:
            return
        doc_cap = self.n if doc_cap is None else doc_cap
        self.tape = torch.empty(min(4 * self.n, len(a) + 3 * doc_cap) + 8, dtype=torch.int64, device=dev)
        self.sbuf = torch.empty(strbuf_bytes(len(a)), dtype=torch.uint8, device=dev)
        self.table = torch.empty((doc_cap + 1) * 4, dtype=torch.int32, device=dev)
        self.code, self.docs, self.tw, self.sb = self.stage2()

    def stage2(self):
        """sjgpu_stage2_many_device over the same buffers, once more -> (code, docs, tape words, string bytes)"""
        return self.p.stage2_many_device(self.buf.data_ptr(), self.length, self.idx.data_ptr(), self.n, self.tape.data_ptr(), self.tape.numel(), self.sbuf.data_ptr(),
                                         self.sbuf.numel(), self.table.data_ptr(), self.table.numel() // 4, self.max_depth, self.stream)

    def args(self):
        """the six arguments every query call begins with"""
        return self.tape.data_ptr(), self.tw, self.sbuf.data_ptr(), self.sb, self.table.data_ptr(), self.docs

    def synchronize(self):
        self._stream.synchronize()


class DomParserImplementation:
    """One GPU parser context == one simdjson dom_parser_implementation instance (stage-1 part).

    Mirrors the members the reference's callers touch: `n_structural_indexes`, `structural_indexes`,
    `capacity()` / `set_capacity()`, `stage1(buf, len, mode)`."""

    def __init__(self, capacity, device=0):
        self.L = load_library()
        h = ctypes.c_void_p()
        rc = self.L.sjgpu_ctx_create(int(device), int(capacity), ctypes.byref(h))
        if rc != 0:
            raise SjgpuError(f"sjgpu_ctx_create(device={device}, capacity={capacity}) failed with {rc} "
                             f"(-1 = no HIP device; this backend has no CPU fallback)")
        self.h = h
        self.device = device
        self.n_structural_indexes = 0
        self.next_structural_index = 0
        self.structural_indexes = np.zeros(((int(capacity) + 63) // 64) * 64 + 9, dtype=np.uint32)

    def close(self):
        if getattr(self, "h", None):
            self.L.sjgpu_ctx_destroy(self.h)
            self.h = None

    __del__ = close

    def capacity(self):
        return int(self.L.sjgpu_capacity(self.h))

    def set_capacity(self, capacity):
        rc = self.L.sjgpu_set_capacity(self.h, int(capacity))
        if rc == 0:
            self.structural_indexes = np.zeros(((int(capacity) + 63) // 64) * 64 + 9, dtype=np.uint32)
        return rc

    def last_error(self):
        return self.L.sjgpu_last_error(self.h).decode()

    # ---- host-buffer path (what dom::parser / ondemand::parser drive through the plug-in shim) ----
    def stage1(self, data, mode=REGULAR):
        a = _as_u8(data)
        n = ctypes.c_uint32(self.n_structural_indexes)
        nxt = ctypes.c_uint32(self.next_structural_index)
        rc = self.L.sjgpu_stage1(self.h, a.ctypes.data, len(a), int(mode), self.structural_indexes.ctypes.data,
                                 len(self.structural_indexes), ctypes.byref(n), ctypes.byref(nxt))
        self.n_structural_indexes = int(n.value)
        self.next_structural_index = int(nxt.value)
        if rc < 0:
            raise SjgpuError(f"sjgpu_stage1 infrastructure error {rc}: {self.last_error()}")
        return rc

    def minify(self, data):
        """-> (error_code, minified bytes).  The bytes are a view of a buffer owned by this object (like
        structural_indexes: allocated once, reused), valid until the next minify() call."""
        a = _as_u8(data)
        if getattr(self, "_minify_out", None) is None or len(self._minify_out) < max(len(a), 1):
            self._minify_out = np.zeros(max(len(a), 1), dtype=np.uint8)
        dst = self._minify_out
        n = ctypes.c_size_t(0)
        rc = self.L.sjgpu_minify(self.h, a.ctypes.data, len(a), dst.ctypes.data, ctypes.byref(n))
        if rc < 0:
            raise SjgpuError(f"sjgpu_minify infrastructure error {rc}: {self.last_error()}")
        return rc, dst[: n.value]

    def validate_utf8(self, data, piece_bytes=None):
        """piece_bytes: sjgpu_validate_utf8_pieces -- the same verdict with the input taken in pieces of that size"""
        a = _as_u8(data)
        ok = ctypes.c_int(0)
        if piece_bytes is None:
            rc = self.L.sjgpu_validate_utf8(self.h, a.ctypes.data, len(a), ctypes.byref(ok))
        else:
            rc = self.L.sjgpu_validate_utf8_pieces(self.h, a.ctypes.data, len(a), int(piece_bytes), ctypes.byref(ok))
        if rc != 0:
            raise SjgpuError(f"sjgpu_validate_utf8 error {rc}: {self.last_error()}")
        return bool(ok.value)

    # ---- device-resident path (pointers are raw device addresses, e.g. torch.Tensor.data_ptr()) ----
    def stage1_device(self, buf_ptr, length, idx_ptr, idx_words, stream=0):
        rc = self.L.sjgpu_stage1_device(self.h, buf_ptr, int(length), idx_ptr, int(idx_words), stream or None)
        if rc < 0:
            raise SjgpuError(f"sjgpu_stage1_device error {rc}: {self.last_error()}")
        return rc

    def stage1_tokens_device(self, buf_ptr, length, idx_ptr, idx_words, tok_ptr, tok_bytes, stream=0):
        """sjgpu_stage1_tokens_device: stage1_device + tok[i] = buf[idx[i]] beside the offsets (either pipeline; AUTO: the split one beyond the small-input limit)"""
        rc = self.L.sjgpu_stage1_tokens_device(self.h, buf_ptr, int(length), idx_ptr, int(idx_words), tok_ptr, int(tok_bytes), stream or None)
        if rc < 0:
            raise SjgpuError(f"sjgpu_stage1_tokens_device error {rc}: {self.last_error()}")
        return rc

    def minify_device(self, buf_ptr, length, dst_ptr, stream=0):
        rc = self.L.sjgpu_minify_device(self.h, buf_ptr, int(length), dst_ptr, stream or None)
        if rc < 0:
            raise SjgpuError(f"sjgpu_minify_device error {rc}: {self.last_error()}")
        return rc

    def validate_utf8_device(self, buf_ptr, length, stream=0):
        rc = self.L.sjgpu_validate_utf8_device(self.h, buf_ptr, int(length), stream or None)
        if rc < 0:
            raise SjgpuError(f"sjgpu_validate_utf8_device error {rc}: {self.last_error()}")
        return rc

    # ---- shards of one large document (sjgpu.h, "one large document sharded across GPUs") ----
    def string_parity_device(self, buf_ptr, length, stream=0):
        """-> 1 iff the shard holds an odd number of unescaped quotes (waits for `stream`)."""
        rc = self.L.sjgpu_string_parity_device(self.h, buf_ptr, int(length), stream or None)
        if rc != 0:
            raise SjgpuError(f"sjgpu_string_parity_device error {rc}: {self.last_error()}")
        return self.result(stream)[0] & 1

    def stage1_shard_device(self, buf_ptr, length, in_string, idx_ptr, idx_words, stream=0):
        rc = self.L.sjgpu_stage1_shard_device(self.h, buf_ptr, int(length), int(in_string), idx_ptr, int(idx_words), stream or None)
        if rc != 0:
            raise SjgpuError(f"sjgpu_stage1_shard_device error {rc}: {self.last_error()}")

    def minify_shard_device(self, buf_ptr, length, in_string, dst_ptr, stream=0):
        rc = self.L.sjgpu_minify_shard_device(self.h, buf_ptr, int(length), int(in_string), dst_ptr, stream or None)
        if rc != 0:
            raise SjgpuError(f"sjgpu_minify_shard_device error {rc}: {self.last_error()}")

    # ---- ranges of one resident buffer (sjgpu.h, "ranges of ONE resident buffer") ----
    def stage1_range_device(self, buf_ptr, begin, end, more, in_string, n_before, idx_ptr, idx_words, stream=0):
        rc = self.L.sjgpu_stage1_range_device(self.h, buf_ptr, int(begin), int(end), int(more), int(in_string), int(n_before),
                                              idx_ptr, int(idx_words), stream or None)
        if rc != 0:
            raise SjgpuError(f"sjgpu_stage1_range_device error {rc}: {self.last_error()}")

    def minify_range_device(self, buf_ptr, begin, end, more, in_string, out_before, dst_ptr, stream=0):
        rc = self.L.sjgpu_minify_range_device(self.h, buf_ptr, int(begin), int(end), int(more), int(in_string), int(out_before),
                                              dst_ptr, stream or None)
        if rc != 0:
            raise SjgpuError(f"sjgpu_minify_range_device error {rc}: {self.last_error()}")

    # ---- many small documents in one launch (sjgpu.h, "many small documents in one launch") ----
    def stage1_many(self, documents):
        """documents: list of bytes-like.  -> list of (error_code, n, idx[0..n+2]) as stage1(doc, REGULAR) would give."""
        arrays = [_as_u8(d) for d in documents]
        outs = [np.zeros(len(a) + 3, dtype=np.uint32) for a in arrays]
        docs = (Doc * len(arrays))()
        for k, (a, o) in enumerate(zip(arrays, outs)):
            docs[k] = Doc(a.ctypes.data if len(a) else 1, len(a), o.ctypes.data, len(o), 0, 0)
        rc = self.L.sjgpu_stage1_many(self.h, docs, len(arrays))
        if rc != 0:
            raise SjgpuError(f"sjgpu_stage1_many error {rc}: {self.last_error()}")
        return [(int(d.error), int(d.n), o[: d.n + 3].copy()) for d, o in zip(docs, outs)]

    def prepare_many(self, documents):
        """The sjgpu_doc array of a batch, marshalled ONCE: (docs, arrays, outs).  stage1_many_prepared then times the library, not ctypes."""
        arrays = [_as_u8(d) for d in documents]
        total = sum(len(a) + 3 for a in arrays)
        pool = np.zeros(total, dtype=np.uint32)  # one allocation for all lists
        docs = (Doc * len(arrays))()
        at = 0
        outs = []
        for k, a in enumerate(arrays):
            o = pool[at: at + len(a) + 3]
            at += len(a) + 3
            outs.append(o)
            docs[k] = Doc(a.ctypes.data if len(a) else 1, len(a), o.ctypes.data, len(o), 0, 0)
        return docs, arrays, outs

    def stage1_many_prepared(self, prepared):
        docs = prepared[0]
        rc = self.L.sjgpu_stage1_many(self.h, docs, len(docs))
        if rc != 0:
            raise SjgpuError(f"sjgpu_stage1_many error {rc}: {self.last_error()}")
        return docs

    # ---- the structural list after the scan, on the device ----
    def stage1_finish_device(self, buf_ptr, length, mode, idx_ptr, n_raw, flags, stream=0):
        """-> (error_code, n, next_start); idx (device) is left holding what stage1(mode) would have delivered."""
        n = ctypes.c_uint32(0)
        nxt = ctypes.c_uint32(0)
        rc = self.L.sjgpu_stage1_finish_device(self.h, buf_ptr, int(length), int(mode), idx_ptr, int(n_raw), int(flags), stream or None,
                                               ctypes.byref(n), ctypes.byref(nxt))
        if rc < 0:
            raise SjgpuError(f"sjgpu_stage1_finish_device error {rc}: {self.last_error()}")
        return rc, int(n.value), int(nxt.value)

    def depth_scan_device(self, buf_ptr, idx_ptr, n, depth_ptr, stream=0):
        rc = self.L.sjgpu_depth_scan_device(self.h, buf_ptr, idx_ptr, int(n), depth_ptr, stream or None)
        if rc != 0:
            raise SjgpuError(f"sjgpu_depth_scan_device error {rc}: {self.last_error()}")

    def depth_scan_tokens_device(self, tok_ptr, n, depth_ptr, stream=0):
        rc = self.L.sjgpu_depth_scan_tokens_device(self.h, tok_ptr, int(n), depth_ptr, stream or None)
        if rc != 0:
            raise SjgpuError(f"sjgpu_depth_scan_tokens_device error {rc}: {self.last_error()}")

    def parse_strings_device(self, buf_ptr, length, idx_ptr, n, out_ptr, out_bytes, offsets_ptr=0, allow_replacement=False, stream=0):
        """sjgpu_parse_strings_device -> (error_code, string buffer bytes used, strings, index of the first invalid string)"""
        used, cnt, bad = ctypes.c_uint64(0), ctypes.c_uint32(0), ctypes.c_uint32(0)
        rc = self.L.sjgpu_parse_strings_device(self.h, buf_ptr, int(length), idx_ptr, int(n), int(bool(allow_replacement)), out_ptr, int(out_bytes),
                                               offsets_ptr or None, stream or None, ctypes.byref(used), ctypes.byref(cnt), ctypes.byref(bad))
        if rc < 0:
            raise SjgpuError(f"sjgpu_parse_strings_device error {rc}: {self.last_error()}")
        return rc, int(used.value), int(cnt.value), int(bad.value)

    def string_path(self):
        """sjgpu_debug_string_path: 1 = the last string buffer came from the stream compaction, 2 = from the per-string walk"""
        return int(self.L.sjgpu_debug_string_path(self.h))

    def match_keys_device(self, buf_ptr, length, idx_ptr, n, names, match_ptr, stream=0):
        """sjgpu_match_keys_device: names = list of bytes; match_ptr -> n uint32 on the device.  Returns the number of matching keys."""
        m = ctypes.c_uint32(0)
        rc = self.L.sjgpu_match_keys_device(self.h, buf_ptr, int(length), idx_ptr, int(n), *_blob(names), match_ptr, stream or None, ctypes.byref(m))
        if rc != 0:
            raise SjgpuError(f"sjgpu_match_keys_device error {rc}: {self.last_error()}")
        return int(m.value)

    def stage2_device(self, buf_ptr, length, idx_ptr, n, tape_ptr, tape_cap_words, strbuf_ptr, strbuf_bytes, max_depth=1024, stream=0, tok_ptr=0):
        """sjgpu_stage2_device (tok_ptr: sjgpu_stage2_tokens_device, the token stream of stage1_tokens_device beside the list)
        -> (simdjson error_code, tape words, string buffer bytes); raises on infrastructure errors"""
        tw, sb = ctypes.c_uint64(0), ctypes.c_uint64(0)
        rc = self.L.sjgpu_stage2_tokens_device(self.h, buf_ptr, int(length), idx_ptr, int(n), tok_ptr or None, int(max_depth), tape_ptr, int(tape_cap_words), strbuf_ptr,
                                               int(strbuf_bytes), stream or None, ctypes.byref(tw), ctypes.byref(sb))
        if rc < 0:
            raise SjgpuError(f"sjgpu_stage2_device error {rc}: {self.last_error()}")
        return rc, int(tw.value), int(sb.value)

    def parse(self, data, max_depth=1024):
        """dom_parser_implementation::parse for a host buffer: (error_code, tape as uint64 array, string_buf as uint8 array)"""
        a = _as_u8(data)
        tape = np.zeros(len(a) + 8, dtype=np.uint64)
        sbuf = np.zeros(strbuf_bytes(len(a)), dtype=np.uint8)
        tw, sb = ctypes.c_uint64(0), ctypes.c_uint64(0)
        rc = self.L.sjgpu_parse(self.h, a.ctypes.data if len(a) else None, len(a), int(max_depth), tape.ctypes.data, len(tape), sbuf.ctypes.data, len(sbuf),
                                ctypes.byref(tw), ctypes.byref(sb))
        if rc < 0:
            raise SjgpuError(f"sjgpu_parse error {rc}: {self.last_error()}")
        return rc, tape[: tw.value], sbuf[: sb.value]

    def stage2_many_device(self, buf_ptr, length, idx_ptr, n, tape_ptr, tape_cap_words, strbuf_ptr, strbuf_bytes, docs_ptr, doc_cap, max_depth=1024, stream=0):
        """sjgpu_stage2_many_device: the tapes of a document stream, one per document (docs_ptr: doc_cap entries of DOC_SPAN on the device)
        -> (simdjson error_code of the first broken document or 0, documents delivered, tape words, string buffer bytes); raises on infrastructure errors"""
        docs, tw, sb = ctypes.c_uint32(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
        rc = self.L.sjgpu_stage2_many_device(self.h, buf_ptr, int(length), idx_ptr, int(n), int(max_depth), tape_ptr, int(tape_cap_words), strbuf_ptr, int(strbuf_bytes),
                                             docs_ptr, int(doc_cap), stream or None, ctypes.byref(docs), ctypes.byref(tw), ctypes.byref(sb))
        if rc < 0:
            raise SjgpuError(f"sjgpu_stage2_many_device error {rc}: {self.last_error()}")
        return rc, int(docs.value), int(tw.value), int(sb.value)

    def parse_many(self, data, max_depth=1024):
        """sjgpu_parse_many for a host buffer that holds a stream of documents: (error_code of the first broken document or 0, documents delivered,
        [(tape, string_buf) views per document], the raw arrays (tape, string_buf, table as a DOC_SPAN array of documents + 1 entries))"""
        a = _as_u8(data)
        tape = np.zeros(4 * len(a) + 8, dtype=np.uint64)  # (4 words per token always suffice, and a token is at least one byte)
        sbuf = np.zeros(strbuf_bytes(len(a)), dtype=np.uint8)
        table = np.zeros(len(a) + 2, dtype=DOC_SPAN)
        docs, tw, sb = ctypes.c_uint32(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
        rc = self.L.sjgpu_parse_many(self.h, a.ctypes.data if len(a) else None, len(a), int(max_depth), tape.ctypes.data, len(tape), sbuf.ctypes.data, len(sbuf),
                                     table.ctypes.data, len(table), ctypes.byref(docs), ctypes.byref(tw), ctypes.byref(sb))
        if rc < 0:
            raise SjgpuError(f"sjgpu_parse_many error {rc}: {self.last_error()}")
        d = int(docs.value)
        table = table[: d + 1] if d else table[:0]
        views = [(tape[int(table["tape_begin"][k]): int(table["tape_begin"][k + 1])], sbuf[int(table["string_begin"][k]): int(table["string_begin"][k + 1])])
                 for k in range(d)]
        return rc, d, views, (tape[: tw.value], sbuf[: sb.value], table)

    def at_pointers_device(self, tape_ptr, tape_words, strbuf_ptr, strbuf_bytes, docs_ptr, docs, pointers, value_ptr, tag_ptr, stream=0):
        """sjgpu_at_pointers_device: pointers = list of bytes (JSON pointers); value_ptr -> len(pointers) * docs uint64, tag_ptr -> as many bytes, row k = pointer k.
        Only enqueues the walk.  -> 0 or a negative SJGPU_E_* for arguments the call refuses (raises on HIP errors)"""
        return self._raise_infra("sjgpu_at_pointers_device", self.L.sjgpu_at_pointers_device(
            self.h, tape_ptr, int(tape_words), strbuf_ptr, int(strbuf_bytes), docs_ptr, int(docs), *_blob(pointers), value_ptr, tag_ptr, stream or None))

    def _raise_infra(self, name, rc):
        """-> rc, unless it is SJGPU_E_HIP or SJGPU_E_NOMEM: those are nobody's to handle"""
        if rc in (-2, -3):
            raise SjgpuError(f"{name} error {rc}: {self.last_error()}")
        return rc

    def gather_strings_device(self, strbuf_ptr, strbuf_bytes, value_row_ptr, tag_row_ptr, docs, offsets_ptr, chars_ptr, chars_cap, stream=0):
        """sjgpu_gather_strings_device: one column -> offsets_ptr (docs + 1 uint32) + chars_ptr (chars_cap bytes).  -> (code, bytes the characters take)"""
        total = ctypes.c_uint64(0)
        rc = self.L.sjgpu_gather_strings_device(self.h, strbuf_ptr, int(strbuf_bytes), value_row_ptr, tag_row_ptr, int(docs), offsets_ptr, chars_ptr or None, int(chars_cap),
                                                stream or None, ctypes.byref(total))
        return self._raise_infra("sjgpu_gather_strings_device", rc), int(total.value)

    def extract_many(self, data, pointers, max_depth=1024):
        """Field X of every record as a column: upload, stage 1, sjgpu_stage2_many_device and sjgpu_at_pointers_device with everything resident; only the columns come back.
        -> (error_code of the first broken document or 0, documents delivered, tags uint8[K, docs], values uint64[K, docs])"""
        import torch
        K = len(pointers)
        S = ResidentStream(self, data, max_depth)
        if S.docs == 0 or K == 0:
            return S.code, S.docs, np.zeros((K, S.docs), np.uint8), np.zeros((K, S.docs), np.uint64)
        values = torch.empty((K, S.docs), dtype=torch.int64, device=S.dev)
        tags = torch.empty((K, S.docs), dtype=torch.uint8, device=S.dev)
        _refused("sjgpu_at_pointers_device", self.at_pointers_device(*S.args(), pointers, values.data_ptr(), tags.data_ptr(), S.stream))
        S.synchronize()
        return S.code, S.docs, tags.cpu().numpy(), values.cpu().numpy().view(np.uint64)

    def at_paths_device(self, tape_ptr, tape_words, strbuf_ptr, strbuf_bytes, docs_ptr, docs, paths, offsets_ptr, status_ptr, value_ptr, tag_ptr, match_cap, stream=0):
        """sjgpu_at_paths_device: paths = list of bytes (JSONPath, wildcards allowed); offsets_ptr -> len(paths) * docs + 1 uint32, status_ptr -> len(paths) * docs bytes,
        value_ptr / tag_ptr -> match_cap uint64 / bytes.  -> (code, matches): 0, CAPACITY or a negative SJGPU_E_* (raises on HIP errors)"""
        return self._at_paths("sjgpu_at_paths_device", tape_ptr, tape_words, strbuf_ptr, strbuf_bytes, docs_ptr, docs, paths, offsets_ptr, status_ptr, value_ptr, tag_ptr, match_cap,
                              stream)

    def at_paths_wide_device(self, tape_ptr, tape_words, strbuf_ptr, strbuf_bytes, docs_ptr, docs, paths, offsets_ptr, status_ptr, value_ptr, tag_ptr, match_cap, stream=0):
        """sjgpu_at_paths_wide_device: the arguments and results of at_paths_device, the levels expanded breadth first (one large document is many lanes' work)"""
        return self._at_paths("sjgpu_at_paths_wide_device", tape_ptr, tape_words, strbuf_ptr, strbuf_bytes, docs_ptr, docs, paths, offsets_ptr, status_ptr, value_ptr, tag_ptr,
                              match_cap, stream)

    def _at_paths(self, name, tape_ptr, tape_words, strbuf_ptr, strbuf_bytes, docs_ptr, docs, paths, offsets_ptr, status_ptr, value_ptr, tag_ptr, match_cap, stream, roots=()):
        """roots: (root_value_ptr, root_tag_ptr, rows) for the call rooted at cells, which takes them behind docs"""
        matches = ctypes.c_uint64(0)
        roots = (roots[0] or None, roots[1] or None, int(roots[2])) if roots else ()
        rc = getattr(self.L, name)(self.h, tape_ptr, int(tape_words), strbuf_ptr, int(strbuf_bytes), docs_ptr, int(docs), *roots, *_blob(paths), offsets_ptr, status_ptr or None,
                                   value_ptr or None, tag_ptr or None, int(match_cap), stream or None, ctypes.byref(matches))
        return self._raise_infra(name, rc), int(matches.value)

    def _matches(self, name, S, paths, offsets, status, cap, roots=()):
        """one call of a paths entry point over the tapes of S, into values / tags it allocates for cap matches: the `call` of _to_capacity -> (rc, matches, (values, tags))"""
        import torch
        values = torch.empty(max(cap, 1), dtype=torch.int64, device=S.dev)
        tags = torch.empty(max(cap, 1), dtype=torch.uint8, device=S.dev)
        rc, matches = self._at_paths(name, *S.args(), paths, offsets.data_ptr(), status.data_ptr(), values.data_ptr(), tags.data_ptr(), cap, S.stream, roots)
        return rc, matches, (values, tags)

    def _rows_of(self, S, row_path, wide):
        """the rows of a table: the matches of row_path in the documents of S, ONE call with K = 1 (wide: of sjgpu_at_paths_wide_device), repeated once at the capacity it
        reported -> (row_offsets int32[docs + 1], row_status uint8[docs], root_values int64[>= rows], root_tags uint8[>= rows], rows), tensors of the device, enqueued only"""
        import torch
        row_offsets = torch.empty(S.docs + 1, dtype=torch.int32, device=S.dev)
        row_status = torch.empty(S.docs, dtype=torch.uint8, device=S.dev)
        name = "sjgpu_at_paths_wide_device" if wide else "sjgpu_at_paths_device"
        rc, rows, (root_values, root_tags) = _to_capacity(lambda cap: self._matches(name, S, [row_path], row_offsets, row_status, cap), int(S.tw // 8 + 1))
        _refused(name, rc)
        return row_offsets, row_status, root_values, root_tags, rows

    def explode_many(self, data, paths, max_depth=1024, first_cap=None, wide=False):
        """The arrays of every record as one ragged column: upload, stage 1, sjgpu_stage2_many_device and sjgpu_at_paths_device with everything resident (the twin of
        extract_many).  At most two calls of sjgpu_at_paths_device: a second one with the capacity the first reported (first_cap: the first call's guess, by default one
        match per tape word in eight).  wide: sjgpu_at_paths_wide_device in its place (the same column; the choice is the caller's).
        -> (error_code of the first broken document or 0, documents delivered, status uint8[K, docs], offsets uint32[K * docs + 1], tags uint8[matches], values uint64[matches])"""
        import torch
        K = len(paths)
        S = ResidentStream(self, data, max_depth)
        if S.docs == 0 or K == 0:
            return S.code, S.docs, np.zeros((K, S.docs), np.uint8), np.zeros(K * S.docs + 1, np.uint32), np.zeros(0, np.uint8), np.zeros(0, np.uint64)
        offsets = torch.empty(K * S.docs + 1, dtype=torch.int32, device=S.dev)
        status = torch.empty((K, S.docs), dtype=torch.uint8, device=S.dev)
        name = "sjgpu_at_paths_wide_device" if wide else "sjgpu_at_paths_device"
        rc, matches, (values, tags) = _to_capacity(lambda cap: self._matches(name, S, paths, offsets, status, cap), int(S.tw // 8 + 1 if first_cap is None else first_cap))
        _refused(name, rc)
        S.synchronize()
        return S.code, S.docs, status.cpu().numpy(), offsets.cpu().numpy().view(np.uint32), tags[:matches].cpu().numpy(), values[:matches].cpu().numpy().view(np.uint64)

    def at_pointers_from_cells_device(self, tape_ptr, tape_words, strbuf_ptr, strbuf_bytes, docs_ptr, docs, root_value_ptr, root_tag_ptr, rows, pointers, value_ptr, tag_ptr,
                                      stream=0):
        """sjgpu_at_pointers_from_cells_device: at_pointer rooted at the `rows` cells root_value_ptr / root_tag_ptr (a row of at_pointers_device's output, the matches of
        at_paths_device, a row of this call's own); pointers = list of bytes; value_ptr -> len(pointers) * rows uint64, tag_ptr -> as many bytes, row k = pointer k.
        Only enqueues the walk.  -> 0 or a negative SJGPU_E_* for arguments the call refuses (raises on HIP errors and on memory the context could not get)"""
        return self._raise_infra("sjgpu_at_pointers_from_cells_device", self.L.sjgpu_at_pointers_from_cells_device(
            self.h, tape_ptr, int(tape_words), strbuf_ptr, int(strbuf_bytes), docs_ptr, int(docs), root_value_ptr, root_tag_ptr, int(rows), *_blob(pointers), value_ptr, tag_ptr,
            stream or None))

    def table_many(self, data, row_path, pointers, max_depth=1024, wide=False):
        """One row per match of row_path, one column per pointer: upload, stage 1, sjgpu_stage2_many_device, ONE sjgpu_at_paths_device call with K = 1 (wide:
        sjgpu_at_paths_wide_device) and sjgpu_at_pointers_from_cells_device over its matches, with everything resident (the twin of extract_many and explode_many).
        Row r of the table is match r of the path; the rows of document d are row_offsets[d] .. row_offsets[d + 1] (a document whose status is not 0 has none).
        -> (error_code of the first broken document or 0, documents delivered, row_offsets uint32[docs + 1], tags uint8[K, rows], values uint64[K, rows])"""
        code, docs, offsets, tags, values, _ = self._table_cells(data, row_path, pointers, max_depth, wide)
        if offsets is None:
            return code, docs, np.zeros(docs + 1, np.uint32), np.zeros((len(pointers), 0), np.uint8), np.zeros((len(pointers), 0), np.uint64)
        return code, docs, offsets.cpu().numpy().view(np.uint32), tags.cpu().numpy(), values.cpu().numpy().view(np.uint64)

    def _table_cells(self, data, row_path, pointers, max_depth=1024, wide=False):
        """table_many's work with the table left on the device -> (code, docs, row_offsets int32[docs + 1], tags uint8[K, rows], values int64[K, rows], (string buffer,
        its bytes)), all torch tensors of the device, complete (the stream has been waited for); (code, 0, None, None, None, None) when no document was delivered"""
        import torch
        K = len(pointers)
        S = ResidentStream(self, data, max_depth)
        if S.docs == 0:
            return S.code, 0, None, None, None, None
        offsets, status, root_values, root_tags, rows = self._rows_of(S, row_path, wide)
        values = torch.empty((K, rows), dtype=torch.int64, device=S.dev)
        tags = torch.empty((K, rows), dtype=torch.uint8, device=S.dev)
        if K and rows:
            _refused("sjgpu_at_pointers_from_cells_device", self.at_pointers_from_cells_device(*S.args(), root_values.data_ptr(), root_tags.data_ptr(), rows, pointers,
                                                                                               values.data_ptr(), tags.data_ptr(), S.stream))
        S.synchronize()  # (S, status and the roots live until here: the walks read them)
        return S.code, S.docs, offsets, tags, values, (S.sbuf, S.sb)

    def at_paths_from_cells_device(self, tape_ptr, tape_words, strbuf_ptr, strbuf_bytes, docs_ptr, docs, root_value_ptr, root_tag_ptr, rows, paths, offsets_ptr, status_ptr,
                                   value_ptr, tag_ptr, match_cap, stream=0):
        """sjgpu_at_paths_from_cells_device: at_path_with_wildcard rooted at the `rows` cells root_value_ptr / root_tag_ptr (as for at_pointers_from_cells_device); paths = list
        of bytes; offsets_ptr -> len(paths) * rows + 1 uint32, status_ptr -> len(paths) * rows bytes, value_ptr / tag_ptr -> match_cap uint64 / bytes.
        -> (code, matches): 0, CAPACITY or a negative SJGPU_E_* (raises on HIP errors and on memory the context could not get)"""
        return self._at_paths("sjgpu_at_paths_from_cells_device", tape_ptr, tape_words, strbuf_ptr, strbuf_bytes, docs_ptr, docs, paths, offsets_ptr, status_ptr, value_ptr, tag_ptr,
                              match_cap, stream, (root_value_ptr, root_tag_ptr, rows))

    def lists_many(self, data, row_path, paths, max_depth=1024, wide=False, first_cap=None):
        """One row per match of row_path, one LIST column per path: upload, stage 1, sjgpu_stage2_many_device, ONE sjgpu_at_paths_device call with K = 1 (wide:
        sjgpu_at_paths_wide_device) and sjgpu_at_paths_from_cells_device over its matches, with everything resident (the twin of table_many).  The new call is repeated once
        with the capacity it reported (first_cap: its first guess, by default one match per tape word in eight).  Row r is match r of row_path; the rows of document d
        are row_offsets[d] .. row_offsets[d + 1]; the list of row r under path k is tags / values[offsets[k * rows + r] .. offsets[k * rows + r + 1]).
        -> (error_code of the first broken document or 0, documents delivered, row_offsets uint32[docs + 1], status uint8[K, rows], offsets uint32[K * rows + 1],
        tags uint8[matches], values uint64[matches])"""
        import torch
        K = len(paths)
        S = ResidentStream(self, data, max_depth)
        if S.docs == 0:
            return S.code, 0, np.zeros(1, np.uint32), np.zeros((K, 0), np.uint8), np.zeros(1, np.uint32), np.zeros(0, np.uint8), np.zeros(0, np.uint64)
        row_offsets, row_status, root_values, root_tags, rows = self._rows_of(S, row_path, wide)
        offsets = torch.empty(K * rows + 1, dtype=torch.int32, device=S.dev)
        status = torch.empty((K, rows), dtype=torch.uint8, device=S.dev)
        name, roots = "sjgpu_at_paths_from_cells_device", (root_values.data_ptr(), root_tags.data_ptr(), rows)
        rc, matches, (values, tags) = _to_capacity(lambda cap: self._matches(name, S, paths, offsets, status, cap, roots), int(S.tw // 8 + 1 if first_cap is None else first_cap))
        _refused(name, rc)
        S.synchronize()
        return (S.code, S.docs, row_offsets.cpu().numpy().view(np.uint32), status.cpu().numpy(), offsets.cpu().numpy().view(np.uint32), tags[:matches].cpu().numpy(),
                values[:matches].cpu().numpy().view(np.uint64))

    def object_fields_from_cells_device(self, tape_ptr, tape_words, strbuf_ptr, strbuf_bytes, docs_ptr, docs, root_value_ptr, root_tag_ptr, rows, offsets_ptr, status_ptr,
                                        key_value_ptr, key_tag_ptr, value_ptr, tag_ptr, field_cap, stream=0):
        """sjgpu_object_fields_from_cells_device: the fields of the objects the `rows` cells root_value_ptr / root_tag_ptr describe (as for at_pointers_from_cells_device);
        offsets_ptr -> rows + 1 uint32, status_ptr -> rows bytes, key_value_ptr / value_ptr -> field_cap uint64, key_tag_ptr / tag_ptr -> field_cap bytes.
        -> (code, fields): 0, CAPACITY or a negative SJGPU_E_* (raises on HIP errors and on memory the context could not get)"""
        fields = ctypes.c_uint64(0)
        rc = self.L.sjgpu_object_fields_from_cells_device(self.h, tape_ptr, int(tape_words), strbuf_ptr, int(strbuf_bytes), docs_ptr, int(docs), root_value_ptr or None,
                                                          root_tag_ptr or None, int(rows), offsets_ptr, status_ptr or None, key_value_ptr or None, key_tag_ptr or None,
                                                          value_ptr or None, tag_ptr or None, int(field_cap), stream or None, ctypes.byref(fields))
        return self._raise_infra("sjgpu_object_fields_from_cells_device", rc), int(fields.value)

    def cell_sizes_device(self, tape_ptr, tape_words, docs_ptr, docs, root_value_ptr, root_tag_ptr, rows, size_ptr, code_ptr, stream=0):
        """sjgpu_cell_sizes_device: size() of the containers the `rows` cells describe; size_ptr -> rows uint32, code_ptr -> rows bytes.  Only enqueues the launches.
        -> 0 or a negative SJGPU_E_* for arguments the call refuses (raises on HIP errors and on memory the context could not get)"""
        return self._raise_infra("sjgpu_cell_sizes_device", self.L.sjgpu_cell_sizes_device(
            self.h, tape_ptr, int(tape_words), docs_ptr, int(docs), root_value_ptr or None, root_tag_ptr or None, int(rows), size_ptr or None, code_ptr or None, stream or None))

    def _fields(self, S, roots, offsets, status, cap):
        """one sjgpu_object_fields_from_cells_device over the tapes of S, into key and value rows it allocates for cap fields: the `call` of _to_capacity
        -> (rc, fields, (key_values, key_tags, values, tags))"""
        import torch
        rows64 = [torch.empty(max(cap, 1), dtype=torch.int64, device=S.dev) for _ in range(2)]
        rows8 = [torch.empty(max(cap, 1), dtype=torch.uint8, device=S.dev) for _ in range(2)]
        rc, fields = self.object_fields_from_cells_device(*S.args(), *roots, offsets.data_ptr(), status.data_ptr(), rows64[0].data_ptr(), rows8[0].data_ptr(),
                                                          rows64[1].data_ptr(), rows8[1].data_ptr(), cap, S.stream)
        return rc, fields, (rows64[0], rows8[0], rows64[1], rows8[1])

    def fields_many(self, data, row_path, max_depth=1024, wide=False, first_cap=None):
        """One row per match of row_path, one MAP column: the fields of each row's object, keys and values.  Upload, stage 1, sjgpu_stage2_many_device, ONE
        sjgpu_at_paths_device call with K = 1 (wide: sjgpu_at_paths_wide_device), sjgpu_object_fields_from_cells_device over its matches -- repeated once with the capacity
        it reported (first_cap: its first guess, by default one field per tape word in eight) -- and ONE sjgpu_gather_strings_device over the key row, with everything
        resident (the twin of lists_many).  Row r is match r of row_path; the rows of document d are row_offsets[d] .. row_offsets[d + 1]; the fields of row r are
        offsets[r] .. offsets[r + 1] (a row whose status is not 0 has none), field i with the key key_chars[key_offsets[i] .. key_offsets[i + 1]).
        -> (error_code of the first broken document or 0, documents delivered, row_offsets uint32[docs + 1], status uint8[rows], offsets uint32[rows + 1],
        key_offsets uint32[fields + 1], key_chars uint8[...], tags uint8[fields], values uint64[fields])"""
        import torch
        S = ResidentStream(self, data, max_depth)
        if S.docs == 0:
            return (S.code, 0, np.zeros(1, np.uint32), np.zeros(0, np.uint8), np.zeros(1, np.uint32), np.zeros(1, np.uint32), np.zeros(0, np.uint8), np.zeros(0, np.uint8),
                    np.zeros(0, np.uint64))
        row_offsets, row_status, root_values, root_tags, rows = self._rows_of(S, row_path, wide)
        offsets = torch.empty(rows + 1, dtype=torch.int32, device=S.dev)
        status = torch.empty(max(rows, 1), dtype=torch.uint8, device=S.dev)
        name, roots = "sjgpu_object_fields_from_cells_device", (root_values.data_ptr(), root_tags.data_ptr(), rows)
        rc, fields, (key_values, key_tags, values, tags) = _to_capacity(lambda cap: self._fields(S, roots, offsets, status, cap),
                                                                        int(S.tw // 8 + 1 if first_cap is None else first_cap))
        _refused(name, rc)
        key_offsets = torch.empty(fields + 1, dtype=torch.int32, device=S.dev)
        gather = lambda cap: self._key_chars(S, key_values, key_tags, fields, key_offsets, cap)  # noqa: E731
        rc, total, key_chars = _to_capacity(gather, int(min(S.sb, 16 * fields)))  # (distinct keys take less than the string buffer: one call, unless keys are long)
        _refused("sjgpu_gather_strings_device", rc)
        S.synchronize()
        return (S.code, S.docs, row_offsets.cpu().numpy().view(np.uint32), status[:rows].cpu().numpy(), offsets.cpu().numpy().view(np.uint32),
                key_offsets.cpu().numpy().view(np.uint32), key_chars[:total].cpu().numpy(), tags[:fields].cpu().numpy(), values[:fields].cpu().numpy().view(np.uint64))

    def _key_chars(self, S, key_values, key_tags, fields, key_offsets, cap):
        """one sjgpu_gather_strings_device over a key row, into characters it allocates for cap bytes: the `call` of _to_capacity -> (rc, bytes, chars)"""
        import torch
        chars = torch.empty(max(cap, 1), dtype=torch.uint8, device=S.dev)
        rc, total = self.gather_strings_device(S.sbuf.data_ptr(), S.sb, key_values.data_ptr(), key_tags.data_ptr(), fields, key_offsets.data_ptr(), chars.data_ptr(), cap, S.stream)
        return rc, total, chars

    def cell_kinds_device(self, value_ptr, tag_ptr, n, K, kinds_ptr, stream=0):
        """sjgpu_cell_kinds_device: the census of K rows of n cells; kinds_ptr -> K * 16 uint32.  Only enqueues.  -> 0 or a negative SJGPU_E_* for arguments the call
        refuses (raises on HIP errors)"""
        return self._raise_infra("sjgpu_cell_kinds_device",
                                 self.L.sjgpu_cell_kinds_device(self.h, value_ptr or None, tag_ptr or None, int(n), int(K), kinds_ptr or None, stream or None))

    def cast_cells_device(self, value_ptr, tag_ptr, n, getters, value_out_ptr, code_out_ptr, valid_out_ptr, counts_out_ptr, stream=0):
        """sjgpu_cast_cells_device: row k of the K = len(getters) rows of n cells asks getters[k] (SJGPU_GET_*) of each of its cells; value_out_ptr -> K * n uint64,
        code_out_ptr -> K * n bytes, valid_out_ptr -> K * ceil(n / 64) uint64, counts_out_ptr -> K * 4 uint32; value_out_ptr / code_out_ptr may be value_ptr / tag_ptr.
        Only enqueues.  -> 0 or a negative SJGPU_E_* for arguments the call refuses (raises on HIP errors)"""
        g = np.array(list(getters), dtype=np.uint8)
        rc = self.L.sjgpu_cast_cells_device(self.h, value_ptr or None, tag_ptr or None, int(n), len(g), g.ctypes.data if len(g) else None, value_out_ptr or None,
                                            code_out_ptr or None, valid_out_ptr or None, counts_out_ptr or None, stream or None)
        return self._raise_infra("sjgpu_cast_cells_device", rc)

    def typed_table_many(self, data, row_path, pointers, getters=None, wide=False, max_depth=1024):
        """table_many with typed columns: its cells stay on the device, sjgpu_cell_kinds_device takes their census, infer_getters picks a getter per column where
        `getters` (a list of SJGPU_GET_* or 0 per pointer) gives none, ONE sjgpu_cast_cells_device call casts the columns that have a getter, and
        sjgpu_gather_strings_device turns every STRING column into offsets + characters (its invalid cells have length 0).
        -> (error_code of the first broken document or 0, documents delivered, row_offsets uint32[docs + 1], columns), columns: one dict per pointer with
            "getter"  SJGPU_GET_* or 0 (left as cells)         "kinds"   the column's census, uint32[16]
            "tags", "cells"   the column as table_many returns it, uint8[rows] / uint64[rows]
          and, with a getter,
            "values"  int64 / uint64 / float64 / bool [rows]; the cells' words (uint64) for ARRAY and OBJECT; for STRING "offsets" uint32[rows + 1] and "chars" uint8
            "valid"   the Arrow validity buffer, uint8[ceil(rows / 64) * 8], least significant bit first      "codes"  uint8[rows], 0 = valid
            "counts"  uint32[4]: valid cells, nulls, NUMBER_OUT_OF_RANGE cells, cells that held a code before the cast"""
        import torch
        K = len(pointers)
        code, docs, offsets, tags, values, strings = self._table_cells(data, row_path, pointers, max_depth, wide)
        if offsets is None:
            return code, docs, np.zeros(docs + 1, np.uint32), [{"getter": 0, "kinds": np.zeros(16, np.uint32), "tags": np.zeros(0, np.uint8), "cells": np.zeros(0, np.uint64)}
                                                                for _ in range(K)]
        dev = tags.device
        stream = torch.cuda.current_stream(dev).cuda_stream
        rows = tags.shape[1]
        kinds = torch.empty((K, 16), dtype=torch.int32, device=dev)
        if K:
            _refused("sjgpu_cell_kinds_device", self.cell_kinds_device(values.data_ptr(), tags.data_ptr(), rows, K, kinds.data_ptr(), stream))
        kinds_h = kinds.cpu().numpy().view(np.uint32)
        inferred = infer_getters(kinds_h)
        picked = [inferred[k] if getters is None or not getters[k] else int(getters[k]) for k in range(K)]
        cast = [k for k in range(K) if picked[k]]
        tags_h, cells_h = tags.cpu().numpy(), values.cpu().numpy().view(np.uint64)
        columns = [{"getter": picked[k], "kinds": kinds_h[k], "tags": tags_h[k], "cells": cells_h[k]} for k in range(K)]
        if not cast:
            return code, docs, offsets.cpu().numpy().view(np.uint32), columns
        C, W = len(cast), (rows + 63) // 64
        index = torch.tensor(cast, dtype=torch.int64, device=dev)
        in_values, in_tags = values.index_select(0, index).contiguous(), tags.index_select(0, index).contiguous()  # the rows with a getter, back to back
        out_values = torch.empty((C, rows), dtype=torch.int64, device=dev)
        out_codes = torch.empty((C, rows), dtype=torch.uint8, device=dev)
        valid = torch.empty((C, W), dtype=torch.int64, device=dev)
        counts = torch.empty((C, 4), dtype=torch.int32, device=dev)
        _refused("sjgpu_cast_cells_device", self.cast_cells_device(in_values.data_ptr(), in_tags.data_ptr(), rows, [picked[k] for k in cast], out_values.data_ptr(),
                                                                   out_codes.data_ptr(), valid.data_ptr(), counts.data_ptr(), stream))
        sbuf, sb = strings
        gathered = {}
        for j, k in enumerate(cast):
            if picked[k] != GET_STRING:
                continue
            # a cell that is no string has code != 0 and value 0; the gather wants the tags: the valid cells of a STRING column are exactly its `"` cells
            soff = torch.empty(rows + 1, dtype=torch.int32, device=dev)

            def gather(cap):  # the first call only asks: capacity 0 and no characters' address
                chars = torch.empty(max(cap, 1), dtype=torch.uint8, device=dev)
                rc, total = self.gather_strings_device(sbuf.data_ptr(), sb, in_values[j].data_ptr(), in_tags[j].data_ptr(), rows, soff.data_ptr(), chars.data_ptr() if cap else 0, cap,
                                                       stream)
                return rc, total, chars
            rc, total, chars = _to_capacity(gather, 0)
            _refused("sjgpu_gather_strings_device", rc)
            gathered[k] = (soff, chars[:total])
        torch.cuda.current_stream(dev).synchronize()
        out_h, codes_h, valid_h, counts_h = out_values.cpu().numpy(), out_codes.cpu().numpy(), valid.cpu().numpy(), counts.cpu().numpy().view(np.uint32)
        for j, k in enumerate(cast):
            col = columns[k]
            col["codes"], col["counts"], col["valid"] = codes_h[j], counts_h[j], valid_h[j].view(np.uint8)
            g = picked[k]
            if g == GET_STRING:
                col["offsets"], col["chars"] = gathered[k][0].cpu().numpy().view(np.uint32), gathered[k][1].cpu().numpy()
            elif g == GET_INT64:
                col["values"] = out_h[j]
            elif g == GET_DOUBLE:
                col["values"] = out_h[j].view(np.float64)
            elif g == GET_BOOL:
                col["values"] = out_h[j] != 0
            else:
                col["values"] = out_h[j].view(np.uint64)
        return code, docs, offsets.cpu().numpy().view(np.uint32), columns

    def result(self, stream=0):  # waits for `stream`
        r = ScanResult()
        rc = self.L.sjgpu_result(self.h, stream or None, ctypes.byref(r))
        if rc != 0:
            raise SjgpuError(f"sjgpu_result error {rc}: {self.last_error()}")
        return int(r.n), int(r.flags), int(r.out_len)


    def debug_trace_stage1(self, buf_ptr, length, idx_ptr, idx_words, tiles):
        """-> uint64[tiles, 8] wall-clock stamps (100 MHz) of the single-pass kernel's phases."""
        out = np.zeros((int(tiles), 8), dtype=np.uint64)
        rc = self.L.sjgpu_debug_trace_stage1(self.h, buf_ptr, int(length), idx_ptr, int(idx_words), out.ctypes.data, int(tiles))
        if rc != 0:
            raise SjgpuError(f"sjgpu_debug_trace_stage1 error {rc}: {self.last_error()}")
        return out

    def read_workspace(self):
        """sjgpu_debug_read_workspace -> ((n, flags, out_len) as the device holds them, uint64[words allocated]: the single-pass workspace,
        [tile descriptors][control words], which every single-pass kernel leaves all zero.  Waits for the device; changes nothing."""
        r = ScanResult()
        words = ctypes.c_size_t(0)
        rc = self.L.sjgpu_debug_read_workspace(self.h, ctypes.byref(r), None, 0, ctypes.byref(words))
        out = np.zeros(int(words.value), dtype=np.uint64)
        if rc == 0 and len(out):
            rc = self.L.sjgpu_debug_read_workspace(self.h, ctypes.byref(r), out.ctypes.data, len(out), ctypes.byref(words))
        if rc != 0 or int(words.value) != len(out):
            raise SjgpuError(f"sjgpu_debug_read_workspace error {rc}: {self.last_error()}")
        return (int(r.n), int(r.flags), int(r.out_len)), out

    def gave_up_count(self):
        """sjgpu_debug_gave_up_count: results with F_INTERNAL this context has read since it was created or taken from the pool"""
        return int(self.L.sjgpu_debug_gave_up_count(self.h))

    def set_pipeline(self, pipeline="auto"):
        """"split" | "fused" | "auto" (also accepts True = fused / False = split)."""
        if isinstance(pipeline, bool):
            pipeline = "fused" if pipeline else "split"
        return self.L.sjgpu_set_pipeline(self.h, {"split": 0, "fused": 1, "auto": 2}[pipeline])

    def last_pipeline(self):
        """"fused" | "split": what the last enqueued scan used (AUTO decides by size and, for stage 1, output density)."""
        return "fused" if self.L.sjgpu_last_pipeline(self.h) == 1 else "split"

    def profile_kernel(self):
        """Name(s) of the scan kernel(s) the last enqueued call launched, as the launcher reported them."""
        return self.L.sjgpu_profile_kernel(self.h).decode()

    def profile_enable(self, on=True):
        rc = self.L.sjgpu_profile_enable(self.h, 1 if on else 0)
        if rc != 0:
            raise SjgpuError(f"sjgpu_profile_enable error {rc}: {self.last_error()}")

    def profile_read(self):
        """-> ([ms_sum per kernel slot], calls) accumulated since the last read (HIP events on the launch stream)."""
        ms = (ctypes.c_double * 3)()
        calls = ctypes.c_uint32(0)
        rc = self.L.sjgpu_profile_read(self.h, ms, ctypes.byref(calls))
        if rc != 0:
            raise SjgpuError(f"sjgpu_profile_read error {rc}: {self.last_error()}")
        return [float(x) for x in ms], int(calls.value)


COMM_ID_BYTES = 128


# ---- numbers held in strings (include/sjgpu_cast_strings.h): free functions over a parser, as simdjson_amd/dictionary.py's are ----------------------------------
def cast_string_cells_device(p, strbuf_ptr, strbuf_bytes, value_ptr, tag_ptr, n, getters, value_out_ptr, code_out_ptr, valid_out_ptr, counts_out_ptr, stream=0):
    """sjgpu_cast_string_cells_device: row k of the K = len(getters) rows of n cells asks getters[k] (GETS_INT64 / GETS_UINT64 / GETS_DOUBLE, optionally
    | GETS_OR_NUMBER) of each of its cells, whose strings lie in strbuf_ptr[0 .. strbuf_bytes); value_out_ptr -> K * n uint64, code_out_ptr -> K * n bytes,
    valid_out_ptr -> K * ceil(n / 64) uint64, counts_out_ptr -> K * 8 uint32; value_out_ptr / code_out_ptr may be value_ptr / tag_ptr.
    Only enqueues.  -> 0 or a negative SJGPU_E_* for arguments the call refuses (raises on HIP errors)"""
    g = np.array(list(getters), dtype=np.uint8)
    rc = p.L.sjgpu_cast_string_cells_device(p.h, strbuf_ptr or None, int(strbuf_bytes), value_ptr or None, tag_ptr or None, int(n), len(g),
                                            g.ctypes.data if len(g) else None, value_out_ptr or None, code_out_ptr or None, valid_out_ptr or None,
                                            counts_out_ptr or None, stream or None)
    return p._raise_infra("sjgpu_cast_string_cells_device", rc)


def numbers_in_strings_many(p, data, row_path, pointers, getters, wide=False, max_depth=1024):
    """table_many whose columns are numbers written inside strings (`"id_str": "505874924095815700"`): its cells stay on the device and ONE
    sjgpu_cast_string_cells_device call asks getters[k] (GETS_INT64 / GETS_UINT64 / GETS_DOUBLE, optionally | GETS_OR_NUMBER for columns that hold numbers
    as well) of the cells of pointer k, reading each string where it lies in the stream's string buffer.
    -> (error_code of the first broken document or 0, documents delivered, row_offsets uint32[docs + 1], columns), columns: one dict per pointer with
        "getter"  the getter byte                          "tags", "cells"   the column as table_many returns it, uint8[rows] / uint64[rows]
        "values"  int64 / uint64 / float64 [rows]           "valid"   the Arrow validity buffer, uint8[ceil(rows / 64) * 8], least significant bit first
        "codes"   uint8[rows], 0 = valid, else NUMBER_ERROR 9, INCORRECT_TYPE 17, NUMBER_OUT_OF_RANGE 18 or the code the cell held
        "counts"  uint32[8]: valid cells, nulls, NUMBER_ERROR cells, cells that held a code, cells refused for their kind, cells decided by the exact road,
                  string cells that point outside the buffer, 0"""
    import torch
    K = len(pointers)
    if len(getters) != K:
        raise ValueError("one getter per pointer")
    code, docs, offsets, tags, values, strings = p._table_cells(data, row_path, pointers, max_depth, wide)
    if offsets is None:
        return code, docs, np.zeros(docs + 1, np.uint32), [{"getter": int(getters[k]), "tags": np.zeros(0, np.uint8), "cells": np.zeros(0, np.uint64)} for k in range(K)]
    dev = tags.device
    stream = torch.cuda.current_stream(dev).cuda_stream
    rows = tags.shape[1]
    W = (rows + 63) // 64
    out_values = torch.empty((K, rows), dtype=torch.int64, device=dev)
    out_codes = torch.empty((K, rows), dtype=torch.uint8, device=dev)
    valid = torch.empty((K, W), dtype=torch.int64, device=dev)
    counts = torch.zeros((K, 8), dtype=torch.int32, device=dev)
    sbuf, sb = strings
    _refused("sjgpu_cast_string_cells_device", cast_string_cells_device(p, sbuf.data_ptr(), sb, values.data_ptr(), tags.data_ptr(), rows, getters, out_values.data_ptr(),
                                                                        out_codes.data_ptr(), valid.data_ptr(), counts.data_ptr(), stream))
    torch.cuda.current_stream(dev).synchronize()
    tags_h, cells_h = tags.cpu().numpy(), values.cpu().numpy().view(np.uint64)
    out_h, codes_h, valid_h, counts_h = out_values.cpu().numpy(), out_codes.cpu().numpy(), valid.cpu().numpy(), counts.cpu().numpy().view(np.uint32)
    columns = []
    for k in range(K):
        g = int(getters[k]) & 0x0F
        columns.append({"getter": int(getters[k]), "tags": tags_h[k], "cells": cells_h[k], "codes": codes_h[k], "counts": counts_h[k], "valid": valid_h[k].view(np.uint8),
                        "values": out_h[k] if g == GETS_INT64 else out_h[k].view(np.float64) if g == GETS_DOUBLE else out_h[k].view(np.uint64)})
    return code, docs, offsets.cpu().numpy().view(np.uint32), columns


def comm_unique_id():
    """128 bytes rank 0 makes and hands to every other rank (sjgpu_comm_unique_id = ncclGetUniqueId)"""
    L = load_library()
    buf = ctypes.create_string_buffer(COMM_ID_BYTES)
    rc = L.sjgpu_comm_unique_id(buf, COMM_ID_BYTES)
    if rc != 0:
        raise SjgpuError(f"sjgpu_comm_unique_id error {rc}")
    return bytes(buf.raw)


class Comm:
    """sjgpu_comm_*: the RCCL communicator of the index concatenation, one process per GPU (collective calls)."""

    def __init__(self, rank, world, unique_id, device):
        self.L = load_library()
        self.h = ctypes.c_void_p()
        self.rank, self.world = rank, world
        rc = self.L.sjgpu_comm_create(rank, world, unique_id, len(unique_id), device, ctypes.byref(self.h))
        if rc != 0:
            raise SjgpuError(f"sjgpu_comm_create error {rc}: {self.L.sjgpu_comm_last_error(None).decode()}")

    def ranks(self):
        """ncclCommCount: the ranks RCCL itself sees in this communicator"""
        return int(self.L.sjgpu_comm_ranks(self.h))

    def close(self):
        if self.h:
            self.L.sjgpu_comm_destroy(self.h)
            self.h = ctypes.c_void_p()

    def gather_indices(self, idx_ptr, n, base, root, out_ptr, out_cap_words, stream=0):
        """-> (total structurals, [n of every rank]); the root's out array holds base + offset as u64, shards in rank order"""
        total = ctypes.c_uint64(0)
        counts = (ctypes.c_uint64 * self.world)()
        rc = self.L.sjgpu_comm_gather_indices(self.h, idx_ptr, int(n), int(base), int(root), out_ptr or None, int(out_cap_words), ctypes.byref(total), counts,
                                              stream or None)
        if rc != 0:
            raise SjgpuError(f"sjgpu_comm_gather_indices error {rc}: {self.L.sjgpu_comm_last_error(self.h).decode()}")
        return int(total.value), [int(c) for c in counts]


class MultiGpu:
    """sjgpu_mgpu (include/sjgpu.h): one host buffer, one shard per listed device, one process.  Same member names as
    DomParserImplementation for the host-buffer calls."""

    def __init__(self, devices):
        self.L = load_library()
        arr = (ctypes.c_int * len(devices))(*devices)
        h = ctypes.c_void_p()
        rc = self.L.sjgpu_mgpu_create(arr, len(devices), ctypes.byref(h))
        if rc != 0:
            raise SjgpuError(f"sjgpu_mgpu_create({list(devices)}) failed with {rc}")
        self.h = h
        self.n_structural_indexes = 0
        self.next_structural_index = 0
        self.structural_indexes = np.zeros(0, dtype=np.uint32)

    def close(self):
        if getattr(self, "h", None):
            self.L.sjgpu_mgpu_destroy(self.h)
            self.h = None

    __del__ = close

    def stage1(self, data, mode=REGULAR):
        a = _as_u8(data)
        if len(self.structural_indexes) < len(a) + 3:
            self.structural_indexes = np.zeros(len(a) + 64, dtype=np.uint32)
        n = ctypes.c_uint32(self.n_structural_indexes)
        nxt = ctypes.c_uint32(self.next_structural_index)
        rc = self.L.sjgpu_mgpu_stage1(self.h, a.ctypes.data, len(a), int(mode), self.structural_indexes.ctypes.data, len(self.structural_indexes),
                                      ctypes.byref(n), ctypes.byref(nxt))
        self.n_structural_indexes, self.next_structural_index = int(n.value), int(nxt.value)
        if rc < 0:
            raise SjgpuError(f"sjgpu_mgpu_stage1 infrastructure error {rc}")
        return rc

    def minify(self, data):
        a = _as_u8(data)
        dst = np.zeros(max(len(a), 1), dtype=np.uint8)
        n = ctypes.c_size_t(0)
        rc = self.L.sjgpu_mgpu_minify(self.h, a.ctypes.data, len(a), dst.ctypes.data, ctypes.byref(n))
        if rc < 0:
            raise SjgpuError(f"sjgpu_mgpu_minify infrastructure error {rc}")
        return rc, dst[: n.value]

    def validate_utf8(self, data):
        a = _as_u8(data)
        ok = ctypes.c_int(0)
        rc = self.L.sjgpu_mgpu_validate_utf8(self.h, a.ctypes.data, len(a), ctypes.byref(ok))
        if rc != 0:
            raise SjgpuError(f"sjgpu_mgpu_validate_utf8 error {rc}")
        return bool(ok.value)


def stream_register(arr):
    """sjgpu_stream_register over a numpy uint8 array: stage1 calls on windows (views) of it are answered from a look-ahead span"""
    L = load_library()
    L.sjgpu_stream_register.restype = ctypes.c_int
    L.sjgpu_stream_register.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
    return L.sjgpu_stream_register(arr.ctypes.data, arr.nbytes)


def stream_unregister(arr, named=False):
    """named: say WHICH registration over that base leaves (sjgpu_stream_unregister_len: the one made with this array's length)"""
    L = load_library()
    L.sjgpu_stream_unregister.restype = ctypes.c_int
    L.sjgpu_stream_unregister.argtypes = [ctypes.c_void_p]
    L.sjgpu_stream_unregister_len.restype = ctypes.c_int
    L.sjgpu_stream_unregister_len.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
    return L.sjgpu_stream_unregister_len(arr.ctypes.data, arr.nbytes) if named else L.sjgpu_stream_unregister(arr.ctypes.data)


def stream_extent(arr):
    L = load_library()
    L.sjgpu_debug_stream_extent.restype = ctypes.c_size_t
    L.sjgpu_debug_stream_extent.argtypes = [ctypes.c_void_p]
    return int(L.sjgpu_debug_stream_extent(arr.ctypes.data))


def stage1_error_from_flags(n, flags):
    return int(load_library().sjgpu_stage1_error_from_flags(int(n), int(flags)))


def host_register(arr):
    """Page-lock a long-lived numpy array (sjgpu_host_register); call host_unregister before dropping it."""
    rc = load_library().sjgpu_host_register(arr.ctypes.data, arr.nbytes)
    if rc != 0:
        raise SjgpuError(f"sjgpu_host_register failed with {rc}")


def host_unregister(arr):
    load_library().sjgpu_host_unregister(arr.ctypes.data)


def clean_cut(buf, target):
    """First cut >= target where only the in-string bit crosses (sjgpu_clean_cut), or len(buf)."""
    a = _as_u8(buf)
    return int(load_library().sjgpu_clean_cut(a.ctypes.data, len(a), int(target)))


def device_count():
    return int(load_library().sjgpu_device_count())
