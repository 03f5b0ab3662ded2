"""CPU tier: include/sjgpu_write.h -- typed columns as JSON records, an extension of the C-ABI with a header of its own -- declares exactly what capi.WRITE_EXPORTS
lists, the library exports it, and the header stands on include/sjgpu_json.h and the headers below it without changing them (the twin of tests/test_json_header.py)."""
import os
import re
import subprocess

from simdjson_amd import _paths, build, capi


def test_write_exports_match_header():
    build.build_sjgpu()
    lib = capi.load_library()
    hdr = open(os.path.join(_paths.INCLUDE_DIR, "sjgpu_write.h")).read()
    declared = sorted(set(re.findall(r"^int (sjgpu_[a-z0-9_]+)\(", hdr, re.M)))
    assert declared == sorted(capi.WRITE_EXPORTS) == ["sjgpu_write_records_device"]
    for name in declared:
        assert hasattr(lib, name), name
    for other in ("sjgpu.h", "sjgpu_stream.h", "sjgpu_query.h", "sjgpu_paths.h", "sjgpu_rows.h", "sjgpu_lists.h", "sjgpu_cast.h", "sjgpu_fields.h", "sjgpu_dict.h", "sjgpu_json.h"):
        text = open(os.path.join(_paths.INCLUDE_DIR, other)).read()
        assert not any(name in text for name in declared)  # declared once, in the extension
    assert not set(capi.WRITE_EXPORTS) & (set(capi.EXPORTS) | set(capi.STREAM_EXPORTS) | set(capi.QUERY_EXPORTS) | set(capi.PATH_EXPORTS) | set(capi.ROWS_EXPORTS) |
                                          set(capi.LISTS_EXPORTS) | set(capi.CAST_EXPORTS) | set(capi.FIELDS_EXPORTS) | set(capi.DICT_EXPORTS) | set(capi.JSON_EXPORTS))
    assert '#include "sjgpu_json.h"' in hdr
    assert lib.sjgpu_write_records_device.argtypes is not None and len(lib.sjgpu_write_records_device.argtypes) == 12


def test_the_constants_and_the_column_are_the_headers():
    hdr = open(os.path.join(_paths.INCLUDE_DIR, "sjgpu_write.h")).read()
    names = dict((k, int(v)) for k, v in re.findall(r"(SJGPU_(?:COL|WRITE)_[A-Z0-9_]+) = (\d+)", hdr))
    assert names == {"SJGPU_COL_INT64": capi.COL_INT64, "SJGPU_COL_UINT64": capi.COL_UINT64, "SJGPU_COL_DOUBLE": capi.COL_DOUBLE, "SJGPU_COL_BOOL": capi.COL_BOOL,
                     "SJGPU_COL_STRING": capi.COL_STRING, "SJGPU_COL_JSON": capi.COL_JSON, "SJGPU_COL_STRING_CELLS": capi.COL_STRING_CELLS,
                     "SJGPU_WRITE_OMIT_NULLS": capi.WRITE_OMIT_NULLS, "SJGPU_WRITE_NEWLINE": capi.WRITE_NEWLINE}
    assert (capi.COL_INT64, capi.COL_UINT64, capi.COL_DOUBLE, capi.COL_BOOL) == (capi.GET_INT64, capi.GET_UINT64, capi.GET_DOUBLE, capi.GET_BOOL)
    import ctypes
    assert ctypes.sizeof(capi.WriteColumn) == 56 and capi.WriteColumn.chars_bytes.offset == 48 and capi.WriteColumn.kind.offset == 12


def test_the_bindings_are_functions_of_a_module_of_their_own():
    """tests/test_stream_order_cases.py asks every public method of the parser that takes a stream to be a key of a table that may not change: the bindings of
    this header are free functions that take the parser first"""
    import inspect

    from simdjson_amd import writer
    for name in ("write_records_device", "write_records", "project_many"):
        f = getattr(writer, name)
        assert inspect.isfunction(f) and next(iter(inspect.signature(f).parameters)) == "p" and not hasattr(capi.DomParserImplementation, name)
    assert inspect.signature(writer.write_records_device).parameters["stream"].default == 0
    assert list(inspect.signature(writer.write_records_device).parameters) == ["p", "columns", "n", "flags", "offsets_ptr", "status_ptr", "chars_ptr", "chars_cap", "counts_ptr",
                                                                                "stream"]
    assert list(inspect.signature(writer.write_records).parameters) == ["p", "columns", "n", "omit_nulls", "newline", "stream"]
    assert list(inspect.signature(writer.project_many).parameters)[:4] == ["p", "data", "fields", "omit_nulls"]


def test_the_library_is_built_from_the_new_unit_and_its_headers():
    assert "sjgpu_write.hip" in build.SJGPU_SOURCES and {"sj_dtoa.h", "sj_json_text.h", "sj_write_table.h"} <= set(build.SJGPU_HEADERS)


def test_the_staged_road_is_a_build_macro_not_a_switch():
    """-DSJGPU_WRITE_DIRECT_ONLY compiles the staged road out for the lab; nothing reads the environment"""
    src = open(os.path.join(_paths.PKG_DIR, "csrc", "sjgpu_write.hip")).read()
    assert "#ifndef SJGPU_WRITE_DIRECT_ONLY" in src and "getenv" not in src and "static_assert" in src


def test_write_header_is_plain_c(tmp_path):
    """the header compiles as C99 and as C++ on its own"""
    src = ('#include "sjgpu_write.h"\ntypedef char column_is_56_bytes[sizeof(sjgpu_write_column) == 56 ? 1 : -1];\n'
           "int main(void) { sjgpu_write_column c; c.kind = SJGPU_COL_STRING_CELLS; c.key_len = SJGPU_WRITE_OMIT_NULLS | SJGPU_WRITE_NEWLINE;\n"
           "  return sjgpu_write_records_device == 0 || sjgpu_serialize_cells_device == 0 || sjgpu_gather_strings_device == 0 || c.kind == c.key_len; }\n")
    for name, cc, std in (("t.c", "gcc", "-std=c99"), ("t.cpp", "g++", "-std=c++17")):
        path = tmp_path / name
        path.write_text(src)
        subprocess.run([cc, std, "-Wall", "-Werror", "-Wno-address", "-I", _paths.INCLUDE_DIR, "-c", str(path), "-o", str(tmp_path / (name + ".o"))], check=True)
