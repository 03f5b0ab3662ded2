"""CPU tier: include/sjgpu_nested.h -- list columns and array rows as nested JSON, an extension of the C-ABI with a header of its own -- declares exactly what
capi.NESTED_EXPORTS lists, the library exports it, and the header stands on include/sjgpu_write.h without changing it (the twin of tests/test_write_header.py)."""
import ctypes
import os
import re
import subprocess

from simdjson_amd import _paths, build, capi


def test_nested_exports_match_header():
    build.build_sjgpu()
    lib = capi.load_library()
    hdr = open(os.path.join(_paths.INCLUDE_DIR, "sjgpu_nested.h")).read()
    declared = sorted(set(re.findall(r"^int (sjgpu_[a-z0-9_]+)\(", hdr, re.M)))
    assert declared == sorted(capi.NESTED_EXPORTS) == ["sjgpu_write_nested_device"]
    for name in declared:
        assert hasattr(lib, name), name
    for other in ("sjgpu.h", "sjgpu_stream.h", "sjgpu_query.h", "sjgpu_paths.h", "sjgpu_rows.h", "sjgpu_lists.h", "sjgpu_cast.h", "sjgpu_fields.h", "sjgpu_dict.h", "sjgpu_json.h",
                  "sjgpu_write.h"):
        text = open(os.path.join(_paths.INCLUDE_DIR, other)).read()
        assert not any(name in text for name in declared) and "sjgpu_write_field" not in text  # declared once, in the extension
    assert not set(capi.NESTED_EXPORTS) & (set(capi.EXPORTS) | set(capi.STREAM_EXPORTS) | set(capi.QUERY_EXPORTS) | set(capi.PATH_EXPORTS) | set(capi.ROWS_EXPORTS) |
                                           set(capi.LISTS_EXPORTS) | set(capi.CAST_EXPORTS) | set(capi.FIELDS_EXPORTS) | set(capi.DICT_EXPORTS) | set(capi.JSON_EXPORTS) |
                                           set(capi.WRITE_EXPORTS))
    assert '#include "sjgpu_write.h"' in hdr
    assert lib.sjgpu_write_nested_device.argtypes is not None and len(lib.sjgpu_write_nested_device.argtypes) == 12


def test_the_constants_and_the_field_are_the_headers():
    hdr = open(os.path.join(_paths.INCLUDE_DIR, "sjgpu_nested.h")).read()
    names = dict((k, int(v)) for k, v in re.findall(r"(SJGPU_WRITE_[A-Z0-9_]+) = (\d+)", hdr))
    assert names == {"SJGPU_WRITE_ARRAY_ROWS": capi.WRITE_ARRAY_ROWS, "SJGPU_WRITE_BARE": capi.WRITE_BARE, "SJGPU_WRITE_OMIT_NULLS": capi.WRITE_OMIT_NULLS,
                     "SJGPU_WRITE_NEWLINE": capi.WRITE_NEWLINE}
    assert len({capi.WRITE_OMIT_NULLS, capi.WRITE_NEWLINE, capi.WRITE_ARRAY_ROWS, capi.WRITE_BARE}) == 4
    assert ctypes.sizeof(capi.WriteField) == 80 and capi.WriteField.col.offset == 0 and capi.WriteField.list_offsets_dev.offset == 56
    assert capi.WriteField.list_valid_dev.offset == 64 and capi.WriteField.elements.offset == 72


def test_the_bindings_are_functions_of_the_writers_module():
    import inspect

    from simdjson_amd import writer
    for name in ("write_nested_device", "write_nested", "project_rows_many"):
        f = getattr(writer, name)
        assert inspect.isfunction(f) and next(iter(inspect.signature(f).parameters)) == "p" and not hasattr(capi.DomParserImplementation, name)
    assert inspect.signature(writer.write_nested_device).parameters["stream"].default == 0
    assert list(inspect.signature(writer.write_nested_device).parameters) == ["p", "fields", "n", "flags", "offsets_ptr", "status_ptr", "chars_ptr", "chars_cap", "counts_ptr", "stream"]
    assert list(inspect.signature(writer.write_nested).parameters)[:7] == ["p", "fields", "n", "omit_nulls", "newline", "array_rows", "bare"]
    assert list(inspect.signature(writer.project_rows_many).parameters)[:5] == ["p", "data", "row_path", "fields", "omit_nulls"]


def test_the_library_is_built_from_the_kernels_and_the_hosts_table():
    assert "sjgpu_write.hip" in build.SJGPU_SOURCES and "sj_nested_table.h" in build.SJGPU_HEADERS
    src = open(os.path.join(_paths.PKG_DIR, "csrc", "sjgpu_write.hip")).read()
    assert "k_nested_count" in src and "k_nested_fill" in src and "write_row<true, true>" in src and "write_row<false, true>" in src


def test_the_split_is_a_build_macro_not_a_switch():
    """-DSJGPU_NESTED_SPLIT compiles the groups of 128, 64 and 32 rows in for the lab (they lost the measurement); nothing reads the environment"""
    src = open(os.path.join(_paths.PKG_DIR, "csrc", "sjgpu_write.hip")).read()
    assert "#ifdef SJGPU_NESTED_SPLIT" in src and "getenv" not in src


def test_nested_header_is_plain_c(tmp_path):
    """the header compiles as C99 and as C++ on its own"""
    src = ('#include "sjgpu_nested.h"\ntypedef char field_is_80_bytes[sizeof(sjgpu_write_field) == 80 ? 1 : -1];\n'
           "int main(void) { sjgpu_write_field f; f.col.kind = SJGPU_COL_STRING_CELLS; f.elements = SJGPU_WRITE_ARRAY_ROWS | SJGPU_WRITE_BARE | SJGPU_WRITE_NEWLINE;\n"
           "  f.list_offsets_dev = 0; f.list_valid_dev = 0;\n"
           "  return sjgpu_write_nested_device == 0 || sjgpu_write_records_device == 0 || f.col.kind == f.elements || f.list_offsets_dev != f.list_valid_dev; }\n")
    for name, cc, std in (("t.c", "gcc", "-std=c99"), ("t.cpp", "g++", "-std=c++17")):
        path = tmp_path / name
        path.write_text(src)
        subprocess.run([cc, std, "-Wall", "-Werror", "-Wno-address", "-I", _paths.INCLUDE_DIR, "-c", str(path), "-o", str(tmp_path / (name + ".o"))], check=True)
