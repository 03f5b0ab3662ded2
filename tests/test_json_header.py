"""CPU tier: include/sjgpu_json.h -- cells as JSON text, an extension of the C-ABI with a header of its own -- declares exactly what capi.JSON_EXPORTS lists, the
library exports it, and the header stands on include/sjgpu_dict.h and the headers below it without changing them (the twin of tests/test_dict_header.py)."""
import os
import re
import subprocess

from simdjson_amd import _paths, build, capi


def test_json_exports_match_header():
    build.build_sjgpu()
    lib = capi.load_library()
    hdr = open(os.path.join(_paths.INCLUDE_DIR, "sjgpu_json.h")).read()
    declared = sorted(set(re.findall(r"^int (sjgpu_[a-z0-9_]+)\(", hdr, re.M)))
    assert declared == sorted(capi.JSON_EXPORTS) == ["sjgpu_serialize_cells_device"]
    for name in declared:
        assert hasattr(lib, name), name
    for other in ("sjgpu.h", "sjgpu_stream.h", "sjgpu_query.h", "sjgpu_paths.h", "sjgpu_rows.h", "sjgpu_lists.h", "sjgpu_cast.h", "sjgpu_fields.h", "sjgpu_dict.h"):
        text = open(os.path.join(_paths.INCLUDE_DIR, other)).read()
        assert not any(name in text for name in declared)  # declared once, in the extension
    assert not set(capi.JSON_EXPORTS) & (set(capi.EXPORTS) | set(capi.STREAM_EXPORTS) | set(capi.QUERY_EXPORTS) | set(capi.PATH_EXPORTS) | set(capi.ROWS_EXPORTS) |
                                         set(capi.LISTS_EXPORTS) | set(capi.CAST_EXPORTS) | set(capi.FIELDS_EXPORTS) | set(capi.DICT_EXPORTS))
    assert '#include "sjgpu_dict.h"' in hdr
    assert lib.sjgpu_serialize_cells_device.argtypes is not None and len(lib.sjgpu_serialize_cells_device.argtypes) == 16


def test_the_bindings_are_functions_of_a_module_of_their_own():
    """tests/test_stream_order_cases.py asks every public method of the parser that takes a stream to be a key of a table that may not change: the bindings of
    this header are free functions that take the parser first"""
    import inspect

    from simdjson_amd import json_text
    for name in ("serialize_cells_device", "json_column_many", "documents_as_json_many"):
        f = getattr(json_text, name)
        assert inspect.isfunction(f) and next(iter(inspect.signature(f).parameters)) == "p" and not hasattr(capi.DomParserImplementation, name)
    assert inspect.signature(json_text.serialize_cells_device).parameters["stream"].default == 0
    assert list(inspect.signature(json_text.json_column_many).parameters) == ["p", "data", "path", "wide", "max_depth"]


def test_the_library_is_built_from_the_new_unit_and_its_headers():
    assert "sjgpu_json.hip" in build.SJGPU_SOURCES and {"sj_dtoa.h", "sj_json_text.h", "sj_pow10_table.inc"} <= set(build.SJGPU_HEADERS)


def test_json_header_is_plain_c(tmp_path):
    """the header compiles as C99 and as C++ on its own"""
    src = ('#include "sjgpu_json.h"\ntypedef char span_is_16_bytes[sizeof(sjgpu_doc_span) == 16 ? 1 : -1];\n'
           "int main(void) { return sjgpu_serialize_cells_device == 0 || sjgpu_dictionary_encode_device == 0 || sjgpu_object_fields_from_cells_device == 0 || "
           "sjgpu_gather_strings_device == 0; }\n")
    for name, cc, std in (("t.c", "gcc", "-std=c99"), ("t.cpp", "g++", "-std=c++17")):
        path = tmp_path / name
        path.write_text(src)
        subprocess.run([cc, std, "-Wall", "-Werror", "-Wno-address", "-I", _paths.INCLUDE_DIR, "-c", str(path), "-o", str(tmp_path / (name + ".o"))], check=True)
