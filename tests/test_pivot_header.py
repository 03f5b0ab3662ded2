"""CPU tier: include/sjgpu_pivot.h -- a map column pivoted into a record table, an extension of the C-ABI with a header of its own -- declares exactly what
capi.PIVOT_EXPORTS lists, the library exports it, and the header stands on include/sjgpu_dict.h and the headers below it without changing them (the twin of
tests/test_dict_header.py)."""
import inspect
import os
import re
import subprocess

from simdjson_amd import _paths, build, capi

OTHER_LISTS = ("EXPORTS", "STREAM_EXPORTS", "QUERY_EXPORTS", "PATH_EXPORTS", "ROWS_EXPORTS", "LISTS_EXPORTS", "CAST_EXPORTS", "CAST_STRINGS_EXPORTS", "FIELDS_EXPORTS",
               "DICT_EXPORTS", "JSON_EXPORTS", "JSON_WIDE_EXPORTS", "PRETTY_EXPORTS", "WRITE_EXPORTS", "NESTED_EXPORTS")


def test_pivot_exports_match_header():
    build.build_sjgpu()
    lib = capi.load_library()
    hdr = open(os.path.join(_paths.INCLUDE_DIR, "sjgpu_pivot.h")).read()
    declared = sorted(set(re.findall(r"^int (sjgpu_[a-z0-9_]+)\(", hdr, re.M)))
    assert declared == sorted(capi.PIVOT_EXPORTS) == ["sjgpu_pivot_fields_device"]
    for name in declared:
        assert hasattr(lib, name), name
    for other in sorted(f for f in os.listdir(_paths.INCLUDE_DIR) if f.endswith(".h") and f != "sjgpu_pivot.h"):
        text = open(os.path.join(_paths.INCLUDE_DIR, other)).read()
        assert not any(name in text for name in declared), other  # declared once, in the extension
    for other in OTHER_LISTS:
        assert not set(capi.PIVOT_EXPORTS) & set(getattr(capi, other)), other
    assert '#include "sjgpu_dict.h"' in hdr and "Cost, not hidden" in hdr
    assert len(lib.sjgpu_pivot_fields_device.argtypes) == 14
    assert "sjgpu_pivot.h" in inspect.getsource(build.sjgpu_source_stamp) and "sjgpu_pivot.hip" in build.SJGPU_SOURCES


def test_the_bindings_are_functions_of_a_module_of_their_own():
    """tests/test_stream_order_cases.py asks every public method of the parser that takes a stream to be a key of a table that may not change: the bindings of
    this header are free functions that take the parser first"""
    from simdjson_amd import pivot
    for name in ("pivot_fields_device", "records_many"):
        f = getattr(pivot, name)
        assert inspect.isfunction(f) and next(iter(inspect.signature(f).parameters)) == "p" and not hasattr(capi.DomParserImplementation, name)
    assert inspect.signature(pivot.pivot_fields_device).parameters["stream"].default == 0
    assert list(inspect.signature(pivot.records_many).parameters) == ["p", "data", "row_path", "keys", "min_count", "fold_case", "wide", "max_depth"]


def test_pivot_header_is_plain_c(tmp_path):
    """the header compiles as C99 and as C++ on its own"""
    src = ('#include "sjgpu_pivot.h"\ntypedef char internal_is_negative[SJGPU_E_INTERNAL < 0 ? 1 : -1];\n'
           "int main(void) { return sjgpu_pivot_fields_device == 0 || sjgpu_dictionary_encode_device == 0 || sjgpu_object_fields_from_cells_device == 0 || "
           "sjgpu_cell_kinds_device == 0; }\n")
    for name, cc, std in (("t.c", "gcc", "-std=c99"), ("t.cpp", "g++", "-std=c++17")):
        path = tmp_path / name
        path.write_text(src)
        subprocess.run([cc, std, "-Wall", "-Werror", "-Wno-address", "-I", _paths.INCLUDE_DIR, "-c", str(path), "-o", str(tmp_path / (name + ".o"))], check=True)
