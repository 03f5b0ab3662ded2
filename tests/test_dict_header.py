"""CPU tier: include/sjgpu_dict.h -- dictionaries over device cells, an extension of the C-ABI with a header of its own -- declares exactly what
capi.DICT_EXPORTS lists, the library exports it, and the header stands on include/sjgpu_fields.h and the headers below it without changing them (the twin of
tests/test_fields_header.py)."""
import os
import re
import subprocess

from simdjson_amd import _paths, build, capi


def test_dict_exports_match_header():
    build.build_sjgpu()
    lib = capi.load_library()
    hdr = open(os.path.join(_paths.INCLUDE_DIR, "sjgpu_dict.h")).read()
    declared = sorted(set(re.findall(r"^int (sjgpu_[a-z0-9_]+)\(", hdr, re.M)))
    assert declared == sorted(capi.DICT_EXPORTS) == ["sjgpu_cell_kinds_by_code_device", "sjgpu_dictionary_encode_device"]
    for name in declared:
        assert hasattr(lib, name), name
    for other in ("sjgpu.h", "sjgpu_stream.h", "sjgpu_query.h", "sjgpu_paths.h", "sjgpu_rows.h", "sjgpu_lists.h", "sjgpu_cast.h", "sjgpu_fields.h"):
        text = open(os.path.join(_paths.INCLUDE_DIR, other)).read()
        assert not any(name in text for name in declared)  # declared once, in the extension
    assert not set(capi.DICT_EXPORTS) & (set(capi.EXPORTS) | set(capi.STREAM_EXPORTS) | set(capi.QUERY_EXPORTS) | set(capi.PATH_EXPORTS) | set(capi.ROWS_EXPORTS) |
                                         set(capi.LISTS_EXPORTS) | set(capi.CAST_EXPORTS) | set(capi.FIELDS_EXPORTS))
    assert '#include "sjgpu_fields.h"' in hdr
    assert int(re.search(r"#define SJGPU_E_INTERNAL \((-\d+)\)", hdr).group(1)) == capi.SJGPU_E_INTERNAL
    codes = [int(c) for other in ("sjgpu.h",) for c in re.findall(r"#define SJGPU_E_[A-Z_]+ +\((-\d+)\)", open(os.path.join(_paths.INCLUDE_DIR, other)).read())]
    assert codes and capi.SJGPU_E_INTERNAL not in codes  # a code of its own


def test_the_bindings_are_functions_of_a_module_of_their_own():
    """tests/test_stream_order_cases.py asks every public method of the parser that takes a stream to be a key of a table that may not change: the bindings of
    this header are free functions that take the parser first"""
    import inspect

    from simdjson_amd import dictionary
    for name in ("dictionary_encode_device", "kinds_by_code_device", "dictionary_many", "schema_many"):
        f = getattr(dictionary, name)
        assert inspect.isfunction(f) and next(iter(inspect.signature(f).parameters)) == "p" and not hasattr(capi.DomParserImplementation, name)
    for name in ("dictionary_encode_device", "kinds_by_code_device"):
        assert inspect.signature(getattr(dictionary, name)).parameters["stream"].default == 0


def test_dict_header_is_plain_c(tmp_path):
    """the header compiles as C99 and as C++ on its own"""
    src = ('#include "sjgpu_dict.h"\ntypedef char span_is_16_bytes[sizeof(sjgpu_doc_span) == 16 ? 1 : -1];\ntypedef char internal_is_negative[SJGPU_E_INTERNAL < 0 ? 1 : -1];\n'
           "int main(void) { return sjgpu_dictionary_encode_device == 0 || sjgpu_cell_kinds_by_code_device == 0 || sjgpu_object_fields_from_cells_device == 0 || "
           "sjgpu_cell_kinds_device == 0 || sjgpu_gather_strings_device == 0; }\n")
    for name, cc, std in (("t.c", "gcc", "-std=c99"), ("t.cpp", "g++", "-std=c++17")):
        path = tmp_path / name
        path.write_text(src)
        subprocess.run([cc, std, "-Wall", "-Werror", "-Wno-address", "-I", _paths.INCLUDE_DIR, "-c", str(path), "-o", str(tmp_path / (name + ".o"))], check=True)
