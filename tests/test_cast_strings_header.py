"""CPU tier: include/sjgpu_cast_strings.h -- numbers held in strings, an extension of the C-ABI with a header of its own -- declares exactly what
capi.CAST_STRINGS_EXPORTS lists, the library exports it, and the header stands on include/sjgpu_cast.h and the headers below it without changing them (the twin of
tests/test_cast_header.py)."""
import inspect
import os
import re
import subprocess

from simdjson_amd import _paths, build, capi

OTHER_LISTS = ("EXPORTS", "STREAM_EXPORTS", "QUERY_EXPORTS", "PATH_EXPORTS", "ROWS_EXPORTS", "LISTS_EXPORTS", "CAST_EXPORTS", "FIELDS_EXPORTS", "DICT_EXPORTS", "JSON_EXPORTS",
               "JSON_WIDE_EXPORTS", "PRETTY_EXPORTS", "WRITE_EXPORTS", "NESTED_EXPORTS", "DEBUG_EXPORTS")


def test_cast_strings_exports_match_header():
    build.build_sjgpu()
    lib = capi.load_library()
    hdr = open(os.path.join(_paths.INCLUDE_DIR, "sjgpu_cast_strings.h")).read()
    declared = sorted(set(re.findall(r"^int (sjgpu_[a-z0-9_]+)\(", hdr, re.M)))
    assert declared == sorted(capi.CAST_STRINGS_EXPORTS) == ["sjgpu_cast_string_cells_device"]
    assert hasattr(lib, declared[0]) and len(lib.sjgpu_cast_string_cells_device.argtypes) == 13
    for other in sorted(f for f in os.listdir(_paths.INCLUDE_DIR) if f.endswith(".h") and f != "sjgpu_cast_strings.h"):
        text = open(os.path.join(_paths.INCLUDE_DIR, other)).read()
        assert declared[0] not in text and "SJGPU_GETS_" not in text and "sjgpu_cast_strings.h" not in text, other  # declared once, in the extension; no older header names it
    for other in OTHER_LISTS:
        assert not set(capi.CAST_STRINGS_EXPORTS) & set(getattr(capi, other)), other
    assert '#include "sjgpu_cast.h"' in hdr
    # the getters' numbers are the header's
    enum = dict((name, int(value, 0)) for name, value in re.findall(r"SJGPU_GETS_([A-Z0-9_]+) = (0x[0-9A-Fa-f]+|\d+)", hdr))
    assert enum == {"INT64": capi.GETS_INT64, "UINT64": capi.GETS_UINT64, "DOUBLE": capi.GETS_DOUBLE, "OR_NUMBER": capi.GETS_OR_NUMBER} == {"INT64": 1, "UINT64": 2, "DOUBLE": 3,
                                                                                                                                   "OR_NUMBER": 0x10}
    # what the header promises to say
    for words in ("On-Demand", "get_float_in_string", "utf8", "transactions", "an accident"):
        assert words in hdr, words


def test_the_library_is_built_from_the_new_files():
    assert "sjgpu_cast_strings.hip" in build.SJGPU_SOURCES and "sj_number_in_string.h" in build.SJGPU_HEADERS
    assert "sjgpu_cast_strings.h" in inspect.getsource(build.sjgpu_source_stamp)


def test_cast_strings_header_is_plain_c(tmp_path):
    """the header compiles as C99 and as C++ on its own"""
    src = ('#include "sjgpu_cast_strings.h"\ntypedef char getters_are_small[SJGPU_GETS_INT64 == 1 && SJGPU_GETS_DOUBLE == 3 && SJGPU_GETS_OR_NUMBER == 16 ? 1 : -1];\n'
           "int main(void) { return sjgpu_cast_string_cells_device == 0 || sjgpu_cast_cells_device == 0 || sjgpu_gather_strings_device == 0; }\n")
    for name, cc, std in (("t.c", "gcc", "-std=c99"), ("t.cpp", "g++", "-std=c++17")):
        path = tmp_path / name
        path.write_text(src)
        subprocess.run([cc, std, "-Wall", "-Werror", "-Wno-address", "-I", _paths.INCLUDE_DIR, "-c", str(path), "-o", str(tmp_path / (name + ".o"))], check=True)
