"""CPU tier: include/sjgpu_cast.h -- typed getters over a column, an extension of the C-ABI with a header of its own -- declares exactly what
capi.CAST_EXPORTS lists, the library exports it, and the header stands on include/sjgpu_lists.h, include/sjgpu_rows.h, include/sjgpu_paths.h,
include/sjgpu_query.h, include/sjgpu_stream.h and include/sjgpu.h without changing them (the twin of tests/test_lists_header.py)."""
import os
import re
import subprocess

from simdjson_amd import _paths, build, capi


def test_cast_exports_match_header():
    build.build_sjgpu()
    lib = capi.load_library()
    hdr = open(os.path.join(_paths.INCLUDE_DIR, "sjgpu_cast.h")).read()
    declared = sorted(set(re.findall(r"^int (sjgpu_[a-z0-9_]+)\(", hdr, re.M)))
    assert declared == sorted(capi.CAST_EXPORTS) == ["sjgpu_cast_cells_device", "sjgpu_cell_kinds_device"]
    for name in declared:
        assert hasattr(lib, name), name
    for other in ("sjgpu.h", "sjgpu_stream.h", "sjgpu_query.h", "sjgpu_paths.h", "sjgpu_rows.h", "sjgpu_lists.h"):
        text = open(os.path.join(_paths.INCLUDE_DIR, other)).read()
        assert not any(name in text for name in declared) and "SJGPU_GET_" not in text  # declared once, in the extension
    assert not set(capi.CAST_EXPORTS) & (set(capi.EXPORTS) | set(capi.STREAM_EXPORTS) | set(capi.QUERY_EXPORTS) | set(capi.PATH_EXPORTS) | set(capi.ROWS_EXPORTS) |
                                         set(capi.LISTS_EXPORTS))
    assert '#include "sjgpu_lists.h"' in hdr
    # the getters' numbers are the header's
    enum = dict((name, int(value)) for name, value in re.findall(r"SJGPU_GET_([A-Z0-9]+) = (\d+)", hdr))
    assert enum == {name[4:]: getattr(capi, name) for name in ("GET_INT64", "GET_UINT64", "GET_DOUBLE", "GET_BOOL", "GET_STRING", "GET_ARRAY", "GET_OBJECT")}


def test_cast_header_is_plain_c(tmp_path):
    """the header compiles as C99 and as C++ on its own"""
    src = ('#include "sjgpu_cast.h"\ntypedef char getters_are_small[SJGPU_GET_INT64 == 1 && SJGPU_GET_OBJECT == 7 ? 1 : -1];\n'
           "int main(void) { return sjgpu_cast_cells_device == 0 || sjgpu_cell_kinds_device == 0 || sjgpu_at_paths_from_cells_device == 0 || "
           "sjgpu_at_pointers_from_cells_device == 0 || sjgpu_gather_strings_device == 0; }\n")
    for name, cc, std in (("t.c", "gcc", "-std=c99"), ("t.cpp", "g++", "-std=c++17")):
        path = tmp_path / name
        path.write_text(src)
        subprocess.run([cc, std, "-Wall", "-Werror", "-Wno-address", "-I", _paths.INCLUDE_DIR, "-c", str(path), "-o", str(tmp_path / (name + ".o"))], check=True)
