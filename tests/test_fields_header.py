"""CPU tier: include/sjgpu_fields.h -- map columns over device tapes, an extension of the C-ABI with a header of its own -- declares exactly what
capi.FIELDS_EXPORTS lists, the library exports it, and the header stands on include/sjgpu_cast.h and the headers below it without changing them (the twin of
tests/test_lists_header.py)."""
import os
import re
import subprocess

from simdjson_amd import _paths, build, capi


def test_fields_exports_match_header():
    build.build_sjgpu()
    lib = capi.load_library()
    hdr = open(os.path.join(_paths.INCLUDE_DIR, "sjgpu_fields.h")).read()
    declared = sorted(set(re.findall(r"^int (sjgpu_[a-z0-9_]+)\(", hdr, re.M)))
    assert declared == sorted(capi.FIELDS_EXPORTS) == ["sjgpu_cell_sizes_device", "sjgpu_object_fields_from_cells_device"]
    for name in declared:
        assert hasattr(lib, name), name
    for other in ("sjgpu.h", "sjgpu_stream.h", "sjgpu_query.h", "sjgpu_paths.h", "sjgpu_rows.h", "sjgpu_lists.h", "sjgpu_cast.h"):
        text = open(os.path.join(_paths.INCLUDE_DIR, other)).read()
        assert not any(name in text for name in declared)  # declared once, in the extension
    assert not set(capi.FIELDS_EXPORTS) & (set(capi.EXPORTS) | set(capi.STREAM_EXPORTS) | set(capi.QUERY_EXPORTS) | set(capi.PATH_EXPORTS) | set(capi.ROWS_EXPORTS) |
                                           set(capi.LISTS_EXPORTS) | set(capi.CAST_EXPORTS))
    assert '#include "sjgpu_cast.h"' in hdr


def test_fields_header_is_plain_c(tmp_path):
    """the header compiles as C99 and as C++ on its own"""
    src = ('#include "sjgpu_fields.h"\ntypedef char span_is_16_bytes[sizeof(sjgpu_doc_span) == 16 ? 1 : -1];\n'
           "int main(void) { return sjgpu_object_fields_from_cells_device == 0 || sjgpu_cell_sizes_device == 0 || sjgpu_at_paths_from_cells_device == 0 || "
           "sjgpu_cast_cells_device == 0 || sjgpu_gather_strings_device == 0; }\n")
    for name, cc, std in (("t.c", "gcc", "-std=c99"), ("t.cpp", "g++", "-std=c++17")):
        path = tmp_path / name
        path.write_text(src)
        subprocess.run([cc, std, "-Wall", "-Werror", "-Wno-address", "-I", _paths.INCLUDE_DIR, "-c", str(path), "-o", str(tmp_path / (name + ".o"))], check=True)
