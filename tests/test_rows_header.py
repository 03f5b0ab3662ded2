"""CPU tier: include/sjgpu_rows.h -- record tables over device tapes, an extension of the C-ABI with a header of its own -- declares exactly what
capi.ROWS_EXPORTS lists, the library exports it, and the header stands on include/sjgpu_paths.h, include/sjgpu_query.h, include/sjgpu_stream.h and
include/sjgpu.h without changing them (the twin of tests/test_paths_header.py)."""
import os
import re
import subprocess

from simdjson_amd import _paths, build, capi


def test_rows_exports_match_header():
    build.build_sjgpu()
    lib = capi.load_library()
    hdr = open(os.path.join(_paths.INCLUDE_DIR, "sjgpu_rows.h")).read()
    declared = sorted(set(re.findall(r"^int (sjgpu_[a-z0-9_]+)\(", hdr, re.M)))
    assert declared == sorted(capi.ROWS_EXPORTS)
    for name in declared:
        assert hasattr(lib, name), name
    for other in ("sjgpu.h", "sjgpu_stream.h", "sjgpu_query.h", "sjgpu_paths.h"):
        text = open(os.path.join(_paths.INCLUDE_DIR, other)).read()
        assert not any(name in text for name in declared)  # declared once, in the extension
    assert not set(capi.ROWS_EXPORTS) & (set(capi.EXPORTS) | set(capi.STREAM_EXPORTS) | set(capi.QUERY_EXPORTS) | set(capi.PATH_EXPORTS))
    assert '#include "sjgpu_paths.h"' in hdr


def test_rows_header_is_plain_c(tmp_path):
    """the header compiles as C99 and as C++ on its own"""
    src = ('#include "sjgpu_rows.h"\ntypedef char span_is_16_bytes[sizeof(sjgpu_doc_span) == 16 ? 1 : -1];\n'
           "int main(void) { return sjgpu_at_pointers_from_cells_device == 0 || sjgpu_at_paths_device == 0 || sjgpu_gather_strings_device == 0; }\n")
    for name, cc, std in (("t.c", "gcc", "-std=c99"), ("t.cpp", "g++", "-std=c++17")):
        path = tmp_path / name
        path.write_text(src)
        subprocess.run([cc, std, "-Wall", "-Werror", "-Wno-address", "-I", _paths.INCLUDE_DIR, "-c", str(path), "-o", str(tmp_path / (name + ".o"))], check=True)
