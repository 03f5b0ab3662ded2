"""CPU tier: include/sjgpu_stream.h -- the document-stream extension of the C-ABI -- declares exactly what capi.STREAM_EXPORTS lists, the library
exports it, and the header stands on include/sjgpu.h without changing it: the programs built against sjgpu.h alone (the plug-in shim, the test
programs linked with it: oracle/ref_build.py stamps them by that header) need no rebuild for the extension."""
import os
import re
import subprocess

from simdjson_amd import _paths, build, capi


def test_stream_exports_match_header():
    build.build_sjgpu()
    lib = capi.load_library()
    hdr = open(os.path.join(_paths.INCLUDE_DIR, "sjgpu_stream.h")).read()
    declared = sorted(set(re.findall(r"^int (sjgpu_[a-z0-9_]+)\(", hdr, re.M)))  # (the comments name functions of sjgpu.h too)
    assert declared == sorted(capi.STREAM_EXPORTS)
    for name in declared:
        assert hasattr(lib, name), name
    base = open(os.path.join(_paths.INCLUDE_DIR, "sjgpu.h")).read()
    assert not any(name in base for name in declared)  # declared once, in the extension


def test_stream_header_is_plain_c(tmp_path):
    """the header compiles as C99 and as C++ on its own, and sjgpu_doc_span is the four words the kernels write (16 bytes)"""
    src = '#include "sjgpu_stream.h"\ntypedef char span_is_16_bytes[sizeof(sjgpu_doc_span) == 16 ? 1 : -1];\nint main(void) { return 0; }\n'
    for name, cc, std in (("t.c", "gcc", "-std=c99"), ("t.cpp", "g++", "-std=c++17")):
        path = tmp_path / name
        path.write_text(src)
        subprocess.run([cc, std, "-Wall", "-Werror", "-I", _paths.INCLUDE_DIR, "-c", str(path), "-o", str(tmp_path / (name + ".o"))], check=True)
