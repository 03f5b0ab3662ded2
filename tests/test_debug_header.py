"""CPU tier: include/sjgpu_debug.h -- the diagnostics of the single-pass workspace, an extension of the C-ABI with a header of its own -- declares exactly what
capi.DEBUG_EXPORTS lists, the library exports it, and include/sjgpu.h does not change for it: the plug-in shim and the test programs that link the reference
are built against sjgpu.h and carry its hash (oracle/ref_build.py: source_stamp), so a diagnostic must not make them stale."""
import inspect
import os
import re
import subprocess

from simdjson_amd import _paths, build, capi

OTHER_LISTS = ("EXPORTS", "STREAM_EXPORTS", "QUERY_EXPORTS", "PATH_EXPORTS", "ROWS_EXPORTS", "LISTS_EXPORTS", "CAST_EXPORTS", "FIELDS_EXPORTS", "DICT_EXPORTS",
               "JSON_EXPORTS", "WRITE_EXPORTS", "NESTED_EXPORTS")


def test_debug_exports_match_header():
    build.build_sjgpu()
    lib = capi.load_library()
    hdr = open(os.path.join(_paths.INCLUDE_DIR, "sjgpu_debug.h")).read()
    declared = sorted(set(re.findall(r"^(?:int|uint64_t) (sjgpu_[a-z0-9_]+)\(", hdr, re.M)))
    assert declared == sorted(capi.DEBUG_EXPORTS) == ["sjgpu_debug_gave_up_count", "sjgpu_debug_read_workspace"]
    for name in declared:
        assert hasattr(lib, name), name
    for other in sorted(f for f in os.listdir(_paths.INCLUDE_DIR) if f.endswith(".h") and f != "sjgpu_debug.h"):
        text = open(os.path.join(_paths.INCLUDE_DIR, other)).read()
        assert not any(name in text for name in declared), other  # declared once, in the extension
    for other in OTHER_LISTS:
        assert not set(capi.DEBUG_EXPORTS) & set(getattr(capi, other)), other
    assert '#include "sjgpu.h"' in hdr
    assert len(lib.sjgpu_debug_read_workspace.argtypes) == 5 and len(lib.sjgpu_debug_gave_up_count.argtypes) == 1


def test_the_library_is_stamped_with_the_header_and_the_test_programs_are_not():
    import ref_build  # (oracle/ is on the path once simdjson_amd.build is imported)
    assert "sjgpu_debug.h" not in {os.path.basename(f) for f in ref_build._stamp_sources()}
    assert "sjgpu_debug.h" in inspect.getsource(build.sjgpu_source_stamp)


def test_the_bindings_take_no_stream():
    """tests/test_stream_order_cases.py pins the table of parser methods that take a stream: these two are synchronous and take none"""
    for name in ("read_workspace", "gave_up_count"):
        assert list(inspect.signature(getattr(capi.DomParserImplementation, name)).parameters) == ["self"], name


def test_debug_header_is_plain_c(tmp_path):
    """the header compiles as C99 and as C++ on its own"""
    src = '#include "sjgpu_debug.h"\nint main(void) { return sjgpu_debug_read_workspace == 0 || sjgpu_debug_gave_up_count == 0 || sjgpu_result == 0; }\n'
    for name, cc, std in (("t.c", "gcc", "-std=c99"), ("t.cpp", "g++", "-std=c++17")):
        path = tmp_path / name
        path.write_text(src)
        subprocess.run([cc, std, "-Wall", "-Werror", "-Wno-address", "-I", _paths.INCLUDE_DIR, "-c", str(path), "-o", str(tmp_path / (name + ".o"))], check=True)
