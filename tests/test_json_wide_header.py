"""CPU tier: include/sjgpu_json_wide.h -- cells as JSON text with one lane per tape word, an extension of the C-ABI with a header of its own -- declares exactly what
capi.JSON_WIDE_EXPORTS lists, the library exports it, and the header stands on include/sjgpu_json.h without changing it (the twin of tests/test_json_header.py)."""
import inspect
import os
import re
import subprocess

from simdjson_amd import _paths, build, capi


def test_json_wide_exports_match_header():
    build.build_sjgpu()
    lib = capi.load_library()
    hdr = open(os.path.join(_paths.INCLUDE_DIR, "sjgpu_json_wide.h")).read()
    declared = sorted(set(re.findall(r"^int (sjgpu_[a-z0-9_]+)\(", hdr, re.M)))
    assert declared == sorted(capi.JSON_WIDE_EXPORTS) == ["sjgpu_serialize_cells_wide_device"]
    for name in declared:
        assert hasattr(lib, name), name
    for other in sorted(f for f in os.listdir(_paths.INCLUDE_DIR) if f.endswith(".h") and f != "sjgpu_json_wide.h"):
        text = open(os.path.join(_paths.INCLUDE_DIR, other)).read()
        assert not any(name in text for name in declared), other  # declared once, in the extension
    for other in ("EXPORTS", "STREAM_EXPORTS", "QUERY_EXPORTS", "PATH_EXPORTS", "ROWS_EXPORTS", "LISTS_EXPORTS", "CAST_EXPORTS", "FIELDS_EXPORTS", "DICT_EXPORTS", "JSON_EXPORTS",
                  "WRITE_EXPORTS", "NESTED_EXPORTS", "DEBUG_EXPORTS"):
        assert not set(capi.JSON_WIDE_EXPORTS) & set(getattr(capi, other)), other
    assert '#include "sjgpu_json.h"' in hdr
    assert len(lib.sjgpu_serialize_cells_wide_device.argtypes) == 16
    assert list(lib.sjgpu_serialize_cells_wide_device.argtypes) == list(lib.sjgpu_serialize_cells_device.argtypes)
    assert re.search(r"#define SJGPU_E_RANGE \(-8\)", hdr) and capi.SJGPU_E_RANGE == -8


def test_the_two_declarations_have_the_same_parameters():
    """the sixteen parameters of the narrow call, in its order"""
    def params(path, name):
        text = open(os.path.join(_paths.INCLUDE_DIR, path)).read()
        body = re.search(r"^int " + name + r"\((.*?)\);", text, re.M | re.S).group(1)
        return [re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", a)).strip() for a in body.split(",")]
    narrow, wide = params("sjgpu_json.h", "sjgpu_serialize_cells_device"), params("sjgpu_json_wide.h", "sjgpu_serialize_cells_wide_device")
    assert narrow == wide and len(wide) == 16


def test_the_header_says_what_the_call_costs():
    hdr = re.sub(r"\s+", " ", open(os.path.join(_paths.INCLUDE_DIR, "sjgpu_json_wide.h")).read().replace(" * ", " "))
    for said in ("10 bytes per slot", "WAITS FOR THE STREAM TWICE", "A STRING IS STILL ONE LANE'S WORK", "WHICH CALL TO TAKE IS THE CALLER'S DECISION", "0xFFFFFFF0",
                 "sjgpu_serialize_cells_device, or split the row"):
        assert said in hdr, said


def test_the_bindings_are_functions_of_a_module_of_their_own():
    from simdjson_amd import json_text, json_text_wide
    for name, twin in (("serialize_cells_wide_device", "serialize_cells_device"), ("json_column_wide_many", "json_column_many"),
                       ("documents_as_json_wide_many", "documents_as_json_many")):
        f = getattr(json_text_wide, name)
        assert inspect.isfunction(f) and next(iter(inspect.signature(f).parameters)) == "p" and not hasattr(capi.DomParserImplementation, name)
        assert list(inspect.signature(f).parameters) == list(inspect.signature(getattr(json_text, twin)).parameters), name
    assert inspect.signature(json_text_wide.serialize_cells_wide_device).parameters["stream"].default == 0


def test_the_library_is_built_from_the_new_unit_and_its_headers():
    assert "sjgpu_json_wide.hip" in build.SJGPU_SOURCES and "sj_json_walk.h" in build.SJGPU_HEADERS
    assert "sjgpu_json_wide.h" in inspect.getsource(build.sjgpu_source_stamp)


def test_json_wide_header_is_plain_c(tmp_path):
    """the header compiles as C99 and as C++ on its own"""
    src = ('#include "sjgpu_json_wide.h"\ntypedef char range_is_minus_8[SJGPU_E_RANGE == -8 ? 1 : -1];\n'
           "int main(void) { return sjgpu_serialize_cells_wide_device == 0 || sjgpu_serialize_cells_device == 0 || sjgpu_dictionary_encode_device == 0; }\n")
    for name, cc, std in (("t.c", "gcc", "-std=c99"), ("t.cpp", "g++", "-std=c++17")):
        path = tmp_path / name
        path.write_text(src)
        subprocess.run([cc, std, "-Wall", "-Werror", "-Wno-address", "-I", _paths.INCLUDE_DIR, "-c", str(path), "-o", str(tmp_path / (name + ".o"))], check=True)
