"""CPU tier: include/sjgpu_pretty.h -- cells as indented JSON text, an extension of the C-ABI with a header of its own -- declares exactly what capi.PRETTY_EXPORTS
lists, the library exports it, and the header stands on include/sjgpu_json_wide.h without changing it (the twin of tests/test_json_wide_header.py)."""
import inspect
import os
import re
import subprocess

from simdjson_amd import _paths, build, capi

NAMES = ["sjgpu_prettify_cells_device", "sjgpu_prettify_cells_wide_device"]


def test_pretty_exports_match_header():
    build.build_sjgpu()
    lib = capi.load_library()
    hdr = open(os.path.join(_paths.INCLUDE_DIR, "sjgpu_pretty.h")).read()
    declared = sorted(set(re.findall(r"^int (sjgpu_[a-z0-9_]+)\(", hdr, re.M)))
    assert declared == sorted(capi.PRETTY_EXPORTS) == NAMES
    for name in declared:
        assert hasattr(lib, name), name
        assert list(getattr(lib, name).argtypes) == list(lib.sjgpu_serialize_cells_device.argtypes) and len(getattr(lib, name).argtypes) == 16
    for other in sorted(f for f in os.listdir(_paths.INCLUDE_DIR) if f.endswith(".h") and f != "sjgpu_pretty.h"):
        text = open(os.path.join(_paths.INCLUDE_DIR, other)).read()
        assert not any(name in text for name in declared), other  # declared once, in the extension
    for other in ("EXPORTS", "STREAM_EXPORTS", "QUERY_EXPORTS", "PATH_EXPORTS", "ROWS_EXPORTS", "LISTS_EXPORTS", "CAST_EXPORTS", "FIELDS_EXPORTS", "DICT_EXPORTS", "JSON_EXPORTS",
                  "JSON_WIDE_EXPORTS", "WRITE_EXPORTS", "NESTED_EXPORTS", "DEBUG_EXPORTS"):
        assert not set(capi.PRETTY_EXPORTS) & set(getattr(capi, other)), other
    assert '#include "sjgpu_json_wide.h"' in hdr


def test_the_declarations_have_the_narrow_calls_parameters():
    """the sixteen parameters of sjgpu_serialize_cells_device, in its order"""
    def params(path, name):
        text = open(os.path.join(_paths.INCLUDE_DIR, path)).read()
        body = re.search(r"^int " + name + r"\((.*?)\);", text, re.M | re.S).group(1)
        return [re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", a)).strip() for a in body.split(",")]
    narrow = params("sjgpu_json.h", "sjgpu_serialize_cells_device")
    for name in NAMES:
        assert params("sjgpu_pretty.h", name) == narrow and len(narrow) == 16, name


def test_the_header_says_what_the_text_is_and_what_the_calls_cost():
    hdr = re.sub(r"\s+", " ", open(os.path.join(_paths.INCLUDE_DIR, "sjgpu_pretty.h")).read().replace(" * ", " "))
    for said in ("simdjson::prettify(e)", "l = a mod 16", "The indent step is 4", "a container with l = 15", "FLAT", "WITHOUT the blank", "ENDS WITH A \\n OF ITS OWN",
                 "ends with ONE \\n", "A refused cell has length 0 and no newline", "ITS CONTRACT, WORD FOR WORD", "SJGPU_E_RANGE", "bit for bit",
                 "Nothing grows", "10 bytes per slot", "A STRING IS STILL ONE LANE'S WORK", "WHICH CALL TO TAKE IS THE CALLER'S DECISION", "profiles/pretty_text.txt"):
        assert said in hdr, said


def test_the_bindings_are_functions_of_a_module_of_their_own():
    from simdjson_amd import json_text, pretty_text
    for name in ("prettify_cells_device", "prettify_cells_wide_device"):
        f = getattr(pretty_text, name)
        assert inspect.isfunction(f) and not hasattr(capi.DomParserImplementation, name)
        assert list(inspect.signature(f).parameters) == list(inspect.signature(json_text.serialize_cells_device).parameters), name
        assert inspect.signature(f).parameters["stream"].default == 0
    assert list(inspect.signature(pretty_text.pretty_column_many).parameters)[:5] == ["p", "data", "path", "wide", "one_lane_per_word"]
    assert list(inspect.signature(pretty_text.documents_as_pretty_many).parameters)[:3] == ["p", "data", "one_lane_per_word"]
    assert inspect.signature(pretty_text.pretty_column_many).parameters["one_lane_per_word"].default is False


def test_the_library_is_built_from_the_header():
    assert "sjgpu_pretty.h" in inspect.getsource(build.sjgpu_source_stamp) and "sj_json_walk.h" in build.SJGPU_HEADERS


def test_pretty_header_is_plain_c(tmp_path):
    """the header compiles as C99 and as C++ on its own"""
    src = ('#include "sjgpu_pretty.h"\ntypedef char range_is_minus_8[SJGPU_E_RANGE == -8 ? 1 : -1];\n'
           "int main(void) { return sjgpu_prettify_cells_device == 0 || sjgpu_prettify_cells_wide_device == 0 || sjgpu_serialize_cells_device == 0; }\n")
    for name, cc, std in (("t.c", "gcc", "-std=c99"), ("t.cpp", "g++", "-std=c++17")):
        path = tmp_path / name
        path.write_text(src)
        subprocess.run([cc, std, "-Wall", "-Werror", "-Wno-address", "-I", _paths.INCLUDE_DIR, "-c", str(path), "-o", str(tmp_path / (name + ".o"))], check=True)
