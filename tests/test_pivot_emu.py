"""CPU tier: a map column pivoted into a record table -- the gfx950 kernel source sjgpu_pivot.hip, compiled as C++ against tests/host/emu -- runs the launches of
sjgpu_pivot_fields_device (tests/host/test_pivot_emu.cpp) and is compared cell for cell with tests/pivot_model.py: rows at the wave's and the workgroup's edges
times columns on both sides of the cast's chunk of 64, rows without fields, every slot of a row on one column, one row of 70 000 slots over 300 codes, codes of
-1, `groups` and beyond, a map with -1, with `columns` and beyond and with two and three codes on one column, the NULL map, every status, a slice that runs
backwards and one that ends beyond `fields`.  The outputs have exactly their size inside 0x5A guards at both alignments of the words, and every call runs twice
with identical bytes (the driver checks both).  The driver also runs built with -fsanitize=address,undefined: a stand-alone program, nothing preloaded."""
import os
import struct
import subprocess

import numpy as np
import pytest

import pivot_cases
import pivot_model
from simdjson_amd import _paths

CSRC = os.path.join(_paths.PKG_DIR, "csrc")
EMU = os.path.join(_paths.REPO_ROOT, "tests", "host", "emu")


def build(out, sanitize=()):
    """the way tests/test_dict_emu.py builds its units"""
    inc = ["-I", EMU, "-I", _paths.INCLUDE_DIR, "-I", CSRC]
    jobs = [subprocess.Popen(["g++", "-std=c++17", "-O2", *sanitize, "-Wno-attributes", "-Wno-unknown-pragmas", "-x", "c++", *inc, "-c", os.path.join(CSRC, "sjgpu_pivot.hip"),
                              "-o", str(out / "sjgpu_pivot.o")]),
            subprocess.Popen(["g++", "-std=c++17", "-O2", *sanitize, *inc, "-c", os.path.join(EMU, "sj_emu.cpp"), "-o", str(out / "sj_emu.o")]),
            subprocess.Popen(["g++", "-std=c++17", "-O2", *sanitize, "-Wno-attributes", *inc, "-c", os.path.join(_paths.REPO_ROOT, "tests", "host", "test_pivot_emu.cpp"),
                              "-o", str(out / "driver.o")])]
    assert all(j.wait() == 0 for j in jobs)
    exe = str(out / "test_pivot_emu")
    subprocess.run(["g++", *sanitize, *[str(out / (f + ".o")) for f in ("sjgpu_pivot", "sj_emu", "driver")], "-lpthread", "-o", exe], check=True)
    return exe


def blob_of(c, skew):
    return (struct.pack("<6I", len(c["status"]), c["fields"], c["groups"], c["columns"], c["map"] is not None, skew) + c["offsets"].tobytes() + c["status"].tobytes() +
            c["codes"].tobytes() + c["values"].tobytes() + c["tags"].tobytes() + (b"" if c["map"] is None else c["map"].tobytes()))


def check(out, cases):
    """the driver's records against the model, cell for cell"""
    at = 0
    for c in cases:
        rows, columns = len(c["status"]), c["columns"]
        cells = rows * columns
        code, = struct.unpack_from("<i", out, at)
        tags = np.frombuffer(out, np.uint8, cells, at + 4).reshape(columns, rows)
        values = np.frombuffer(out, np.uint64, cells, at + 4 + cells).reshape(columns, rows)
        at += 4 + 9 * cells
        want_tags, want_values = pivot_model.pivot(c["offsets"], c["status"], c["codes"], c["values"], c["tags"], c["fields"], c["map"], c["groups"], columns)
        assert code == 0 and np.array_equal(tags, want_tags) and np.array_equal(values, want_values), (rows, columns, c["groups"])
    assert at == len(out)


def run(exe, cases, env=None):
    """every case at both alignments of the output words"""
    twice = [c for c in cases for _ in (0, 1)]
    p = subprocess.run([exe], input=b"".join(blob_of(c, k & 1) for k, c in enumerate(twice)), capture_output=True, timeout=1500, env=env)
    assert p.returncode == 0 and b"runtime error" not in p.stderr and b"AddressSanitizer" not in p.stderr, p.stderr.decode(errors="replace")[-3000:]
    check(p.stdout, twice)


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return build(tmp_path_factory.mktemp("pivot_emu"))


def test_rows_times_columns(emu):
    cases = pivot_cases.shapes()
    assert len(cases) == len(pivot_cases.ROWS) * len(pivot_cases.COLUMNS)
    run(emu, cases)


@pytest.mark.parametrize("name", list(pivot_cases.special()))
def test_special_cases(emu, name):
    c = pivot_cases.special()[name]
    run(emu, [c])
    tags, values = pivot_model.pivot(c["offsets"], c["status"], c["codes"], c["values"], c["tags"], c["fields"], c["map"], c["groups"], c["columns"])
    if name == "statuses":
        assert tags.T.tolist()[1:5] == [[17] * 3, [19] * 3, [20] * 3, [22] * 3] and tags[0, 0] != 20 and tags[1, 5] != 20 and not values[:, 1:5].any()
    if name in ("a slice that runs backwards", "a slice that ends beyond fields"):
        assert (tags[:, 1] == 20).all() and not values[:, 1].any() and (tags[:, 0] != 20).all()
    if name == "every slot on one column":
        first = c["offsets"][:-1]
        assert np.array_equal(values[2], c["values"][first]) and (tags[[0, 1, 3]] == 20).all()
    if name == "one row of 70 000 slots":
        assert (tags[:, 1] != 20).all() and values[7, 0] == c["values"][0]


def test_the_driver_runs_clean_under_the_sanitizers(tmp_path):
    """the stand-alone driver -- kernels and launcher -- built with -fsanitize=address,undefined: the inputs are heap blocks of their exact size, so a slot read
    from a slice that ends beyond `fields` is an error here"""
    exe = build(tmp_path, ("-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer", "-g"))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    special = pivot_cases.special()
    cases = [c for name, c in special.items() if name != "one row of 70 000 slots"] + [c for c in pivot_cases.shapes() if len(c["status"]) in (1, 65, 257) and c["columns"] in (1, 65)]
    run(exe, cases, env)
