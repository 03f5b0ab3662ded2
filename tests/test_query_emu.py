"""CPU tier: the queries over tapes -- the gfx950 kernel sources of sjgpu_query.hip and the scans of sjgpu_finish.hip, compiled as C++ against
tests/host/emu -- run the launches of sjgpu_at_pointers_device and sjgpu_gather_strings_device (tests/host/test_query_emu.cpp) over tapes the
oracle built document by document, laid out as the document table says, and are compared cell by cell with tests/pointer_model.py: the fixture's
documents as one stream, thousands of small records, and one long level."""
import os
import struct
import subprocess

import numpy as np
import pytest

import checkers
import pointer_model
import query_cases
import stream_cases
from simdjson_amd import _paths

CSRC = os.path.join(_paths.PKG_DIR, "csrc")
EMU = os.path.join(_paths.REPO_ROOT, "tests", "host", "emu")
KERNEL_TUS = ("sjgpu_query", "sjgpu_finish")


def build(out):
    """the way tests/test_tape_many_emu.py builds its units"""
    inc = ["-I", EMU, "-I", _paths.INCLUDE_DIR, "-I", CSRC]
    jobs = []
    for name in KERNEL_TUS:
        jobs.append(subprocess.Popen(["g++", "-std=c++17", "-O1", "-Wno-attributes", "-Wno-unknown-pragmas", "-x", "c++", *inc, "-c",
                                      os.path.join(CSRC, name + ".hip"), "-o", str(out / (name + ".o"))]))
    jobs.append(subprocess.Popen(["g++", "-std=c++17", "-O2", *inc, "-c", os.path.join(EMU, "sj_emu.cpp"), "-o", str(out / "sj_emu.o")]))
    jobs.append(subprocess.Popen(["g++", "-std=c++17", "-O2", "-Wno-attributes", *inc, "-c",
                                  os.path.join(_paths.REPO_ROOT, "tests", "host", "test_query_emu.cpp"), "-o", str(out / "driver.o")]))
    assert all(j.wait() == 0 for j in jobs)
    exe = str(out / "test_query_emu")
    subprocess.run(["g++", *[str(out / (f + ".o")) for f in (*KERNEL_TUS, "sj_emu", "driver")], "-lpthread", "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def orc():
    return checkers.Oracle()


@pytest.fixture(scope="module")
def emu(tmp_path_factory, orc):
    exe = build(tmp_path_factory.mktemp("query_emu"))

    def run(docs, pointers):
        """-> the parsed documents; everything the driver wrote is compared with the model here"""
        parsed = []
        for d in docs:
            err, tape, sbuf = orc.dom_parse(d)
            assert err == 0, d[:100]
            parsed.append((tape, sbuf))
        tape, sbuf, table = query_cases.lay_out(parsed)
        lens = np.array([len(p) for p in pointers], np.uint32)
        blob = (struct.pack("<IQQ", len(docs), len(tape), len(sbuf)) + tape.tobytes() + sbuf.tobytes() + table.tobytes() + struct.pack("<I", len(pointers)) + lens.tobytes() +
                b"".join(pointers))
        p = subprocess.run([exe], input=blob, capture_output=True, timeout=1500)
        assert p.returncode == 0, p.stderr.decode(errors="replace")[-3000:]
        out, n, K = p.stdout, len(docs), len(pointers)
        tags = np.frombuffer(out, np.uint8, K * n).reshape(K, n)
        values = np.frombuffer(out, np.uint64, K * n, K * n).reshape(K, n)
        want_tags, want_values = pointer_model.columns(parsed, pointers)
        assert np.array_equal(tags, want_tags), np.argwhere(tags != want_tags)[:5]
        assert np.array_equal(values, want_values), np.argwhere(values != want_values)[:5]
        query_cases.check_container_cells(tags, values, tape, table)
        at = 9 * K * n
        for k in range(K):
            strings = [pointer_model.string_of(sbuf, int(values[k, d])) if tags[k, d] == ord('"') else b"" for d in range(n)]
            total = struct.unpack_from("<Q", out, at)[0]
            offsets = np.frombuffer(out, np.uint32, n + 1, at + 8)
            chars = out[at + 8 + 4 * (n + 1): at + 8 + 4 * (n + 1) + total]
            at += 8 + 4 * (n + 1) + total
            assert total == sum(len(s) for s in strings), (k, total)
            assert np.array_equal(offsets, np.concatenate([[0], np.cumsum([len(s) for s in strings])]).astype(np.uint32)), k
            assert chars == b"".join(strings), k
        assert at == len(out)
        return tags
    return run


def test_the_fixture_as_one_stream(emu):
    docs, pointers, cells = query_cases.fixture()
    for first in range(0, len(pointers), 64):  # K <= 64 per call
        emu(docs, pointers[first: first + 64])
    assert emu(docs[:3], []).size == 0


def test_six_thousand_small_records(emu):
    rng = np.random.default_rng(51)
    tags = emu(stream_cases.small_records(rng, 6000), query_cases.SMALL_RECORD_POINTERS)
    hits = (tags >= 34).sum(axis=1)
    assert (hits[[0, 1, 2, 3, 4, 5, 6, 7]] > 500).all() and hits[9] == 6000, hits  # every pointer finds its records (`/1/` asks an array's scalar for the key "")


def test_one_long_level(emu):
    """a root object of 20 000 fields whose values are nested objects, a root array of 20 000 mixed elements: one lane passes every sibling"""
    fields = [b'"key%d":{"v":{"w":[%d]},"s":"%d"}' % (i, i, i) for i in range(20000)]
    obj = b"{" + b",".join(fields) + b"}"
    arr = b"[" + b",".join([b"%d" % i, b'"s%d"' % i, b"[[%d]]" % i, b'{"k":%d.5}' % i, b"null"][i % 5] for i in range(20000)) + b"]"
    pointers = [b"/key0", b"/key19999", b"/key20000", b"/key1999", b"/key1999/v/w/0", b"/key19999/s", b"/0", b"/19999", b"/20000", b"/19998/k", b"/19997/0/0", b""]
    tags = emu([obj, arr, b'{"key19999":1}'], pointers)
    assert [chr(t) if t >= 34 else int(t) for t in tags[:, 0]] == ["{", "{", 20, "{", "l", '"', 20, 20, 20, 20, 20, "{"]
    assert [chr(t) if t >= 34 else int(t) for t in tags[:, 1]] == [17, 17, 17, 17, 17, 17, "l", "n", 19, "d", "l", "["]
