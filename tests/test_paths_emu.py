"""CPU tier: the paths over tapes -- the gfx950 kernel sources of sjgpu_query.hip and the scans of sjgpu_finish.hip, compiled as C++ against
tests/host/emu -- run the launches of sjgpu_at_paths_device and, over the flattened column, of sjgpu_gather_strings_device
(tests/host/test_paths_emu.cpp) over tapes the oracle built document by document, laid out as the document table says, and are compared match for
match with tests/path_model.py: the fixture's documents as one stream, thousands of small records, and one long level."""
import os
import struct
import subprocess

import numpy as np
import pytest

import checkers
import path_cases
import pointer_model
import query_cases
import stream_cases
from simdjson_amd import _paths

CSRC = os.path.join(_paths.PKG_DIR, "csrc")
EMU = os.path.join(_paths.REPO_ROOT, "tests", "host", "emu")
KERNEL_TUS = ("sjgpu_query", "sjgpu_finish")


def build(out):
    """the way tests/test_query_emu.py builds its units"""
    inc = ["-I", EMU, "-I", _paths.INCLUDE_DIR, "-I", CSRC]
    jobs = []
    for name in KERNEL_TUS:
        jobs.append(subprocess.Popen(["g++", "-std=c++17", "-O1", "-Wno-attributes", "-Wno-unknown-pragmas", "-x", "c++", *inc, "-c",
                                      os.path.join(CSRC, name + ".hip"), "-o", str(out / (name + ".o"))]))
    jobs.append(subprocess.Popen(["g++", "-std=c++17", "-O2", *inc, "-c", os.path.join(EMU, "sj_emu.cpp"), "-o", str(out / "sj_emu.o")]))
    jobs.append(subprocess.Popen(["g++", "-std=c++17", "-O2", "-Wno-attributes", *inc, "-c",
                                  os.path.join(_paths.REPO_ROOT, "tests", "host", "test_paths_emu.cpp"), "-o", str(out / "driver.o")]))
    assert all(j.wait() == 0 for j in jobs)
    exe = str(out / "test_paths_emu")
    subprocess.run(["g++", *[str(out / (f + ".o")) for f in (*KERNEL_TUS, "sj_emu", "driver")], "-lpthread", "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def orc():
    return checkers.Oracle()


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build(tmp_path_factory.mktemp("paths_emu"))


@pytest.fixture(scope="module")
def emu(exe, orc):

    def run(docs, paths):
        """-> (the model's column, the stream's string buffer); everything the driver wrote is compared with the model here"""
        parsed = []
        for d in docs:
            err, tape, sbuf = orc.dom_parse(d)
            assert err == 0, d[:100]
            parsed.append((tape, sbuf))
        tape, sbuf, table = query_cases.lay_out(parsed)
        lens = np.array([len(p) for p in paths], np.uint32)
        blob = (struct.pack("<IQQ", len(docs), len(tape), len(sbuf)) + tape.tobytes() + sbuf.tobytes() + table.tobytes() + struct.pack("<I", len(paths)) + lens.tobytes() +
                b"".join(paths))
        p = subprocess.run([exe], input=blob, capture_output=True, timeout=1500)
        assert p.returncode == 0, p.stderr.decode(errors="replace")[-3000:]
        out, cells = p.stdout, len(docs) * len(paths)
        matches = struct.unpack_from("<Q", out, 0)[0]
        at = 8
        status = np.frombuffer(out, np.uint8, cells, at).reshape(len(paths), len(docs))
        at += cells
        offsets = np.frombuffer(out, np.uint32, cells + 1, at)
        at += 4 * (cells + 1)
        tags = np.frombuffer(out, np.uint8, matches, at)
        at += matches
        values = np.frombuffer(out, np.uint64, matches, at)
        at += 8 * matches
        want = path_cases.model_column([(t.tolist(), s.tobytes()) for t, s in parsed], paths)
        assert matches == len(want[2]) == int(offsets[-1])
        path_cases.assert_column((status, offsets, tags, values), want)
        path_cases.check_container_matches(tags, values, tape)
        # the gather over the flattened column: one string slice per match
        strings = [pointer_model.string_of(sbuf, int(v)) if t == ord('"') else b"" for t, v in zip(tags, values)]
        total = struct.unpack_from("<Q", out, at)[0]
        goffsets = np.frombuffer(out, np.uint32, matches + 1, at + 8)
        chars = out[at + 8 + 4 * (matches + 1): at + 8 + 4 * (matches + 1) + total]
        at += 8 + 4 * (matches + 1) + total
        assert at == len(out)
        assert total == sum(len(s) for s in strings)
        assert np.array_equal(goffsets, np.concatenate([[0], np.cumsum([len(s) for s in strings])]).astype(np.uint32))
        assert chars == b"".join(strings)
        return want, strings
    return run


def test_the_fixture_as_one_stream(emu):
    docs, paths, cells = path_cases.fixture()
    for first in range(0, len(paths), 64):  # K <= 64 per call
        (status, offsets, tags, values), _ = emu(docs, paths[first: first + 64])
    (status, offsets, tags, values), _ = emu(docs[:3], [])
    assert offsets.tolist() == [0] and tags.size == 0


def test_six_thousand_small_records(emu):
    """the shares are asserted on the model alone by tests/test_path_model.py::test_the_small_records_are_not_vacuous, and here once more on the model's column,
    which is what emu() returns once the kernels' column has been found equal to it"""
    rng = np.random.default_rng(51)
    docs = stream_cases.small_records(rng, 6000)
    (status, offsets, tags, values), strings = emu(docs, path_cases.SMALL_RECORD_PATHS)
    share = (np.diff(offsets.astype(np.int64)).reshape(len(path_cases.SMALL_RECORD_PATHS), len(docs)) > 0).mean(axis=1)
    assert share[0] > 0.10 and share[1] > 0.10 and share[5] > 0.10 and share[3] > 0.50, share
    # the gather over the flattened `$.tags[*]` column alone: the tags of the records that have them, two strings each
    (_, offsets, _, _), strings = emu(docs, [b"$.tags[*]"])
    have = [d.startswith(b'{"id":') for d in docs]
    assert strings == [s for h in have if h for s in (b"a", b"b\n")] and int(offsets[-1]) == 2 * sum(have) > 1200


def test_one_long_level(emu):
    """a root array of 20 000 mixed elements and a root object of 20 000 fields beside a tiny document: one lane visits every child, twice"""
    n = 20000
    obj = b"{" + b",".join(b'"key%d":{"v":{"w":[%d,"s%d"]},"s":"%d"}' % (i, i, i, i) for i in range(n)) + b"}"
    arr = b"[" + b",".join([b"%d" % i, b'"s%d"' % i, b"[[%d]]" % i, b'{"k":%d.5}' % i, b"null"][i % 5] for i in range(n)) + b"]"
    (status, offsets, tags, values), _ = emu([arr, obj, b'{"key":{"v":{"w":[1]}}}'], [b"$[*]", b"$.*", b"$[*][0]", b"$.*.v.w[*]"])
    counts = np.diff(offsets.astype(np.int64)).reshape(4, 3)
    assert counts.tolist() == [[n, n, 1], [n, n, 1], [n // 5, 0, 0], [0, 2 * n, 1]] and (status == 0).all()


def test_the_limits_of_the_level_program(exe, orc, emu):
    """what sjgpu_at_paths_device refuses with SJGPU_E_BADARG is what compile_path_program refuses: the driver ends with 1 and says so"""
    doc = b"[" * 8 + b"[1,2],[3]" + b"]" * 8
    err, tape, sbuf = orc.dom_parse(doc)
    assert err == 0
    tape, sbuf, table = query_cases.lay_out([(tape, sbuf)])

    def refused(paths):
        lens = np.array([len(p) for p in paths], np.uint32)
        blob = (struct.pack("<IQQ", 1, len(tape), len(sbuf)) + tape.tobytes() + sbuf.tobytes() + table.tobytes() + struct.pack("<I", len(paths)) + lens.tobytes() + b"".join(paths))
        p = subprocess.run([exe], input=blob, capture_output=True, timeout=300)
        assert p.returncode in (0, 1), p.stderr
        assert (p.returncode == 1) == (b"beyond the limits" in p.stderr)
        return p.returncode == 1
    assert refused([b"$[*]"] * 65) and not refused([b"$[*]"] * 64)
    assert refused([b"$." + b"a" * 1023]) and not refused([b"$." + b"a" * 1022])                # 1 025 bytes, 1 024
    assert refused([b"$" + b"[*]" * 9]) and not refused([b"$" + b"[*]" * 8])                    # 9 wildcards, 8
    assert refused([b"$" + b"[*]" * 9 + b".a"]) and not refused([b"$" + b"[*]" * 8 + b".a.b"])  # ... with a tail behind them
    assert refused([b"$" + b".a" * 32 + b"[*]"]) and not refused([b"$" + b".a" * 31 + b"[*]"])  # 33 levels, 32
    assert refused([b"$" + b".a" * 33]) and not refused([b"$" + b".a" * 32])                    # 33 pointer tokens, 32
    assert refused([b"$" + b".a/b" * 16 + b".c[*]"]) and not refused([b"$" + b".a/b" * 16 + b"[*]"])  # 33 tokens over 17 levels, 32 over 16
    # eight frames deep: the paths at the limit against the model
    (status, offsets, tags, values), _ = emu([doc, b"[[[[[[[[[[7]]]]]]]]]]"], [b"$" + b"[*]" * 8, b"$" + b"[*]" * 8 + b"[0]", b"$" + b"[*]" * 7 + b"[0][*]", b"$" + b"[*]" * 8 + b"[0][0]"])
    # (the third: `[0]` in front of a `*` is INVALID_JSON_POINTER, swallowed below the root; the fourth: `[0]` of the scalar 1 is an error, swallowed too)
    assert np.diff(offsets.astype(np.int64)).tolist() == [2, 1, 2, 1, 0, 0, 0, 1]
