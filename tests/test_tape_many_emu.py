"""CPU tier: stage 2 of a document STREAM -- the gfx950 kernel sources of sjgpu_tape.hip (STREAM instantiation), sjgpu_tape_many.hip, the string
pass and the scans, compiled as C++ against tests/host/emu -- run the launches of sjgpu_stage2_many_device on whole streams and are compared
document by document with the oracle's serial walk over each document's own bytes (tests/host/test_tape_many_emu.cpp): code and documents
delivered always; tape words, string records and table entries of every document delivered."""
import os
import struct
import subprocess

import numpy as np
import pytest

import stream_cases
from simdjson_amd import _paths

CSRC = os.path.join(_paths.PKG_DIR, "csrc")
EMU = os.path.join(_paths.REPO_ROOT, "tests", "host", "emu")
KERNEL_TUS = ("sjgpu_tape", "sjgpu_tape_many", "sjgpu_strings", "sjgpu_string_stream", "sjgpu_finish")


def build(out):
    """the way tests/test_tape_emu.py builds the single document's kernels, plus the new unit"""
    inc = ["-I", EMU, "-I", _paths.INCLUDE_DIR, "-I", CSRC, "-I", _paths.ORACLE_DIR]
    jobs = []
    for name in KERNEL_TUS:
        jobs.append(subprocess.Popen(["g++", "-std=c++17", "-O1", "-Wno-attributes", "-Wno-unknown-pragmas", "-x", "c++", *inc, "-c",
                                      os.path.join(CSRC, name + ".hip"), "-o", str(out / (name + ".o"))]))
    jobs.append(subprocess.Popen(["g++", "-std=c++17", "-O2", *inc, "-c", os.path.join(EMU, "sj_emu.cpp"), "-o", str(out / "sj_emu.o")]))
    jobs.append(subprocess.Popen(["g++", "-std=c++17", "-O2", "-Wno-attributes", *inc, "-c",
                                  os.path.join(_paths.REPO_ROOT, "tests", "host", "test_tape_many_emu.cpp"), "-o", str(out / "driver.o")]))
    for name in ("sj_oracle", "sj_oracle_stage2"):
        jobs.append(subprocess.Popen(["gcc", "-O2", "-std=c99", "-D_POSIX_C_SOURCE=200809L", "-c", os.path.join(_paths.ORACLE_DIR, name + ".c"),
                                      "-o", str(out / (name + ".o"))]))
    assert all(j.wait() == 0 for j in jobs)
    exe = str(out / "test_tape_many_emu")
    objs = [str(out / (f + ".o")) for f in (*KERNEL_TUS, "sj_emu", "driver", "sj_oracle", "sj_oracle_stage2")]
    subprocess.run(["g++", *objs, "-lpthread", "-lm", "-o", exe], check=True)
    return exe


def record(stream, begins=(), max_depth=1024, want=None):
    want_docs, want_code = want if want is not None else (-1, -1)
    return (struct.pack("<I", len(stream)) + stream + struct.pack("<IiiI", max_depth, want_docs, want_code, len(begins)) +
            b"".join(struct.pack("<I", b) for b in begins))


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    exe = build(tmp_path_factory.mktemp("tape_many_emu"))

    def run(records):
        p = subprocess.run([exe], input=b"".join(records), capture_output=True, timeout=1500)
        assert p.returncode == 0, p.stderr.decode(errors="replace")[-3000:]
        out = p.stdout.decode()
        assert " 0 mismatches" in out and f"{len(records)} streams," in out and " 0 skipped" in out, out
        return out
    return run


def joined(docs, max_depth=1024):
    return [record(*stream_cases.join(docs, sep), max_depth=max_depth) for sep in stream_cases.SEPARATORS]


def test_valid_streams(emu):
    rng = np.random.default_rng(21)
    records = []
    for count in (1, 2, 3, 17, 400):
        records += joined(stream_cases.valid_documents(rng, count))
    out = emu(records)
    assert f"{3 * (1 + 2 + 3 + 17 + 400)} documents delivered" in out and " 0 broken streams" in out, out


def test_fixtures_three_times_each(emu):
    docs = [open(os.path.join(_paths.REPO_ROOT, "tests", "golden", "jsonexamples", name), "rb").read() for name in ("twitter.json", "citm_catalog.json")]
    out = emu(joined([docs[0], docs[1], docs[0], docs[1], docs[0], docs[1]]))
    assert "18 documents delivered" in out, out


def test_root_scalars_every_valid_number(emu):
    import jsongen
    orc_valid = [t.encode() for t in jsongen.number_corner_cases()[::5]]
    # (the driver's oracle decides which texts are valid: a stream made of ALL of them stops at the first invalid one, so each text gets a stream of
    # its own between two valid neighbours -- and the valid ones one long stream)
    records = [record(*stream_cases.join([b"1", t, b'"z"'], b"\n")) for t in orc_valid]
    emu(records)


def test_streams_of_many_blocks(emu):
    """token blocks of 4 096, sort tiles of 2 048 elements, string segments of 16 KiB: thousands of small records, documents across every boundary"""
    rng = np.random.default_rng(22)
    docs = stream_cases.small_records(rng, 6000)
    out = emu(joined(docs))
    assert "18000 documents delivered" in out, out
    # a few large documents between small ones: documents that span several blocks, tiles and segments
    big = [b"[" + b",".join(stream_cases.valid_documents(rng, 700)) + b"]" for _ in range(3)]
    mixed = docs[:50] + [big[0]] + docs[50:60] + [big[1], big[2]] + docs[60:90]
    out = emu(joined(mixed))
    assert f"{3 * len(mixed)} documents delivered" in out, out


def test_deep_documents_between_flat_ones(emu):
    """both roads of the sort: documents nested 63, 64, 65 and 200 deep"""
    deep = [b"[" * d + b"1" + b"]" * d for d in (63, 64, 65, 200)] + [b'{"a":[' * 100 + b"{}" + b"]}" * 100]
    docs = [b'{"a":1}', deep[0], b"[1,2]", deep[1], b"3", deep[2], deep[3], b'"s"', deep[4], b"[]"]
    out = emu(joined(docs))
    assert f"{3 * len(docs)} documents delivered" in out, out


@pytest.mark.parametrize("count", [1, 2, 500])
def test_one_broken_document(emu, count):
    """a broken document first, in the middle and last: the code of its own parse, the documents in front of it delivered in full"""
    rng = np.random.default_rng(23 + count)
    valid = stream_cases.valid_documents(rng, count)
    records = []
    broken = stream_cases.broken_documents()
    if count == 500:
        broken = broken[::3]
    for where in sorted({0, count // 2, count - 1}):
        for k, (_, bad) in enumerate(broken):
            docs = list(valid)
            docs[where] = bad
            records.append(record(*stream_cases.join(docs, stream_cases.SEPARATORS[k % 3])))
    out = emu(records)
    assert f"{len(records)} broken streams" in out, out
    if count != 500:  # (every breakage is in: every code the classes lead to)
        for code in (3, 5, 6, 7, 8, 9, 10):
            assert f"code {code}:" in out, out


@pytest.mark.parametrize("max_depth", [1, 2, 3, 16])
def test_nesting_beyond_max_depth(emu, max_depth):
    flat = [b"1", b"[]", b"{}", b'"s"', b"true"] + ([b"[1]", b'{"a":2}'] if max_depth > 1 else [])
    records = []
    for count in (1, 2, 40):
        for where in sorted({0, count // 2, count - 1}):
            docs = [flat[k % len(flat)] for k in range(count)]
            docs[where] = stream_cases.too_deep(max_depth)
            records += joined(docs, max_depth)
    out = emu(records)
    assert f"code 4: {len(records)}" in out, out


def test_hand_written_table(emu):
    records = [record(stream, max_depth=max_depth, want=(docs, code)) for stream, max_depth, docs, code in stream_cases.HAND_WRITTEN]
    emu(records)


def test_stray_close_leaves_the_first_document_intact(emu):
    rng = np.random.default_rng(29)
    out = emu([record(stream_cases.stray_close_behind_a_large_document(rng), want=(1, 3))])
    assert "1 documents delivered" in out and "1 second runs" in out, out
