"""CPU tier: at_pointer rooted at cells -- the gfx950 kernel sources of sjgpu_query.hip, compiled as C++ against tests/host/emu -- run the launches of
sjgpu_at_pointers_from_cells_device (tests/host/test_rows_emu.cpp) over tapes the oracle built document by document, laid out as the document table says,
and are compared cell by cell with tests/rows_model.py: the fixture's cells as roots of the fixture's pointers, the arrays and the fields of thousands of
small records, the 20 000 elements of one document beside a stream of 4 097, roots that are no elements, and the limits."""
import os
import struct
import subprocess

import numpy as np
import pytest

import checkers
import path_model
import pointer_model
import query_cases
import rows_model
import stream_cases
from simdjson_amd import _paths

CSRC = os.path.join(_paths.PKG_DIR, "csrc")
EMU = os.path.join(_paths.REPO_ROOT, "tests", "host", "emu")
KERNEL_TUS = ("sjgpu_query", "sjgpu_finish")


def build(out):
    """the way tests/test_paths_emu.py builds its units"""
    inc = ["-I", EMU, "-I", _paths.INCLUDE_DIR, "-I", CSRC]
    jobs = []
    for name in KERNEL_TUS:
        jobs.append(subprocess.Popen(["g++", "-std=c++17", "-O1", "-Wno-attributes", "-Wno-unknown-pragmas", "-x", "c++", *inc, "-c",
                                      os.path.join(CSRC, name + ".hip"), "-o", str(out / (name + ".o"))]))
    jobs.append(subprocess.Popen(["g++", "-std=c++17", "-O2", *inc, "-c", os.path.join(EMU, "sj_emu.cpp"), "-o", str(out / "sj_emu.o")]))
    jobs.append(subprocess.Popen(["g++", "-std=c++17", "-O2", "-Wno-attributes", *inc, "-c",
                                  os.path.join(_paths.REPO_ROOT, "tests", "host", "test_rows_emu.cpp"), "-o", str(out / "driver.o")]))
    assert all(j.wait() == 0 for j in jobs)
    exe = str(out / "test_rows_emu")
    subprocess.run(["g++", *[str(out / (f + ".o")) for f in (*KERNEL_TUS, "sj_emu", "driver")], "-lpthread", "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def orc():
    return checkers.Oracle()


class Stream:
    """documents parsed by the oracle and laid out as one stream"""

    def __init__(self, orc, docs):
        self.parsed = []
        for d in docs:
            err, tape, sbuf = orc.dom_parse(d)
            assert err == 0, d[:100]
            self.parsed.append((tape, sbuf))
        self.tape, self.sbuf, self.table = query_cases.lay_out(self.parsed)
        self.docs = len(docs)

    def matches(self, path):
        """the flattened matches of one path over all documents (tests/path_model.py): a row of root cells"""
        _, _, tags, values = path_model.column([(t.tolist(), s.tobytes()) for t, s in self.parsed], [path])
        return np.array(tags, np.uint8), np.array(values, np.uint64)


def blob_of(S, roots, pointers):
    root_tags, root_values = np.ascontiguousarray(roots[0], np.uint8), np.ascontiguousarray(roots[1], np.uint64)
    lens = np.array([len(p) for p in pointers], np.uint32)
    return (struct.pack("<IQQ", S.docs, len(S.tape), len(S.sbuf)) + S.tape.tobytes() + S.sbuf.tobytes() + S.table.tobytes() + struct.pack("<I", len(root_tags)) +
            root_tags.tobytes() + root_values.tobytes() + struct.pack("<I", len(pointers)) + lens.tobytes() + b"".join(pointers))


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    exe = build(tmp_path_factory.mktemp("rows_emu"))

    def run(S, roots, pointers, want=None):
        """-> (tags, values) of the driver, compared with the model (or with `want`) here"""
        p = subprocess.run([exe], input=blob_of(S, roots, pointers), capture_output=True, timeout=1500)
        assert p.returncode == 0, p.stderr.decode(errors="replace")[-3000:]
        rows, K = len(roots[0]), len(pointers)
        assert len(p.stdout) == 9 * K * rows
        tags = np.frombuffer(p.stdout, np.uint8, K * rows).reshape(K, rows)
        values = np.frombuffer(p.stdout, np.uint64, K * rows, K * rows).reshape(K, rows)
        want_tags, want_values = rows_model.columns(S.tape, S.sbuf, S.table, roots, pointers) if want is None else want
        assert np.array_equal(tags, want_tags), np.argwhere(tags != want_tags)[:5]
        assert np.array_equal(values, want_values), np.argwhere(values != want_values)[:5]
        return tags, values
    run.exe = exe
    return run


def test_the_fixture_cells_as_roots(emu, orc):
    """every cell the fixture's pointers find in the fixture's documents -- hits and failures, 5 915 of them -- is a root of the fixture's pointers"""
    docs, pointers, cells = query_cases.fixture()
    S = Stream(orc, docs)
    root_tags, root_values = pointer_model.columns(S.parsed, pointers)
    roots = (root_tags.reshape(-1), root_values.reshape(-1))
    tape, sbuf = S.tape.tolist(), S.sbuf.tobytes()
    # the model over the DISTINCT roots: most of the fixture's cells are one of four failures
    memo = {}
    want_tags, want_values = np.zeros((len(pointers), len(roots[0])), np.uint8), np.zeros((len(pointers), len(roots[0])), np.uint64)
    for r, cell in enumerate(zip(roots[0].tolist(), roots[1].tolist())):
        if cell not in memo:
            memo[cell] = [rows_model.walk_from(tape, sbuf, cell, p, S.table) for p in pointers]
        for k, (t, v) in enumerate(memo[cell]):
            want_tags[k, r], want_values[k, r] = t, v
    assert len(memo) > 150
    hits = 0
    for first in range(0, len(pointers), 64):  # K <= 64 per call
        tags, _ = emu(S, roots, pointers[first: first + 64], (want_tags[first: first + 64], want_values[first: first + 64]))
        hits += int((tags >= 34).sum())
    assert b"" in pointers and (roots[0] >= 34).sum() > 150 and hits >= (roots[0] >= 34).sum(), hits  # the empty pointer alone finds every root that is an element
    assert emu(S, roots, [])[0].size == 0 and emu(S, (roots[0][:0], roots[1][:0]), pointers[:3])[0].size == 0


def test_six_thousand_small_records(emu, orc):
    rng = np.random.default_rng(71)
    S = Stream(orc, stream_cases.small_records(rng, 6000))
    tags_rows = S.matches(b"$.tags[*]")
    assert len(tags_rows[0]) > 1500 and (tags_rows[0] == ord('"')).all()
    emu(S, tags_rows, [b"", b"/0", b"x", b"/~"])
    fields = S.matches(b"$.*")  # every field of the objects, every element of the arrays: all kinds of cells
    assert len(fields[0]) > 12000 and set(b'{["ldtn') <= set(fields[0].tolist())
    tags, _ = emu(S, fields, [b"", b"/1", b"/b/c/1/d", b"/k", b"/1/0", b"b", b"/-"])
    hits = (tags >= 34).sum(axis=1)
    assert hits[0] == len(fields[0]) and (hits[1:5] > 500).all() and hits[5] == hits[6] == 0, hits


def test_one_document_of_twenty_thousand_rows_beside_a_stream(emu, orc):
    """one table entry pair (the search is no search) and 4 097 of them, the same kernels"""
    arr = b"[" + b",".join(b'{"id":%d,"user":{"name":"u%d","tags":[%d,"t"]},"n":null}' % (i, i, i) for i in range(20000)) + b"]"
    pointers = [b"/id", b"/user/name", b"/user/tags/1", b"/user/tags/2", b"/missing", b""]
    S = Stream(orc, [arr])
    rows = S.matches(b"$[*]")
    assert len(rows[0]) == 20000
    tags, values = emu(S, rows, pointers)
    assert np.array_equal(values[0], np.arange(20000, dtype=np.uint64)) and (tags[3] == 19).all() and (tags[4] == 20).all() and np.array_equal(values[5], rows[1])
    rng = np.random.default_rng(72)
    S = Stream(orc, stream_cases.small_records(rng, 4097))
    rows = S.matches(b"$.*")
    order = rng.permutation(len(rows[0]))  # the roots of a row need no order
    tags, _ = emu(S, (rows[0][order], rows[1][order]), [b"", b"/0", b"/b/c"])
    assert (tags[0] >= 34).all()
    roots = pointer_model.columns(S.parsed, [b""])  # the documents' roots: the first and the last document among them
    emu(S, (roots[0][0], roots[1][0]), [b"/id", b"/0", b""])


def test_roots_that_are_no_elements(emu, orc):
    docs = [b'[8863084066665136133,"x",{"k":1}]', b'{"a":{"b":[1,2,{"c":"d"}]},"n":12}', b'[[1],[2,3]]', b"7"]
    S = Stream(orc, docs)
    begins = [int(b) for b in S.table["tape_begin"]]
    assert int(S.tape[3]) == (ord("{") << 56) | 5  # a number's value word that reads like an opening word
    a_tag, a_value = rows_model.walk_from(S.tape.tolist(), S.sbuf.tobytes(), rows_model.root_cell(S.tape.tolist(), S.sbuf.tobytes(), S.table, 1), b"/a", S.table)
    assert chr(a_tag) == "{"
    c, high = a_value & 0xFFFFFFFF, a_value >> 32
    cells = [(a_tag, a_value),                                              # the good one
             (a_tag, (high << 32) | begins[1]), (a_tag, (high << 32) | begins[2]), (a_tag, (high << 32) | begins[0]),  # on a root word
             (a_tag, (high << 32) | (begins[2] - 1)),                        # on a document's last word
             (a_tag, (high << 32) | begins[4]), (a_tag, (high << 32) | (begins[4] + 5)), (a_tag, (high << 32) | 0xFFFFFFFF),  # past the last document
             (ord("["), a_value),                                            # wrong tag
             (a_tag, ((high + 1) << 32) | c), (a_tag, ((high - 1) << 32) | c), (a_tag, c), (a_tag, (0xFFFFFFFF << 32) | c),  # wrong high half
             (ord("l"), 3), (ord("{"), (5 << 32) | 3), (ord("{"), (6 << 32) | 3), (ord("["), (5 << 32) | 3),  # a number's value word as an opening index
             (ord("{"), (high << 32) | (c + 1)),                             # a key word as an opening index
             (0, 0), (1, 5), (16, 0), (18, 0), (21, 0), (23, 0), (33, 0), (ord("r"), a_value), (ord("}"), a_value), (ord("]"), a_value), (0x5A, 0x5A5A5A5A5A5A5A5A),
             (255, 1),                                                       # tags that are none
             (17, 0), (19, 9), (20, a_value), (22, 1 << 63),                 # failed roots keep their code
             (ord('"'), (2 << 32) | 4), (ord('"'), 0xFFFFFFFFFFFFFFFF), (ord("l"), 1 << 63), (ord("u"), 7), (ord("d"), 0), (ord("t"), 1), (ord("f"), 0), (ord("n"), 0)]
    roots = (np.array([t for t, _ in cells], np.uint8), np.array([v for _, v in cells], np.uint64))
    pointers = [b"", b"/b", b"/b/2/c", b"b", b"/~", b"/k", b"/0"]
    tags, values = emu(S, roots, pointers)
    assert [chr(t) for t in tags[:3, 0]] == ["{", "[", '"'] and tags[3, 0] == 22
    bad = list(range(1, 13)) + [15, 16] + list(range(17, 30))
    assert (tags[:, bad] == 20).all() and (values[:, bad] == 0).all()
    assert tags[0, 14] == ord("{") and (tags[1:, 14] == [20, 20, 22, 22, 20, 20]).all()  # (the value word agrees with the cell made for it: an object without fields)
    for j, code in zip(range(30, 34), (17, 19, 20, 22)):
        assert (tags[:, j] == code).all() and (values[:, j] == 0).all()
    scalars = list(range(34, 42)) + [13]
    assert np.array_equal(tags[0, scalars], roots[0][scalars]) and np.array_equal(values[0, scalars], roots[1][scalars])
    assert (tags[1:, scalars] == np.array([20, 20, 22, 22, 20, 20])[:, None]).all() and (values[1:, scalars] == 0).all()
    # no documents at all: no container root has one
    E = Stream(orc, [])
    tags, values = emu(E, roots, pointers)
    containers = [j for j, (t, _) in enumerate(cells) if t in (ord("{"), ord("["))]
    assert (tags[:, containers] == 20).all()


def test_the_limits(emu, orc):
    S = Stream(orc, [b'{"a":{"a":1}}'])
    roots = pointer_model.columns(S.parsed, [b""])
    roots = (roots[0][0], roots[1][0])

    def code(pointers):
        return subprocess.run([emu.exe], input=blob_of(S, roots, pointers), capture_output=True, timeout=300).returncode
    assert code([b"/a"] * 64) == 0 and code([b"/a"] * 65) == 3
    assert code([b"/" + b"a" * 1023]) == 0 and code([b"/" + b"a" * 1024]) == 3
    assert code([b"/a" * 32]) == 0 and code([b"/a" * 33]) == 3
