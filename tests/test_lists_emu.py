"""CPU tier: at_path_with_wildcard rooted at cells -- the gfx950 kernel sources of sjgpu_query.hip and the scans of sjgpu_finish.hip, compiled as C++ against
tests/host/emu -- run the launches of sjgpu_at_paths_from_cells_device (tests/host/test_lists_emu.cpp) over tapes the oracle built document by document, laid
out as the document table says, and are compared match for match with tests/lists_model.py: the fixture's rows under the fixture's paths, the fields of
thousands of small records, the 20 000 elements of one document beside a stream of 4 097, roots that are no elements, the capacities and the limits.  The
driver also runs built with -fsanitize=address,undefined."""
import os
import struct
import subprocess

import numpy as np
import pytest

import checkers
import lists_model
import path_cases
import path_model
import pointer_model
import query_cases
import rows_model
import stream_cases
from simdjson_amd import _paths
from test_lists_model import fixture

CSRC = os.path.join(_paths.PKG_DIR, "csrc")
EMU = os.path.join(_paths.REPO_ROOT, "tests", "host", "emu")
KERNEL_TUS = ("sjgpu_query", "sjgpu_finish")
EXACT, ONE_SHORT, NONE = 0, 1, 2
OVERFLOW = -5


def build(out, sanitize=()):
    """the way tests/test_rows_emu.py builds its units"""
    inc = ["-I", EMU, "-I", _paths.INCLUDE_DIR, "-I", CSRC]
    jobs = []
    for name in KERNEL_TUS:
        jobs.append(subprocess.Popen(["g++", "-std=c++17", "-O1", *sanitize, "-Wno-attributes", "-Wno-unknown-pragmas", "-x", "c++", *inc, "-c",
                                      os.path.join(CSRC, name + ".hip"), "-o", str(out / (name + ".o"))]))
    jobs.append(subprocess.Popen(["g++", "-std=c++17", "-O2", *sanitize, *inc, "-c", os.path.join(EMU, "sj_emu.cpp"), "-o", str(out / "sj_emu.o")]))
    jobs.append(subprocess.Popen(["g++", "-std=c++17", "-O2", *sanitize, "-Wno-attributes", *inc, "-c",
                                  os.path.join(_paths.REPO_ROOT, "tests", "host", "test_lists_emu.cpp"), "-o", str(out / "driver.o")]))
    assert all(j.wait() == 0 for j in jobs)
    exe = str(out / "test_lists_emu")
    subprocess.run(["g++", *sanitize, *[str(out / (f + ".o")) for f in (*KERNEL_TUS, "sj_emu", "driver")], "-lpthread", "-o", exe], check=True)
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
        self.model = lists_model.Stream(self.tape, self.sbuf, self.table)

    def matches(self, path):
        """the flattened matches of one path over all documents (tests/path_model.py): a row of root cells"""
        _, _, tags, values = path_model.column([(t.tolist(), s.tobytes()) for t, s in self.parsed], [path])
        return np.array(tags, np.uint8), np.array(values, np.uint64)


def blob_of(S, roots, paths, capacity=EXACT):
    root_tags, root_values = np.ascontiguousarray(roots[0], np.uint8), np.ascontiguousarray(roots[1], np.uint64)
    lens = np.array([len(p) for p in paths], np.uint32)
    return (struct.pack("<IQQ", S.docs, len(S.tape), len(S.sbuf)) + S.tape.tobytes() + S.sbuf.tobytes() + S.table.tobytes() + struct.pack("<I", len(root_tags)) +
            root_tags.tobytes() + root_values.tobytes() + struct.pack("<I", len(paths)) + lens.tobytes() + b"".join(paths) + struct.pack("<I", capacity))


def columns_of(out, calls):
    """the driver's records, one per (rows, K): [(code, matches, status[K, rows], offsets, tags, values)]"""
    at, got = 0, []
    for rows, K in calls:
        code, matches = struct.unpack_from("<iQ", out, at)
        at += 12
        cells = rows * K
        status = np.frombuffer(out, np.uint8, cells, at).reshape(K, rows)
        at += cells
        offsets = np.frombuffer(out, np.uint32, cells + 1, at)
        at += 4 * (cells + 1)
        written = 0 if code else matches
        tags = np.frombuffer(out, np.uint8, written, at)
        at += written
        values = np.frombuffer(out, np.uint64, written, at)
        at += 8 * written
        got.append((code, matches, status, offsets, tags, values))
    assert at == len(out)
    return got


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    exe = build(tmp_path_factory.mktemp("lists_emu"))

    def run(S, roots, paths, want=None, capacity=EXACT):
        """-> the model's column; everything the driver wrote is compared with it (or with `want`) here"""
        p = subprocess.run([exe], input=blob_of(S, roots, paths, capacity), capture_output=True, timeout=1500)
        assert p.returncode == 0, p.stderr.decode(errors="replace")[-3000:]
        (code, matches, status, offsets, tags, values), = columns_of(p.stdout, [(len(roots[0]), len(paths))])
        want = lists_model.column(S.model, None, None, roots, paths) if want is None else want
        assert matches == len(want[2]) == int(offsets[-1])
        if capacity == EXACT or matches == 0:
            assert code == 0
            path_cases.assert_column((status, offsets, tags, values), want)
            path_cases.check_container_matches(tags, values, S.tape)
        else:  # the matches do not fit: statuses and offsets complete, nothing written (the driver checks that), the total reported
            assert code == OVERFLOW and tags.size == 0
            path_cases.assert_column((status, offsets), want[:2])
        return want
    run.exe = exe
    return run


@pytest.fixture(scope="module")
def fixture_stream(orc):
    docs, row_paths, paths, tables = fixture()
    S = Stream(orc, docs)
    tags, values = zip(*[S.matches(rp) for rp in row_paths])
    return S, (np.concatenate(tags), np.concatenate(values)), paths


def test_the_fixture_rows_under_the_fixture_paths(emu, fixture_stream):
    """the rows of all five row paths over all documents as ONE row of roots (the model is pinned against the fixture by tests/test_lists_model.py)"""
    S, roots, paths = fixture_stream
    assert len(roots[0]) > 300 and set(b'{["ldtfn') <= set(roots[0].tolist())
    status, offsets, tags, values = emu(S, roots, paths)
    assert {0, 17, 19, 20, 22} <= set(status.reshape(-1).tolist()) and (np.diff(offsets.astype(np.int64)) >= 2).sum() >= 100
    status, offsets, tags, values = emu(S, roots, [])
    assert offsets.tolist() == [0] and emu(S, (roots[0][:0], roots[1][:0]), paths[:3])[1].tolist() == [0]
    # the output is a row of roots again: a second level
    emu(S, (tags, values), [b"[*]", b"$.*", b"$.b", b""])


def test_the_capacities(emu, fixture_stream):
    S, roots, paths = fixture_stream
    for capacity in (ONE_SHORT, NONE):
        emu(S, roots, paths[:8], capacity=capacity)
    nothing = [b"$.nothing[*]", b"", b"$.nothing"]  # no match at all: capacity 0 with null outputs is exact
    assert len(emu(S, roots, nothing, capacity=NONE)[2]) == 0 and len(emu(S, roots, nothing, capacity=ONE_SHORT)[2]) == 0


def test_the_driver_runs_clean_under_the_sanitizers(tmp_path, fixture_stream):
    """the stand-alone driver -- kernels, launchers, path compiler -- built with -fsanitize=address,undefined: the fixture, all three capacities"""
    S, roots, paths = fixture_stream
    # (the runtimes linked statically: the program stands alone, whatever else the loader is told to bring in)
    exe = build(tmp_path, ("-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer", "-g"))
    blob = b"".join(blob_of(S, roots, paths, c) for c in (EXACT, ONE_SHORT, NONE))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe], input=blob, capture_output=True, timeout=1500, env=env)
    assert p.returncode == 0 and b"runtime error" not in p.stderr and b"AddressSanitizer" not in p.stderr, p.stderr.decode(errors="replace")[-3000:]
    got = columns_of(p.stdout, [(len(roots[0]), len(paths))] * 3)
    want = lists_model.column(S.model, None, None, roots, paths)
    path_cases.assert_column(got[0][2:], want)
    assert [g[0] for g in got] == [0, OVERFLOW, OVERFLOW]


def test_six_thousand_small_records(emu, orc):
    rng = np.random.default_rng(81)
    S = Stream(orc, stream_cases.small_records(rng, 6000))
    rows = S.matches(b"$.*")  # every field of the objects, every element of the arrays: all kinds of cells
    assert len(rows[0]) > 12000 and set(b'{["ldtn') <= set(rows[0].tolist())
    paths = path_cases.SMALL_RECORD_PATHS + [p[1:] for p in path_cases.SMALL_RECORD_PATHS] + [b".b.c[*].d", b"$.b.c[*]", b"[*][*]", b"$.k[*]"]
    status, offsets, tags, values = emu(S, rows, paths)
    counts = np.diff(offsets.astype(np.int64)).reshape(len(paths), len(rows[0]))
    share = (counts > 0).mean(axis=1)
    k = {p: i for i, p in enumerate(paths)}
    assert share[k[b"$[*]"]] > 0.10 and share[k[b"[*]"]] == share[k[b"$[*]"]] and share[k[b".b.c[*].d"]] > 0.02 and share[k[b"[*][*]"]] > 0.02, share
    assert set(status[k[b"$.name"]].tolist()) == {0, 17, 20} and (status[k[b"$.tags[*]"]] == 0).all()


def test_one_document_of_twenty_thousand_rows_beside_a_stream(emu, orc):
    """one table entry pair (the search is no search) and 4 097 of them, the same kernels"""
    arr = b"[" + b",".join(b'{"id":%d,"user":{"name":"u%d","tags":[%d,"t"]},"n":null,"e":[]}' % (i, i, i) for i in range(20000)) + b"]"
    paths = [b"$.user.tags[*]", b"$.*", b"$.id", b"$.e[*]", b"$.missing", b"$.user[*]"]
    S = Stream(orc, [arr])
    rows = S.matches(b"$[*]")
    assert len(rows[0]) == 20000
    status, offsets, tags, values = emu(S, rows, paths)
    counts = np.diff(offsets.astype(np.int64)).reshape(len(paths), 20000)
    assert (counts == np.array([2, 4, 1, 0, 0, 2])[:, None]).all() and (status[4] == 20).all() and (np.delete(status, 4, axis=0) == 0).all()
    assert np.array_equal(values[: 40000: 2], np.arange(20000, dtype=np.uint64))
    rng = np.random.default_rng(82)
    S = Stream(orc, stream_cases.small_records(rng, 4097))
    rows = S.matches(b"$.*")
    order = rng.permutation(len(rows[0]))  # the roots of a row need no order
    emu(S, (rows[0][order], rows[1][order]), [b"$[*]", b".*", b"$.b.c[*].d"])
    roots = pointer_model.columns(S.parsed, [b""])  # the documents' roots, the first and the last document among them: 4 097 counts, the scan's second level
    status, offsets, tags, values = emu(S, (roots[0][0], roots[1][0]), [b"$.tags[*]", b"$[*]", b"$.name"])
    flat = path_cases.model_column([(t.tolist(), s.tobytes()) for t, s in S.parsed], [b"$.tags[*]", b"$[*]", b"$.name"])
    path_cases.assert_column((status, offsets, tags, values), flat)  # rooted at the documents' roots: the column of sjgpu_at_paths_device


def test_roots_that_are_no_elements(emu, orc):
    """the hand-made roots of tests/test_rows_emu.py::test_roots_that_are_no_elements"""
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
    paths = [b"$.b[*]", b"$.*", b"$.b", b"", b"b[*]", b"$.b[*].c", b"$.x"]
    status, offsets, tags, values = emu(S, roots, paths)
    counts = np.diff(offsets.astype(np.int64)).reshape(len(paths), len(cells))
    assert counts[:, 0].tolist() == [3, 1, 1, 0, 0, 1, 0] and status[:, 0].tolist() == [0, 0, 0, 22, 22, 0, 20]
    bad = list(range(1, 13)) + [15, 16] + list(range(17, 30))
    assert (status[:, bad] == 20).all() and (counts[:, 1:] == 0).all()
    assert status[:, 14].tolist() == [0, 0, 20, 22, 22, 0, 20]  # (the value word agrees with the cell made for it: an object without fields)
    for j, code in zip(range(30, 34), (17, 19, 20, 22)):
        assert (status[:, j] == code).all()
    scalars = list(range(34, 42)) + [13]
    assert (status[:, scalars] == 0).all()
    # no documents at all: no container root has one
    E = Stream(orc, [])
    status, offsets, tags, values = emu(E, roots, paths)
    containers = [j for j, (t, _) in enumerate(cells) if t in (ord("{"), ord("["))]
    assert (status[:, containers] == 20).all() and int(offsets[-1]) == 0 and (status[:, scalars] == 0).all()


def test_the_limits(emu, orc):
    S = Stream(orc, [b"[" * 8 + b"[1,2],[3]" + b"]" * 8])
    roots = pointer_model.columns(S.parsed, [b""])
    roots = (roots[0][0], roots[1][0])

    def code(paths):
        return subprocess.run([emu.exe], input=blob_of(S, roots, paths), capture_output=True, timeout=300).returncode
    assert code([b"$[*]"] * 64) == 0 and code([b"$[*]"] * 65) == 3
    assert code([b"$." + b"a" * 1022]) == 0 and code([b"$." + b"a" * 1023]) == 3                  # 1 024 bytes, 1 025
    assert code([b"$" + b".a" * 31 + b"[*]"]) == 0 and code([b"$" + b".a" * 32 + b"[*]"]) == 3    # 32 levels, 33
    assert code([b"$" + b"[*]" * 8]) == 0 and code([b"$" + b"[*]" * 9]) == 3                      # 8 wildcards, 9
    assert code([b"$" + b".a" * 32]) == 0 and code([b"$" + b".a" * 33]) == 3                      # 32 pointer tokens, 33
    # eight frames deep below a root that is itself one level down
    inner = S.matches(b"$[*]")
    status, offsets, tags, values = emu(S, inner, [b"$" + b"[*]" * 7, b"[*]" * 8, b"$" + b"[*]" * 6 + b"[0][*]"])
    assert np.diff(offsets.astype(np.int64)).tolist() == [2, 3, 0]
