"""CPU tier: the fields of the cells' objects and the sizes of the cells' containers -- the gfx950 kernel sources of sjgpu_query.hip and the scans of
sjgpu_finish.hip, compiled as C++ against tests/host/emu -- run the launches of sjgpu_object_fields_from_cells_device and sjgpu_cell_sizes_device
(tests/host/test_fields_emu.cpp) over tapes the oracle built document by document, laid out as the document table says, and are compared slot for slot with
tests/fields_model.py: the fixture's rows, thousands of small records beside one object of 20 000 fields, rows at the wave's and the workgroup's edges, roots
that are no elements, the capacities, and tapes whose count fields were patched by hand.  The driver also runs built with -fsanitize=address,undefined."""
import os
import struct
import subprocess

import numpy as np
import pytest

import checkers
import fields_model
import path_model
import pointer_model
import query_cases
import stream_cases
from simdjson_amd import _paths
from test_fields_model import fixture

CSRC = os.path.join(_paths.PKG_DIR, "csrc")
EMU = os.path.join(_paths.REPO_ROOT, "tests", "host", "emu")
KERNEL_TUS = ("sjgpu_query", "sjgpu_finish")
EXACT, ONE_SHORT, NONE = 0, 1, 2
OVERFLOW = -5


def build(out, sanitize=()):
    """the way tests/test_lists_emu.py builds its units"""
    inc = ["-I", EMU, "-I", _paths.INCLUDE_DIR, "-I", CSRC]
    jobs = []
    for name in KERNEL_TUS:
        jobs.append(subprocess.Popen(["g++", "-std=c++17", "-O1", *sanitize, "-Wno-attributes", "-Wno-unknown-pragmas", "-x", "c++", *inc, "-c",
                                      os.path.join(CSRC, name + ".hip"), "-o", str(out / (name + ".o"))]))
    jobs.append(subprocess.Popen(["g++", "-std=c++17", "-O2", *sanitize, *inc, "-c", os.path.join(EMU, "sj_emu.cpp"), "-o", str(out / "sj_emu.o")]))
    jobs.append(subprocess.Popen(["g++", "-std=c++17", "-O2", *sanitize, "-Wno-attributes", *inc, "-c",
                                  os.path.join(_paths.REPO_ROOT, "tests", "host", "test_fields_emu.cpp"), "-o", str(out / "driver.o")]))
    assert all(j.wait() == 0 for j in jobs)
    exe = str(out / "test_fields_emu")
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
        self.model = fields_model.Stream(self.tape, self.sbuf, self.table)

    def matches(self, path):
        """the flattened matches of one path over all documents (tests/path_model.py): a row of root cells"""
        _, _, tags, values = path_model.column([(t.tolist(), s.tobytes()) for t, s in self.parsed], [path])
        return np.array(tags, np.uint8), np.array(values, np.uint64)

    def patched(self, at, count):
        """the same stream with the count field of the opening word at `at` replaced"""
        P = object.__new__(Stream)
        P.parsed, P.sbuf, P.table, P.docs = self.parsed, self.sbuf, self.table, self.docs
        P.tape = self.tape.copy()
        P.tape[at] = (int(P.tape[at]) & ~(0xFFFFFF << 32)) | (count << 32)
        P.model = fields_model.Stream(P.tape, P.sbuf, P.table)
        return P


def blob_of(S, roots, capacity=EXACT, docs=None):
    root_tags, root_values = np.ascontiguousarray(roots[0], np.uint8), np.ascontiguousarray(roots[1], np.uint64)
    docs = S.docs if docs is None else docs
    return (struct.pack("<IQQ", docs, len(S.tape), len(S.sbuf)) + S.tape.tobytes() + S.sbuf.tobytes() + S.table[: docs + 1].tobytes() + struct.pack("<I", len(root_tags)) +
            root_tags.tobytes() + root_values.tobytes() + struct.pack("<I", capacity))


def records_of(out, calls):
    """the driver's records, one per call of `rows` roots: [(code, fields, (status, offsets, key_tags, key_values, tags, values), (sizes, size codes))]"""
    at, got = 0, []
    for rows in calls:
        code, fields = struct.unpack_from("<iQ", out, at)
        at += 12
        status = np.frombuffer(out, np.uint8, rows, at)
        at += rows
        offsets = np.frombuffer(out, np.uint32, rows + 1, at)
        at += 4 * (rows + 1)
        written = 0 if code else fields
        cols = []
        for dtype, width in ((np.uint8, 1), (np.uint64, 8), (np.uint8, 1), (np.uint64, 8)):
            cols.append(np.frombuffer(out, dtype, written, at))
            at += width * written
        sizes = np.frombuffer(out, np.uint32, rows, at)
        at += 4 * rows
        size_codes = np.frombuffer(out, np.uint8, rows, at)
        at += rows
        got.append((code, fields, (status, offsets, *cols), (sizes, size_codes)))
    assert at == len(out)
    return got


def compare(record, want, want_sizes, capacity):
    code, fields, cols, sizes = record
    assert fields == len(want[2]) == int(cols[1][-1])
    if capacity == EXACT or fields == 0:
        assert code == 0
        fields_model.assert_columns(cols, want)
    else:  # the fields do not fit: statuses and offsets complete, nothing written (the driver checks that), the total reported
        assert code == OVERFLOW and cols[2].size == 0
        fields_model.assert_columns(cols[:2], want[:2])
    assert np.array_equal(sizes[0], want_sizes[0]) and np.array_equal(sizes[1], want_sizes[1])


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    exe = build(tmp_path_factory.mktemp("fields_emu"))

    def run(S, roots, capacity=EXACT, docs=None, model=None):
        """-> the model's columns; everything the driver wrote is compared with them here"""
        p = subprocess.run([exe], input=blob_of(S, roots, capacity, docs), capture_output=True, timeout=1500)
        assert p.returncode == 0, p.stderr.decode(errors="replace")[-3000:]
        record, = records_of(p.stdout, [len(roots[0])])
        model = S.model if model is None else model
        want = fields_model.column(model, roots)
        compare(record, want, fields_model.sizes(model, roots), capacity)
        return want
    return run


@pytest.fixture(scope="module")
def fixture_stream(orc):
    docs, row_paths, tables, _ = fixture()
    S = Stream(orc, docs)
    tags, values = zip(*[S.matches(rp) for rp in row_paths])
    return S, (np.concatenate(tags), np.concatenate(values))


def test_the_fixture_rows(emu, fixture_stream):
    """the rows of all five row paths over all documents as ONE row of roots (the model is pinned against the fixture by tests/test_fields_model.py)"""
    S, roots = fixture_stream
    assert len(roots[0]) > 700 and set(b'{["ludtfn') <= set(roots[0].tolist())
    status, offsets, key_tags, key_values, tags, values = emu(S, roots)
    assert set(status.tolist()) == {0, 17} and int(np.diff(offsets.astype(np.int64)).max()) == 300 and (key_tags == ord('"')).all()
    wide = int(offsets[int(np.argmax(np.diff(offsets.astype(np.int64)) == 300))])
    assert [pointer_model.string_of(S.sbuf, int(v)) for v in key_values[wide: wide + 300]] == [b"k%03d" % i for i in range(300)]
    # the value row is a row of roots again: a second nesting level, and a third
    again = emu(S, (tags, values))
    assert len(again[4]) > 100
    emu(S, (again[4], again[5]))
    # ... and so is the key row: strings, INCORRECT_TYPE
    assert (emu(S, (key_tags, key_values))[0] == 17).all()


def test_the_capacities(emu, fixture_stream):
    S, roots = fixture_stream
    for capacity in (ONE_SHORT, NONE):
        emu(S, roots, capacity)
    scalars = roots[0] != ord("{")  # no field at all: capacity 0 with null outputs is exact
    nothing = (roots[0][scalars], roots[1][scalars])
    assert len(emu(S, nothing, NONE)[2]) == 0 and len(emu(S, nothing, ONE_SHORT)[2]) == 0


def test_the_driver_runs_clean_under_the_sanitizers(tmp_path, fixture_stream):
    """the stand-alone driver -- kernels and launchers -- built with -fsanitize=address,undefined: the fixture, all three capacities"""
    S, roots = fixture_stream
    # (the runtimes linked statically: the program stands alone, whatever else the loader is told to bring in)
    exe = build(tmp_path, ("-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer", "-g"))
    blob = b"".join(blob_of(S, roots, c) for c in (EXACT, ONE_SHORT, NONE))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe], input=blob, capture_output=True, timeout=1500, env=env)
    assert p.returncode == 0 and b"runtime error" not in p.stderr and b"AddressSanitizer" not in p.stderr, p.stderr.decode(errors="replace")[-3000:]
    got = records_of(p.stdout, [len(roots[0])] * 3)
    want, want_sizes = fields_model.column(S.model, roots), fields_model.sizes(S.model, roots)
    for record, capacity in zip(got, (EXACT, ONE_SHORT, NONE)):
        compare(record, want, want_sizes, capacity)
    assert [g[0] for g in got] == [0, OVERFLOW, OVERFLOW]


@pytest.fixture(scope="module")
def records_stream(orc):
    """4 097 small records as one stream and one object of 20 000 fields beside them"""
    rng = np.random.default_rng(101)
    wide = b"{" + b",".join(b'"key%d":%s' % (i, (b"%d" % i, b'"v"', b'{"i":[%d]}' % i)[i % 3]) for i in range(20000)) + b"}"
    docs = stream_cases.small_records(rng, 4097)
    docs.insert(2000, wide)
    return Stream(orc, docs)


def test_small_records_and_one_object_of_twenty_thousand_fields(emu, records_stream):
    S = records_stream
    whole = pointer_model.columns(S.parsed, [b""])  # the documents' roots: 4 098 counts, the scan's second level
    roots = (whole[0][0], whole[1][0])
    status, offsets, key_tags, key_values, tags, values = emu(S, roots)
    counts = np.diff(offsets.astype(np.int64))
    assert counts[2000] == 20000 and (status == 0).sum() > 2000 and (status == 17).sum() > 500
    lo = int(offsets[2000])
    assert [pointer_model.string_of(S.sbuf, int(v)) for v in key_values[lo: lo + 20000: 4999]] == [b"key%d" % i for i in range(0, 20000, 4999)]
    # every field's value and every element of the arrays, in any order: all kinds of cells, the nested objects' fields
    rows = S.matches(b"$.*")
    assert len(rows[0]) > 28000 and set(b'{["ldtn') <= set(rows[0].tolist())
    order = np.random.default_rng(102).permutation(len(rows[0]))
    status, offsets, key_tags, key_values, tags, values = emu(S, (rows[0][order], rows[1][order]))
    assert len(tags) > 7000 and set(status.tolist()) == {0, 17}


@pytest.mark.parametrize("rows", [0, 1, 63, 64, 65, 255, 256, 257])
def test_rows_at_the_wave_and_workgroup_edges(emu, records_stream, rows):
    S = records_stream
    whole = pointer_model.columns(S.parsed, [b""])
    part = (whole[0][0][1990: 1990 + rows], whole[1][0][1990: 1990 + rows])  # (the wide object among them from 11 rows on)
    status, offsets, key_tags, key_values, tags, values = emu(S, part)
    assert offsets[0] == 0 and len(offsets) == rows + 1 and (rows < 63 or len(tags) > 20000)
    emu(S, part, ONE_SHORT)


def bad_cells(S, a_tag, a_value):
    begins = [int(b) for b in S.table["tape_begin"]]
    c, high = a_value & 0xFFFFFFFF, a_value >> 32
    return [(a_tag, a_value),                                              # the good one
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


def test_roots_that_are_no_elements(emu, orc):
    """the hand-made roots of tests/test_lists_emu.py::test_roots_that_are_no_elements"""
    docs = [b'[8863084066665136133,"x",{"k":1}]', b'{"a":{"b":[1,2,{"c":"d"}],"e":null},"n":12}', b'[[1],[2,3]]', b"7"]
    S = Stream(orc, docs)
    assert int(S.tape[3]) == (ord("{") << 56) | 5  # a number's value word that reads like an opening word
    a_tag, a_value = S.model.matches_from(fields_model.rows_model.root_cell(S.model.tape, S.model.sbuf, S.table, 1), b"$.a")[1][0]
    assert chr(a_tag) == "{"
    cells = bad_cells(S, a_tag, a_value)
    roots = (np.array([t for t, _ in cells], np.uint8), np.array([v for _, v in cells], np.uint64))
    status, offsets, key_tags, key_values, tags, values = emu(S, roots)
    counts = np.diff(offsets.astype(np.int64))
    assert counts[0] == 2 and status[0] == 0 and (counts[1:] == 0).all() and [chr(t) for t in tags] == ["[", "n"]
    bad = list(range(1, 13)) + [15, 16] + list(range(17, 30))
    assert (status[bad] == 20).all() and status[14] == 0  # (14: the value word agrees with the cell made for it: an object without fields)
    assert status[30:34].tolist() == [17, 19, 20, 22] and (status[list(range(34, 42)) + [13]] == 17).all()
    # a table without documents: no container root has one
    status, offsets, key_tags, key_values, tags, values = emu(S, roots, docs=0, model=fields_model.Stream(S.tape, S.sbuf, S.table[:1]))
    containers = [j for j, (t, _) in enumerate(cells) if t in (ord("{"), ord("["))]
    assert (status[containers] == 20).all() and int(offsets[-1]) == 0 and status[30:34].tolist() == [17, 19, 20, 22]


def test_patched_count_fields(emu, orc):
    """what no parser writes: a count field that is saturated on a small object (the walk counts), one that claims more than there is (padding), one that
    claims less (the fill stops at the root's last slot)"""
    docs = [b'{"p":1}', b'[{"a":1,"b":[2,{"x":3}],"c":"s"},{"after":true}]', b'{"q":[2]}']
    S = Stream(orc, docs)
    inner, whole = S.matches(b"$[*]"), pointer_model.columns(S.parsed, [b""])
    keep = inner[0] == ord("{")  # the two objects of the second document
    roots = (np.concatenate([inner[0][keep], whole[0][0]]), np.concatenate([inner[1][keep], whole[1][0]]))
    assert [chr(t) for t in roots[0]] == ["{", "{", "{", "[", "{"]
    at = int(roots[1][0]) & 0xFFFFFFFF
    assert (int(S.tape[at]) >> 56, fields_model.count_field(S.tape[at])) == (ord("{"), 3)
    plain = emu(S, roots)
    for count, want_counts, want_tags in ((0xFFFFFF, 3, "l[\""), (5, 5, "l[\"\x14\x14"), (2, 2, "l["), (0, 0, "")):
        P = S.patched(at, count)
        for capacity in (EXACT, ONE_SHORT, NONE):
            status, offsets, key_tags, key_values, tags, values = emu(P, roots, capacity)
        assert int(offsets[1]) == want_counts and bytes(tags[:want_counts]).decode("latin1") == want_tags
        assert np.array_equal(tags[want_counts:], plain[4][3:]) and np.array_equal(key_values[want_counts:], plain[3][3:])  # the neighbours are what they were
        if count == 5:
            assert key_tags[3:5].tolist() == [20, 20] and key_values[3:5].tolist() == [0, 0] and values[3:5].tolist() == [0, 0]
