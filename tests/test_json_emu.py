"""CPU tier: cells as JSON text -- the gfx950 kernel sources of sjgpu_json.hip with k_rows_locate of sjgpu_query.hip and the scans of sjgpu_finish.hip, compiled as
C++ against tests/host/emu -- run the launches of sjgpu_serialize_cells_device (tests/host/test_json_emu.cpp) and are compared byte for byte with
tests/json_text_model.py and, through it, with tests/golden/json_text.json: the fixture's rows, rows at the wave's and the workgroup's edges, every kind of root,
strings of every length and byte, nesting on both sides of the bit stack's spill, tapes broken on purpose, and the three capacities.  The driver also runs built
with -fsanitize=address,undefined."""
import os
import struct
import subprocess

import numpy as np
import pytest

import checkers
import json_text_cases
import json_text_model
import path_model
from json_text_cases import DEPTHS, MAX_DEPTH, ROW_COUNTS
from simdjson_amd import _paths

CSRC = os.path.join(_paths.PKG_DIR, "csrc")
EMU = os.path.join(_paths.REPO_ROOT, "tests", "host", "emu")
KERNEL_TUS = ("sjgpu_json", "sjgpu_query", "sjgpu_finish")
EXACT, ONE_SHORT, NONE = 0, 1, 2
OVERFLOW, BADARG = -5, -2


def build(out, sanitize=()):
    """the way tests/test_dict_emu.py builds its units"""
    inc = ["-I", EMU, "-I", _paths.INCLUDE_DIR, "-I", CSRC]
    jobs = []
    for name in KERNEL_TUS:
        jobs.append(subprocess.Popen(["g++", "-std=c++17", "-O2", *sanitize, "-Wno-attributes", "-Wno-unknown-pragmas", "-x", "c++", *inc, "-c", os.path.join(CSRC, name + ".hip"),
                                      "-o", str(out / (name + ".o"))]))
    jobs.append(subprocess.Popen(["g++", "-std=c++17", "-O2", *sanitize, *inc, "-c", os.path.join(EMU, "sj_emu.cpp"), "-o", str(out / "sj_emu.o")]))
    jobs.append(subprocess.Popen(["g++", "-std=c++17", "-O2", *sanitize, "-Wno-attributes", *inc, "-c", os.path.join(_paths.REPO_ROOT, "tests", "host", "test_json_emu.cpp"),
                                  "-o", str(out / "driver.o")]))
    assert all(j.wait() == 0 for j in jobs)
    exe = str(out / "test_json_emu")
    subprocess.run(["g++", *sanitize, *[str(out / (f + ".o")) for f in (*KERNEL_TUS, "sj_emu", "driver")], "-lpthread", "-o", exe], check=True)
    return exe


def blob_of(stream, row, capacity):
    tape, sbuf, table = stream
    tape, sbuf = np.ascontiguousarray(tape, np.uint64), np.ascontiguousarray(sbuf, np.uint8)
    tags, values = np.ascontiguousarray(row[0], np.uint8), np.ascontiguousarray(row[1], np.uint64)
    assert len(tags) == len(values)
    return (struct.pack("<Q", len(tape)) + tape.tobytes() + struct.pack("<Q", len(sbuf)) + sbuf.tobytes() + struct.pack("<I", len(table) - 1) + table.tobytes() +
            struct.pack("<I", len(tags)) + tags.tobytes() + values.tobytes() + struct.pack("<I", capacity))


def records_of(out, rows_per_call):
    """the driver's records -> [(code, bytes, offsets, status, chars)]"""
    at, got = 0, []
    for rows in rows_per_call:
        code, total = struct.unpack_from("<iQ", out, at)
        at += 12
        assert code != BADARG
        offsets = np.frombuffer(out, np.uint32, rows + 1, at)
        at += 4 * (rows + 1)
        status = np.frombuffer(out, np.uint8, rows, at)
        at += rows
        written = 0 if code else total
        got.append((code, total, offsets, status, out[at: at + written]))
        at += written
    assert at == len(out)
    return got


def compare(record, want, capacity):
    code, total, offsets, status, chars = record
    want_offsets, want_chars, want_status = want
    assert total == len(want_chars) and np.array_equal(offsets, want_offsets) and np.array_equal(status, want_status)  # (whatever the capacity)
    if capacity == EXACT or total == 0:
        assert code == 0 and chars == want_chars
    else:  # the texts do not fit: offsets and status complete, nothing written (the driver checks that), the total reported
        assert code == OVERFLOW and chars == b""


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    exe = build(tmp_path_factory.mktemp("json_emu"))

    def run(stream, row, capacity=EXACT):
        """-> the model's (offsets, chars, status); everything the driver wrote is compared with the model here"""
        p = subprocess.run([exe], input=blob_of(stream, row, capacity), capture_output=True, timeout=1500)
        assert p.returncode == 0, p.stderr.decode(errors="replace")[-3000:]
        record, = records_of(p.stdout, [len(row[0])])
        want = json_text_model.column(json_text_model.Stream(*stream), row)
        compare(record, want, capacity)
        return want
    return run


@pytest.fixture(scope="module")
def orc():
    return checkers.Oracle()


@pytest.fixture(scope="module")
def fixture_rows(orc):
    return json_text_cases.fixture_rows(orc)


def parsed_stream(orc, docs, max_depth=1024):
    parsed = []
    for d in docs:
        err, tape, sbuf = orc.dom_parse(d, max_depth=max_depth)
        assert err == 0
        parsed.append((tape, sbuf))
    return json_text_cases.stream_of(parsed)


def test_the_fixture_rows(emu, fixture_rows):
    """every row of the fixture, cell by cell the reference's text (the model is pinned against the fixture by tests/test_json_text_model.py; here the fixture is asked again)"""
    for c, stream, row in fixture_rows:
        offsets, chars, status = emu(stream, row)
        assert not status.any()
        json_text_cases.assert_texts_are_the_fixtures(c, json_text_cases.split(offsets, chars))


def test_the_capacities(emu, fixture_rows):
    for c, stream, row in fixture_rows:
        if c["path"] in (b"$.statuses[*].entities", b"$.statuses[*].id", b"$[*]", b"$", b"$.statuses[*].no_such_field"):
            for capacity in (ONE_SHORT, NONE):
                emu(stream, row, capacity)


def test_the_driver_runs_clean_under_the_sanitizers(tmp_path, orc, fixture_rows):
    """the stand-alone driver -- kernels and launchers -- built with -fsanitize=address,undefined: the fixture's small rows at all three capacities, every kind of root, a
    deep document on the far side of the spill and the broken tapes"""
    # (the runtimes linked statically: the program stands alone, whatever else the loader is told to bring in)
    exe = build(tmp_path, ("-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer", "-g"))
    capacities = (EXACT, ONE_SHORT, NONE)
    calls = [(stream, row, cap) for c, stream, row in fixture_rows if c["document"] == 2 or c["path"] in (b"$.statuses[*].entities", b"$.search_metadata") for cap in capacities]
    deep = parsed_stream(orc, [json_text_cases.deep_document(70), json_text_cases.strings_document()], MAX_DEPTH)
    calls.append((deep, json_text_cases.root_row(*deep), EXACT))
    hand = [s for c, s, _ in fixture_rows if c["document"] == 2][0]
    root = json_text_cases.root_row(*hand)
    cells = json_text_cases.every_kind_of_cell(len(hand[1]), (int(root[0][0]), int(root[1][0])))
    calls.append((hand, (np.array([t for t, _, _ in cells], np.uint8), np.array([v for _, v, _ in cells], np.uint64)), EXACT))
    calls += [((broken, hand[1], hand[2]), root, EXACT) for _, broken in json_text_cases.broken_tapes(hand[0], hand[2])]
    blob = b"".join(blob_of(stream, row, cap) for stream, row, cap in calls)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe], input=blob, capture_output=True, timeout=1500, env=env)
    assert p.returncode == 0 and b"runtime error" not in p.stderr and b"AddressSanitizer" not in p.stderr, p.stderr.decode(errors="replace")[-3000:]
    got = records_of(p.stdout, [len(row[0]) for _, row, _ in calls])
    for record, (stream, row, cap) in zip(got, calls):
        compare(record, json_text_model.column(json_text_model.Stream(*stream), row), cap)
    assert OVERFLOW in [g[0] for g in got] and 0 in [g[0] for g in got]


@pytest.mark.parametrize("rows", ROW_COUNTS)
def test_rows_at_the_wave_and_workgroup_edges(emu, orc, rows):
    """`rows` cells drawn from the values and the nested values of a stream of three documents, every fifth one a cell that is refused"""
    docs, _, _ = json_text_cases.fixture()
    stream = parsed_stream(orc, [docs[2], json_text_cases.deep_document(5), b'{"a":[1,2.5,{"b":null}],"c":"d"}'])
    pool_tags, pool_values = [], []
    for path in (b"$[*]", b"$[*][*]", b"$.*", b"$.*.*"):
        for d in range(3):
            tb, te = int(stream[2]["tape_begin"][d]), int(stream[2]["tape_begin"][d + 1])
            sb, se = int(stream[2]["string_begin"][d]), int(stream[2]["string_begin"][d + 1])
            code, found = path_model.matches(stream[0][tb:te].tolist(), stream[1][sb:se].tobytes(), path, tb, sb)
            pool_tags += [t for t, _ in found]
            pool_values += [v for _, v in found]
    assert len(pool_tags) > 60
    rng = np.random.default_rng(300 + rows)
    pick = rng.integers(0, len(pool_tags), rows)
    tags, values = np.array(pool_tags, np.uint8)[pick], np.array(pool_values, np.uint64)[pick]
    root = json_text_cases.root_row(*stream)
    bad = [(t, v) for t, v, served in json_text_cases.every_kind_of_cell(len(stream[1]), (int(root[0][0]), int(root[1][0]))) if not served]
    for k, i in enumerate(range(0, rows, 5)):
        tags[i], values[i] = bad[k % len(bad)]
    for capacity in (EXACT, ONE_SHORT, NONE):
        offsets, chars, status = emu(stream, (tags, values), capacity)
    assert (status[::5] != 0).all() and (rows < 2 or not status[1]) and len(offsets) == rows + 1


def test_every_kind_of_root(emu, orc, fixture_rows):
    """every scalar from the cell alone, every code forwarded, bytes that are neither, string cells outside the buffer, container cells that disagree with the tape"""
    hand = [s for c, s, _ in fixture_rows if c["document"] == 2][0]
    root = json_text_cases.root_row(*hand)
    cells = json_text_cases.every_kind_of_cell(len(hand[1]), (int(root[0][0]), int(root[1][0])))
    row = (np.array([t for t, _, _ in cells], np.uint8), np.array([v for _, v, _ in cells], np.uint64))
    offsets, chars, status = emu(hand, row)
    assert [(s == 0) for s in status.tolist()] == [served for _, _, served in cells]
    assert status.tolist().count(17) == 1 and status.tolist().count(19) == 1 and status.tolist().count(22) == 1
    emu(hand, row, ONE_SHORT)
    # no document at all: scalars are served, containers have no tape to agree with
    empty = (np.zeros(0, np.uint64), hand[1], np.zeros(1, hand[2].dtype))
    offsets, chars, status = emu(empty, row)
    assert [(s == 0) for s in status.tolist()] == [served and chr(t) not in "{[" for t, _, served in cells]


def test_strings_of_every_length_and_byte(emu, orc):
    stream = parsed_stream(orc, [json_text_cases.strings_document()])
    root = json_text_cases.root_row(*stream)
    emu(stream, root)
    _, found = path_model.matches(stream[0].tolist(), stream[1].tobytes(), b"$[*]", 0, 0)
    row = (np.array([t for t, _ in found], np.uint8), np.array([v for _, v in found], np.uint64))
    for capacity in (EXACT, ONE_SHORT):
        offsets, chars, status = emu(stream, row, capacity)  # each string a root of its own: every text's ragged ends meet a neighbour's
    assert not status.any() and len(row[0]) > 70


@pytest.mark.parametrize("depth", DEPTHS)
def test_nesting_on_both_sides_of_the_spill(emu, orc, depth):
    doc = json_text_cases.deep_document(depth)
    stream = parsed_stream(orc, [doc, json_text_cases.deep_document(depth - 1), b"[]"], MAX_DEPTH)
    offsets, chars, status = emu(stream, json_text_cases.root_row(*stream))
    assert not status.any() and chars.startswith(doc) and len(chars) == len(doc) + len(json_text_cases.deep_document(depth - 1)) + 2


def test_broken_sub_tapes(emu, fixture_rows):
    hand = [s for c, s, _ in fixture_rows if c["document"] == 2][0]
    root = json_text_cases.root_row(*hand)
    good = emu(hand, root)
    assert not good[2].any()
    for what, broken in json_text_cases.broken_tapes(hand[0], hand[2]):
        for capacity in (EXACT, NONE):
            offsets, chars, status = emu((broken, hand[1], hand[2]), root, capacity)
            assert status.tolist() == [20] and offsets.tolist() == [0, 0] and chars == b"", what
