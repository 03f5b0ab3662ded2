"""CPU tier: cells as indented JSON text -- the gfx950 kernel sources of sjgpu_json.hip, their PRETTY instantiations, with k_rows_locate of sjgpu_query.hip and the scans
of sjgpu_finish.hip, compiled as C++ against tests/host/emu -- run the launches of sjgpu_prettify_cells_device (tests/host/test_pretty_emu.cpp) and are compared byte
for byte with tests/pretty_model.py and, through it, with tests/golden/pretty.json (the real reference's simdjson::prettify): the fixture's rows -- the chains on either
side of the 16th, 32nd, ... level among them --, rows at the wave's and the workgroup's edges, every kind of root, strings of every length, nesting on both sides of
the bit stack's spill, a flat container of more children than a workgroup has lanes, tapes broken on purpose, the three capacities, and a total beyond 32 bits.  The
driver also runs built with -fsanitize=address,undefined, as a program of its own.

tests/test_pretty_wide_emu.py imports the tests below and runs them through the wide call's driver: the two calls have one contract."""
import os
import subprocess

import numpy as np
import pytest

import checkers
import json_text_cases
import path_model
import pretty_cases
import pretty_model
import rows_model
from json_text_cases import DEPTHS, MAX_DEPTH, ROW_COUNTS
from simdjson_amd import _paths
from test_json_emu import EXACT, NONE, ONE_SHORT, OVERFLOW, blob_of, compare, parsed_stream, records_of

CSRC = os.path.join(_paths.PKG_DIR, "csrc")
EMU = os.path.join(_paths.REPO_ROOT, "tests", "host", "emu")
KERNEL_TUS = ("sjgpu_json", "sjgpu_query", "sjgpu_finish")
DRIVER = "test_pretty_emu"
CAPACITY = 1
SANITIZE = ("-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer", "-g")
FLAT_CHILDREN = 307  # more than a workgroup's 256 lanes


def build(out, driver=DRIVER, tus=KERNEL_TUS, sanitize=()):
    """the way tests/test_json_emu.py builds its units"""
    inc = ["-I", EMU, "-I", _paths.INCLUDE_DIR, "-I", CSRC]
    jobs = []
    for name in tus:
        jobs.append(subprocess.Popen(["g++", "-std=c++17", "-O2", *sanitize, "-Wno-attributes", "-Wno-unknown-pragmas", "-x", "c++", *inc, "-c", os.path.join(CSRC, name + ".hip"),
                                      "-o", str(out / (name + ".o"))]))
    jobs.append(subprocess.Popen(["g++", "-std=c++17", "-O2", *sanitize, *inc, "-c", os.path.join(EMU, "sj_emu.cpp"), "-o", str(out / "sj_emu.o")]))
    jobs.append(subprocess.Popen(["g++", "-std=c++17", "-O2", *sanitize, "-Wno-attributes", *inc, "-c", os.path.join(_paths.REPO_ROOT, "tests", "host", driver + ".cpp"),
                                  "-o", str(out / "driver.o")]))
    assert all(j.wait() == 0 for j in jobs)
    exe = str(out / driver)
    subprocess.run(["g++", *sanitize, *[str(out / (f + ".o")) for f in (*tus, "sj_emu", "driver")], "-lpthread", "-o", exe], check=True)
    return exe


def runner(exe):
    def run(stream, row, capacity=EXACT):
        """-> the model's (offsets, chars, status); everything the driver wrote is compared with the model here"""
        p = subprocess.run([exe], input=blob_of(stream, row, capacity), capture_output=True, timeout=1500)
        assert p.returncode == 0, p.stderr.decode(errors="replace")[-3000:]
        record, = records_of(p.stdout, [len(row[0])])
        want = pretty_model.column(pretty_model.Stream(*stream), row)
        compare(record, want, capacity)
        return want
    run.exe = exe
    return run


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return runner(build(tmp_path_factory.mktemp("pretty_emu")))


@pytest.fixture(scope="module")
def orc():
    return checkers.Oracle()


@pytest.fixture(scope="module")
def fixture_rows(orc):
    return pretty_cases.fixture_rows(orc)


def hand_made(fixture_rows):
    return [s for c, s, _ in fixture_rows if c["document"] == 2][0]


def test_the_fixture_rows(emu, fixture_rows):
    """every row of the fixture, cell by cell the reference's text: the fourteen cases of the minify fixture and the 96 chains, a column of twelve per level"""
    assert len(fixture_rows) == 14 + len(pretty_cases.CHAIN_LEVELS) and sum(len(row[0]) for _, _, row in fixture_rows[14:]) == len(pretty_cases.chains())
    for c, stream, row in fixture_rows:
        offsets, chars, status = emu(stream, row)
        assert not status.any()
        texts = json_text_cases.split(offsets, chars)
        pretty_cases.assert_texts_are_the_fixtures(c, texts)
        assert all(t.endswith(b"\n") and not t.endswith(b"\n\n") for t in texts)


def test_the_capacities(emu, fixture_rows):
    for c, stream, row in fixture_rows:
        if c["path"] in (b"$.statuses[*].entities", b"$.statuses[*].id", b"$[*]", b"$.statuses[*].no_such_field") or c["document"] in (2, 3 + 2, 3 + 7):
            for capacity in (ONE_SHORT, NONE):
                emu(stream, row, capacity)


def test_the_chains_in_one_row(emu, orc):
    """all the chains as one stream, a root per document: restarts at different depths side by side in one wave"""
    stream = parsed_stream(orc, pretty_cases.chains())
    for capacity in (EXACT, ONE_SHORT, NONE):
        offsets, chars, status = emu(stream, json_text_cases.root_row(*stream), capacity)
    assert not status.any()


@pytest.mark.parametrize("rows", ROW_COUNTS)
def test_rows_at_the_wave_and_workgroup_edges(emu, orc, rows):
    """`rows` cells drawn from the values and the nested values of a stream of three documents, every fifth one a cell that is refused (length 0, no newline)"""
    docs, _ = pretty_cases.fixture()
    stream = parsed_stream(orc, [docs[2], pretty_cases.chain(17, b'{"a":[1,{}]}', 1), b'{"a":[1,2.5,{"b":null}],"c":"d"}'])
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
    assert all(int(offsets[i + 1]) == int(offsets[i]) for i in range(0, rows, 5))


def test_every_kind_of_root(emu, orc, fixture_rows):
    """every scalar from the cell alone and a newline, every code forwarded, bytes that are neither, string cells outside the buffer, container cells that disagree"""
    hand = hand_made(fixture_rows)
    root = json_text_cases.root_row(*hand)
    cells = json_text_cases.every_kind_of_cell(len(hand[1]), (int(root[0][0]), int(root[1][0])))
    row = (np.array([t for t, _, _ in cells], np.uint8), np.array([v for _, v, _ in cells], np.uint64))
    offsets, chars, status = emu(hand, row)
    assert [(s == 0) for s in status.tolist()] == [served for _, _, served in cells]
    texts = json_text_cases.split(offsets, chars)
    assert texts[0] == b"true\n" and texts[3] == b"0\n" and all((t == b"") == (s != 0) for t, s in zip(texts, status.tolist()))
    emu(hand, row, ONE_SHORT)
    empty = (np.zeros(0, np.uint64), hand[1], np.zeros(1, hand[2].dtype))  # no document at all: scalars are served, containers have no tape to agree with
    offsets, chars, status = emu(empty, row)
    assert [(s == 0) for s in status.tolist()] == [served and chr(t) not in "{[" for t, _, served in cells]


def test_strings_of_every_length_and_byte(emu, orc):
    stream = parsed_stream(orc, [json_text_cases.strings_document()])
    emu(stream, json_text_cases.root_row(*stream))
    _, found = path_model.matches(stream[0].tolist(), stream[1].tobytes(), b"$[*]", 0, 0)
    row = (np.array([t for t, _ in found], np.uint8), np.array([v for _, v in found], np.uint64))
    for capacity in (EXACT, ONE_SHORT):
        offsets, chars, status = emu(stream, row, capacity)  # each string a root of its own: "..." and a newline
    assert not status.any() and len(row[0]) > 70


@pytest.mark.parametrize("depth", DEPTHS)
def test_nesting_on_both_sides_of_the_spill_and_the_hand_off(emu, orc, depth):
    """63 levels stay in the register (and with the wide call's scans), 64 and more spill (and go to the one-lane walk); a restart falls inside every one of them"""
    doc = json_text_cases.deep_document(depth)
    stream = parsed_stream(orc, [doc, json_text_cases.deep_document(depth - 1), b"[]"], MAX_DEPTH)
    offsets, chars, status = emu(stream, json_text_cases.root_row(*stream))
    assert not status.any() and chars.endswith(b"[]\n") and b"\n" + b" " * 60 + b'"' in chars and b" " * 61 not in chars


@pytest.mark.parametrize("as_object", [False, True])
def test_a_flat_container_of_more_children_than_a_workgroup(emu, orc, as_object):
    doc = pretty_cases.flat_container_of(FLAT_CHILDREN, as_object)
    stream = parsed_stream(orc, [doc, b"[]"])
    for capacity in (EXACT, ONE_SHORT):
        offsets, chars, status = emu(stream, json_text_cases.root_row(*stream), capacity)
    assert not status.any() and (b',"k306":306\n}' if as_object else b',"v301"\n,[]\n,') in chars


def test_broken_sub_tapes(emu, fixture_rows):
    hand = hand_made(fixture_rows)
    root = json_text_cases.root_row(*hand)
    assert not emu(hand, root)[2].any()
    for what, broken in json_text_cases.broken_tapes(hand[0], hand[2]):
        for capacity in (EXACT, NONE):
            offsets, chars, status = emu((broken, hand[1], hand[2]), root, capacity)
            assert status.tolist() == [20] and offsets.tolist() == [0, 0] and chars == b"", what


def test_a_total_beyond_32_bits(emu, orc):
    """CAPACITY asked with no capacity: the same 2 MB root until the total passes 2^32.  The 64-bit total is the model's arithmetic: one root's length times the rows"""
    stream = parsed_stream(orc, [pretty_cases.CAPACITY_DOCUMENT])
    tag, value = rows_model.root_cell(*stream, 0)
    one = pretty_model.text_bytes(pretty_model.Stream(*stream), (tag, value))
    n = pretty_cases.CAPACITY_ONES
    # the elements (the first has no comma); 15 brackets that open and 15 that close, each behind a newline and its indent -- but for the root's, which has none in front
    # and one behind
    assert one == 63 * n - 1 + 2 * sum(2 + 4 * a for a in range(15))
    rows = pretty_cases.CAPACITY_ROWS
    assert (rows - 1) * one < (1 << 32) < rows * one
    row = (np.full(rows, tag, np.uint8), np.full(rows, value, np.uint64))
    p = subprocess.run([emu.exe], input=blob_of(stream, row, NONE), capture_output=True, timeout=1500)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-3000:]
    (code, total, offsets, status, chars), = records_of(p.stdout, [rows])
    assert code == CAPACITY and total == rows * one and chars == b"" and not status.any()
    fewer = (row[0][:3], row[1][:3])
    p = subprocess.run([emu.exe], input=blob_of(stream, fewer, NONE), capture_output=True, timeout=1500)
    (code, total, offsets, status, chars), = records_of(p.stdout, [3])
    assert code == OVERFLOW and total == 3 * one and offsets.tolist() == [0, one, 2 * one, 3 * one]


def sanitizer_calls(orc, fixture_rows):
    """what the driver built with the sanitizers is given: the hand-made document's rows and a few chains at all three capacities, a deep document on the far side of the
    spill, the strings, every kind of root, the broken tapes and a flat container"""
    capacities = (EXACT, ONE_SHORT, NONE)
    calls = [(stream, row, cap) for c, stream, row in fixture_rows if c["document"] in (2, 3 + 2, 3 + 5, 3 + 7) or c["path"] == b"$.search_metadata"
             for cap in capacities]
    deep = parsed_stream(orc, [json_text_cases.deep_document(70), json_text_cases.strings_document(), json_text_cases.deep_document(63)], MAX_DEPTH)
    calls.append((deep, json_text_cases.root_row(*deep), EXACT))
    hand = hand_made(fixture_rows)
    root = json_text_cases.root_row(*hand)
    cells = json_text_cases.every_kind_of_cell(len(hand[1]), (int(root[0][0]), int(root[1][0])))
    calls.append((hand, (np.array([t for t, _, _ in cells], np.uint8), np.array([v for _, v, _ in cells], np.uint64)), EXACT))
    calls += [((broken, hand[1], hand[2]), root, EXACT) for _, broken in json_text_cases.broken_tapes(hand[0], hand[2])]
    flat = parsed_stream(orc, [pretty_cases.flat_container_of(FLAT_CHILDREN, True), pretty_cases.flat_container_of(5)])
    calls.append((flat, json_text_cases.root_row(*flat), EXACT))
    return calls


def run_under_the_sanitizers(exe, calls):
    blob = b"".join(blob_of(stream, row, cap) for stream, row, cap in calls)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe], input=blob, capture_output=True, timeout=1500, env=env)
    assert p.returncode == 0 and b"runtime error" not in p.stderr and b"AddressSanitizer" not in p.stderr, p.stderr.decode(errors="replace")[-3000:]
    got = records_of(p.stdout, [len(row[0]) for _, row, _ in calls])
    for record, (stream, row, cap) in zip(got, calls):
        compare(record, pretty_model.column(pretty_model.Stream(*stream), row), cap)
    assert OVERFLOW in [g[0] for g in got] and 0 in [g[0] for g in got]


def test_the_driver_runs_clean_under_the_sanitizers(tmp_path, orc, fixture_rows):
    """the stand-alone driver -- kernels and launchers -- built with -fsanitize=address,undefined (the runtimes linked statically: the program stands alone)"""
    run_under_the_sanitizers(build(tmp_path, sanitize=SANITIZE), sanitizer_calls(orc, fixture_rows))
