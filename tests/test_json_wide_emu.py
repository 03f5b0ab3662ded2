"""CPU tier: cells as JSON text, breadth first -- the gfx950 kernel sources of sjgpu_json_wide.hip with the narrow count of sjgpu_json.hip, k_rows_locate of
sjgpu_query.hip and the scans of sjgpu_finish.hip, compiled as C++ against tests/host/emu -- run the launches of sjgpu_serialize_cells_wide_device
(tests/host/test_json_wide_emu.cpp) and are compared byte for byte with tests/json_text_model.py and, through it, with tests/golden/json_text.json.  The cases of
tests/test_json_emu.py through the wide call (tests/json_text_cases.py, imported), and the ones of tests/json_wide_cases.py that only a call with one lane per tape
word can get wrong.  The driver also runs built with -fsanitize=address,undefined."""
import os
import subprocess

import numpy as np
import pytest

import checkers
import json_text_cases
import json_text_model
import json_wide_cases
import path_model
from json_text_cases import DEPTHS, MAX_DEPTH, ROW_COUNTS
from simdjson_amd import _paths
from test_json_emu import BADARG, EXACT, NONE, ONE_SHORT, OVERFLOW, blob_of, compare, parsed_stream, records_of

CSRC = os.path.join(_paths.PKG_DIR, "csrc")
EMU = os.path.join(_paths.REPO_ROOT, "tests", "host", "emu")
KERNEL_TUS = ("sjgpu_json_wide", "sjgpu_json", "sjgpu_query", "sjgpu_finish")
RANGE = -8


def build(out, sanitize=()):
    """the way tests/test_json_emu.py builds its units"""
    inc = ["-I", EMU, "-I", _paths.INCLUDE_DIR, "-I", CSRC]
    jobs = []
    for name in KERNEL_TUS:
        jobs.append(subprocess.Popen(["g++", "-std=c++17", "-O2", *sanitize, "-Wno-attributes", "-Wno-unknown-pragmas", "-x", "c++", *inc, "-c", os.path.join(CSRC, name + ".hip"),
                                      "-o", str(out / (name + ".o"))]))
    jobs.append(subprocess.Popen(["g++", "-std=c++17", "-O2", *sanitize, *inc, "-c", os.path.join(EMU, "sj_emu.cpp"), "-o", str(out / "sj_emu.o")]))
    jobs.append(subprocess.Popen(["g++", "-std=c++17", "-O2", *sanitize, "-Wno-attributes", *inc, "-c", os.path.join(_paths.REPO_ROOT, "tests", "host", "test_json_wide_emu.cpp"),
                                  "-o", str(out / "driver.o")]))
    assert all(j.wait() == 0 for j in jobs)
    exe = str(out / "test_json_wide_emu")
    subprocess.run(["g++", *sanitize, *[str(out / (f + ".o")) for f in (*KERNEL_TUS, "sj_emu", "driver")], "-lpthread", "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build(tmp_path_factory.mktemp("json_wide_emu"))


@pytest.fixture(scope="module")
def emu(exe):
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


# ---- the narrow call's cases ------------------------------------------------------------------------------------------------------------------------------------
def test_the_fixture_rows(emu, fixture_rows):
    for c, stream, row in fixture_rows:
        offsets, chars, status = emu(stream, row)
        assert not status.any()
        json_text_cases.assert_texts_are_the_fixtures(c, json_text_cases.split(offsets, chars))


def test_the_capacities(emu, fixture_rows):
    for c, stream, row in fixture_rows:
        if c["path"] in (b"$.statuses[*].entities", b"$.statuses[*].id", b"$[*]", b"$", b"$.statuses[*].no_such_field"):
            for capacity in (ONE_SHORT, NONE):
                emu(stream, row, capacity)


@pytest.mark.parametrize("rows", ROW_COUNTS)
def test_rows_at_the_wave_and_workgroup_edges(emu, orc, rows):
    """the narrow test's rows: `rows` cells drawn from the values and the nested values of three documents, every fifth one a cell that is refused"""
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
    hand = [s for c, s, _ in fixture_rows if c["document"] == 2][0]
    root = json_text_cases.root_row(*hand)
    cells = json_text_cases.every_kind_of_cell(len(hand[1]), (int(root[0][0]), int(root[1][0])))
    row = (np.array([t for t, _, _ in cells], np.uint8), np.array([v for _, v, _ in cells], np.uint64))
    offsets, chars, status = emu(hand, row)
    assert [(s == 0) for s in status.tolist()] == [served for _, _, served in cells]
    assert status.tolist().count(17) == 1 and status.tolist().count(19) == 1 and status.tolist().count(22) == 1
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
        offsets, chars, status = emu(stream, row, capacity)
    assert not status.any() and len(row[0]) > 70


@pytest.mark.parametrize("depth", DEPTHS)
def test_nesting_on_both_sides_of_the_hand_off(emu, orc, depth):
    """63 levels below the root stay with the scans, 64 and more go to the one-lane walk; a document of depth - 1 and an empty array ride in the same row"""
    doc = json_text_cases.deep_document(depth)
    stream = parsed_stream(orc, [doc, json_text_cases.deep_document(depth - 1), b"[]"], MAX_DEPTH)
    offsets, chars, status = emu(stream, json_text_cases.root_row(*stream))
    assert not status.any() and chars.startswith(doc) and len(chars) == len(doc) + len(json_text_cases.deep_document(depth - 1)) + 2


def test_broken_sub_tapes(emu, fixture_rows):
    hand = [s for c, s, _ in fixture_rows if c["document"] == 2][0]
    root = json_text_cases.root_row(*hand)
    assert not emu(hand, root)[2].any()
    for what, broken in json_text_cases.broken_tapes(hand[0], hand[2]):
        for capacity in (EXACT, NONE):
            offsets, chars, status = emu((broken, hand[1], hand[2]), root, capacity)
            assert status.tolist() == [20] and offsets.tolist() == [0, 0] and chars == b"", what


# ---- what one lane per tape word can get wrong -------------------------------------------------------------------------------------------------------------------
def test_the_same_container_twice_and_a_container_beside_its_own_child(emu, orc):
    stream = parsed_stream(orc, [json_wide_cases.NESTED_DOCUMENT])
    row = json_wide_cases.overlapping_row(stream)
    offsets, chars, status = emu(stream, row)
    texts = json_text_cases.split(offsets, chars)
    assert not status.any() and texts[0] == texts[1] == json_wide_cases.NESTED_DOCUMENT and texts[2] in texts[0] and texts[3] == texts[0]
    emu(stream, row, ONE_SHORT)


@pytest.mark.parametrize("words", json_wide_cases.SHARE_EDGE_WORDS)
def test_documents_at_the_edges_of_the_shares(emu, orc, words):
    """A lane's share of every kernel of the wide call is ONE slot, a wave's 64, a workgroup's 256 (sjgpu_json_wide.hip: JW_THREADS); the kernels over the slots and the
    settle kernel, which has one slot more, stand on the same edges.  A container has at least two words, so a lane's share is met by [] alone; the roots here have
    63 / 64 / 65 and 255 / 256 / 257 words (and 511 / 512 / 513: two workgroups), once at slot 0 and once behind a scalar's slot, which moves every edge by one."""
    stream = parsed_stream(orc, [json_wide_cases.document_of_words(words), b"[]"])
    root = json_text_cases.root_row(*stream)
    assert int(root[1][0] >> np.uint64(32)) - int(root[1][0] & np.uint64(0xFFFFFFFF)) == words
    offsets, chars, status = emu(stream, root)
    assert not status.any()
    shifted = (np.concatenate([np.array([ord("t")], np.uint8), root[0], root[0]]), np.concatenate([np.array([1], np.uint64), root[1], root[1]]))
    emu(stream, shifted)


def test_an_object_whose_fields_cross_two_workgroups(emu, orc):
    """more fields than two workgroups' shares: whether a string is a key is a parity carried across the workgroups"""
    doc = json_wide_cases.wide_object(300)
    stream = parsed_stream(orc, [doc])
    root = json_text_cases.root_row(*stream)
    assert int(root[1][0] >> np.uint64(32)) - int(root[1][0] & np.uint64(0xFFFFFFFF)) > 3 * 256
    offsets, chars, status = emu(stream, root)
    assert not status.any() and chars == doc


@pytest.mark.parametrize("slot", json_wide_cases.BORDER_SLOTS)
def test_a_number_whose_second_word_looks_like_a_tag_at_a_share_border(emu, orc, slot):
    """the second word of an `l` with 0x7B / 0x5D / 0x6C on top ({ ] l) as the last slot of a share and as the first of the next"""
    for value in json_wide_cases.TAG_LIKE_INTEGERS:
        doc = json_wide_cases.number_at_slot(slot, value)
        stream = parsed_stream(orc, [doc])
        root = json_text_cases.root_row(*stream)
        low = int(root[1][0] & np.uint64(0xFFFFFFFF))
        assert int(stream[0][low + slot]) == value and chr(int(stream[0][low + slot - 1]) >> 56) == "l"
        offsets, chars, status = emu(stream, root)
        assert not status.any() and chars == doc


def test_empty_containers_as_first_middle_and_last_children(emu, orc):
    stream = parsed_stream(orc, json_wide_cases.EMPTY_CONTAINER_DOCUMENTS)
    offsets, chars, status = emu(stream, json_text_cases.root_row(*stream))
    assert not status.any() and json_text_cases.split(offsets, chars) == json_wide_cases.EMPTY_CONTAINER_DOCUMENTS


def test_the_range_refusal(exe, orc):
    """65 537 roots over one array of 32 767 ones (65 536 words): 2^32 + 65 536 slots.  status complete (the narrow count's), offsets and characters untouched (the driver
    checks the poison), nothing reported"""
    stream, row = json_wide_cases.range_refusal(orc, parsed_stream)
    p = subprocess.run([exe], input=blob_of(stream, row, EXACT), capture_output=True, timeout=1500)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-3000:]
    (code, total, offsets, status, chars), = records_of(p.stdout, [len(row[0])])
    assert code == RANGE and total == 0 and chars == b"" and not status.any() and len(status) == 65537
    assert (offsets == 0x5A5A5A5A).all()
    # one root fewer is served
    fewer = (row[0][:3], row[1][:3])
    p = subprocess.run([exe], input=blob_of(stream, fewer, NONE), capture_output=True, timeout=1500)
    (code, total, offsets, status, chars), = records_of(p.stdout, [3])
    assert code == OVERFLOW and total == 3 * (2 * 32767 + 1)


def test_the_driver_runs_clean_under_the_sanitizers(tmp_path, orc, fixture_rows):
    """the stand-alone driver -- kernels and launchers -- built with -fsanitize=address,undefined: the narrow test's calls and the new cases but the refusal"""
    exe = build(tmp_path, ("-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer", "-g"))
    capacities = (EXACT, ONE_SHORT, NONE)
    calls = [(stream, row, cap) for c, stream, row in fixture_rows if c["document"] == 2 or c["path"] in (b"$.statuses[*].entities", b"$.search_metadata") for cap in capacities]
    deep = parsed_stream(orc, [json_text_cases.deep_document(70), json_text_cases.strings_document(), json_text_cases.deep_document(63)], MAX_DEPTH)
    calls.append((deep, json_text_cases.root_row(*deep), EXACT))
    hand = [s for c, s, _ in fixture_rows if c["document"] == 2][0]
    root = json_text_cases.root_row(*hand)
    cells = json_text_cases.every_kind_of_cell(len(hand[1]), (int(root[0][0]), int(root[1][0])))
    calls.append((hand, (np.array([t for t, _, _ in cells], np.uint8), np.array([v for _, v, _ in cells], np.uint64)), EXACT))
    calls += [((broken, hand[1], hand[2]), root, EXACT) for _, broken in json_text_cases.broken_tapes(hand[0], hand[2])]
    nested = parsed_stream(orc, [json_wide_cases.NESTED_DOCUMENT])
    calls.append((nested, json_wide_cases.overlapping_row(nested), EXACT))
    for doc in (json_wide_cases.document_of_words(257), json_wide_cases.wide_object(300), json_wide_cases.number_at_slot(256, json_wide_cases.TAG_LIKE_INTEGERS[0])):
        stream = parsed_stream(orc, [doc])
        calls.append((stream, json_text_cases.root_row(*stream), EXACT))
    empties = parsed_stream(orc, json_wide_cases.EMPTY_CONTAINER_DOCUMENTS)
    calls.append((empties, json_text_cases.root_row(*empties), ONE_SHORT))
    blob = b"".join(blob_of(stream, row, cap) for stream, row, cap in calls)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe], input=blob, capture_output=True, timeout=1500, env=env)
    assert p.returncode == 0 and b"runtime error" not in p.stderr and b"AddressSanitizer" not in p.stderr, p.stderr.decode(errors="replace")[-3000:]
    got = records_of(p.stdout, [len(row[0]) for _, row, _ in calls])
    for record, (stream, row, cap) in zip(got, calls):
        compare(record, json_text_model.column(json_text_model.Stream(*stream), row), cap)
    assert OVERFLOW in [g[0] for g in got] and 0 in [g[0] for g in got] and BADARG not in [g[0] for g in got]
