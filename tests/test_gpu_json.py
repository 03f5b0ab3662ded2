"""GPU tier (-m gpu): cells as JSON text -- sjgpu_serialize_cells_device (k_rows_locate, k_json_count, k_json_fill; sjgpu_json.hip, include/sjgpu_json.h) and
json_text.json_column_many / documents_as_json_many -- against tests/json_text_model.py (pinned against tests/golden/json_text.json on the CPU tier), the fixture
itself, and the library's own parser: a text that is parsed again gives the tape it came from.  The tapes are the device's own (sjgpu_stage2_many_device, sjgpu_parse),
the rows what sjgpu_at_paths_device and sjgpu_at_pointers_device delivered.  Every output has exactly the contracted size inside a poisoned tensor whose poison is
checked after every call, the status row, the characters and the root tags begin at odd addresses, and every column is made twice: with capacity 0 and a null
chars_dev, then at the capacity that call reported."""
import os

import numpy as np
import pytest

import json_text_cases
import json_text_model
from json_text_cases import DEPTHS, MAX_DEPTH, ROW_COUNTS
from simdjson_amd import _paths, build, capi, json_text
from test_gpu_fields import device_roots, matches
from test_gpu_query import Tapes, query

pytestmark = pytest.mark.gpu

CAP = 128 << 20
E_BADARG, E_OVERFLOW = -4, -5
GUARD = 65  # odd: with it the status row and the characters begin at odd addresses
P32, P8 = 0x5A5A5A5A, 0x5A
EXAMPLES = os.path.join(_paths.REPO_ROOT, "tests", "golden", "jsonexamples")


@pytest.fixture(scope="module")
def parser():
    build.build_sjgpu()
    p = capi.DomParserImplementation(CAP)
    yield p
    p.close()


def call(p, T, roots, cap, null_chars=False, docs=None, offsets_skew=0, root_skew=0, expect=None):
    """one sjgpu_serialize_cells_device over the roots (tags[rows], values[rows]) with outputs of exactly rows + 1 words, rows bytes and `cap` characters between
    poisoned guards -> (rc, bytes, offsets[rows + 1], status[rows], chars: bytes); expect: the rc the caller counts on"""
    torch = T.torch
    root_tags, root_values, d_tags, d_values = device_roots(T, roots)
    rows = len(root_tags)
    offsets = torch.full((rows + 1 + 2 * GUARD,), P32, dtype=torch.int32, device="cuda")
    status = torch.full((rows + 2 * GUARD,), P8, dtype=torch.uint8, device="cuda")
    chars = torch.full((cap + 2 * GUARD,), P8, dtype=torch.uint8, device="cuda")
    rc, total = json_text.serialize_cells_device(p, T.d_tape.data_ptr(), len(T.tape), T.d_sbuf.data_ptr(), len(T.sbuf), T.d_table.data_ptr(), T.docs if docs is None else docs,
                                                 d_values.data_ptr() + root_skew, d_tags.data_ptr() + 1, rows, offsets.data_ptr() + 4 * GUARD + offsets_skew,
                                                 status.data_ptr() + GUARD, 0 if null_chars else chars.data_ptr() + GUARD, cap, T.stream)
    torch.cuda.synchronize()
    if expect is not None:
        assert rc == expect, (rc, expect, p.last_error())
    nothing = rc == E_BADARG
    wrote_offsets, wrote_status = (0, 0) if nothing else (rows + 1, rows)
    wrote = total if rc == 0 else 0
    oh, sh, ch = offsets.cpu().numpy().view(np.uint32), status.cpu().numpy(), chars.cpu().numpy()
    assert (oh[:GUARD] == P32).all() and (oh[GUARD + wrote_offsets:] == P32).all(), "offsets poison"
    assert (sh[:GUARD] == P8).all() and (sh[GUARD + wrote_status:] == P8).all(), "status poison"
    assert not (sh[GUARD: GUARD + wrote_status] == P8).any(), "a status was not written"
    assert (ch[:GUARD] == P8).all() and (ch[GUARD + wrote:] == P8).all(), "chars poison: a byte outside [0, bytes), or characters written although they do not fit"
    assert np.array_equal(d_tags.cpu().numpy()[1:], root_tags) and np.array_equal(d_values.cpu().numpy().view(np.uint64)[:rows], root_values), "the roots were written"
    if not nothing:
        assert int(oh[GUARD]) == 0 and int(oh[GUARD + rows]) == total, "the offsets end at the total"
    return rc, total, oh[GUARD: GUARD + wrote_offsets].copy(), sh[GUARD: GUARD + wrote_status].copy(), ch[GUARD: GUARD + wrote].tobytes()


def column(p, T, roots, docs=None):
    """the texts at their EXACT capacity: a call with room for nothing and a null chars_dev says what is needed and leaves offsets and status complete; one with one
    byte too few writes nothing either; the third fills -> (offsets, chars, status)"""
    rc, total, offsets0, status0, _ = call(p, T, roots, 0, null_chars=True, docs=docs)
    if total == 0:
        assert rc == 0
        return offsets0, b"", status0
    assert rc == E_OVERFLOW
    rc, again, offsets1, status1, _ = call(p, T, roots, total - 1, docs=docs, expect=E_OVERFLOW)
    assert again == total and np.array_equal(offsets1, offsets0) and np.array_equal(status1, status0)
    rc, again, offsets, status, chars = call(p, T, roots, total, docs=docs, expect=0)
    assert again == total == len(chars) and np.array_equal(offsets, offsets0) and np.array_equal(status, status0)
    return offsets, chars, status


def check(p, T, roots, docs=None):
    """the call over one row of roots against the model -> (offsets, chars, status)"""
    offsets, chars, status = column(p, T, roots, docs)
    want = json_text_model.column(json_text_model.Stream(T.tape, T.sbuf, T.table if docs is None else T.table[: docs + 1]), roots)
    assert np.array_equal(status, want[2]), "status"
    assert np.array_equal(offsets, want[0]), "offsets"
    if chars != want[1]:
        at = next(i for i, (a, b) in enumerate(zip(chars, want[1])) if a != b)
        raise AssertionError(f"chars differ at byte {at}: {chars[max(0, at - 40): at + 40]!r}, the model {want[1][max(0, at - 40): at + 40]!r}")
    return offsets, chars, status


def roots_of(p, T):
    """the root cell of every document: sjgpu_at_pointers_device with the empty pointer"""
    tags, values = query(p, T, [b""])
    return tags[0], values[0]


def parsed_tapes(p, docs, max_depth=1024):
    """the tapes of sjgpu_parse for each document, laid out as a stream"""
    parsed = []
    for d in docs:
        err, tape, sbuf = p.parse(d, max_depth)
        assert err == 0, err
        parsed.append((tape.copy(), sbuf.copy()))
    return Tapes(*json_text_cases.stream_of(parsed))


# ---- 1. the fixture's documents through the device's own tapes ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("document", [0, 1, 2], ids=["twitter", "citm_catalog", "hand_made"])
def test_fixture_cell_by_cell(parser, document):
    docs, cases, _ = json_text_cases.fixture()
    T = Tapes.of_stream(parser, [docs[document]])
    cells = 0
    for c in cases:
        if c["document"] != document:
            continue
        row = roots_of(parser, T) if c["path"] == b"$" else matches(parser, T, c["path"])
        offsets, chars, status = check(parser, T, row)
        assert not status.any(), c["path"]
        json_text_cases.assert_texts_are_the_fixtures(c, json_text_cases.split(offsets, chars))
        cells += len(row[0])
    assert cells > 50


# ---- 2. rows at the wave's and the workgroup's edges, every kind of root -------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", ROW_COUNTS)
def test_rows_at_the_wave_and_workgroup_edges(parser, rows):
    docs, _, _ = json_text_cases.fixture()
    T = Tapes.of_stream(parser, [docs[2], json_text_cases.deep_document(5), b'{"a":[1,2.5,{"b":null}],"c":"d"}'])
    pool = [matches(parser, T, path) for path in (b"$[*]", b"$[*][*]", b"$.*", b"$.*.*")]
    pool_tags, pool_values = np.concatenate([t for t, _ in pool]), np.concatenate([v for _, v in pool])
    assert len(pool_tags) > 60
    rng = np.random.default_rng(300 + rows)
    pick = rng.integers(0, len(pool_tags), rows)
    tags, values = pool_tags[pick].copy(), pool_values[pick].copy()
    root = roots_of(parser, T)
    bad = [(t, v) for t, v, served in json_text_cases.every_kind_of_cell(len(T.sbuf), (int(root[0][0]), int(root[1][0]))) if not served]
    for k, i in enumerate(range(0, rows, 5)):
        tags[i], values[i] = bad[k % len(bad)]
    offsets, chars, status = check(parser, T, (tags, values))
    assert (status[::5] != 0).all() and len(offsets) == rows + 1
    if rows == 0:
        rc, total, offsets, _, _ = call(parser, T, (tags, values), 0, null_chars=True, expect=0)
        assert total == 0 and offsets.tolist() == [0]


def test_every_kind_of_root(parser):
    docs, _, _ = json_text_cases.fixture()
    T = Tapes.of_stream(parser, [docs[2]])
    root = roots_of(parser, T)
    cells = json_text_cases.every_kind_of_cell(len(T.sbuf), (int(root[0][0]), int(root[1][0])))
    row = (np.array([t for t, _, _ in cells], np.uint8), np.array([v for _, v, _ in cells], np.uint64))
    offsets, chars, status = check(parser, T, row)
    assert [(s == 0) for s in status.tolist()] == [served for _, _, served in cells]
    offsets, chars, status = check(parser, T, row, docs=0)  # no document: scalars are served from the cell, no container has a tape to agree with
    assert [(s == 0) for s in status.tolist()] == [served and chr(t) not in "{[" for t, _, served in cells]


def test_refusals(parser):
    docs, _, _ = json_text_cases.fixture()
    T = Tapes.of_stream(parser, [docs[2]])
    row = roots_of(parser, T)
    call(parser, T, row, 16, offsets_skew=2, expect=E_BADARG)
    call(parser, T, row, 16, root_skew=4, expect=E_BADARG)
    call(parser, T, row, 16, null_chars=True, expect=E_BADARG)  # a capacity without characters
    import torch
    out = torch.zeros(64, dtype=torch.int32, device="cuda")
    args = (T.d_tape.data_ptr(), len(T.tape), T.d_sbuf.data_ptr(), len(T.sbuf), T.d_table.data_ptr(), T.docs)
    assert json_text.serialize_cells_device(parser, *args, 0, 0, 1, out.data_ptr(), out.data_ptr() + 64, 0, 0, T.stream)[0] == E_BADARG  # rows without roots
    assert json_text.serialize_cells_device(parser, *args, 0, 0, 0, out.data_ptr(), 0, 0, 0, T.stream) == (0, 0)  # no rows: offsets[0] = 0
    assert int(out[0]) == 0


# ---- 3. strings, nesting, broken tapes ---------------------------------------------------------------------------------------------------------------------------
def test_strings_of_every_length_and_byte(parser):
    T = Tapes.of_stream(parser, [json_text_cases.strings_document()])
    check(parser, T, roots_of(parser, T))
    row = matches(parser, T, b"$[*]")
    offsets, chars, status = check(parser, T, row)  # each string a root of its own: every text's ragged ends meet a neighbour's
    assert not status.any() and len(row[0]) > 70


@pytest.mark.parametrize("depth", DEPTHS)
def test_nesting_on_both_sides_of_the_spill(parser, depth):
    doc = json_text_cases.deep_document(depth)
    T = parsed_tapes(parser, [doc, json_text_cases.deep_document(depth - 1), b"[]"], MAX_DEPTH)
    offsets, chars, status = check(parser, T, roots_of(parser, T))
    assert not status.any() and chars.startswith(doc)


def test_broken_sub_tapes_are_refused_in_the_count(parser):
    docs, _, _ = json_text_cases.fixture()
    T = Tapes.of_stream(parser, [docs[2]])
    root = roots_of(parser, T)
    for what, broken in json_text_cases.broken_tapes(T.tape, T.table):
        B = Tapes(broken, T.sbuf, T.table)
        offsets, chars, status = check(parser, B, root)
        assert status.tolist() == [20] and offsets.tolist() == [0, 0], what


# ---- 4. the round trip, without the reference ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("document", [0, 1, 2], ids=["twitter", "citm_catalog", "hand_made"])
def test_a_text_parsed_again_is_the_tape_it_came_from(parser, document):
    docs, _, _ = json_text_cases.fixture()
    err, tape, sbuf = parser.parse(docs[document])
    assert err == 0
    tape, sbuf = tape.copy(), sbuf.copy()
    T = Tapes(*json_text_cases.stream_of([(tape, sbuf)]))
    _, text, status = column(parser, T, roots_of(parser, T))
    assert not status.any() and len(text) > 0
    err, tape2, sbuf2 = parser.parse(np.frombuffer(text, np.uint8))
    assert err == 0 and np.array_equal(tape2, tape) and np.array_equal(sbuf2, sbuf)
    T2 = Tapes(*json_text_cases.stream_of([(tape2.copy(), sbuf2.copy())]))
    _, again, _ = column(parser, T2, roots_of(parser, T2))
    assert again == text


# ---- 5. the calls above ----------------------------------------------------------------------------------------------------------------------------------------
def test_documents_as_json_many_over_an_ndjson_stream(parser):
    data = np.fromfile(os.path.join(EXAMPLES, "amazon_cellphones.ndjson"), np.uint8)
    lines = [ln for ln in data.tobytes().split(b"\n") if ln.strip()]
    offsets, chars, status = json_text.documents_as_json_many(parser, data)
    T = Tapes.of_stream(parser, lines)
    want = json_text_model.column(json_text_model.Stream(T.tape, T.sbuf, T.table), json_text_cases.root_row(T.tape, T.sbuf, T.table))
    assert len(status) == len(lines) > 100 and not status.any()
    assert np.array_equal(offsets, want[0]) and chars.tobytes() == want[1]


def test_json_column_many_takes_the_overflow_road_too(parser):
    docs, cases, _ = json_text_cases.fixture()
    c = [c for c in cases if (c["document"], c["path"]) == (0, b"$.statuses[*].entities")][0]
    for wide in (False, True):
        offsets, chars, status = json_text.json_column_many(parser, docs[0], c["path"], wide=wide)
        assert not status.any()
        json_text_cases.assert_texts_are_the_fixtures(c, json_text_cases.split(offsets, chars))
    # a document whose text is longer than its source: the first guess is short, the second call fills
    grows = b"[" + b",".join([b"1e2"] * 500) + b"]"
    offsets, chars, status = json_text.json_column_many(parser, grows, b"$[*]")
    assert chars.tobytes() == b"100.0" * 500 and offsets.tolist() == list(range(0, 2501, 5)) and not status.any()
