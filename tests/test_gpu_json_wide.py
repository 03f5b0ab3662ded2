"""GPU tier (-m gpu): cells as JSON text, breadth first -- sjgpu_serialize_cells_wide_device (sjgpu_json_wide.hip, include/sjgpu_json_wide.h) and
json_text_wide.json_column_wide_many / documents_as_json_wide_many.  Every row goes through BOTH calls: the outputs of the wide one must be the narrow one's byte for
byte -- offsets, status, characters, the total and the return code at capacity 0 with a null chars_dev, one byte short and exact -- and both must be the model's
(tests/json_text_model.py, pinned against tests/golden/json_text.json on the CPU tier).  The cases of tests/test_gpu_json.py (tests/json_text_cases.py, imported), the
ones of tests/json_wide_cases.py, the SJGPU_E_RANGE refusal, one document of about 1 MiB as ONE root cell and as `$.statuses[*]` with its text parsed again, and the
serialize cases of tests/offset_limit_cases.py.  Every output lies at exactly its contracted size between poisoned guards of 4 KiB and a byte (odd: the status row and
the characters begin at odd addresses)."""
import os

import numpy as np
import pytest

import json_text_cases
import json_text_model
import json_wide_cases
import offset_limit_cases as C
from json_text_cases import DEPTHS, MAX_DEPTH, ROW_COUNTS
from simdjson_amd import _paths, build, capi, corpus, json_text, json_text_wide
from test_gpu_fields import device_roots, matches
from test_gpu_json import parsed_tapes, roots_of
from test_gpu_query import Tapes

pytestmark = pytest.mark.gpu

CAP = 128 << 20
E_BADARG, E_OVERFLOW, E_RANGE = -4, -5, -8
GUARD = 4097
P32, P8 = 0x5A5A5A5A, 0x5A
EXAMPLES = os.path.join(_paths.REPO_ROOT, "tests", "golden", "jsonexamples")
NARROW, WIDE = json_text.serialize_cells_device, json_text_wide.serialize_cells_wide_device


@pytest.fixture(scope="module")
def parser():
    build.build_sjgpu()
    p = capi.DomParserImplementation(CAP)
    yield p
    p.close()


def call(p, T, roots, cap, entry, null_chars=False, docs=None, offsets_skew=0, root_skew=0, expect=None):
    """one call of `entry` over the roots (tags[rows], values[rows]) with outputs of exactly rows + 1 words, rows bytes and `cap` characters between poisoned guards
    -> (rc, bytes, offsets, status, chars: bytes); SJGPU_E_RANGE leaves the statuses and nothing else"""
    torch = T.torch
    root_tags, root_values, d_tags, d_values = device_roots(T, roots)
    rows = len(root_tags)
    offsets = torch.full((rows + 1 + 2 * GUARD,), P32, dtype=torch.int32, device="cuda")
    status = torch.full((rows + 2 * GUARD,), P8, dtype=torch.uint8, device="cuda")
    chars = torch.full((cap + 2 * GUARD,), P8, dtype=torch.uint8, device="cuda")
    rc, total = entry(p, T.d_tape.data_ptr(), len(T.tape), T.d_sbuf.data_ptr(), len(T.sbuf), T.d_table.data_ptr(), T.docs if docs is None else docs,
                      d_values.data_ptr() + root_skew, d_tags.data_ptr() + 1, rows, offsets.data_ptr() + 4 * GUARD + offsets_skew, status.data_ptr() + GUARD,
                      0 if null_chars else chars.data_ptr() + GUARD, cap, T.stream)
    torch.cuda.synchronize()
    if expect is not None:
        assert rc == expect, (rc, expect, p.last_error())
    wrote_offsets = 0 if rc in (E_BADARG, E_RANGE) else rows + 1
    wrote_status = 0 if rc == E_BADARG else rows
    wrote = total if rc == 0 else 0
    oh, sh, ch = offsets.cpu().numpy().view(np.uint32), status.cpu().numpy(), chars.cpu().numpy()
    assert (oh[:GUARD] == P32).all() and (oh[GUARD + wrote_offsets:] == P32).all(), "offsets poison"
    assert (sh[:GUARD] == P8).all() and (sh[GUARD + wrote_status:] == P8).all(), "status poison"
    assert not (sh[GUARD: GUARD + wrote_status] == P8).any(), "a status was not written"
    assert (ch[:GUARD] == P8).all() and (ch[GUARD + wrote:] == P8).all(), "chars poison: a byte outside [0, bytes), or characters written although they do not fit"
    assert np.array_equal(d_tags.cpu().numpy()[1:], root_tags) and np.array_equal(d_values.cpu().numpy().view(np.uint64)[:rows], root_values), "the roots were written"
    if wrote_offsets:
        assert int(oh[GUARD]) == 0 and int(oh[GUARD + rows]) == total, "the offsets end at the total"
    return rc, total, oh[GUARD: GUARD + wrote_offsets].copy(), sh[GUARD: GUARD + wrote_status].copy(), ch[GUARD: GUARD + wrote].tobytes()


def same(a, b, what):
    assert a[0] == b[0] and a[1] == b[1], (what, "rc and bytes", a[:2], b[:2])
    assert np.array_equal(a[2], b[2]), (what, "offsets")
    assert np.array_equal(a[3], b[3]), (what, "status")
    if a[4] != b[4]:
        at = next((i for i, (x, y) in enumerate(zip(a[4], b[4])) if x != y), min(len(a[4]), len(b[4])))
        raise AssertionError(f"{what}: chars differ at byte {at}: wide {a[4][max(0, at - 40): at + 40]!r}, narrow {b[4][max(0, at - 40): at + 40]!r}")


def both(p, T, roots, docs=None):
    """the row through both calls at three capacities -- none with a null chars_dev, one byte short, exact --, each output of the wide call the narrow call's
    -> (offsets, chars, status) at the exact capacity"""
    w0, n0 = (call(p, T, roots, 0, e, null_chars=True, docs=docs) for e in (WIDE, NARROW))
    same(w0, n0, "capacity 0")
    total = n0[1]
    if total == 0:
        assert n0[0] == 0
        return n0[2], b"", n0[3]
    assert n0[0] == E_OVERFLOW
    w1, n1 = (call(p, T, roots, total - 1, e, docs=docs, expect=E_OVERFLOW) for e in (WIDE, NARROW))
    same(w1, n1, "one byte short")
    w2, n2 = (call(p, T, roots, total, e, docs=docs, expect=0) for e in (WIDE, NARROW))
    same(w2, n2, "exact capacity")
    assert np.array_equal(w2[2], w0[2]) and np.array_equal(w2[3], w0[3]) and w2[1] == total == len(w2[4])
    return w2[2], w2[4], w2[3]


def check(p, T, roots, docs=None):
    """both calls, and the model -> (offsets, chars, status)"""
    offsets, chars, status = both(p, T, roots, docs)
    want = json_text_model.column(json_text_model.Stream(T.tape, T.sbuf, T.table if docs is None else T.table[: docs + 1]), roots)
    assert np.array_equal(status, want[2]) and np.array_equal(offsets, want[0]) and chars == want[1], "the model"
    return offsets, chars, status


# ---- 1. the narrow module's cases through both calls ---------------------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("rows", ROW_COUNTS)
def test_rows_at_the_wave_and_workgroup_edges(parser, rows):
    docs, _, _ = json_text_cases.fixture()
    T = Tapes.of_stream(parser, [docs[2], json_text_cases.deep_document(5), b'{"a":[1,2.5,{"b":null}],"c":"d"}'])
    pool = [matches(parser, T, path) for path in (b"$[*]", b"$[*][*]", b"$.*", b"$.*.*")]
    pool_tags, pool_values = np.concatenate([t for t, _ in pool]), np.concatenate([v for _, v in pool])
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
        rc, total, offsets, _, _ = call(parser, T, (tags, values), 0, WIDE, null_chars=True, expect=0)
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
    call(parser, T, row, 16, WIDE, offsets_skew=2, expect=E_BADARG)
    call(parser, T, row, 16, WIDE, root_skew=4, expect=E_BADARG)
    call(parser, T, row, 16, WIDE, null_chars=True, expect=E_BADARG)  # a capacity without characters
    import torch
    out = torch.zeros(64, dtype=torch.int32, device="cuda")
    args = (T.d_tape.data_ptr(), len(T.tape), T.d_sbuf.data_ptr(), len(T.sbuf), T.d_table.data_ptr(), T.docs)
    assert WIDE(parser, *args, 0, 0, 1, out.data_ptr(), out.data_ptr() + 64, 0, 0, T.stream)[0] == E_BADARG  # rows without roots
    out[0] = 7
    assert WIDE(parser, *args, 0, 0, 0, out.data_ptr(), 0, 0, 0, T.stream) == (0, 0)  # no rows: offsets[0] = 0
    assert int(out[0]) == 0


def test_strings_of_every_length_and_byte(parser):
    T = Tapes.of_stream(parser, [json_text_cases.strings_document()])
    check(parser, T, roots_of(parser, T))
    row = matches(parser, T, b"$[*]")
    offsets, chars, status = check(parser, T, row)
    assert not status.any() and len(row[0]) > 70


@pytest.mark.parametrize("depth", DEPTHS)
def test_nesting_on_both_sides_of_the_hand_off(parser, depth):
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


def test_the_wide_many_calls_take_the_overflow_road_too(parser):
    docs, cases, _ = json_text_cases.fixture()
    c = [c for c in cases if (c["document"], c["path"]) == (0, b"$.statuses[*].entities")][0]
    for wide in (False, True):
        offsets, chars, status = json_text_wide.json_column_wide_many(parser, docs[0], c["path"], wide=wide)
        assert not status.any()
        json_text_cases.assert_texts_are_the_fixtures(c, json_text_cases.split(offsets, chars))
    grows = b"[" + b",".join([b"1e2"] * 500) + b"]"  # a text longer than its source: the first guess is short, the second call fills
    offsets, chars, status = json_text_wide.json_column_wide_many(parser, grows, b"$[*]")
    assert chars.tobytes() == b"100.0" * 500 and offsets.tolist() == list(range(0, 2501, 5)) and not status.any()
    offsets, chars, status = json_text_wide.documents_as_json_wide_many(parser, grows)
    assert chars.tobytes() == b"[" + b",".join([b"100.0"] * 500) + b"]" and offsets.tolist() == [0, len(chars)] and status.tolist() == [0]
    data = np.fromfile(os.path.join(EXAMPLES, "amazon_cellphones.ndjson"), np.uint8)
    got, want = json_text_wide.documents_as_json_wide_many(parser, data), json_text.documents_as_json_many(parser, data)
    assert len(got[2]) > 100 and all(np.array_equal(g, w) for g, w in zip(got, want))


# ---- 2. what one lane per tape word can get wrong -------------------------------------------------------------------------------------------------------------
def test_the_same_container_twice_and_a_container_beside_its_own_child(parser):
    T = parsed_tapes(parser, [json_wide_cases.NESTED_DOCUMENT])
    row = json_wide_cases.overlapping_row((T.tape, T.sbuf, T.table))
    offsets, chars, status = check(parser, T, row)
    texts = json_text_cases.split(offsets, chars)
    assert not status.any() and texts[0] == texts[1] == texts[3] == json_wide_cases.NESTED_DOCUMENT and texts[2] in texts[0]


@pytest.mark.parametrize("words", json_wide_cases.SHARE_EDGE_WORDS)
def test_documents_at_the_edges_of_the_shares(parser, words):
    """a lane's share is one slot (a container has two words at the least: [] rides along), a wave's 64, a workgroup's 256: roots of 63 / 64 / 65, 255 / 256 / 257 and
    511 / 512 / 513 words at slot 0, and behind a scalar's slot, which moves every edge by one"""
    T = parsed_tapes(parser, [json_wide_cases.document_of_words(words), b"[]"])
    root = roots_of(parser, T)
    assert int(root[1][0] >> np.uint64(32)) - int(root[1][0] & np.uint64(0xFFFFFFFF)) == words
    check(parser, T, root)
    shifted = (np.concatenate([np.array([ord("t")], np.uint8), root[0], root[0]]), np.concatenate([np.array([1], np.uint64), root[1], root[1]]))
    offsets, chars, status = check(parser, T, shifted)
    assert not status.any()


def test_an_object_whose_fields_cross_two_workgroups(parser):
    doc = json_wide_cases.wide_object(300)
    T = parsed_tapes(parser, [doc])
    offsets, chars, status = check(parser, T, roots_of(parser, T))
    assert not status.any() and chars == doc


@pytest.mark.parametrize("slot", json_wide_cases.BORDER_SLOTS)
def test_a_number_whose_second_word_looks_like_a_tag_at_a_share_border(parser, slot):
    for value in json_wide_cases.TAG_LIKE_INTEGERS:
        doc = json_wide_cases.number_at_slot(slot, value)
        T = parsed_tapes(parser, [doc])
        root = roots_of(parser, T)
        low = int(root[1][0] & np.uint64(0xFFFFFFFF))
        assert int(T.tape[low + slot]) == value and chr(int(T.tape[low + slot - 1]) >> 56) == "l"
        offsets, chars, status = check(parser, T, root)
        assert not status.any() and chars == doc


def test_empty_containers_as_first_middle_and_last_children(parser):
    T = parsed_tapes(parser, json_wide_cases.EMPTY_CONTAINER_DOCUMENTS)
    offsets, chars, status = check(parser, T, roots_of(parser, T))
    assert not status.any() and json_text_cases.split(offsets, chars) == json_wide_cases.EMPTY_CONTAINER_DOCUMENTS


def test_the_range_refusal(parser):
    """65 537 roots over one array of 32 767 ones: SJGPU_E_RANGE, every status written (0: the narrow count serves them), offsets and characters poisoned as they
    were (call() checks both), nothing reported; three of the roots are counted"""
    T = parsed_tapes(parser, [json_wide_cases.RANGE_DOCUMENT])
    root = roots_of(parser, T)
    row = json_wide_cases.range_row(root[0][0], root[1][0])
    rc, total, offsets, status, chars = call(parser, T, row, 4096, WIDE, expect=E_RANGE)
    assert total == 0 and len(offsets) == 0 and len(status) == json_wide_cases.RANGE_ROOTS and not status.any() and chars == b""
    few = (row[0][:3], row[1][:3])
    rc, total, offsets, status, chars = call(parser, T, few, 0, WIDE, null_chars=True, expect=E_OVERFLOW)
    assert total == 3 * len(json_wide_cases.RANGE_DOCUMENT) and not status.any()


# ---- 3. one large document ---------------------------------------------------------------------------------------------------------------------------------
def test_one_document_of_a_mebibyte_as_one_cell_and_as_its_statuses(parser):
    """the wide call's own ground: ONE root cell over the whole tape, then `$.statuses[*]`.  Wide and narrow agree byte for byte, and the text of the root parsed
    again is the tape it came from"""
    a, n_statuses = corpus.twitter_like(1 << 20, 47)
    err, tape, sbuf = parser.parse(a)
    assert err == 0
    tape, sbuf = tape.copy(), sbuf.copy()
    T = Tapes(*json_text_cases.stream_of([(tape, sbuf)]))
    root = roots_of(parser, T)
    offsets, text, status = both(parser, T, root)
    assert status.tolist() == [0] and offsets.tolist() == [0, len(text)] and len(text) > 500000
    err, tape2, sbuf2 = parser.parse(np.frombuffer(text, np.uint8))
    assert err == 0 and np.array_equal(tape2, tape) and np.array_equal(sbuf2, sbuf)
    row = matches(parser, T, b"$.statuses[*]")
    offsets, chars, status = both(parser, T, row)
    assert len(row[0]) == n_statuses and not status.any() and text.startswith(b'{"statuses":[' + b",".join(json_text_cases.split(offsets, chars)) + b"]")


# ---- 4. the 32-bit offsets at their limit: the serialize cases of tests/offset_limit_cases.py, aliased string cells (a range space of 65 536 slots at the most) ----
import test_gpu_offset_limits as L  # noqa: E402
from test_gpu_offset_limits import env  # noqa: E402,F401  (fixture; it stands on this module's parser)

LIMIT_CASES = [c for c in C.SERIALIZE if all(name in ("s", "t", "one") for name, _ in c.runs)]


def run_serialize_wide(e, case, cap, data):
    tags, values = L.cells_of(e, case, e.cells)
    rows = C.rows_of(case)
    c = L.Call(e, rows, rows + 1, rows)
    rc, total = WIDE(e.p, *e.tape_args, values.data_ptr(), tags.data_ptr(), rows, c.offsets.ptr, c.status.ptr, L.ptr(data, 0), cap, e.stream)
    e.torch.cuda.synchronize()
    return c, rc, total, C.lengths_of(case, C.TEXT_LENGTHS), None


def test_the_limit_cases_are_the_string_cells():
    assert [c.level for c in LIMIT_CASES] == ["T1", "T2", "T3"]


def test_a_total_beyond_2_31_is_counted_and_served(env):  # noqa: F811
    case, = [c for c in LIMIT_CASES if c.level == "T1"]
    c, rc, total, lengths, _ = run_serialize_wide(env, case, 0, None)
    c.check(("serialize wide", case.name), rc, total, E_OVERFLOW, case.total, lengths, None)
    torch = env.torch
    rows, row = C.rows_of(case), L.model_row(env, case)
    assert len(row) * rows == case.total and C.HALF < case.total < C.LIMIT
    data = L.data_arrays(env, (1,), case.total)
    c, rc, total, lengths, _ = run_serialize_wide(env, case, case.total, data)
    c.check(("serialize wide", case.name), rc, total, 0, case.total, lengths, data, written_bytes=[case.total])
    want = torch.from_numpy(np.frombuffer(row, np.uint8).copy()).cuda()
    rows_same = (data[0].view(torch.uint8).view(rows, len(row)) == want).all(dim=1)
    first_beyond = C.HALF // len(row)
    low, high = bool(rows_same[:first_beyond].all().item()), bool(rows_same[first_beyond:].all().item())
    del rows_same, want, data, c
    torch.cuda.empty_cache()
    assert low, "a row in front of 2^31 is not the model's"
    assert high, "a row that ends beyond 2^31 is not the model's"


def test_a_total_of_2_32_minus_1_is_counted_exactly(env):  # noqa: F811
    case, = [c for c in LIMIT_CASES if c.level == "T2"]
    data = L.data_arrays(env, (1,), L.MIB)
    c, rc, total, lengths, _ = run_serialize_wide(env, case, 0, data)
    c.check(("serialize wide", case.name), rc, total, E_OVERFLOW, 0xFFFFFFFF, lengths, data)


@pytest.mark.parametrize("cap", [0, 1 << 20], ids=["capacity 0", "capacity 1 MiB"])
def test_a_total_beyond_32_bits_is_refused(env, cap):  # noqa: F811
    case, = [c for c in LIMIT_CASES if c.level == "T3"]
    data = L.data_arrays(env, (1,), L.MIB)
    c, rc, total, lengths, _ = run_serialize_wide(env, case, cap, data)
    c.check(("serialize wide", case.name, cap), rc, total, capi.CAPACITY, case.total, lengths, data)
