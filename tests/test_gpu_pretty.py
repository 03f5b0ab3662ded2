"""GPU tier (-m gpu): cells as indented JSON text -- sjgpu_prettify_cells_device and sjgpu_prettify_cells_wide_device (include/sjgpu_pretty.h; the PRETTY instantiations
of the kernels of sjgpu_json.hip and sjgpu_json_wide.hip) and pretty_text.pretty_column_many / documents_as_pretty_many.  Every row goes through BOTH calls: the outputs
of the wide one must be the narrow one's byte for byte -- offsets, status, characters, the total and the return code at capacity 0 with a null chars_dev, one byte
short and exact -- and both must be the model's (tests/pretty_model.py, pinned against tests/golden/pretty.json -- the real reference's simdjson::prettify -- on the CPU
tier).  Every output lies at exactly its contracted size between poisoned guards of 4 KiB and a byte (odd: the status row and the characters begin at odd addresses);
the harness is the one of tests/test_gpu_json_wide.py.  The minify calls are asked once more on the same rows: they still give tests/json_text_model.py's bytes."""
import json
import os

import numpy as np
import pytest

import json_text_cases
import json_text_model
import json_wide_cases
import pretty_cases
import pretty_model
from json_text_cases import DEPTHS, MAX_DEPTH, ROW_COUNTS
from simdjson_amd import _paths, build, capi, corpus, json_text, json_text_wide, pretty_text
from test_gpu_fields import device_roots, matches
from test_gpu_json import parsed_tapes, roots_of
from test_gpu_query import Tapes

pytestmark = pytest.mark.gpu

CAP = 128 << 20
E_BADARG, E_OVERFLOW, E_RANGE = -4, -5, -8
GUARD = 4097
P32, P8 = 0x5A5A5A5A, 0x5A
EXAMPLES = os.path.join(_paths.REPO_ROOT, "tests", "golden", "jsonexamples")
NARROW, WIDE = pretty_text.prettify_cells_device, pretty_text.prettify_cells_wide_device
MINIFY_NARROW, MINIFY_WIDE = json_text.serialize_cells_device, json_text_wide.serialize_cells_wide_device


@pytest.fixture(scope="module")
def parser():
    build.build_sjgpu()
    p = capi.DomParserImplementation(CAP)
    yield p
    p.close()


@pytest.fixture(params=["the NULL stream", "a stream of the caller's"])
def stream(request):
    """the test's body -- the uploads, the poison, the calls -- on the NULL stream, and once more on a stream of the caller's (Tapes takes the current one)"""
    import torch
    if request.param == "the NULL stream":
        yield 0
    else:
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            yield s.cuda_stream
        s.synchronize()


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


def both(p, T, roots, docs=None, entries=(WIDE, NARROW)):
    """the row through both calls at three capacities -- none with a null chars_dev, one byte short, exact --, each output of the wide call the narrow call's
    -> (offsets, chars, status) at the exact capacity"""
    w0, n0 = (call(p, T, roots, 0, e, null_chars=True, docs=docs) for e in entries)
    same(w0, n0, "capacity 0")
    total = n0[1]
    if total == 0:
        assert n0[0] == 0
        return n0[2], b"", n0[3]
    assert n0[0] == E_OVERFLOW
    w1, n1 = (call(p, T, roots, total - 1, e, docs=docs, expect=E_OVERFLOW) for e in entries)
    same(w1, n1, "one byte short")
    w2, n2 = (call(p, T, roots, total, e, docs=docs, expect=0) for e in entries)
    same(w2, n2, "exact capacity")
    assert np.array_equal(w2[2], w0[2]) and np.array_equal(w2[3], w0[3]) and w2[1] == total == len(w2[4])
    return w2[2], w2[4], w2[3]


def check(p, T, roots, docs=None):
    """both calls, and the model -> (offsets, chars, status)"""
    offsets, chars, status = both(p, T, roots, docs)
    want = pretty_model.column(pretty_model.Stream(T.tape, T.sbuf, T.table if docs is None else T.table[: docs + 1]), roots)
    assert np.array_equal(status, want[2]) and np.array_equal(offsets, want[0]) and chars == want[1], "the model"
    return offsets, chars, status


def minify_is_what_it_was(p, T, roots):
    """one call of each minify entry at the exact capacity: tests/json_text_model.py's bytes, as before this module's calls existed"""
    want = json_text_model.column(json_text_model.Stream(T.tape, T.sbuf, T.table), roots)
    for entry in (MINIFY_NARROW, MINIFY_WIDE):
        rc, total, offsets, status, chars = call(p, T, roots, len(want[1]), entry, expect=0)
        assert np.array_equal(offsets, want[0]) and np.array_equal(status, want[2]) and chars == want[1], entry.__name__


# ---- 1. the fixture ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("document", [0, 1, 2], ids=["twitter", "citm_catalog", "hand_made"])
def test_fixture_cell_by_cell(parser, document):
    docs, cases = pretty_cases.fixture()
    T = Tapes.of_stream(parser, [docs[document]])
    cells = 0
    for c in cases:
        if c["document"] != document:
            continue
        row = roots_of(parser, T) if c["path"] == b"$" else matches(parser, T, c["path"])
        offsets, chars, status = check(parser, T, row)
        assert not status.any(), c["path"]
        pretty_cases.assert_texts_are_the_fixtures(c, json_text_cases.split(offsets, chars))
        cells += len(row[0])
    assert cells > 50


def test_the_chains_on_both_streams(parser, stream):
    """the 96 chains whose leaf lies 14 .. 65 containers deep, a document per level and a cell per chain, in one row: the reference's texts"""
    docs, cases = pretty_cases.fixture()
    T = parsed_tapes(parser, docs[3:])
    assert T.stream == stream
    row = matches(parser, T, b"$[*]")
    offsets, chars, status = check(parser, T, row)
    texts = json_text_cases.split(offsets, chars)
    assert not status.any() and len(texts) == len(pretty_cases.chains()) == 12 * (len(cases) - 14)
    for k, c in enumerate(cases[14:]):
        pretty_cases.assert_texts_are_the_fixtures(c, texts[12 * k: 12 * k + 12])
    minify_is_what_it_was(parser, T, row)


def test_the_hand_made_document_on_both_streams(parser, stream):
    docs, cases = pretty_cases.fixture()
    T = Tapes.of_stream(parser, [docs[2]])
    assert T.stream == stream
    for c in cases:
        if c["document"] == 2:
            row = roots_of(parser, T) if c["path"] == b"$" else matches(parser, T, c["path"])
            offsets, chars, status = check(parser, T, row)
            pretty_cases.assert_texts_are_the_fixtures(c, json_text_cases.split(offsets, chars))
            minify_is_what_it_was(parser, T, row)


# ---- 2. rows, roots, strings, depths, broken tapes -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", ROW_COUNTS)
def test_rows_at_the_wave_and_workgroup_edges(parser, rows):
    docs, _ = pretty_cases.fixture()
    T = Tapes.of_stream(parser, [docs[2], pretty_cases.chain(17, b'{"a":[1,{}]}', 1), b'{"a":[1,2.5,{"b":null}],"c":"d"}'])
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
        for entry in (WIDE, NARROW):
            rc, total, offsets, _, _ = call(parser, T, (tags, values), 0, entry, null_chars=True, expect=0)
            assert total == 0 and offsets.tolist() == [0]


def test_every_kind_of_root(parser):
    docs, _ = pretty_cases.fixture()
    T = Tapes.of_stream(parser, [docs[2]])
    root = roots_of(parser, T)
    cells = json_text_cases.every_kind_of_cell(len(T.sbuf), (int(root[0][0]), int(root[1][0])))
    row = (np.array([t for t, _, _ in cells], np.uint8), np.array([v for _, v, _ in cells], np.uint64))
    offsets, chars, status = check(parser, T, row)
    assert [(s == 0) for s in status.tolist()] == [served for _, _, served in cells]
    minify_is_what_it_was(parser, T, row)
    offsets, chars, status = check(parser, T, row, docs=0)  # no document: scalars are served from the cell, no container has a tape to agree with
    assert [(s == 0) for s in status.tolist()] == [served and chr(t) not in "{[" for t, _, served in cells]


def test_refusals(parser):
    docs, _ = pretty_cases.fixture()
    T = Tapes.of_stream(parser, [docs[2]])
    row = roots_of(parser, T)
    import torch
    out = torch.zeros(64, dtype=torch.int32, device="cuda")
    args = (T.d_tape.data_ptr(), len(T.tape), T.d_sbuf.data_ptr(), len(T.sbuf), T.d_table.data_ptr(), T.docs)
    for entry in (WIDE, NARROW):
        call(parser, T, row, 16, entry, offsets_skew=2, expect=E_BADARG)
        call(parser, T, row, 16, entry, root_skew=4, expect=E_BADARG)
        call(parser, T, row, 16, entry, null_chars=True, expect=E_BADARG)  # a capacity without characters
        assert entry(parser, *args, 0, 0, 1, out.data_ptr(), out.data_ptr() + 64, 0, 0, T.stream)[0] == E_BADARG  # rows without roots
        out[0] = 7
        assert entry(parser, *args, 0, 0, 0, out.data_ptr(), 0, 0, 0, T.stream) == (0, 0)  # no rows: offsets[0] = 0
        assert int(out[0]) == 0


def test_strings_of_every_length_and_byte(parser):
    T = Tapes.of_stream(parser, [json_text_cases.strings_document()])
    check(parser, T, roots_of(parser, T))
    row = matches(parser, T, b"$[*]")
    offsets, chars, status = check(parser, T, row)
    assert not status.any() and len(row[0]) > 70


@pytest.mark.parametrize("depth", DEPTHS)
def test_nesting_on_both_sides_of_the_hand_off(parser, depth):
    T = parsed_tapes(parser, [json_text_cases.deep_document(depth), json_text_cases.deep_document(depth - 1), b"[]"], MAX_DEPTH)
    offsets, chars, status = check(parser, T, roots_of(parser, T))
    assert not status.any() and chars.endswith(b"[]\n") and b" " * 61 not in chars


def test_broken_sub_tapes_are_refused_in_the_count(parser):
    docs, _ = pretty_cases.fixture()
    T = Tapes.of_stream(parser, [docs[2]])
    root = roots_of(parser, T)
    for what, broken in json_text_cases.broken_tapes(T.tape, T.table):
        B = Tapes(broken, T.sbuf, T.table)
        offsets, chars, status = check(parser, B, root)
        assert status.tolist() == [20] and offsets.tolist() == [0, 0], what


# ---- 3. the share edges ------------------------------------------------------------------------------------------------------------------------------------------
def test_the_same_container_twice_and_a_container_beside_its_own_child(parser):
    T = parsed_tapes(parser, [json_wide_cases.NESTED_DOCUMENT])
    row = json_wide_cases.overlapping_row((T.tape, T.sbuf, T.table))
    offsets, chars, status = check(parser, T, row)
    texts = json_text_cases.split(offsets, chars)
    assert not status.any() and texts[0] == texts[1] == texts[3] and texts[2].startswith(b"[\n    1,\n    {\n")


@pytest.mark.parametrize("words", json_wide_cases.SHARE_EDGE_WORDS)
def test_documents_at_the_edges_of_the_shares(parser, words):
    """roots of 63 / 64 / 65, 255 / 256 / 257 and 511 / 512 / 513 words at slot 0 and behind a scalar's slot; the same words as a flat container, below 15 arrays"""
    inner = json_wide_cases.document_of_words(words)
    T = parsed_tapes(parser, [inner, b"[" * 15 + inner + b"]" * 15, b"[]"])
    root = roots_of(parser, T)
    assert int(root[1][0] >> np.uint64(32)) - int(root[1][0] & np.uint64(0xFFFFFFFF)) == words
    shifted = (np.concatenate([np.array([ord("t")], np.uint8), root[0], root[0]]), np.concatenate([np.array([1], np.uint64), root[1], root[1]]))
    offsets, chars, status = check(parser, T, shifted)
    assert not status.any()


@pytest.mark.parametrize("as_object", [False, True])
def test_a_flat_container_of_more_children_than_a_workgroup(parser, as_object):
    T = parsed_tapes(parser, [pretty_cases.flat_container_of(307, as_object), json_wide_cases.wide_object(300)])
    offsets, chars, status = check(parser, T, roots_of(parser, T))
    assert not status.any() and (b',"k306":306\n}' if as_object else b',"v301"\n,[]\n,') in chars


def test_empty_containers_and_tag_like_second_words(parser):
    docs = json_wide_cases.EMPTY_CONTAINER_DOCUMENTS + [b"[" * 15 + d + b"]" * 15 for d in json_wide_cases.EMPTY_CONTAINER_DOCUMENTS]
    docs += [json_wide_cases.number_at_slot(slot, value) for slot in json_wide_cases.BORDER_SLOTS for value in json_wide_cases.TAG_LIKE_INTEGERS]
    T = parsed_tapes(parser, docs)
    offsets, chars, status = check(parser, T, roots_of(parser, T))
    texts = json_text_cases.split(offsets, chars)
    assert not status.any() and texts[6] == b"{}\n" and texts[7] == b"[]\n" and texts[3] == b"[\n    {}\n]\n"


# ---- 4. one large document, and the *_many calls ---------------------------------------------------------------------------------------------------------------
def test_twitter_as_one_cell_and_as_its_statuses(parser):
    """twitter.json as ONE root cell and as `$.statuses[*]`: wide and narrow agree byte for byte, and every text parsed again is the value of its minified text"""
    data = open(os.path.join(EXAMPLES, "twitter.json"), "rb").read()
    T = Tapes.of_stream(parser, [data])
    root = roots_of(parser, T)
    offsets, text, status = both(parser, T, root)
    assert status.tolist() == [0] and offsets.tolist() == [0, len(text)] and len(text) > len(data) and text.endswith(b"\n}\n")
    mini = both(parser, T, root, entries=(MINIFY_WIDE, MINIFY_NARROW))[1]
    assert json.loads(text) == json.loads(mini) == json.loads(data)
    row = matches(parser, T, b"$.statuses[*]")
    offsets, chars, status = both(parser, T, row)
    mini = both(parser, T, row, entries=(MINIFY_WIDE, MINIFY_NARROW))
    assert len(row[0]) == 100 and not status.any()
    for pretty, plain in zip(json_text_cases.split(offsets, chars), json_text_cases.split(mini[0], mini[1])):
        assert json.loads(pretty) == json.loads(plain) and pretty.startswith(b"{\n    \"") and pretty.endswith(b"\n}\n")


def test_the_many_calls_on_an_ndjson_stream(parser):
    data = np.fromfile(os.path.join(EXAMPLES, "amazon_cellphones.ndjson"), np.uint8)
    plain = json_text.documents_as_json_many(parser, data)
    narrow, wide = (pretty_text.documents_as_pretty_many(parser, data, one_lane_per_word=w) for w in (False, True))
    assert len(narrow[2]) > 100 and not narrow[2].any() and all(np.array_equal(n, w) for n, w in zip(narrow, wide))
    texts, plains = json_text_cases.split(narrow[0], narrow[1].tobytes()), json_text_cases.split(plain[0], plain[1].tobytes())
    assert all(json.loads(t) == json.loads(m) and t.endswith(b"\n") for t, m in zip(texts, plains))
    lines = data.tobytes().splitlines()
    err, tape, sbuf = parser.parse(np.frombuffer(lines[5], np.uint8))
    one = json_text_cases.stream_of([(tape.copy(), sbuf.copy())])
    assert err == 0 and texts[5] == pretty_model.column(pretty_model.Stream(*one), json_text_cases.root_row(*one))[1]
    columns = [pretty_text.pretty_column_many(parser, data, b"$[*]", wide=pw, one_lane_per_word=w) for pw in (False, True) for w in (False, True)]
    assert len(columns[0][2]) > 1000 and not columns[0][2].any() and all(np.array_equal(a, b) for c in columns[1:] for a, b in zip(columns[0], c))
    column_plain = json_text.json_column_many(parser, data, b"$[*]")
    assert np.array_equal(np.diff(columns[0][0].astype(np.int64)), np.diff(column_plain[0].astype(np.int64)) + 1)  # scalars: the minified text and a newline
