"""GPU tier (-m gpu): record tables over device tapes -- sjgpu_at_pointers_from_cells_device (k_rows_locate and k_at_pointers_rooted in sjgpu_query.hip,
include/sjgpu_rows.h) and capi.table_many -- against tests/rows_model.py (pinned against tests/golden/pointers.json on the CPU tier) and against Python's json.
The tapes are the device's own (sjgpu_stage2_many_device), the roots what sjgpu_at_pointers_device, sjgpu_at_paths_device and the call itself delivered.
Every output has exactly the contracted size inside a poisoned tensor whose poison is checked after every call, and its tag rows begin at any byte."""
import ctypes
import json
import os
import struct

import numpy as np
import pytest

import query_cases
import rows_model
import stream_cases
from simdjson_amd import _paths, build, capi
from test_gpu_paths import column
from test_gpu_query import Tapes, gather, query

pytestmark = pytest.mark.gpu

CAP = 128 << 20
E_BADARG = -4
GUARD = 65  # odd: with it the tag rows begin at odd addresses
P64 = 0x5A5A5A5A5A5A5A5A
TWITTER = os.path.join(_paths.REPO_ROOT, "tests", "golden", "jsonexamples", "twitter.json")
TWITTER_POINTERS = [b"/user/id", b"/text", b"/retweeted_status/user/screen_name", b"/entities/urls/0/url", b""]


@pytest.fixture(scope="module")
def parser():
    build.build_sjgpu()
    p = capi.DomParserImplementation(CAP)
    yield p
    p.close()


def rooted(p, T, roots, pointers, raw=False, docs=None, table_ptr=None, tape_ptr=None, value_skew=0, root_skew=0):
    """one sjgpu_at_pointers_from_cells_device over the roots (tags[rows], values[rows]) -> (tags[K, rows], values[K, rows]) from columns of exactly K * rows
    cells between poisoned guards; the root tags begin at an odd address.  raw: -> rc, nothing but the poison checked"""
    torch = T.torch
    root_tags, root_values = np.ascontiguousarray(roots[0], np.uint8), np.ascontiguousarray(roots[1], np.uint64)
    rows, K = len(root_tags), len(pointers)
    cells = K * rows
    d_tags = torch.from_numpy(np.concatenate([np.zeros(1, np.uint8), root_tags])).cuda()
    d_values = torch.from_numpy(np.concatenate([root_values, np.zeros(1, np.uint64)]).view(np.int64)).cuda()  # (never empty: an address to pass)
    values = torch.full((cells + 2 * GUARD,), P64, dtype=torch.int64, device="cuda")
    tags = torch.full((cells + 2 * GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
    rc = p.at_pointers_from_cells_device(tape_ptr or T.d_tape.data_ptr(), len(T.tape), T.d_sbuf.data_ptr(), len(T.sbuf), table_ptr or T.d_table.data_ptr(),
                                         T.docs if docs is None else docs, d_values.data_ptr() + root_skew, d_tags.data_ptr() + 1, rows, pointers,
                                         values.data_ptr() + 8 * GUARD + value_skew, tags.data_ptr() + GUARD, T.stream)
    torch.cuda.synchronize()
    vh, th = values.cpu().numpy().view(np.uint64), tags.cpu().numpy()
    written = cells if rc == 0 else 0
    assert (vh[:GUARD] == P64).all() and (vh[GUARD + written:] == P64).all(), "value poison"
    assert (th[:GUARD] == 0x5A).all() and (th[GUARD + written:] == 0x5A).all(), "tag poison"
    assert np.array_equal(d_tags.cpu().numpy()[1:], root_tags) and np.array_equal(d_values.cpu().numpy().view(np.uint64)[:rows], root_values), "the roots were written"
    if raw:
        return rc
    assert rc == 0, (rc, p.last_error())
    return th[GUARD: GUARD + cells].reshape(K, rows).copy(), vh[GUARD: GUARD + cells].reshape(K, rows).copy()


def model(T, roots, pointers):
    """tests/rows_model.py over the distinct roots"""
    tape, sbuf = T.tape.tolist(), T.sbuf.tobytes()
    memo = {}
    tags, values = np.zeros((len(pointers), len(roots[0])), np.uint8), np.zeros((len(pointers), len(roots[0])), np.uint64)
    for r, cell in enumerate(zip(np.asarray(roots[0]).tolist(), np.asarray(roots[1]).tolist())):
        if cell not in memo:
            memo[cell] = [rows_model.walk_from(tape, sbuf, cell, ptr, T.table) for ptr in pointers]
        for k, (t, v) in enumerate(memo[cell]):
            tags[k, r], values[k, r] = t, v
    return tags, values


def assert_columns(got, want, what=""):
    for g, w, name in zip(got, want, ("tags", "values")):
        if not np.array_equal(g, w):
            k, r = np.argwhere(g != w)[0]
            raise AssertionError(f"{what}{name}[{k}, {r}] = {int(g[k, r])}, the model {int(w[k, r])}")


def matches(p, T, path):
    """the matches of one path over all documents: a row of root cells made by sjgpu_at_paths_device"""
    status, offsets, tags, values = column(p, T, [path])
    return tags, values


# ---- 1. the fixture -----------------------------------------------------------------------------------------------------------------------------
def test_fixture_cells_as_roots(parser):
    """every cell the fixture's pointers find in the fixture's documents, hits and failures, is a root of the fixture's pointers"""
    docs, pointers, cells = query_cases.fixture()
    T = Tapes.of_stream(parser, docs)
    parts = [query(parser, T, pointers[first: first + 64]) for first in range(0, len(pointers), 64)]
    roots = (np.concatenate([t for t, _ in parts]).reshape(-1), np.concatenate([v for _, v in parts]).reshape(-1))
    assert len(roots[0]) == len(docs) * len(pointers)
    want = model(T, roots, pointers)
    hits = 0
    for first in range(0, len(pointers), 64):
        got = rooted(parser, T, roots, pointers[first: first + 64])
        assert_columns(got, (want[0][first: first + 64], want[1][first: first + 64]))
        check_containers(got, T)
        hits += int((got[0] >= 34).sum())
    assert b"" in pointers and hits >= (roots[0] >= 34).sum() > 150  # the empty pointer alone finds every root that is an element


def check_containers(got, T):
    """a container cell delimits a sub-tape inside ONE document: its first word opens, its last closes and points back"""
    tags, values = got
    begins = T.table["tape_begin"]
    for k, r in zip(*np.nonzero((tags == ord("{")) | (tags == ord("[")))):
        lo, hi = int(values[k, r]) & 0xFFFFFFFF, int(values[k, r]) >> 32
        d = int(np.searchsorted(begins, lo, side="right")) - 1
        assert int(begins[d]) < lo < hi < int(begins[d + 1])
        assert int(T.tape[lo]) >> 56 == int(tags[k, r]) and int(T.tape[hi - 1]) >> 56 == int(tags[k, r]) + 2
        assert (int(T.tape[hi - 1]) & 0xFFFFFFFF) + int(begins[d]) == lo


# ---- 2. twitter.json as a table -------------------------------------------------------------------------------------------------------------------
def check_twitter(statuses, tags, values, strings=None):
    assert tags.shape == values.shape == (5, 100)
    for r, s in enumerate(statuses):
        assert chr(tags[0, r]) == "l" and int(values[0, r]) == s["user"]["id"]
        text = s["text"].encode()
        assert chr(tags[1, r]) == '"' and int(values[1, r]) >> 32 == len(text)
        if "retweeted_status" in s:
            name = s["retweeted_status"]["user"]["screen_name"].encode()
            assert chr(tags[2, r]) == '"' and int(values[2, r]) >> 32 == len(name)
        else:
            name = b""
            assert (tags[2, r], values[2, r]) == (20, 0)
        if s["entities"]["urls"]:
            url = s["entities"]["urls"][0]["url"].encode()
            assert chr(tags[3, r]) == '"' and int(values[3, r]) >> 32 == len(url)
        else:
            url = b""
            assert (tags[3, r], values[3, r]) == (19, 0)
        assert chr(tags[4, r]) == "{"
        if strings is not None:
            assert [strings[k][r] for k in (1, 2, 3)] == [text, name, url]
    assert (tags[2] == ord('"')).sum() == 73 and (tags[2] == 20).sum() == 27
    assert (tags[3] == ord('"')).sum() == 12 and (tags[3] == 19).sum() == 88
    spans = [(int(v) & 0xFFFFFFFF, int(v) >> 32) for v in values[4]]
    assert all(a < b for a, b in spans) and all(spans[r][1] == spans[r + 1][0] for r in range(99))  # the statuses lie side by side, in order


@pytest.mark.parametrize("wide", [False, True])
def test_twitter_through_table_many(parser, wide):
    data = open(TWITTER, "rb").read()
    statuses = json.loads(data)["statuses"]
    code, docs, row_offsets, tags, values = parser.table_many(data, b"$.statuses[*]", TWITTER_POINTERS, wide=wide)
    assert (code, docs, row_offsets.tolist()) == (0, 1, [0, 100])
    check_twitter(statuses, tags, values)


def test_twitter_strings_and_both_roads_agree(parser):
    """the same table from the entry points themselves, its string columns gathered and compared byte for byte with Python's json"""
    data = open(TWITTER, "rb").read()
    statuses = json.loads(data)["statuses"]
    T = Tapes.of_stream(parser, [data])
    roots = matches(parser, T, b"$.statuses[*]")
    assert len(roots[0]) == 100
    tags, values = rooted(parser, T, roots, TWITTER_POINTERS)
    assert_columns((tags, values), model(T, roots, TWITTER_POINTERS))
    strings = {}
    for k in (1, 2, 3):
        want_total = sum(int(v) >> 32 for t, v in zip(tags[k], values[k]) if t == ord('"'))
        rc, total, offsets, chars = gather(parser, T, tags[k], values[k], want_total=want_total)
        assert (rc, total) == (0, want_total)
        strings[k] = [chars[int(offsets[r]): int(offsets[r + 1])] for r in range(100)]
    check_twitter(statuses, tags, values, strings)
    assert np.array_equal(values[4], roots[1]) and np.array_equal(tags[4], roots[0])  # the empty pointer: the roots themselves
    for wide in (False, True):
        code, docs, row_offsets, t2, v2 = parser.table_many(data, b"$.statuses[*]", TWITTER_POINTERS, wide=wide)
        assert_columns((t2, v2), (tags, values), f"wide={wide}: ")
    # no rows, no pointers, no documents
    code, docs, row_offsets, t0, v0 = parser.table_many(data, b"$.nothing[*]", TWITTER_POINTERS)
    assert (code, docs, row_offsets.tolist(), t0.shape, v0.shape) == (0, 1, [0, 0], (5, 0), (5, 0))
    code, docs, row_offsets, t0, v0 = parser.table_many(data, b"$.statuses[*]", [])
    assert (code, docs, row_offsets.tolist(), t0.shape) == (0, 1, [0, 100], (0, 100))
    assert parser.table_many(b"", b"$[*]", [b"/a"])[:2] == (13, 0)


# ---- 3. workgroup edges, tables of 1, 2 and 4 097 documents ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(parser):
    rng = np.random.default_rng(81)
    docs = stream_cases.small_records(rng, 4097)
    T = Tapes.of_stream(parser, docs)
    roots = matches(parser, T, b"$.*")  # every field of the objects, every element of the arrays: all kinds of cells
    assert len(roots[0]) > 8000 and set(b'{["ldtn') <= set(roots[0].tolist())
    return T, roots


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("rows", [0, 1, 255, 256, 257, 4097])
def test_rows_at_the_workgroup_edges(parser, small, rows, K):
    T, roots = small
    part = (roots[0][:rows], roots[1][:rows])
    pointers = [b"/1", b"", b"/b/c/1/d"][:K]
    if rows == 0:
        assert rooted(parser, T, part, pointers, raw=True) == 0  # nothing written: the poison check inside
        return
    assert_columns(rooted(parser, T, part, pointers), model(T, part, pointers))


def test_all_rows_of_the_small_records_in_any_order(parser, small):
    T, roots = small
    order = np.random.default_rng(82).permutation(len(roots[0]))
    part = (roots[0][order], roots[1][order])
    pointers = [b"", b"/1", b"/b/c/1/d", b"/k", b"/1/0", b"b", b"/-"]
    got = rooted(parser, T, part, pointers)
    assert_columns(got, model(T, part, pointers))
    check_containers(got, T)
    hits = (got[0] >= 34).sum(axis=1)
    assert hits[0] == len(order) and (hits[1:5] > 300).all() and hits[5] == hits[6] == 0, hits


@pytest.mark.parametrize("docs", [1, 2, 4097])
def test_tables_of_one_two_and_many_documents(parser, docs):
    """roots in the first and the last document, on the first and the last element of a document"""
    T = Tapes.of_stream(parser, [b'[{"v":%d,"w":[%d]},%d,"s%d",[%d,{"v":"last"}]]' % (d, d, d, d, d) for d in range(docs)])
    roots = matches(parser, T, b"$[*]")
    assert len(roots[0]) == 4 * docs
    begins = T.table["tape_begin"]
    assert int(roots[1][0]) & 0xFFFFFFFF == 2 and int(roots[1][-1]) >> 32 == int(begins[-1]) - 2  # right behind the first document's opening word, up to the last one's closing word
    pointers = [b"/v", b"/w/0", b"/1/v", b""]
    got = rooted(parser, T, roots, pointers)
    assert_columns(got, model(T, roots, pointers))
    assert np.array_equal(got[1][0][0::4], np.arange(docs, dtype=np.uint64)) and (got[0][2][3::4] == ord('"')).all()
    # the documents' own roots, the first and the last document alone
    whole = query(parser, T, [b""])
    for part in ((whole[0][0], whole[1][0]), (whole[0][0][[0, -1]], whole[1][0][[0, -1]])):
        assert_columns(rooted(parser, T, part, [b"/0/v", b"/3/1/v", b"/4"]), model(T, part, [b"/0/v", b"/3/1/v", b"/4"]))


# ---- 4. roots that are no elements ----------------------------------------------------------------------------------------------------------------
def test_scalar_failed_and_bad_roots_in_one_row(parser):
    docs = [b'[8863084066665136133,"x",{"k":1}]', b'{"a":{"b":[1,2,{"c":"d"}]},"n":12}', b'[[1],[2,3]]', b"7"]
    T = Tapes.of_stream(parser, docs)
    begins = [int(b) for b in T.table["tape_begin"]]
    assert int(T.tape[3]) == (ord("{") << 56) | 5  # a number's value word that reads like an opening word
    a_tag, a_value = (int(x[0, 1]) for x in query(parser, T, [b"/a"]))
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
             (0, 0), (1, 5), (16, 0), (18, 0), (21, 0), (23, 0), (33, 0), (ord("r"), a_value), (ord("}"), a_value), (ord("]"), a_value), (0x5A, P64),
             (255, 1),                                                       # tags that are none
             (17, 0), (19, 9), (20, a_value), (22, 1 << 63),                 # failed roots keep their code
             (ord('"'), (2 << 32) | 4), (ord('"'), 0xFFFFFFFFFFFFFFFF), (ord("l"), 1 << 63), (ord("u"), 7), (ord("d"), 0), (ord("t"), 1), (ord("f"), 0), (ord("n"), 0)]
    roots = (np.array([t for t, _ in cells], np.uint8), np.array([v for _, v in cells], np.uint64))
    pointers = [b"", b"/b", b"/b/2/c", b"b", b"/~", b"/k", b"/0"]
    tags, values = rooted(parser, T, roots, pointers)
    assert_columns((tags, values), model(T, roots, pointers))
    assert [chr(t) for t in tags[:3, 0]] == ["{", "[", '"'] and tags[3, 0] == 22
    bad = list(range(1, 13)) + [15, 16] + list(range(17, 30))
    assert (tags[:, bad] == 20).all() and (values[:, bad] == 0).all()
    assert tags[0, 14] == ord("{") and (tags[1:, 14] == [20, 20, 22, 22, 20, 20]).all()  # (the value word agrees with the cell made for it: an object without fields)
    for j, code in zip(range(30, 34), (17, 19, 20, 22)):
        assert (tags[:, j] == code).all() and (values[:, j] == 0).all()
    scalars = list(range(34, 42)) + [13]
    assert np.array_equal(tags[0, scalars], roots[0][scalars]) and np.array_equal(values[0, scalars], roots[1][scalars])
    assert (tags[1:, scalars] == np.array([20, 20, 22, 22, 20, 20])[:, None]).all() and (values[1:, scalars] == 0).all()
    # a table without documents: no container root has one
    tags, values = rooted(parser, T, roots, pointers, docs=0)
    containers = [j for j, (t, _) in enumerate(cells) if t in (ord("{"), ord("["))]
    assert (tags[:, containers] == 20).all() and (values[:, containers] == 0).all() and np.array_equal(tags[0, scalars], roots[0][scalars])


# ---- 5. the calls compose -------------------------------------------------------------------------------------------------------------------------
def test_the_output_is_an_input_of_the_call_and_of_the_gather(parser):
    rng = np.random.default_rng(83)
    docs = [b'{"id":%d,"user":{"name":"user %d","langs":["en","%s"],"geo":{"lat":%d.5}},"tags":[{"t":"a%d"},{"t":"b"}]}' % (k, k, b"x" * int(rng.integers(0, 40)), k % 90, k)
            if k % 5 else b'{"id":%d,"user":null}' % k for k in range(3000)]
    T = Tapes.of_stream(parser, docs)
    whole = query(parser, T, [b""])
    roots = (whole[0][0], whole[1][0])
    first = rooted(parser, T, roots, [b"/user", b"/tags/0", b"/id"])
    assert_columns(first, model(T, roots, [b"/user", b"/tags/0", b"/id"]))
    assert (first[0][0] == ord("{")).sum() == 2400 and (first[0][0] == ord("n")).sum() == 600 and (first[0][1] == 20).sum() == 600
    # row 0 (objects and nulls), row 1 (objects and failures) and row 2 (numbers) as roots
    for k, pointers in ((0, [b"/name", b"/langs/1", b"/geo/lat", b""]), (1, [b"/t", b"/t/x", b"t"]), (2, [b"", b"/0"])):
        part = (first[0][k], first[1][k])
        second = rooted(parser, T, part, pointers)
        assert_columns(second, model(T, part, pointers))
        if k == 0:
            # a.at_pointer(b) is at_pointer(a + b) wherever the first call succeeded
            direct = query(parser, T, [b"/user/name", b"/user/langs/1", b"/user/geo/lat", b"/user"])
            assert_columns(second, direct, "composed against direct: ")
            names = [b"user %d" % d if d % 5 else b"" for d in range(3000)]
            rc, total, offsets, chars = gather(parser, T, second[0][0], second[1][0], want_total=sum(len(n) for n in names))
            assert rc == 0 and chars == b"".join(names) and np.array_equal(offsets, np.concatenate([[0], np.cumsum([len(n) for n in names])]).astype(np.uint32))
            lats = [struct.unpack("<d", struct.pack("<Q", int(v)))[0] for t, v in zip(second[0][2], second[1][2]) if t == ord("d")]
            assert lats == [d % 90 + 0.5 for d in range(3000) if d % 5]
            third = rooted(parser, T, (second[0][3], second[1][3]), [b"/langs/0"])  # ... and once more
            assert_columns(third, query(parser, T, [b"/user/langs/0"]))
        if k == 1:
            assert (second[0][0][first[0][1] == 20] == 20).all() and (second[0][2] == np.where(first[0][1] == 20, 20, 22)).all()


# ---- 6. contract ----------------------------------------------------------------------------------------------------------------------------------
def test_contract(parser):
    import torch
    rng = np.random.default_rng(84)
    T = Tapes.of_stream(parser, stream_cases.small_records(rng, 300))
    roots = matches(parser, T, b"$.*")
    pointers = [b"/1", b"", b"/b/c"]
    base = rooted(parser, T, roots, pointers)
    assert rooted(parser, T, roots, [], raw=True) == 0 and rooted(parser, T, (roots[0][:0], roots[1][:0]), pointers, raw=True) == 0  # nothing written: the poison check inside
    assert rooted(parser, T, roots, pointers, raw=True, tape_ptr=T.d_tape.data_ptr() + 4) == E_BADARG
    assert rooted(parser, T, roots, pointers, raw=True, table_ptr=T.d_table.data_ptr() + 8) == E_BADARG
    assert rooted(parser, T, roots, pointers, raw=True, value_skew=4) == E_BADARG
    assert rooted(parser, T, roots, pointers, raw=True, root_skew=4) == E_BADARG
    assert rooted(parser, T, roots, [b"/a"] * 65, raw=True) == E_BADARG and rooted(parser, T, roots, [b"/a"] * 64, raw=True) == 0
    assert rooted(parser, T, roots, [b"/" + b"a" * 1024], raw=True) == E_BADARG and rooted(parser, T, roots, [b"/" + b"a" * 1023], raw=True) == 0
    assert rooted(parser, T, roots, [b"/a" * 33], raw=True) == E_BADARG and rooted(parser, T, roots, [b"/a" * 32], raw=True) == 0
    for field in ("tape_begin", "string_begin"):
        table = T.table.copy()
        table[field][[100, 101]] = table[field][[101, 100]]
        assert table[field][100] > table[field][101]
        back = torch.from_numpy(table.view(np.int32)).cuda()
        assert rooted(parser, T, roots, pointers, raw=True, table_ptr=back.data_ptr()) == E_BADARG
    table = T.table.copy()
    table["tape_begin"][-1] += 1  # ends behind the tape
    assert rooted(parser, T, roots, pointers, raw=True, table_ptr=torch.from_numpy(table.view(np.int32)).cuda().data_ptr()) == E_BADARG
    # null pointers, one at a time
    ok = torch.zeros(64, dtype=torch.int64, device="cuda")
    lens = np.array([2], np.uint32)
    good = [parser.h, T.d_tape.data_ptr(), len(T.tape), T.d_sbuf.data_ptr(), len(T.sbuf), T.d_table.data_ptr(), T.docs, ok.data_ptr(), ok.data_ptr(), 1,
            ctypes.cast(ctypes.c_char_p(b"/a"), ctypes.c_void_p), lens.ctypes.data, 1, ok.data_ptr() + 64, ok.data_ptr() + 128, T.stream]
    for at in (0, 1, 3, 5, 7, 8, 10, 11, 13, 14):
        args = list(good)
        args[at] = None
        assert parser.L.sjgpu_at_pointers_from_cells_device(*args) == E_BADARG, at
    assert parser.L.sjgpu_at_pointers_from_cells_device(*good) == 0
    torch.cuda.synchronize()
    # a pointer without its leading slash is INVALID_JSON_POINTER for every root that is an element, and its neighbours' rows are what they were
    tags, values = rooted(parser, T, roots, [b"1"] + pointers)
    assert (tags[0] == 22).all() and (values[0] == 0).all()
    assert_columns((tags[1:], values[1:]), base)
    # the sibling call is what it was: the documents' roots through it and through this call are one column
    whole = query(parser, T, [b"", b"/1", b"/b/c"])
    again = rooted(parser, T, (whole[0][0], whole[1][0]), [b"", b"/1", b"/b/c"])
    assert_columns(again, whole)
