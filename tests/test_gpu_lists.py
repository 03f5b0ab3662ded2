"""GPU tier (-m gpu): list columns over device tapes -- sjgpu_at_paths_from_cells_device (k_rows_locate and k_at_paths_rooted in sjgpu_query.hip,
include/sjgpu_lists.h) and capi.lists_many -- against tests/lists_model.py (pinned against tests/golden/lists.json and tests/golden/paths.json on the CPU
tier) and against Python's json.  The tapes are the device's own (sjgpu_stage2_many_device), the roots what sjgpu_at_paths_device, sjgpu_at_pointers_device
and the call itself delivered.  Every output has exactly the contracted size inside a poisoned tensor whose poison is checked after every call, and its
status and tag rows and the root tags begin at odd addresses."""
import ctypes
import json
import os

import numpy as np
import pytest

import lists_model
import path_cases
import pointer_model
import stream_cases
from simdjson_amd import _paths, build, capi
from test_gpu_paths import column as flat_column
from test_gpu_query import Tapes, gather, query
from test_gpu_rows import rooted as rooted_pointers
from test_lists_model import fixture

pytestmark = pytest.mark.gpu

CAP = 128 << 20
E_BADARG, E_OVERFLOW = -4, -5
GUARD = 65  # odd: with it the status and tag rows begin at odd addresses
P64, P32, P8 = 0x5A5A5A5A5A5A5A5A, 0x5A5A5A5A, 0x5A
TWITTER = os.path.join(_paths.REPO_ROOT, "tests", "golden", "jsonexamples", "twitter.json")
TWITTER_PATHS = [b"$.entities.hashtags[*].text", b"$.entities.user_mentions[*].screen_name", b"$.entities.urls[*]", b"$.retweeted_status.user.id"]


@pytest.fixture(scope="module")
def parser():
    build.build_sjgpu()
    p = capi.DomParserImplementation(CAP)
    yield p
    p.close()


def call(p, T, roots, paths, cap, docs=None, table_ptr=None, tape_ptr=None, offsets_skew=0, value_skew=0, root_skew=0, expect=None):
    """one sjgpu_at_paths_from_cells_device over the roots (tags[rows], values[rows]) with outputs of exactly K * rows + 1 words, K * rows bytes and `cap` matches
    between poisoned guards -> (rc, matches, status[K, rows], offsets[K * rows + 1], tags[matches], values[matches]); expect: the rc the caller counts on"""
    torch = T.torch
    root_tags, root_values = np.ascontiguousarray(roots[0], np.uint8), np.ascontiguousarray(roots[1], np.uint64)
    rows, K = len(root_tags), len(paths)
    cells = K * rows
    d_tags = torch.from_numpy(np.concatenate([np.zeros(1, np.uint8), root_tags])).cuda()
    d_values = torch.from_numpy(np.concatenate([root_values, np.zeros(1, np.uint64)]).view(np.int64)).cuda()  # (never empty: an address to pass)
    offsets = torch.full((cells + 1 + 2 * GUARD,), P32, dtype=torch.int32, device="cuda")
    status = torch.full((cells + 2 * GUARD,), P8, dtype=torch.uint8, device="cuda")
    values = torch.full((cap + 2 * GUARD,), P64, dtype=torch.int64, device="cuda")
    tags = torch.full((cap + 2 * GUARD,), P8, dtype=torch.uint8, device="cuda")
    rc, matches = p.at_paths_from_cells_device(tape_ptr or T.d_tape.data_ptr(), len(T.tape), T.d_sbuf.data_ptr(), len(T.sbuf), table_ptr or T.d_table.data_ptr(),
                                               T.docs if docs is None else docs, d_values.data_ptr() + root_skew, d_tags.data_ptr() + 1, rows, paths,
                                               offsets.data_ptr() + 4 * GUARD + offsets_skew, status.data_ptr() + GUARD, values.data_ptr() + 8 * GUARD + value_skew,
                                               tags.data_ptr() + GUARD, cap, T.stream)
    torch.cuda.synchronize()
    oh, sh = offsets.cpu().numpy().view(np.uint32), status.cpu().numpy()
    vh, th = values.cpu().numpy().view(np.uint64), tags.cpu().numpy()
    if expect is not None:
        assert rc == expect, (rc, expect, p.last_error())
    nothing = rc == E_BADARG
    empty = K == 0 or rows == 0
    wrote_offsets = 0 if nothing else (1 if empty else cells + 1)
    wrote_status = 0 if nothing or empty else cells
    wrote_matches = matches if rc == 0 else 0
    assert (oh[:GUARD] == P32).all() and (oh[GUARD + wrote_offsets:] == P32).all(), "offsets poison"
    assert (sh[:GUARD] == P8).all() and (sh[GUARD + wrote_status:] == P8).all(), "status poison"
    assert (vh[:GUARD] == P64).all() and (vh[GUARD + wrote_matches:] == P64).all(), "value poison"
    assert (th[:GUARD] == P8).all() and (th[GUARD + wrote_matches:] == P8).all(), "tag poison"
    assert np.array_equal(d_tags.cpu().numpy()[1:], root_tags) and np.array_equal(d_values.cpu().numpy().view(np.uint64)[:rows], root_values), "the roots were written"
    return (rc, matches, sh[GUARD: GUARD + wrote_status].reshape(K, -1).copy() if wrote_status else np.zeros((K, rows), np.uint8), oh[GUARD: GUARD + wrote_offsets].copy(),
            th[GUARD: GUARD + wrote_matches].copy(), vh[GUARD: GUARD + wrote_matches].copy())


def column(p, T, roots, paths, docs=None):
    """the list column at its EXACT capacity: a call with room for nothing (and null outputs' worth of it) says what is needed and leaves offsets and status
    complete, the second fills -> (status, offsets, tags, values)"""
    rc, matches, status0, offsets0, _, _ = call(p, T, roots, paths, 0, docs)
    if matches == 0:
        assert rc == 0
        return status0, offsets0, np.zeros(0, np.uint8), np.zeros(0, np.uint64)
    assert rc == E_OVERFLOW and int(offsets0[-1]) == matches
    rc, again, status, offsets, tags, values = call(p, T, roots, paths, matches, docs, expect=0)
    assert again == matches and np.array_equal(status, status0) and np.array_equal(offsets, offsets0)
    return status, offsets, tags, values


def model(T, roots, paths):
    """tests/lists_model.py over the distinct roots"""
    S = lists_model.Stream(T.tape, T.sbuf, T.table)
    memo = {}
    status = np.zeros((len(paths), len(roots[0])), np.uint8)
    cells = list(zip(np.asarray(roots[0]).tolist(), np.asarray(roots[1]).tolist()))
    for cell in cells:
        if cell not in memo:
            memo[cell] = [S.matches_from(cell, path) for path in paths]
    offsets, tags, values = [0], [], []
    for k in range(len(paths)):
        for r, cell in enumerate(cells):
            code, found = memo[cell][k]
            status[k, r] = code
            for t, v in found:
                tags.append(t)
                values.append(v)
            offsets.append(len(tags))
    return status, np.array(offsets, np.uint32), np.array(tags, np.uint8), np.array(values, np.uint64)


def matches(p, T, path):
    """the matches of one path over all documents: a row of root cells made by sjgpu_at_paths_device"""
    status, offsets, tags, values = flat_column(p, T, [path])
    return tags, values


# ---- 1. the fixture -----------------------------------------------------------------------------------------------------------------------------
def test_fixture_rows_from_the_paths_and_from_the_pointers(parser):
    docs, row_paths, paths, tables = fixture()
    T = Tapes.of_stream(parser, docs)
    rows = [matches(parser, T, rp) for rp in row_paths]
    # against the fixture itself: the rows of each row path, document by document
    sbuf = T.sbuf.tobytes()
    for j, (rp, roots) in enumerate(zip(row_paths, rows)):
        status, offsets, tags, values = column(parser, T, roots, paths)
        want = [row for i in range(len(docs)) for row in tables[i][j]]
        assert len(want) == len(roots[0])
        for r, row in enumerate(want):
            for k in range(len(paths)):
                assert path_cases.render(*path_cases.cell(status, offsets, tags, values, k, r, len(want)), sbuf) == row[k], (rp, r, paths[k])
    # all of them as one row, and a row of sjgpu_at_pointers_device's cells (hits and failures), against the model
    roots = (np.concatenate([t for t, _ in rows]), np.concatenate([v for _, v in rows]))
    got = column(parser, T, roots, paths)
    path_cases.assert_column(got, model(T, roots, paths))
    path_cases.check_container_matches(got[2], got[3], T.tape)
    cells = query(parser, T, [b"", b"/a", b"/0", b"/statuses", b"/k", b"/missing", b"/a/0", b"x"])
    roots = (cells[0].reshape(-1), cells[1].reshape(-1))
    assert {17, 19, 20, 22, ord("{"), ord("["), ord("l"), ord('"')} <= set(roots[0].tolist())
    got = column(parser, T, roots, paths)
    path_cases.assert_column(got, model(T, roots, paths))
    assert {0, 17, 19, 20, 22} <= set(got[0].reshape(-1).tolist()) and len(got[2]) > 300


# ---- 2. twitter.json: the lists of each status ------------------------------------------------------------------------------------------------------
def check_twitter(statuses, status, offsets, tags, values, strings=None):
    assert status.shape == (4, 100) and len(offsets) == 401
    counts = np.diff(offsets.astype(np.int64)).reshape(4, 100)
    want = [[h["text"].encode() for h in s["entities"]["hashtags"]] for s in statuses]
    mentions = [[m["screen_name"].encode() for m in s["entities"]["user_mentions"]] for s in statuses]
    urls = [len(s["entities"]["urls"]) for s in statuses]
    assert counts[0].tolist() == [len(w) for w in want] and counts[0].sum() == 8 and (counts[0] > 0).sum() == 7 and counts[0].max() == 2
    assert counts[1].tolist() == [len(m) for m in mentions] and counts[1].sum() == 87 and (counts[1] > 0).sum() == 83 and counts[1].max() == 3
    assert counts[2].tolist() == urls and counts[2].sum() == 13
    assert (status[:3] == 0).all()
    retweets = ["retweeted_status" in s for s in statuses]
    assert counts[3].tolist() == [int(r) for r in retweets] and status[3].tolist() == [0 if r else 20 for r in retweets] and sum(retweets) == 73
    lo = int(offsets[300])
    assert [int(v) for v in values[lo:]] == [s["retweeted_status"]["user"]["id"] for s in statuses if "retweeted_status" in s] and (tags[lo:] == ord("l")).all()
    assert (tags[: int(offsets[200])] == ord('"')).all() and (tags[int(offsets[200]): lo] == ord("{")).all()
    assert [int(v) >> 32 for v in values[: int(offsets[200])]] == [len(x) for per in want + mentions for x in per]
    if strings is not None:
        for k, per_row in enumerate((want, mentions)):
            for r in range(100):
                assert strings[int(offsets[k * 100 + r]): int(offsets[k * 100 + r + 1])] == per_row[r], (k, r)


@pytest.mark.parametrize("wide", [False, True])
def test_twitter_through_lists_many(parser, wide):
    data = open(TWITTER, "rb").read()
    statuses = json.loads(data)["statuses"]
    code, docs, row_offsets, status, offsets, tags, values = parser.lists_many(data, b"$.statuses[*]", TWITTER_PATHS, wide=wide)
    assert (code, docs, row_offsets.tolist()) == (0, 1, [0, 100])
    check_twitter(statuses, status, offsets, tags, values)
    # the same column from the entry points themselves, its strings gathered and compared byte for byte with Python's json
    T = Tapes.of_stream(parser, [data])
    roots = matches(parser, T, b"$.statuses[*]")
    got = column(parser, T, roots, TWITTER_PATHS)
    path_cases.assert_column((status, offsets, tags, values), got, f"wide={wide}: ")
    path_cases.assert_column(got, model(T, roots, TWITTER_PATHS))
    n = int(offsets[200])  # the two string columns
    want_total = sum(int(v) >> 32 for v in values[:n])
    rc, total, goffsets, chars = gather(parser, T, tags, values, want_total=want_total)  # (the containers and numbers behind them are strings of no bytes)
    assert (rc, total) == (0, want_total)
    check_twitter(statuses, status, offsets, tags, values, [chars[int(goffsets[i]): int(goffsets[i + 1])] for i in range(len(tags))])
    # a first guess that is too small, no rows, no paths, no input
    for first_cap in (0, len(tags) - 1):
        again = parser.lists_many(data, b"$.statuses[*]", TWITTER_PATHS, wide=wide, first_cap=first_cap)
        path_cases.assert_column(again[3:], got)
    code, docs, row_offsets, s0, o0, t0, v0 = parser.lists_many(data, b"$.nothing[*]", TWITTER_PATHS, wide=wide)
    assert (code, docs, row_offsets.tolist(), s0.shape, o0.tolist(), t0.size) == (0, 1, [0, 0], (4, 0), [0], 0)
    code, docs, row_offsets, s0, o0, t0, v0 = parser.lists_many(data, b"$.statuses[*]", [], wide=wide)
    assert (code, docs, row_offsets.tolist(), s0.shape, o0.tolist()) == (0, 1, [0, 100], (0, 100), [0])
    assert parser.lists_many(b"", b"$[*]", [b"$[*]"])[:2] == (13, 0)


# ---- 3. three levels --------------------------------------------------------------------------------------------------------------------------------
def test_three_levels_equal_the_flat_path(parser):
    data = open(TWITTER, "rb").read()
    T = Tapes.of_stream(parser, [data])
    level1 = matches(parser, T, b"$.statuses[*]")
    s2, o2, t2, v2 = column(parser, T, level1, [b"$.entities.hashtags[*]"])
    s3, o3, t3, v3 = column(parser, T, (t2, v2), [b"$.indices[*]"])
    assert len(t2) == 8 and np.diff(o3.astype(np.int64)).tolist() == [2] * 8 and (t3 == ord("l")).all()
    flat = flat_column(parser, T, [b"$.statuses[*].entities.hashtags[*].indices[*]"])
    assert len(flat[2]) == 16 and np.array_equal(flat[2], t3) and np.array_equal(flat[3], v3)
    statuses = json.loads(data)["statuses"]
    assert [int(v) for v in v3] == [i for s in statuses for h in s["entities"]["hashtags"] for i in h["indices"]]


@pytest.fixture(scope="module")
def small(parser):
    rng = np.random.default_rng(91)
    docs = stream_cases.small_records(rng, 4097)
    T = Tapes.of_stream(parser, docs)
    roots = matches(parser, T, b"$.*")  # every field of the objects, every element of the arrays: all kinds of cells
    assert len(roots[0]) > 8000 and set(b'{["ldtn') <= set(roots[0].tolist())
    return T, roots


def test_the_law_on_the_small_records(parser, small):
    """the matches of A + B from the documents' roots are, in order, the rooted matches of B over the matches of A"""
    T, _ = small
    for a, b, c in ((b"$.f[*]", b"$[*]", None), (b"$.a.b.c[*]", b".d", None), (b"$.*", b"[*]", b"$[*]"), (b"$[*]", b".k[*]", None), (b"$.*", b"$.b.c[*]", b"$.d")):
        rows = matches(parser, T, a)
        status, offsets, tags, values = column(parser, T, rows, [b])
        whole = a + (b[1:] if b[:1] == b"$" else b)
        if c is not None:
            status, offsets, tags, values = column(parser, T, (tags, values), [c])
            whole += c[1:] if c[:1] == b"$" else c
        flat = flat_column(parser, T, [whole])
        assert np.array_equal(flat[2], tags) and np.array_equal(flat[3], values), whole
        if whole != b"$[*].k[*]":  # (every `k` of the records is an empty array)
            assert len(tags) > 300, whole


# ---- 4. workgroup edges, the scan's second level, tables of 1, 2 and 4 097 documents -------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("rows", [0, 1, 255, 256, 257, 4097])
def test_rows_at_the_workgroup_edges(parser, small, rows, K):
    T, roots = small
    part = (roots[0][:rows], roots[1][:rows])
    paths = [b"$[*]", b".b.c[*].d", b"$.*"][:K]
    got = column(parser, T, part, paths)
    if rows == 0:
        assert got[1].tolist() == [0]
        return
    path_cases.assert_column(got, model(T, part, paths))
    assert rows < 255 or len(got[2]) > 30


def test_all_rows_of_the_small_records_in_any_order(parser, small):
    T, roots = small
    order = np.random.default_rng(92).permutation(len(roots[0]))
    part = (roots[0][order], roots[1][order])
    paths = [b"$[*]", b".*", b"$.b.c[*].d", b"$[*][*]", b"$.k", b"", b"$[1]"]
    got = column(parser, T, part, paths)
    path_cases.assert_column(got, model(T, part, paths))
    path_cases.check_container_matches(got[2], got[3], T.tape)
    counts = np.diff(got[1].astype(np.int64)).reshape(len(paths), -1).sum(axis=1)
    assert (counts[:5] > 300).all() and counts[5] == 0 and counts[6] > 300, counts
    assert set(got[0][5].tolist()) == {0, 22} and set(got[0][6].tolist()) == {0, 20}  # (scalar rows: 0; `/1` asked of the objects among the rows: 20; every array has two elements)


@pytest.mark.parametrize("docs", [1, 2, 4097])
def test_tables_of_one_two_and_many_documents(parser, docs):
    """roots in the first and the last document, on the first and the last element of a document"""
    T = Tapes.of_stream(parser, [b'[{"v":%d,"w":[%d]},%d,"s%d",[%d,{"v":"last"}]]' % (d, d, d, d, d) for d in range(docs)])
    roots = matches(parser, T, b"$[*]")
    assert len(roots[0]) == 4 * docs
    begins = T.table["tape_begin"]
    assert int(roots[1][0]) & 0xFFFFFFFF == 2 and int(roots[1][-1]) >> 32 == int(begins[-1]) - 2  # right behind the first document's opening word, up to the last one's closing word
    paths = [b"$.w[*]", b"$[*]", b"$[*].v", b"$.v"]
    got = column(parser, T, roots, paths)
    path_cases.assert_column(got, model(T, roots, paths))
    counts = np.diff(got[1].astype(np.int64)).reshape(4, docs, 4)
    assert (counts == np.array([[1, 0, 0, 0], [2, 0, 0, 2], [0, 0, 0, 1], [1, 0, 0, 0]])[:, None, :]).all()  # (a wildcard gives an object's values too)
    assert (got[0][3].reshape(docs, 4) == [0, 0, 0, 17]).all() and (got[0][:3] == 0).all()  # `.v` asked of the array row
    assert np.array_equal(got[3][:docs], np.arange(docs, dtype=np.uint64))
    # the documents' own roots, the first and the last document alone: the column of sjgpu_at_paths_device
    whole = query(parser, T, [b""])
    flat = flat_column(parser, T, [b"$[*].w[*]", b"$[3][*]"])
    path_cases.assert_column(column(parser, T, (whole[0][0], whole[1][0]), [b"$[*].w[*]", b"$[3][*]"]), flat)
    ends = (whole[0][0][[0, -1]], whole[1][0][[0, -1]])
    path_cases.assert_column(column(parser, T, ends, [b"$[3][*]"]), model(T, ends, [b"$[3][*]"]))


# ---- 5. roots that are no elements ----------------------------------------------------------------------------------------------------------------
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
    paths = [b"$.b[*]", b"$.*", b"$.b", b"", b"b[*]", b"$.b[*].c", b"$.x"]
    got = column(parser, T, roots, paths)
    path_cases.assert_column(got, model(T, roots, paths))
    status, offsets, tags, values = got
    counts = np.diff(offsets.astype(np.int64)).reshape(len(paths), len(cells))
    assert counts[:, 0].tolist() == [3, 1, 1, 0, 0, 1, 0] and status[:, 0].tolist() == [0, 0, 0, 22, 22, 0, 20] and (counts[:, 1:] == 0).all()
    bad = list(range(1, 13)) + [15, 16] + list(range(17, 30))
    assert (status[:, bad] == 20).all()
    assert status[:, 14].tolist() == [0, 0, 20, 22, 22, 0, 20]  # (the value word agrees with the cell made for it: an object without fields)
    for j, code in zip(range(30, 34), (17, 19, 20, 22)):
        assert (status[:, j] == code).all()
    scalars = list(range(34, 42)) + [13]
    assert (status[:, scalars] == 0).all()
    # a table without documents: no container root has one
    status, offsets, tags, values = column(parser, T, roots, paths, docs=0)
    containers = [j for j, (t, _) in enumerate(cells) if t in (ord("{"), ord("["))]
    assert (status[:, containers] == 20).all() and (status[:, scalars] == 0).all() and int(offsets[-1]) == 0 and (status[:, 30:34] == [17, 19, 20, 22]).all()


# ---- 6. capacities --------------------------------------------------------------------------------------------------------------------------------
def test_capacities(parser, small):
    T, roots = small
    part = (roots[0][:1000], roots[1][:1000])
    paths = [b"$[*]", b"$.b.c[*].d"]
    status, offsets, tags, values = column(parser, T, part, paths)  # (capacity 0, then exact: inside)
    n = len(tags)
    assert n > 100
    rc, matches, s1, o1, t1, v1 = call(parser, T, part, paths, n - 1, expect=E_OVERFLOW)  # one short: nothing written (the poison check inside), the rest complete
    assert matches == n and np.array_equal(s1, status) and np.array_equal(o1, offsets) and t1.size == 0
    rc, matches, s1, o1, t1, v1 = call(parser, T, part, paths, n + 3, expect=0)  # room to spare: only the matches are written
    assert matches == n and np.array_equal(t1, tags) and np.array_equal(v1, values)
    # match_cap == 0 with null outputs: what is needed is reported, and nothing that matches nothing needs them
    import torch
    d_tags = torch.from_numpy(np.concatenate([np.zeros(1, np.uint8), part[0]])).cuda()
    d_values = torch.from_numpy(part[1].view(np.int64)).cuda()
    out_offsets = torch.zeros(2 * 1000 + 1, dtype=torch.int32, device="cuda")
    out_status = torch.zeros(2 * 1000, dtype=torch.uint8, device="cuda")

    def null_outputs(paths):
        return parser.at_paths_from_cells_device(T.d_tape.data_ptr(), len(T.tape), T.d_sbuf.data_ptr(), len(T.sbuf), T.d_table.data_ptr(), T.docs, d_values.data_ptr(),
                                                 d_tags.data_ptr() + 1, 1000, paths, out_offsets.data_ptr(), out_status.data_ptr(), 0, 0, 0, T.stream)
    assert null_outputs(paths) == (E_OVERFLOW, n) and np.array_equal(out_offsets.cpu().numpy().view(np.uint32), offsets)
    assert null_outputs([b"$.nothing[*]", b"$.nothing"]) == (0, 0) and set(out_status.cpu().numpy()[1000:].tolist()) <= {0, 17, 20}


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_refusals(parser):
    import torch
    rng = np.random.default_rng(94)
    T = Tapes.of_stream(parser, stream_cases.small_records(rng, 300))
    roots = matches(parser, T, b"$.*")
    paths = [b"$[*]", b"", b"$.b.c[*]"]
    base = column(parser, T, roots, paths)

    def refused(paths=paths, **kw):
        return call(parser, T, roots, paths, len(base[2]), **kw)[0] == E_BADARG  # (nothing written: the poison check inside)
    assert refused(tape_ptr=T.d_tape.data_ptr() + 4) and refused(table_ptr=T.d_table.data_ptr() + 8) and refused(value_skew=4) and refused(offsets_skew=2) and refused(root_skew=4)
    assert refused([b"$[*]"] * 65) and not refused([b"$[*]"] * 64)
    assert refused([b"$." + b"a" * 1023]) and not refused([b"$." + b"a" * 1022])                # 1 025 bytes, 1 024
    assert refused([b"$" + b".a" * 32 + b"[*]"]) and not refused([b"$" + b".a" * 31 + b"[*]"])  # 33 levels, 32
    assert refused([b"$" + b"[*]" * 9]) and not refused([b"$" + b"[*]" * 8])                    # 9 wildcards, 8
    assert refused([b"$" + b".a" * 33]) and not refused([b"$" + b".a" * 32])                    # 33 pointer tokens, 32
    for field in ("tape_begin", "string_begin"):
        table = T.table.copy()
        table[field][[100, 101]] = table[field][[101, 100]]
        assert table[field][100] > table[field][101]
        back = torch.from_numpy(table.view(np.int32)).cuda()
        assert refused(table_ptr=back.data_ptr())
    table = T.table.copy()
    table["tape_begin"][-1] += 1  # ends behind the tape
    assert refused(table_ptr=torch.from_numpy(table.view(np.int32)).cuda().data_ptr())
    # null pointers, one at a time, and K * rows + 1 beyond what the scan indexes: refused before anything is read
    ok = torch.zeros(256, dtype=torch.int64, device="cuda")
    lens = np.array([4], np.uint32)
    total = ctypes.c_uint64(7)
    good = [parser.h, T.d_tape.data_ptr(), len(T.tape), T.d_sbuf.data_ptr(), len(T.sbuf), T.d_table.data_ptr(), T.docs, ok.data_ptr(), ok.data_ptr() + 64, 1,
            ctypes.cast(ctypes.c_char_p(b"$[*]"), ctypes.c_void_p), lens.ctypes.data, 1, ok.data_ptr() + 128, ok.data_ptr() + 192, ok.data_ptr() + 256, ok.data_ptr() + 320, 8,
            T.stream, ctypes.byref(total)]
    f = parser.L.sjgpu_at_paths_from_cells_device
    for at in (0, 1, 3, 5, 7, 8, 10, 11, 13, 14, 15, 16, 19):
        args = list(good)
        args[at] = None
        assert f(*args) == E_BADARG, at
    many = list(good)
    blob, lens64 = b"$[*]" * 64, np.full(64, 4, np.uint32)
    many[9], many[10], many[11], many[12] = 1 << 26, ctypes.cast(ctypes.c_char_p(blob), ctypes.c_void_p), lens64.ctypes.data, 64
    assert f(*many) == E_BADARG and total.value == 0
    many[9] = 0xFFFFFFF0
    many[12] = 1
    assert f(*many) == E_BADARG
    assert f(*good) == 0 and total.value == 0  # (the root cell is a zero: no tag, status 20)
    torch.cuda.synchronize()
    assert int(ok[16].item()) & 0xFFFFFFFF == 0 and int(ok[24].item()) & 0xFF == 20
    # the neighbours of a call that was refused are what they were, and the sibling call is what it was
    path_cases.assert_column(column(parser, T, roots, paths), base)
    whole = query(parser, T, [b""])
    flat_paths = [b"$.tags[*]", b"$[*]", b"$.name"]
    path_cases.assert_column(column(parser, T, (whole[0][0], whole[1][0]), flat_paths), flat_column(parser, T, flat_paths))


# ---- 8. composition -------------------------------------------------------------------------------------------------------------------------------
def test_the_output_is_a_row_of_roots_for_the_pointers(parser):
    docs = [b'{"id":%d,"tags":[{"t":"a%d","n":[%d,2]},{"t":"b"}],"u":{"langs":["en","x%d"]}}' % (k, k, k, k) if k % 5 else b'{"id":%d,"tags":null}' % k for k in range(3000)]
    T = Tapes.of_stream(parser, docs)
    whole = query(parser, T, [b""])
    roots = (whole[0][0], whole[1][0])
    status, offsets, tags, values = column(parser, T, roots, [b"$.tags[*]", b"$.u.langs[*]"])
    path_cases.assert_column((status, offsets, tags, values), model(T, roots, [b"$.tags[*]", b"$.u.langs[*]"]))
    assert int(offsets[3000]) == 4800 and len(tags) == 9600
    cells = rooted_pointers(parser, T, (tags, values), [b"/t", b"/n/0", b""])
    direct = query(parser, T, [b"/tags/0/t", b"/tags/0/n/0", b"/tags/1/t"])
    keep = np.array([k % 5 != 0 for k in range(3000)])
    assert np.array_equal(cells[0][0][:4800:2], direct[0][0][keep]) and np.array_equal(cells[1][0][:4800:2], direct[1][0][keep])
    assert np.array_equal(cells[1][1][:4800:2], np.arange(3000, dtype=np.uint64)[keep]) and (cells[0][1][1:4800:2] == 20).all()
    assert np.array_equal(cells[1][0][1:4800:2], direct[1][2][keep]) and (cells[0][0][4800:] == 20).all()  # (the strings of the second column answer `/t` as scalars do)
    assert np.array_equal(cells[0][2], tags) and np.array_equal(cells[1][2], values)
    strings = [pointer_model.string_of(T.sbuf, int(v)) for v in values[4800:]]
    assert strings == [x for k in range(3000) if k % 5 for x in (b"en", b"x%d" % k)]
