"""GPU tier (-m gpu): map columns over device tapes -- sjgpu_object_fields_from_cells_device and sjgpu_cell_sizes_device (k_rows_locate, k_object_fields_count,
k_object_fields_fill and k_cell_sizes in sjgpu_query.hip, include/sjgpu_fields.h) and capi.fields_many -- against tests/fields_model.py (pinned against
tests/golden/fields.json, tests/golden/lists.json and tests/golden/paths.json on the CPU tier) and against Python's json.  The tapes are the device's own
(sjgpu_stage2_many_device), the roots what sjgpu_at_paths_device, sjgpu_at_pointers_device, sjgpu_at_pointers_from_cells_device and the call itself delivered.
Every output has exactly the contracted size inside a poisoned tensor whose poison is checked after every call, the status, tag and code rows and the root tags
begin at odd addresses, and every column is made twice: with capacity 0, then at the capacity that call reported."""
import ctypes
import json
import os
import struct

import numpy as np
import pytest

import fields_model
import pointer_model
import stream_cases
from simdjson_amd import _paths, build, capi
from test_fields_model import fixture
from test_gpu_paths import column as flat_column
from test_gpu_query import Tapes, gather, query
from test_gpu_rows import rooted as rooted_pointers

pytestmark = pytest.mark.gpu

CAP = 128 << 20
E_BADARG, E_OVERFLOW = -4, -5
GUARD = 65  # odd: with it the status, tag and code rows begin at odd addresses
P64, P32, P8 = 0x5A5A5A5A5A5A5A5A, 0x5A5A5A5A, 0x5A
TWITTER = os.path.join(_paths.REPO_ROOT, "tests", "golden", "jsonexamples", "twitter.json")


@pytest.fixture(scope="module")
def parser():
    build.build_sjgpu()
    p = capi.DomParserImplementation(CAP)
    yield p
    p.close()


def device_roots(T, roots):
    torch = T.torch
    root_tags, root_values = np.ascontiguousarray(roots[0], np.uint8), np.ascontiguousarray(roots[1], np.uint64)
    d_tags = torch.from_numpy(np.concatenate([np.zeros(1, np.uint8), root_tags])).cuda()  # the row begins at an odd address
    d_values = torch.from_numpy(np.concatenate([root_values, np.zeros(1, np.uint64)]).view(np.int64)).cuda()  # (never empty: an address to pass)
    return root_tags, root_values, d_tags, d_values


def call(p, T, roots, cap, docs=None, table_ptr=None, tape_ptr=None, offsets_skew=0, value_skew=0, key_skew=0, root_skew=0, expect=None):
    """one sjgpu_object_fields_from_cells_device over the roots (tags[rows], values[rows]) with outputs of exactly rows + 1 words, rows bytes and `cap` slots between
    poisoned guards -> (rc, fields, (status[rows], offsets[rows + 1], key_tags, key_values, tags, values)[fields]); expect: the rc the caller counts on"""
    torch = T.torch
    root_tags, root_values, d_tags, d_values = device_roots(T, roots)
    rows = len(root_tags)
    offsets = torch.full((rows + 1 + 2 * GUARD,), P32, dtype=torch.int32, device="cuda")
    status = torch.full((rows + 2 * GUARD,), P8, dtype=torch.uint8, device="cuda")
    words = [torch.full((cap + 2 * GUARD,), P64, dtype=torch.int64, device="cuda") for _ in range(2)]
    tags = [torch.full((cap + 2 * GUARD,), P8, dtype=torch.uint8, device="cuda") for _ in range(2)]
    rc, fields = p.object_fields_from_cells_device(tape_ptr or T.d_tape.data_ptr(), len(T.tape), T.d_sbuf.data_ptr(), len(T.sbuf), table_ptr or T.d_table.data_ptr(),
                                                   T.docs if docs is None else docs, d_values.data_ptr() + root_skew, d_tags.data_ptr() + 1, rows,
                                                   offsets.data_ptr() + 4 * GUARD + offsets_skew, status.data_ptr() + GUARD, words[0].data_ptr() + 8 * GUARD + key_skew,
                                                   tags[0].data_ptr() + GUARD, words[1].data_ptr() + 8 * GUARD + value_skew, tags[1].data_ptr() + GUARD, cap, T.stream)
    torch.cuda.synchronize()
    if expect is not None:
        assert rc == expect, (rc, expect, p.last_error())
    nothing = rc == E_BADARG
    wrote_offsets = 0 if nothing else rows + 1
    wrote_status = 0 if nothing else rows
    wrote = fields if rc == 0 else 0
    oh, sh = offsets.cpu().numpy().view(np.uint32), status.cpu().numpy()
    assert (oh[:GUARD] == P32).all() and (oh[GUARD + wrote_offsets:] == P32).all(), "offsets poison"
    assert (sh[:GUARD] == P8).all() and (sh[GUARD + wrote_status:] == P8).all(), "status poison"
    cols = []
    for t, w, name in zip(tags, words, ("key", "value")):
        th, wh = t.cpu().numpy(), w.cpu().numpy().view(np.uint64)
        assert (th[:GUARD] == P8).all() and (th[GUARD + wrote:] == P8).all(), name + " tag poison"
        assert (wh[:GUARD] == P64).all() and (wh[GUARD + wrote:] == P64).all(), name + " word poison"
        assert not (th[GUARD: GUARD + wrote] == P8).any(), name + " tags: a slot was not written"
        cols += [th[GUARD: GUARD + wrote].copy(), wh[GUARD: GUARD + wrote].copy()]
    assert np.array_equal(d_tags.cpu().numpy()[1:], root_tags) and np.array_equal(d_values.cpu().numpy().view(np.uint64)[:rows], root_values), "the roots were written"
    return rc, fields, (sh[GUARD: GUARD + wrote_status].copy(), oh[GUARD: GUARD + wrote_offsets].copy(), *cols)


def column(p, T, roots, docs=None):
    """the map column at its EXACT capacity: a call with room for nothing says what is needed and leaves offsets and status complete, the second fills
    -> (status, offsets, key_tags, key_values, tags, values)"""
    rc, fields, first = call(p, T, roots, 0, docs)
    if fields == 0:
        assert rc == 0
        return first
    assert rc == E_OVERFLOW and int(first[1][-1]) == fields and first[2].size == 0
    rc, again, cols = call(p, T, roots, fields, docs, expect=0)
    assert again == fields and np.array_equal(cols[0], first[0]) and np.array_equal(cols[1], first[1])
    return cols


def sizes(p, T, roots, docs=None, size_skew=0, raw=False):
    """one sjgpu_cell_sizes_device: rows words and rows bytes between poisoned guards -> (size[rows], code[rows])"""
    torch = T.torch
    root_tags, root_values, d_tags, d_values = device_roots(T, roots)
    rows = len(root_tags)
    size = torch.full((rows + 2 * GUARD,), P32, dtype=torch.int32, device="cuda")
    code = torch.full((rows + 2 * GUARD,), P8, dtype=torch.uint8, device="cuda")
    rc = p.cell_sizes_device(T.d_tape.data_ptr(), len(T.tape), T.d_table.data_ptr(), T.docs if docs is None else docs, d_values.data_ptr(), d_tags.data_ptr() + 1, rows,
                             size.data_ptr() + 4 * GUARD + size_skew, code.data_ptr() + GUARD, T.stream)
    torch.cuda.synchronize()
    wrote = rows if rc == 0 else 0
    sh, ch = size.cpu().numpy().view(np.uint32), code.cpu().numpy()
    assert (sh[:GUARD] == P32).all() and (sh[GUARD + wrote:] == P32).all(), "size poison"
    assert (ch[:GUARD] == P8).all() and (ch[GUARD + wrote:] == P8).all(), "code poison"
    if raw:
        return rc
    assert rc == 0, (rc, p.last_error())
    return sh[GUARD: GUARD + rows].copy(), ch[GUARD: GUARD + rows].copy()


def model(T, roots, docs=None):
    """tests/fields_model.py over the roots -> (columns, sizes)"""
    S = fields_model.Stream(T.tape, T.sbuf, T.table if docs is None else T.table[: docs + 1])
    return fields_model.column(S, roots), fields_model.sizes(S, roots)


def check(p, T, roots, docs=None):
    """both calls over one row of roots against the model -> the columns"""
    got = column(p, T, roots, docs)
    want, want_sizes = model(T, roots, docs)
    fields_model.assert_columns(got, want)
    got_sizes = sizes(p, T, roots, docs)
    assert np.array_equal(got_sizes[0], want_sizes[0]) and np.array_equal(got_sizes[1], want_sizes[1])
    return got


def matches(p, T, path):
    """the matches of one path over all documents: a row of root cells made by sjgpu_at_paths_device"""
    status, offsets, tags, values = flat_column(p, T, [path])
    return tags, values


def keys_of(T, key_values):
    return [pointer_model.string_of(T.sbuf, int(v)) for v in key_values]


# ---- 1. the fixture -----------------------------------------------------------------------------------------------------------------------------
def test_fixture_rows_from_the_paths_from_the_pointers_and_from_the_call_itself(parser):
    docs, row_paths, tables, _ = fixture()
    T = Tapes.of_stream(parser, docs)
    rows = [matches(parser, T, rp) for rp in row_paths]
    assert [len(r[0]) for r in rows] == [sum(len(tables[i][j]) for i in range(len(docs)) if not isinstance(tables[i][j], str)) for j in range(len(row_paths))]
    roots = (np.concatenate([t for t, _ in rows]), np.concatenate([v for _, v in rows]))
    assert set(b'{["ludtfn') <= set(roots[0].tolist())
    status, offsets, key_tags, key_values, tags, values = check(parser, T, roots)
    counts = np.diff(offsets.astype(np.int64))
    assert set(status.tolist()) == {0, 17} and (key_tags == ord('"')).all() and counts.max() == 300
    # the 300-field object, and the mixed row: an array of objects of every shape, an array, every scalar
    lo = int(offsets[int(np.argmax(counts == 300))])
    assert keys_of(T, key_values[lo: lo + 300]) == [b"k%03d" % i for i in range(300)] and set(tags[lo: lo + 300].tolist()) == set(b'l"[{nd')
    mixed = next(i for i, d in enumerate(docs) if d.startswith(b'[{},{"one":1}'))
    first = sum(len(tables[i][0]) for i in range(mixed) if not isinstance(tables[i][0], str))
    n = len(tables[mixed][0])
    assert status[first: first + n].tolist() == [0] * 5 + [17] * (n - 5) and counts[first: first + 5].tolist() == [0, 1, 4, 9, 3]
    lo = int(offsets[first + 2])
    assert keys_of(T, key_values[lo: lo + 13]) == [b"d", b"d", b"e", b"d", b"", b"\x00", b"a\x00b", b"line\nfeed", b'q"uote', b"sl/ash", "\U0001F600".encode(),
                                                   "é€\U0001F600".encode(), b"tab\tback\\slash"]
    # a row of sjgpu_at_pointers_device's cells (hits and failures), and the call's own value row: a second nesting level
    cells = query(parser, T, [b"", b"/a", b"/0", b"/statuses", b"/k", b"/missing", b"/a/0", b"x"])
    roots = (cells[0].reshape(-1), cells[1].reshape(-1))
    assert {17, 19, 20, 22, ord("{"), ord("["), ord("l"), ord('"')} <= set(roots[0].tolist())
    assert {0, 17, 19, 20, 22} <= set(check(parser, T, roots)[0].tolist())
    second = check(parser, T, (tags, values))
    assert len(second[4]) > 100 and (check(parser, T, (key_tags, key_values))[0] == 17).all()
    # the key row through the gather
    want = keys_of(T, key_values)
    rc, total, goffsets, chars = gather(parser, T, key_tags, key_values, want_total=sum(len(k) for k in want))
    assert rc == 0 and [chars[int(goffsets[i]): int(goffsets[i + 1])] for i in range(len(want))] == want


# ---- 2. twitter.json -------------------------------------------------------------------------------------------------------------------------------
class Pairs(list):
    """an object as the list of its (key, value) pairs, duplicate keys and order kept"""


def assert_value(T, tag, value, want, what):
    tag, value = int(tag), int(value)
    if isinstance(want, Pairs):
        assert tag == ord("{"), what
    elif isinstance(want, list):
        assert tag == ord("["), what
    elif isinstance(want, str):
        assert tag == ord('"') and pointer_model.string_of(T.sbuf, value) == want.encode(), what
    elif want is True or want is False or want is None:
        assert (tag, value) == {True: (ord("t"), 1), False: (ord("f"), 0), None: (ord("n"), 0)}[want], what
    elif isinstance(want, int):
        assert (tag, value) == (ord("l"), want & ((1 << 64) - 1)), what
    else:
        assert (tag, value) == (ord("d"), struct.unpack("<Q", struct.pack("<d", want))[0]), what


def test_twitter_users_through_fields_many(parser):
    data = open(TWITTER, "rb").read()
    statuses = [dict(s) for s in json.loads(data, object_pairs_hook=Pairs)[0][1]]
    users = [s["user"] for s in statuses]
    code, docs, row_offsets, status, offsets, key_offsets, key_chars, tags, values = parser.fields_many(data, b"$.statuses[*].user")
    assert (code, docs, row_offsets.tolist()) == (0, 1, [0, 100]) and (status == 0).all()
    assert np.diff(offsets.astype(np.int64)).tolist() == [len(u) for u in users] and int(offsets[-1]) == len(tags) == len(values) == len(key_offsets) - 1
    keys = [key_chars[int(key_offsets[i]): int(key_offsets[i + 1])].tobytes() for i in range(len(tags))]
    assert keys == [k.encode() for u in users for k, _ in u]
    # the same column from the entry points themselves; the values against Python's json through the tapes
    T = Tapes.of_stream(parser, [data])
    roots = matches(parser, T, b"$.statuses[*].user")
    got = check(parser, T, roots)
    fields_model.assert_columns((status, offsets, got[2], got[3], tags, values), got)
    assert keys_of(T, got[3]) == keys
    flat = [(k, v) for u in users for k, v in u]
    for i, (k, v) in enumerate(flat):
        assert_value(T, tags[i], values[i], v, (i, k))
    # roots from sjgpu_at_pointers_from_cells_device: a retweeted status or NO_SUCH_FIELD
    level1 = matches(parser, T, b"$.statuses[*]")
    cells = rooted_pointers(parser, T, level1, [b"/retweeted_status"])
    retweets = check(parser, T, (cells[0][0], cells[1][0]))
    assert (retweets[0] == 0).sum() == 73 and (retweets[0] == 20).sum() == 27
    assert np.diff(retweets[1].astype(np.int64))[retweets[0] == 0].tolist() == [len(s["retweeted_status"]) for s in statuses if "retweeted_status" in s]
    # a first guess that is too small, no rows, no input
    for first_cap in (0, len(tags) - 1):
        again = parser.fields_many(data, b"$.statuses[*].user", first_cap=first_cap)
        assert all(np.array_equal(a, b) for a, b in zip(again[2:], (row_offsets, status, offsets, key_offsets, key_chars, tags, values)))
    wide = parser.fields_many(data, b"$.statuses[*].user", wide=True)
    assert all(np.array_equal(a, b) for a, b in zip(wide[2:], (row_offsets, status, offsets, key_offsets, key_chars, tags, values)))
    code, docs, row_offsets, s0, o0, k0, c0, t0, v0 = parser.fields_many(data, b"$.nothing[*]")
    assert (code, docs, row_offsets.tolist(), s0.size, o0.tolist(), k0.tolist(), c0.size, t0.size, v0.size) == (0, 1, [0, 0], 0, [0], [0], 0, 0, 0)
    assert parser.fields_many(b"", b"$[*]")[:2] == (13, 0)


# ---- 3. wave and workgroup edges, the scan's second level -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(parser):
    rng = np.random.default_rng(111)
    docs = stream_cases.small_records(rng, 4097)
    T = Tapes.of_stream(parser, docs)
    whole = query(parser, T, [b""])
    return T, (whole[0][0], whole[1][0])


@pytest.mark.parametrize("rows", [0, 1, 63, 64, 65, 255, 256, 257, 4097])
def test_rows_at_the_wave_and_workgroup_edges(parser, small, rows):
    T, roots = small
    got = check(parser, T, (roots[0][:rows], roots[1][:rows]))
    assert got[1][0] == 0 and len(got[1]) == rows + 1 and (rows < 63 or len(got[4]) > rows)


def test_all_values_of_the_small_records_in_any_order(parser, small):
    T, _ = small
    roots = matches(parser, T, b"$.*")  # every field of the objects, every element of the arrays: all kinds of cells
    assert len(roots[0]) > 8000 and set(b'{["ldtn') <= set(roots[0].tolist())
    order = np.random.default_rng(112).permutation(len(roots[0]))
    got = check(parser, T, (roots[0][order], roots[1][order]))
    assert set(got[0].tolist()) == {0, 17} and len(got[4]) > 1000


# ---- 4. roots that are no elements, a table without documents ----------------------------------------------------------------------------------------
def test_scalar_failed_and_bad_roots_in_one_row(parser):
    from test_fields_emu import bad_cells
    docs = [b'[8863084066665136133,"x",{"k":1}]', b'{"a":{"b":[1,2,{"c":"d"}],"e":null},"n":12}', b'[[1],[2,3]]', b"7"]
    T = Tapes.of_stream(parser, docs)
    assert int(T.tape[3]) == (ord("{") << 56) | 5  # a number's value word that reads like an opening word
    a_tag, a_value = (int(x[0, 1]) for x in query(parser, T, [b"/a"]))
    assert chr(a_tag) == "{"
    cells = bad_cells(T, a_tag, a_value)
    roots = (np.array([t for t, _ in cells], np.uint8), np.array([v for _, v in cells], np.uint64))
    status, offsets, key_tags, key_values, tags, values = check(parser, T, roots)
    counts = np.diff(offsets.astype(np.int64))
    assert counts[0] == 2 and status[0] == 0 and (counts[1:] == 0).all() and [chr(t) for t in tags] == ["[", "n"] and keys_of(T, key_values) == [b"b", b"e"]
    bad = list(range(1, 13)) + [15, 16] + list(range(17, 30))
    assert (status[bad] == 20).all() and status[14] == 0  # (14: the value word agrees with the cell made for it: an object without fields)
    assert status[30:34].tolist() == [17, 19, 20, 22] and (status[list(range(34, 42)) + [13]] == 17).all()
    status, offsets, key_tags, key_values, tags, values = check(parser, T, roots, docs=0)
    containers = [j for j, (t, _) in enumerate(cells) if t in (ord("{"), ord("["))]
    assert (status[containers] == 20).all() and int(offsets[-1]) == 0 and status[30:34].tolist() == [17, 19, 20, 22]


# ---- 5. capacities ----------------------------------------------------------------------------------------------------------------------------------
def test_capacities(parser, small):
    T, roots = small
    part = (roots[0][:1000], roots[1][:1000])
    cols = column(parser, T, part)  # (capacity 0, then exact: inside)
    n = len(cols[4])
    assert n > 1000
    rc, fields, short = call(parser, T, part, n - 1, expect=E_OVERFLOW)  # one short: nothing written (the poison check inside), the rest complete
    assert fields == n and np.array_equal(short[0], cols[0]) and np.array_equal(short[1], cols[1]) and short[4].size == 0
    rc, fields, spare = call(parser, T, part, n + 3, expect=0)  # room to spare: only the fields are written
    fields_model.assert_columns(spare, cols)
    # field_cap == 0 with null outputs: what is needed is reported, and rows without a field need none
    import torch
    out_offsets = torch.zeros(1001, dtype=torch.int32, device="cuda")
    out_status = torch.zeros(1000, dtype=torch.uint8, device="cuda")

    def null_outputs(roots):
        _, _, d_tags, d_values = device_roots(T, roots)
        return parser.object_fields_from_cells_device(T.d_tape.data_ptr(), len(T.tape), T.d_sbuf.data_ptr(), len(T.sbuf), T.d_table.data_ptr(), T.docs, d_values.data_ptr(),
                                                      d_tags.data_ptr() + 1, len(roots[0]), out_offsets.data_ptr(), out_status.data_ptr(), 0, 0, 0, 0, 0, T.stream)
    assert null_outputs(part) == (E_OVERFLOW, n) and np.array_equal(out_offsets.cpu().numpy().view(np.uint32), cols[1])
    arrays = part[0] == ord("[")
    assert arrays.sum() > 50
    assert null_outputs((part[0][arrays], part[1][arrays])) == (0, 0) and set(out_status.cpu().numpy()[: int(arrays.sum())].tolist()) == {17}


# ---- 6. size() at the saturation of the count field ----------------------------------------------------------------------------------------------------
def test_size_of_an_array_beyond_the_count_field():
    """[1,1,...] of 0x1000000 elements, a document of 32 MiB whose tape is 256 MiB, with a parser of its own: the count field saturates where the reference's does
    (the fixture's number for this case; its two others, 0xFFFFFE and 0xFFFFFF elements, are not run here), and the fields call answers an array root without a walk"""
    import torch
    _, _, _, array_sizes = fixture()
    n = 0x1000000
    assert array_sizes[n] == 0xFFFFFF
    data = np.concatenate([np.frombuffer(b"[1", np.uint8), np.tile(np.frombuffer(b",1", np.uint8), n - 1), np.frombuffer(b"]", np.uint8)])
    build.build_sjgpu()
    p = capi.DomParserImplementation(len(data) + 64)
    try:
        S = capi.ResidentStream(p, data, doc_cap=1)
        assert (S.code, S.docs, S.tw) == (0, 1, 2 * n + 4)
        values = torch.empty(1, dtype=torch.int64, device=S.dev)
        tags = torch.empty(1, dtype=torch.uint8, device=S.dev)
        assert p.at_pointers_device(*S.args(), [b""], values.data_ptr(), tags.data_ptr(), S.stream) == 0
        size = torch.full((1 + 2,), P32, dtype=torch.int32, device=S.dev)
        code = torch.full((1 + 2,), P8, dtype=torch.uint8, device=S.dev)
        assert p.cell_sizes_device(S.tape.data_ptr(), S.tw, S.table.data_ptr(), S.docs, values.data_ptr(), tags.data_ptr(), 1, size.data_ptr() + 4, code.data_ptr() + 1, S.stream) == 0
        offsets = torch.empty(2, dtype=torch.int32, device=S.dev)
        status = torch.empty(1, dtype=torch.uint8, device=S.dev)
        assert p.object_fields_from_cells_device(*S.args(), values.data_ptr(), tags.data_ptr(), 1, offsets.data_ptr(), status.data_ptr(), 0, 0, 0, 0, 0, S.stream) == (0, 0)
        S.synchronize()
        assert tags.cpu().tolist() == [ord("[")]
        assert size.cpu().numpy().view(np.uint32).tolist() == [P32, array_sizes[n], P32] and code.cpu().tolist() == [P8, 0, P8]
        assert status.cpu().tolist() == [17] and offsets.cpu().tolist() == [0, 0]
    finally:
        p.close()


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(parser):
    import torch
    rng = np.random.default_rng(114)
    T = Tapes.of_stream(parser, stream_cases.small_records(rng, 300))
    whole = query(parser, T, [b""])
    roots = (whole[0][0], whole[1][0])
    base = column(parser, T, roots)

    def refused(**kw):
        return call(parser, T, roots, len(base[4]), **kw)[0] == E_BADARG  # (nothing written: the poison check inside)
    assert refused(tape_ptr=T.d_tape.data_ptr() + 4) and refused(table_ptr=T.d_table.data_ptr() + 8) and refused(value_skew=4) and refused(key_skew=4)
    assert refused(offsets_skew=2) and refused(root_skew=4) and not refused()
    assert sizes(parser, T, roots, size_skew=2, raw=True) == E_BADARG
    for field in ("tape_begin", "string_begin"):
        table = T.table.copy()
        table[field][[100, 101]] = table[field][[101, 100]]
        assert table[field][100] > table[field][101]
        back = torch.from_numpy(table.view(np.int32)).cuda()
        assert refused(table_ptr=back.data_ptr())
    table = T.table.copy()
    table["tape_begin"][-1] += 1  # ends behind the tape
    assert refused(table_ptr=torch.from_numpy(table.view(np.int32)).cuda().data_ptr())
    # null pointers, one at a time, and rows + 1 beyond what the scan indexes: refused before anything is read
    ok = torch.zeros(256, dtype=torch.int64, device="cuda")
    total = ctypes.c_uint64(7)
    good = [parser.h, T.d_tape.data_ptr(), len(T.tape), T.d_sbuf.data_ptr(), len(T.sbuf), T.d_table.data_ptr(), T.docs, ok.data_ptr(), ok.data_ptr() + 64, 1,
            ok.data_ptr() + 128, ok.data_ptr() + 192, ok.data_ptr() + 256, ok.data_ptr() + 320, ok.data_ptr() + 384, ok.data_ptr() + 448, 8, T.stream, ctypes.byref(total)]
    f = parser.L.sjgpu_object_fields_from_cells_device
    for at in (0, 1, 3, 5, 7, 8, 10, 11, 12, 13, 14, 15, 18):
        args = list(good)
        args[at] = None
        assert f(*args) == E_BADARG, at
    many = list(good)
    many[9] = 0xFFFFFFF0
    assert f(*many) == E_BADARG and total.value == 0
    assert f(*good) == 0 and total.value == 0  # (the root cell is a zero: no tag, status 20)
    torch.cuda.synchronize()
    assert int(ok[16].item()) & 0xFFFFFFFF == 0 and int(ok[24].item()) & 0xFF == 20
    g = parser.L.sjgpu_cell_sizes_device
    good = [parser.h, T.d_tape.data_ptr(), len(T.tape), T.d_table.data_ptr(), T.docs, ok.data_ptr(), ok.data_ptr() + 64, 1, ok.data_ptr() + 128, ok.data_ptr() + 192, T.stream]
    for at in (0, 1, 3, 5, 6, 8, 9):
        args = list(good)
        args[at] = None
        assert g(*args) == E_BADARG, at
    many = list(good)
    many[7] = 0xFFFFFFF0
    assert g(*many) == E_BADARG and g(*good) == 0
    torch.cuda.synchronize()
    assert int(ok[16].item()) & 0xFFFFFFFF == 0 and int(ok[24].item()) & 0xFF == 20
    # the neighbours of a call that was refused are what they were
    fields_model.assert_columns(column(parser, T, roots), base)
