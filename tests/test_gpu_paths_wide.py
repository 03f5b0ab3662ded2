"""GPU tier (-m gpu): sjgpu_at_paths_wide_device (the k_wide_* kernels in sjgpu_query.hip, include/sjgpu_paths.h) -- the column of sjgpu_at_paths_device with the
levels expanded breadth first -- against tests/golden/paths.json, tests/path_model.py and, bit for bit, the narrow call.  The tapes are the device's own
(sjgpu_stage2_many_device / sjgpu_stage2_device).  Every call goes through tests/test_gpu_paths.py's call(): outputs of exactly the contracted size inside
poisoned tensors whose poison is checked after every call, after SJGPU_E_OVERFLOW too, when the rows must be untouched."""
import numpy as np
import pytest

import path_cases
import stream_cases
import test_gpu_paths as narrow
from simdjson_amd import build, capi
from test_gpu_paths import E_BADARG, E_OVERFLOW, as_column, call, column, model_cells
from test_gpu_query import Tapes
from test_gpu_stream_tape import Resident
from test_paths_wide_emu import LOOKALIKE_PATHS, LOOKALIKES, RUN_PAIRS, lookalike_number

pytestmark = pytest.mark.gpu


class Wide:
    """a parser whose at_paths_device is the wide call: call() and column() of tests/test_gpu_paths.py then check the wide call's outputs and poison"""

    def __init__(self, p):
        self._p = p

    def __getattr__(self, name):
        return getattr(self._p, name)

    def at_paths_device(self, *args, **kw):
        return self._p.at_paths_wide_device(*args, **kw)


@pytest.fixture(scope="module")
def parser():
    build.build_sjgpu()
    p = capi.DomParserImplementation(narrow.CAP)
    yield p
    p.close()


@pytest.fixture(scope="module")
def wide(parser):
    return Wide(parser)


def same(got, want, what=""):
    """all four outputs bit for bit"""
    for name, a, b in zip(("status", "offsets", "tags", "values"), got, want):
        assert a.shape == b.shape and np.array_equal(a, b), what + name


# ---- 1. the fixture -----------------------------------------------------------------------------------------------------------------------------
def test_fixture_as_one_stream_and_document_by_document(parser, wide):
    import torch
    docs, paths, cells = path_cases.fixture()
    T = Tapes.of_stream(parser, docs)
    for first in range(0, len(paths), 64):
        part = paths[first: first + 64]
        status, offsets, tags, values = column(wide, T, part)
        for i in range(len(docs)):
            for j in range(len(part)):
                got = path_cases.render(*path_cases.cell(status, offsets, tags, values, j, i, len(docs)), T.sbuf)
                assert got == cells[i][first + j], (docs[i][:80], part[j][:40], got)
        path_cases.check_container_matches(tags, values, T.tape)
    # every document alone through sjgpu_stage2_device, served by the table of two entries
    for i, d in enumerate(docs):
        res = Resident(parser, d)
        tape = torch.zeros(len(d) + 8, dtype=torch.int64, device="cuda")
        sbuf = torch.zeros(5 * (len(d) // 3) + 256, dtype=torch.uint8, device="cuda")
        rc, tw, sb = parser.stage2_device(res.buf.data_ptr(), res.length, res.idx.data_ptr(), res.n, tape.data_ptr(), len(d) + 8, sbuf.data_ptr(), sbuf.numel(), stream=res.stream)
        assert rc == 0
        table = np.zeros(2, capi.DOC_SPAN)
        table[1] = (res.n, len(d), tw, sb)
        one = Tapes(tape.cpu().numpy().view(np.uint64)[:tw], sbuf.cpu().numpy()[:sb], table)
        for first in range(0, len(paths), 64):
            part = paths[first: first + 64]
            status, offsets, tags, values = column(wide, one, part)
            for j in range(len(part)):
                assert path_cases.render(*path_cases.cell(status, offsets, tags, values, j, 0, 1), one.sbuf) == cells[i][first + j], (d[:80], part[j][:40])


# ---- 2. bit for bit the narrow call ------------------------------------------------------------------------------------------------------------------
def test_two_thousand_random_documents(parser, wide):
    rng = np.random.default_rng(61)
    docs = stream_cases.valid_documents(rng, 2000)
    T = Tapes.of_stream(parser, docs)
    paths = path_cases.wildcard_paths(docs, 14)
    assert len(paths) == 16
    got = column(wide, T, paths)
    same(got, column(parser, T, paths))
    assert len(got[2]) > 2000 and (got[0] != 0).any()


@pytest.fixture(scope="module")
def small(parser):
    docs = stream_cases.small_records(np.random.default_rng(71), 5000)
    return docs, Tapes.of_stream(parser, docs)


@pytest.mark.parametrize("docs", [1, 63, 64, 65, 257, 4097])
def test_prefixes_of_small_records(parser, wide, small, docs):
    """the edges of the workgroup and of the scans' block, with one path and with three; the tape goes on behind the last document of the prefix"""
    _, T = small
    for paths in (narrow.DENSE_ZERO_DENSE[:1], narrow.DENSE_ZERO_DENSE):
        got = column(wide, T, paths, docs)
        same(got, column(parser, T, paths, docs), "K = %d: " % len(paths))
        assert len(got[2]) > 0


# ---- 3. one large document ---------------------------------------------------------------------------------------------------------------------------
STATUS_PATHS = [b"$.statuses[*].user.id", b"$.statuses[*].tags[*]", b"$.statuses[*].*", b"$.statuses[*]"]


@pytest.fixture(scope="module")
def statuses():
    n = 9000
    doc = b'{"statuses":[' + b",".join(b'{"id":%d,"user":{"id":%d,"name":"u%d"},"tags":["a%d","b",%d.5]}' % (i, 7 * i, i, i, i) for i in range(n)) + b"]}"
    return n, doc


@pytest.mark.parametrize("among", [False, True], ids=["alone", "between short documents"])
def test_one_large_document(parser, wide, statuses, among):
    """about 1.4e5 tape words in one document: many blocks of the scans, many workgroups of every kernel"""
    n, doc = statuses
    docs = [doc]
    if among:
        short = stream_cases.small_records(np.random.default_rng(75), 40)
        docs = short[:20] + [b'{"statuses":[{"user":{"id":1},"tags":[]},7,{"tags":[[1]],"user":{}}]}', doc, b'{"statuses":{"a":{"user":{"id":"x"}}}}'] + short[20:]
    T = Tapes.of_stream(parser, docs)
    at = docs.index(doc)
    assert int(T.table["tape_begin"][at + 1]) - int(T.table["tape_begin"][at]) > 130000
    got = column(wide, T, STATUS_PATHS)
    path_cases.assert_column(got, as_column(model_cells(T, STATUS_PATHS)))
    same(got, column(parser, T, STATUS_PATHS))
    counts = np.diff(got[1].astype(np.int64)).reshape(4, len(docs))
    assert counts[:, at].tolist() == [n, 3 * n, 3 * n, n]
    path_cases.check_container_matches(got[2], got[3], T.tape)


# ---- 4. numbers whose second word looks like a tag; keys and values ----------------------------------------------------------------------------------
@pytest.mark.parametrize("as_double", [False, True], ids=["integers", "doubles"])
@pytest.mark.parametrize("where", ["root", "a", "b.k"])
def test_numbers_that_look_like_tags(parser, wide, where, as_double):
    """tests/test_paths_wide_emu.py's runs, on the device's own tapes: every tag byte on top of the value words of runs that sit on both sides of every edge of
    the annotation, with nothing and with one plain element in front"""
    docs, lengths, patterns = [], [], []
    for byte in LOOKALIKES:
        for pairs in RUN_PAIRS:
            for front in (0, 1):
                texts, bits = zip(*[lookalike_number(byte, as_double, i % 7) for i in range(pairs)])
                array = b"[" + b",".join((b"null",) * front + texts) + b"]"
                docs.append({"root": array, "a": b'{"a":' + array + b"}", "b.k": b'{"a":1,"b":{"j":[2],"k":' + array + b'},"c":[3]}'}[where])
                lengths.append(pairs + front)
                patterns.append((front, bits))
    T = Tapes.of_stream(parser, docs)
    # the device's tapes do carry the bytes: behind the array's opening word (and the plain element) come (tag, bits) pairs
    skip = {"root": 2, "a": 4, "b.k": 14}[where]
    for d, (front, bits) in enumerate(patterns):
        first = int(T.table["tape_begin"][d]) + skip + front
        run = T.tape[first: first + 2 * len(bits)]
        assert ((run[0::2] >> np.uint64(56)) == ord("d" if as_double else "l")).all() and np.array_equal(run[1::2], np.array(bits, np.uint64)), docs[d][:100]
        assert ((run[1::2] >> np.uint64(56)) == (bits[0] >> 56)).all() and chr(bits[0] >> 56).encode() in LOOKALIKES
    got = column(wide, T, LOOKALIKE_PATHS)
    same(got, column(parser, T, LOOKALIKE_PATHS))
    path_cases.assert_column(got, as_column(model_cells(T, LOOKALIKE_PATHS)))
    counts = np.diff(got[1].astype(np.int64)).reshape(len(LOOKALIKE_PATHS), len(docs))
    assert counts[{"root": 0, "a": 1, "b.k": 2}[where]].tolist() == lengths and (got[0] == 0).all()


def test_an_objects_children_are_keys_and_values_in_turn(parser, wide):
    n = 5000
    flat = b"{" + b",".join(b'"k%d":"v%d"' % (i, i) for i in range(n)) + b"}"
    docs = [flat, b'{"o":' + flat + b',"p":{"k":"v"}}', b'{"a":{},"b":[],"c":{"d":{}},"e":[[]],"f":"s","g":{"h":1,"i":[]}}', b'[[],[1],[],[2,3],{},[[]],[],{"a":[]}]', b"[]", b"{}",
            b"[[],[]]", b"[[1,2,3]]", b"[" * 8 + b"[1,2],[3]" + b"]" * 8, b"[[[[[[[[[[7]]]]]]]]]]"]
    T = Tapes.of_stream(parser, docs)
    paths = [b"$.*", b"$.*.*", b"$[*][*]", b"$[*]"]
    got = column(wide, T, paths)
    path_cases.assert_column(got, as_column(model_cells(T, paths)))
    same(got, column(parser, T, paths))
    counts = np.diff(got[1].astype(np.int64)).reshape(4, len(docs))
    assert counts[:, :2].tolist() == [[n, 2], [0, n + 1], [0, n + 1], [n, 2]] and counts[:, 2:8].tolist() == [[6, 8, 0, 0, 2, 1], [4, 5, 0, 0, 0, 3], [4, 5, 0, 0, 0, 3], [6, 8, 0, 0, 2, 1]]
    # eight wildcard levels deep: the paths at the limit
    deep = [b"$" + b"[*]" * 8, b"$" + b"[*]" * 8 + b"[0]", b"$" + b"[*]" * 7 + b"[0][*]", b"$" + b"[*]" * 8 + b"[0][0]"]
    got = column(wide, T, deep)
    same(got, column(parser, T, deep))
    assert np.diff(got[1].astype(np.int64)).reshape(4, len(docs))[:, 8:].ravel().tolist() == [2, 1, 2, 1, 0, 0, 0, 1]


# ---- 5. capacity, nothing at all, refusals -----------------------------------------------------------------------------------------------------------
def test_capacity_and_a_total_of_zero(parser, wide, small):
    _, T = small
    paths = narrow.DENSE_ZERO_DENSE
    want = column(parser, T, paths, 1000)
    total = len(want[2])
    assert total > 2000
    same(call(wide, T, paths, total, 1000, expect=0)[2:], want)
    for cap in (total - 1, 0):
        rc, matches, status, offsets, tags, values = call(wide, T, paths, cap, 1000, expect=E_OVERFLOW)  # (values and tags still poison: checked inside)
        assert matches == total and tags.size == 0
        same((status, offsets), want[:2])
    same(call(wide, T, paths, total + 100, 1000, expect=0)[2:], want)  # room to spare stays poison
    # nothing matches anywhere: offsets all zero, nothing written to the (empty) rows
    status, offsets, tags, values = column(wide, T, [b"$.missing[*]", b"$.nope.*"], 1200)
    assert not offsets.any() and offsets.shape == (2401,) and not status.any() and tags.size == values.size == 0
    scalars = Tapes.of_stream(parser, [b"1", b'"s"', b"null", b"[]", b"{}"] * 60)
    status, offsets, tags, values = column(wide, scalars, [b"$[*]", b"$.*", b""])
    assert not offsets.any() and status[:2].sum() == 0 and tags.size == 0
    assert status[2].tolist() == [0, 0, 0, 22, 22] * 60  # the empty path: nothing for a scalar root, INVALID_JSON_POINTER for a container
    # K == 0 and docs == 0: success, offsets[0] = 0 and nothing else
    rc, matches, _, offsets, _, _ = call(wide, T, [], 0, expect=0)
    assert matches == 0 and offsets.tolist() == [0]
    rc, matches, _, offsets, _, _ = call(wide, T, paths, 0, docs=0, expect=0)
    assert matches == 0 and offsets.tolist() == [0]


def test_refusals(parser, wide):
    """every refusal tests/test_gpu_paths.py::test_contract lists for the narrow call"""
    import torch
    docs = stream_cases.small_records(np.random.default_rng(73), 300)
    T = Tapes.of_stream(parser, docs)
    paths = [b"$[*]", b"$.name", b"$.*"]
    base = column(wide, T, paths)
    same(base, column(parser, T, paths))
    total = len(base[2])

    def refused(paths=paths, **kw):
        return call(wide, T, paths, total, **kw)[0] == E_BADARG  # (nothing written: the poison check inside)
    assert refused([b"$[*]"] * 65) and call(wide, T, [b"$.nope[*]"] * 64, 0, expect=0)[1] == 0
    assert refused([b"$." + b"a" * 1023]) and call(wide, T, [b"$." + b"a" * 1022], 0, expect=0)[1] == 0
    assert refused([b"$" + b"[*]" * 9]) and call(wide, T, [b"$" + b"[*]" * 8], 0, expect=0)[1] == 0
    assert refused([b"$" + b"[*]" * 8 + b".a.b"]) is False and refused([b"$" + b"[*]" * 9 + b".a"])
    assert refused([b"$" + b".a" * 32 + b"[*]"]) and call(wide, T, [b"$" + b".a" * 31 + b"[*]"], 0, expect=0)[1] == 0  # 33 levels, 32 levels
    assert refused([b"$" + b".a" * 33]) and call(wide, T, [b"$" + b".a" * 32], 0, expect=0)[1] == 0                      # 33 pointer tokens in one level, 32
    assert refused(offsets_skew=2) and refused(value_skew=4)
    assert refused(tape_ptr=T.d_tape.data_ptr() + 4) and refused(table_ptr=T.d_table.data_ptr() + 8)
    for field in ("tape_begin", "string_begin"):
        table = T.table.copy()
        i = 100 + int(np.argmax(np.diff(table[field][100:].astype(np.int64)) > 0))
        table[field][[i, i + 1]] = table[field][[i + 1, i]]
        assert table[field][i] > table[field][i + 1]
        back = torch.from_numpy(table.view(np.int32)).cuda()
        assert refused(table_ptr=back.data_ptr())
    table = T.table.copy()
    table["tape_begin"][-1] += 1  # ends behind the tape
    assert refused(table_ptr=torch.from_numpy(table.view(np.int32)).cuda().data_ptr())
    out = np.zeros(1, np.uint64)
    L, h = parser.L, parser.h
    assert L.sjgpu_at_paths_wide_device(h, None, 0, None, 0, None, 1, None, None, 0, None, None, None, None, 0, None, out.ctypes.data_as(capi.ctypes.POINTER(capi.ctypes.c_uint64))) == E_BADARG
    assert L.sjgpu_at_paths_wide_device(None, None, 0, None, 0, None, 1, None, None, 0, None, None, None, None, 0, None, None) == E_BADARG
    # a path that is an error for every container root, between its neighbours: their rows are what they were
    status, offsets, tags, values = column(wide, T, [b"$[*]", b"a[*]", b"$.name", b"$.*"])
    roots = np.array([d[:1] in (b"{", b"[") for d in docs])
    assert (status[1][roots] == 22).all() and (status[1][~roots] == 0).all() and (np.diff(offsets.astype(np.int64))[300:600] == 0).all()
    assert np.array_equal(tags, base[2]) and np.array_equal(values, base[3]) and np.array_equal(np.delete(status, 1, axis=0), base[0])


# ---- 6. one context, call after call -----------------------------------------------------------------------------------------------------------------
def test_a_smaller_stream_behind_a_larger_one(parser, small, statuses):
    """the annotation and the workspace of the first call must not show in the second: both equal what fresh contexts give"""
    _, big = small
    n, doc = statuses
    little = Tapes.of_stream(parser, [doc[:13] + doc[13:].split(b"},{", 1)[0] + b"}]}", b"[[1],[2,[3]]]", b'{"statuses":[]}'])
    first_paths, second_paths = [b"$.tags[*]", b"$[*]", b"$.*"], [b"$.statuses[*].tags[*]", b"$[*][*]"]
    fresh = []
    for T, paths in ((big, first_paths), (little, second_paths)):
        q = capi.DomParserImplementation(narrow.CAP)
        fresh.append(column(Wide(q), T, paths))
        q.close()
    q = capi.DomParserImplementation(narrow.CAP)
    same(column(Wide(q), big, first_paths), fresh[0])
    same(column(Wide(q), little, second_paths), fresh[1])
    q.close()
    same(fresh[1], column(parser, little, second_paths))
    assert len(fresh[1][2]) == 3 + 4


# ---- 7. composition --------------------------------------------------------------------------------------------------------------------------------
def test_explode_many(parser):
    rng = np.random.default_rng(74)
    paths = [b"$.tags[*]", b"$[*]", b"$.f[*][*]", b"$.name", b"$.a.b.c[*].d"]
    valid = stream_cases.small_records(rng, 3000)
    stream, _ = stream_cases.join(valid, b"\n")
    want = parser.explode_many(stream, paths)
    assert want[:2] == (0, 3000) and len(want[4]) > 3000
    got = parser.explode_many(stream, paths, wide=True)
    assert got[:2] == want[:2]
    same(got[2:], want[2:])
    for first_cap in (0, 1, len(want[4]) - 1):  # a first guess that is too small
        got = parser.explode_many(stream, paths, first_cap=first_cap, wide=True)
        assert got[:2] == want[:2]
        same(got[2:], want[2:])
    broken = valid[:1200] + [b'{"a":tru}'] + valid[1200:]
    stream, _ = stream_cases.join(broken, b"\n")
    want = parser.explode_many(stream, paths)
    got = parser.explode_many(stream, paths, wide=True)
    assert got[:2] == want[:2] == (6, 1200)
    same(got[2:], want[2:])
    assert parser.explode_many(b"", paths, wide=True)[:2] == (13, 0)
