"""GPU tier (-m gpu): JSONPath with wildcards over device tapes -- sjgpu_at_paths_device (k_at_paths in sjgpu_query.hip, include/sjgpu_paths.h) and
capi.explode_many -- against tests/golden/paths.json (the real reference's at_path_with_wildcard, cell by cell) and tests/path_model.py (pinned against that
fixture and against Python's json on the CPU tier).  The tapes are the device's own: sjgpu_stage2_many_device / sjgpu_stage2_device.  Every output has
exactly the contracted size inside a poisoned tensor whose poison is checked after every call."""
import numpy as np
import pytest

import path_cases
import path_model
import pointer_model
import stream_cases
from simdjson_amd import build, capi
from test_gpu_query import Tapes, gather
from test_gpu_stream_tape import Resident

pytestmark = pytest.mark.gpu

CAP = 128 << 20
E_BADARG, E_OVERFLOW = -4, -5
GUARD = 65  # odd: with it the status and tag rows begin at odd addresses
P64, P32, P8 = 0x5A5A5A5A5A5A5A5A, 0x5A5A5A5A, 0x5A


@pytest.fixture(scope="module")
def parser():
    build.build_sjgpu()
    p = capi.DomParserImplementation(CAP)
    yield p
    p.close()


def call(p, T, paths, cap, docs=None, table_ptr=None, tape_ptr=None, offsets_skew=0, value_skew=0, expect=None):
    """one sjgpu_at_paths_device with outputs of exactly K * docs + 1 words, K * docs bytes and `cap` matches between poisoned guards
    -> (rc, matches, status[K, docs], offsets[K * docs + 1], tags[matches], values[matches]); expect: the rc the caller counts on (decides what must have been written)"""
    torch = T.torch
    docs = T.docs if docs is None else docs
    K = len(paths)
    cells = K * docs
    offsets = torch.full((cells + 1 + 2 * GUARD,), P32, dtype=torch.int32, device="cuda")
    status = torch.full((cells + 2 * GUARD,), P8, dtype=torch.uint8, device="cuda")
    values = torch.full((cap + 2 * GUARD,), P64, dtype=torch.int64, device="cuda")
    tags = torch.full((cap + 2 * GUARD,), P8, dtype=torch.uint8, device="cuda")
    rc, matches = p.at_paths_device(tape_ptr or T.d_tape.data_ptr(), len(T.tape), T.d_sbuf.data_ptr(), len(T.sbuf), table_ptr or T.d_table.data_ptr(), docs, paths,
                                    offsets.data_ptr() + 4 * GUARD + offsets_skew, status.data_ptr() + GUARD, values.data_ptr() + 8 * GUARD + value_skew,
                                    tags.data_ptr() + GUARD, cap, T.stream)
    torch.cuda.synchronize()
    oh, sh = offsets.cpu().numpy().view(np.uint32), status.cpu().numpy()
    vh, th = values.cpu().numpy().view(np.uint64), tags.cpu().numpy()
    if expect is not None:
        assert rc == expect, (rc, expect, p.last_error())
    nothing = rc == E_BADARG
    empty = K == 0 or docs == 0
    wrote_offsets = 0 if nothing else (1 if empty else cells + 1)
    wrote_status = 0 if nothing or empty else cells
    wrote_matches = matches if rc == 0 else 0
    assert (oh[:GUARD] == P32).all() and (oh[GUARD + wrote_offsets:] == P32).all(), "offsets poison"
    assert (sh[:GUARD] == P8).all() and (sh[GUARD + wrote_status:] == P8).all(), "status poison"
    assert (vh[:GUARD] == P64).all() and (vh[GUARD + wrote_matches:] == P64).all(), "value poison"
    assert (th[:GUARD] == P8).all() and (th[GUARD + wrote_matches:] == P8).all(), "tag poison"
    return (rc, matches, sh[GUARD: GUARD + wrote_status].reshape(K, -1).copy() if wrote_status else np.zeros((K, docs), np.uint8), oh[GUARD: GUARD + wrote_offsets].copy(),
            th[GUARD: GUARD + wrote_matches].copy(), vh[GUARD: GUARD + wrote_matches].copy())


def column(p, T, paths, docs=None):
    """the ragged column at its EXACT capacity: a call with room for nothing says what is needed (and leaves offsets and status complete), the second fills
    -> (status, offsets, tags, values)"""
    rc, matches, status0, offsets0, _, _ = call(p, T, paths, 0, docs)
    if matches == 0:
        assert rc == 0
        return status0, offsets0, np.zeros(0, np.uint8), np.zeros(0, np.uint64)
    assert rc == E_OVERFLOW and int(offsets0[-1]) == matches
    rc, again, status, offsets, tags, values = call(p, T, paths, matches, docs, expect=0)
    assert again == matches and np.array_equal(status, status0) and np.array_equal(offsets, offsets0)
    return status, offsets, tags, values


def model_cells(T, paths, which=None):
    """[k][j] -> (status, [(tag, value)]) for the documents `which`, offsets and indices absolute in the stream"""
    which = range(T.docs) if which is None else which
    out = [[None] * len(which) for _ in paths]
    for j, d in enumerate(which):
        tape, sbuf, t0, s0 = T.parsed(d)
        for k, path in enumerate(paths):
            out[k][j] = path_model.matches(tape, sbuf, path, t0, s0)
    return out


def as_column(cells, docs=None):
    """the first `docs` documents of model_cells' rows as (status, offsets, tags, values)"""
    K = len(cells)
    docs = (len(cells[0]) if K else 0) if docs is None else docs
    status = np.array([[cells[k][d][0] for d in range(docs)] for k in range(K)], np.uint8).reshape(K, docs)
    offsets, tags, values = [0], [], []
    for k in range(K):
        for d in range(docs):
            for t, v in cells[k][d][1]:
                tags.append(t)
                values.append(v)
            offsets.append(len(tags))
    return status, np.array(offsets, np.uint32), np.array(tags, np.uint8), np.array(values, np.uint64)


# ---- 1. the fixture -----------------------------------------------------------------------------------------------------------------------------
def test_fixture_as_one_stream_and_document_by_document(parser):
    import torch
    docs, paths, cells = path_cases.fixture()
    T = Tapes.of_stream(parser, docs)
    for first in range(0, len(paths), 64):
        part = paths[first: first + 64]
        status, offsets, tags, values = column(parser, T, part)
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
            status, offsets, tags, values = column(parser, one, part)
            for j in range(len(part)):
                assert path_cases.render(*path_cases.cell(status, offsets, tags, values, j, 0, 1), one.sbuf) == cells[i][first + j], (d[:80], part[j][:40])


# ---- 2. shapes where count, scan and fill can disagree ---------------------------------------------------------------------------------------------
DENSE_ZERO_DENSE = [b"$[*]", b"$.missing[*]", b"$.*"]  # a path without any match between two dense ones


@pytest.fixture(scope="module")
def small(parser):
    rng = np.random.default_rng(71)
    docs = stream_cases.small_records(rng, 5000)
    T = Tapes.of_stream(parser, docs)
    return docs, T, model_cells(T, DENSE_ZERO_DENSE)


@pytest.mark.parametrize("docs", [1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 5000])
def test_small_records_in_front_of_a_cut(parser, small, docs):
    """the edges of the workgroup (256 cells) and of the scan's block (4 096 entries of K * docs + 1), with one path and with three"""
    _, T, cells = small
    path_cases.assert_column(column(parser, T, DENSE_ZERO_DENSE[:1], docs), as_column(cells[:1], docs), "K = 1: ")
    got = column(parser, T, DENSE_ZERO_DENSE, docs)
    path_cases.assert_column(got, as_column(cells, docs), "K = 3: ")
    counts = np.diff(got[1].astype(np.int64)).reshape(3, docs)
    assert (counts[1] == 0).all() and (got[0] == 0).all()
    if docs >= 63:
        assert (counts[0] > 0).mean() > 0.5 and (counts[2] > 0).mean() > 0.5


def test_one_long_document_among_short_ones_and_a_total_of_zero(parser):
    docs = stream_cases.small_records(np.random.default_rng(72), 600)
    docs[300] = b"[" + b",".join([b"%d" % i, b'"s%d"' % i, b"[%d,[%d]]" % (i, i), b'{"k":%d.5}' % i, b"null"][i % 5] for i in range(3000)) + b"]"
    T = Tapes.of_stream(parser, docs)
    paths = [b"$[*]", b"$[*][*]", b"$[*].k"]
    got = column(parser, T, paths)
    path_cases.assert_column(got, as_column(model_cells(T, paths)))
    counts = np.diff(got[1].astype(np.int64)).reshape(3, 600)
    assert counts[0, 300] == 3000 and counts[1, 300] == 1800 and counts[2, 300] == 600
    path_cases.check_container_matches(got[2], got[3], T.tape)
    # nothing matches anywhere: offsets all zero, nothing written to the (empty) rows
    status, offsets, tags, values = column(parser, T, [b"$.missing[*]", b"$.nope.*"])
    assert not offsets.any() and offsets.shape == (1201,) and not status.any() and tags.size == values.size == 0
    scalars = Tapes.of_stream(parser, [b"1", b'"s"', b"null", b"[]", b"{}"] * 60)
    status, offsets, tags, values = column(parser, scalars, [b"$[*]", b"$.*", b""])
    assert not offsets.any() and status[:2].sum() == 0 and tags.size == 0
    assert status[2].tolist() == [0, 0, 0, 22, 22] * 60  # the empty path: nothing for a scalar root, INVALID_JSON_POINTER for a container


# ---- 3. capacity ----------------------------------------------------------------------------------------------------------------------------------
def test_capacity(parser, small):
    _, T, cells = small
    want = as_column(cells, 1000)
    total = len(want[2])
    assert total > 2000
    rc, matches, status, offsets, tags, values = call(parser, T, DENSE_ZERO_DENSE, total, 1000, expect=0)
    path_cases.assert_column((status, offsets, tags, values), want)
    for cap in (total - 1, 0):
        rc, matches, status, offsets, tags, values = call(parser, T, DENSE_ZERO_DENSE, cap, 1000, expect=E_OVERFLOW)  # (values and tags still poison: checked inside)
        assert matches == total and tags.size == 0
        path_cases.assert_column((status, offsets), want[:2])
    rc, matches, status, offsets, tags, values = call(parser, T, DENSE_ZERO_DENSE, total + 100, 1000, expect=0)  # room to spare stays poison
    path_cases.assert_column((status, offsets, tags, values), want)


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------------------------------
def test_contract(parser):
    import torch
    docs = stream_cases.small_records(np.random.default_rng(73), 300)
    T = Tapes.of_stream(parser, docs)
    paths = [b"$[*]", b"$.name", b"$.*"]
    base = column(parser, T, paths)
    total = len(base[2])

    def refused(paths=paths, **kw):
        return call(parser, T, paths, total, **kw)[0] == E_BADARG  # (nothing written: the poison check inside)
    assert refused([b"$[*]"] * 65) and call(parser, T, [b"$.nope[*]"] * 64, 0, expect=0)[1] == 0
    assert refused([b"$." + b"a" * 1023]) and call(parser, T, [b"$." + b"a" * 1022], 0, expect=0)[1] == 0
    assert refused([b"$" + b"[*]" * 9]) and call(parser, T, [b"$" + b"[*]" * 8], 0, expect=0)[1] == 0
    assert refused([b"$" + b"[*]" * 8 + b".a.b"]) is False and refused([b"$" + b"[*]" * 9 + b".a"])
    assert refused([b"$" + b".a" * 32 + b"[*]"]) and call(parser, T, [b"$" + b".a" * 31 + b"[*]"], 0, expect=0)[1] == 0  # 33 levels, 32 levels
    assert refused([b"$" + b".a" * 33]) and call(parser, T, [b"$" + b".a" * 32], 0, expect=0)[1] == 0                      # 33 pointer tokens in one level, 32
    assert refused(offsets_skew=2) and refused(value_skew=4)
    assert refused(tape_ptr=T.d_tape.data_ptr() + 4) and refused(table_ptr=T.d_table.data_ptr() + 8)
    for field in ("tape_begin", "string_begin"):
        table = T.table.copy()
        i = 100 + int(np.argmax(np.diff(table[field][100:].astype(np.int64)) > 0))  # (a document without a string takes no byte of the string buffer)
        table[field][[i, i + 1]] = table[field][[i + 1, i]]
        assert table[field][i] > table[field][i + 1]
        back = torch.from_numpy(table.view(np.int32)).cuda()
        assert refused(table_ptr=back.data_ptr())
    table = T.table.copy()
    table["tape_begin"][-1] += 1  # ends behind the tape
    assert refused(table_ptr=torch.from_numpy(table.view(np.int32)).cuda().data_ptr())
    out = np.zeros(1, np.uint64)
    L, h = parser.L, parser.h
    assert L.sjgpu_at_paths_device(h, None, 0, None, 0, None, 1, None, None, 0, None, None, None, None, 0, None, out.ctypes.data_as(capi.ctypes.POINTER(capi.ctypes.c_uint64))) == E_BADARG
    assert L.sjgpu_at_paths_device(None, None, 0, None, 0, None, 1, None, None, 0, None, None, None, None, 0, None, None) == E_BADARG
    # K == 0 and docs == 0: success, offsets[0] = 0 and nothing else
    rc, matches, _, offsets, _, _ = call(parser, T, [], 0, expect=0)
    assert matches == 0 and offsets.tolist() == [0]
    rc, matches, _, offsets, _, _ = call(parser, T, paths, 0, docs=0, expect=0)
    assert matches == 0 and offsets.tolist() == [0]
    # a path that is an error for every container root, between its neighbours: their rows are what they were
    status, offsets, tags, values = column(parser, T, [b"$[*]", b"a[*]", b"$.name", b"$.*"])
    roots = np.array([d[:1] in (b"{", b"[") for d in docs])
    assert (status[1][roots] == 22).all() and (status[1][~roots] == 0).all() and (np.diff(offsets.astype(np.int64))[300:600] == 0).all()
    assert np.array_equal(tags, base[2]) and np.array_equal(values, base[3]) and np.array_equal(np.delete(status, 1, axis=0), base[0])


# ---- 5. random documents --------------------------------------------------------------------------------------------------------------------------
def test_two_thousand_random_documents(parser):
    """16 paths: the 14 commonest pointers of the documents rendered as JSONPaths with every index turned into `[*]`, then `$[*]` and `$.*`"""
    rng = np.random.default_rng(61)
    docs = stream_cases.valid_documents(rng, 2000)
    T = Tapes.of_stream(parser, docs)
    paths = path_cases.wildcard_paths(docs, 14)
    assert len(paths) == len(set(paths)) == 16
    got = column(parser, T, paths)
    path_cases.assert_column(got, as_column(model_cells(T, paths)))
    path_cases.check_container_matches(got[2], got[3], T.tape)
    counts = np.diff(got[1].astype(np.int64)).reshape(16, 2000)
    print("matches per path:", counts.sum(axis=1).tolist(), "cells with a status:", int((got[0] != 0).sum()))
    assert (counts[14] + counts[15] > 0).sum() > 500  # (every container root with a child)


# ---- 6. composition -----------------------------------------------------------------------------------------------------------------------------
def test_gather_over_the_flattened_column(parser, small):
    docs, T, _ = small
    status, offsets, tags, values = column(parser, T, [b"$.tags[*]"])
    cells = model_cells(T, [b"$.tags[*]"])
    strings = [pointer_model.string_of(T.sbuf, v) for _, found in cells[0] for t, v in found]
    assert len(strings) == len(tags) > 1000 and set(strings) == {b"a", b"b\n"} and (tags == ord('"')).all()
    lengths = np.array([len(s) for s in strings], np.uint64)
    total = int(lengths.sum())
    rc, got_total, goffsets, chars = gather(parser, T, tags, values, want_total=total)  # the flattened rows are one row of `matches` cells
    assert (rc, got_total) == (0, total) and chars == b"".join(strings)
    assert np.array_equal(goffsets, np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint32))


def test_explode_many(parser):
    rng = np.random.default_rng(74)
    paths = [b"$.tags[*]", b"$[*]", b"$.f[*][*]", b"$.name", b"$.a.b.c[*].d"]
    valid = stream_cases.small_records(rng, 3000)
    stream, _ = stream_cases.join(valid, b"\n")
    T = Tapes.of_stream(parser, valid)
    want = column(parser, T, paths)
    code, docs, status, offsets, tags, values = parser.explode_many(stream, paths)
    assert (code, docs) == (0, 3000)
    path_cases.assert_column((status, offsets, tags, values), want)
    # a first guess that is too small: the second call has the capacity the first reported
    for first_cap in (0, 1, len(want[2]) - 1):
        code, docs, status, offsets, tags, values = parser.explode_many(stream, paths, first_cap=first_cap)
        assert (code, docs) == (0, 3000)
        path_cases.assert_column((status, offsets, tags, values), want)
    # a broken document in the middle: the documents in front of it, and its code
    broken = valid[:1200] + [b'{"a":tru}'] + valid[1200:]
    stream, _ = stream_cases.join(broken, b"\n")
    code, docs, status, offsets, tags, values = parser.explode_many(stream, paths)
    assert (code, docs) == (6, 1200) and status.shape == (len(paths), 1200)
    path_cases.assert_column((status, offsets, tags, values), column(parser, T, paths, docs=1200))
    assert parser.explode_many(b"", paths)[:2] == (13, 0)
