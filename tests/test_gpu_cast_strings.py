"""GPU tier (-m gpu): numbers held in strings -- sjgpu_cast_string_cells_device (k_cast_string_cells and k_cast_strings_exact in sjgpu_cast_strings.hip,
include/sjgpu_cast_strings.h) and capi.numbers_in_strings_many -- bit for bit against tests/golden/in_string.json (the real reference's answers) on cells the
device's own parse made, against tests/in_string_model.py (pinned against that fixture on the CPU tier) on synthetic rows, and against Python's int() on
twitter.json's id_str fields.  Every output has exactly the contracted size inside a poisoned tensor whose poison is checked after every call; the tag and
code rows and the string buffer begin at odd addresses."""
import json
import os

import numpy as np
import pytest

import in_string_cases as cases
import in_string_model as model
from simdjson_amd import _paths, build, capi

pytestmark = pytest.mark.gpu

CAP = 128 << 20
E_BADARG = -4
GUARD = 65  # odd: with it the byte rows begin at odd addresses
P64, P32, P8 = 0x5A5A5A5A5A5A5A5A, 0x5A5A5A5A, 0x5A
MARKER = 0xFF
TWITTER = os.path.join(_paths.REPO_ROOT, "tests", "golden", "jsonexamples", "twitter.json")


@pytest.fixture(scope="module")
def parser():
    build.build_sjgpu()
    p = capi.DomParserImplementation(CAP)
    yield p
    p.close()


@pytest.fixture(scope="module")
def buffer():
    return cases.string_buffer(cases.pool())


def call(p, tags, values, sbuf, getters, in_place=False, skew=None, null=(), expect=0, stream=None):
    """sjgpu_cast_string_cells_device over tags uint8[K, n] / values uint64[K, n] and the string buffer's bytes, every output at exactly its contracted size
    between poisoned guards, the byte rows and the string buffer from an odd byte on.  skew: bytes added to an argument's address, null: arguments passed as
    null (by name); expect: the code the call is counted on to return (a refusal must leave everything poisoned); stream: a torch stream, None = the NULL stream
    -> (value_out[K, n], code_out[K, n], valid[K, W], counts[K, 8]) or None after a refusal"""
    import torch
    skew = skew or {}
    tags, values = np.ascontiguousarray(tags, np.uint8), np.ascontiguousarray(values, np.uint64)
    K, n = tags.shape
    cells, W = K * n, (n + 63) // 64
    d_tags = torch.from_numpy(np.concatenate([np.full(GUARD, P8, np.uint8), tags.reshape(-1), np.full(GUARD, P8, np.uint8)])).cuda()
    d_values = torch.from_numpy(np.concatenate([np.full(GUARD, P64, np.uint64), values.reshape(-1), np.full(GUARD, P64, np.uint64)]).view(np.int64)).cuda()
    d_sbuf = torch.from_numpy(np.concatenate([np.full(GUARD, P8, np.uint8), np.frombuffer(sbuf, np.uint8), np.full(GUARD, P8, np.uint8)])).cuda()
    value_out = torch.full((cells + 2 * GUARD,), P64, dtype=torch.int64, device="cuda")
    code_out = torch.full((cells + 2 * GUARD,), P8, dtype=torch.uint8, device="cuda")
    valid = torch.full((K * W + 2 * GUARD,), P64, dtype=torch.int64, device="cuda")
    counts = torch.full((K * 8 + 2 * GUARD,), P32, dtype=torch.int32, device="cuda")
    args = {"sbuf": d_sbuf.data_ptr() + GUARD, "value": d_values.data_ptr() + 8 * GUARD, "tag": d_tags.data_ptr() + GUARD,
            "value_out": (d_values if in_place else value_out).data_ptr() + 8 * GUARD, "code_out": (d_tags if in_place else code_out).data_ptr() + GUARD,
            "valid": valid.data_ptr() + 8 * GUARD, "counts": counts.data_ptr() + 4 * GUARD}
    assert args["tag"] % 2 == 1 and args["code_out"] % 2 == 1 and args["sbuf"] % 2 == 1
    for name, by in skew.items():
        args[name] += by
    for name in null:
        args[name] = 0
    torch.cuda.synchronize()
    rc = capi.cast_string_cells_device(p, args["sbuf"], len(sbuf), args["value"], args["tag"], n, getters, args["value_out"], args["code_out"], args["valid"], args["counts"],
                                       stream.cuda_stream if stream is not None else 0)
    torch.cuda.synchronize()
    assert rc == expect, (rc, p.last_error())
    th, vh, sh = d_tags.cpu().numpy(), d_values.cpu().numpy().view(np.uint64), d_sbuf.cpu().numpy()
    oh, ch = value_out.cpu().numpy().view(np.uint64), code_out.cpu().numpy()
    bh, nh = valid.cpu().numpy().view(np.uint64), counts.cpu().numpy().view(np.uint32)
    done = rc == 0 and K > 0
    wrote_cells = cells if done and not in_place else 0
    assert (oh[:GUARD] == P64).all() and (oh[GUARD + wrote_cells:] == P64).all(), "value_out poison"
    assert (ch[:GUARD] == P8).all() and (ch[GUARD + wrote_cells:] == P8).all(), "code_out poison"
    assert (bh[:GUARD] == P64).all() and (bh[GUARD + (K * W if done and n else 0):] == P64).all(), "valid_out poison"
    assert (nh[:GUARD] == P32).all() and (nh[GUARD + (K * 8 if done else 0):] == P32).all(), "counts poison"
    assert (th[:GUARD] == P8).all() and (th[GUARD + cells:] == P8).all() and (vh[:GUARD] == P64).all() and (vh[GUARD + cells:] == P64).all(), "the guards of the cells"
    assert (sh[:GUARD] == P8).all() and (sh[GUARD + len(sbuf):] == P8).all() and sh[GUARD: GUARD + len(sbuf)].tobytes() == bytes(sbuf), "the string buffer"
    if not (done and in_place):
        assert np.array_equal(th[GUARD: GUARD + cells], tags.reshape(-1)) and np.array_equal(vh[GUARD: GUARD + cells], values.reshape(-1)), "the cells were written"
    if rc or K == 0:
        return None
    src_v, src_c = (vh, th) if in_place else (oh, ch)
    return (src_v[GUARD: GUARD + cells].reshape(K, n).copy(), src_c[GUARD: GUARD + cells].reshape(K, n).copy(), bh[GUARD: GUARD + K * W].reshape(K, W).copy(),
            nh[GUARD: GUARD + K * 8].reshape(K, 8).copy())


def assert_equals(got, want, n):
    for name, mine, theirs in zip(("value_out", "code_out", "valid_out", "counts"), got, want):
        assert np.array_equal(mine, theirs), (name, np.argwhere(mine != theirs)[:5].tolist())
    assert not (got[1] == MARKER).any(), "a marker survived the call"
    if n % 64:
        assert not (got[2][:, -1] >> np.uint64(n % 64)).any(), "the tail bits of a row's last word"


# ---- 1. the fixture end to end ----------------------------------------------------------------------------------------------------------------------------
def check_against_the_fixture(columns, fixture):
    for col, g in zip(columns, model.ALL_GETTERS):
        assert col["getter"] == g and (col["tags"] == 0x22).all() and len(col["codes"]) == len(fixture)
        words = col["values"].view(np.uint64)
        for i, (content, answers) in enumerate(fixture):
            assert (int(col["codes"][i]), int(words[i])) == answers[(g & 0x0F) - 1], (g, content[:60])
        packed = np.packbits(col["codes"] == 0, bitorder="little")
        assert np.array_equal(col["valid"][: len(packed)], packed) and not col["valid"][len(packed):].any()
        assert col["counts"][0] == (col["codes"] == 0).sum() and col["counts"][2] == (col["codes"] == 9).sum() and not col["counts"][[1, 3, 4, 6, 7]].any()
        want_exact = sum(model.takes_the_exact_road(c) for c, _ in fixture) if g & 0x0F == model.DOUBLE else 0
        assert col["counts"][5] == want_exact and (want_exact > 50 or not want_exact)


def test_the_fixture_as_one_document(parser):
    fixture = model.load_fixture()
    doc = b'["' + b'","'.join(c for c, _ in fixture) + b'"]'
    code, docs, row_offsets, columns = capi.numbers_in_strings_many(parser, doc, b"$[*]", [b""] * 6, model.ALL_GETTERS)
    assert (code, docs, row_offsets.tolist()) == (0, 1, [0, len(fixture)])
    check_against_the_fixture(columns, fixture)


def test_the_fixture_as_a_stream_of_documents(parser):
    """one string per document, the cells from sjgpu_at_pointers_device"""
    import torch
    fixture = model.load_fixture()
    data = b"".join(b'"' + c + b'"\n' for c, _ in fixture)
    S = capi.ResidentStream(parser, data)
    assert (S.code, S.docs) == (0, len(fixture))
    K, n = 6, S.docs
    values = torch.empty((K, n), dtype=torch.int64, device=S.dev)
    tags = torch.empty((K, n), dtype=torch.uint8, device=S.dev)
    assert parser.at_pointers_device(*S.args(), [b""] * K, values.data_ptr(), tags.data_ptr(), S.stream) == 0
    valid = torch.empty((K, (n + 63) // 64), dtype=torch.int64, device=S.dev)
    counts = torch.empty((K, 8), dtype=torch.int32, device=S.dev)
    tags_before, cells_before = tags.clone(), values.clone()
    # in place, on the stream of the parse
    assert capi.cast_string_cells_device(parser, S.sbuf.data_ptr(), S.sb, values.data_ptr(), tags.data_ptr(), n, model.ALL_GETTERS, values.data_ptr(), tags.data_ptr(), valid.data_ptr(),
                                         counts.data_ptr(), S.stream) == 0
    S.synchronize()
    vh, ch, bh, nh = values.cpu().numpy().view(np.uint64), tags.cpu().numpy(), valid.cpu().numpy(), counts.cpu().numpy().view(np.uint32)
    columns = [{"getter": g, "tags": tags_before[k].cpu().numpy(), "cells": cells_before[k].cpu().numpy(), "values": vh[k], "codes": ch[k], "valid": bh[k].view(np.uint8), "counts": nh[k]}
               for k, g in enumerate(model.ALL_GETTERS)]
    check_against_the_fixture(columns, fixture)


# ---- 2. random synthetic rows against the model -----------------------------------------------------------------------------------------------------------
SHAPES = [(n, K) for n in (0, 1, 63, 64, 65, 255, 256, 257) for K in (1, 3, 64)] + [(8449, 64)]  # (the last: 32 workgroups per row, a second grid-stride step with a tail)


@pytest.fixture(scope="module")
def random_rows(buffer):
    """the random cells of every shape and the model's answer, made once and left unchanged"""
    sbuf, words = buffer
    rng = np.random.default_rng(291)
    out = {}
    for i, (n, K) in enumerate(SHAPES):
        tags, values = cases.random_cells(rng, n, K, words, len(sbuf))
        getters = cases.cycled(K, i)
        out[(n, K)] = (tags, values, getters, model.cast(tags, values, sbuf, getters)[:4])
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_random_cells_equal_the_model(parser, buffer, random_rows, shape):
    import torch
    n, K = shape
    tags, values, getters, want = random_rows[shape]
    own = torch.cuda.Stream()
    for stream in (None, own, own):  # the NULL stream, a caller's stream, and that once more on the same context: the counters start from zero in every call
        got = call(parser, tags, values, buffer[0], getters, stream=stream)
        if n == 0:
            assert not got[3].any() and got[0].size == 0
        assert_equals(got, want, n)


# ---- 3. exact capacity -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_exact_capacity_with_a_parked_cell(parser, buffer, n):
    """call() lays every output at exactly its contracted size inside a poisoned tensor and checks the poison; a cell of the exact road is in every row, as the
    row's last cell, so its validity bit is the last one the call sets in the row's last word"""
    sbuf, words = buffer
    pool = cases.pool()
    slow = words[pool.index(b"1234567890123456789012345678901234567890e-20")]
    rng = np.random.default_rng(292)
    tags, values = cases.random_cells(rng, n, 3, words, len(sbuf))
    tags[:, -1], values[:, -1] = 0x22, slow
    getters = [model.DOUBLE, model.DOUBLE | model.OR_NUMBER, model.DOUBLE]
    want = model.cast(tags, values, sbuf, getters)
    assert want[4][:, -1].all() and (want[1][:, -1] == 0).all() and (want[0][:, -1] == 0x43E56A95319D63E1).all()
    apart, inplace = call(parser, tags, values, sbuf, getters), call(parser, tags, values, sbuf, getters, in_place=True)
    assert_equals(apart, want[:4], n)
    assert_equals(inplace, want[:4], n)


# ---- 4. the parked road alone ----------------------------------------------------------------------------------------------------------------------------
def test_every_cell_takes_the_exact_road(parser):
    longs = cases.long_decimals()
    sbuf, words = cases.string_buffer(longs)
    n = 257
    values = np.array([[words[i % len(words)] for i in range(n)]], np.uint64)
    tags = np.full((1, n), 0x22, np.uint8)
    want = model.cast(tags, values, sbuf, [model.DOUBLE])
    assert want[3][0].tolist() == [n, 0, 0, 0, 0, n, 0, 0] and len(set(want[0][0].tolist())) >= 6
    assert_equals(call(parser, tags, values, sbuf, [model.DOUBLE]), want[:4], n)
    assert_equals(call(parser, tags, values, sbuf, [model.DOUBLE], in_place=True), want[:4], n)
    # one such cell per wave, at lane 0 and at lane 63: the exact road's bit lands in a word the other road stored
    sbuf, words = cases.string_buffer(longs + [b"1.5"])
    for lane in (0, 63):
        values = np.full((1, n), words[-1], np.uint64)
        values[0, lane::64] = words[1]
        want = model.cast(tags, values, sbuf, [model.DOUBLE])
        assert want[3][0, 5] == len(range(lane, n, 64)) and want[3][0, 0] == n
        assert_equals(call(parser, tags, values, sbuf, [model.DOUBLE]), want[:4], n)


# ---- 5. real data ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
def test_the_id_strings_of_twitter(parser, wide):
    data = open(TWITTER, "rb").read()
    statuses = json.loads(data)["statuses"]
    rows = len(statuses)
    pointers = [b"/id_str", b"/user/id_str", b"/in_reply_to_status_id_str"]
    picks = [lambda s: s["id_str"], lambda s: s["user"]["id_str"], lambda s: s["in_reply_to_status_id_str"]]
    for g in (capi.GETS_INT64, capi.GETS_UINT64):
        code, docs, row_offsets, columns = capi.numbers_in_strings_many(parser, data, b"$.statuses[*]", pointers, [g] * 3, wide=wide)
        assert (code, docs, row_offsets.tolist()) == (0, 1, [0, rows]) and rows == 100
        for col, pick in zip(columns, picks):
            want = [pick(s) for s in statuses]
            nulls = sum(w is None for w in want)
            assert col["values"].dtype == (np.int64 if g == capi.GETS_INT64 else np.uint64)
            assert col["values"].tolist() == [0 if w is None else int(w) for w in want] and col["codes"].tolist() == [17 if w is None else 0 for w in want]
            assert col["counts"].tolist() == [rows - nulls, nulls, 0, 0, nulls, 0, 0, 0]
            assert np.array_equal(col["valid"][: (rows + 7) // 8], np.packbits(col["codes"] == 0, bitorder="little"))
        assert 0 < columns[2]["counts"][1] < rows
    # a column of numbers under the flag is the plain cast of that column
    code, docs, row_offsets, (mixed,) = capi.numbers_in_strings_many(parser, data, b"$.statuses[*]", [b"/id"], [capi.GETS_INT64 | capi.GETS_OR_NUMBER], wide=wide)
    code, docs, row_offsets, (plain,) = parser.typed_table_many(data, b"$.statuses[*]", [b"/id"], getters=[capi.GET_INT64], wide=wide)
    assert mixed["values"].tolist() == plain["values"].tolist() == [s["id"] for s in statuses] and not mixed["codes"].any() and mixed["counts"].tolist() == [rows, 0, 0, 0, 0, 0, 0, 0]
    # ... and without the flag it is refused cell by cell
    code, docs, row_offsets, (refused,) = capi.numbers_in_strings_many(parser, data, b"$.statuses[*]", [b"/id"], [capi.GETS_INT64], wide=wide)
    assert (refused["codes"] == 17).all() and refused["counts"].tolist() == [0, 0, 0, 0, rows, 0, 0, 0] and not refused["values"].any()


# ---- 6. the refusals -----------------------------------------------------------------------------------------------------------------------------------------
def test_the_refusals(parser, buffer):
    sbuf, words = buffer
    rng = np.random.default_rng(293)
    tags, values = cases.random_cells(rng, 65, 3, words, len(sbuf))
    g = [1, 2 | 0x10, 3]
    assert call(parser, tags, values, sbuf, g) is not None
    for name in ("sbuf", "value", "tag", "value_out", "code_out", "valid", "counts"):
        call(parser, tags, values, sbuf, g, null=(name,), expect=E_BADARG)
    for name, by in (("value", 4), ("value_out", 4), ("valid", 4), ("counts", 2)):
        call(parser, tags, values, sbuf, g, skew={name: by}, expect=E_BADARG)
    for bad in (0, 4, 7, 0x10, 0x14, 0x21, 0x81, 255):
        call(parser, tags, values, sbuf, [1, bad, 3], expect=E_BADARG)
    t65, v65 = cases.random_cells(rng, 5, 65, words, len(sbuf))
    call(parser, t65, v65, sbuf, cases.cycled(65), expect=E_BADARG)
    # K == 0: 0 and nothing written; n == 0: the counters alone; a null string buffer of no bytes: every string points outside or is empty
    assert call(parser, np.zeros((0, 9), np.uint8), np.zeros((0, 9), np.uint64), sbuf, []) is None
    got = call(parser, np.zeros((2, 0), np.uint8), np.zeros((2, 0), np.uint64), sbuf, [1, 3], null=("sbuf", "value", "tag", "value_out", "code_out", "valid"))
    assert not got[3].any()
    got = call(parser, np.full((1, 2), 0x22, np.uint8), np.array([[0, 1 << 32]], np.uint64), b"", [3], null=("sbuf",))
    assert got[1].tolist() == [[17, 17]] and got[3].tolist() == [[0, 0, 0, 0, 0, 0, 1, 0]]
    # no context
    assert parser.L.sjgpu_cast_string_cells_device(None, None, 0, None, None, 0, 0, None, None, None, None, None, None) == E_BADARG
