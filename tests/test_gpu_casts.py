"""GPU tier (-m gpu): typed getters over cells -- sjgpu_cast_cells_device and sjgpu_cell_kinds_device (k_cast_cells and k_cell_kinds in sjgpu_cast.hip,
include/sjgpu_cast.h) and capi.typed_table_many -- bit for bit against tests/cast_model.py (pinned against tests/golden/casts.json on the CPU tier), against
the fixture's own bits where the compiler's conversions round, and against Python's json on the device's own tapes.  Every output has exactly the contracted
size inside a poisoned tensor whose poison is checked after every call; the tag and code rows begin at odd addresses."""
import json
import os

import numpy as np
import pytest

import cast_model
from simdjson_amd import _paths, build, capi
from test_cast_model import fixture
from test_casts_emu import cycled, random_cells

pytestmark = pytest.mark.gpu

CAP = 128 << 20
E_BADARG = -4
GUARD = 65  # odd: with it the code rows begin at odd addresses
P64, P32, P8 = 0x5A5A5A5A5A5A5A5A, 0x5A5A5A5A, 0x5A
TWITTER = os.path.join(_paths.REPO_ROOT, "tests", "golden", "jsonexamples", "twitter.json")


@pytest.fixture(scope="module")
def parser():
    build.build_sjgpu()
    p = capi.DomParserImplementation(CAP)
    yield p
    p.close()


def call(p, tags, values, getters, in_place=False, skew=None, null=(), expect=0):
    """sjgpu_cell_kinds_device and sjgpu_cast_cells_device over tags uint8[K, n] / values uint64[K, n], every output at exactly its contracted size between
    poisoned guards, the tags (and the codes) from an odd byte on.  skew: bytes added to an argument's address, null: arguments passed as null (by name).
    expect: the code both calls are counted on to return (a refusal must leave everything poisoned)
    -> (kinds[K, 16], value_out[K, n], code_out[K, n], valid[K, W], counts[K, 4]) or None after a refusal"""
    import torch
    skew = skew or {}
    tags, values = np.ascontiguousarray(tags, np.uint8), np.ascontiguousarray(values, np.uint64)
    K, n = tags.shape
    cells, W = K * n, (n + 63) // 64
    stream = torch.cuda.current_stream().cuda_stream
    d_tags = torch.from_numpy(np.concatenate([np.full(GUARD, P8, np.uint8), tags.reshape(-1), np.full(GUARD, P8, np.uint8)])).cuda()
    d_values = torch.from_numpy(np.concatenate([np.full(GUARD, P64, np.uint64), values.reshape(-1), np.full(GUARD, P64, np.uint64)]).view(np.int64)).cuda()
    kinds = torch.full((K * 16 + 2 * GUARD,), P32, dtype=torch.int32, device="cuda")
    value_out = torch.full((cells + 2 * GUARD,), P64, dtype=torch.int64, device="cuda")
    code_out = torch.full((cells + 2 * GUARD,), P8, dtype=torch.uint8, device="cuda")
    valid = torch.full((K * W + 2 * GUARD,), P64, dtype=torch.int64, device="cuda")
    counts = torch.full((K * 4 + 2 * GUARD,), P32, dtype=torch.int32, device="cuda")
    args = {"value": d_values.data_ptr() + 8 * GUARD, "tag": d_tags.data_ptr() + GUARD, "kinds": kinds.data_ptr() + 4 * GUARD,
            "value_out": (d_values if in_place else value_out).data_ptr() + 8 * GUARD, "code_out": (d_tags if in_place else code_out).data_ptr() + GUARD,
            "valid": valid.data_ptr() + 8 * GUARD, "counts": counts.data_ptr() + 4 * GUARD}
    assert args["tag"] % 2 == 1 and args["code_out"] % 2 == 1
    for name, by in skew.items():
        args[name] += by
    for name in null:
        args[name] = 0
    rc_kinds = p.cell_kinds_device(args["value"], args["tag"], n, K, args["kinds"], stream)
    torch.cuda.synchronize()
    kh = kinds.cpu().numpy().view(np.uint32)
    rc_cast = p.cast_cells_device(args["value"], args["tag"], n, getters, args["value_out"], args["code_out"], args["valid"], args["counts"], stream)
    torch.cuda.synchronize()
    assert (rc_kinds, rc_cast) == (expect, expect) or isinstance(expect, tuple) and (rc_kinds, rc_cast) == expect, (rc_kinds, rc_cast, p.last_error())
    th, vh = d_tags.cpu().numpy(), d_values.cpu().numpy().view(np.uint64)
    oh, ch = value_out.cpu().numpy().view(np.uint64), code_out.cpu().numpy()
    bh, nh = valid.cpu().numpy().view(np.uint64), counts.cpu().numpy().view(np.uint32)
    wrote_kinds = 0 if rc_kinds or K == 0 else K * 16
    done = rc_cast == 0 and K > 0
    wrote_cells = cells if done and not in_place else 0
    assert (kh[:GUARD] == P32).all() and (kh[GUARD + wrote_kinds:] == P32).all(), "kinds poison"
    assert (oh[:GUARD] == P64).all() and (oh[GUARD + wrote_cells:] == P64).all(), "value_out poison"
    assert (ch[:GUARD] == P8).all() and (ch[GUARD + wrote_cells:] == P8).all(), "code_out poison"
    assert (bh[:GUARD] == P64).all() and (bh[GUARD + (K * W if done else 0):] == P64).all(), "valid_out poison"
    assert (nh[:GUARD] == P32).all() and (nh[GUARD + (K * 4 if done else 0):] == P32).all(), "counts poison"
    assert (th[:GUARD] == P8).all() and (th[GUARD + cells:] == P8).all() and (vh[:GUARD] == P64).all() and (vh[GUARD + cells:] == P64).all(), "the guards of the cells"
    if not (done and in_place):
        assert np.array_equal(th[GUARD: GUARD + cells], tags.reshape(-1)) and np.array_equal(vh[GUARD: GUARD + cells], values.reshape(-1)), "the cells were written"
    if rc_kinds or rc_cast or K == 0:
        return None
    src_v, src_c = (vh, th) if in_place else (oh, ch)
    return (kh[GUARD: GUARD + K * 16].reshape(K, 16).copy(), src_v[GUARD: GUARD + cells].reshape(K, n).copy(), src_c[GUARD: GUARD + cells].reshape(K, n).copy(),
            bh[GUARD: GUARD + K * W].reshape(K, W).copy(), nh[GUARD: GUARD + K * 4].reshape(K, 4).copy())


def assert_equals_model(got, tags, values, getters):
    kinds, value_out, code_out, valid, counts = got
    assert np.array_equal(kinds, cast_model.kinds(tags, values)), "kinds"
    for name, mine, want in zip(("value_out", "code_out", "valid_out", "counts"), (value_out, code_out, valid, counts), cast_model.cast(tags, values, getters)):
        assert np.array_equal(mine, want), name
    n = tags.shape[1]
    if n % 64:
        assert not (valid[:, -1] >> np.uint64(n % 64)).any(), "the tail bits of a row's last word"


SHAPES = [(0, 3), (1, 1), (63, 2), (64, 1), (65, 3), (255, 1), (256, 2), (257, 64), (1000, 7), (4097, 3),
          (8449, 64)]  # (64 rows share 2 048 workgroups, 32 each: the second step of the grid-stride loop, with a tail)


@pytest.fixture(scope="module")
def cells():
    """the random cells of every shape, made once"""
    rng = np.random.default_rng(95)
    return {shape: random_cells(rng, *shape) for shape in SHAPES}


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_random_cells_equal_the_model(parser, cells, shape):
    n, K = shape
    tags, values = cells[shape]
    for first in range(7 if K < 7 else 1):  # all seven getters on every shape
        getters = cycled(K, first)
        assert_equals_model(call(parser, tags, values, getters), tags, values, getters)


@pytest.mark.parametrize("shape", [(65, 3), (257, 2)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_exact_capacity_and_tail_bits(parser, shape):
    """call() lays every output at exactly its contracted size inside a poisoned tensor and checks the poison; here also rows whose cells are all valid: the
    tail of each row's last word stays 0 where every lane of the wave would vote 1"""
    n, K = shape
    tags = np.full((K, n), ord("l"), np.uint8)
    values = np.arange(K * n, dtype=np.uint64).reshape(K, n)
    getters = [cast_model.INT64, cast_model.DOUBLE, cast_model.UINT64][:K]
    got = call(parser, tags, values, getters)
    assert_equals_model(got, tags, values, getters)
    kinds, value_out, code_out, valid, counts = got
    assert (counts[:, 0] == n).all() and not code_out.any()
    assert (valid[:, :-1] == np.uint64(0xFFFFFFFFFFFFFFFF)).all() and (valid[:, -1] == np.uint64((1 << (n % 64)) - 1)).all()
    rng = np.random.default_rng(96)
    tags, values = random_cells(rng, n, K)
    assert_equals_model(call(parser, tags, values, cycled(K, 2)), tags, values, cycled(K, 2))


@pytest.mark.parametrize("shape", [(65, 3), (257, 64), (4097, 3), (0, 3)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_in_place_gives_what_out_of_place_gives(parser, cells, shape):
    n, K = shape
    tags, values = cells[shape]
    getters = cycled(K, 3)
    inplace, apart = call(parser, tags, values, getters, in_place=True), call(parser, tags, values, getters)
    assert_equals_model(inplace, tags, values, getters)
    for a, b in zip(inplace, apart):
        assert np.array_equal(a, b)


def test_the_rounding_cases_on_the_device(parser):
    """one row asked DOUBLE must carry the bits the REFERENCE's get_double gave (tests/golden/casts.json): a mismatch is a finding about the compiler's
    conversion on the device, not a question of tolerance"""
    xs, pointers, table = fixture()
    first = {x: t[0] for x, t in zip(xs, table) if not isinstance(t, str)}
    u = [b"18446744073709551615", b"18446744073709550592", b"18446744073709550591", b"9223372036854775809"]
    l = [b"9007199254740993", b"-9007199254740993", b"-9223372036854775808"]
    tags = np.array([[ord("u")] * len(u) + [ord("l")] * len(l)], np.uint8)
    values = np.array([[int(x) & 0xFFFFFFFFFFFFFFFF for x in u + l]], np.uint64)
    want = np.array([[int(first[x][2], 16) for x in u + l]], np.uint64)
    assert want.tolist() == [[0x43F0000000000000, 0x43F0000000000000, 0x43EFFFFFFFFFFFFF, 0x43E0000000000000, 0x4340000000000000, 0xC340000000000000, 0xC3E0000000000000]]
    kinds, value_out, code_out, valid, counts = call(parser, tags, values, [cast_model.DOUBLE])
    assert np.array_equal(value_out, want) and not code_out.any() and counts.tolist() == [[7, 0, 0, 0]] and valid.tolist() == [[0x7F]]
    # the same cells asked the integers: the reference's answers, too
    for k, g in ((0, cast_model.INT64), (1, cast_model.UINT64)):
        kinds, value_out, code_out, valid, counts = call(parser, tags, values, [g])
        for i, x in enumerate(u + l):
            a = first[x][k]
            assert (int(code_out[0, i]), int(value_out[0, i])) == ((int(a[2:]), 0) if a.startswith("E ") else (0, int(a, 16))), (x, g)


TWITTER_POINTERS = [b"/id", b"/user/screen_name", b"/favorited", b"/retweeted_status/user/id", b"/in_reply_to_status_id", b"/user", b"/entities/hashtags", b"/text",
                    b"/user/followers_count"]


@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
def test_typed_table_of_twitter(parser, wide):
    data = open(TWITTER, "rb").read()
    statuses = json.loads(data)["statuses"]
    rows = len(statuses)
    code, docs, row_offsets, columns = parser.typed_table_many(data, b"$.statuses[*]", TWITTER_POINTERS, wide=wide)
    assert (code, docs, row_offsets.tolist()) == (0, 1, [0, rows]) and rows == 100
    col = dict(zip(TWITTER_POINTERS, columns))

    def bitmap_is_arrow(c):
        packed = np.packbits(c["codes"] == 0, bitorder="little")
        assert c["valid"].dtype == np.uint8 and len(c["valid"]) == 8 * ((rows + 63) // 64)
        assert np.array_equal(c["valid"][: len(packed)], packed) and not c["valid"][len(packed):].any()
    for c in columns:
        assert c["getter"] != 0 and np.array_equal(c["kinds"], cast_model.kinds(c["tags"][None, :], c["cells"][None, :])[0])
        bitmap_is_arrow(c)
    c = col[b"/id"]
    assert c["getter"] == capi.GET_INT64 and c["values"].dtype == np.int64 and c["values"].tolist() == [s["id"] for s in statuses]
    assert c["counts"].tolist() == [100, 0, 0, 0] and not c["codes"].any()
    c = col[b"/user/screen_name"]
    names = [s["user"]["screen_name"].encode() for s in statuses]
    assert c["getter"] == capi.GET_STRING and c["chars"].tobytes() == b"".join(names) and c["offsets"].tolist() == np.cumsum([0] + [len(x) for x in names]).tolist()
    assert c["counts"].tolist() == [100, 0, 0, 0]
    c = col[b"/text"]
    texts = [s["text"].encode() for s in statuses]
    assert c["getter"] == capi.GET_STRING and c["chars"].tobytes() == b"".join(texts) and c["offsets"].tolist() == np.cumsum([0] + [len(x) for x in texts]).tolist()
    c = col[b"/favorited"]
    assert c["getter"] == capi.GET_BOOL and c["values"].dtype == np.bool_ and c["values"].tolist() == [s["favorited"] for s in statuses] and c["counts"][0] == 100
    c = col[b"/retweeted_status/user/id"]
    want = [s["retweeted_status"]["user"]["id"] if "retweeted_status" in s else None for s in statuses]
    assert c["getter"] == capi.GET_INT64 and c["counts"].tolist() == [73, 0, 0, 27] and sum(w is None for w in want) == 27
    assert c["codes"].tolist() == [20 if w is None else 0 for w in want] and c["values"].tolist() == [w or 0 for w in want]
    c = col[b"/in_reply_to_status_id"]
    want = [s["in_reply_to_status_id"] for s in statuses]
    nulls = sum(w is None for w in want)
    assert 0 < nulls < 100 and c["getter"] == capi.GET_INT64 and c["counts"].tolist() == [100 - nulls, nulls, 0, 0]
    assert c["codes"].tolist() == [17 if w is None else 0 for w in want] and c["values"].tolist() == [w or 0 for w in want]
    c = col[b"/user/followers_count"]
    assert c["getter"] == capi.GET_INT64 and c["values"].tolist() == [s["user"]["followers_count"] for s in statuses]
    for pointer, getter, tag in ((b"/user", capi.GET_OBJECT, "{"), (b"/entities/hashtags", capi.GET_ARRAY, "[")):
        c = col[pointer]
        assert c["getter"] == getter and (c["tags"] == ord(tag)).all() and np.array_equal(c["values"], c["cells"]) and c["counts"].tolist() == [100, 0, 0, 0]
    # getters given: /id as a double and as a string, the inferred ones beside them
    code, docs, row_offsets, given = parser.typed_table_many(data, b"$.statuses[*]", [b"/id", b"/id", b"/favorited"], getters=[capi.GET_DOUBLE, capi.GET_STRING, 0], wide=wide)
    assert [c["getter"] for c in given] == [capi.GET_DOUBLE, capi.GET_STRING, capi.GET_BOOL]
    assert given[0]["values"].dtype == np.float64 and given[0]["values"].tolist() == [float(s["id"]) for s in statuses]
    assert (given[1]["codes"] == 17).all() and given[1]["counts"].tolist() == [0, 0, 0, 0] and not given[1]["valid"].any() and not given[1]["offsets"].any()
    assert len(given[1]["chars"]) == 0


def test_the_refusals(parser):
    rng = np.random.default_rng(97)
    tags, values = random_cells(rng, 65, 3)
    g = cycled(3)
    assert call(parser, tags, values, g) is not None
    for name in ("value", "tag"):
        call(parser, tags, values, g, null=(name,), expect=E_BADARG)
    call(parser, tags, values, g, null=("kinds", "counts"), expect=E_BADARG)
    for name in ("value_out", "code_out", "valid"):
        call(parser, tags, values, g, null=(name,), expect=(0, E_BADARG))
    call(parser, tags, values, g, skew={"value": 4}, expect=E_BADARG)
    for name in ("value_out", "valid"):
        call(parser, tags, values, g, skew={name: 4}, expect=(0, E_BADARG))
    call(parser, tags, values, g, skew={"kinds": 2, "counts": 2}, expect=E_BADARG)
    for bad in (0, 8, 255):
        call(parser, tags, values, [1, bad, 3], expect=(0, E_BADARG))
    t65, v65 = random_cells(rng, 5, 65)
    call(parser, t65, v65, cycled(65), expect=E_BADARG)
    # K == 0: 0 and nothing written; n == 0: the counters alone
    assert call(parser, np.zeros((0, 9), np.uint8), np.zeros((0, 9), np.uint64), []) is None
    kinds, value_out, code_out, valid, counts = call(parser, np.zeros((2, 0), np.uint8), np.zeros((2, 0), np.uint64), [1, 5], null=("value", "tag", "value_out", "code_out", "valid"))
    assert not kinds.any() and not counts.any()
    # no context
    assert parser.L.sjgpu_cell_kinds_device(None, None, None, 0, 0, None, None) == E_BADARG
    assert parser.L.sjgpu_cast_cells_device(None, None, None, 0, 0, None, None, None, None, None, None) == E_BADARG
