"""GPU tier (-m gpu): dictionaries over device cells -- sjgpu_dictionary_encode_device and sjgpu_cell_kinds_by_code_device (sjgpu_dict.hip, include/sjgpu_dict.h) and
dictionary.dictionary_many / schema_many -- against tests/dictionary_model.py (pinned against tests/golden/dictionary.json on the CPU tier), the fixture itself and
Python's json.  The tapes are the device's own (sjgpu_stage2_many_device), the rows what sjgpu_at_paths_device delivered, the key row of
sjgpu_object_fields_from_cells_device and the dictionary row of the encode itself.  Every output has exactly the contracted size inside a poisoned tensor whose
poison is checked after every call, the tag rows begin at odd addresses, and every dictionary is made twice: with capacity 0, then at the capacity that call
reported, with identical codes."""
import ctypes
import json
import os

import numpy as np
import pytest

import dictionary_cases
import dictionary_model
import stream_cases
from dictionary_cases import KEYS, ROW_COUNTS, STRING
from simdjson_amd import _paths, build, capi, dictionary
from test_gpu_fields import column as fields_column
from test_gpu_fields import matches
from test_gpu_query import Tapes, query

pytestmark = pytest.mark.gpu

CAP = 128 << 20
E_BADARG, E_OVERFLOW = -4, -5
GUARD = 65  # odd: with it the tag rows begin at odd addresses
P64, P32, P8 = 0x5A5A5A5A5A5A5A5A, 0x5A5A5A5A, 0x5A
TWITTER = os.path.join(_paths.REPO_ROOT, "tests", "golden", "jsonexamples", "twitter.json")


@pytest.fixture(scope="module")
def parser():
    build.build_sjgpu()
    p = capi.DomParserImplementation(CAP)
    yield p
    p.close()


class Buffer:
    """a string buffer in device memory at its exact size (what lies behind is no slack), and its host copy"""

    def __init__(self, sbuf):
        import torch
        self.torch = torch
        self.stream = torch.cuda.current_stream().cuda_stream
        self.sbuf = np.ascontiguousarray(sbuf, np.uint8)
        self.d_sbuf = torch.from_numpy(np.concatenate([self.sbuf, np.full(16, P8, np.uint8)])).cuda()


def device_row(B, row):
    torch = B.torch
    tags, values = np.ascontiguousarray(row[0], np.uint8), np.ascontiguousarray(row[1], np.uint64)
    d_tags = torch.from_numpy(np.concatenate([np.zeros(1, np.uint8), tags])).cuda()  # the row begins at an odd address
    d_values = torch.from_numpy(np.concatenate([values, np.zeros(1, np.uint64)]).view(np.int64)).cuda()  # (never empty: an address to pass)
    return tags, values, d_tags, d_values


def call(p, B, row, cap, row_skew=0, codes_skew=0, value_skew=0, first_skew=0, count_skew=0, expect=None):
    """one sjgpu_dictionary_encode_device over the row (tags[n], values[n]) with outputs of exactly n codes and `cap` dictionary slots between poisoned guards
    -> (rc, distinct, codes[n], (first, values, tags, counts)[distinct]); B: a Buffer or the Tapes of a stream; expect: the rc the caller counts on"""
    torch = B.torch
    tags, values, d_tags, d_values = device_row(B, row)
    n = len(tags)
    codes = torch.full((n + 2 * GUARD,), P32, dtype=torch.int32, device="cuda")
    words = torch.full((cap + 2 * GUARD,), P64, dtype=torch.int64, device="cuda")
    dtags = torch.full((cap + 2 * GUARD,), P8, dtype=torch.uint8, device="cuda")
    first, counts = (torch.full((cap + 2 * GUARD,), P32, dtype=torch.int32, device="cuda") for _ in range(2))
    rc, distinct = dictionary.dictionary_encode_device(p, B.d_sbuf.data_ptr(), len(B.sbuf), d_values.data_ptr() + row_skew, d_tags.data_ptr() + 1, n,
                                                       codes.data_ptr() + 4 * GUARD + codes_skew, words.data_ptr() + 8 * GUARD + value_skew, dtags.data_ptr() + GUARD,
                                                       first.data_ptr() + 4 * GUARD + first_skew, counts.data_ptr() + 4 * GUARD + count_skew, cap, B.stream)
    torch.cuda.synchronize()
    if expect is not None:
        assert rc == expect, (rc, expect, p.last_error())
    wrote_codes = 0 if rc == E_BADARG else n
    wrote = distinct if rc == 0 else 0
    ch = codes.cpu().numpy()
    assert (ch[:GUARD] == P32).all() and (ch[GUARD + wrote_codes:] == P32).all(), "codes poison"
    assert not (ch[GUARD: GUARD + wrote_codes] == P32).any(), "a code was not written"
    wh, th, fh, nh = words.cpu().numpy().view(np.uint64), dtags.cpu().numpy(), first.cpu().numpy().view(np.uint32), counts.cpu().numpy().view(np.uint32)
    for a, poison, name in ((wh, P64, "value"), (th, P8, "tag"), (fh, P32, "first"), (nh, P32, "count")):
        assert (a[:GUARD] == poison).all() and (a[GUARD + wrote:] == poison).all(), f"dictionary {name} poison"
    assert (th[GUARD: GUARD + wrote] == STRING).all(), "a dictionary slot was not written"
    assert np.array_equal(d_tags.cpu().numpy()[1:], tags) and np.array_equal(d_values.cpu().numpy().view(np.uint64)[:n], values), "the row was written"
    s = slice(GUARD, GUARD + wrote)
    return rc, distinct, ch[GUARD: GUARD + wrote_codes].copy(), (fh[s].copy(), wh[s].copy(), th[s].copy(), nh[s].copy())


def encode(p, B, row):
    """the dictionary at its EXACT capacity: a call with room for nothing says what is needed and leaves the codes complete, the second fills; the codes of both
    calls are identical -> (codes, first, values, counts), compared with the model"""
    rc, distinct, codes0, _ = call(p, B, row, 0)
    want = dictionary_model.encode(row[0], row[1], B.sbuf)
    assert distinct == len(want[1]) and np.array_equal(codes0, want[0])
    if distinct == 0:
        assert rc == 0
        return want
    assert rc == E_OVERFLOW
    rc, again, codes, (first, values, tags, counts) = call(p, B, row, distinct, expect=0)
    assert again == distinct and np.array_equal(codes, codes0)
    assert np.array_equal(first, want[1]) and np.array_equal(values, want[2]) and np.array_equal(counts, want[3])
    return want


def census(p, B, codes, value_row, groups, codes_skew=0, kinds_skew=0, raw=False):
    """one sjgpu_cell_kinds_by_code_device: groups * 16 counters between poisoned guards, compared with the model -> kinds[groups, 16]"""
    torch = B.torch
    tags, values, d_tags, d_values = device_row(B, value_row)
    n = len(tags)
    d_codes = torch.from_numpy(np.concatenate([np.ascontiguousarray(codes, np.int32), np.zeros(1, np.int32)])).cuda()
    kinds = torch.full((groups * 16 + 2 * GUARD,), P32, dtype=torch.int32, device="cuda")
    rc = dictionary.kinds_by_code_device(p, d_codes.data_ptr() + codes_skew, d_values.data_ptr(), d_tags.data_ptr() + 1, n, groups, kinds.data_ptr() + 4 * GUARD + kinds_skew, B.stream)
    torch.cuda.synchronize()
    wrote = groups * 16 if rc == 0 else 0
    kh = kinds.cpu().numpy().view(np.uint32)
    assert (kh[:GUARD] == P32).all() and (kh[GUARD + wrote:] == P32).all(), "kinds poison"
    if raw:
        return rc
    assert rc == 0, (rc, p.last_error())
    got = kh[GUARD: GUARD + wrote].reshape(groups, 16).copy()
    assert np.array_equal(got, dictionary_model.kinds_by_code(codes, tags, values, groups)), groups
    return got


# ---- 1. the fixture's documents through the device's own tapes ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("document", [0, 1, 2], ids=["twitter", "citm_catalog", "hand_made"])
def test_fixture_rows_from_the_paths_the_fields_and_the_encode_itself(parser, document):
    docs, cases = dictionary_cases.fixture()
    T = Tapes.of_stream(parser, [docs[document]])
    for c in cases:
        if c["document"] != document:
            continue
        row = matches(parser, T, c["path"])  # sjgpu_at_paths_device
        value_row = row
        if c["mode"] == KEYS:
            _, _, key_tags, key_values, vtags, vvalues = fields_column(parser, T, row)  # sjgpu_object_fields_from_cells_device
            row, value_row = (key_tags, key_values), (vtags, vvalues)
        codes, first, values, counts = encode(parser, T, row)
        what = (c["mode"], c["path"])
        assert codes.tolist() == c["codes"] and first.tolist() == c["first"] and counts.tolist() == c["counts"], what
        assert [dictionary_model.string_of(T.sbuf, STRING, v) for v in values.tolist()] == c["strings"], what
        G = len(first)
        kinds = census(parser, T, codes, value_row, G)
        assert kinds[:, :10].tolist() == c["kinds"], what
        # the dictionary row is a row of string cells: encoded again it gives the codes 0 .. G - 1
        again = encode(parser, T, (np.full(G, STRING, np.uint8), values))
        assert again[0].tolist() == list(range(G)) and (again[3] == 1).all()


def test_small_records(parser):
    """4 097 small records: a string column with nulls, a flattened list column, every value of every object, and the keys of every object with their census"""
    rng = np.random.default_rng(141)
    T = Tapes.of_stream(parser, stream_cases.small_records(rng, 4097))
    for path in (b"$.name", b"$.tags[*]", b"$.*", b"$[*]"):
        row = matches(parser, T, path)
        codes, first, _, counts = encode(parser, T, row)
        assert len(row[0]) > 500 and len(first) > 1
    whole = query(parser, T, [b""])  # sjgpu_at_pointers_device: the root cell of every record
    roots = (whole[0][0], whole[1][0])
    _, _, key_tags, key_values, vtags, vvalues = fields_column(parser, T, roots)
    codes, first, values, counts = encode(parser, T, (key_tags, key_values))
    keys = [dictionary_model.string_of(T.sbuf, STRING, v) for v in values.tolist()]
    assert sorted(keys) == sorted([b"id", b"name", b"ok", b"tags", b"score", b"text", b"n", b"a", b"e", b"f", b"g"]) and int(counts.sum()) == len(key_tags) > 6000
    kinds = census(parser, T, codes, (vtags, vvalues), len(keys))
    assert kinds[keys.index(b"ok")].tolist()[:9] == [0, 0, 0, 0, 0, 0, int(counts[keys.index(b"ok")]), 0, 0] and kinds[keys.index(b"score"), 5] == counts[keys.index(b"score")]


# ---- 2. rows made by hand -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ROW_COUNTS)
def test_rows_at_the_wave_and_workgroup_edges(parser, n):
    rng = np.random.default_rng(200 + n)
    sbuf, (tags, values) = dictionary_cases.string_row(dictionary_cases.mixed_strings(rng, n))
    B = Buffer(sbuf)
    encode(parser, B, (tags, values))
    bad = dictionary_cases.non_string_cells(len(sbuf))
    tags, values = tags.copy(), values.copy()
    for k, i in enumerate(range(0, n, 5)):
        tags[i], values[i] = bad[k % len(bad)]
    codes, first, _, counts = encode(parser, B, (tags, values))
    assert (codes[::5] == -1).all() and int(counts.sum()) == n - len(range(0, n, 5))
    census(parser, B, codes, (tags, values), len(first))


def test_cells_that_are_no_strings(parser):
    sbuf, (tags, values) = dictionary_cases.string_row([b"in", b"side", b"in"])
    B = Buffer(sbuf)
    bad = dictionary_cases.non_string_cells(len(sbuf))
    cells = [(STRING, int(values[0]))] + bad + [(STRING, int(values[1])), (STRING, len(sbuf)), (STRING, int(values[2]))]  # (the empty string at the buffer's end is one)
    row = (np.array([t for t, _ in cells], np.uint8), np.array([v for _, v in cells], np.uint64))
    codes, first, _, counts = encode(parser, B, row)
    assert codes.tolist() == [0] + [-1] * len(bad) + [1, 2, 0] and counts.tolist() == [2, 1, 1]
    nothing = (np.array([t for t, _ in bad], np.uint8), np.array([v for _, v in bad], np.uint64))
    assert len(encode(parser, B, nothing)[1]) == 0


def test_seventy_thousand_cells_of_one_string(parser):
    sbuf, row = dictionary_cases.string_row([b"the only one"] * 70000)
    codes, first, _, counts = encode(parser, Buffer(sbuf), row)
    assert first.tolist() == [0] and counts.tolist() == [70000]


def test_seventy_thousand_distinct_strings(parser):
    sbuf, row = dictionary_cases.string_row([b"%05d" % i + b"-" * (i % 23) for i in range(70000)])
    codes, first, _, counts = encode(parser, Buffer(sbuf), row)
    assert np.array_equal(codes, np.arange(70000)) and (counts == 1).all()


def test_every_wave_holds_the_same_three_strings_in_rotating_order(parser):
    sbuf, row = dictionary_cases.string_row(dictionary_cases.rotating_row(64 * 40 + 17))
    codes, first, _, counts = encode(parser, Buffer(sbuf), row)
    assert first.tolist() == [0, 1, 2]


@pytest.mark.parametrize("groups", [1, 40, 512, 513, 5000])
def test_census_by_code_on_both_sides_of_the_lds_threshold(parser, groups):
    rng = np.random.default_rng(groups)
    n = 20011  # 79 workgroups, the last one partly filled; codes outside the groups on both sides
    B = Buffer(np.zeros(0, np.uint8))
    vtags = rng.choice(np.frombuffer(b'{["ludtfn\x11\x13\x14\x16\x00Z', np.uint8), n)
    vvalues = rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n, dtype=np.uint64)
    codes = rng.integers(-3, groups + 3, n).astype(np.int32)
    codes[:7] = [-1, -2147483648, 2147483647, groups, groups - 1, 0, -1]
    got = census(parser, B, codes, (vtags, vvalues), groups)
    inside = int(((codes >= 0) & (codes < groups)).sum())
    assert inside > n // 8 and inside <= int(got.sum()) <= 2 * inside  # (a negative l counts twice)
    census(parser, B, codes[:0], (vtags[:0], vvalues[:0]), groups)  # n == 0: the rows zeroed


# ---- 3. the calls of simdjson_amd/dictionary.py ----------------------------------------------------------------------------------------------------------------
def test_dictionary_many_and_schema_many_over_twitter(parser):
    data = open(TWITTER, "rb").read()
    statuses = json.loads(data)["statuses"]

    def factorize(column):
        seen, codes = {}, []
        for v in column:
            codes.append(seen.setdefault(v, len(seen)) if isinstance(v, str) else -1)
        return list(seen), codes

    for path, column in ((b"$.statuses[*].lang", [s["lang"] for s in statuses]), (b"$.statuses[*].user.time_zone", [s["user"]["time_zone"] for s in statuses]),
                         (b"$.statuses[*].user.screen_name", [s["user"]["screen_name"] for s in statuses]), (b"$.statuses[*].id", [s["id"] for s in statuses])):
        for wide in (False, True):
            code, docs, row_offsets, codes, dict_offsets, dict_chars, counts = dictionary.dictionary_many(parser, data, path, wide=wide)
            want_strings, want_codes = factorize(column)
            chars = dict_chars.tobytes()
            assert (code, docs) == (0, 1) and row_offsets.tolist() == [0, len(column)] and codes.dtype == np.int32 and codes.tolist() == want_codes, path
            assert [chars[dict_offsets[j]: dict_offsets[j + 1]].decode() for j in range(len(counts))] == want_strings, path
            assert counts.tolist() == [want_codes.count(j) for j in range(len(want_strings))], path
    for row_path, records in ((b"$.statuses[*].user", [s["user"] for s in statuses]), (b"$.statuses[*]", statuses)):
        code, docs, keys, counts, kinds, getters = dictionary.schema_many(parser, data, row_path)
        seen = {}
        for r in records:
            for k, v in r.items():
                seen.setdefault(k, []).append(v)
        assert (code, docs) == (0, 1) and keys == [k.encode() for k in seen] and counts.tolist() == [len(v) for v in seen.values()]
        assert kinds.shape == (len(seen), 16) and kinds.dtype == np.uint32 and getters == capi.infer_getters(kinds)
        for j, values in enumerate(seen.values()):
            want = [sum(isinstance(v, dict) for v in values), sum(isinstance(v, list) for v in values), sum(isinstance(v, str) for v in values),
                    sum(isinstance(v, int) and not isinstance(v, bool) for v in values), 0, sum(isinstance(v, float) for v in values), sum(v is True for v in values),
                    sum(v is False for v in values), sum(v is None for v in values)]
            assert kinds[j, :9].tolist() == want, keys[j]
    assert len(keys) == 25 and getters[keys.index(b"lang")] == capi.GET_STRING and getters[keys.index(b"id")] == capi.GET_INT64
    # no document: nothing to encode
    code, docs, row_offsets, codes, dict_offsets, dict_chars, counts = dictionary.dictionary_many(parser, b"", b"$.a")
    assert docs == 0 and len(codes) == 0 and dict_offsets.tolist() == [0]


# ---- 4. refusals -----------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(parser):
    import torch
    sbuf, row = dictionary_cases.string_row(dictionary_cases.mixed_strings(np.random.default_rng(9), 300))
    B = Buffer(sbuf)
    base = encode(parser, B, row)
    G = len(base[1])

    def refused(**kw):
        return call(parser, B, row, G, **kw)[0] == E_BADARG  # (nothing written: the poison check inside)
    assert refused(row_skew=4) and refused(value_skew=4) and refused(codes_skew=2) and refused(first_skew=2) and refused(count_skew=2) and not refused()
    assert census(parser, B, base[0], row, G, codes_skew=2, raw=True) == E_BADARG and census(parser, B, base[0], row, G, kinds_skew=2, raw=True) == E_BADARG
    # null pointers, one at a time, n above 2^30 and a string buffer beyond 32 bits: refused before anything is read
    ok = torch.zeros(256, dtype=torch.int64, device="cuda")
    total = ctypes.c_uint64(7)
    good = [parser.h, ok.data_ptr(), 8, ok.data_ptr() + 64, ok.data_ptr() + 128, 1, ok.data_ptr() + 192, ok.data_ptr() + 256, ok.data_ptr() + 320, ok.data_ptr() + 384,
            ok.data_ptr() + 448, 8, B.stream, ctypes.byref(total)]
    f = parser.L.sjgpu_dictionary_encode_device
    for at in (0, 1, 3, 4, 6, 7, 8, 9, 10, 13):
        args = list(good)
        args[at] = None
        assert f(*args) == E_BADARG, at
    for at, value in ((5, (1 << 30) + 1), (5, 0xFFFFFFFF), (2, 1 << 32)):
        args = list(good)
        args[at] = value
        assert f(*args) == E_BADARG and total.value == 0, (at, value)
    torch.cuda.synchronize()
    assert not ok.any().item()
    assert f(*good) == 0 and total.value == 0  # (the cell is a zero: no tag, a null)
    torch.cuda.synchronize()
    assert int(ok[24].item()) & 0xFFFFFFFF == 0xFFFFFFFF and not ok[32:].any().item()  # code -1, no dictionary entry
    none = list(good)
    none[7:12] = [None, None, None, None, 0]
    assert f(*none) == 0  # the dictionary arrays may be null when dict_cap is 0
    ok.zero_()
    g = parser.L.sjgpu_cell_kinds_by_code_device
    good = [parser.h, ok.data_ptr(), ok.data_ptr() + 64, ok.data_ptr() + 128, 1, 1, ok.data_ptr() + 192, B.stream]
    for at in (0, 1, 2, 3, 6):
        args = list(good)
        args[at] = None
        assert g(*args) == E_BADARG, at
    torch.cuda.synchronize()
    assert not ok.any().item()
    assert g(*good) == 0
    torch.cuda.synchronize()
    assert ok.view(torch.int32)[48: 64].tolist() == [0] * 14 + [1, 0]  # code 0, tag 0: "every other byte"
    # the neighbours of a call that was refused are what they were
    again = encode(parser, B, row)
    assert all(np.array_equal(a, b) for a, b in zip(again, base))
