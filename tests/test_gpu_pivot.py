"""GPU tier (-m gpu): a map column pivoted into a record table -- sjgpu_pivot_fields_device (k_pivot_fill, k_pivot_scatter; sjgpu_pivot.hip, include/sjgpu_pivot.h)
and pivot.records_many -- against tests/pivot_model.py (pinned against tests/golden/pivot.json, the real reference's at_key and at_key_case_insensitive, on the CPU
tier), the fixture itself end to end, sjgpu_at_pointers_from_cells_device cell for cell, and Python's json.  Every output has exactly the contracted size inside
a poisoned tensor whose poison is checked after every call, the status and tag rows begin at odd addresses, the output words lie at both alignments, and every
call is made twice with identical bytes."""
import json
import os

import numpy as np
import pytest

import dictionary_model
import pivot_cases
import pivot_model
from dictionary_cases import STRING
from simdjson_amd import _paths, build, capi, pivot
from test_gpu_dict import encode
from test_gpu_fields import column as fields_column
from test_gpu_fields import matches
from test_gpu_json import column as json_column
from test_gpu_json import roots_of
from test_gpu_query import Tapes
from test_gpu_rows import rooted

pytestmark = pytest.mark.gpu

CAP = 128 << 20
E_BADARG = -4
GUARD = 65  # odd: with it the tag rows begin at odd addresses
P64, P8 = 0x5A5A5A5A5A5A5A5A, 0x5A
EXAMPLES = os.path.join(_paths.REPO_ROOT, "tests", "golden", "jsonexamples")


@pytest.fixture(scope="module")
def parser():
    build.build_sjgpu()
    p = capi.DomParserImplementation(CAP)
    yield p
    p.close()


def device(a, odd=False):
    """an input in device memory with one element of slack (never empty: an address to pass); odd: behind one byte, so that a byte row begins at an odd address"""
    import torch
    a = np.ascontiguousarray(a)
    a = a.view({np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}.get(a.dtype, a.dtype))
    pad = np.zeros(1, a.dtype)
    return torch.from_numpy(np.concatenate([pad, a] if odd else [a, pad])).cuda()


def call(p, c, raw=False, skews=None, **skew):
    """sjgpu_pivot_fields_device over the case c, made TWICE with outputs of exactly columns * rows cells between poisoned guards -- the words once at a 16-byte
    address and once 8 bytes past one -- and identical bytes; nothing but the cells written -> (tags[columns, rows], values[columns, rows]), or the rc when raw"""
    import torch
    stream = torch.cuda.current_stream().cuda_stream
    rows, columns = len(c["status"]), c["columns"]
    cells = rows * columns
    d_offsets, d_status, d_codes = device(c["offsets"]), device(c["status"], odd=True), device(c["codes"])
    d_values, d_tags = device(c["values"]), device(c["tags"], odd=True)
    d_map = None if c["map"] is None else device(c["map"])
    got = []
    for words_skew in (0, 8):
        values = torch.full((cells + 2 * GUARD + 2,), P64, dtype=torch.int64, device="cuda")
        tags = torch.full((cells + 2 * GUARD,), P8, dtype=torch.uint8, device="cuda")
        lead = GUARD + (((values.data_ptr() + 8 * GUARD + words_skew) % 16) != 0)  # the first cell's word: at a 16-byte address, or 8 bytes past one
        assert (values.data_ptr() + 8 * lead) % 16 == words_skew
        rc = pivot.pivot_fields_device(p, d_offsets.data_ptr() + skew.get("offsets", 0), d_status.data_ptr() + 1, rows, d_codes.data_ptr() + skew.get("codes", 0),
                                       d_values.data_ptr() + skew.get("values", 0), d_tags.data_ptr() + 1, c["fields"], 0 if d_map is None else d_map.data_ptr() + skew.get("map", 0),
                                       c["groups"], columns, values.data_ptr() + 8 * lead + skew.get("out", 0), tags.data_ptr() + GUARD, stream)
        torch.cuda.synchronize()
        wrote = cells if rc == 0 else 0
        vh, th = values.cpu().numpy().view(np.uint64), tags.cpu().numpy()
        assert (vh[:lead] == P64).all() and (vh[lead + wrote:] == P64).all(), "value poison"
        assert (th[:GUARD] == P8).all() and (th[GUARD + wrote:] == P8).all(), "tag poison"
        assert not (th[GUARD: GUARD + wrote] == P8).any() and not (vh[lead: lead + wrote] == P64).any(), "a cell was not written"
        got.append((rc, th[GUARD: GUARD + wrote].copy(), vh[lead: lead + wrote].copy()))
    for name, d, a in (("offsets", d_offsets, c["offsets"]), ("codes", d_codes, c["codes"]), ("values", d_values, c["values"])):
        assert np.array_equal(d.cpu().numpy()[:-1].view(a.dtype), a), f"the {name} were written"
    assert np.array_equal(d_status.cpu().numpy()[1:], c["status"]) and np.array_equal(d_tags.cpu().numpy()[1:], c["tags"]), "the statuses or the tags were written"
    assert got[0][0] == got[1][0] and np.array_equal(got[0][1], got[1][1]) and np.array_equal(got[0][2], got[1][2]), "two runs gave different bytes"
    if raw:
        return got[0][0]
    assert got[0][0] == 0, (got[0][0], p.last_error())
    return got[0][1].reshape(columns, rows), got[0][2].reshape(columns, rows)


def check(p, c):
    tags, values = call(p, c)
    want_tags, want_values = pivot_model.pivot(c["offsets"], c["status"], c["codes"], c["values"], c["tags"], c["fields"], c["map"], c["groups"], c["columns"])
    assert np.array_equal(tags, want_tags) and np.array_equal(values, want_values), (len(c["status"]), c["columns"], c["groups"])
    return tags, values


# ---- 1. the emulator's cases through the library ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", pivot_cases.ROWS)
def test_rows_times_columns(parser, rows):
    for c in pivot_cases.shapes():
        if len(c["status"]) == rows:
            check(parser, c)


@pytest.mark.parametrize("name", list(pivot_cases.special()))
def test_special_cases(parser, name):
    check(parser, pivot_cases.special()[name])


# ---- 2. the fixture end to end --------------------------------------------------------------------------------------------------------------------------------
def long_format(p, T, roots):
    """the fields of the roots and the codes of their keys, by the library -> (a case without map and columns, the dictionary's strings)"""
    status, offsets, key_tags, key_values, vtags, vvalues = fields_column(p, T, roots)  # sjgpu_object_fields_from_cells_device
    codes, first, dict_values, counts = encode(p, T, (key_tags, key_values))            # sjgpu_dictionary_encode_device
    dictionary = [dictionary_model.string_of(T.sbuf, STRING, v) for v in dict_values.tolist()]
    return {"offsets": offsets, "status": status, "codes": codes, "values": vvalues, "tags": vtags, "fields": len(codes), "groups": len(dictionary)}, dictionary


@pytest.mark.parametrize("which", [0, 1, 2])
def test_the_fixture_end_to_end(parser, which):
    """parse_many's tapes -> the root of every record -> its fields -> the dictionary of the keys -> the pivot -> sjgpu_serialize_cells_device per column: the
    texts and codes the reference answers for at_key and, through the map of the folded classes, for at_key_case_insensitive"""
    records, keys, plain, folded = pivot_model.fixture()[which]
    T = Tapes.of_stream(parser, records)
    c, dictionary = long_format(parser, T, roots_of(parser, T))
    for fold, want in ((False, plain), (True, folded)):
        column_of_code, pick = pivot_model.column_map(dictionary, keys, fold)
        columns = max(pick) + 1
        tags, values = check(parser, dict(c, map=column_of_code if dictionary else None, columns=columns))
        texts = []
        for col in range(columns):
            offsets, chars, status = json_column(parser, T, (tags[col], values[col]))
            texts.append(["E %d" % t if 16 <= t < 32 else "V " + chars[int(offsets[r]): int(offsets[r + 1])].decode("utf-8") for r, t in enumerate(tags[col].tolist())])
            assert np.array_equal(status, np.where((tags[col] >= 16) & (tags[col] < 32), tags[col], 0))
        got = [[texts[col][r] for col in pick] for r in range(len(records))]
        assert got == want, (which, fold)


# ---- 3. every pivoted column is the row at_pointer gives for / + the escaped key ----------------------------------------------------------------------------------
def escaped(key):
    return b"/" + key.replace(b"~", b"~0").replace(b"/", b"~1")


def cross_check(p, T, roots, extra_keys=()):
    c, dictionary = long_format(p, T, roots)
    keys = dictionary + list(extra_keys)
    column_of_code, pick = pivot_model.column_map(dictionary, keys, False)
    assert pick == list(range(len(keys)))
    tags, values = check(p, dict(c, map=column_of_code if dictionary else None, columns=len(keys)))
    for k0 in range(0, len(keys), 64):  # the pointer call takes 64 pointers
        want_tags, want_values = rooted(p, T, roots, [escaped(k) for k in keys[k0: k0 + 64]])
        assert np.array_equal(tags[k0: k0 + 64], want_tags) and np.array_equal(values[k0: k0 + 64], want_values), k0
    return keys, tags


@pytest.mark.parametrize("path, distinct", [(b"$.statuses[*]", 25), (b"$.statuses[*].user", 40)])
def test_twitter_against_the_pointers(parser, path, distinct):
    T = Tapes.of_stream(parser, [open(os.path.join(EXAMPLES, "twitter.json"), "rb").read()])
    roots = matches(parser, T, path)
    keys, tags = cross_check(parser, T, roots, [b"absent"])
    assert len(roots[0]) == 100 and len(keys) == distinct + 1 and (tags[-1] == 20).all() and (tags[0] != 20).all()


def test_amazon_against_the_pointers(parser):
    """every record is an array: no field, no key, and every cell of any column is the 17 at_key answers a non-object -- which is what at_pointer answers an array
    for a token that is no index"""
    lines = open(os.path.join(EXAMPLES, "amazon_cellphones.ndjson"), "rb").read().splitlines()
    T = Tapes.of_stream(parser, lines)
    roots = roots_of(parser, T)
    keys, tags = cross_check(parser, T, roots, [b"asin", b"brand", b"title"])
    assert len(roots[0]) == len(lines) > 500 and keys == [b"asin", b"brand", b"title"] and (tags == 17).all()


# ---- 4. records_many ----------------------------------------------------------------------------------------------------------------------------------------------
def test_records_many_over_twitter(parser):
    data = open(os.path.join(EXAMPLES, "twitter.json"), "rb").read()
    statuses = json.loads(data)["statuses"]
    for row_path, records in ((b"$.statuses[*]", statuses), (b"$.statuses[*].user", [s["user"] for s in statuses])):
        code, docs, rows, names, tags, cells, kinds, getters, values, valid, codes = pivot.records_many(parser, data, row_path)
        seen = {}
        for r in records:
            for k in r:
                seen.setdefault(k.encode(), None)
        assert (code, docs, rows) == (0, 1, len(records)) and names == list(seen)
        C, W = len(names), (rows + 63) // 64
        assert tags.shape == cells.shape == values.shape == codes.shape == (C, rows) and kinds.shape == (C, 16) and valid.shape == (C, W) and getters == capi.infer_getters(kinds)
        bits = np.unpackbits(valid.view(np.uint8), axis=1, bitorder="little")[:, :rows].astype(bool)
        for c, name in enumerate(names):
            column = [r.get(name.decode(), KeyError) for r in records]
            present = [v for v in column if v is not KeyError and v is not None]
            assert [t == 20 for t in tags[c].tolist()] == [v is KeyError for v in column], name
            kind = {type(v) for v in present}
            want = (capi.GET_BOOL if kind == {bool} else capi.GET_STRING if kind == {str} else capi.GET_INT64 if kind == {int} else capi.GET_OBJECT if kind == {dict} else
                    capi.GET_ARRAY if kind == {list} else capi.GET_DOUBLE if kind in ({float}, {int, float}) else 0)
            assert getters[c] == want, (name, kind)
            if not want:
                assert not values[c].any() and not valid[c].any() and not codes[c].any()
                continue
            assert bits[c].tolist() == [v is not KeyError and v is not None for v in column] == [x == 0 for x in codes[c].tolist()], name
            for r, v in enumerate(column):
                if v is KeyError or v is None:
                    continue
                if want == capi.GET_INT64:
                    assert int(values[c, r].view(np.int64)) == v
                elif want == capi.GET_BOOL:
                    assert int(values[c, r]) == int(v)
                elif want == capi.GET_DOUBLE:
                    assert float(values[c, r].view(np.float64)) == float(v)
                elif want == capi.GET_STRING:
                    assert int(values[c, r]) >> 32 == len(v.encode()) and values[c, r] == cells[c, r]
                else:
                    assert values[c, r] == cells[c, r]
    assert names.index(b"id") == 0 and getters[names.index(b"id")] == capi.GET_INT64 and getters[names.index(b"screen_name")] == capi.GET_STRING
    # listed keys: their order, an unknown one, one named twice; min_count; the folded classes
    users = [s["user"] for s in statuses]
    listed = [b"screen_name", b"nope", b"id", b"screen_name"]
    code, docs, rows, names, tags, cells, kinds, getters, values, valid, codes = pivot.records_many(parser, data, b"$.statuses[*].user", keys=listed)
    assert names == listed and getters == [capi.GET_STRING, 0, capi.GET_INT64, capi.GET_STRING] and (tags[1] == 20).all() and np.array_equal(cells[0], cells[3])
    assert values[2].view(np.int64).tolist() == [u["id"] for u in users]
    full = pivot.records_many(parser, data, b"$.statuses[*]", min_count=100)
    assert full[3] == [k.encode() for k in statuses[0] if all(k in s for s in statuses)]
    folded = pivot.records_many(parser, data, b"$.statuses[*].user", keys=[b"SCREEN_NAME", b"Id"], fold_case=True)
    assert folded[3] == [b"SCREEN_NAME", b"Id"] and np.array_equal(folded[5][0], cells[0]) and np.array_equal(folded[5][1], cells[2])
    assert (pivot.records_many(parser, data, b"$.statuses[*].user", keys=[b"SCREEN_NAME"])[4] == 20).all()
    # a stream of two documents of small records with ID / Id / id: one column when folded, named by the first spelling
    feed = b'[{"ID":1,"x":true},{"id":2}]\n[{"Id":3,"id":4},[5],{}]\n'
    code, docs, rows, names, tags, cells, kinds, getters, values, valid, codes = pivot.records_many(parser, feed, b"$[*]", fold_case=True)
    assert (code, docs, rows, names) == (0, 2, 5, [b"ID", b"x"]) and values[0].tolist() == [1, 2, 3, 0, 0] and tags[0].tolist() == [ord("l")] * 3 + [17, 20]
    assert getters == [capi.GET_INT64, capi.GET_BOOL] and values[1].tolist() == [1, 0, 0, 0, 0] and tags[1].tolist() == [ord("t"), 20, 20, 17, 20]
    assert pivot.records_many(parser, feed, b"$[*]")[3] == [b"ID", b"x", b"id", b"Id"]
    # no document, no rows
    assert pivot.records_many(parser, b"", b"$[*]")[:4] == (13, 0, 0, [])
    assert pivot.records_many(parser, data, b"$.nothing[*]")[1:4] == (1, 0, [])


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(parser):
    import torch
    c = pivot_cases.special()["a map that merges and drops"]
    base = check(parser, c)
    for name in ("values", "out", "offsets", "codes", "map"):
        assert call(parser, c, raw=True, **{name: 4 if name in ("values", "out") else 2}) == E_BADARG, name  # (nothing written: the poison check inside)
    ok = torch.zeros(256, dtype=torch.int64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    f = parser.L.sjgpu_pivot_fields_device
    # (ctx, offsets, status, rows, codes, value, tag, fields, map, groups, columns, value_out, tag_out, stream): one row, one field of code 0, one column
    good = [parser.h, ok.data_ptr(), ok.data_ptr() + 64, 1, ok.data_ptr() + 128, ok.data_ptr() + 192, ok.data_ptr() + 256, 0, ok.data_ptr() + 320, 1, 1, ok.data_ptr() + 384,
            ok.data_ptr() + 448, stream]
    for at in (0, 1, 2, 11, 12):
        args = list(good)
        args[at] = None
        assert f(*args) == E_BADARG, at
    some = list(good)
    some[7] = 1
    for at in (4, 5, 6):
        args = list(some)
        args[at] = None
        assert f(*args) == E_BADARG, at
    for at, value in ((7, 1 << 32), (9, 0), (3, 0xFFFFFFF1), (10, 0xFFFFFFF1)):
        args = list(some)
        args[at] = value
        assert f(*args) == E_BADARG, (at, value)
    args = list(some)
    args[3], args[10] = 0x10000, 0x10000  # 2^32 cells
    assert f(*args) == E_BADARG
    torch.cuda.synchronize()
    assert not ok.any().item()
    # rows == 0 or columns == 0: 0, nothing written; a null map with groups == 0 is no refusal
    for at in (3, 10):
        args = list(good)
        args[at] = 0
        assert f(*args) == 0
    torch.cuda.synchronize()
    assert not ok.any().item()
    args = list(good)
    args[8], args[9] = None, 0
    assert f(*args) == 0  # fields == 0 is served
    torch.cuda.synchronize()
    assert int(ok[48].item()) == 0 and int(ok[56].item()) & 0xFF == 20 and not ok[:48].any().item()
    ok.zero_()
    ok.view(torch.int32)[1] = 1  # offsets = [0, 1]: the row's one field
    assert f(*some) == 0  # code 0 through map[0] = 0 into the one cell: a zero word under tag 0
    torch.cuda.synchronize()
    assert int(ok[0].item()) == 1 << 32 and not ok[1:].any().item()
    # the neighbours of a call that was refused are what they were
    again = check(parser, c)
    assert np.array_equal(again[0], base[0]) and np.array_equal(again[1], base[1])
