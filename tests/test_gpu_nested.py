"""GPU tier (-m gpu): list columns and array rows as nested JSON -- sjgpu_write_nested_device (k_nested_count, k_nested_fill; sjgpu_write.hip,
include/sjgpu_nested.h) and writer.write_nested / project_rows_many -- against tests/nested_write_model.py (pinned against tests/golden/nested_write.json on the CPU
tier), the fixture itself, the plain writer, and Python's json.  The kit is that of tests/test_gpu_write.py: every output has exactly the contracted size inside a
poisoned tensor whose poison is checked after every call, the status row and the characters begin at odd addresses (the characters at each of the sixteen
alignments where a test says so), and every table is made three times: with capacity 0 and a null chars_dev, with one byte too few, then at the capacity the first
call reported."""
import json
import os

import numpy as np
import pytest

import nested_write_cases as cases
import nested_write_model as model
import write_records_cases as plain_cases
from simdjson_amd import _paths, build, capi, writer
from test_gpu_write import CAP, CHARS_GUARD, E_BADARG, E_OVERFLOW, EXAMPLES, GUARD, P8, P32, P64
from test_gpu_write import Device as PlainDevice
from test_gpu_write import call as plain_call

pytestmark = pytest.mark.gpu

NEWLINE, OMIT_NULLS, ARRAY_ROWS, BARE = cases.NEWLINE, cases.OMIT_NULLS, cases.ARRAY_ROWS, cases.BARE


@pytest.fixture(scope="module")
def parser():
    build.build_sjgpu()
    p = capi.DomParserImplementation(CAP)
    yield p
    p.close()


class Device:
    """a table's arrays in device memory at their exact sizes (the characters behind one byte, at an odd address), and the addresses the call takes"""

    def __init__(self, arrays):
        import torch
        self.torch, self.arrays, self.keep, self.fields = torch, arrays, [], []
        for f in arrays["fields"]:
            d = {"key": f["key"], "kind": f["kind"], "chars_bytes": f["chars_bytes"], "elements": f["elements"]}
            for name, dtype in (("values", np.int64), ("valid", np.int64), ("offsets", np.int32), ("list_offsets", np.int32), ("list_valid", np.int64)):
                if f[name] is not None:
                    host = np.ascontiguousarray(f[name]).view(dtype)
                    t = torch.from_numpy(np.concatenate([host, np.zeros(1, dtype)])).cuda()  # (never empty: an address to pass)
                    self.keep.append((t, host))
                    d[name] = t.data_ptr()
            if f["chars"] is not None:
                host = np.concatenate([np.full(1, P8, np.uint8), np.ascontiguousarray(f["chars"], np.uint8), np.full(16, P8, np.uint8)])
                t = torch.from_numpy(host).cuda()
                self.keep.append((t, host))
                d["chars"] = t.data_ptr() + 1
            self.fields.append(d)

    def unchanged(self):
        return all(np.array_equal(t.cpu().numpy()[: len(host)], host) for t, host in self.keep)


def call(p, D, flags, cap, null_chars=False, skew=1, offsets_skew=0, counts_skew=0, expect=None, fields=None, n=None):
    """one sjgpu_write_nested_device over the device table D with outputs of exactly n + 1 words, n bytes, 6 counts and `cap` characters between poisoned guards
    -> (rc, bytes, offsets[n + 1], status[n], counts[6], chars: bytes); expect: the rc the caller counts on"""
    torch = D.torch
    n = D.arrays["n"] if n is None else n
    offsets = torch.full((n + 1 + 2 * GUARD,), P32, dtype=torch.int32, device="cuda")
    status = torch.full((n + 2 * GUARD,), P8, dtype=torch.uint8, device="cuda")
    counts = torch.full((6 + 2 * GUARD,), P64, dtype=torch.int64, device="cuda")
    chars = torch.full((cap + 2 * CHARS_GUARD + 16,), P8, dtype=torch.uint8, device="cuda")
    first = CHARS_GUARD + skew
    assert chars.data_ptr() % 16 == 0
    stream = torch.cuda.current_stream().cuda_stream
    rc, total = writer.write_nested_device(p, D.fields if fields is None else fields, n, flags, offsets.data_ptr() + 4 * GUARD + offsets_skew, status.data_ptr() + GUARD,
                                           0 if null_chars else chars.data_ptr() + first, cap, counts.data_ptr() + 8 * GUARD + counts_skew, stream)
    torch.cuda.synchronize()
    if expect is not None:
        assert rc == expect, (rc, expect, p.last_error())
    nothing = rc == E_BADARG
    wrote_offsets, wrote_status, wrote_counts = (0, 0, 0) if nothing else (n + 1, n, 6)
    wrote = total if rc == 0 else 0
    oh, sh, ch, kh = offsets.cpu().numpy().view(np.uint32), status.cpu().numpy(), chars.cpu().numpy(), counts.cpu().numpy().view(np.uint64)
    assert (oh[:GUARD] == P32).all() and (oh[GUARD + wrote_offsets:] == P32).all(), "offsets poison"
    assert (sh[:GUARD] == P8).all() and (sh[GUARD + wrote_status:] == P8).all(), "status poison"
    assert not (sh[GUARD: GUARD + wrote_status] == P8).any(), "a status was not written"
    assert (kh[:GUARD] == P64).all() and (kh[GUARD + wrote_counts:] == P64).all(), "counts poison"
    assert not (kh[GUARD: GUARD + wrote_counts] == P64).any(), "a count was not written"
    assert (ch[:first] == P8).all() and (ch[first + wrote:] == P8).all(), "chars poison: a byte outside [0, bytes), or characters written although they do not fit"
    assert D.unchanged(), "an input was written"
    if not nothing:
        assert int(oh[GUARD]) == 0 and int(oh[GUARD + n]) == total, "the offsets end at the total"
    return (rc, total, oh[GUARD: GUARD + wrote_offsets].copy(), sh[GUARD: GUARD + wrote_status].copy(), kh[GUARD: GUARD + wrote_counts].copy(),
            ch[first: first + wrote].tobytes())


def records(p, D, flags, skew=1):
    """the texts at their EXACT capacity: a call with room for nothing and a null chars_dev says what is needed and leaves offsets, status and counts complete; one with
    one byte too few writes nothing either; the third fills -> (offsets, chars, status, counts)"""
    rc, total, offsets0, status0, counts0, _ = call(p, D, flags, 0, null_chars=True)
    if total == 0:
        assert rc == 0
        return offsets0, b"", status0, counts0
    assert rc == E_OVERFLOW
    rc, again, offsets1, status1, counts1, _ = call(p, D, flags, total - 1, skew=skew, expect=E_OVERFLOW)
    assert again == total and np.array_equal(offsets1, offsets0) and np.array_equal(status1, status0) and np.array_equal(counts1, counts0)
    rc, again, offsets, status, counts, chars = call(p, D, flags, total, skew=skew, expect=0)
    assert again == total == len(chars) and np.array_equal(offsets, offsets0) and np.array_equal(status, status0) and np.array_equal(counts, counts0)
    return offsets, chars, status, counts


def same(got, want):
    offsets, chars, status, counts = got
    assert np.array_equal(status, want[2]), "status"
    assert np.array_equal(offsets, want[0]), "offsets"
    assert np.array_equal(counts, want[3]), (counts, want[3])
    if chars != want[1]:
        at = next(i for i, (a, b) in enumerate(zip(chars, want[1])) if a != b)
        raise AssertionError(f"chars differ at byte {at}: {chars[max(0, at - 40): at + 40]!r}, the model {want[1][max(0, at - 40): at + 40]!r}")


def check(p, arrays, flags, skew=1, D=None, want=None):
    """the call over one table against the model -> (offsets, chars, status, counts)"""
    got = records(p, D or Device(arrays), flags, skew)
    same(got, want or model.records(arrays, flags))
    return got


# ---- 1. the fixture ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("table", cases.fixture_tables(), ids=[t["name"] for t in cases.fixture_tables()])
def test_fixture_row_by_row(parser, table):
    """every legal combination of the flags, row by row the reference's text; the list offsets begin at a base of 5 and end exactly at `elements`"""
    fixture = cases.fixture()
    arrays = cases.arrays_of(table, tail_ones=True, lead=5)
    assert all(f["list_offsets"] is None or (int(f["list_offsets"][0]) == 5 and int(f["list_offsets"][-1]) == f["elements"]) for f in arrays["fields"])
    D = Device(arrays)
    for flags in cases.legal_flags(len(table["fields"])):
        offsets, chars, status, _ = check(parser, arrays, flags, skew=3 + flags, D=D)
        assert not status.any()
        cases.assert_rows_are_the_fixtures(fixture[table["name"]][flags], cases.split(offsets, chars), (table["name"], flags))


# ---- 2. the shapes ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", plain_cases.ROW_COUNTS)
def test_rows_at_the_wave_and_workgroup_edges(parser, n):
    """nine fields, lists among them, whose 256 rows do not fit the window; two whose 256 rows fit it at once; array rows under NEWLINE"""
    arrays = cases.arrays_of(cases.mixed_table(n), tail_ones=True, lead=1)
    D = Device(arrays)
    wide = check(parser, arrays, NEWLINE, D=D)
    check(parser, arrays, ARRAY_ROWS | NEWLINE, skew=4, D=D)
    narrow = check(parser, cases.arrays_of(cases.narrow_table(n), tail_ones=True), NEWLINE)
    check(parser, cases.arrays_of(cases.narrow_table(n)), OMIT_NULLS, skew=9)
    if n >= cases.ROWS_PER_STEP:
        assert cases.group_rows(wide[0], 0) in (128, 64) and cases.group_rows(narrow[0], 0) == 256
    if n == 0:
        assert wide[0].tolist() == [0] and wide[3].tolist() == [0] * 6


def test_one_row_more_than_the_grid_takes_at_once(parser):
    """(grid cap x 256) + 1 rows of one list of at most two int64: every workgroup goes round its loop -- the windows' turn carries over --, the first one a second
    time for one row"""
    n = cases.GRID_ROWS
    values = (np.arange(2 * n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15))
    lengths = (np.arange(n) * 7 // 3) % 3
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint32)
    m = int(offsets[-1])
    valid = np.full((m + 63) // 64, 0xFFFFFFFFFFFFFFF7, np.uint64)  # element 3 of every 64 is null
    arrays = {"n": n, "fields": [{"key": b"v", "kind": cases.INT64, "values": values[:m], "valid": valid, "offsets": None, "chars": None, "chars_bytes": 0,
                                  "list_offsets": offsets, "list_valid": None, "elements": m}]}
    offsets, chars, status, counts = check(parser, arrays, NEWLINE)
    assert counts.tolist() == [n, 0, 0, 0, m, len(range(3, m, 64))] and chars.startswith(b'{"v":[]}\n{"v":[0,-7046029254386353131]}\n')


@pytest.mark.parametrize("K", plain_cases.COLUMN_COUNTS)
def test_field_counts(parser, K):
    arrays = cases.arrays_of(cases.wide_table(K), lead=3)
    D = Device(arrays)
    for flags in cases.legal_flags(K):
        offsets, chars, _, _ = check(parser, arrays, flags, D=D)
        if K == 0:
            assert chars == {0: b"{}", 1: b"{}", 2: b"{}\n", 3: b"{}\n", 4: b"[]", 6: b"[]\n"}[flags] * 70


def test_the_validity_words_edge_inside_one_list_and_garbage_under_an_invalid_list(parser):
    """elements 63, 64 and 65 inside one list, on both sides of a validity word, at three bases; the offset between two invalid lists is 0xFFFFFFF0: status 0"""
    t = cases._lengths()
    for lead in (0, 1, 2):
        arrays = cases.arrays_of(t, lead=lead)
        assert all(int(f["list_offsets"][7]) == cases.GARBAGE for f in arrays["fields"])
        offsets, chars, status, counts = check(parser, arrays, NEWLINE | OMIT_NULLS)
        assert not status.any() and counts.tolist()[2] == 2 * 4


# ---- 3. status 19, doubles without a text, the refusals -------------------------------------------------------------------------------------------------------
def test_bad_lists_are_status_19_and_a_validity_bit_of_0_hides_them(parser):
    arrays, bad = cases.bad_lists()
    D = Device(arrays)
    for flags in (0, NEWLINE | OMIT_NULLS, ARRAY_ROWS):
        offsets, chars, status, counts = check(parser, arrays, flags, D=D)
        assert [r for r in range(arrays["n"]) if status[r]] == bad and set(status[bad].tolist()) == {19} and all(offsets[r] == offsets[r + 1] for r in bad)
        served = [x for r, x in enumerate(cases.split(offsets, chars)) if r not in bad]
        assert all(x[:1] in (b"{", b"[") and x.rstrip(b"\n")[-1:] in (b"}", b"]") for x in served)  # the neighbours are intact
    offsets, chars, status, counts = check(parser, cases.hidden_bad_lists(), 0)
    assert not status.any() and counts.tolist()[:3] == [10, 0, 2]


def test_doubles_without_a_text_are_null_elements_under_omit_nulls_too(parser):
    inf, nan = 0x7FF0000000000000, 0x7FF8000000000ABC
    t = {"name": "t", "n": 3, "fields": [cases.list_field(b"d", cases.DOUBLE, [[cases.bits_of(1.5), inf, None], [nan], []]), cases.column(b"p", cases.DOUBLE, [nan, 0, inf])]}
    arrays = cases.arrays_of(t)
    D = Device(arrays)
    assert check(parser, arrays, 0, D=D)[1] == b'{"d":[1.5,null,null],"p":null}{"d":[null],"p":0.0}{"d":[],"p":null}'
    offsets, chars, status, counts = check(parser, arrays, OMIT_NULLS, D=D)
    assert chars == b'{"d":[1.5,null,null]}{"d":[null],"p":0.0}{"d":[]}' and counts.tolist() == [3, 0, 2, 4, 4, 3]


def test_refusals(parser):
    """each new SJGPU_E_BADARG of the header and the old ones per field, with every poison untouched (call() looks)"""
    t = {"name": "t", "n": 4, "fields": [cases.list_field(b"a", cases.INT64, [[1], None, [3, None], []]), cases.list_field(b"s", cases.STRING, [[b"x"]] * 4),
                                         cases.list_field(b"c", cases.STRING_CELLS, [[b"y"]] * 4), cases.column(b"p", cases.INT64, [1, 2, None, 4])]}
    arrays = cases.arrays_of(t)
    D = Device(arrays)

    def changed(k, **fields):
        out = [dict(f) for f in D.fields]
        out[k].update(fields)
        return out
    want = model.records(arrays, NEWLINE)
    assert call(parser, D, NEWLINE, 256, expect=0)[5] == want[1] == b'{"a":[1],"s":["x"],"c":["y"],"p":1}\n{"a":null,"s":["x"],"c":["y"],"p":2}\n{"a":[3,null],"s":["x"],"c":["y"],"p":null}\n{"a":[],"s":["x"],"c":["y"],"p":4}\n'
    one = D.fields[:1]
    for fields, flags in [(changed(0, kind=0), 0), (changed(0, kind=6), 0), (changed(0, kind=7), 0), (changed(0, kind=10), 0), (changed(0, values=0), 0), (changed(1, offsets=0), 0),
                          (changed(1, chars=0), 0), (changed(2, chars=0), 0), (changed(2, values=0), 0), (changed(3, values=0), 0), (changed(0, key=b"k" * 1025), 0),
                          (changed(1, chars_bytes=1 << 32), 0), (changed(0, values=D.fields[0]["values"] + 4), 0), (changed(0, valid=D.fields[0]["valid"] + 4), 0),
                          (changed(1, offsets=D.fields[1]["offsets"] + 2), 0), (changed(0, list_offsets=D.fields[0]["list_offsets"] + 2), 0),
                          (changed(0, list_valid=D.fields[0]["list_valid"] + 4), 0), (changed(0, elements=0xFFFFFFF0), 0), (changed(0, elements=1 << 40), 0),
                          ([dict(D.fields[0], key=b"k%d" % k) for k in range(65)], 0), ([dict(D.fields[0], key=bytes([0x61 + k]) * 1024) for k in range(8)], 0),
                          (D.fields, 16), (D.fields, 0x80000000), (D.fields, ARRAY_ROWS | OMIT_NULLS), (D.fields, ARRAY_ROWS | BARE), (one, ARRAY_ROWS | BARE),
                          (D.fields, BARE), ([], BARE), (D.fields[:2], BARE | NEWLINE)]:
        call(parser, D, flags, 256, fields=fields, expect=E_BADARG)
    # the plain entry point keeps refusing the new flags
    PD = PlainDevice(plain_cases.arrays_of(plain_cases.mixed_table(3)))
    for flags in (ARRAY_ROWS, BARE, ARRAY_ROWS | NEWLINE):
        plain_call(parser, PD, flags, 256, expect=E_BADARG)
    # not refused: keys nobody looks at (too long, or null), the null element arrays of a field without elements, elements + 1 == 0xFFFFFFF0 with lists that stay below
    call(parser, D, ARRAY_ROWS, 256, fields=changed(0, key=b"k" * 5000), expect=0)
    call(parser, D, ARRAY_ROWS, 256, fields=[dict(f, key=b"") for f in D.fields], expect=0)
    assert call(parser, D, 0, 256, fields=changed(0, elements=0xFFFFFFEF), expect=0)[5] == want[1].replace(b"\n", b"")
    empty = cases.arrays_of({"name": "t", "n": 3, "fields": [cases.list_field(b"e", cases.STRING, [[], None, []])]})
    for name in ("values", "valid", "offsets", "chars"):
        empty["fields"][0][name] = None
    assert check(parser, empty, BARE | OMIT_NULLS | NEWLINE)[1] == b"[]\n[]\n"
    call(parser, D, 0, 256, offsets_skew=2, expect=E_BADARG)
    call(parser, D, 0, 256, counts_skew=4, expect=E_BADARG)
    call(parser, D, 0, 256, null_chars=True, expect=E_BADARG)  # a capacity without characters
    import torch
    out = torch.zeros(64, dtype=torch.int64, device="cuda")
    assert writer.write_nested_device(parser, D.fields, 4, 0, out.data_ptr(), 0, out.data_ptr() + 128, 64, out.data_ptr() + 256)[0] == E_BADARG  # rows without a status
    assert writer.write_nested_device(parser, D.fields, 4, 0, 0, out.data_ptr(), out.data_ptr() + 128, 64, out.data_ptr() + 256)[0] == E_BADARG
    assert writer.write_nested_device(parser, D.fields, 4, 0, out.data_ptr(), out.data_ptr() + 64, out.data_ptr() + 128, 64, 0)[0] == E_BADARG
    assert writer.write_nested_device(parser, D.fields, 0xFFFFFFF0, 0, out.data_ptr(), out.data_ptr() + 64, out.data_ptr() + 128, 64, out.data_ptr() + 256)[0] == E_BADARG
    assert not out.any()
    out.fill_(-1)
    assert writer.write_nested_device(parser, [], 0, ARRAY_ROWS, out.data_ptr(), 0, 0, 0, out.data_ptr() + 256) == (0, 0)  # no rows: offsets[0] = 0 and six zero counts
    torch.cuda.synchronize()
    assert int(out.view(torch.int32)[0]) == 0 and int(out.view(torch.int32)[1]) == -1 and out[32:38].tolist() == [0] * 6 and int(out[38]) == -1


# ---- 4. the fill's grouping -------------------------------------------------------------------------------------------------------------------------------------
def test_the_window_is_the_one_the_cases_stand_on():
    from simdjson_amd import capi as c
    assert (cases.WINDOW, cases.ROWS_PER_STEP, cases.GRID_ROWS) == (28 << 10, 256, 512 * 256 + 1)
    src = open(os.path.join(_paths.PKG_DIR, "csrc", "sjgpu_write.hip")).read()
    assert "constexpr u32 WRITE_WINDOW = 28u << 10;" in src and "constexpr u32 WRITE_MAX_WORKGROUPS = 512;" in src and c.COL_JSON == cases.JSON


@pytest.mark.parametrize("name", list(cases.grouping_cases()))
def test_the_edges_of_the_grouping(parser, name):
    """a span of 256 rows, of 128, of 64 and of 32 at the window and one byte beyond it, at the first and the last alignment of the output (the product stages the
    first and writes the others directly; a build with -DSJGPU_NESTED_SPLIT stages them in groups -- the cases are the edges of both)"""
    t, group = cases.grouping_cases()[name]
    arrays = cases.arrays_of(t)
    D = Device(arrays)
    want = model.records(arrays, NEWLINE)
    assert cases.group_rows(want[0], 0) == group
    for skew in (0, 15):
        check(parser, arrays, NEWLINE, skew=skew, D=D, want=want)


def test_one_row_of_64_kib_between_staged_neighbours(parser):
    t = cases.long_row_table(65536)
    offsets, _, _, _ = check(parser, cases.arrays_of(t), NEWLINE, skew=7)
    assert [cases.group_rows(offsets, r) for r in range(0, t["n"], cases.ROWS_PER_STEP)] == [256, 0, 256, 256]
    assert int(offsets[cases.ROWS_PER_STEP + 101]) - int(offsets[cases.ROWS_PER_STEP + 100]) > 65536


def test_every_alignment_of_the_output_on_a_split_case(parser):
    arrays = cases.arrays_of(cases.grouping_cases()["64-row groups fit, a 128-row group does not"][0])
    D = Device(arrays)
    want = model.records(arrays, NEWLINE)
    for skew in range(16):
        rc, total, offsets, status, counts, chars = call(parser, D, NEWLINE, len(want[1]), skew=skew, expect=0)
        assert chars == want[1] and np.array_equal(offsets, want[0]), skew


# ---- 5. the row shapes, parity, composition -----------------------------------------------------------------------------------------------------------------------
def test_bare_rows_under_omit_nulls_leave_empty_rows_between_full_ones(parser):
    arrays = cases.arrays_of(cases._bare_strings())
    D = Device(arrays)
    assert check(parser, arrays, BARE | NEWLINE, D=D)[1] == b'["a","\\"",null]\nnull\n[]\nnull\nnull\n["zzzzzzzzzzzzzzzzzzzz"]\n'
    offsets, chars, status, counts = check(parser, arrays, BARE | OMIT_NULLS | NEWLINE, D=D)
    assert np.diff(offsets.astype(np.int64)).tolist() == [16, 0, 3, 0, 0, 25] and not status.any() and counts.tolist() == [6, 0, 3, 0, 4, 1]


def test_parity_with_the_plain_writer(parser):
    """a table with no list field and no new flag: the bytes, offsets, statuses and counts of sjgpu_write_records_device over the same columns"""
    for t in (plain_cases.mixed_table(257), plain_cases.narrow_table(513), plain_cases._every_kind(), plain_cases._keys()):
        arrays = cases.arrays_of({"name": t["name"], "n": t["n"], "fields": t["columns"]}, tail_ones=True)
        D, PD = Device(arrays), PlainDevice(cases.as_plain_arrays(arrays))
        for flags in plain_cases.ALL_FLAGS:
            offsets, chars, status, counts = records(parser, D, flags)
            rc, total, poffsets, pstatus, pcounts, pchars = plain_call(parser, PD, flags, len(chars), expect=0)
            assert chars == pchars and np.array_equal(offsets, poffsets) and np.array_equal(status, pstatus) and counts.tolist() == pcounts.tolist() + [0, 0]


def test_list_of_lists_through_a_bare_call_fed_back_as_json_elements(parser):
    """list<list<int64>>: the inner lists written bare under OMIT_NULLS -- an invalid one leaves an empty row --, those rows taken as JSON elements of the outer lists"""
    import torch
    inner = [[1, 2], [], None, [3], [None, -4 % (1 << 64)], None, [5, 6, 7]]
    outer_offsets = np.array([0, 3, 3, 7], np.uint32)  # three outer rows: inner 0 .. 3, none, inner 3 .. 7
    t = {"name": "inner", "n": len(inner), "fields": [cases.list_field(b"", cases.INT64, inner)]}
    offsets, chars, status, counts = check(parser, cases.arrays_of(t), BARE | OMIT_NULLS)
    d_offsets, d_chars = torch.from_numpy(offsets.view(np.int32)).cuda(), torch.from_numpy(np.frombuffer(chars, np.uint8).copy()).cuda()
    fields = [{"key": b"ll", "kind": capi.COL_JSON, "offsets": d_offsets, "chars": d_chars, "list_offsets": torch.from_numpy(outer_offsets.view(np.int32)).cuda(),
               "elements": len(inner)}]
    o, c, s, k = writer.write_nested(parser, fields, 3)
    lines = c.cpu().numpy().tobytes().split(b"\n")
    assert [json.loads(x) for x in lines[:-1]] == [{"ll": [[1, 2], [], None]}, {"ll": []}, {"ll": [[3], [None, -4], None, [5, 6, 7]]}]
    assert k.cpu().numpy().tolist() == [3, 0, 0, 0, 7, 2] and not s.cpu().numpy().any()


def test_list_of_structs_through_the_plain_writer_fed_in_as_json_elements(parser):
    """list<struct>: sjgpu_write_records_device over the ELEMENT rows, its texts taken as the JSON elements of a list field beside a plain one"""
    import torch
    m = 9
    names = [b"n%d" % e for e in range(m)]
    child = plain_cases.arrays_of({"name": "child", "n": m, "columns": [plain_cases.column(b"name", plain_cases.STRING, names),
                                                                        plain_cases.column(b"x", plain_cases.INT64, [None if e == 4 else e * e for e in range(m)])]})
    s, x = child["columns"]
    cols = [{"key": b"name", "kind": capi.COL_STRING, "offsets": torch.from_numpy(s["offsets"].view(np.int32)).cuda(), "chars": torch.from_numpy(s["chars"]).cuda()},
            {"key": b"x", "kind": capi.COL_INT64, "values": torch.from_numpy(x["values"].view(np.int64)).cuda(), "valid": torch.from_numpy(x["valid"].view(np.int64)).cuda()}]
    eo, ec, es, ek = writer.write_records(parser, cols, m, newline=False)
    list_offsets = torch.tensor([0, 2, 2, 9], dtype=torch.int32, device="cuda")
    ids = torch.tensor([10, 11, 12], dtype=torch.int64, device="cuda")
    fields = [{"key": b"id", "kind": capi.COL_INT64, "values": ids}, {"key": b"items", "kind": capi.COL_JSON, "offsets": eo, "chars": ec, "list_offsets": list_offsets, "elements": m}]
    o, c, st, k = writer.write_nested(parser, fields, 3, first_cap=8)  # (a first guess that is too small: the second call fills)
    got = [json.loads(line) for line in c.cpu().numpy().tobytes().split(b"\n")[:-1]]
    struct = [{"name": "n%d" % e, "x": None if e == 4 else e * e} for e in range(m)]
    assert got == [{"id": 10, "items": struct[0:2]}, {"id": 11, "items": []}, {"id": 12, "items": struct[2:9]}] and k.cpu().numpy().tolist() == [3, 0, 0, 0, 9, 0]


def test_project_rows_many_over_twitter(parser):
    """rows $.statuses[*]; the id, the hashtag texts as list<string> and the mention ids as list<int64>: line by line what Python's json gives for the same projection"""
    data = open(os.path.join(EXAMPLES, "twitter.json"), "rb").read()
    statuses = json.loads(data)["statuses"]
    fields = [(b"/id", capi.GET_INT64, b"id"), (b"$.entities.hashtags[*].text", capi.GET_STRING, b"hashtags"), (b"$.entities.user_mentions[*].id", capi.GET_INT64, b"mentions"),
              (b"/user/screen_name", capi.GET_STRING, b"user"), (b"$.entities.urls[*]", capi.GET_OBJECT, b"urls"), (b"$.entities.hashtags[*].text", capi.GET_INT64, b"not_numbers"),
              (b"/retweeted_status/id", capi.GET_UINT64, b"retweet_of")]

    def host(s, omit):
        row = {"id": s["id"], "hashtags": [h["text"] for h in s["entities"]["hashtags"]], "mentions": [m["id"] for m in s["entities"]["user_mentions"]],
               "user": s["user"]["screen_name"], "urls": s["entities"]["urls"], "not_numbers": [None] * len(s["entities"]["hashtags"]),
               "retweet_of": s.get("retweeted_status", {}).get("id")}
        return {k: v for k, v in row.items() if v is not None} if omit else row
    for omit in (False, True):
        offsets, chars, status, counts = writer.project_rows_many(parser, data, b"$.statuses[*]", fields, omit_nulls=omit)
        lines = cases.split(offsets, chars.tobytes())
        assert len(lines) == len(statuses) == 100 and not status.any() and int(offsets[-1]) == len(chars) and all(x.endswith(b"\n") for x in lines)
        for r, (line, s) in enumerate(zip(lines, statuses)):
            assert json.loads(line) == host(s, omit), (r, line, host(s, omit))
        hashtags = sum(len(s["entities"]["hashtags"]) for s in statuses)
        assert counts.tolist() == [100, 0, sum("retweeted_status" not in s for s in statuses), 0,
                                   2 * hashtags + sum(len(s["entities"]["user_mentions"]) + len(s["entities"]["urls"]) for s in statuses), hashtags]
    # the issue's three fields alone, and a stream of two documents
    three = fields[:3]
    offsets, chars, status, counts = writer.project_rows_many(parser, data + b"\n" + data, b"$.statuses[*]", three)
    got = [json.loads(x) for x in cases.split(offsets, chars.tobytes())]
    assert got == [{k: host(s, False)[k] for k in ("id", "hashtags", "mentions")} for s in statuses] * 2
    offsets, chars, status, counts = writer.project_rows_many(parser, data, b"$.nothing[*]", three)
    assert offsets.tolist() == [0] and len(chars) == 0 and counts.tolist() == [0] * 6
    with pytest.raises(ValueError):
        writer.project_rows_many(parser, data, b"$.statuses[*]", [(b"$.id", capi.GET_INT64, b"id")])
