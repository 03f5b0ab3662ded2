"""GPU tier (-m gpu): typed columns as JSON records -- sjgpu_write_records_device (k_write_count, k_write_fill; sjgpu_write.hip, include/sjgpu_write.h) and
writer.write_records / project_many -- against tests/write_records_model.py (pinned against tests/golden/write_records.json on the CPU tier), the fixture itself, and
the library's own parser: records that are parsed again give back the columns they came from.  Every output has exactly the contracted size inside a poisoned tensor
whose poison is checked after every call, the status row and the characters begin at odd addresses (the characters at each of the sixteen alignments where a test says
so), and every table is made three times: with capacity 0 and a null chars_dev, with one byte too few, then at the capacity the first call reported."""
import json
import os

import numpy as np
import pytest

import write_records_cases as cases
import write_records_model as model
from simdjson_amd import _paths, build, capi, writer
from test_gpu_query import Tapes, query

pytestmark = pytest.mark.gpu

CAP = 128 << 20
E_BADARG, E_OVERFLOW = -4, -5
GUARD = 65  # odd: with it the status row begins at an odd address
CHARS_GUARD = 64  # the characters begin at a 16-byte line + the skew a call asks for (by default 1)
P32, P8, P64 = 0x5A5A5A5A, 0x5A, 0x5A5A5A5A5A5A5A5A
EXAMPLES = os.path.join(_paths.REPO_ROOT, "tests", "golden", "jsonexamples")


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
        self.torch, self.arrays, self.keep, self.columns = torch, arrays, [], []
        for c in arrays["columns"]:
            d = {"key": c["key"], "kind": c["kind"], "chars_bytes": c["chars_bytes"]}
            for name, dtype in (("values", np.int64), ("valid", np.int64), ("offsets", np.int32)):
                if c[name] is not None:
                    host = np.ascontiguousarray(c[name]).view(dtype)
                    t = torch.from_numpy(np.concatenate([host, np.zeros(1, dtype)])).cuda()  # (never empty: an address to pass)
                    self.keep.append((t, host))
                    d[name] = t.data_ptr()
            if c["chars"] is not None:
                host = np.concatenate([np.full(1, P8, np.uint8), np.ascontiguousarray(c["chars"], np.uint8), np.full(16, P8, np.uint8)])
                t = torch.from_numpy(host).cuda()
                self.keep.append((t, host))
                d["chars"] = t.data_ptr() + 1
            self.columns.append(d)

    def unchanged(self):
        return all(np.array_equal(t.cpu().numpy()[: len(host)], host) for t, host in self.keep)


def call(p, D, flags, cap, null_chars=False, skew=1, offsets_skew=0, counts_skew=0, expect=None, columns=None, n=None):
    """one sjgpu_write_records_device over the device table D with outputs of exactly n + 1 words, n bytes, 4 counts and `cap` characters between poisoned guards
    -> (rc, bytes, offsets[n + 1], status[n], counts[4], chars: bytes); expect: the rc the caller counts on"""
    torch = D.torch
    n = D.arrays["n"] if n is None else n
    offsets = torch.full((n + 1 + 2 * GUARD,), P32, dtype=torch.int32, device="cuda")
    status = torch.full((n + 2 * GUARD,), P8, dtype=torch.uint8, device="cuda")
    counts = torch.full((4 + 2 * GUARD,), P64, dtype=torch.int64, device="cuda")
    chars = torch.full((cap + 2 * CHARS_GUARD + 16,), P8, dtype=torch.uint8, device="cuda")
    first = CHARS_GUARD + skew
    assert chars.data_ptr() % 16 == 0
    stream = torch.cuda.current_stream().cuda_stream
    rc, total = writer.write_records_device(p, D.columns if columns is None else columns, n, flags, offsets.data_ptr() + 4 * GUARD + offsets_skew, status.data_ptr() + GUARD,
                                            0 if null_chars else chars.data_ptr() + first, cap, counts.data_ptr() + 8 * GUARD + counts_skew, stream)
    torch.cuda.synchronize()
    if expect is not None:
        assert rc == expect, (rc, expect, p.last_error())
    nothing = rc == E_BADARG
    wrote_offsets, wrote_status, wrote_counts = (0, 0, 0) if nothing else (n + 1, n, 4)
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


def check(p, arrays, flags, skew=1, D=None):
    """the call over one table against the model -> (offsets, chars, status, counts)"""
    offsets, chars, status, counts = records(p, D or Device(arrays), flags, skew)
    want = model.records(arrays, flags)
    assert np.array_equal(status, want[2]), "status"
    assert np.array_equal(offsets, want[0]), "offsets"
    assert np.array_equal(counts, want[3]), (counts, want[3])
    if chars != want[1]:
        at = next(i for i, (a, b) in enumerate(zip(chars, want[1])) if a != b)
        raise AssertionError(f"chars differ at byte {at}: {chars[max(0, at - 40): at + 40]!r}, the model {want[1][max(0, at - 40): at + 40]!r}")
    return offsets, chars, status, counts


# ---- 1. the fixture ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("table", cases.fixture_tables(), ids=[t["name"] for t in cases.fixture_tables()])
def test_fixture_row_by_row(parser, table):
    fixture = cases.fixture()
    arrays = cases.arrays_of(table, tail_ones=True)
    D = Device(arrays)
    for flags in cases.ALL_FLAGS:
        offsets, chars, status, _ = check(parser, arrays, flags, skew=3 + flags, D=D)
        assert not status.any()
        cases.assert_rows_are_the_fixtures(fixture[table["name"]][flags], cases.split(offsets, chars), (table["name"], flags))


# ---- 2. the shapes ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", cases.ROW_COUNTS)
def test_rows_at_the_wave_and_workgroup_edges(parser, n):
    """six columns whose 256 rows take the direct road, two whose 256 rows take the staged one"""
    wide = check(parser, cases.arrays_of(cases.mixed_table(n), tail_ones=True), cases.NEWLINE)
    narrow = check(parser, cases.arrays_of(cases.narrow_table(n), tail_ones=True), cases.NEWLINE)
    check(parser, cases.arrays_of(cases.narrow_table(n)), cases.OMIT_NULLS, skew=9)
    if n >= cases.ROWS_PER_STEP:
        assert int(wide[0][cases.ROWS_PER_STEP]) > cases.WINDOW > int(narrow[0][cases.ROWS_PER_STEP])
    if n == 0:
        assert wide[0].tolist() == [0] and wide[3].tolist() == [0, 0, 0, 0]


def test_one_row_more_than_the_grid_takes_at_once(parser):
    """(grid cap x 256) + 1 rows: every workgroup goes round its loop, the first one a second time for one row"""
    n = cases.GRID_ROWS
    ids = (np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)).tolist()
    t = {"name": "grid", "n": n, "columns": [cases.column(b"id", cases.INT64, [None if r % 7 == 3 else v for r, v in enumerate(ids)]),
                                            cases.column(b"odd", cases.BOOL, [r & 1 for r in range(n)])]}
    offsets, chars, status, counts = check(parser, cases.arrays_of(t, tail_ones=True), cases.NEWLINE)
    assert counts.tolist() == [n, 0, len(range(3, n, 7)), 0] and chars.endswith(b',"odd":false}\n')


@pytest.mark.parametrize("K", cases.COLUMN_COUNTS)
def test_column_counts(parser, K):
    arrays = cases.arrays_of(cases.wide_table(K))
    D = Device(arrays)
    for flags in cases.ALL_FLAGS:
        offsets, chars, _, _ = check(parser, arrays, flags, D=D)
    if K == 0:
        assert chars == b"{}\n" * 70


def test_every_shape_of_validity(parser):
    n = 130
    t = cases.mixed_table(n)
    for shape in ("none", "zeros", "alternating", "tail_ones"):
        arrays = cases.arrays_of(t)
        for c in arrays["columns"]:
            if shape == "none":
                c["valid"] = None
            elif shape == "zeros":
                c["valid"] = np.zeros((n + 63) // 64, np.uint64)
            elif shape == "alternating":
                c["valid"] = np.full((n + 63) // 64, 0x5555555555555555, np.uint64)
            else:
                c["valid"] = cases.valid_words([True] * n, n, tail_ones=True)
        offsets, chars, status, counts = check(parser, arrays, 0)
        omitted = check(parser, arrays, cases.OMIT_NULLS | cases.NEWLINE)
        if shape == "zeros":
            assert omitted[1] == b"{}\n" * n and counts.tolist() == [n, 0, 6 * n, 0]


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_a_span_at_the_window(parser, delta):
    """the texts of one workgroup iteration take exactly the window, one byte less, one byte more; the rows behind them are another iteration's"""
    arrays = cases.arrays_of(cases.span_table(cases.WINDOW + delta, rows_after=5))
    D = Device(arrays)
    for skew in (0, 15):
        offsets, _, _, _ = check(parser, arrays, cases.NEWLINE, skew=skew, D=D)
    assert int(offsets[cases.ROWS_PER_STEP]) == cases.WINDOW + delta


def test_a_long_string_between_short_rows(parser):
    """one row longer than the window: its iteration takes the direct road, the iterations on either side of it the staged one"""
    n = 3 * cases.ROWS_PER_STEP + 7
    t = cases.narrow_table(n)
    t["columns"][1]["cells"][cases.ROWS_PER_STEP + 100] = (b'long "string" \\ with\nescapes ' * 2400)[: 65536]
    offsets, _, _, _ = check(parser, cases.arrays_of(t), cases.NEWLINE, skew=7)
    spans = [int(offsets[min(r + cases.ROWS_PER_STEP, n)]) - int(offsets[r]) for r in range(0, n, cases.ROWS_PER_STEP)]
    assert spans[1] > 65536 and all(s <= cases.WINDOW for s in spans[:1] + spans[2:])


def test_every_alignment_of_the_output(parser):
    arrays, short = cases.arrays_of(cases.narrow_table(300)), cases.arrays_of(cases.mixed_table(3))
    D, Ds = Device(arrays), Device(short)
    want, want_short = model.records(arrays, cases.NEWLINE), model.records(short, 0)
    for skew in range(16):
        rc, total, offsets, status, counts, chars = call(parser, D, cases.NEWLINE, len(want[1]), skew=skew, expect=0)
        assert chars == want[1] and np.array_equal(offsets, want[0]), skew
        rc, total, offsets, status, counts, chars = call(parser, Ds, 0, len(want_short[1]), skew=skew, expect=0)
        assert chars == want_short[1], skew


# ---- 3. status 19, doubles without a text, the refusals -------------------------------------------------------------------------------------------------------
def test_bad_offsets_are_status_19_and_a_validity_bit_of_0_hides_them(parser):
    arrays, bad = cases.bad_offsets()
    for flags in (0, cases.NEWLINE | cases.OMIT_NULLS):
        offsets, chars, status, counts = check(parser, arrays, flags)
        assert [r for r in range(arrays["n"]) if status[r]] == bad and set(status[bad].tolist()) == {19} and all(offsets[r] == offsets[r + 1] for r in bad)
    hidden, none = cases.bad_offsets(arrays_under_valid_bits=True)
    offsets, chars, status, counts = check(parser, hidden, 0)
    assert not status.any() and counts.tolist() == [hidden["n"], 0, 6, 0]


def test_every_row_refused(parser):
    t = {"name": "t", "n": 300, "columns": [cases.column(b"s", cases.STRING, [b"abc"] * 300)]}
    arrays = cases.arrays_of(t)
    arrays["columns"][0]["chars_bytes"] = 2
    D = Device(arrays)
    rc, total, offsets, status, counts, chars = call(parser, D, cases.NEWLINE, 0, null_chars=True, expect=0)
    assert total == 0 and (status == 19).all() and not offsets.any() and counts.tolist() == [0, 300, 0, 0]
    rc, total, offsets, status, counts, chars = call(parser, D, cases.NEWLINE, 64, expect=0)
    assert total == 0 and chars == b""


def test_doubles_without_a_text_under_both_policies(parser):
    arrays = cases.arrays_of(cases.nonfinite_table())
    D = Device(arrays)
    for flags in cases.ALL_FLAGS:
        offsets, chars, status, counts = check(parser, arrays, flags, D=D)
        assert counts.tolist() == [10, 0, 7, 6]
    assert b'{"r":4}\n' in chars and b"null" not in chars and b"NaN" not in chars


def test_refusals(parser):
    """each SJGPU_E_BADARG of the header, with every poison untouched (call() looks)"""
    t = {"name": "t", "n": 4, "columns": [cases.column(b"a", cases.INT64, [1, None, 3, 4]), cases.column(b"s", cases.STRING, [b"x"] * 4),
                                          cases.column(b"c", cases.STRING_CELLS, [b"y"] * 4)]}
    D = Device(cases.arrays_of(t))

    def changed(k, **fields):
        cols = [dict(c) for c in D.columns]
        cols[k].update(fields)
        return cols
    assert call(parser, D, 3, 256, expect=0)[5] == model.records(D.arrays, 3)[1] == b'{"a":1,"s":"x","c":"y"}\n{"s":"x","c":"y"}\n{"a":3,"s":"x","c":"y"}\n{"a":4,"s":"x","c":"y"}\n'
    for cols in (changed(0, kind=0), changed(0, kind=6), changed(0, kind=7), changed(0, kind=10), changed(0, values=0), changed(1, offsets=0), changed(1, chars=0),
                 changed(2, chars=0), changed(2, values=0), changed(0, key=b"k" * 1025), changed(1, chars_bytes=1 << 32), changed(0, values=D.columns[0]["values"] + 4),
                 changed(0, valid=D.columns[0]["valid"] + 4), changed(1, offsets=D.columns[1]["offsets"] + 2),
                 [dict(D.columns[0], key=b"k%d" % k) for k in range(65)], [dict(D.columns[0], key=bytes([0x61 + k]) * 1024) for k in range(8)]):
        call(parser, D, 0, 256, columns=cols, expect=E_BADARG)
    call(parser, D, 0, 256, columns=[dict(D.columns[0], key=bytes([0x61 + k]) * 1021) for k in range(8)], expect=E_OVERFLOW)  # 8 x 1 024 bytes of prefixes: the limit itself is served (and says what 256 bytes cannot hold)
    call(parser, D, 4, 256, expect=E_BADARG)
    call(parser, D, 0x80000000, 256, expect=E_BADARG)
    call(parser, D, 0, 256, offsets_skew=2, expect=E_BADARG)
    call(parser, D, 0, 256, counts_skew=4, expect=E_BADARG)
    call(parser, D, 0, 256, null_chars=True, expect=E_BADARG)  # a capacity without characters
    import torch
    out = torch.zeros(64, dtype=torch.int64, device="cuda")
    assert writer.write_records_device(parser, D.columns, 4, 0, out.data_ptr(), 0, out.data_ptr() + 128, 64, out.data_ptr() + 256)[0] == E_BADARG  # rows without a status
    assert writer.write_records_device(parser, D.columns, 4, 0, 0, out.data_ptr(), out.data_ptr() + 128, 64, out.data_ptr() + 256)[0] == E_BADARG
    assert writer.write_records_device(parser, D.columns, 4, 0, out.data_ptr(), out.data_ptr() + 64, out.data_ptr() + 128, 64, 0)[0] == E_BADARG
    assert writer.write_records_device(parser, D.columns, 0xFFFFFFF0, 0, out.data_ptr(), out.data_ptr() + 64, out.data_ptr() + 128, 64, out.data_ptr() + 256)[0] == E_BADARG
    assert not out.any()
    out.fill_(-1)
    assert writer.write_records_device(parser, [], 0, 0, out.data_ptr(), 0, 0, 0, out.data_ptr() + 256) == (0, 0)  # no rows: offsets[0] = 0 and four zero counts
    torch.cuda.synchronize()
    assert int(out.view(torch.int32)[0]) == 0 and int(out.view(torch.int32)[1]) == -1 and out[32:36].tolist() == [0, 0, 0, 0] and int(out[36]) == -1


# ---- 4. the round trips ------------------------------------------------------------------------------------------------------------------------------------
def test_records_parsed_again_give_back_the_columns(parser):
    """the chars of a NEWLINE call through sjgpu_parse_many, sjgpu_at_pointers_device and sjgpu_cast_cells_device: doubles bit for bit, -0.0 included, strings byte
    for byte, an invalid cell as an invalid cell"""
    import torch
    n = 300
    rng = np.random.default_rng(7)
    doubles = (rng.standard_normal(n) * 10.0 ** rng.integers(-300, 300, n)).view(np.uint64).tolist()
    doubles[0], doubles[1], doubles[2] = cases.bits_of(-0.0), cases.bits_of(5e-324), 0x7FEFFFFFFFFFFFFF
    alphabet = [bytes([c]) for c in range(0x80)] + ["é".encode(), "€".encode(), "😀".encode()]
    strings = [b"".join(alphabet[i] for i in rng.integers(0, len(alphabet), int(m))) for m in rng.integers(0, 40, n)]
    i64 = (rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + np.uint64(1)).tolist()
    u64 = [(1 << 63) + int(v) for v in rng.integers(0, 1 << 62, n)]

    def holes(cells, k):
        return [None if (r + k) % 11 == 0 else x for r, x in enumerate(cells)]
    t = {"name": "round", "n": n, "columns": [cases.column(b"i", cases.INT64, holes(i64, 0)), cases.column(b"u", cases.UINT64, holes(u64, 1)),
                                              cases.column(b"d", cases.DOUBLE, holes(doubles, 2)), cases.column(b"b", cases.BOOL, holes([r % 3 == 0 for r in range(n)], 3)),
                                              cases.column(b"s p/~", cases.STRING, holes(strings, 4)), cases.column(b"c", cases.STRING_CELLS, holes(strings[::-1], 5))]}
    offsets, chars, status, counts = check(parser, cases.arrays_of(t), cases.NEWLINE)
    code, docs, _, (tape, sbuf, table) = parser.parse_many(np.frombuffer(chars, np.uint8))
    assert (code, docs) == (0, n)
    T = Tapes(tape.copy(), sbuf.copy(), table.copy())
    tags, values = query(parser, T, [b"/i", b"/u", b"/d", b"/b", b"/s p~1~0", b"/c"])
    getters = [capi.GET_INT64, capi.GET_UINT64, capi.GET_DOUBLE, capi.GET_BOOL, capi.GET_STRING, capi.GET_STRING]
    K, W = 6, (n + 63) // 64
    d_values, d_tags = torch.from_numpy(values.view(np.int64)).cuda(), torch.from_numpy(tags).cuda()
    out, codes = torch.empty((K, n), dtype=torch.int64, device="cuda"), torch.empty((K, n), dtype=torch.uint8, device="cuda")
    valid, cast_counts = torch.empty((K, W), dtype=torch.int64, device="cuda"), torch.empty((K, 4), dtype=torch.int32, device="cuda")
    assert parser.cast_cells_device(d_values.data_ptr(), d_tags.data_ptr(), n, getters, out.data_ptr(), codes.data_ptr(), valid.data_ptr(), cast_counts.data_ptr(), T.stream) == 0
    torch.cuda.synchronize()
    out, valid = out.cpu().numpy().view(np.uint64), valid.cpu().numpy().view(np.uint64)
    for k, c in enumerate(t["columns"]):
        bits = [(int(valid[k][r >> 6]) >> (r & 63)) & 1 for r in range(n)]
        assert bits == [x is not None for x in c["cells"]], c["key"]
        for r, x in enumerate(c["cells"]):
            if x is None:
                continue
            w = int(out[k][r])
            if c["kind"] in (cases.STRING, cases.STRING_CELLS):
                assert T.sbuf[w & 0xFFFFFFFF: (w & 0xFFFFFFFF) + (w >> 32)].tobytes() == x, (c["key"], r)
            else:
                assert w == int(x), (c["key"], r, hex(w), hex(int(x)))


def test_project_many_over_an_ndjson_stream(parser):
    """NDJSON in, projected NDJSON out: record by record what the same projection gives on the host, after json.loads on both sides"""
    data = open(os.path.join(EXAMPLES, "amazon_cellphones.ndjson"), "rb").read()
    lines = [json.loads(ln) for ln in data.split(b"\n") if ln.strip()]
    fields = [(b"/0", capi.GET_STRING, b"asin"), (b"/5", capi.GET_DOUBLE, b"rating"), (b"/7", capi.GET_INT64, b"reviews"), (b"/8", capi.GET_STRING, b'price "as is"'),
              (b"", capi.GET_ARRAY, b"all"), (b"/9", capi.GET_BOOL, b"missing"), (b"/2", capi.GET_UINT64, b"title_as_number")]

    def host(line, omit):
        def at(i, types):
            v = line[i] if i < len(line) else None
            return v if isinstance(v, types) and not (isinstance(v, bool) and bool not in types) else None
        row = {"asin": at(0, (str,)), "rating": None if at(5, (int, float)) is None else float(at(5, (int, float))), "reviews": at(7, (int,)),
               'price "as is"': at(8, (str,)), "all": line, "missing": None, "title_as_number": None}
        return {k: v for k, v in row.items() if v is not None} if omit else row
    for omit in (False, True):
        offsets, chars, status, counts = writer.project_many(parser, data, fields, omit_nulls=omit)
        assert len(status) == len(lines) > 100 and not status.any() and int(offsets[-1]) == len(chars)
        got = [json.loads(x) for x in cases.split(offsets, chars.tobytes())]
        assert all(x.endswith(b"\n") for x in cases.split(offsets, chars.tobytes()))
        for r, (g, line) in enumerate(zip(got, lines)):
            assert g == host(line, omit), (r, g, host(line, omit))
            assert g.get("rating") is None or type(g["rating"]) is float  # (a rating written 3 in the source leaves as 3.0: the column is of doubles)
        assert int(counts[0]) == len(lines) and int(counts[2]) >= 2 * len(lines)


def test_write_records_takes_the_overflow_road_too(parser):
    """torch tensors in; a first guess of 32 bytes per cell that one long string exceeds: the second call fills"""
    import torch
    n = 50
    t = {"name": "t", "n": n, "columns": [cases.column(b"s", cases.STRING, [b"x" * 100] * n), cases.column(b"v", cases.INT64, [None if r % 2 else r for r in range(n)])]}
    arrays = cases.arrays_of(t)
    s, v = arrays["columns"]
    cols = [{"key": b"s", "kind": capi.COL_STRING, "offsets": torch.from_numpy(s["offsets"].view(np.int32)).cuda(), "chars": torch.from_numpy(s["chars"]).cuda()},
            {"key": b"v", "kind": capi.COL_INT64, "values": torch.from_numpy(v["values"].view(np.int64)).cuda(), "valid": torch.from_numpy(v["valid"].view(np.int64)).cuda()}]
    offsets, chars, status, counts = writer.write_records(parser, cols, n)
    want = model.records(arrays, cases.NEWLINE)
    assert chars.cpu().numpy().tobytes() == want[1] and np.array_equal(offsets.cpu().numpy().view(np.uint32), want[0]) and len(want[1]) > 32 * 2 * n
    assert counts.cpu().numpy().tolist() == want[3].tolist() and not status.cpu().numpy().any()
