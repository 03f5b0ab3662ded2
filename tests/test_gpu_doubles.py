"""GPU tier (-m gpu): doubles in bulk through the DEVICE compilation of simdjson_amd/csrc/sj_dtoa.h, sj_number.h and sj_number_in_string.h -- __umul64hi where the host
has unsigned __int128, __clzll, the __device__ copies of the power tables, what the gfx950 back end makes of the 128-bit products -- in every kernel family that
holds it: the five groups of json_text_cases.double_groups() (every power of two, the subnormal ones too, and every power of ten with their neighbours one ulp either
side, 4 000 random bit patterns, 768 doubles whose top byte is a tape tag) through every printer (sjgpu_json.hip and sjgpu_json_wide.hip, minified and indented;
sjgpu_write.hip, records and nested) and every parser (sjgpu_tape.hip, sjgpu_tape_many.hip, sjgpu_cast_strings.hip), byte for byte and bit for bit.  What is expected
comes from tests/double_bulk_cases.py and the digests of tests/golden/json_text.json (the real reference's texts), pinned together by tests/test_double_bulk_cases.py
on the CPU tier; nothing here has a tolerance, and a difference is a finding about the device compilation.  The calls go through the kits of the modules that test
each entry point: outputs at their exact capacity between poisoned guards.  Beside them, the doubles that look like tag words through the calls with one lane per
tape word (the wide texts, sjgpu_at_paths_wide_device) and through the calls that find their way by tags (sizes, fields)."""
import numpy as np
import pytest

import double_bulk_cases as B
import json_text_cases
import nested_write_cases as N
import write_records_cases as W
import test_gpu_cast_strings as cast_strings
import test_gpu_fields as fields
import test_gpu_json as narrow_json
import test_gpu_nested as nested
import test_gpu_paths as paths
import test_gpu_pretty as texts
import test_gpu_write as write
from simdjson_amd import build, capi
from test_gpu_json import parsed_tapes, roots_of
from test_gpu_paths_wide import Wide
from test_gpu_query import Tapes
from test_gpu_stream_tape import Resident, many_device

pytestmark = pytest.mark.gpu

CAP = 128 << 20
MINIFY, PRETTIFY = (texts.MINIFY_WIDE, texts.MINIFY_NARROW), (texts.WIDE, texts.NARROW)  # (wide, narrow): texts.both() runs both and wants the same bytes of them
SIGNED = [(name, False) for name in B.GROUPS] + [(name, True) for name in B.SIGNED_GROUPS]
SIGNED_IDS = [name + (", negated" if negated else "") for name, negated in SIGNED]
HOLE = 7  # every 7th cell invalid


@pytest.fixture(scope="module")
def parser():
    build.build_sjgpu()
    p = capi.DomParserImplementation(CAP)
    yield p
    p.close()


@pytest.fixture(scope="module")
def trees(parser):
    """name -> the tapes of the group's array document (sjgpu_parse), made once per group"""
    made = {}

    def of(name):
        if name not in made:
            made[name] = parsed_tapes(parser, [B.group(name).array])
        return made[name]
    return of


def digest_is_the_fixtures(name, got):
    kept = json_text_cases.fixture_double_groups()[name]
    assert len(got) == kept["count"] and json_text_cases.group_digest(got) == kept["sha256"], name


def first_difference(got, want):
    return next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))


def assert_bytes(got, want, what):
    if got != want:
        at = first_difference(got, want)
        raise AssertionError(f"{what}: {len(got)} bytes, expected {len(want)}; they differ at byte {at}: {got[max(0, at - 40): at + 40]!r}, expected {want[max(0, at - 40): at + 40]!r}")


def assert_bits(got, want, what):
    got, want = np.asarray(got, np.uint64), np.asarray(want, np.uint64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        at = int(np.flatnonzero(got != want)[0])
        raise AssertionError(f"{what}: {int((got != want).sum())} words differ, the first at {at}: {int(got[at]):016x}, expected {int(want[at]):016x}")


# ---- 1. the printers of sjgpu_json.hip and sjgpu_json_wide.hip ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", B.GROUPS)
def test_narrow_minify_of_loose_cells_has_the_fixtures_digest(parser, trees, name):
    g = B.group(name)
    offsets, chars, status = narrow_json.column(parser, trees(name), g.cells(), docs=0)
    assert not status.any()
    got = json_text_cases.split(offsets, chars)
    for r, (a, b) in enumerate(zip(got, g.texts)):
        assert a == b, (name, r, hex(g.bits[r]), a, b)
    digest_is_the_fixtures(name, got)


@pytest.mark.parametrize("name", B.GROUPS)
def test_all_four_text_calls_over_loose_cells(parser, trees, name):
    g = B.group(name)
    for entries, want in ((MINIFY, b"".join(g.texts)), (PRETTIFY, g.loose_pretty)):
        offsets, chars, status = texts.both(parser, trees(name), g.cells(), docs=0, entries=entries)
        assert not status.any() and len(offsets) == g.n + 1
        assert_bytes(chars, want, (name, entries[0].__name__))
        digest_is_the_fixtures(name, [t.rstrip(b"\n") for t in json_text_cases.split(offsets, chars)])


@pytest.mark.parametrize("name", B.GROUPS)
def test_all_four_text_calls_over_the_tree(parser, trees, name):
    g, T = B.group(name), trees(name)
    root = roots_of(parser, T)
    assert chr(root[0][0]) == "[" and int(root[1][0] >> np.uint64(32)) - int(root[1][0] & np.uint64(0xFFFFFFFF)) == 2 * g.n + 2
    for entries, want in ((MINIFY, g.array), (PRETTIFY, g.pretty)):
        offsets, chars, status = texts.both(parser, T, root, entries=entries)
        assert status.tolist() == [0] and offsets.tolist() == [0, len(want)]
        assert_bytes(chars, want, (name, entries[0].__name__))


@pytest.mark.parametrize("name", B.GROUPS)
def test_the_wide_text_calls_with_the_doubles_at_every_parity(parser, name):
    """one, two and three small integers in front of the doubles -- two tape words each, as the issue of this module asks -- and one, two and three literals, one word
    each: the `d` words and their payloads at both parities and at six distances from the edges of the lanes' shares"""
    g = B.group(name)
    prefixes = B.INTEGER_PREFIXES + B.LITERAL_PREFIXES
    T = parsed_tapes(parser, [B.array_document(g.texts, prefix) for prefix in prefixes])
    root = roots_of(parser, T)
    words = [int(v >> np.uint64(32)) - int(v & np.uint64(0xFFFFFFFF)) - 2 * g.n - 2 for v in root[1]]
    assert words == [2, 4, 6, 1, 2, 3]
    for entries, want in ((MINIFY, [B.array_document(g.texts, prefix) for prefix in prefixes]), (PRETTIFY, [B.pretty_array(g.texts, prefix) for prefix in prefixes])):
        offsets, chars, status = texts.both(parser, T, root, entries=entries)
        assert not status.any()
        for got, w, prefix in zip(json_text_cases.split(offsets, chars), want, prefixes):
            assert_bytes(got, w, (name, entries[0].__name__, prefix))


# ---- 2. the printers of sjgpu_write.hip --------------------------------------------------------------------------------------------------------------------------
def holes(cells):
    return [None if r % HOLE == 3 else x for r, x in enumerate(cells)]


@pytest.mark.parametrize("name", B.GROUPS)
def test_the_record_writer_over_a_column_of_doubles(parser, name):
    """sjgpu_write_records_device: the rows {"d":t}; with every 7th cell invalid that row is {"d":null} or {} and the others keep their texts"""
    g = B.group(name)
    t = {"name": name, "n": g.n, "columns": [W.column(b"d", W.DOUBLE, g.bits)]}
    offsets, chars, status, counts = write.records(parser, write.Device(W.arrays_of(t)), W.NEWLINE)
    assert not status.any() and counts.tolist() == [g.n, 0, 0, 0]
    assert_bytes(chars, b"".join(b'{"d":' + x + b"}\n" for x in g.texts), name)
    digest_is_the_fixtures(name, [row[len(b'{"d":'): -len(b"}\n")] for row in W.split(offsets, chars)])
    t = {"name": name, "n": g.n, "columns": [W.column(b"d", W.DOUBLE, holes(g.bits))]}
    D = write.Device(W.arrays_of(t, tail_ones=True))
    nulls = len(range(3, g.n, HOLE))
    for flags, hole in ((W.NEWLINE, b'{"d":null}\n'), (W.NEWLINE | W.OMIT_NULLS, b"{}\n")):
        offsets, chars, status, counts = write.records(parser, D, flags, skew=5)
        assert not status.any() and counts.tolist() == [g.n, 0, nulls, 0]
        assert_bytes(chars, b"".join(hole if r % HOLE == 3 else b'{"d":' + x + b"}\n" for r, x in enumerate(g.texts)), (name, flags))


@pytest.mark.parametrize("name", B.GROUPS)
def test_bare_rows_of_a_column_of_doubles(parser, name):
    """sjgpu_write_nested_device over the plain column with SJGPU_WRITE_BARE: the row is the text alone; an invalid cell is null, or a row of length 0"""
    g = B.group(name)
    t = {"name": name, "n": g.n, "fields": [N.column(b"", N.DOUBLE, g.bits)]}
    offsets, chars, status, counts = nested.records(parser, nested.Device(N.arrays_of(t)), N.BARE | N.NEWLINE)
    assert not status.any() and counts.tolist() == [g.n, 0, 0, 0, 0, 0]
    assert_bytes(chars, g.ndjson, name)
    digest_is_the_fixtures(name, [row[:-1] for row in N.split(offsets, chars)])
    t = {"name": name, "n": g.n, "fields": [N.column(b"", N.DOUBLE, holes(g.bits))]}
    D = nested.Device(N.arrays_of(t, tail_ones=True))
    nulls = len(range(3, g.n, HOLE))
    for flags, hole in ((N.BARE | N.NEWLINE, b"null\n"), (N.BARE | N.NEWLINE | N.OMIT_NULLS, b"")):
        offsets, chars, status, counts = nested.records(parser, D, flags, skew=9)
        assert not status.any() and counts.tolist() == [g.n, 0, nulls, 0, 0, 0]
        assert_bytes(chars, b"".join(hole if r % HOLE == 3 else x + b"\n" for r, x in enumerate(g.texts)), (name, flags))


@pytest.mark.parametrize("name", B.GROUPS)
def test_the_nested_writer_over_one_list_of_the_whole_group(parser, name):
    g = B.group(name)
    t = {"name": name, "n": 1, "fields": [N.list_field(b"d", N.DOUBLE, [g.bits])]}
    D = nested.Device(N.arrays_of(t, lead=1))
    offsets, chars, status, counts = nested.records(parser, D, N.BARE)
    assert status.tolist() == [0] and counts.tolist() == [1, 0, 0, 0, g.n, 0]
    assert_bytes(chars, g.array, name)
    offsets, chars, status, counts = nested.records(parser, D, N.NEWLINE, skew=2)
    assert_bytes(chars, b'{"d":' + g.array + b"}\n", name)


# ---- 3. the parsers --------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,negated", SIGNED, ids=SIGNED_IDS)
def test_parse_of_the_array_document(parser, name, negated):
    """sjgpu_parse (sjgpu_tape.hip): [, then `d` and the bits for each element, then ], word for word"""
    g = B.group(name, negated)
    err, tape, sbuf = parser.parse(g.array)
    assert err == 0 and len(sbuf) == 0
    assert_bits(tape, g.array_tape(), g.name)


@pytest.mark.parametrize("name,negated", SIGNED, ids=SIGNED_IDS)
def test_parse_many_of_the_ndjson_stream(parser, name, negated):
    """sjgpu_parse_many and sjgpu_stage2_many_device (sjgpu_tape_many.hip): one document per text, each a root scalar with the group's bits; the device call once with
    room to spare, once at exactly what it took"""
    g = B.group(name, negated)
    want = g.scalar_tapes()
    err, docs, _, (tape, sbuf, table) = parser.parse_many(g.ndjson)
    assert (err, docs, len(sbuf)) == (0, g.n, 0) and np.array_equal(table["tape_begin"], 4 * np.arange(g.n + 1, dtype=np.uint32))
    assert_bits(tape, want, g.name)
    res = Resident(parser, g.ndjson)
    for caps in ({}, {"tape_cap": 4 * g.n, "str_cap": 0, "doc_cap": g.n + 1}):
        code, docs, tape, sbuf, table = many_device(parser, res, **caps)
        assert (code, docs, len(sbuf)) == (0, g.n, 0) and np.array_equal(table["tape_begin"], 4 * np.arange(g.n + 1, dtype=np.uint32))
        assert_bits(tape, want, (g.name, caps))


@pytest.mark.parametrize("name,negated", SIGNED, ids=SIGNED_IDS)
def test_get_double_in_string_over_the_quoted_texts(parser, name, negated):
    """sjgpu_cast_string_cells_device (sjgpu_cast_strings.hip) over the cells of ["t0","t1",...]: the bits, all valid, every code 0"""
    g = B.group(name, negated)
    T = parsed_tapes(parser, [g.quoted])
    tags, values = fields.matches(parser, T, b"$[*]")
    assert len(tags) == g.n and (tags == 0x22).all()
    for getter in (capi.GETS_DOUBLE, capi.GETS_DOUBLE | capi.GETS_OR_NUMBER):
        value_out, code_out, valid, counts = cast_strings.call(parser, tags[None, :], values[None, :], T.sbuf.tobytes(), [getter])
        assert not code_out.any() and counts[0].tolist()[:5] == [g.n, 0, 0, 0, 0] and counts[0].tolist()[6:] == [0, 0]
        assert_bits(value_out[0], g.words, (g.name, getter))
        assert np.array_equal(np.unpackbits(valid[0].view(np.uint8), bitorder="little")[: 64 * len(valid[0])], np.arange(64 * len(valid[0])) < g.n)


# ---- 4. a payload word that looks like a tag word ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", B.LANE_PER_WORD_GROUPS)
def test_the_path_calls_tell_a_payload_from_a_tag(parser, trees, name):
    """$[*] over the array: exactly n matches, all `d`, the bits in order -- from the call with one lane per tape word and from the narrow one"""
    g, T = B.group(name), trees(name)
    wide, narrow = paths.column(Wide(parser), T, [b"$[*]"]), paths.column(parser, T, [b"$[*]"])
    for what, (status, offsets, tags, values) in (("wide", wide), ("narrow", narrow)):
        assert status.tolist() == [[0]] and offsets.tolist() == [0, g.n] and len(tags) == g.n and (tags == ord("d")).all(), what
        assert_bits(values, g.words, (name, what))
    assert all(np.array_equal(a, b) for a, b in zip(wide, narrow))


@pytest.mark.parametrize("name", B.LANE_PER_WORD_GROUPS)
def test_sizes_and_fields_tell_a_payload_from_a_tag(parser, trees, name):
    g, T = B.group(name), trees(name)
    size, code = fields.sizes(parser, T, roots_of(parser, T))
    assert g.n < 0xFFFFFF and size.tolist() == [g.n] and code.tolist() == [0]  # (the count field saturates at 0xFFFFFF: far from here)
    O = parsed_tapes(parser, [g.object])
    root = roots_of(parser, O)
    size, code = fields.sizes(parser, O, root)
    assert size.tolist() == [g.n] and code.tolist() == [0]
    status, offsets, key_tags, key_values, tags, values = fields.column(parser, O, root)
    assert status.tolist() == [0] and offsets.tolist() == [0, g.n] and (key_tags == 0x22).all() and (tags == ord("d")).all()
    assert_bits(values, g.words, name)
    assert fields.keys_of(O, key_values) == [b"k%d" % i for i in range(g.n)]


# ---- 5. across kernels -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", B.GROUPS)
def test_the_texts_of_the_wide_minify_parsed_again_as_a_stream(parser, trees, name):
    g = B.group(name)
    total = sum(len(t) for t in g.texts)
    rc, again, offsets, status, chars = texts.call(parser, trees(name), g.cells(), total, texts.MINIFY_WIDE, docs=0, expect=0)
    assert again == total and not status.any()
    stream = b"".join(t + b"\n" for t in json_text_cases.split(offsets, chars))
    err, docs, _, (tape, sbuf, table) = parser.parse_many(stream)
    assert (err, docs) == (0, g.n)
    assert_bits(tape, g.scalar_tapes(), name)
