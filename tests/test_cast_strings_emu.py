"""CPU tier: numbers held in strings -- the gfx950 kernel source sjgpu_cast_strings.hip, compiled as C++ against tests/host/emu -- run what
sjgpu_cast_string_cells_device enqueues (tests/host/test_cast_strings_emu.cpp) and are compared bit for bit with tests/in_string_model.py: the fixture's contents
under all six getter bytes, random rows whose tag bytes cover all 256 values and whose words point into and out of a synthetic string buffer, the row lengths
around a wave, a workgroup and a grid stride, rows in which every cell, no cell and one cell per wave takes the exact road, in place, and the refusals.
The driver also runs built with -fsanitize=address,undefined, its string buffer a heap block that ends with the buffer's last byte."""
import os
import struct
import subprocess

import numpy as np
import pytest

import in_string_cases as cases
import in_string_model as model
from simdjson_amd import _paths

CSRC = os.path.join(_paths.PKG_DIR, "csrc")
EMU = os.path.join(_paths.REPO_ROOT, "tests", "host", "emu")
BADARG = -4


def build(out, sanitize=()):
    """the way tests/test_casts_emu.py builds its units"""
    inc = ["-I", EMU, "-I", _paths.INCLUDE_DIR, "-I", CSRC]
    jobs = [subprocess.Popen(["g++", "-std=c++17", "-O1", *sanitize, "-Wno-attributes", "-Wno-unknown-pragmas", "-x", "c++", *inc, "-c",
                              os.path.join(CSRC, "sjgpu_cast_strings.hip"), "-o", str(out / "sjgpu_cast_strings.o")]),
            subprocess.Popen(["g++", "-std=c++17", "-O2", *sanitize, *inc, "-c", os.path.join(EMU, "sj_emu.cpp"), "-o", str(out / "sj_emu.o")]),
            subprocess.Popen(["g++", "-std=c++17", "-O2", *sanitize, "-Wno-attributes", *inc, "-c",
                              os.path.join(_paths.REPO_ROOT, "tests", "host", "test_cast_strings_emu.cpp"), "-o", str(out / "driver.o")])]
    assert all(j.wait() == 0 for j in jobs)
    exe = str(out / "test_cast_strings_emu")
    subprocess.run(["g++", *sanitize, *[str(out / (f + ".o")) for f in ("sjgpu_cast_strings", "sj_emu", "driver")], "-lpthread", "-o", exe], check=True)
    return exe


def blob_of(tags, values, sbuf, getters, in_place=False, spoil=0):
    tags, values = np.ascontiguousarray(tags, np.uint8), np.ascontiguousarray(values, np.uint64)
    K, n = tags.shape
    assert values.shape == (K, n) and len(getters) == K
    return struct.pack("<IIIIQ", n, K, int(in_place), spoil, len(sbuf)) + bytes(getters) + tags.tobytes() + values.tobytes() + bytes(sbuf)


def results_of(out, calls):
    """the driver's records, one per (n, K): [(code, (value_out, code_out, valid, counts) | None)]"""
    at, got = 0, []
    for n, K in calls:
        code, = struct.unpack_from("<i", out, at)
        at += 4
        cast = None
        W = (n + 63) // 64
        if code == 0 and K:
            value_out = np.frombuffer(out, np.uint64, K * n, at).reshape(K, n)
            at += K * n * 8
            code_out = np.frombuffer(out, np.uint8, K * n, at).reshape(K, n)
            at += K * n
            valid = np.frombuffer(out, np.uint64, K * W, at).reshape(K, W)
            at += K * W * 8
            counts = np.frombuffer(out, np.uint32, K * 8, at).reshape(K, 8)
            at += K * 32
            cast = (value_out, code_out, valid, counts)
        got.append((code, cast))
    assert at == len(out)
    return got


def assert_equals_model(got, tags, values, sbuf, getters):
    """-> the model's answer"""
    code, cast = got
    assert code == 0
    want = model.cast(tags, values, sbuf, getters)
    for name, mine, theirs in zip(("value_out", "code_out", "valid_out", "counts"), cast, want):
        assert np.array_equal(mine, theirs), (name, np.argwhere(mine != theirs)[:5].tolist())
    value_out, code_out, valid, counts = want[:4]
    # the counts sum to n, by what a cell is: it held a code [3], was refused for its kind [4], is a string that points outside [6] -- or is a string inside
    # the buffer, or a number under the flag, and was answered by the rule; and by what it got: valid [0] (the bits of the bitmap), or a code
    n = tags.shape[1]
    flag = (np.array(getters, np.uint8) & 0x10).astype(bool)[:, None]
    answered = ((tags == 0x22).sum(axis=1) - cast[3][:, 6]) + (flag & np.isin(tags, np.frombuffer(b"lud", np.uint8))).sum(axis=1)
    assert np.array_equal(cast[3][:, [3, 4]].sum(axis=1) + cast[3][:, 6] + answered, np.full(len(getters), n))
    assert np.array_equal(cast[3][:, 0] + (cast[1] != 0).sum(axis=1), np.full(len(getters), n))
    assert cast[3][:, 0].tolist() == [sum(bin(int(w)).count("1") for w in row) for row in cast[2]] and not cast[3][:, 7].any()
    return want


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    exe = build(tmp_path_factory.mktemp("cast_strings_emu"))

    def run(blob, calls):
        p = subprocess.run([exe], input=blob, capture_output=True, timeout=1500)
        assert p.returncode == 0, p.stderr.decode(errors="replace")[-3000:]
        return results_of(p.stdout, calls)
    return run


@pytest.fixture(scope="module")
def buffer():
    return cases.string_buffer(cases.pool())


def test_the_fixture_under_all_six_getter_bytes(emu, buffer):
    sbuf, words = buffer
    fixture = model.load_fixture()
    n = len(fixture)
    tags, values = np.full((6, n), 0x22, np.uint8), np.tile(np.array(words[:n], np.uint64), (6, 1))
    (code, cast), = emu(blob_of(tags, values, sbuf, model.ALL_GETTERS), [(n, 6)])
    assert code == 0
    for k, g in enumerate(model.ALL_GETTERS):  # against the reference's own answers, not the model's
        for i, (content, answers) in enumerate(fixture):
            assert (int(cast[1][k, i]), int(cast[0][k, i])) == answers[(g & 0x0F) - 1], (g, content[:60])
    assert_equals_model((code, cast), tags, values, sbuf, model.ALL_GETTERS)
    assert cast[3][2, 5] > 50 and not cast[3][0, 5] and not cast[3][1, 5]  # the exact road is the double's alone


def test_random_rows_of_every_length_and_height(emu, buffer):
    sbuf, words = buffer
    rng = np.random.default_rng(191)
    shapes = [(n, K) for n in (0, 1, 63, 64, 65, 255, 256, 257) for K in (1, 3, 64)]
    shapes.append((8449, 64))  # 64 rows share 2 048 workgroups, 32 each: the second step of the grid-stride loop, with a tail
    cells = [cases.random_cells(rng, n, K, words, len(sbuf)) for n, K in shapes]
    blob = b"".join(blob_of(t, v, sbuf, cases.cycled(K, i)) for i, ((n, K), (t, v)) in enumerate(zip(shapes, cells)))
    seen = set()
    for i, (got, (n, K), (t, v)) in enumerate(zip(emu(blob, shapes), shapes, cells)):
        want = assert_equals_model(got, t, v, sbuf, cases.cycled(K, i))
        seen |= set(want[1].reshape(-1).tolist())
    assert {0, 9, 17, 18, 19, 20, 22} <= seen
    assert set(cells[shapes.index((257, 1))][0].reshape(-1).tolist()) == set(range(256))


def test_the_buffers_first_and_last_bytes_and_words_that_point_outside(emu):
    contents = [b"7", b"", b"12345", b"-0", b"1.25e2"]
    for last in (b"9", b"18446744073709551615", b"0." + b"1" * 25, b"1" * 40):  # the last record ends on the buffer's last byte: within 16, 32 and more bytes of it
        sbuf, words = cases.string_buffer(contents + [last])
        assert words[0] & 0xFFFFFFFF == 4 and (words[-1] & 0xFFFFFFFF) + (words[-1] >> 32) == len(sbuf)
        every = words + cases.outside_words(len(sbuf)) + [(0 << 32) | len(sbuf)]  # (length 0 at the very end is inside)
        tags, values = np.full((6, len(every)), 0x22, np.uint8), np.tile(np.array(every, np.uint64), (6, 1))
        got, = emu(blob_of(tags, values, sbuf, model.ALL_GETTERS), [(len(every), 6)])
        want = assert_equals_model(got, tags, values, sbuf, model.ALL_GETTERS)
        assert want[3][:, 6].tolist() == [6] * 6 and want[1][0, 0] == 0 and want[0][0, 0] == 7 and want[1][2, len(words) - 1] == 0
    # a buffer shorter than one wide load, and an empty one (a null buffer is allowed with no bytes)
    for contents in ([b"42"], [b""]):
        sbuf, words = cases.string_buffer(contents)
        tags, values = np.full((3, 1), 0x22, np.uint8), np.full((3, 1), words[0], np.uint64)
        got, = emu(blob_of(tags, values, sbuf, [1, 2, 3]), [(1, 3)])
        assert_equals_model(got, tags, values, sbuf, [1, 2, 3])
    tags, values = np.full((1, 2), 0x22, np.uint8), np.array([[0, 1 << 32]], np.uint64)
    got, = emu(blob_of(tags, values, b"", [3], spoil=12), [(2, 1)])
    assert got[1][1].tolist() == [[17, 17]] and got[1][3][0].tolist() == [0, 0, 0, 0, 0, 0, 1, 0]


def test_in_place_gives_what_out_of_place_gives(emu, buffer):
    sbuf, words = buffer
    rng = np.random.default_rng(192)
    shapes = [(257, 3), (1025, 1), (64, 64), (0, 2)]
    cells = [cases.random_cells(rng, n, K, words, len(sbuf)) for n, K in shapes]
    blob = b"".join(blob_of(t, v, sbuf, cases.cycled(K, 2), in_place=True) for (n, K), (t, v) in zip(shapes, cells))
    for got, (n, K), (t, v) in zip(emu(blob, shapes), shapes, cells):
        assert_equals_model(got, t, v, sbuf, cases.cycled(K, 2))


def test_rows_where_all_none_and_one_cell_per_wave_take_the_exact_road(emu):
    long_ones = cases.long_decimals() + [b"1" * 40 + b"x"]
    short_ones = [b"1.5", b"-2e3", b"12345678901234567", b"x"]
    sbuf, words = cases.string_buffer(long_ones + short_ones)
    slow, fast = np.array(words[:len(long_ones)], np.uint64), np.array(words[len(long_ones):], np.uint64)
    n = 257
    rng = np.random.default_rng(193)
    rows = [slow[rng.integers(0, len(slow), n)], fast[rng.integers(0, len(fast), n)]]
    for lane in (0, 63):  # the exact road's validity bit lands in a word of the other road's cells
        row = fast[rng.integers(0, len(fast) - 1, n)]  # (no `x`: every bit around it is set)
        row[lane::64] = slow[0]
        rows.append(row)
    values = np.stack(rows)
    tags = np.full(values.shape, 0x22, np.uint8)
    for in_place in (False, True):
        got, = emu(blob_of(tags, values, sbuf, [3, 3, 3, 3 | 0x10], in_place=in_place), [(n, 4)])
        want = assert_equals_model(got, tags, values, sbuf, [3, 3, 3, 3 | 0x10])
        assert want[3][:, 5].tolist() == [257, 0, 5, 4] and want[3][2, 0] == 257 and want[2][3, 0] == (1 << 64) - 1
    assert not (got[1][1] == 0xFF).any()


def test_the_refusals(emu, buffer):
    sbuf, words = buffer
    rng = np.random.default_rng(194)
    t, v = cases.random_cells(rng, 65, 3, words, len(sbuf))
    g = [1, 2 | 0x10, 3]

    def code(tags=t, values=v, getters=g, sbuf=sbuf, **kw):
        (c, cast), = emu(blob_of(tags, values, sbuf, getters, **kw), [tags.shape[::-1]])
        return c
    assert code() == 0
    # (spoil: see the driver) a null pointer while K * n > 0, per argument; the string buffer only while it has bytes; the alignments
    for spoil in range(1, 13):
        assert code(spoil=spoil) == BADARG, spoil
    # a getter outside 1 .. 3 in its low four bits, or with a bit other than 0x10 above them
    for bad in (0, 4, 7, 0x10, 0x14, 0x21, 0x41, 0x81, 0x31, 255):
        assert code(getters=[1, bad, 3]) == BADARG, bad
    for good in (1, 2, 3, 0x11, 0x12, 0x13):
        assert code(getters=[1, good, 3]) == 0, good
    # K > 64
    t65, v65 = cases.random_cells(rng, 5, 65, words, len(sbuf))
    assert code(t65, v65, cases.cycled(65)) == BADARG and code(t65[:64], v65[:64], cases.cycled(64)) == 0
    # K == 0: 0, nothing written, whatever the pointers are; n == 0 with K > 0: the cells' pointers and the buffer may be null
    none = (np.zeros((0, 9), np.uint8), np.zeros((0, 9), np.uint64))
    assert code(*none, []) == code(*none, [], spoil=1) == code(*none, [], spoil=3) == code(*none, [], spoil=7) == code(*none, [], spoil=12) == 0
    assert code(*none, [], spoil=8) == BADARG  # (the alignments hold for every K)
    empty = (np.zeros((2, 0), np.uint8), np.zeros((2, 0), np.uint64))
    for spoil in (1, 2, 4, 5, 6, 12):
        (c, cast), = emu(blob_of(*empty, sbuf, [1, 3], spoil=spoil), [(0, 2)])
        assert c == 0 and not cast[3].any()
    assert code(*empty, [1, 3], spoil=3) == code(*empty, [1, 3], spoil=7) == code(*empty, [1, 5]) == BADARG


def test_the_driver_runs_clean_under_the_sanitizers(tmp_path, buffer):
    """the stand-alone driver -- kernels, launcher, argument check -- built with -fsanitize=address,undefined: every output at its exact size, the string buffer a
    heap block that ends with its last byte and begins at an odd address, out of place and in place: no byte is read outside the buffer"""
    # (the runtimes linked statically: the program stands alone, whatever else the loader is told to bring in)
    exe = build(tmp_path, ("-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer", "-g"))
    sbuf, words = buffer
    t, v = cases.random_cells(np.random.default_rng(195), 257, 3, words, len(sbuf))
    g = [3, 1 | 0x10, 2]
    tail, tail_words = cases.string_buffer([b"1", b"2.5", b"0." + b"1" * 25, b"18446744073709551615"])  # strings within 16 and 32 bytes of the end
    tt, tv = np.full((3, len(tail_words)), 0x22, np.uint8), np.tile(np.array(tail_words, np.uint64), (3, 1))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe], input=blob_of(t, v, sbuf, g) + blob_of(t, v, sbuf, g, in_place=True) + blob_of(tt, tv, tail, g), capture_output=True, timeout=1500, env=env)
    assert p.returncode == 0 and b"runtime error" not in p.stderr and b"AddressSanitizer" not in p.stderr, p.stderr.decode(errors="replace")[-3000:]
    got = results_of(p.stdout, [(257, 3)] * 2 + [(len(tail_words), 3)])
    assert_equals_model(got[0], t, v, sbuf, g)
    assert_equals_model(got[1], t, v, sbuf, g)
    assert_equals_model(got[2], tt, tv, tail, g)
