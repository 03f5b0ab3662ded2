"""CPU tier: the typed getters over cells -- the gfx950 kernel source sjgpu_cast.hip, compiled as C++ against tests/host/emu -- run what
sjgpu_cell_kinds_device and sjgpu_cast_cells_device enqueue (tests/host/test_casts_emu.cpp) and are compared bit for bit with tests/cast_model.py: the
fixture's cells under all seven getters, random rows whose tag bytes cover all 256 values and whose words sit on the edges of the number formats, the row
lengths around a wave, a workgroup and a grid stride, in place, and the refusals.  The driver also runs built with -fsanitize=address,undefined."""
import os
import struct
import subprocess

import numpy as np
import pytest

import cast_model
import checkers
from simdjson_amd import _paths
from test_cast_model import fixture_cells

CSRC = os.path.join(_paths.PKG_DIR, "csrc")
EMU = os.path.join(_paths.REPO_ROOT, "tests", "host", "emu")
BADARG = -4
EDGE_WORDS = np.array([0, 1, (1 << 64) - 1, (1 << 63) - 1, 1 << 63, (1 << 63) + 1, 1 << 53, (1 << 53) + 1, (1 << 64) - ((1 << 53) + 1), 18446744073709549568,
                       18446744073709550591, 18446744073709550592, 0x43E158E460913D00, 0x3FF8000000000000, 0x7FEFFFFFFFFFFFFF, (3 << 32) | 4, (9 << 32) | 2,
                       0x5A5A5A5A5A5A5A5A], np.uint64)


def build(out, sanitize=()):
    """the way tests/test_lists_emu.py builds its units"""
    inc = ["-I", EMU, "-I", _paths.INCLUDE_DIR, "-I", CSRC]
    jobs = [subprocess.Popen(["g++", "-std=c++17", "-O1", *sanitize, "-Wno-attributes", "-Wno-unknown-pragmas", "-x", "c++", *inc, "-c",
                              os.path.join(CSRC, "sjgpu_cast.hip"), "-o", str(out / "sjgpu_cast.o")]),
            subprocess.Popen(["g++", "-std=c++17", "-O2", *sanitize, *inc, "-c", os.path.join(EMU, "sj_emu.cpp"), "-o", str(out / "sj_emu.o")]),
            subprocess.Popen(["g++", "-std=c++17", "-O2", *sanitize, "-Wno-attributes", *inc, "-c",
                              os.path.join(_paths.REPO_ROOT, "tests", "host", "test_casts_emu.cpp"), "-o", str(out / "driver.o")])]
    assert all(j.wait() == 0 for j in jobs)
    exe = str(out / "test_casts_emu")
    subprocess.run(["g++", *sanitize, *[str(out / (f + ".o")) for f in ("sjgpu_cast", "sj_emu", "driver")], "-lpthread", "-o", exe], check=True)
    return exe


def blob_of(tags, values, getters, in_place=False, spoil=0):
    tags, values = np.ascontiguousarray(tags, np.uint8), np.ascontiguousarray(values, np.uint64)
    K, n = tags.shape
    assert values.shape == (K, n) and len(getters) == K
    return struct.pack("<IIII", n, K, int(in_place), spoil) + bytes(getters) + tags.tobytes() + values.tobytes()


def results_of(out, calls):
    """the driver's records, one per (n, K): [(census code, cast code, kinds | None, (value_out, code_out, valid, counts) | None)]"""
    at, got = 0, []
    for n, K in calls:
        kinds_code, cast_code = struct.unpack_from("<ii", out, at)
        at += 8
        kinds = cast = None
        W = (n + 63) // 64
        if kinds_code == 0 and K:
            kinds = np.frombuffer(out, np.uint32, K * 16, at).reshape(K, 16)
            at += K * 64
        if cast_code == 0 and K:
            value_out = np.frombuffer(out, np.uint64, K * n, at).reshape(K, n)
            at += K * n * 8
            code_out = np.frombuffer(out, np.uint8, K * n, at).reshape(K, n)
            at += K * n
            valid = np.frombuffer(out, np.uint64, K * W, at).reshape(K, W)
            at += K * W * 8
            counts = np.frombuffer(out, np.uint32, K * 4, at).reshape(K, 4)
            at += K * 16
            cast = (value_out, code_out, valid, counts)
        got.append((kinds_code, cast_code, kinds, cast))
    assert at == len(out)
    return got


def assert_equals_model(got, tags, values, getters):
    kinds_code, cast_code, kinds, cast = got
    assert kinds_code == 0 and cast_code == 0
    assert np.array_equal(kinds, cast_model.kinds(tags, values))
    for name, mine, want in zip(("value_out", "code_out", "valid_out", "counts"), cast, cast_model.cast(tags, values, getters)):
        assert np.array_equal(mine, want), name


def random_cells(rng, n, K):
    """tag bytes over all 256 values (the nine tags and the four codes more often), words from the edges"""
    common = np.frombuffer(b'{["ludtfn' + bytes([17, 19, 20, 22]), np.uint8)
    tags = np.where(rng.random((K, n)) < 0.6, common[rng.integers(0, len(common), (K, n))], rng.integers(0, 256, (K, n)).astype(np.uint8)).astype(np.uint8)
    flat = tags.reshape(-1)
    flat[: min(256, flat.size)] = np.arange(min(256, flat.size), dtype=np.uint8)  # every byte at least once where there is room
    values = EDGE_WORDS[rng.integers(0, len(EDGE_WORDS), (K, n))]
    return tags, values


def cycled(K, first=0):
    return [1 + (first + k) % 7 for k in range(K)]


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    exe = build(tmp_path_factory.mktemp("casts_emu"))

    def run(blob, calls):
        p = subprocess.run([exe], input=blob, capture_output=True, timeout=1500)
        assert p.returncode == 0, p.stderr.decode(errors="replace")[-3000:]
        return results_of(p.stdout, calls)
    return run


def test_the_fixture_cells_under_all_seven_getters(emu):
    tags, words, answers, sbufs = fixture_cells(checkers.Oracle())
    tags, values = np.tile(tags, (7, 1)), np.tile(words, (7, 1))
    getters = list(range(1, 8))
    got, = emu(blob_of(tags, values, getters), [tags.shape[::-1]])
    assert_equals_model(got, tags, values, getters)  # (the model is pinned against the fixture by tests/test_cast_model.py)
    assert {0, 17, 18, 19, 20, 22} <= set(got[3][1].reshape(-1).tolist())


def test_random_rows_of_every_length_and_height(emu):
    rng = np.random.default_rng(91)
    cases = [(n, K) for n in (0, 1, 63, 64, 65, 255, 256, 257, 4097) for K in (1, 3, 64)]
    cases.append((8449, 64))  # 64 rows share 2 048 workgroups, 32 each: the second step of the grid-stride loop, with a tail
    cells = [random_cells(rng, n, K) for n, K in cases]
    blob = b"".join(blob_of(t, v, cycled(K, i)) for i, ((n, K), (t, v)) in enumerate(zip(cases, cells)))
    for i, (got, (n, K), (t, v)) in enumerate(zip(emu(blob, cases), cases, cells)):
        assert_equals_model(got, t, v, cycled(K, i))
    assert set(cells[cases.index((4097, 1))][0].reshape(-1).tolist()) == set(range(256))


def test_in_place_gives_what_out_of_place_gives(emu):
    rng = np.random.default_rng(92)
    cases = [(257, 3), (4097, 1), (64, 64), (0, 2)]
    cells = [random_cells(rng, n, K) for n, K in cases]
    blob = b"".join(blob_of(t, v, cycled(K), in_place=True) for (n, K), (t, v) in zip(cases, cells))
    for got, (n, K), (t, v) in zip(emu(blob, cases), cases, cells):
        assert_equals_model(got, t, v, cycled(K))


def test_the_refusals(emu):
    rng = np.random.default_rng(93)
    t, v = random_cells(rng, 65, 3)
    g = cycled(3)

    def codes(tags=t, values=v, getters=g, **kw):
        (kinds_code, cast_code, kinds, cast), = emu(blob_of(tags, values, getters, **kw), [tags.shape[::-1]])
        return kinds_code, cast_code
    assert codes() == (0, 0)
    # (spoil: see the driver) a null pointer while K * n > 0, per argument
    assert codes(spoil=1) == codes(spoil=2) == (BADARG, BADARG) and codes(spoil=3) == (BADARG, BADARG)
    assert codes(spoil=4) == codes(spoil=5) == codes(spoil=6) == codes(spoil=7) == (0, BADARG)
    # the alignments
    assert codes(spoil=8) == (BADARG, BADARG) and codes(spoil=9) == codes(spoil=10) == (0, BADARG) and codes(spoil=11) == (BADARG, BADARG)
    # a getter outside 1 .. 7 (the census asks none)
    for bad in (0, 8, 255):
        assert codes(getters=[1, bad, 3]) == (0, BADARG)
    # K > 64
    t65, v65 = random_cells(rng, 5, 65)
    assert codes(t65, v65, cycled(65)) == (BADARG, BADARG) and codes(t65[:64], v65[:64], cycled(64)) == (0, 0)
    # K == 0: 0, nothing written, whatever the pointers are; n == 0 with K > 0: the cells' pointers may be null
    none = (np.zeros((0, 9), np.uint8), np.zeros((0, 9), np.uint64))
    assert codes(*none, []) == (0, 0) and codes(*none, [], spoil=1) == codes(*none, [], spoil=3) == codes(*none, [], spoil=7) == (0, 0)
    assert codes(*none, [], spoil=8) == (BADARG, BADARG)  # (the alignments hold for every K)
    empty = (np.zeros((2, 0), np.uint8), np.zeros((2, 0), np.uint64))
    for spoil in (1, 2, 4, 5, 6):
        (kinds_code, cast_code, kinds, cast), = emu(blob_of(*empty, [1, 5], spoil=spoil), [(0, 2)])
        assert (kinds_code, cast_code) == (0, 0) and not kinds.any() and not cast[3].any()
    assert codes(*empty, [1, 5], spoil=3) == (BADARG, BADARG) and codes(*empty, [1, 5], spoil=7) == (0, BADARG) and codes(*empty, [1, 9]) == (0, BADARG)


def test_the_driver_runs_clean_under_the_sanitizers(tmp_path):
    """the stand-alone driver -- kernels, launchers, argument checks -- built with -fsanitize=address,undefined: 257 cells x 3 rows, every output at its exact size,
    out of place and in place"""
    # (the runtimes linked statically: the program stands alone, whatever else the loader is told to bring in)
    exe = build(tmp_path, ("-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer", "-g"))
    t, v = random_cells(np.random.default_rng(94), 257, 3)
    g = [cast_model.DOUBLE, cast_model.INT64, cast_model.UINT64]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe], input=blob_of(t, v, g) + blob_of(t, v, g, in_place=True), capture_output=True, timeout=1500, env=env)
    assert p.returncode == 0 and b"runtime error" not in p.stderr and b"AddressSanitizer" not in p.stderr, p.stderr.decode(errors="replace")[-3000:]
    for got in results_of(p.stdout, [(257, 3)] * 2):
        assert_equals_model(got, t, v, g)
