"""CPU tier: the dictionary of a row of string cells and the census per code -- the gfx950 kernel sources of sjgpu_dict.hip and the scans of sjgpu_finish.hip,
compiled as C++ against tests/host/emu -- run the launches of sjgpu_dictionary_encode_device and sjgpu_cell_kinds_by_code_device (tests/host/test_dict_emu.cpp)
and are compared slot for slot with tests/dictionary_model.py: the fixture's rows, rows at the wave's and the workgroup's edges, strings of every length around
the compare's 8-byte steps, pairs that differ in their last byte or of which one is a prefix of the other, 70 000 cells of one string, 70 000 distinct ones, waves
that hold the same three strings in rotating order, cells that are no strings, and the three capacities.  Every test that runs the driver through `emu` -- all
but the sanitizer build -- runs twice: with the 64-bit hash and with the hash cut to 3 bits (-DSJGPU_DICT_HASH_BITS=3: every string meets equal hashes with unequal
bytes and long probe chains); the model is the same, so the outputs are.  The driver also runs built with -fsanitize=address,undefined."""
import os
import struct
import subprocess

import numpy as np
import pytest

import checkers
import dictionary_cases
import dictionary_model
from dictionary_cases import LENGTHS, ROW_COUNTS, STRING
from simdjson_amd import _paths

CSRC = os.path.join(_paths.PKG_DIR, "csrc")
EMU = os.path.join(_paths.REPO_ROOT, "tests", "host", "emu")
KERNEL_TUS = ("sjgpu_dict", "sjgpu_finish")
EXACT, ONE_SHORT, NONE = 0, 1, 2
OVERFLOW = -5
DISTINCT = 0xFFFFFFFF  # a census with as many groups as there are distinct strings


def build(out, hash_bits=64, sanitize=()):
    """the way tests/test_fields_emu.py builds its units"""
    inc = ["-I", EMU, "-I", _paths.INCLUDE_DIR, "-I", CSRC]
    jobs = []
    for name in KERNEL_TUS:
        jobs.append(subprocess.Popen(["g++", "-std=c++17", "-O2", *sanitize, f"-DSJGPU_DICT_HASH_BITS={hash_bits}", "-Wno-attributes", "-Wno-unknown-pragmas", "-x", "c++", *inc,
                                      "-c", os.path.join(CSRC, name + ".hip"), "-o", str(out / (name + ".o"))]))
    jobs.append(subprocess.Popen(["g++", "-std=c++17", "-O2", *sanitize, *inc, "-c", os.path.join(EMU, "sj_emu.cpp"), "-o", str(out / "sj_emu.o")]))
    jobs.append(subprocess.Popen(["g++", "-std=c++17", "-O2", *sanitize, "-Wno-attributes", *inc, "-c",
                                  os.path.join(_paths.REPO_ROOT, "tests", "host", "test_dict_emu.cpp"), "-o", str(out / "driver.o")]))
    assert all(j.wait() == 0 for j in jobs)
    exe = str(out / "test_dict_emu")
    subprocess.run(["g++", *sanitize, *[str(out / (f + ".o")) for f in (*KERNEL_TUS, "sj_emu", "driver")], "-lpthread", "-o", exe], check=True)
    return exe


def blob_of(sbuf, row, value_row, capacity, groups):
    tags, values = np.ascontiguousarray(row[0], np.uint8), np.ascontiguousarray(row[1], np.uint64)
    vtags, vvalues = np.ascontiguousarray(value_row[0], np.uint8), np.ascontiguousarray(value_row[1], np.uint64)
    assert len(tags) == len(values) == len(vtags) == len(vvalues)
    sbuf = np.ascontiguousarray(sbuf, np.uint8)
    return (struct.pack("<Q", len(sbuf)) + sbuf.tobytes() + struct.pack("<I", len(tags)) + tags.tobytes() + values.tobytes() + vtags.tobytes() + vvalues.tobytes() +
            struct.pack("<II", capacity, len(groups)) + np.array(groups, np.uint32).tobytes())


def records_of(out, calls):
    """the driver's records, one per call of (n cells, the censuses' groups): [(code, distinct, codes, (first, values, tags, counts), [kinds per census])]"""
    at, got = 0, []
    for n, groups in calls:
        code, distinct = struct.unpack_from("<iQ", out, at)
        at += 12
        codes = np.frombuffer(out, np.int32, n, at)
        at += 4 * n
        written = 0 if code else distinct
        cols = []
        for dtype, width in ((np.uint32, 4), (np.uint64, 8), (np.uint8, 1), (np.uint32, 4)):
            cols.append(np.frombuffer(out, dtype, written, at))
            at += width * written
        kinds = []
        for G in groups:
            G = distinct if G == DISTINCT else G
            kinds.append(np.frombuffer(out, np.uint32, G * 16, at).reshape(G, 16))
            at += 64 * G
        got.append((code, distinct, codes, cols, kinds))
    assert at == len(out)
    return got


def compare(record, want, capacity, value_row, groups):
    code, distinct, codes, (first, values, tags, counts), kinds = record
    want_codes, want_first, want_values, want_counts = want
    assert distinct == len(want_first)
    assert np.array_equal(codes, want_codes)  # (whatever the capacity)
    if capacity == EXACT or distinct == 0:
        assert code == 0
        assert np.array_equal(first, want_first) and np.array_equal(values, want_values) and np.array_equal(counts, want_counts) and (tags == STRING).all()
    else:  # the dictionary does not fit: the codes complete, nothing written (the driver checks that), the total reported
        assert code == OVERFLOW and first.size == 0
    for G, got in zip(groups, kinds):
        G = distinct if G == DISTINCT else G
        assert np.array_equal(got, dictionary_model.kinds_by_code(want_codes, value_row[0], value_row[1], G)), G


@pytest.fixture(scope="module", params=[64, 3], ids=["hash64", "hash3"])
def emu(request, tmp_path_factory):
    exe = build(tmp_path_factory.mktemp(f"dict_emu{request.param}"), request.param)

    def run(sbuf, row, value_row=None, capacity=EXACT, groups=(DISTINCT,)):
        """-> the model's (codes, first, dictionary values, counts); everything the driver wrote is compared with the model here"""
        value_row = row if value_row is None else value_row
        p = subprocess.run([exe], input=blob_of(sbuf, row, value_row, capacity, groups), capture_output=True, timeout=1500)
        assert p.returncode == 0, p.stderr.decode(errors="replace")[-3000:]
        record, = records_of(p.stdout, [(len(row[0]), groups)])
        want = dictionary_model.encode(row[0], row[1], sbuf)
        compare(record, want, capacity, value_row, groups)
        return want
    return run


@pytest.fixture(scope="module")
def fixture_rows():
    return dictionary_cases.fixture_rows(checkers.Oracle())


def test_the_fixture_rows(emu, fixture_rows):
    """every row of the fixture (the model is pinned against the fixture by tests/test_dictionary_model.py), its value row counted per code; and the dictionary
    row encoded again gives the codes 0 .. G - 1"""
    for c, sbuf, row, value_row in fixture_rows:
        codes, first, dict_values, counts = emu(sbuf, row, value_row, groups=(DISTINCT, 1, 0))
        assert len(first) == len(c["strings"]) and counts.tolist() == c["counts"]
        again = emu(sbuf, (np.full(len(first), STRING, np.uint8), dict_values))
        assert again[0].tolist() == list(range(len(first))) and (again[3] == 1).all()


def test_the_capacities(emu, fixture_rows):
    for c, sbuf, row, value_row in fixture_rows:
        if c["path"] in (b"$.statuses[*].user", b"$.statuses[*].id", b"$[*]", b"$.events.*.logo"):
            for capacity in (ONE_SHORT, NONE):
                emu(sbuf, row, value_row, capacity)


def test_the_driver_runs_clean_under_the_sanitizers(tmp_path, fixture_rows):
    """the stand-alone driver -- kernels and launchers -- built with -fsanitize=address,undefined: the fixture, all three capacities"""
    # (the runtimes linked statically: the program stands alone, whatever else the loader is told to bring in)
    exe = build(tmp_path, 64, ("-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer", "-g"))
    capacities = (EXACT, ONE_SHORT, NONE)
    blob = b"".join(blob_of(sbuf, row, value_row, cap, (DISTINCT,)) for _, sbuf, row, value_row in fixture_rows for cap in capacities)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe], input=blob, capture_output=True, timeout=1500, env=env)
    assert p.returncode == 0 and b"runtime error" not in p.stderr and b"AddressSanitizer" not in p.stderr, p.stderr.decode(errors="replace")[-3000:]
    got = records_of(p.stdout, [(len(row[0]), (DISTINCT,)) for _, _, row, _ in fixture_rows for _ in capacities])
    at = 0
    for _, sbuf, row, value_row in fixture_rows:
        want = dictionary_model.encode(row[0], row[1], sbuf)
        for cap in capacities:
            compare(got[at], want, cap, value_row, (DISTINCT,))
            at += 1
    assert OVERFLOW in [g[0] for g in got] and 0 in [g[0] for g in got]


@pytest.mark.parametrize("n", ROW_COUNTS)
def test_rows_at_the_wave_and_workgroup_edges(emu, n):
    """n strings of every length, many repeats, tricky pairs; with every fifth cell no string"""
    rng = np.random.default_rng(100 + n)
    sbuf, (tags, values) = dictionary_cases.string_row(dictionary_cases.mixed_strings(rng, n))
    codes, first, _, counts = emu(sbuf, (tags, values))
    assert n < 255 or len(first) > 30
    bad = dictionary_cases.non_string_cells(len(sbuf))
    tags, values = tags.copy(), values.copy()
    for k, i in enumerate(range(0, n, 5)):
        tags[i], values[i] = bad[k % len(bad)]
    codes, first, _, counts = emu(sbuf, (tags, values), capacity=ONE_SHORT)
    assert (codes[::5] == -1).all() and int(counts.sum()) == n - len(range(0, n, 5))


def test_string_lengths_and_tricky_pairs(emu):
    """every length twice at two offsets; pairs that differ only in the last byte; one a prefix of the other; NULs inside"""
    strings = []
    for length in LENGTHS:
        base = bytes((7 * i + length) & 0xFF for i in range(length))
        strings += [base, base, base[:-1] + bytes([(base[-1] + 1) & 0xFF]) if length else b"", base + b"\0", base[:-1] if length else b"\0\0", base]
    strings += [b"a\0b", b"a", b"a\0", b"A", b"", b"a\0b"]
    sbuf, row = dictionary_cases.string_row(strings)
    codes, first, dict_values, counts = emu(sbuf, row)
    want = {}
    for s in strings:
        want[s] = want.get(s, 0) + 1
    assert [dictionary_model.string_of(sbuf, STRING, v) for v in dict_values.tolist()] == list(want) and counts.tolist() == list(want.values())
    for capacity in (ONE_SHORT, NONE):
        emu(sbuf, row, capacity=capacity)


def test_cells_that_are_no_strings(emu):
    """every tag, every code, bytes that are neither, string cells that point outside the buffer: all nulls; a string that ends with the buffer is one"""
    sbuf, (tags, values) = dictionary_cases.string_row([b"in", b"side", b"in"])
    bad = dictionary_cases.non_string_cells(len(sbuf))
    last = (0 << 32) | len(sbuf)  # the empty string at the buffer's end
    cells = [(STRING, int(values[0]))] + bad + [(STRING, int(values[1])), (STRING, last), (STRING, int(values[2]))]
    row = (np.array([t for t, _ in cells], np.uint8), np.array([v for _, v in cells], np.uint64))
    codes, first, _, counts = emu(sbuf, row, groups=(DISTINCT, 2, 513))
    assert codes.tolist() == [0] + [-1] * len(bad) + [1, 2, 0] and counts.tolist() == [2, 1, 1]
    nothing = (np.array([t for t, _ in bad], np.uint8), np.array([v for _, v in bad], np.uint64))
    for capacity in (EXACT, ONE_SHORT, NONE):
        assert len(emu(sbuf, nothing, capacity=capacity)[1]) == 0


def test_seventy_thousand_cells_of_one_string(emu):
    sbuf, row = dictionary_cases.string_row([b"the only one"] * 70000)
    codes, first, _, counts = emu(sbuf, row)
    assert first.tolist() == [0] and counts.tolist() == [70000]


def test_seventy_thousand_distinct_strings(emu):
    sbuf, row = dictionary_cases.string_row([b"%05d" % i + b"-" * (i % 23) for i in range(70000)])
    codes, first, _, counts = emu(sbuf, row, groups=(DISTINCT, 5000))
    assert np.array_equal(codes, np.arange(70000)) and (counts == 1).all()
    emu(sbuf, row, capacity=ONE_SHORT, groups=())


def test_every_wave_holds_the_same_three_strings_in_rotating_order(emu):
    sbuf, row = dictionary_cases.string_row(dictionary_cases.rotating_row(64 * 40 + 17))
    codes, first, _, counts = emu(sbuf, row)
    assert first.tolist() == [0, 1, 2] and int(counts.sum()) == 64 * 40 + 17


def test_census_groups_on_both_sides_of_the_lds_threshold(emu):
    """G = 1, 40, 512, 513 and 5 000 over a value row of every kind of cell"""
    rng = np.random.default_rng(5)
    n = 6000
    sbuf, row = dictionary_cases.string_row([b"key%d" % int(k) for k in rng.integers(0, 700, n)])
    vtags = rng.choice(np.frombuffer(b'{["ludtfn\x11\x13\x14\x16\x00Z', np.uint8), n)
    vvalues = rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n, dtype=np.uint64)
    emu(sbuf, row, (vtags, vvalues), groups=(1, 40, 512, 513, 5000, DISTINCT, 0))
