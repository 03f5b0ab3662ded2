"""CPU tier: typed columns as JSON records -- the gfx950 kernel sources of sjgpu_write.hip with the total of sjgpu_query.hip and the scans of sjgpu_finish.hip,
compiled as C++ against tests/host/emu -- run the launches of sjgpu_write_records_device behind the host's own table (tests/host/test_write_emu.cpp) and are compared
byte for byte with tests/write_records_model.py and, through it, with tests/golden/write_records.json: the fixture's tables under every combination of the flags, row
counts at the wave's and the workgroup's edges, column counts up to the interface's 64, every shape of validity, spans on both sides of the staged road's window and at
every alignment of the output, bad offsets, doubles without a text, the refusals, and the three capacities.  The driver also runs built with
-fsanitize=address,undefined."""
import os
import struct
import subprocess

import numpy as np
import pytest

import write_records_cases as cases
import write_records_model as model
from simdjson_amd import _paths

CSRC = os.path.join(_paths.PKG_DIR, "csrc")
EMU = os.path.join(_paths.REPO_ROOT, "tests", "host", "emu")
KERNEL_TUS = ("sjgpu_write", "sjgpu_query", "sjgpu_finish")
EXACT, ONE_SHORT, NONE = 0, 1, 2
OVERFLOW, BADARG = -5, -4


def build(out, sanitize=()):
    """the way tests/test_json_emu.py builds its units"""
    inc = ["-I", EMU, "-I", _paths.INCLUDE_DIR, "-I", CSRC]
    jobs = []
    for name in KERNEL_TUS:
        jobs.append(subprocess.Popen(["g++", "-std=c++17", "-O2", *sanitize, "-Wno-attributes", "-Wno-unknown-pragmas", "-x", "c++", *inc, "-c", os.path.join(CSRC, name + ".hip"),
                                      "-o", str(out / (name + ".o"))]))
    jobs.append(subprocess.Popen(["g++", "-std=c++17", "-O2", *sanitize, *inc, "-c", os.path.join(EMU, "sj_emu.cpp"), "-o", str(out / "sj_emu.o")]))
    jobs.append(subprocess.Popen(["g++", "-std=c++17", "-O2", *sanitize, "-Wno-attributes", *inc, "-c", os.path.join(_paths.REPO_ROOT, "tests", "host", "test_write_emu.cpp"),
                                  "-o", str(out / "driver.o")]))
    assert all(j.wait() == 0 for j in jobs)
    exe = str(out / "test_write_emu")
    subprocess.run(["g++", *sanitize, *[str(out / (f + ".o")) for f in (*KERNEL_TUS, "sj_emu", "driver")], "-lpthread", "-o", exe], check=True)
    return exe


def blob_of(arrays, flags, capacity=EXACT, skew=1):
    n, out = arrays["n"], [struct.pack("<IIIII", arrays["n"], len(arrays["columns"]), flags, capacity, skew)]
    for c in arrays["columns"]:
        chars = b"" if c["chars"] is None else np.ascontiguousarray(c["chars"], np.uint8).tobytes()
        out.append(struct.pack("<I", len(c["key"])) + c["key"] + struct.pack("<I", c["kind"]) +
                   bytes([c["values"] is not None, c["valid"] is not None, c["offsets"] is not None, c["chars"] is not None]) + struct.pack("<QQ", c["chars_bytes"], len(chars)))
        if c["values"] is not None:
            assert len(c["values"]) == n
            out.append(np.ascontiguousarray(c["values"], np.uint64).tobytes())
        if c["valid"] is not None:
            assert len(c["valid"]) == (n + 63) // 64
            out.append(np.ascontiguousarray(c["valid"], np.uint64).tobytes())
        if c["offsets"] is not None:
            assert len(c["offsets"]) == n + 1
            out.append(np.ascontiguousarray(c["offsets"], np.uint32).tobytes())
        out.append(chars)
    return b"".join(out)


def records_of(out, calls):
    """the driver's records -> [(code, bytes, offsets, status, counts, chars)], (BADARG, 0) for a refusal"""
    at, got = 0, []
    for arrays, _, _, _ in calls:
        n = arrays["n"]
        code, total = struct.unpack_from("<iQ", out, at)
        at += 12
        if code == BADARG:
            got.append((code, total))
            continue
        offsets = np.frombuffer(out, np.uint32, n + 1, at)
        at += 4 * (n + 1)
        status = np.frombuffer(out, np.uint8, n, at)
        at += n
        counts = np.frombuffer(out, np.uint64, 4, at)
        at += 32
        written = 0 if code else total
        got.append((code, total, offsets, status, counts, out[at: at + written]))
        at += written
    assert at == len(out)
    return got


def compare(record, want, capacity):
    code, total, offsets, status, counts, chars = record
    want_offsets, want_chars, want_status, want_counts = want
    assert np.array_equal(status, want_status), "status"
    assert total == len(want_chars) and np.array_equal(offsets, want_offsets), "offsets"  # (whatever the capacity)
    assert np.array_equal(counts, want_counts), (counts, want_counts)
    if capacity == EXACT or total == 0:
        assert code == 0
        if chars != want_chars:
            at = next(i for i, (a, b) in enumerate(zip(chars, want_chars)) if a != b)
            raise AssertionError(f"chars differ at byte {at}: {chars[max(0, at - 40): at + 40]!r}, the model {want_chars[max(0, at - 40): at + 40]!r}")
    else:  # the texts do not fit: offsets, status and counts complete, nothing written (the driver checks that), the total reported
        assert code == OVERFLOW and chars == b""


def run_calls(exe, calls, env=None):
    """calls: [(arrays, flags, capacity, skew)] through ONE run of the driver, each compared with the model -> the model's results"""
    p = subprocess.run([exe], input=b"".join(blob_of(*c) for c in calls), capture_output=True, timeout=1500, env=env)
    assert p.returncode == 0 and b"runtime error" not in p.stderr and b"AddressSanitizer" not in p.stderr, p.stderr.decode(errors="replace")[-3000:]
    wants = []
    for record, (arrays, flags, capacity, _) in zip(records_of(p.stdout, calls), calls):
        want = model.records(arrays, flags)
        compare(record, want, capacity)
        wants.append(want)
    return wants


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    exe = build(tmp_path_factory.mktemp("write_emu"))

    def run(calls):
        return run_calls(exe, calls)
    run.exe = exe
    return run


def three_capacities(arrays, flags, skew=1):
    return [(arrays, flags, cap, skew) for cap in (NONE, ONE_SHORT, EXACT)]


def test_the_fixture_tables(emu):
    """every table of the fixture under the four combinations of the flags: row by row the reference's text"""
    fixture = cases.fixture()
    for t in cases.fixture_tables():
        arrays = cases.arrays_of(t, tail_ones=True)
        wants = emu([(arrays, flags, EXACT, 3) for flags in cases.ALL_FLAGS] + three_capacities(arrays, cases.NEWLINE)[:2])
        for flags, (offsets, chars, status, _) in zip(cases.ALL_FLAGS, wants):
            cases.assert_rows_are_the_fixtures(fixture[t["name"]][flags], cases.split(offsets, chars), (t["name"], flags))


@pytest.mark.parametrize("n", cases.ROW_COUNTS)
def test_rows_at_the_wave_and_workgroup_edges(emu, n):
    """six columns whose 256 rows take the direct road, two whose 256 rows take the staged one"""
    arrays, narrow = cases.arrays_of(cases.mixed_table(n), tail_ones=True), cases.arrays_of(cases.narrow_table(n), tail_ones=True)
    wants = emu(three_capacities(arrays, cases.NEWLINE) + [(arrays, cases.OMIT_NULLS, EXACT, 9)] + three_capacities(narrow, cases.NEWLINE) + [(narrow, 0, EXACT, 6)])
    assert len(wants[0][0]) == n + 1 and (n < 12 or wants[0][3][3] > 0)
    if n >= cases.ROWS_PER_STEP:
        assert int(wants[0][0][cases.ROWS_PER_STEP]) > cases.WINDOW > int(wants[4][0][cases.ROWS_PER_STEP])


@pytest.mark.parametrize("K", cases.COLUMN_COUNTS)
def test_column_counts(emu, K):
    arrays = cases.arrays_of(cases.wide_table(K))
    wants = emu([(arrays, flags, EXACT, 5) for flags in cases.ALL_FLAGS] + three_capacities(arrays, 0)[:2])
    if K == 0:
        assert wants[2][1] == b"{}\n" * 70 and wants[0][1] == b"{}" * 70


def test_every_shape_of_validity(emu):
    n = 130
    t = cases.mixed_table(n)
    calls = []
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
        calls += [(arrays, 0, EXACT, 1), (arrays, cases.OMIT_NULLS | cases.NEWLINE, EXACT, 2)]
    wants = emu(calls)
    assert wants[2][1] == b'{"id":null,"count":null,"score":null,"ok":null,"name":null,"tag":null}' * n and wants[3][1] == b"{}\n" * n
    assert wants[2][3].tolist() == [n, 0, 6 * n, 0]


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_a_span_at_the_window(emu, delta):
    """the texts of one workgroup iteration take exactly the window, one byte less, one byte more; the rows behind them are another iteration's"""
    arrays = cases.arrays_of(cases.span_table(cases.WINDOW + delta, rows_after=5))
    wants = emu([(arrays, cases.NEWLINE, EXACT, 0), (arrays, cases.NEWLINE, EXACT, 15), (arrays, cases.NEWLINE, ONE_SHORT, 0)])
    assert int(wants[0][0][cases.ROWS_PER_STEP]) == cases.WINDOW + delta


def test_a_long_string_between_short_rows(emu):
    """one row longer than the window: its iteration takes the direct road, the iterations on either side of it the staged one"""
    n = 3 * cases.ROWS_PER_STEP + 7
    t = cases.narrow_table(n)
    t["columns"][1]["cells"][cases.ROWS_PER_STEP + 100] = (b'long "string" \\ with\nescapes ' * 1200)[: cases.WINDOW + 300]
    arrays = cases.arrays_of(t)
    offsets = emu(three_capacities(arrays, cases.NEWLINE, skew=7))[0][0]
    spans = [int(offsets[min(r + cases.ROWS_PER_STEP, n)]) - int(offsets[r]) for r in range(0, n, cases.ROWS_PER_STEP)]
    assert spans[1] > cases.WINDOW and all(s <= cases.WINDOW for s in spans[:1] + spans[2:])


def test_every_alignment_of_the_output(emu):
    arrays = cases.arrays_of(cases.narrow_table(300))
    short = cases.arrays_of(cases.mixed_table(3))
    emu([(arrays, cases.NEWLINE, EXACT, skew) for skew in range(16)] + [(short, 0, EXACT, skew) for skew in range(16)])


def test_bad_offsets_are_status_19_and_a_validity_bit_of_0_hides_them(emu):
    arrays, bad = cases.bad_offsets()
    for flags in (0, cases.NEWLINE | cases.OMIT_NULLS):
        offsets, chars, status, counts = emu(three_capacities(arrays, flags))[0]
        assert [r for r in range(arrays["n"]) if status[r]] == bad and counts.tolist()[:2] == [arrays["n"] - len(bad), len(bad)]
    hidden, none = cases.bad_offsets(arrays_under_valid_bits=True)
    offsets, chars, status, counts = emu([(hidden, 0, EXACT, 1)])[0]
    assert not status.any() and counts.tolist() == [hidden["n"], 0, 6, 0]


def test_every_row_refused(emu):
    t = {"name": "t", "n": 300, "columns": [cases.column(b"s", cases.STRING, [b"abc"] * 300)]}
    arrays = cases.arrays_of(t)
    arrays["columns"][0]["chars_bytes"] = 2
    for offsets, chars, status, counts in emu(three_capacities(arrays, cases.NEWLINE)):
        assert (status == 19).all() and chars == b"" and not offsets.any() and counts.tolist() == [0, 300, 0, 0]


def test_doubles_without_a_text(emu):
    arrays = cases.arrays_of(cases.nonfinite_table())
    wants = emu([(arrays, flags, EXACT, 1) for flags in cases.ALL_FLAGS])
    assert all(w[3].tolist() == [10, 0, 7, 6] for w in wants) and b'{"d":null,"r":4}' in wants[0][1] and b'{"r":4}\n' in wants[3][1]


def test_the_refusals(emu):
    """every SJGPU_E_BADARG the host's table decides, with nothing written (the driver checks the poison)"""
    def table(changes=()):
        arrays = cases.arrays_of({"name": "t", "n": 4, "columns": [cases.column(b"a", cases.INT64, [1, None, 3, 4]), cases.column(b"s", cases.STRING, [b"x"] * 4),
                                                                   cases.column(b"c", cases.STRING_CELLS, [b"y"] * 4)]})
        for (k, field), v in dict(changes).items():
            arrays["columns"][k][field] = v
        return arrays
    good = table()
    refused = [table({(0, "kind"): 0}), table({(0, "kind"): 6}), table({(0, "kind"): 7}), table({(0, "kind"): 10}), table({(0, "values"): None}),
               table({(1, "offsets"): None}), table({(1, "chars"): None}), table({(2, "chars"): None}), table({(2, "values"): None}),
               table({(0, "key"): b"k" * 1025}), table({(1, "chars_bytes"): 1 << 32})]
    many = cases.arrays_of({"name": "t", "n": 1, "columns": [cases.column(b"k%d" % k, cases.BOOL, [1]) for k in range(65)]})
    long_keys = cases.arrays_of({"name": "t", "n": 1, "columns": [cases.column(bytes([k]) * 1024, cases.BOOL, [1]) for k in range(0x61, 0x69)]})  # 8 x 1 027 > 8 192
    at_the_limit = cases.arrays_of({"name": "t", "n": 1, "columns": [cases.column(bytes([k]) * 1021, cases.BOOL, [1]) for k in range(0x61, 0x69)]})  # 8 x 1 024
    calls = [(a, 0, EXACT, 1) for a in refused + [many, long_keys]] + [(good, 4, EXACT, 1), (good, 0x80000000, EXACT, 1)]
    p = subprocess.run([emu.exe], input=b"".join(blob_of(*c) for c in calls), capture_output=True, timeout=600)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-3000:]
    assert [g[0] for g in records_of(p.stdout, calls)] == [BADARG] * len(calls)
    emu([(good, 3, EXACT, 1), (at_the_limit, 0, EXACT, 1)])


def test_the_driver_runs_clean_under_the_sanitizers(tmp_path):
    """the stand-alone driver -- the host's table, kernels and launchers -- built with -fsanitize=address,undefined: the fixture's tables, both roads, bad offsets, the
    three capacities"""
    # (the runtimes linked statically: the program stands alone, whatever else the loader is told to bring in)
    exe = build(tmp_path, ("-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer", "-g"))
    calls = []
    for t in cases.fixture_tables():
        calls += three_capacities(cases.arrays_of(t, tail_ones=True), cases.NEWLINE, skew=3) + [(cases.arrays_of(t), cases.OMIT_NULLS, EXACT, 0)]
    calls += three_capacities(cases.bad_offsets()[0], cases.NEWLINE) + [(cases.bad_offsets(True)[0], 0, EXACT, 1)]
    calls += [(cases.arrays_of(cases.span_table(cases.WINDOW + d, rows_after=3)), cases.NEWLINE, EXACT, 11) for d in (0, 1)]
    calls += [(cases.arrays_of(cases.wide_table(64)), 0, EXACT, 1), (cases.arrays_of(cases.mixed_table(257)), cases.NEWLINE, EXACT, 13), (cases.arrays_of(cases.narrow_table(257)), cases.NEWLINE, EXACT, 13), (cases.arrays_of(cases.mixed_table(0)), 0, EXACT, 1)]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run_calls(exe, calls, env)
