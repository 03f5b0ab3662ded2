"""CPU tier: list columns and array rows as nested JSON -- the gfx950 kernel sources of sjgpu_write.hip (k_nested_count, k_nested_fill) with the total of
sjgpu_query.hip and the scans of sjgpu_finish.hip, compiled as C++ against tests/host/emu -- run the launches of sjgpu_write_nested_device behind the host's own
table (tests/host/test_nested_emu.cpp) and are compared byte for byte with tests/nested_write_model.py and, through it, with tests/golden/nested_write.json: the
fixture's tables under every legal combination of the flags, row counts at the wave's and the workgroup's edges, field counts up to the interface's 64, list offsets
from a base, the validity word's edge inside a list, garbage under an invalid list, bad lists and bad elements, every edge of the fill's grouping at every alignment
of the output -- through the product's kernels and through a build with -DSJGPU_NESTED_SPLIT --, the row shapes, the refusals, parity with the plain writer, and the three capacities.  The driver also runs built with -fsanitize=address,undefined
(a stand-alone program: nothing is loaded into Python)."""
import os
import struct
import subprocess

import numpy as np
import pytest

import nested_write_cases as cases
import nested_write_model as model
import write_records_cases as plain_cases
import write_records_model as plain_model
from simdjson_amd import _paths

CSRC = os.path.join(_paths.PKG_DIR, "csrc")
EMU = os.path.join(_paths.REPO_ROOT, "tests", "host", "emu")
KERNEL_TUS = ("sjgpu_write", "sjgpu_query", "sjgpu_finish")
EXACT, ONE_SHORT, NONE = 0, 1, 2
OVERFLOW, BADARG = -5, -4
NEWLINE, OMIT_NULLS, ARRAY_ROWS, BARE = cases.NEWLINE, cases.OMIT_NULLS, cases.ARRAY_ROWS, cases.BARE


def build(out, sanitize=(), defines=()):
    """the way tests/test_write_emu.py builds its units; defines: build macros for the kernel sources"""
    sanitize = (*sanitize, *defines)
    inc = ["-I", EMU, "-I", _paths.INCLUDE_DIR, "-I", CSRC]
    jobs = []
    for name in KERNEL_TUS:
        jobs.append(subprocess.Popen(["g++", "-std=c++17", "-O2", *sanitize, "-Wno-attributes", "-Wno-unknown-pragmas", "-x", "c++", *inc, "-c", os.path.join(CSRC, name + ".hip"),
                                      "-o", str(out / (name + ".o"))]))
    jobs.append(subprocess.Popen(["g++", "-std=c++17", "-O2", *sanitize, *inc, "-c", os.path.join(EMU, "sj_emu.cpp"), "-o", str(out / "sj_emu.o")]))
    jobs.append(subprocess.Popen(["g++", "-std=c++17", "-O2", *sanitize, "-Wno-attributes", *inc, "-c", os.path.join(_paths.REPO_ROOT, "tests", "host", "test_nested_emu.cpp"),
                                  "-o", str(out / "driver.o")]))
    assert all(j.wait() == 0 for j in jobs)
    exe = str(out / "test_nested_emu")
    subprocess.run(["g++", *sanitize, *[str(out / (f + ".o")) for f in (*KERNEL_TUS, "sj_emu", "driver")], "-lpthread", "-o", exe], check=True)
    return exe


def blob_of(arrays, flags, capacity=EXACT, skew=1):
    n, out = arrays["n"], [struct.pack("<IIIII", arrays["n"], len(arrays["fields"]), flags, capacity, skew)]
    for f in arrays["fields"]:
        chars = b"" if f["chars"] is None else np.ascontiguousarray(f["chars"], np.uint8).tobytes()
        listed = f["list_offsets"] is not None
        m = f["elements"] if listed else n
        key = f["key"] if f["key"] is not None else b""
        out.append(struct.pack("<I", len(key)) + key + struct.pack("<I", f["kind"]) +
                   bytes([f["values"] is not None, f["valid"] is not None, f["offsets"] is not None, f["chars"] is not None, listed, f["list_valid"] is not None, 0, 0]) +
                   struct.pack("<QQQ", f["chars_bytes"], len(chars), f["elements"]))
        for name, dtype, count in (("values", np.uint64, m), ("valid", np.uint64, (m + 63) // 64), ("offsets", np.uint32, m + 1)):
            if f[name] is not None:
                assert len(f[name]) == count, (name, len(f[name]), count)
                out.append(np.ascontiguousarray(f[name], dtype).tobytes())
        out.append(chars)
        if listed:
            assert len(f["list_offsets"]) == n + 1
            out.append(np.ascontiguousarray(f["list_offsets"], np.uint32).tobytes())
        if f["list_valid"] is not None:
            assert len(f["list_valid"]) == (n + 63) // 64
            out.append(np.ascontiguousarray(f["list_valid"], np.uint64).tobytes())
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
        counts = np.frombuffer(out, np.uint64, 6, at)
        at += 48
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
    exe = build(tmp_path_factory.mktemp("nested_emu"))

    def run(calls):
        return run_calls(exe, calls)
    run.exe = exe
    return run


@pytest.fixture(scope="module")
def emu_split(tmp_path_factory):
    """the same driver over the kernel sources with -DSJGPU_NESTED_SPLIT: the groups of 128, 64 and 32 rows, which the product compiles out"""
    exe = build(tmp_path_factory.mktemp("nested_emu_split"), defines=("-DSJGPU_NESTED_SPLIT",))
    return lambda calls: run_calls(exe, calls)


def three_capacities(arrays, flags, skew=1):
    return [(arrays, flags, cap, skew) for cap in (NONE, ONE_SHORT, EXACT)]


def test_the_fixture_tables(emu):
    """every table of the fixture under every legal combination of the flags: row by row the reference's text; list offsets from 0 and from a base"""
    fixture = cases.fixture()
    for t in cases.fixture_tables():
        flags_list = cases.legal_flags(len(t["fields"]))
        for lead in (0, 5):
            arrays = cases.arrays_of(t, tail_ones=True, lead=lead)
            assert all(f["list_offsets"] is None or (int(f["list_offsets"][0]) == lead and int(f["list_offsets"][-1]) == f["elements"]) for f in arrays["fields"])
            wants = emu([(arrays, flags, EXACT, 3) for flags in flags_list] + three_capacities(arrays, NEWLINE)[:2])
            for flags, (offsets, chars, status, _) in zip(flags_list, wants):
                cases.assert_rows_are_the_fixtures(fixture[t["name"]][flags], cases.split(offsets, chars), (t["name"], flags))


@pytest.mark.parametrize("n", plain_cases.ROW_COUNTS)
def test_rows_at_the_wave_and_workgroup_edges(emu, emu_split, n):
    """nine fields, lists among them, whose 256 rows do not fit the window (direct; split in the build that has the split); two whose 256 rows fit it at once"""
    emu_split(three_capacities(cases.arrays_of(cases.mixed_table(n), tail_ones=True, lead=1), NEWLINE))
    arrays, narrow = cases.arrays_of(cases.mixed_table(n), tail_ones=True, lead=1), cases.arrays_of(cases.narrow_table(n), tail_ones=True)
    wants = emu(three_capacities(arrays, NEWLINE) + [(arrays, OMIT_NULLS, EXACT, 9), (arrays, ARRAY_ROWS | NEWLINE, EXACT, 4)] + three_capacities(narrow, NEWLINE) +
                [(narrow, 0, EXACT, 6)])
    assert len(wants[0][0]) == n + 1 and (n < 40 or (wants[0][3][3] > 0 and wants[0][3][5] > 0))
    if n >= cases.ROWS_PER_STEP:
        assert cases.group_rows(wants[0][0], 0) in (128, 64) and cases.group_rows(wants[5][0], 0) == 256
    if n == 0:
        assert wants[0][0].tolist() == [0] and wants[0][3].tolist() == [0] * 6


@pytest.mark.parametrize("K", plain_cases.COLUMN_COUNTS)
def test_field_counts(emu, K):
    arrays = cases.arrays_of(cases.wide_table(K), lead=3)
    wants = emu([(arrays, flags, EXACT, 5) for flags in cases.legal_flags(K)] + three_capacities(arrays, 0)[:2])
    if K == 0:
        assert wants[2][1] == b"{}\n" * 70 and wants[0][1] == b"{}" * 70 and wants[4][1] == b"[]" * 70 and wants[5][1] == b"[]\n" * 70


def test_the_validity_words_edge_inside_one_list_and_garbage_under_an_invalid_list(emu):
    """the lists of 63, 64 and 65 elements of the fixture's table moved by every lead from 0 to 2: elements 63, 64 and 65 lie inside one list, on both sides of a
    validity word; the offset between the table's two invalid lists is 0xFFFFFFF0 and nobody reads it"""
    t = cases._lengths()
    for lead in (0, 1, 2):
        arrays = cases.arrays_of(t, lead=lead)
        assert all(int(f["list_offsets"][7]) == cases.GARBAGE for f in arrays["fields"])
        offsets, chars, status, counts = emu(three_capacities(arrays, NEWLINE | OMIT_NULLS))[0]
        assert not status.any() and counts.tolist()[2] == 2 * 4


def test_bad_lists_are_status_19_and_a_validity_bit_of_0_hides_them(emu):
    arrays, bad = cases.bad_lists()
    for flags in (0, NEWLINE | OMIT_NULLS, ARRAY_ROWS):
        offsets, chars, status, counts = emu(three_capacities(arrays, flags))[0]
        assert [r for r in range(arrays["n"]) if status[r]] == bad and set(status[bad].tolist()) == {19} and all(offsets[r] == offsets[r + 1] for r in bad)
        assert counts.tolist()[:2] == [arrays["n"] - len(bad), len(bad)]
    offsets, chars, status, counts = emu([(cases.hidden_bad_lists(), 0, EXACT, 1)])[0]
    assert not status.any() and counts.tolist()[:3] == [10, 0, 2]


def test_doubles_without_a_text_are_null_elements(emu):
    inf, nan = 0x7FF0000000000000, 0x7FF8000000000ABC
    t = {"name": "t", "n": 3, "fields": [cases.list_field(b"d", cases.DOUBLE, [[cases.bits_of(1.5), inf, None], [nan], []]), cases.column(b"p", cases.DOUBLE, [nan, 0, inf])]}
    wants = emu([(cases.arrays_of(t), flags, EXACT, 1) for flags in (0, OMIT_NULLS, ARRAY_ROWS)])
    assert wants[0][1] == b'{"d":[1.5,null,null],"p":null}{"d":[null],"p":0.0}{"d":[],"p":null}' and wants[1][1] == b'{"d":[1.5,null,null]}{"d":[null],"p":0.0}{"d":[]}'
    assert wants[2][1] == b"[[1.5,null,null],null][[null],0.0][[],null]" and all(w[3].tolist() == [3, 0, 2, 4, 4, 3] for w in wants)


@pytest.mark.parametrize("name", list(cases.grouping_cases()))
def test_the_edges_of_the_grouping(emu, emu_split, name):
    """the span of 256 rows, of 128, of 64 and of 32 at the window and one byte beyond it, at the first and the last alignment of the output: through the product's
    kernels (256 rows or direct) and through the build with the split"""
    t, group = cases.grouping_cases()[name]
    arrays = cases.arrays_of(t)
    for run in (emu, emu_split):
        wants = run([(arrays, NEWLINE, EXACT, 0), (arrays, NEWLINE, EXACT, 15), (arrays, NEWLINE, ONE_SHORT, 0)])
    assert cases.group_rows(wants[0][0], 0) == group


def test_a_long_row_between_staged_neighbours(emu):
    """one row of more than the window of list text: its iteration takes the direct road, the iterations on either side of it the staged one"""
    t = cases.long_row_table(cases.WINDOW + 300)
    offsets = emu(three_capacities(cases.arrays_of(t), NEWLINE, skew=7))[0][0]
    assert [cases.group_rows(offsets, r) for r in range(0, t["n"], cases.ROWS_PER_STEP)] == [256, 0, 256, 256]


def test_every_alignment_of_the_output_on_a_split_case(emu, emu_split):
    arrays = cases.arrays_of(cases.grouping_cases()["64-row groups fit, a 128-row group does not"][0])
    mixed = cases.arrays_of(cases.mixed_table(300))
    emu([(arrays, NEWLINE, EXACT, skew) for skew in range(16)] + [(mixed, NEWLINE, EXACT, skew) for skew in range(16)])
    wants = emu_split([(arrays, NEWLINE, EXACT, skew) for skew in range(16)] + [(mixed, NEWLINE, EXACT, skew) for skew in range(16)])
    assert cases.group_rows(wants[16][0], 0) in (128, 64)


def test_bare_rows_and_the_empty_rows_between_them(emu):
    t = cases._bare_strings()
    wants = emu([(cases.arrays_of(t), flags, EXACT, 2) for flags in (BARE, BARE | NEWLINE, BARE | OMIT_NULLS, BARE | OMIT_NULLS | NEWLINE)])
    assert wants[1][1] == b'["a","\\"",null]\nnull\n[]\nnull\nnull\n["zzzzzzzzzzzzzzzzzzzz"]\n' and wants[3][1] == b'["a","\\"",null]\n[]\n["zzzzzzzzzzzzzzzzzzzz"]\n'
    assert np.diff(wants[3][0].astype(np.int64)).tolist() == [16, 0, 3, 0, 0, 25] and not wants[3][2].any() and wants[3][3].tolist() == [6, 0, 3, 0, 4, 1]


def test_parity_with_the_plain_writer(emu):
    """a table with no list field and no new flag: byte for byte, offset for offset and count for count what the plain writer's model gives for the same columns"""
    for t in (plain_cases.mixed_table(257), plain_cases._every_kind(), plain_cases._keys()):
        fields = {"name": t["name"], "n": t["n"], "fields": t["columns"]}
        arrays = cases.arrays_of(fields, tail_ones=True)
        wants = emu([(arrays, flags, EXACT, 1) for flags in plain_cases.ALL_FLAGS])
        for flags, want in zip(plain_cases.ALL_FLAGS, wants):
            offsets, chars, status, counts = plain_model.records(cases.as_plain_arrays(arrays), flags)
            assert chars == want[1] and np.array_equal(offsets, want[0]) and np.array_equal(status, want[2]) and counts.tolist() == want[3].tolist()[:4]
            assert want[3].tolist()[4:] == [0, 0]


def test_the_refusals(emu):
    """every SJGPU_E_BADARG the host's table decides, with nothing written (the driver checks the poison)"""
    def table(changes=(), K=None):
        arrays = cases.arrays_of({"name": "t", "n": 4, "fields": [cases.list_field(b"a", cases.INT64, [[1], None, [3, None], []]),
                                                                  cases.list_field(b"s", cases.STRING, [[b"x"]] * 4), cases.list_field(b"c", cases.STRING_CELLS, [[b"y"]] * 4),
                                                                  cases.column(b"p", cases.INT64, [1, 2, None, 4])][:K]})
        for (k, field), v in dict(changes).items():
            arrays["fields"][k][field] = v
        return arrays
    good, one = table(), table(K=1)
    refused = [(table({(0, "kind"): 0}), 0), (table({(0, "kind"): 6}), 0), (table({(0, "kind"): 7}), 0), (table({(0, "kind"): 10}), 0), (table({(0, "values"): None}), 0),
               (table({(1, "offsets"): None}), 0), (table({(1, "chars"): None}), 0), (table({(2, "chars"): None}), 0), (table({(2, "values"): None}), 0),
               (table({(3, "values"): None}), 0), (table({(0, "key"): b"k" * 1025}), 0), (table({(1, "chars_bytes"): 1 << 32}), 0),
               (good, 16), (good, 0x80000000), (good, ARRAY_ROWS | OMIT_NULLS), (good, ARRAY_ROWS | BARE), (one, ARRAY_ROWS | BARE), (good, BARE), (table(K=0), BARE),
               (table(K=2), BARE | NEWLINE)]
    calls = [(a, flags, EXACT, 1) for a, flags in refused]
    p = subprocess.run([emu.exe], input=b"".join(blob_of(*c) for c in calls), capture_output=True, timeout=600)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-3000:]
    assert [g[0] for g in records_of(p.stdout, calls)] == [BADARG] * len(calls)
    # what is NOT refused: keys nobody looks at (too long, or none at all), the element arrays of a field without elements, every legal combination of the flags
    long_keys = table({(0, "key"): b"k" * 5000, (1, "key"): b"", (2, "key"): b"q" * 9000})
    empty = cases.arrays_of({"name": "t", "n": 3, "fields": [cases.list_field(b"e", cases.STRING, [[], None, []])]})
    for name in ("values", "valid", "offsets", "chars"):
        empty["fields"][0][name] = None
    emu([(long_keys, ARRAY_ROWS, EXACT, 1), (empty, 0, EXACT, 1), (empty, BARE | OMIT_NULLS | NEWLINE, EXACT, 1)] + [(good, f, EXACT, 1) for f in cases.legal_flags(4)] +
        [(one, f, EXACT, 1) for f in cases.legal_flags(1)])


def test_the_driver_runs_clean_under_the_sanitizers(tmp_path):
    """the stand-alone driver -- the host's table, kernels and launchers -- built with -fsanitize=address,undefined: the fixture's tables, every road of the fill, bad
    lists, the row shapes, the three capacities"""
    # (the runtimes linked statically: the program stands alone, whatever else the loader is told to bring in)
    exe = build(tmp_path, ("-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer", "-g"))
    calls = []
    for t in cases.fixture_tables():
        arrays = cases.arrays_of(t, tail_ones=True, lead=2)
        calls += three_capacities(arrays, NEWLINE, skew=3) + [(arrays, f, EXACT, 0) for f in cases.legal_flags(len(t["fields"]))[1:]]
    calls += three_capacities(cases.bad_lists()[0], NEWLINE) + [(cases.hidden_bad_lists(), 0, EXACT, 1)]
    calls += [(cases.arrays_of(t), NEWLINE, EXACT, 11) for t, _ in cases.grouping_cases().values()]
    calls += [(cases.arrays_of(cases.wide_table(64)), 0, EXACT, 1), (cases.arrays_of(cases.mixed_table(257)), NEWLINE, EXACT, 13),
              (cases.arrays_of(cases.narrow_table(257)), NEWLINE, EXACT, 13), (cases.arrays_of(cases.mixed_table(0)), 0, EXACT, 1),
              (cases.arrays_of(cases.long_row_table(cases.WINDOW + 300)), NEWLINE, EXACT, 5)]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run_calls(exe, calls, env)
