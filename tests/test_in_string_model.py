"""CPU tier: the rules of numbers held in strings, three times over.  tests/in_string_model.py (regular expressions, Python's integers, Python's float()) is pinned
against tests/golden/in_string.json, the real reference's answers, entry by entry; the contents that need an escape in a document -- which the fixture cannot
hold, because On-Demand reads the raw text -- get the documented answers from the model alone; under SJGPU_GETS_OR_NUMBER number cells get what tests/cast_model.py
gives them; and simdjson_amd/csrc/sj_number_in_string.h, as the host compiler sees it (tests/host/test_number_in_string.cpp, built with
-fsanitize=address,undefined), answers the fixture and agrees with strtoll, strtoull and strtod on a million random decimals."""
import os
import struct
import subprocess

import numpy as np
import pytest

import cast_model
import in_string_cases as cases
import in_string_model as model
from simdjson_amd import _paths


def test_the_model_gives_the_references_answers():
    fixture = model.load_fixture()
    assert len(fixture) > 400 and os.path.getsize(model.FIXTURE) < 256 << 10
    kinds = set()
    for content, answers in fixture:
        assert not any(b in (0x22, 0x5C) or b < 0x20 for b in content) and content.decode("utf-8") is not None  # its own raw JSON form
        for g, want in zip((model.INT64, model.UINT64, model.DOUBLE), answers):
            assert model.answer(content, g) == want, (g, content[:60])
            kinds.add((g, want[0]))
    assert kinds == {(g, c) for g in (1, 2, 3) for c in (0, 9, 17)}
    assert any(len(c) > 800 for c, _ in fixture) and any(max(c, default=0) >= 0x80 for c, _ in fixture)


def test_the_issues_table():
    """the differences from a number token, spelled out (each is in the fixture, too)"""
    table = {b"12": ((0, 12), (0, 12), (0, 0x4028000000000000)), b"-0": ((0, 0), (17, 0), (0, 1 << 63)), b"01": ((9, 0),) * 3, b"": ((17, 0),) * 3, b"+1": ((17, 0),) * 3,
             b".5": ((17, 0),) * 3, b"NaN": ((17, 0),) * 3, b"1 ": ((9, 0),) * 3, b"1.": ((9, 0),) * 3, b"1e+": ((9, 0),) * 3, b"1.5": ((9, 0), (9, 0), (0, 0x3FF8000000000000)),
             b"18446744073709551615": ((17, 0), (0, (1 << 64) - 1), (0, 0x43F0000000000000)), b"18446744073709551616": ((17, 0), (17, 0), (0, 0x43F0000000000000)),
             b"-9223372036854775808": ((0, 1 << 63), (17, 0), (0, 0xC3E0000000000000)), b"1" * 23: ((17, 0), (17, 0), (0, 0x4482D2AD2372ED4D)),
             b"0" * 23: ((17, 0), (17, 0), (9, 0)), b"1e00000000000000000001": ((9, 0),) * 3, b"1e-9999999999999999999": ((9, 0), (9, 0), (0, 0)),
             b"-1e-999": ((9, 0), (17, 0), (0, 1 << 63)), b"1e309": ((9, 0),) * 3, b"2.4703282292062327e-324": ((9, 0), (9, 0), (0, 0)),
             b"2.4703282292062328e-324": ((9, 0), (9, 0), (0, 1))}
    held = dict(model.load_fixture())
    for content, want in table.items():
        assert tuple(model.answer(content, g) for g in (1, 2, 3)) == want == tuple(held[content]), content


def test_contents_that_need_an_escape():
    """a `"`, a backslash or a control byte behind the digits is an ordinary byte that is no digit: NUMBER_ERROR, where On-Demand would have ended the string at the quote.
    In front of the digits: INCORRECT_TYPE"""
    for content in (b'12"', b"1\\", b"12\x01", b"1\t", b"12\x00"):
        assert [model.answer(content, g) for g in (1, 2, 3)] == [(9, 0)] * 3, content
    assert [model.answer(b'"12', g) for g in (1, 2, 3)] == [(17, 0)] * 3
    assert set(cases.ESCAPED) >= {b'12"', b"1\\", b"12\x01"}  # (the kernels meet them in tests/test_cast_strings_emu.py and tests/test_gpu_cast_strings.py)


def test_number_cells_under_the_flag_are_the_casts():
    rng = np.random.default_rng(181)
    sbuf, words = cases.string_buffer(cases.pool())
    tags, values = cases.random_cells(rng, 4097, 6, words, len(sbuf))
    value_out, code, valid, counts, parked = model.cast(tags, values, sbuf, model.ALL_GETTERS)
    numbers = np.isin(tags, np.frombuffer(b"lud", np.uint8))
    assert numbers.sum() > 1000
    for k, g in enumerate(model.ALL_GETTERS):
        want_value, want_code = cast_model.cast_row(tags[k], values[k], g & 0x0F)
        if g & model.OR_NUMBER:
            assert np.array_equal(code[k][numbers[k]], want_code[numbers[k]]) and np.array_equal(value_out[k][numbers[k]], want_value[numbers[k]])
            assert 18 in code[k][numbers[k]] or g & 0x0F == model.DOUBLE
        else:
            assert (code[k][numbers[k]] == 17).all() and not value_out[k][numbers[k]].any()
        held = (tags[k] >= 1) & (tags[k] <= 33)
        assert np.array_equal(code[k][held], tags[k][held])
    assert not parked[[0, 1, 3, 4]].any() and parked[2].any()


@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("number_in_string") / "test_number_in_string")
    subprocess.run(["g++", "-std=c++17", "-O2", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-I",
                    os.path.join(_paths.PKG_DIR, "csrc"), "-I", _paths.INCLUDE_DIR, os.path.join(_paths.REPO_ROOT, "tests", "host", "test_number_in_string.cpp"), "-o", exe], check=True)
    return exe


def test_the_rules_header_gives_the_references_answers(rules):
    contents = [c for c, _ in model.load_fixture()] + cases.ESCAPED + cases.SHORT + cases.long_decimals()
    blob = struct.pack("<I", len(contents)) + b"".join(struct.pack("<I", len(c)) + c for c in contents)
    p = subprocess.run([rules, "answers"], input=blob, capture_output=True, timeout=600)
    assert p.returncode == 0 and b"runtime error" not in p.stderr and b"AddressSanitizer" not in p.stderr, p.stderr.decode(errors="replace")[-3000:]
    lines = p.stdout.decode().splitlines()
    assert len(lines) == len(contents)
    for content, line in zip(contents, lines):
        got = [(int(a[2:]), 0) if a[0] == "E" else (0, int(a, 16)) for a in line.split(";")]
        assert got == [model.answer(content, g) for g in (1, 2, 3)], content[:60]


def test_the_rules_header_against_the_c_library_on_a_million_random_decimals(rules):
    p = subprocess.run([rules, "random", "1000000", "20261021"], capture_output=True, timeout=1200)
    assert p.returncode == 0 and b"runtime error" not in p.stderr and b"AddressSanitizer" not in p.stderr, (p.stdout + p.stderr).decode(errors="replace")[-3000:]
    assert b"1000000 contents, 0 differences" in p.stdout
