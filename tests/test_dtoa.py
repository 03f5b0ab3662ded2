"""CPU tier: simdjson_amd/csrc/sj_dtoa.h -- binary64 bits to the reference's to_chars(double) text, host + device functions -- and the integer printers of
sj_json_text.h, built with g++ (tests/host/test_dtoa.cpp) and compared with tests/golden/json_text.json's doubles -- a table, and groups made by rule and kept as digests -- (the real reference,
tests/golden/make_json_text_golden.py); every text is read back by strtod to the same bits inside the program.  Where oracle/_ref/libsjref.so is present the program
also runs against the LIVE simdjson::internal::to_chars: two million seeded random bit patterns and all 2 046 powers of two.  The same program runs built with
-fsanitize=address,undefined."""
import os
import re
import subprocess
from fractions import Fraction

import pytest

import checkers
import json_text_cases
from simdjson_amd import _paths

CSRC = os.path.join(_paths.PKG_DIR, "csrc")
SRC = os.path.join(_paths.REPO_ROOT, "tests", "host", "test_dtoa.cpp")
LIVE_COUNT = 2000000


def build(out, extra=(), libs=()):
    exe = str(out / "test_dtoa")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function", *extra, "-I", CSRC, SRC, "-o", exe, *libs], check=True)
    return exe


def run_table(exe, doubles, env=None):
    p = subprocess.run([exe, "table"], input="".join("%016x\n" % b for b, _ in doubles), capture_output=True, text=True, env=env)
    assert p.returncode == 0 and "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-3000:]
    got = [line.split() for line in p.stdout.splitlines()]
    assert len(got) == len(doubles)
    for (bits, want), (hexbits, text) in zip(doubles, got):
        assert int(hexbits, 16) == bits and (want is None or text.encode() == want), (hex(bits), text, want)
    return [text.encode() for _, text in got]


def run_fixture(exe, env=None):
    """the fixture's explicit table text by text, its groups (tests/json_text_cases.py makes their bits by rule) by the digest of their texts"""
    _, _, doubles = json_text_cases.fixture()
    assert len(doubles) >= 200
    run_table(exe, doubles, env)
    kept = json_text_cases.fixture_double_groups()
    for name, group in json_text_cases.double_groups().items():
        assert len(group) == kept[name]["count"] and json_text_cases.group_digest(run_table(exe, [(b, None) for b in group], env)) == kept[name]["sha256"], name


INTEGERS = [("l", v & ((1 << 64) - 1)) for v in (0, 1, -1, 9, 10, -10, 99, 100, 12345, -12345, (1 << 63) - 1, -(1 << 63), -(1 << 63) + 1, 10 ** 18, -10 ** 18, 10 ** 18 - 1)]
INTEGERS += [("u", v) for v in (0, 7, 1 << 63, (1 << 64) - 1, 10 ** 19, 10 ** 19 - 1, 9223372036854775808, 18446744073709551615)]
INTEGERS += [("u", 10 ** k + d) for k in range(20) for d in (-1, 0, 1) if 0 <= 10 ** k + d < 1 << 64]


def run_integers(exe, env=None):
    p = subprocess.run([exe, "integers"], input="".join("%s %016x\n" % (t, v) for t, v in INTEGERS), capture_output=True, text=True, env=env)
    assert p.returncode == 0 and "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-3000:]
    got = [line.split() for line in p.stdout.splitlines()]
    assert len(got) == len(INTEGERS)
    for (tag, v), (t, hexbits, text) in zip(INTEGERS, got):
        assert text == str(v - (1 << 64) if tag == "l" and v >> 63 else v), (tag, v, text)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build(tmp_path_factory.mktemp("dtoa"))


def test_pow10_table_is_what_it_says():
    """entries of the generated table against exact rational arithmetic: the 128-bit ceiling of 10^k scaled to [2^127, 2^128)"""
    words = [int(x, 16) for x in re.findall(r"0x([0-9a-f]{16})ull", open(os.path.join(CSRC, "sj_pow10_table.inc")).read())]
    assert len(words) == 2 * 617
    for k in (-292, -291, -100, -28, -27, -1, 0, 1, 2, 27, 28, 38, 39, 55, 56, 200, 323, 324):
        g = (words[2 * (k + 292)] << 64) | words[2 * (k + 292) + 1]
        assert g >> 127 == 1
        v = Fraction(10) ** k
        r = next(r for r in range(-1300, 1300) if (1 << 127) <= v / Fraction(2) ** r < (1 << 128))
        assert Fraction(g - 1) < v / Fraction(2) ** r <= Fraction(g), k


def test_the_fixtures_table(exe):
    run_fixture(exe)


def test_integers(exe):
    run_integers(exe)


def test_against_the_live_reference(tmp_path):
    if not checkers.have_reference_lib():
        pytest.skip("oracle/_ref/libsjref.so is not built")
    ref_dir = os.path.dirname(_paths.LIB_REF)
    live = build(tmp_path, ("-DSJ_DTOA_LIVE",), ("-L", ref_dir, "-lsjref", f"-Wl,-rpath,{ref_dir}"))
    p = subprocess.run([live, "live", "20261019", str(LIVE_COUNT)], capture_output=True, text=True)
    assert p.returncode == 0, (p.stdout, p.stderr[-3000:])
    assert p.stdout.strip() == f"{LIVE_COUNT + 2046} compared, 0 differences"


def test_the_program_runs_clean_under_the_sanitizers(tmp_path):
    """stand-alone, the runtimes linked statically: the fixture's table and the integers"""
    san = build(tmp_path, ("-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer", "-g"))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run_fixture(san, env)
    run_integers(san, env)
