#!/usr/bin/env python3
"""Generates tests/golden/in_string.json from the REAL reference: what ondemand::value::get_int64_in_string(), get_uint64_in_string() and
get_double_in_string() answer for the one element of `["c"]`, for every content c below (the yardstick of sjgpu_cast_string_cells_device,
include/sjgpu_cast_strings.h).

Run where the reference lies (needs its headers and oracle/_ref/libsjref.so):   python tests/golden/make_in_string_golden.py

tests/golden/in_string_golden.cpp -- a small program of our own -- is compiled against them into a temporary directory and fed the list.
Every content must be its own raw JSON form (valid UTF-8, no `"`, no backslash, no byte below 0x20): then the raw text On-Demand parses and the
unescaped string a DOM holds are the same bytes, and no entry has to be left out of a comparison.
The fixture: "getters" (the order of the answers), "contents" as hex, "answers"[i]: three answers joined by `;`, each "E <code>" or 16 hex digits
(the 64 bits of the int64 / uint64 / double).
"""
import json
import os
import struct
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from simdjson_amd import _paths  # noqa: E402

GETTERS = ["int64", "uint64", "double"]
I63, I64 = 1 << 63, 1 << 64


def halfway(digits, odd):
    """an integer of `digits` decimal digits that lies exactly half way between two neighbouring doubles; odd: the one below has an odd significand
    (the tie goes up), else an even one (down)"""
    e = (10 ** digits - 1).bit_length() - 53  # the doubles at the top of this range are multiples of 2^e
    m = ((10 ** digits - 1) >> e) - 7         # a significand of 53 bits there
    m -= (m & 1) != int(odd)
    mid = (2 * m + 1) << (e - 1)
    assert len(str(mid)) == digits and m.bit_length() == 53 and e >= 1, (digits, mid)
    return mid


def contents():
    c = []
    # the issue's table
    c += ["12", "-0", "01", "", "-", "+1", " 1", ".5", "NaN", "Infinity", "-Infinity", "nan", "inf", "1 ", "1x", "1.", "1e", "1e+", "1e-", "1.5", "1e2", "-1.5", "1E2", "1.5e+2",
          "1.e2", "1.5x", "1e2x", "-", "--1", "-x", "0", "-1", "1", "00", "-01", "0.0", "-0.0", "0.", "0e0", "0x10", "1,5", "1_000", "0.1", "-0.1e-1", "123456789",
          "18446744073709551615", "18446744073709551616", "9223372036854775808", "-9223372036854775808", "1" * 23, "0" * 23, "-" + "0" * 23, "0" * 19, "0" * 20, "0" * 21,
          "1e00000000000000000001", "1e9999999999999999999", "1e-9999999999999999999", "-1e-999", "0e99999", "-0e99999", "0e9999999999999999999", "0.0e-9999999999999999999",
          "1e308", "1e309", "1e400", "-1e309", "1e-400", "2.4703282292062327e-324", "2.4703282292062328e-324", "1234567890123456789012345678901234567890e-20"]
    # every integer limit plus or minus 1, both signs
    for v in (I63 - 1, I63, I64 - 1, I64):
        for d in (-1, 0, 1):
            c += [str(v + d), "-" + str(v + d)]
    # 19, 20 and 21 digits with the leading digits 1 and 2, and all nines
    for digits in (18, 19, 20, 21, 22):
        for lead in ("1", "2", "9"):
            body = lead + ("9" if lead == "9" else "0") * (digits - 1)
            c += [body, "-" + body, body[:-1] + "7"]
    c += ["10000000000000000000", "19999999999999999999", "18446744073709551609", "17999999999999999999", "09223372036854775807", "0" + "1" * 19, "0" + "1" * 20,
          "1" * 19 + ".", "1" * 19 + "x", "1" * 20 + "x", "1" * 21 + "x", "-" + "1" * 19 + "x", "-" + "1" * 20 + "x", "9223372036854775807.0", "9223372036854775807e0"]
    # 2^53 plus or minus 1, as integers and with a fraction or an exponent
    for v in ((1 << 53) - 1, 1 << 53, (1 << 53) + 1):
        c += [str(v), "-" + str(v), str(v) + ".0", str(v) + "e0", str(v) + "00e-2"]
    # exact halfway decimals of 17 to 40 digits, the tie going either way, and their neighbours; some with a fraction or an exponent behind them
    for digits in range(17, 41):
        for odd in (False, True):
            mid = halfway(digits, odd)
            c += [str(mid), str(mid - 1), str(mid + 1)]
            if digits % 4 == 1:
                c += [str(mid) + ".0", str(mid) + "." + "0" * 30 + "1", "-" + str(mid), str(mid) + "e-" + str(digits), str(mid) + "000e-3", str(mid)[0] + "." + str(mid)[1:] + "e" + str(digits - 1)]
    # the subnormal limits: half the smallest subnormal exactly (752 significant digits), just above it, the smallest subnormal, the largest, the smallest normal
    half_min = "0." + str(5 ** 1075).rjust(1075, "0")
    c += [half_min, half_min[:-1] + "6", half_min + "0001", "-" + half_min, "4.9406564584124654e-324", "4.9e-324", "5e-324", "3e-324", "2e-324", "2.2250738585072009e-308",
          "2.2250738585072011e-308", "2.2250738585072014e-308", "2.2250738585072012e-308", "0." + "0" * 323 + "49406564584124654"]
    # DBL_MAX, the midpoint to its successor (a tie that goes up, to infinity), the integer below that midpoint
    top_mid = ((1 << 54) - 1) << 970
    c += ["1.7976931348623157e308", "1.7976931348623158e308", "1.7976931348623159e308", "-1.7976931348623159e308", str(top_mid), str(top_mid - 1), str(top_mid + 1),
          str(((1 << 53) - 1) << 971), "179769313486231570000000000000000000000e270", "17976931348623158" + "0" * 292]
    # exponents of 18, 19 and 20 digits, with and without leading zeros
    for lead, rest in (("0", "1"), ("0", "2"), ("1", "0"), ("9", "9")):
        for digits in (18, 19, 20):
            body = lead * (digits - 1) + rest
            c += ["1e" + body, "1e-" + body, "1e+" + body, "0e" + body, "1.5E" + body]
    c += ["1e9223372036854775807", "1e9223372036854775808", "1e-9223372036854775808", "0.1e9223372036854775808", "1e0000000000000000308", "1e0000000000000000309",
          "1e-0000000000000000324", "10e-0000000000000000324", "1e000000000000000022"]
    # a fraction of 400 zeros with e400, its neighbours, and a long integer part with a matching negative exponent
    c += ["0." + "0" * 400 + "1e400", "0." + "0" * 400 + "125e401", "-0." + "0" * 400 + "1e401", "0." + "0" * 400 + "1e-1", "1" + "0" * 400 + "e-400", "1" + "0" * 400,
          "0." + "0" * 400, "0." + "0" * 400 + "e400"]
    # 800 digits; more than the 800 the exact comparison keeps, where only the last digit makes it more than a tie
    c += ["1" * 800, "1" * 800 + "e-500", "0." + "1" * 800, "3" * 799 + "4e-1100", str(halfway(40, False)) + "0" * 800 + "1", str(halfway(40, False)) + "." + "0" * 800]
    # 20 significant digits written in every way that still fits a short window, 19 significant digits behind leading zeros
    c += ["12345678901234567890", "1234567890.1234567890", "0.12345678901234567890", "1.2345678901234567890e10", "0.0001234567890123456789", "0.00012345678901234567891",
          "1234567890123456789e5", "12345678901234567890e5", "9007199254740993.000000000000001", "0.000000000000000000000000000001"]
    # content that is no ASCII
    c += ["١٢٣", "12 ", "1２", "€", "1 ", "é1", "12é"]
    seen, out = set(), []
    for x in c:
        b = x.encode("utf-8")
        assert not any(ch in (0x22, 0x5C) or ch < 0x20 for ch in b), x  # its own raw JSON form
        if b not in seen:
            seen.add(b)
            out.append(b)
    return out


def main():
    ref_inc = os.path.join(_paths.REFERENCE_DIR, "include")
    ref_dir = os.path.dirname(_paths.LIB_REF)
    values = contents()
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "in_string_golden")
        subprocess.run(["g++", "-O1", "-std=c++17", "-DSIMDJSON_THREADS_ENABLED=1", "-I", ref_inc, os.path.join(HERE, "in_string_golden.cpp"), "-o", exe,
                        "-L", ref_dir, "-lsjref", "-lpthread", f"-Wl,-rpath,{ref_dir}"], check=True)
        blob = struct.pack("<I", len(values)) + b"".join(struct.pack("<I", len(x)) + x for x in values)
        lines = subprocess.run([exe], input=blob, capture_output=True, check=True).stdout.decode().splitlines()
    assert len(lines) == len(values) and not any("P" in line for line in lines), [v for v, line in zip(values, lines) if "P" in line]
    out = {"getters": GETTERS, "contents": [x.hex() for x in values], "answers": lines}
    path = os.path.join(HERE, "in_string.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    kinds = {}
    for line in lines:
        for g, a in zip(GETTERS, line.split(";")):
            key = g + " " + (a if a[0] == "E" else "value")
            kinds[key] = kinds.get(key, 0) + 1
    print(len(values), "contents,", os.path.getsize(path), "bytes;", dict(sorted(kinds.items())))


if __name__ == "__main__":
    main()
