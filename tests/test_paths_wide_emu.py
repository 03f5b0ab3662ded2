"""CPU tier: the wide road of the paths over tapes -- the gfx950 kernel sources of sjgpu_query.hip and the scans of sjgpu_finish.hip, compiled as C++
against tests/host/emu -- run launch_paths_wide, the whole level loop of sjgpu_at_paths_wide_device (tests/host/test_paths_wide_emu.cpp), over tapes the
oracle built document by document, laid out as the document table says, and are compared match for match with tests/path_model.py: what
tests/test_paths_emu.py asks of the narrow road, then what only the wide road can get wrong -- numbers whose second word looks like a tag, in runs that
cross every share of the annotation, and the key / value parity of an object's children."""
import os
import struct
import subprocess

import numpy as np
import pytest

import checkers
import path_cases
import pointer_model
import query_cases
import stream_cases
from simdjson_amd import _paths

CSRC = os.path.join(_paths.PKG_DIR, "csrc")
EMU = os.path.join(_paths.REPO_ROOT, "tests", "host", "emu")
KERNEL_TUS = ("sjgpu_query", "sjgpu_finish")


def build(out):
    """the way tests/test_paths_emu.py builds its units"""
    inc = ["-I", EMU, "-I", _paths.INCLUDE_DIR, "-I", CSRC]
    jobs = []
    for name in KERNEL_TUS:
        jobs.append(subprocess.Popen(["g++", "-std=c++17", "-O1", "-Wno-attributes", "-Wno-unknown-pragmas", "-x", "c++", *inc, "-c",
                                      os.path.join(CSRC, name + ".hip"), "-o", str(out / (name + ".o"))]))
    jobs.append(subprocess.Popen(["g++", "-std=c++17", "-O2", *inc, "-c", os.path.join(EMU, "sj_emu.cpp"), "-o", str(out / "sj_emu.o")]))
    jobs.append(subprocess.Popen(["g++", "-std=c++17", "-O2", "-Wno-attributes", *inc, "-c",
                                  os.path.join(_paths.REPO_ROOT, "tests", "host", "test_paths_wide_emu.cpp"), "-o", str(out / "driver.o")]))
    assert all(j.wait() == 0 for j in jobs)
    exe = str(out / "test_paths_wide_emu")
    subprocess.run(["g++", *[str(out / (f + ".o")) for f in (*KERNEL_TUS, "sj_emu", "driver")], "-lpthread", "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def orc():
    return checkers.Oracle()


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build(tmp_path_factory.mktemp("paths_wide_emu"))


@pytest.fixture(scope="module")
def emu(exe, orc):

    def run(docs, paths, parsed=None):
        """-> (the model's column, the stream's strings); everything the driver wrote is compared with the model here.  parsed: the oracle's (tape, sbuf) of
        every document, where the caller has looked at them already"""
        if parsed is None:
            parsed = []
            for d in docs:
                err, tape, sbuf = orc.dom_parse(d)
                assert err == 0, d[:100]
                parsed.append((tape, sbuf))
        tape, sbuf, table = query_cases.lay_out(parsed)
        lens = np.array([len(p) for p in paths], np.uint32)
        blob = (struct.pack("<IQQ", len(docs), len(tape), len(sbuf)) + tape.tobytes() + sbuf.tobytes() + table.tobytes() + struct.pack("<I", len(paths)) + lens.tobytes() +
                b"".join(paths))
        p = subprocess.run([exe], input=blob, capture_output=True, timeout=1500)
        assert p.returncode == 0, p.stderr.decode(errors="replace")[-3000:]
        out, cells = p.stdout, len(docs) * len(paths)
        matches = struct.unpack_from("<Q", out, 0)[0]
        at = 8
        status = np.frombuffer(out, np.uint8, cells, at).reshape(len(paths), len(docs))
        at += cells
        offsets = np.frombuffer(out, np.uint32, cells + 1, at)
        at += 4 * (cells + 1)
        tags = np.frombuffer(out, np.uint8, matches, at)
        at += matches
        values = np.frombuffer(out, np.uint64, matches, at)
        at += 8 * matches
        want = path_cases.model_column([(t.tolist(), s.tobytes()) for t, s in parsed], paths)
        assert matches == len(want[2]) == int(offsets[-1])
        path_cases.assert_column((status, offsets, tags, values), want)
        path_cases.check_container_matches(tags, values, tape)
        # the gather over the flattened column: one string slice per match
        strings = [pointer_model.string_of(sbuf, int(v)) if t == ord('"') else b"" for t, v in zip(tags, values)]
        total = struct.unpack_from("<Q", out, at)[0]
        goffsets = np.frombuffer(out, np.uint32, matches + 1, at + 8)
        chars = out[at + 8 + 4 * (matches + 1): at + 8 + 4 * (matches + 1) + total]
        at += 8 + 4 * (matches + 1) + total
        assert at == len(out)
        assert total == sum(len(s) for s in strings)
        assert np.array_equal(goffsets, np.concatenate([[0], np.cumsum([len(s) for s in strings])]).astype(np.uint32))
        assert chars == b"".join(strings)
        return want, strings
    return run


def counts_of(offsets, K, docs):
    return np.diff(offsets.astype(np.int64)).reshape(K, docs)


# ---- 1 - 3: what the narrow road is asked -----------------------------------------------------------------------------------------------------------
def test_the_fixture_as_one_stream(emu):
    docs, paths, cells = path_cases.fixture()
    assert len(docs) == 40 and len(paths) == 101
    for first in range(0, len(paths), 64):  # K <= 64 per call
        emu(docs, paths[first: first + 64])
    (status, offsets, tags, values), _ = emu(docs[:3], [])
    assert offsets.tolist() == [0] and tags.size == 0


def test_six_thousand_small_records(emu):
    rng = np.random.default_rng(51)
    docs = stream_cases.small_records(rng, 6000)
    (status, offsets, tags, values), strings = emu(docs, path_cases.SMALL_RECORD_PATHS)
    share = (counts_of(offsets, len(path_cases.SMALL_RECORD_PATHS), len(docs)) > 0).mean(axis=1)
    assert share[0] > 0.10 and share[1] > 0.10 and share[5] > 0.10 and share[3] > 0.50, share


def test_one_long_level(emu):
    """a root array of 20 000 mixed elements and a root object of 20 000 fields beside a tiny document: here the children are as many lanes' work"""
    n = 20000
    obj = b"{" + b",".join(b'"key%d":{"v":{"w":[%d,"s%d"]},"s":"%d"}' % (i, i, i, i) for i in range(n)) + b"}"
    arr = b"[" + b",".join([b"%d" % i, b'"s%d"' % i, b"[[%d]]" % i, b'{"k":%d.5}' % i, b"null"][i % 5] for i in range(n)) + b"]"
    (status, offsets, tags, values), _ = emu([arr, obj, b'{"key":{"v":{"w":[1]}}}'], [b"$[*]", b"$.*", b"$[*][0]", b"$.*.v.w[*]"])
    assert counts_of(offsets, 4, 3).tolist() == [[n, n, 1], [n, n, 1], [n // 5, 0, 0], [0, 2 * n, 1]] and (status == 0).all()


# ---- 4: numbers whose second word looks like a tag ------------------------------------------------------------------------------------------------------
LOOKALIKES = b'{}[]"ludtfnr'
# the edges of the annotation in tape words: a lane's share, a wave's, a workgroup's (WIDE_LANE_WORDS, 64 lanes, WIDE_SHARE in sjgpu_query.hip) and the block of the
# depth scan (FIN_BLOCK in sjgpu_finish.hip)
EDGES = (4, 256, 1024, 4096)
RUN_PAIRS = sorted({n for c in EDGES for n in (c - 1, c, c + 1, 2 * c + 1)})
LOOKALIKE_PATHS = [b"$[*]", b"$.*[*]", b"$.b.k[*]", b"$[*][*]"]


def lookalike_number(byte, as_double, i):
    """the text of a number whose second tape word has `byte` on top: an integer below 2^63, or a double, from the bit pattern"""
    bits = (byte << 56) | (0x000123456789AB + i if as_double else 5 + i)
    if as_double:
        value = struct.unpack("<d", struct.pack("<Q", bits))[0]
        assert value == value and abs(value) != float("inf")
        return repr(value).encode(), bits
    return b"%d" % struct.unpack("<q", struct.pack("<Q", bits))[0], bits


@pytest.mark.parametrize("as_double", [False, True], ids=["integers", "doubles"])
@pytest.mark.parametrize("where", ["root", "a", "b.k"])
def test_numbers_that_look_like_tags(emu, orc, where, as_double):
    """every byte that is a tag, on top of the value words of runs of C - 1, C, C + 1 and 2 C + 1 numbers for every edge C of the annotation, with nothing and
    with one plain element in front of the run (both parities cross each edge); l, u and d make the runs of number-looking top bytes that the annotation has
    to carry across shares, the others must not be taken for brackets or strings.  All of it one stream per placement, so every run also lies at some
    offset of its own against the shares."""
    docs, parsed = [], []
    for byte in LOOKALIKES:
        for pairs in RUN_PAIRS:
            for front in (0, 1):
                texts, bits = zip(*[lookalike_number(byte, as_double, i % 7) for i in range(pairs)])
                array = b"[" + b",".join((b"null",) * front + texts) + b"]"
                doc = {"root": array, "a": b'{"a":' + array + b"}", "b.k": b'{"a":1,"b":{"j":[2],"k":' + array + b'},"c":[3]}'}[where]
                err, tape, sbuf = orc.dom_parse(doc)
                assert err == 0, doc[:100]
                # the oracle's tape does carry the byte: the words behind the array's opening word (and the plain element) are (tag, bits) pairs
                words = tape.tolist()
                first = next(i for i, w in enumerate(words) if (w >> 56) == ord("[") and (where != "b.k" or i > 11)) + 1 + front
                got = words[first: first + 2 * pairs]
                assert [w >> 56 for w in got[0::2]] == [ord("d" if as_double else "l")] * pairs and got[1::2] == list(bits) and all((b >> 56) == byte for b in bits), doc[:100]
                docs.append(doc)
                parsed.append((tape, sbuf))
    (status, offsets, tags, values), _ = emu(docs, LOOKALIKE_PATHS, parsed)
    counts = counts_of(offsets, len(LOOKALIKE_PATHS), len(docs))
    lengths = np.array([pairs + front for _ in LOOKALIKES for pairs in RUN_PAIRS for front in (0, 1)])
    ones = np.ones(len(docs), np.int64)
    want = {"root": [lengths, 0 * ones, 0 * ones, 0 * ones],         # (an array's `.*` are its elements, scalars here; `.b` of an array is no index)
            "a": [ones, lengths, 0 * ones, lengths],                 # (an object's `[*]` are its values)
            "b.k": [3 * ones, 3 * ones, lengths, 3 * ones]}[where]   # (`$.*[*]`: j and k of b, the 3 of c)
    assert counts.tolist() == [w.tolist() for w in want] and (status == 0).all()


# ---- 5: keys and values ----------------------------------------------------------------------------------------------------------------------------------
def test_an_objects_children_are_keys_and_values_in_turn(emu):
    n = 5000
    flat = b"{" + b",".join(b'"k%d":"v%d"' % (i, i) for i in range(n)) + b"}"
    (status, offsets, tags, values), strings = emu([flat, b'{"o":' + flat + b',"p":{"k":"v"}}'], [b"$.*", b"$.*.*"])
    assert counts_of(offsets, 2, 2).tolist() == [[n, 2], [0, n + 1]]
    assert strings[:n] == [b"v%d" % i for i in range(n)] and strings[n + 2:] == [b"v%d" % i for i in range(n)] + [b"v"]
    # empty containers among the children, and arrays with and without elements side by side
    mixed = [b'{"a":{},"b":[],"c":{"d":{}},"e":[[]],"f":"s","g":{"h":1,"i":[]}}', b'[[],[1],[],[2,3],{},[[]],[],{"a":[]}]', b"[]", b"{}", b"[[],[]]", b"[[1,2,3]]"]
    (status, offsets, tags, values), _ = emu(mixed, [b"$.*", b"$[*][*]", b"$.*.*", b"$[*]"])
    assert counts_of(offsets, 4, 6).tolist() == [[6, 8, 0, 0, 2, 1], [4, 5, 0, 0, 0, 3], [4, 5, 0, 0, 0, 3], [6, 8, 0, 0, 2, 1]]


def test_the_limits_of_the_level_program(exe, orc, emu):
    """what sjgpu_at_paths_wide_device refuses with SJGPU_E_BADARG is what compile_path_program refuses: the driver ends with 1 and says so, as the narrow one"""
    doc = b"[" * 8 + b"[1,2],[3]" + b"]" * 8
    err, tape, sbuf = orc.dom_parse(doc)
    assert err == 0
    tape, sbuf, table = query_cases.lay_out([(tape, sbuf)])

    def refused(paths):
        lens = np.array([len(p) for p in paths], np.uint32)
        blob = (struct.pack("<IQQ", 1, len(tape), len(sbuf)) + tape.tobytes() + sbuf.tobytes() + table.tobytes() + struct.pack("<I", len(paths)) + lens.tobytes() + b"".join(paths))
        p = subprocess.run([exe], input=blob, capture_output=True, timeout=300)
        assert p.returncode in (0, 1), p.stderr
        assert (p.returncode == 1) == (b"beyond the limits" in p.stderr)
        return p.returncode == 1
    assert refused([b"$[*]"] * 65) and not refused([b"$[*]"] * 64)
    assert refused([b"$." + b"a" * 1023]) and not refused([b"$." + b"a" * 1022])                # 1 025 bytes, 1 024
    assert refused([b"$" + b"[*]" * 9]) and not refused([b"$" + b"[*]" * 8])                    # 9 wildcards, 8
    assert refused([b"$" + b"[*]" * 9 + b".a"]) and not refused([b"$" + b"[*]" * 8 + b".a.b"])  # ... with a tail behind them
    assert refused([b"$" + b".a" * 32 + b"[*]"]) and not refused([b"$" + b".a" * 31 + b"[*]"])  # 33 levels, 32
    assert refused([b"$" + b".a" * 33]) and not refused([b"$" + b".a" * 32])                    # 33 pointer tokens, 32
    assert refused([b"$" + b".a/b" * 16 + b".c[*]"]) and not refused([b"$" + b".a/b" * 16 + b"[*]"])  # 33 tokens over 17 levels, 32 over 16
    # eight wildcard levels deep: the paths at the limit against the model
    (status, offsets, tags, values), _ = emu([doc, b"[[[[[[[[[[7]]]]]]]]]]"], [b"$" + b"[*]" * 8, b"$" + b"[*]" * 8 + b"[0]", b"$" + b"[*]" * 7 + b"[0][*]", b"$" + b"[*]" * 8 + b"[0][0]"])
    assert np.diff(offsets.astype(np.int64)).tolist() == [2, 1, 2, 1, 0, 0, 0, 1]
